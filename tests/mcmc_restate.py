"""The resident sampler (bart_amd/csrc/mcmc_core.hpp) restated in numpy and plain Python floats, for
tests/test_mcmc_core_cpu.py and tests/test_gpu_mcmc_resident.py: its own Philox4x32-10, the draw table, the moves,
shared parameters, priors and the acceptance rule, written from the header's description.  Scalar arithmetic in the
header's order, so results differ from the C++ only by libm's log / sin / cos against Python's."""
import math

import numpy as np

M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
SLOT_PARTNERS, SLOT_SNOOKER, SLOT_ACCEPT, SLOT_JITTER = 0, 1, 2, 3
START_T = 0xFFFFFFFFFFFFFF00
START_ROUNDS = 20


def philox(ctr, key):
    """Philox4x32-10 on Python integers: ctr four words, key two words -> four words."""
    c, (k0, k1) = list(ctr), key
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def uniform53(hi, lo):
    h = ((hi << 32) | lo) >> 11
    u = (float(h) + 0.5) * 2.0 ** -53
    return u if u < 1.0 else 1.0 - 2.0 ** -53


def uniforms(seed, t, chain, slot):
    w = philox([t & MASK, (t >> 32) & MASK, chain, slot], (seed & MASK, (seed >> 32) & MASK))
    return uniform53(w[0], w[1]), uniform53(w[2], w[3])


def normals(seed, t, chain, slot):
    u0, u1 = uniforms(seed, t, chain, slot)
    r, a = math.sqrt(-2.0 * math.log(u0)), 6.283185307179586 * u1
    return r * math.cos(a), r * math.sin(a)


def other(u, nch, i, a=-1, b=-1):
    """Uniform over the chains other than i, a, b (negative: unused)."""
    ex = sorted(v for v in (i, a, b) if v >= 0)
    k = len(ex)
    draw = min(int(u * (nch - k)), nch - k - 1)
    for v in ex:
        draw += draw >= v
    return draw


def draws_row(seed, t, nch, i, npars):
    u_r1, u_r2 = uniforms(seed, t, i, SLOT_PARTNERS)
    u_z, u_g = uniforms(seed, t, i, SLOT_SNOOKER)
    u_a, _ = uniforms(seed, t, i, SLOT_ACCEPT)
    r1 = other(u_r1, nch, i) if nch > 1 else i
    r2 = other(u_r2, nch, i, r1) if nch > 2 else r1
    z = other(u_z, nch, i, r1, r2) if nch > 3 else -1
    nor = []
    for j in range(0, npars, 2):
        nor += list(normals(seed, t, i, SLOT_JITTER + j // 2))
    return [u_r1, u_r2, u_z, u_g, u_a, math.log(u_a), r1, r2, z] + nor[:npars]


class Problem:
    def __init__(self, params, pmin, pmax, stepsize, data, uncert, nch, snooker, seed, prior=None, priorlow=None,
                 priorup=None):
        f = lambda v: [float(x) for x in v]
        self.params, self.pmin, self.pmax, self.stepsize = f(params), f(pmin), f(pmax), f(stepsize)
        self.data, self.uncert = f(data), f(uncert)
        self.nch, self.snooker, self.seed = nch, bool(snooker), seed
        self.npars = len(self.params)
        self.prior = None if prior is None else (f(prior), f(priorlow), f(priorup))
        self.free = [j for j, s in enumerate(self.stepsize) if s > 0]
        self.shared = [(j, int(-s) - 1) for j, s in enumerate(self.stepsize) if s < 0]
        self.nfree = len(self.free)

    def chisq(self, band, p):
        c = 0.0
        for b, d, u in zip(band, self.data, self.uncert):
            r = (float(b) - d) / u
            c += r * r
        pr = 0.0
        if self.prior is not None:
            for j in range(self.npars):
                if self.prior[1][j] == 0.0:
                    continue
                d = float(p[j]) - self.prior[0][j]
                r = d / (self.prior[1][j] if d < 0.0 else self.prior[2][j])
                pr += r * r
        return c + pr

    def start_point(self, rnd, i):
        width = (1.0 if i > 0 else 0.0) if rnd == 0 else 0.1
        x = list(self.params)
        for j in self.free:
            n = normals(self.seed, START_T + rnd, i, SLOT_JITTER + j // 2)[j & 1] if width != 0.0 else 0.0
            x[j] = self.params[j] + width * self.stepsize[j] * n
            x[j] = min(max(x[j], self.pmin[j]), self.pmax[j])
        for j, k in self.shared:
            x[j] = x[k]
        return x

    def propose(self, t, x):
        """x [nch][npars] -> (proposals [nch][npars], inside [nch], logjac [nch]); the rows the model is given are
        the proposals where inside, the current points elsewhere."""
        nch, seed = self.nch, self.seed
        x = [[float(v) for v in row] for row in x]
        props, inside, logjac = [], [], []
        for i in range(nch):
            xi, p = x[i], list(x[i])
            u0, u1 = uniforms(seed, t, i, SLOT_PARTNERS)
            r1 = other(u0, nch, i) if nch > 1 else i
            r2 = other(u1, nch, i, r1) if nch > 2 else r1
            x1, x2 = x[r1], x[r2]
            lj = 0.0
            if self.snooker and nch > 3 and t % 10 != 0:
                uz, ug = uniforms(seed, t, i, SLOT_SNOOKER)
                xz = x[other(uz, nch, i, r1, r2)]
                nd = 0.0
                for j in self.free:
                    nd += (xi[j] - xz[j]) * (xi[j] - xz[j])
                nd = math.sqrt(nd)
                if nd == 0.0:
                    nd = 1.0
                proj = 0.0
                for j in self.free:
                    proj += (x1[j] - x2[j]) * (xi[j] - xz[j]) / nd
                g = 1.2 + ug
                ndn = 0.0
                for j in self.free:
                    p[j] = xi[j] + g * proj * (xi[j] - xz[j]) / nd
                    ndn += (p[j] - xz[j]) * (p[j] - xz[j])
                lj = (self.nfree - 1) * (math.log(max(math.sqrt(ndn), 1e-300)) - math.log(nd))
            else:
                gam = 1.0 if t % 10 == 0 else 2.38 / math.sqrt(2.0 * max(self.nfree, 1))
                for j in self.free:
                    n = normals(seed, t, i, SLOT_JITTER + j // 2)[j & 1]
                    p[j] = xi[j] + gam * (x1[j] - x2[j]) + 1e-3 * self.stepsize[j] * n
            ins = all(self.pmin[j] <= p[j] <= self.pmax[j] for j in self.free)
            for j, k in self.shared:
                p[j] = p[k]
            props.append(p)
            inside.append(ins)
            logjac.append(lj)
        return props, inside, logjac

    def log_u(self, t, i):
        return math.log(uniforms(self.seed, t, i, SLOT_ACCEPT)[0])

    def start(self, model):
        """The start of a run -> (x [nch][npars], cur [nch][ndata], c [nch], statuses of every model call made), or
        None when no chain starts on a physical model."""
        nch, seen = self.nch, []

        def evaluate(x):
            band, status = model(x)
            seen.extend(int(v) for v in status)
            return ([list(b) for b in band],
                    [self.chisq(band[i], x[i]) if status[i] == 0 else math.inf for i in range(nch)])
        x = [self.start_point(0, i) for i in range(nch)]
        cur, c = evaluate(x)
        for rnd in range(1, START_ROUNDS + 1):
            bad = [i for i in range(nch) if not math.isfinite(c[i])]
            if not bad:
                break
            for i in bad:
                x[i] = self.start_point(rnd, i)
            cur, c = evaluate(x)
        if not any(math.isfinite(v) for v in c):
            return None
        return x, cur, c, seen

    def loop(self, model, nsteps, thin=1):
        """The whole run; model(rows [n][npars]) -> (band [n][ndata], status [n]).  Returns chain [nch][nkept][npars],
        chisq, models, accepted [nsteps][nch], counts [nch][4] -- or None when no chain starts on a physical model."""
        nch, inf = self.nch, math.inf
        st = self.start(model)
        if st is None:
            return None
        x, cur, c, _ = st
        chain, chis, models, accepted = [], [], [], []
        counts = [[0, 0, 0, 0] for _ in range(nch)]
        for t in range(nsteps):
            props, inside, logjac = self.propose(t, x)
            band, status = model([props[i] if inside[i] else x[i] for i in range(nch)])
            acc = []
            for i in range(nch):
                cp = inf
                if inside[i]:
                    if 1 <= status[i] <= 3:
                        counts[i][status[i]] += 1
                    if status[i] == 0:
                        cp = self.chisq(band[i], props[i])
                a = math.isfinite(cp) and self.log_u(t, i) < -0.5 * (cp - c[i]) + logjac[i]
                if a:
                    x[i], c[i], cur[i] = props[i], cp, list(band[i])
                    counts[i][0] += 1
                acc.append(a)
            accepted.append(acc)
            if (t + 1) % thin == 0 or t == nsteps - 1:
                chain.append([list(r) for r in x])
                chis.append(list(c))
                models.append([list(r) for r in cur])
        return (np.array(chain).transpose(1, 0, 2), np.array(chis).T, np.array(models).transpose(1, 0, 2),
                np.array(accepted), np.array(counts))
