"""A restatement in numpy of the batched Levenberg-Marquardt fit of bart_amd/csrc/fit_core.hpp, decision for decision,
for the tests that hold the host program (tests/fit_core_host.cpp) and the device kernel (csrc/fit.hip: fit_advance)
against it one iteration at a time.

The linear systems are solved with numpy.linalg.solve on the unfrozen set, not with a copy of the core's Cholesky.  A
and g are summed row after row in the core's order with separate multiplies and adds, so they carry the core's
roundings and the comparison of the trial points is a comparison of the solves:

    |trial_j - want_j| <= 16 nfree 2^-52 cond2(Ms) |y|_2 / sqrt(M_jj) + 2^-52 |x_j|

where M = A + lambda_k diag(D) on the unfrozen set, Ms its Jacobi scaling M_ij / sqrt(M_ii M_jj), y_j = delta_j
sqrt(M_jj) the step in the scaled variables (|delta| measured where the bound of a Cholesky solve holds), and the
last term the rounding of x_j + delta_j."""
import math

import numpy as np

RUNNING, CONVERGED, STALLED, ITER_LIMIT, NO_START = range(5)
EPS = 2.0 ** -52


class Problem:
    def __init__(self, pmin, pmax, stepsize, data, uncert, prior=None, priorlow=None, priorup=None, nrungs=4,
                 fdstep=1e-2, ftol=1e-10, xtol=1e-10, lambda0=1e-3, maxiter=50):
        f = lambda v: None if v is None else np.array(v, float)
        self.pmin, self.pmax, self.stepsize, self.data, self.uncert = f(pmin), f(pmax), f(stepsize), f(data), f(uncert)
        self.prior, self.priorlow, self.priorup = f(prior), f(priorlow), f(priorup)
        self.K, self.fdstep, self.ftol, self.xtol, self.lambda0, self.maxiter = nrungs, fdstep, ftol, xtol, lambda0, maxiter
        self.npars, self.ndata = len(self.stepsize), len(self.data)
        self.free = [j for j in range(self.npars) if self.stepsize[j] > 0]
        self.nfree = len(self.free)

    # ---- parameters and residuals
    def shared(self, p):
        p = np.array(p, float)
        for j in range(self.npars):
            if self.stepsize[j] < 0:
                p[j] = p[int(-self.stepsize[j]) - 1]
        return p

    def prior_rows(self):
        if self.prior is None:
            return []
        return [j for j in range(self.npars) if self.priorlow[j] != 0.0 or self.priorup[j] != 0.0]

    def residuals(self, band, point):
        r = list((np.asarray(band, float) - self.data) / self.uncert)
        for j in self.prior_rows():
            d = point[j] - self.prior[j]
            w = self.priorlow[j] if d < 0.0 else self.priorup[j]
            r.append(d / w if w != 0.0 else 0.0)
        return np.array(r)

    def chisq(self, band, point):
        c = 0.0
        for r in self.residuals(band, point):
            c += r * r
        return c

    def h(self, x):
        out = []
        for j in self.free:
            h = self.fdstep * self.stepsize[j]
            out.append(-h if (x[j] + h > self.pmax[j] or x[j] + h < self.pmin[j]) else h)
        return np.array(out)

    def jacobian_rows(self, x):
        rows, h = [], self.h(x)
        for q, j in enumerate(self.free):
            row = np.array(x, float)
            row[j] = x[j] + h[q]
            rows.append(self.shared(row))
        return np.array(rows)

    # ---- the solve phase
    def solve(self, x, lam, D, cur, pband, pstatus):
        """-> dict(trial [K][npars], valid (bit mask), D, nbad [4], frozen [nfree], cond [K], tol [K][npars])."""
        x, D, n = np.array(x, float), np.array(D, float), self.nfree
        h, rows = self.h(x), self.jacobian_rows(x)
        rej = [int(s) != 0 for s in pstatus]
        nbad = [0, 0, 0, 0]
        for s in pstatus:
            if 1 <= int(s) <= 3:
                nbad[int(s)] += 1
        r0 = self.residuals(cur, x)
        cols = []
        for q in range(n):
            cols.append(np.zeros(len(r0)) if rej[q] else (self.residuals(pband[q], rows[q]) - r0) / h[q])
        J = np.array(cols).T if n else np.zeros((len(r0), 0))
        A, g = np.zeros((n, n)), np.zeros(n)
        for f in range(len(r0)):                       # the core's order: row after row
            A = A + np.outer(J[f], J[f])
            g = g + J[f] * r0[f]
        frozen = []
        for q, j in enumerate(self.free):
            if not rej[q]:
                D[j] = max(D[j], A[q, q])
            outward = (x[j] <= self.pmin[j] and g[q] > 0.0) or (x[j] >= self.pmax[j] and g[q] < 0.0)
            frozen.append(rej[q] or outward)
        U = [q for q in range(n) if not frozen[q]]
        trial, valid, conds, tols = [], 0, [], []
        for k in range(self.K):
            lam_k = lam * 10.0 ** (k - 1)
            row, tol, cond = x.copy(), np.zeros(self.npars), 1.0
            ok = True
            if U:
                M = A[np.ix_(U, U)] + lam_k * np.diag([D[self.free[q]] for q in U])
                dg = np.diag(M)
                ok = bool(np.all(np.isfinite(M)) and np.all(dg > 0.0))
                if ok:
                    sc = np.sqrt(dg)
                    Ms = M / np.outer(sc, sc)
                    ev = np.linalg.eigvalsh(Ms)
                    ok = bool(ev[0] > 0.0)
                if ok:
                    cond = float(ev[-1] / ev[0])
                    delta = np.linalg.solve(Ms, -g[U] / sc) / sc
                    ok = bool(np.all(np.isfinite(delta)))
                if ok:
                    ynorm = float(np.linalg.norm(delta * sc))
                    for q, d, s in zip(U, delta, sc):
                        j = self.free[q]
                        row[j] = min(max(x[j] + d, self.pmin[j]), self.pmax[j])
                        tol[j] = 16 * n * EPS * cond * ynorm / s + EPS * abs(x[j])
            if ok:
                valid |= 1 << k
                row = self.shared(row)
                for j in range(self.npars):            # a copy carries its source's margin
                    if self.stepsize[j] < 0:
                        tol[j] = tol[int(-self.stepsize[j]) - 1]
            else:
                row, tol = x.copy(), np.zeros(self.npars)
            trial.append(row)
            conds.append(cond)
            tols.append(tol)
        return dict(trial=np.array(trial), valid=valid, D=D, nbad=nbad, frozen=frozen, cond=conds, tol=np.array(tols))

    # ---- the pick phase
    def pick0(self, x, band, status):
        """The start's own model -> state dict(x, chisq, lam, status, cur, rung)."""
        x = self.shared(x)
        if int(status) != 0:
            st = dict(x=x, chisq=math.inf, lam=self.lambda0, status=NO_START, cur=None, rung=-1)
        else:
            c = self.chisq(band, x)
            st = dict(x=x, chisq=c, lam=self.lambda0,
                      status=NO_START if not math.isfinite(c) else CONVERGED if c == 0.0 else RUNNING,
                      cur=np.array(band, float), rung=-1)
        if st["status"] == RUNNING and self.maxiter <= 0:
            st["status"] = ITER_LIMIT
        return st

    def pick(self, st, it, trial, valid, tband, tstatus):
        """One decision on the K trial rows -> (new state, nbad [4], margin): margin is the smallest relative distance
        of a comparison the decision rests on from equality (a caller skips decisions that rest on a rounding)."""
        x, c, lam = st["x"], st["chisq"], st["lam"]
        nbad, best, cbest, cs = [0, 0, 0, 0], -1, math.inf, []
        for k in range(self.K):
            if not (valid >> k) & 1:
                continue
            s = int(tstatus[k])
            if 1 <= s <= 3:
                nbad[s] += 1
            if s != 0:
                continue
            ck = self.chisq(tband[k], trial[k])
            cs.append(ck)
            if ck < cbest:
                best, cbest = k, ck
        new = dict(st)
        new["rung"] = -1
        rel = lambda a, b: abs(a - b) / max(abs(a), abs(b), 1e-300)
        margin = min([rel(a, c) for a in cs] + [rel(a, b) for i, a in enumerate(cs) for b in cs[:i]] + [1.0])
        if best >= 0 and cbest < c:
            xn = np.array(trial[best], float)
            conv = c - cbest <= self.ftol * c
            moved = any(abs(xn[j] - x[j]) > self.xtol * (abs(x[j]) + self.stepsize[j]) for j in self.free)
            new.update(x=xn, chisq=cbest, cur=np.array(tband[best], float), rung=best,
                       lam=max(lam * 10.0 ** (best - 1) / 10.0, 1e-12))
            if conv or not moved or cbest == 0.0:
                new["status"] = CONVERGED
        else:
            for _ in range(self.K):
                lam *= 10.0
            new["lam"] = lam
            if lam > 1e12:
                new["status"] = STALLED
        if new["status"] == RUNNING and it >= self.maxiter:
            new["status"] = ITER_LIMIT
        return new, nbad, margin

    # ---- the whole loop for one start, on a model(rows [n][npars]) -> (band [n][ndata], status [n])
    def run(self, model, start):
        band, status = model(np.array([self.shared(start)]))
        st = self.pick0(start, band[0], status[0])
        D, nbad, it = np.zeros(self.npars), [0, 0, 0, 0], 0
        if st["status"] == NO_START and 1 <= int(status[0]) <= 3:
            nbad[int(status[0])] += 1
        trace = [dict(st)]
        while st["status"] == RUNNING:
            it += 1
            pband, pstatus = model(self.jacobian_rows(st["x"]))
            sol = self.solve(st["x"], st["lam"], D, st["cur"], pband, pstatus)
            D = sol["D"]
            tband, tstatus = model(sol["trial"])
            st, nb, _ = self.pick(st, it, sol["trial"], sol["valid"], tband, tstatus)
            nbad = [a + b + c for a, b, c in zip(nbad, sol["nbad"], nb)]
            trace.append(dict(st))
        return dict(x=st["x"], chisq=st["chisq"], status=st["status"], niter=it, nbad=nbad, trace=trace)
