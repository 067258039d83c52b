"""MC3's other two walks restated in plain Python floats, for tests/test_walks_core_cpu.py and tests/test_gpu_walks.py,
written from the descriptions at the heads of bart_amd/csrc/mcmc_core.hpp and grid_core.hpp: the Metropolis random
walk as a move of tests/mcmc_restate.py's Problem (everything but the move is that class's), and the samples of a
model grid.  The generator is mcmc_restate's own Philox."""
import mcmc_restate as mr


class MrwProblem(mr.Problem):
    """mr.Problem with the proposal of `walk = mrw`: prop_j = x_j + stepsize_j n_j for every free parameter, n_j the
    jitter normal of parameter j at iteration t; no partner, no rule on t, logjac 0."""

    def __init__(self, params, pmin, pmax, stepsize, data, uncert, nch, seed, prior=None, priorlow=None, priorup=None):
        super().__init__(params, pmin, pmax, stepsize, data, uncert, nch, False, seed, prior, priorlow, priorup)

    def propose(self, t, x):
        x = [[float(v) for v in row] for row in x]
        props, inside, logjac = [], [], []
        for i in range(self.nch):
            xi, p = x[i], list(x[i])
            for j in self.free:
                n = mr.normals(self.seed, t, i, mr.SLOT_JITTER + j // 2)[j & 1]
                p[j] = xi[j] + self.stepsize[j] * n
            ins = all(self.pmin[j] <= p[j] <= self.pmax[j] for j in self.free)
            for j, k in self.shared:
                p[j] = p[k]
            props.append(p)
            inside.append(ins)
            logjac.append(0.0)
        return props, inside, logjac


def grid_sample(seed, t, i, params, pmin, pmax, stepsize):
    """Row i of iteration t of a model grid: free parameter j at pmin_j + u_j (pmax_j - pmin_j), held to the box; u_j
    the uniform of slot 3 + j // 2 (the first for even j, the second for odd j); fixed ones keep params_j, shared ones
    follow."""
    out = [float(v) for v in params]
    for j, s in enumerate(stepsize):
        if s > 0:
            u = mr.uniforms(seed, t, i, mr.SLOT_JITTER + j // 2)[j & 1]
            lo, hi = float(pmin[j]), float(pmax[j])
            w = u * (hi - lo)
            out[j] = min(max(lo + w, lo), hi)
    for j, s in enumerate(stepsize):
        if s < 0:
            out[j] = out[int(-s) - 1]
    return out


def grid_samples(seed, t, nrows, params, pmin, pmax, stepsize):
    return [grid_sample(seed, t, i, params, pmin, pmax, stepsize) for i in range(nrows)]
