// The samples of a model grid (MC3's `walk = unif`), stated once for host and device: parameters drawn uniformly in
// the box, no data, no chi-square, no acceptance, no population.  Plain inline functions on plain pointers in the
// idiom of mcmc_core.hpp, whose generator and draw table they use: the kernel (grid.hip: grid_draw) runs them one row
// per lane, and a host compiler alone builds them for the CPU tests (tests/walks_core_host.cpp).
//
// SAMPLE (t, i): iteration t, row i.  For every free parameter j (stepsize[j] > 0)
//     p_j = pmin_j + u_j (pmax_j - pmin_j),
// u_j from uniforms(seed, t, i, kSlotJitter + j / 2): u0 for even j, u1 for odd j -- the slots whose normals jitter
// parameter j in the sampler, read here as the uniforms they are made from.  The product and the sum are rounded one
// after the other (no multiply-add), and the result is held to [pmin_j, pmax_j]: the rounded sum can pass pmax_j by a
// unit in the last place.  A fixed parameter keeps params[j]; a shared one follows through copy_shared.  A sample
// depends on (seed, t, i) and the box alone -- not on the number of rows, the chunking or what was made before -- so
// any part of a grid can be restated, or made again, anywhere.
#pragma once
#include "mcmc_core.hpp"

namespace bartrt {
namespace grid {

// 0, or 1 + the index of the first free parameter whose box is empty or not a number
MCMC_HD int check_box(int npars, const double *pmin, const double *pmax, const double *stepsize) {
  for (int j = 0; j < npars; j++)
    if (stepsize[j] > 0 && !(pmin[j] <= pmax[j])) return j + 1;
  return 0;
}

// row i of iteration t into out[npars]
MCMC_HD void sample(unsigned long long seed, unsigned long long t, int i, int npars, const double *params,
                    const double *pmin, const double *pmax, const double *stepsize, double *out) {
  MCMC_EXACT
  for (int j = 0; j < npars; j += 2) {
    const bool f0 = stepsize[j] > 0, f1 = j + 1 < npars && stepsize[j + 1] > 0;
    double u0 = 0.0, u1 = 0.0;
    if (f0 || f1) mcmc::uniforms(seed, t, i, mcmc::kSlotJitter + j / 2, u0, u1);
    out[j] = params[j];
    if (f0) {
      const double w = u0 * (pmax[j] - pmin[j]);
      out[j] = fmin(fmax(pmin[j] + w, pmin[j]), pmax[j]);
    }
    if (j + 1 < npars) {
      out[j + 1] = params[j + 1];
      if (f1) {
        const double w = u1 * (pmax[j + 1] - pmin[j + 1]);
        out[j + 1] = fmin(fmax(pmin[j + 1] + w, pmin[j + 1]), pmax[j + 1]);
      }
    }
  }
  copy_shared(npars, stepsize, out);
}

}  // namespace grid
}  // namespace bartrt
