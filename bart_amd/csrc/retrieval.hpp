// A retrieval problem, stated once for the sampler (mcmc_core.hpp) and the fit (fit_core.hpp): the box, the stepsizes,
// the data and the optional Gaussian priors.  Plain C++ on plain pointers, no HIP include: the kernels read it on the
// device, host code on the host, and a host compiler alone builds it for the CPU tests.
//
// PARAMETERS.  stepsize[j] > 0: free.  stepsize[j] == 0: fixed at its configured value.  stepsize[j] = -k (MC3's
// convention, k counted from 1): shared, a copy of parameter k - 1 wherever a point is made or moved (copy_shared);
// the target must be in range and not itself shared (check_stepsize).  nfree counts the free ones; the box
// [pmin, pmax] applies to them alone.
//
// PRIORS.  prior, priorlow and priorup come together or not at all.  The two cores read them by two rules, each kept
// as it is (DESIGN.md names this an open question):
//   mcmc::prior_term (MC3's)         parameter j has a prior where priorlow[j] != 0; above prior[j] the difference is
//                                    divided by priorup[j] whatever its value.
//   fit::has_prior / fit::prior_res  parameter j has a prior where priorlow[j] != 0 or priorup[j] != 0; a side whose
//                                    width is zero does not constrain (its residual is 0).
// They disagree exactly where one of priorlow[j], priorup[j] is zero and the other is not.  priorlow[j] == 0,
// priorup[j] != 0: the sampler sees no prior, the fit a one-sided one above prior[j].  priorlow[j] != 0,
// priorup[j] == 0: below prior[j] they agree; above it the fit adds nothing and the sampler divides by zero (chisq
// inf, or NaN at p_j == prior[j]: the proposal is refused).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#define RETRIEVAL_HD __host__ __device__ inline
// the same roundings on the host and on the device: no multiply-add contraction in the cores' functions
#if defined(__clang__)
#define RETRIEVAL_EXACT _Pragma("clang fp contract(off)")
#else
#define RETRIEVAL_EXACT
#endif

namespace bartrt {

constexpr int kMaxPars = 64;

// Every pointer is memory of the side that calls (device memory in a kernel, host memory in host code).
struct Objective {
  int npars, ndata, nfree;
  const double *pmin, *pmax, *stepsize;      // [npars]
  const double *data, *uncert;               // [ndata]
  const double *prior, *priorlow, *priorup;  // [npars], or all null: uniform priors
};

// 0, or 1 + the index of the first parameter whose shared target is out of range or itself shared; *nfree counted
RETRIEVAL_HD int check_stepsize(int npars, const double *stepsize, int *nfree) {
  int n = 0;
  for (int j = 0; j < npars; j++) {
    const double s = stepsize[j];
    if (s > 0) n++;
    if (s < 0) {
      const double k = -s;
      if (!(k >= 1.0 && k <= (double)npars) || k != (double)(int)k || stepsize[(int)k - 1] < 0) return j + 1;
    }
  }
  if (nfree) *nfree = n;
  return 0;
}

RETRIEVAL_HD void copy_shared(int npars, const double *stepsize, double *p) {
  for (int j = 0; j < npars; j++)
    if (stepsize[j] < 0) p[j] = p[(int)(-stepsize[j]) - 1];
}

}  // namespace bartrt
