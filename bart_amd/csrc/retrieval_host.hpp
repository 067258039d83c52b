// Host side of a retrieval problem, shared by the resident sampler (mcmc.hip) and the fit (fit.hip): what both refuse,
// the problem's constants in device memory, and the sum of the per-chain / per-start counters.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/bartrt.h"
#include "comm.hpp"
#include "engine.hpp"
#include "retrieval_check.hpp"
#include "step.hpp"

namespace bartrt {

// The problem with nfree counted, or the refusal every retrieval entry point makes, `who` in front.  Without an engine
// (e null: fit_probe) the checks that need none.
inline Objective check_retrieval(const std::string &who, const Engine *e, RetrievalProblem p) {
  p = check_problem(who, p);   // (retrieval_check.hpp: priors and stepsizes)
  if (!e) return p;
  if (p.ndata < 1 || p.ndata != e->step->nfilters)
    throw std::invalid_argument(who + ": data length must equal the number of filters");
  if (e->lbl && e->comm)
    throw CommError{BARTRT_ENOTSUP, who + ": line-by-line engines do not take the communicator's path"};
  if (!e->comm && (e->lo != 0 || e->hi != e->Wfull))
    throw IoError{who + ": the engine is sharded and has no communicator (engine.comm_init); use run()"};
  return p;
}

// The constants of a checked problem in one device buffer, pmin pmax stepsize [prior priorlow priorup] data uncert,
// and the problem with its pointers into it.
struct DeviceObjective {
  DevBuf<double> consts;
  Objective d;

  explicit DeviceObjective(const Objective &h) : d(h) {
    const double **fields[8] = {&d.pmin, &d.pmax, &d.stepsize, &d.prior, &d.priorlow, &d.priorup, &d.data, &d.uncert};
    auto length = [&](int k) { return (size_t)(k < 6 ? h.npars : h.ndata); };
    std::vector<double> c;
    for (int k = 0; k < 8; k++)   // (the priors only where there are any)
      if (*fields[k]) c.insert(c.end(), *fields[k], *fields[k] + length(k));
    consts.upload(c);
    const double *at = consts;
    for (int k = 0; k < 8; k++)
      if (*fields[k]) { *fields[k] = at; at += length(k); }
  }
};

// counts[n][4] in device memory, summed over n onto what total[4] holds
inline void add_counters(const long *d_counts, size_t n, long total[4]) {
  std::vector<long> counts(4 * n);
  HIPCHK(hipMemcpy(counts.data(), d_counts, sizeof(long) * 4 * n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < 4 * n; i++) total[i % 4] += counts[i];
}

}  // namespace bartrt
