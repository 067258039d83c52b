// What every retrieval entry point refuses about a stated problem before any engine is looked at, and what the grouped
// sampler call refuses about its groups.  Host code without a HIP include: retrieval_host.hpp adds the checks that need
// an engine, and a host compiler alone builds this file for the CPU tests (tests/mcmc_groups_host.cpp).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "mcmc_core.hpp"

namespace bartrt {

// The problem with nfree counted, or std::invalid_argument with `who` in front.
inline Objective check_problem(const std::string &who, Objective p) {
  if ((p.prior || p.priorlow || p.priorup) && !(p.prior && p.priorlow && p.priorup))
    throw std::invalid_argument(who + ": prior, priorlow and priorup come together");
  if (const int bad = check_stepsize(p.npars, p.stepsize, &p.nfree))
    throw std::invalid_argument(who + ": stepsize[" + std::to_string(bad - 1) + "] = " +
                                std::to_string(p.stepsize[bad - 1]) + " shares parameter " + std::to_string(bad - 1) +
                                " with a parameter that is out of range or itself shared");
  return p;
}

// The groups of one grouped sampler call (mcmc_core.hpp: GROUPS): its limits, then `check` (who, problem) -> Objective
// on every group's problem with the group named in front ("who: group 2: stepsize[6] = -7 ...").
template <class Check>
inline std::vector<Objective> check_groups(const std::string &who, int ngroups, int nch, const Objective *problems,
                                           Check &&check) {
  if (ngroups < 1) throw std::invalid_argument(who + ": ngroups = " + std::to_string(ngroups) + ": at least one group");
  if (!mcmc::groups_fit(ngroups, nch))
    throw std::invalid_argument(who + ": " + std::to_string(ngroups) + " groups of " + std::to_string(nch) +
                                " chains: one to 1024 chains per group and at most 1024 chains in all groups together");
  std::vector<Objective> out;
  for (int g = 0; g < ngroups; g++) out.push_back(check(who + ": group " + std::to_string(g), problems[g]));
  return out;
}

}  // namespace bartrt
