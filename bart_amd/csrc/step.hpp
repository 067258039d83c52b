// Input/output converters of the per-step callable (reference
// code/BARTfunc.py:309-399), batched over walkers on the device.
#pragma once
#include "engine.hpp"
#include "retrieval.hpp"

namespace bartrt {

enum { PT_LINE = 0, PT_ISO = 1, PT_MADHU_NOINV = 2, PT_MADHU_INV = 3, PT_ADIABATIC = 4, PT_PIETTE = 5 };

struct StepArgs {
  int pttype = PT_LINE, nPT = 5;
  double ptargs[5] = {0, 0, 0, 0, 0};  // R_star[m], T_star[K], T_int[K], sma[m], g[cm s-2]
  int tint_thorngren = 0;
  double tmin = 400, tmax = 3000;
  int nmolfit = 0, nfilters = 0, solution = 0;
  int nrad = 0, ncloud = 0, nray = 0;   // radius / cloud-top / scattering parameters after the T(p) ones
  double rprs = 0;
  int ebalance = 0;
  double e_in = 0, e_fac = 0;  // reject when trapz(spec) * e_fac > e_in
  int iH2 = -1, iHe = -1;
  int nwin = 0;                // total filter samples
  int grad = 0;                // smoothing radius (0 = none)
  double ptop = 0, pbot = 0;
  int pnode[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  DevBuf<double> d_gw;
  // device
  // abund[L][S] base abundances, ratio[L] H2/He of the base abundances, pbar[L]
  // pressure in bar (atm order), in one block (step_profiles stages it as it lies)
  DevBuf<double> d_consts;
  int imol[16] = {0};                // [nmolfit] species index of each fitted molecule
  unsigned long long metal_mask = 0; // bit s: species s is a metal
  DevBuf<int> d_idx0, d_npts, d_woff;  // [F]
  // [nwin] per window sample: filter weight (x rprs^2 / stellar flux for eclipse)
  DevBuf<double> d_gwt;
  // workspaces
  int cap = 0;
  DevBuf<double> d_prof, d_spec;
  DevBuf<double> d_over;                // [cap][3] per-walker overrides for prep (unfused path)
  // carry-over of the reference's worker (BARTfunc.py:318-324): a T(p) model that raises
  // ValueError leaves the chain's previous temperature profile in place.  Off: such a
  // walker is rejected.  On: walker w of a call is chain w; its last generated profile
  // is kept here ([cap][L], zeros before the first one, like the reference's array)
  int carry = 0;
  DevBuf<double> d_prevT;
  DevBuf<int> d_status;
};

void step_setup(Engine &e, const double *ptargs5, int tint_thorngren, int pttype,
                double tmin, double tmax, const double *abund, int nmolfit,
                const int *imol, int nfilters, const int *idx0, const int *npts,
                const double *nifilter, const double *istarfl, double rprs, int solution);
void step_set_ebalance(Engine &e, int on, double e_in, double e_fac);
void step_set_extras(Engine &e, int nrad, int ncloud, int nray);
void step_set_carry(Engine &e, int on);
void step_ensure(Engine &e, int n);
// params[n][npars] -> prof[n][(S+1)][L], status[n]
void step_profiles_dev(Engine &e, const double *d_params, int n, int npars, double *d_prof,
                       int *d_status, hipStream_t st);
// The same converter for the contribution-function front end (contrib.hip): params[n][npars] -> prof[n][(S+1)][L],
// status[n] (0, 1 temperature, 2 abundance) and over[n][3], each walker's reference radius (cm), cloud-top pressure
// (barye) and Rayleigh value as prep_profiles takes them (PrepArgs::over; NaN in a slot step_set_extras did not
// declare).  Samples are independent: the carry-over of step_set_carry is not applied.  Touches no engine state (no
// workspace of the step, no override request for the next preparation launch).
void step_convert_dev(Engine &e, const double *d_params, int n, int npars, double *d_prof, int *d_status,
                      double *d_over, hipStream_t st);
int step_npars(const Engine &e);   // nPT + declared extras + nmolfit (step_setup done)
// full-grid spectra [n][Wfull] -> bandflux[n][F]; may flip status to 3 (energy)
// status_out (optional, device-accessible): final status per walker
void step_bandflux_dev(Engine &e, const double *d_spec_full, int n, int *d_status,
                       double *d_bandflux, hipStream_t st, int *status_out = nullptr);
// the ranks' blocks as an all-gather leaves them (nranks slots of n * step_block_max doubles, slot r = [n][W_r]) ->
// bandflux[n][F]: the same terms in the same order as step_bandflux_dev on the reassembled spectra
size_t step_block_max(int Wfull, int nranks);
void step_bandflux_blocks_dev(Engine &e, const double *d_blocks, int nranks, int n, int *d_status,
                              double *d_bandflux, hipStream_t st, int *status_out = nullptr);
// with a communicator attached (e.comm), the RT block, one all-gather and the block integration; without one the
// engine must hold the whole grid
// sel_walkers > n: the walker count the RT kernel variant is chosen for instead of n (RunRequest::sel_walkers), so that
// a caller that cuts one set of rows into launches of any size gets the same bits from each
void step_run_dev(Engine &e, const double *d_params, int n, int npars, double *d_bandflux,
                  int *d_status, double *d_spec, hipStream_t st, int *status_out = nullptr, int sel_walkers = 0);
void step_run_host(Engine &e, const double *params, int n, int npars, double *bandflux,
                   int *status);
// diagnostics (bartrt_expint_e2): the T(p) kernels' exponential integral E_2 on n host values; needs no engine
void step_expint_e2_probe(const double *x, double *out, long n);
// diagnostics (bartrt_rt_math): the function a BARTRT_RT_MATH_* selector names, of those kernels.hpp defines, on n host
// values; needs no engine.  false: not one of them (nothing is launched)
bool step_rt_math_probe(int which, const double *x, double *out, long n);
// A retrieval problem as a caller states it: retrieval.hpp's Objective on host memory, nothing checked and nfree not
// counted yet.  The entry points below do that (retrieval_host.hpp: check_retrieval; std::invalid_argument).
using RetrievalProblem = Objective;
// DEMC / snooker over all chains, one step_run_host per iteration (mcmc.hip); takes no priors and no shared parameters
void mcmc_run(Engine &e, const RetrievalProblem &p, int nchains, long nsteps, const double *params, int snooker,
              unsigned long long seed, double *chain, double *chisq, long *naccept, long *nbad);
// The same sampler resident on the GPU (mcmc.hip; arithmetic in mcmc_core.hpp): per iteration one mcmc_advance
// launch and one step_run_dev, enqueued without a host wait, in blocks of `block` iterations, two blocks in flight.
struct McmcOpts {
  int snooker = 0;
  unsigned long long seed = 0;
  long thin = 1, block = 256;
  void (*progress)(long iterations, long naccept, void *user) = nullptr;   // per finished block
  void *progress_user = nullptr;
  // convergence tests between blocks (gr_core.hpp), exit and resume: include/bartrt.h has the rules
  long burnin = 0, grcheck = 0;
  double grthreshold = 0.0;
  int grexit = 0;
  double *grstat = nullptr;   // [ngr][npars]
  long *grwhen = nullptr;     // [ngr]
  int ngr = 0;
  int *ngr_out = nullptr;
  long first = 0;
  const double *start = nullptr;   // [nchains][npars]
  long *done = nullptr;
  int walk = 0;   // 0: demc / snooker as `snooker` says; mcmc::kWalkMrw: Metropolis random walk
  // effective-sample-size tests where the convergence tests run (ess_core.hpp); the single call alone takes them
  double esstarget = 0.0;   // 0: no ESS work at all
  int essexit = 0;
  long maxlag = 0;
  double *essstat = nullptr;   // [ngr][npars]
  double *esstau = nullptr;    // [ngr][nchains][npars]
};
// chain[nchains][nkept][npars], chisq[nchains][nkept], models[nchains][nkept][ndata] (may be null),
// nkept = ceil(nsteps / thin); with grexit only the rows of the iterations done are written
void mcmc_run_resident(Engine &e, const RetrievalProblem &p, int nchains, long nsteps, const double *params,
                       const McmcOpts &opts, double *chain, double *chisq, double *models, long *naccept, long *nbad);
// Several independent retrievals of one shape in that loop (mcmc_core.hpp: GROUPS): per iteration one
// mcmc_advance_groups launch, workgroup g advancing group g, and one step_run_dev over the ngroups nchains rows.  A
// group is its problem, its configured point, its seed and, in a resumed call, its start [nchains][npars]; opts.seed
// and opts.start go unread.  chain [ngroups][nchains][nkept][npars], chisq, models likewise; naccept [ngroups],
// nbad [ngroups][4], converged_at [ngroups] (the index of the first test that found the group converged, -1: none)
// may be null; opts.grstat is [ngr][ngroups][npars], and grexit stops at the first test that finds every group converged.
struct McmcGroup {
  RetrievalProblem p;
  const double *params;
  unsigned long long seed;
  const double *start;
};
void mcmc_run_resident_groups(Engine &e, int ngroups, const McmcGroup *groups, int nchains, long nsteps,
                              const McmcOpts &opts, double *chain, double *chisq, double *models, long *naccept,
                              long *nbad, int *converged_at);
// diagnostics (bartrt_mcmc_gr): gr_core.hpp's statistic of a host chain[nchains][nkept][npars], rows [r0, r1),
// evaluated on the device by the loop's own kernels: psrf[npars], triples[nchains][npars][3], *converged; needs no engine
void mcmc_gr_probe(const double *chain, int nchains, long nkept, int npars, const double *stepsize, long r0, long r1,
                   double threshold, double *psrf, double *triples, int *converged);
// diagnostics (bartrt_mcmc_ess): ess_core.hpp's statistic of a host chain, rows [r0, r1), evaluated on the device by
// the loop's own kernels: tau[nchains][npars], ess[npars], truncated[nchains][npars], acf (may be null)
// [nchains][npars][K + 1], *reached; needs no engine
void mcmc_ess_probe(const double *chain, int nchains, long nkept, int npars, const double *stepsize, long r0, long r1,
                    long maxlag, double target, double *tau, double *ess, int *truncated, double *acf, int *reached);
// diagnostics (bartrt_mcmc_draws): the core's draws of chains 0 .. nchains - 1 at iteration t, evaluated on the
// device: out[nchains][9 + npars] (mcmc_core.hpp, draws_row); needs no engine
void mcmc_draws_probe(unsigned long long seed, unsigned long long t, int nchains, int npars, double *out);
// Model grids (MC3's `walk = unif`; grid.hip, samples in grid_core.hpp): per iteration nrows parameter vectors drawn
// uniformly in the box, one step_run_dev on them and their model rows packed into a chunk slot, enqueued without a
// host wait; chunks of `chunk` iterations copied to pinned memory and handed to `sink`, two chunks in flight.
struct GridOpts {
  unsigned long long seed = 0;
  long chunk = 0, first = 0;   // iterations per chunk (0: the whole run); the global iteration of this call's first
  int spectra = 0, f32 = 0;    // whole spectra [Wfull] instead of band fluxes [nfilters]; rows as float
  // chunk k: global iterations t0 .. t0 + niter - 1; params [niter][nrows][npars], status [niter][nrows], rows
  // [niter][nrows][width] (double or float); non-zero: stop
  int (*sink)(long k, long t0, long niter, const double *params, const int *status, const void *rows,
              void *user) = nullptr;
  void *user = nullptr;
};
// 0, or what the sink returned when it stopped the run; nbad[4] (may be null): rows rejected with status 1, 2, 3
int grid_run(Engine &e, int nrows, int npars, long nsteps, const double *params, const double *pmin,
             const double *pmax, const double *stepsize, const GridOpts &opts, long *nbad);
// diagnostics (bartrt_grid_draws): the samples of iteration t, rows 0 .. nrows - 1, evaluated on the device:
// out[nrows][npars]; needs no engine
void grid_draws_probe(unsigned long long seed, unsigned long long t, int nrows, int npars, const double *params,
                      const double *pmin, const double *pmax, const double *stepsize, double *out);
// Batched multi-start Levenberg-Marquardt fit in the box (fit.hip; arithmetic in fit_core.hpp): per iteration the
// S * nfree forward-difference rows and the S * nrungs trial rows in one step_run_dev each, one fit_advance launch
// (one wave per start) after either, no host wait but every `check` iterations.
struct FitOpts {
  long maxiter = 50, check = 4;
  int nrungs = 4;
  double fdstep = 1e-2, ftol = 1e-10, xtol = 1e-10, lambda0 = 1e-3;
  double *trace = nullptr;   // [nstarts][maxiter + 1][npars + 4]: x, chisq, lambda, chosen rung, status after each pick
};
// starts, best [nstarts][npars]; chisq, status (fit_core.hpp: Status), niter [nstarts]; nbad[4] (status, niter and
// nbad may be null)
void fit_run(Engine &e, const RetrievalProblem &p, int nstarts, const double *starts, const FitOpts &opts,
             double *best, double *chisq, int *status, long *niter, long *nbad);
// diagnostics (bartrt_fit_probe): the solve phase of fit_advance once, on the device, for nstarts starts at x
// [nstarts][npars] with damping lambda [nstarts] and scaling D [nstarts][npars] (updated in place), from the band
// fluxes cur [nstarts][ndata] at x and pband [nstarts][nfree][ndata], pstatus [nstarts][nfree] of the forward-difference
// rows: trial [nstarts][nrungs][npars] and valid [nstarts] (bit k: rung k).  Needs no engine
void fit_probe(const RetrievalProblem &p, int nstarts, const FitOpts &opts, const double *x, const double *lambda,
               double *D, const double *cur, const double *pband, const int *pstatus, double *trial, int *valid);

}  // namespace bartrt
