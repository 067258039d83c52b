/*
 * bartrt.h -- C ABI of libbartrt.so, the MI355X-native forward
 * radiative-transfer engine that replaces BART's `transit_module`.
 *
 * Every entry point below stands in for one call BART's per-step callable
 * makes on the SWIG module (reference code/BARTfunc.py, line cited per
 * function).  Plain pointers and sizes only; host pointers unless the name
 * ends in `_dev`.  All functions return 0 on success and a negative code on
 * error (message via bartrt_last_error()) unless documented otherwise.  The
 * library computes ONLY on the GPU: with no HIP device every compute entry
 * point fails with BARTRT_ENODEV -- there is no CPU fallback.
 *
 * Engine state is a process-global SINGLETON, like the reference module's
 * (created by transit_init, destroyed by free_memory; BARTfunc.py:230,406):
 *   - one engine, on one device, per process.  bartrt_init on a live engine REPLACES it
 *     (the old one is destroyed first); a host that drives several GPUs runs one process per GPU (that is
 *     how bench.py, bart_amd.retrieve and the MC3-driven worker shard a node), each with
 *     "--device <n>" or LOCAL_RANK;
 *   - calls are NOT re-entrant and not thread-safe: drive the engine from one host thread
 *     at a time (the reference runs one engine per MPI process).  The launch state of the
 *     kernels (variant switches read from the environment, the timing and walked-layer
 *     records, the prefetch request) belongs to that one engine;
 *   - the `_dev` entry points are asynchronous on the stream they are given; the others
 *     return when their result is in the caller's buffer;
 *   - the environment variables (BARTRT_INTEG, BARTRT_KERNEL, BARTRT_LBL, ...) are read
 *     once per process or per bartrt_init, not per call.
 */
#ifndef BARTRT_H
#define BARTRT_H

#ifdef __cplusplus
extern "C" {
#endif

#define BARTRT_OK        0
#define BARTRT_EINVAL   -1   /* bad argument / not initialised */
#define BARTRT_EIO      -2   /* input file missing or malformed */
#define BARTRT_ENODEV   -3   /* no HIP device / HIP runtime error */
#define BARTRT_ENOTSUP  -4   /* configuration not supported by this build */

/* ---- the eight reference entry points -------------------------------- */

/* trm.transit_init(argc, argv)  [BARTfunc.py:229-230]
 * argv = {"transit", "-c", <transit cfg>}.  Extra flags accepted after the
 * cfg: "--shard <rank> <nranks>" keeps only that contiguous block of the
 * wavenumber grid on this process's GPU; "--device <n>"; "--no-service"
 * (see bartrt_get_share). */
int bartrt_init(int argc, const char **argv);

/* trm.get_no_samples()  [BARTfunc.py:233].  Full-grid sample count (>=0),
 * or a negative error code. */
int bartrt_get_no_samples(void);

/* trm.get_waveno_arr(n)  [BARTfunc.py:234].  out[n] = wavenumbers, cm-1. */
int bartrt_get_waveno_arr(double *out, int n);

/* trm.set_radius(r)  [BARTfunc.py:351].  Reference radius in km. */
int bartrt_set_radius(double refradius_km);

/* trm.set_cloudtop(p)  [BARTfunc.py:354].  log10(cloud-top pressure / bar). */
int bartrt_set_cloudtop(double log10_pbar);

/* trm.set_scattering(flag, value)  [BARTfunc.py:358,360]. */
int bartrt_set_scattering(int flag, double value);

/* trm.run_transit(profiles.flatten(), nwave)  [BARTfunc.py:363].
 * prof[nprof] with nprof = (nspecies+1)*nlayers: row 0 temperature (K), rows
 * 1..S mole mixing ratios in atm-file species order, layers in atm-file order
 * (BARTfunc.py:213-222).  spec[nwave] = emergent flux, erg s-1 cm-2 cm.
 * On a sharded engine nwave may be the full count (only the shard's block is
 * written) or the shard's count. */
int bartrt_run_transit(const double *prof, int nprof, double *spec, int nwave);

/* trm.free_memory()  [BARTfunc.py:406]. */
int bartrt_free_memory(void);

/* Integration rule of the eclipse geometry (no counterpart in the reference's
 * module: its engine, whose source would settle the rule, is an empty submodule --
 * DESIGN.md conventions C6 / C8).
 *   1 (DEFAULT) = the Simpson / trapezoid hybrid SURVEY.md App. A-4 recalls for the
 *       reference's engine: the optical depth over radius and B exp(-tau/mu) over tau
 *       (zero-padded past `last`) -- the only statement about the engine's integrator
 *       the project holds;
 *   0 = trapezoid in the transmittance (exact for isothermal columns);
 *   2 = plain trapezoid in tau of B exp(-tau/mu).
 * Also the cfg key `integ` (number or transmittance / simpson / trapz_tau) and the
 * environment variable BARTRT_INTEG, read by bartrt_init; every eclipse kernel is built
 * for each rule.  bartrt_get_integ writes the rule in force to *rule and returns a status
 * like every other entry point (rule 0 and BARTRT_OK would otherwise share a value); the
 * `transit` executable and the worker log the rule they ran under. */
int bartrt_set_integ(int rule);
int bartrt_get_integ(int *rule);

/* Which optical depth `toomuch` is compared with (no counterpart in the reference's
 * module).  1 (default since round 4) = each ray's SLANT depth tau / mu: SURVEY.md App. A-4 read
 * literally ("slant path ds = dr / cos(theta) ... stops where tau > toomuch") and the reading the
 * engine's call structure is recalled to have -- the optical depth is computed per ray angle, the
 * cut inside that loop; every angle ends on its own layer and rule 1 pads one unit of slant depth.
 * 0 = the vertical depth: the column ends on one layer for every ray angle.  Both run specialised
 * kernels (rules 0, 1 and 2; the slant cut costs 1.10-1.18x per launch, MEASUREMENTS_ARCHIVE.md); under rule 0
 * the two differ by about exp(-toomuch) of the flux, under rule 1 (the default) by far more -- the padded
 * point moves with the cut: 4.6e-3 relative on a 40-layer synthetic column at toomuch 10 (and spline
 * against linear CIA 3.5e-3: the round-4 change of defaults moved spectra at the 0.5 % level).  Also
 * the cfg key `cut vertical|slant` and BARTRT_CUT. */
int bartrt_set_cut(int slant);
int bartrt_get_cut(int *slant);
/* The optimistic loop of rule 1's single-wave `cut slant` kernel (csrc/rt_eclipse_s1s.hpp): whole six-layer blocks
 * are walked without ray flags and event log while every lane's optical depth stands at or below guard * (the
 * smallest ray threshold) at the block's start; a wave that finds a ray dead at such a block's end walks its column
 * again with the flags.  Spectra are the same bits for every guard.  guard: 0 = off, or a power of two 2^-10 .. 1
 * (default 2^-4); anything else is refused.  Process-wide, applies to the launches that follow; needs no engine.
 * BARTRT_SLANT_OPT=n sets it at start-up: 0 = off, n = 1 .. 10 = 2^-n (bartrt_parse_slant_opt is that reading); any
 * other text is refused: bartrt_init and bartrt_get_slant_opt fail with BARTRT_EINVAL until the setter is called. */
int bartrt_set_slant_opt(double guard);
int bartrt_get_slant_opt(double *guard);
int bartrt_parse_slant_opt(const char *text, double *guard);

/* Sharded engines ("--shard r n"): which column count picks the kernel variant.  1 (DEFAULT) = this
 * block's own: a block of a few hundred samples takes the layer-parallel kernels instead of the
 * single-wave kernel's latency floor (the WASP-12b grid on eight GPUs, 303 samples x 10 walkers per
 * rank: 16 us against 52 us per launch); spectra agree with the unsharded run's to rounding (4e-16
 * measured), not bit for bit -- north_star asks for 1e-6.  0 = the WHOLE grid's: every block is computed
 * by the kernel the unsharded run would use, so the blocks concatenate to its spectrum bit for bit.
 * Also cfg `kernel_by local|whole` and BARTRT_KERNEL_BY.  No effect on an unsharded engine. */
int bartrt_set_kernel_by(int local);
int bartrt_get_kernel_by(int *local);

/* How the engine interpolates the cross-section (CIA) files, fixed at bartrt_init by the cfg key
 * `cia_interp linear|spline` / BARTRT_CIA_INTERP: *spline = 1 (default since round 4)
 * natural cubic splines in wavenumber and temperature, 0 linear in both.  Read-only: the tables are
 * resampled at init.  A natural spline may undershoot zero between two samples of a steep table: the
 * values are used as the spline gives them, NOT clamped (engine and oracle alike) -- a clamp would be
 * one more unverified convention. */
int bartrt_get_cia_interp(int *spline);

/* `shareOpacity` (a key of the reference's transit cfg: code/makecfg.py:106-107, BART.py:259-262 --
 * BART's worker processes, one per chain, keep ONE copy of the opacity grid).  With the key in the
 * cfg (or BARTRT_SHARE_OPACITY=1) the worker processes of a run share one grid in one of two ways,
 * chosen by BARTRT_SHARE_MODE:
 *   service (default)  THE CHAIN SERVICE.  The first process to initialise on a (cfg, GPU, wavenumber
 *       block) builds the engine and starts a dispatcher thread; every worker process -- that one's
 *       own caller included -- is a client: bartrt_run_transit copies the profile into the process's
 *       slot of a POSIX shared-memory segment and sleeps on a futex, the dispatcher launches ONE batch
 *       for all the profiles posted together (MC3 releases its workers together: code/BARTfunc.py:312,
 *       399) and wakes the callers.  A client makes no HIP call at all: one context, one grid, one
 *       launch per MCMC step.  The setters (set_radius / set_cloudtop / set_scattering) of a client
 *       act on ITS profiles only, per walker of the batch.  Served to clients: the reference module's
 *       eight calls, bartrt_run_transit_batch and the plain getters; the other entry points return
 *       BARTRT_ENOTSUP.  A client whose owner has gone gets BARTRT_ENODEV; the owner's
 *       bartrt_free_memory keeps serving until the other workers have let go (BARTRT_SHARE_WAIT_S
 *       seconds at most, default 60).  Tunables: BARTRT_SVC_WINDOW_US (30: how long the dispatcher
 *       waits for the workers of the previous batch after the latest arrival), BARTRT_SVC_SPIN_US
 *       (200: a waiting client polls this long before it sleeps), BARTRT_SVC_MAXCLIENTS (256 slots,
 *       1024 at most: one per worker process = per chain).  Which profiles share a launch depends on
 *       the processes' pace; the RESULT does not: the kernel variant is chosen for the number of
 *       registered workers (BARTRT_SVC_KERNEL_WALKERS pins it) and every kernel computes a walker
 *       independently of the others in its launch, so a chain's spectra are the same bits every run.
 *       Runs of fewer than five chains (BARTRT_NCHAINS, else the MPI world size of the spawned
 *       workers) take the `ipc` reading unless BARTRT_SHARE_MODE says otherwise: it is the faster
 *       one there.
 *   ipc  every process runs its own engine; the first uploads the grid, the others map that HBM
 *       allocation through a HIP IPC handle published in a POSIX shared-memory segment
 *       (HSA_ENABLE_IPC_MODE_LEGACY=0 must be in the environment where the host driver supports
 *       dmabuf IPC only).  What "--no-service" in bartrt_init's argv (a caller that needs the whole
 *       API in its own process: bart_amd.engine) turns `service` into.
 *   off  the key is ignored.
 * BARTRT_SERVICE=1 asks for the service without the key.
 * bartrt_get_share: *shared = 1 if this process's grid is shared in either way, *owner = 1 if this
 * process holds the allocation (ipc) / the engine (service). */
int bartrt_get_share(int *shared, int *owner);
/* *mode = 0 engine of its own, 1 chain-service client, 2 client that also owns the service;
 * *owner_pid, this process's *slot, *nclients registered.  Any pointer may be NULL. */
int bartrt_get_service(int *mode, int *owner_pid, int *slot, int *nclients);
/* Chain service only: dispatcher rounds so far, profiles served by them, rounds that held every
 * registered client (nprofiles / nlaunches = the mean batch). */
int bartrt_get_service_stats(unsigned long long *nlaunches, unsigned long long *nprofiles,
                             unsigned long long *nfull);
/* ... and the rounds whose slots were not consecutive (a worker in the middle of the slot
 * range missed the round): served by one launch all the same, through a gather / scatter pair. */
int bartrt_get_service_gathered(unsigned long long *ngathered);

/* Prefetched preparation.  Names the profile batch of the bartrt_run_transit_batch_dev call
 * AFTER the next one: the next call's RT launch prepares that batch's layer records
 * (hydrostatic radii, densities, interpolation weights) in extra workgroups of its own grid,
 * and the call that follows -- if it is made with exactly this buffer and walker count --
 * starts on its RT kernel directly (one launch and ~8 us of dependent latency less per
 * batch).  THE CALLER'S PROMISE: the named buffer is complete, and stays unchanged, from the
 * next call on.  True of batches resident in HBM (a grid or population of models evaluated
 * chunk by chunk; bench.py); not of an MCMC step whose proposal depends on the previous
 * step's spectra -- do not prefetch there.  Without a matching call the records are simply
 * dropped.  Table path of the eclipse geometry; other engines ignore the request.  Results
 * are bit-identical with and without.  nwalkers = 0 withdraws a request. */
int bartrt_prefetch_profiles_dev(const double *d_prof_next, int nwalkers);

/* ---- batched / device-resident variants (same arithmetic) ------------- */

/* nwalkers profiles -> nwalkers spectra; ok[w] = 0 marks a profile the
 * engine cannot evaluate (non-finite or non-positive temperature).  With
 * ok == NULL (and through bartrt_run_transit) such a profile is an error
 * (BARTRT_EINVAL) instead.  spec is [nwalkers][nwave_local]. */
int bartrt_run_transit_batch(const double *prof, int nwalkers, int nprof,
                             double *spec, int nwave, unsigned char *ok);

/* Same with HBM-resident buffers, asynchronous on `stream` (a hipStream_t;
 * NULL = the engine's own non-blocking stream, which nothing else is ordered with: a
 * caller that works on the device's default stream passes hipStreamLegacy, (hipStream_t)1,
 * as bart_amd/engine.py does for torch's default stream).  d_spec is [nwalkers][local samples]. */
int bartrt_run_transit_batch_dev(const double *d_prof, int nwalkers,
                                 double *d_spec, unsigned char *d_ok,
                                 void *stream);

/* ---- per-step callable on the device (BARTfunc.py:309-399) ------------- */

/* One-time setup of the input/output converters around the engine:
 * PT model "line" (code/PT.py:589-701) with PTargs = {R_star[m], T_star[K],
 * T_int[K], sma[m], g[cm s-2]} (BARTfunc.py:204-208), the base abundances
 * abund[L][S] (atm order), indices of the fitted molecules, and the
 * per-filter windows/weights produced by wine.resample
 * (code/wine.py:127-174): for filter f, idx0[f] = first spectrum index,
 * npts[f] = number of samples, weights/starflux concatenated in that order.
 * pttype: 0 "line", 1 "iso".  tint_thorngren: T_int from Thorngren et al.
 * 2019 (PT.py:680-685) instead of ptargs5[2].
 * rprs = Rp/Rs.  solution: 0 eclipse (divide by stellar flux, times rprs^2),
 * 1 transit / 2 direct (no star division) (BARTfunc.py:386-396). */
int bartrt_step_setup(const double *ptargs5, int tint_thorngren, int pttype,
                      double tmin, double tmax,
                      const double *abund, int nmolfit, const int *imol,
                      int nfilters, const int *idx0, const int *npts,
                      const double *nifilter, const double *istarfl,
                      double rprs, int solution);

/* Energy-balance rejection (BARTfunc.py:366-383): reject a walker when
 * trapz(spectrum, wn) * e_fac > e_in  (e_fac = 4 (Rp*100)^2). */
int bartrt_step_set_ebalance(int on, double e_in, double e_fac);

/* Declares the per-walker parameters BARTfunc places between the T(p) parameters
 * and the abundance factors (BARTfunc.py:350-360), each 0 or 1, in this order:
 * planet radius at the reference pressure (km; what trm.set_radius takes), log10
 * of the cloud-top pressure (bar; trm.set_cloudtop), Rayleigh scattering value
 * (trm.set_scattering(1, value); present but unused with the polarisability
 * flavour, flag 2, which is set once with bartrt_set_scattering).  They then act
 * per walker inside the batch instead of through the engine-wide setters. */
int bartrt_step_set_extras(int nrad, int ncloud, int nray);

/* The reference's worker keeps going when its T(p) model raises ValueError: the
 * profile array still holds the previous step's temperatures and is range-checked
 * and used as it is (BARTfunc.py:318-330, marked FINDME there).  on = 1 reproduces
 * that: walker w of every call is chain w, and a parameter set the model rejects
 * is evaluated with chain w's last generated profile (zeros before the first one,
 * i.e. rejected by the temperature bounds).  on = 0 (default): such a walker is
 * rejected with status 1. */
int bartrt_step_set_carry(int on);

/* params[nwalkers][npars] (npars = nPT + extras + nmolfit; nPT = 5 for "line", 1 for
 * "iso") -> bandflux[nwalkers][nfilters]; rejected walkers get -1 in every
 * band (BARTfunc.py:327-330,339-344,378-383).  status[w]: 0 ok, 1 bad
 * temperature, 2 bad abundance, 3 energy balance.  status may be NULL. */
int bartrt_step_batch(const double *params, int nwalkers, int npars,
                      double *bandflux, int *status);
/* The retrieval's driver loop, native: differential-evolution MCMC (snooker = 0,
 * the reference's `walk = demc`) or its snooker variant (snooker = 1) over
 * nchains chains, all of them evaluated by one batched model call per
 * iteration, nsteps iterations.  Arguments are the keys of the reference's
 * [MCMC] section (examples/demo/BART_eclipse.cfg:43-102): params (start),
 * pmin, pmax, stepsize (0 = fixed) of length npars = nPT + nmolfit as in
 * bartrt_step_batch; data, uncert of length ndata = nfilters.  Proposals
 * outside [pmin, pmax] and models rejected by the worker are refused.
 * chain[nchains][nsteps][npars], chisq[nchains][nsteps]; naccept (accepted
 * proposals) and nbad[4] (models rejected with status 1, 2, 3 in nbad[1..3]) may
 * be NULL. */
int bartrt_mcmc_run(int nchains, int npars, long nsteps, const double *params, const double *pmin,
                    const double *pmax, const double *stepsize, int ndata, const double *data,
                    const double *uncert, int snooker, unsigned long long seed, double *chain,
                    double *chisq, long *naccept, long *nbad);
/* The same sampler RESIDENT on the GPU: population, chi-squares and counters stay in device memory, and an iteration
 * is one small sampler launch (one workgroup, chain i on lane i) followed by the model's launches, enqueued without a
 * host wait -- the host works `block` iterations at a time and keeps at most two blocks in flight.  Arguments as
 * bartrt_mcmc_run, and:
 *   - the random draws come from a counter-based generator (Philox4x32-10 keyed by `seed`, counter = iteration,
 *     chain, slot; bart_amd/csrc/mcmc_core.hpp has the table), so a run can be restated draw for draw anywhere; its
 *     stream is not bartrt_mcmc_run's;
 *   - stepsize[j] = -k (MC3's convention, k counted from 1) makes parameter j a copy of parameter k - 1 in every
 *     proposal and start point; a target out of range or itself shared is BARTRT_EINVAL;
 *   - prior / priorlow / priorup ([npars], all three or none): where priorlow[j] != 0, chi-square gains
 *     ((p_j - prior_j) / sigma)^2 with sigma = priorlow[j] below prior_j and priorup[j] above.  THE chisq ARRAY HOLDS
 *     THE DATA TERM PLUS THESE TERMS;
 *   - thin = n writes every n-th iteration: rows t = n - 1, 2n - 1, ... and the last one, nkept = ceil(nsteps / n);
 *   - a proposal outside [pmin, pmax] is not sent to the model (the launch gets the chain's current point in its
 *     place, so every launch has nchains rows) and is not counted in nbad;
 *   - progress (may be NULL) is called after every finished block with the iterations done and the proposals
 *     accepted so far.
 * chain[nchains][nkept][npars], chisq[nchains][nkept]; models (may be NULL) [nchains][nkept][ndata]: the band fluxes
 * of each chain's CURRENT state at the kept iterations (what MC3's `savemodel` holds).  opts may be NULL (demc, seed
 * 0, thin 1, block 256, uniform priors); set opts->size = sizeof(bartrt_mcmc_opts) -- fields past `size` read as zero.
 * At most 1024 chains and 64 parameters (BARTRT_EINVAL beyond; larger populations stay with bartrt_mcmc_run).
 * Sharded engines: whatever the step serves.  LOCKSTEP as for bartrt_mcmc_run: with a communicator attached every
 * rank makes this call with the same arguments, the step's all-gather leaves the same band-flux bits on every rank,
 * so every rank advances the same population and writes the same chain.  The convergence tests below read that
 * chain and nothing else: every rank computes the same statistic bits, takes the same decision at the same block,
 * and has issued the same collectives when it stops.  Chain-service clients and line-by-line engines with a
 * communicator: BARTRT_ENOTSUP.
 *
 * CONVERGENCE TESTS (MC3's grtest / grexit).  grcheck = n > 0: after every n iterations of this call, and after the
 * last one, the Gelman-Rubin statistic of the rows so far is computed ON THE DEVICE from the chain where it lies
 * (bart_amd/csrc/gr_core.hpp states the formula and the fixed order of every sum), enqueued behind the block that
 * ends there.  n must be a multiple of block, and block of thin (BARTRT_EINVAL otherwise), so that every test falls
 * on a block end whose state is a kept row.  Rows of global iterations t < burnin never enter; a test needs two
 * chains and four rows, and where there are fewer none is made or recorded.  Test k is recorded in
 * grstat[k][npars] (0 for parameters that are not free) and grwhen[k] (the GLOBAL iteration count at the test) while
 * k < ngr; *ngr_out is the number of tests made.  grthreshold 0 reads as 1.01 (MC3's "within 1% of unity", as we
 * recall it).  A test finds convergence when every free parameter's statistic is finite and below the threshold.
 * grexit != 0: the call stops at the first test that finds convergence, at iteration count T of this call:
 * *done = T (otherwise nsteps), chain / chisq / models hold the ceil(T / thin) rows of each chain up to there at the
 * places they have in the full arrays -- THE ARRAYS KEEP THEIR FULL SHAPE [nchains][nkept] AND ARE NOT WRITTEN PAST
 * THOSE ROWS -- and naccept / nbad are the counts as they stood at T.  A test's record is read when the host next
 * waits for its block, so up to two further blocks have been enqueued by then; their iterations are discarded, and
 * the stopping point does not depend on timing.
 *
 * RESUME.  first = t0 > 0 with start[nchains][npars] (the last rows of the run before; both or neither, and t0 a
 * multiple of thin: BARTRT_EINVAL otherwise) makes the global iterations t0 ... t0 + nsteps - 1 with the draws of
 * those t; the start's draws are not made and params is not read.  Every rule that reads t -- the gamma = 1 move
 * every tenth iteration, the thinning rule -- uses the global value.  The chains' chi-squares and band fluxes are
 * rebuilt by one model call on the rows of start (a row the model rejects: chisq inf).  A run of N iterations, and a
 * run of N1 followed by a resumed run of N - N1, write the same bytes.  The tests of a resumed call see that call's
 * rows alone (t >= max(burnin, t0)): they know nothing of the run before.
 *
 * WALKS.  walk = 0: demc or snooker, as `snooker` says.  walk = BARTRT_WALK_MRW (2; MC3's `walk = mrw`): Metropolis
 * random walk -- every free parameter of a proposal moves by stepsize_j times the jitter normal of the draw table,
 * no partner chain is drawn, no rule of the move reads the iteration, and one chain is enough.  Box, shared
 * parameters, priors, thinning, models, the convergence tests and resume are as above.  walk = BARTRT_WALK_UNIF (3;
 * MC3's `walk = unif`) is not a chain: BARTRT_EINVAL here, bartrt_grid_run serves it.  Any other value:
 * BARTRT_EINVAL.
 *
 * EFFECTIVE SAMPLE SIZE.  esstarget > 0: at every place where a convergence test runs -- every grcheck iterations and
 * after the last one, on the rows of global iterations >= burnin, enqueued behind the block that ends there -- the
 * integrated autocorrelation time tau of every chain and free parameter and the effective sample size ess_j = sum
 * over the chains of n / tau_ij are computed ON THE DEVICE as well (bart_amd/csrc/ess_core.hpp states the lagged sums,
 * their fixed order and Geyer's initial positive sequence; maxlag lags at most, 0 reads as 1024, more than 4096 is
 * BARTRT_EINVAL).  esstarget > 0 with grcheck == 0 is BARTRT_EINVAL.  One chain is enough for these tests: with them a
 * test is made wherever four rows lie past the burn-in, and where there is one chain grstat[k] is zeros.  Test k is
 * recorded in essstat[k][npars] (0 for parameters that are not free) and esstau[k][nchains][npars] while k < ngr.
 * The target is REACHED when there is a free parameter, every free ess_j is finite and >= esstarget, and no chain's
 * sequence of a free parameter ran out at maxlag before it turned non-positive.  The call stops at the first test at
 * which every requested exit holds: grexit -- converged; essexit -- reached; both set -- both at the same test.
 * *done, the shape of the arrays, the discarded blocks and the independence from timing are as for grexit; a resumed
 * call's tests see its own rows alone; sharded engines in lockstep take the same decision, since the test reads the
 * chain alone.  esstarget == 0: no ESS work at all, and essexit, essstat and esstau must be unset.
 * bartrt_mcmc_run_resident_groups does not serve these fields: any of them set there is BARTRT_EINVAL naming them. */
enum { BARTRT_WALK_MRW = 2, BARTRT_WALK_UNIF = 3 };
typedef struct bartrt_mcmc_opts {
  unsigned long size;                 /* sizeof(bartrt_mcmc_opts) of the caller */
  int snooker;                        /* 0: demc, 1: snooker */
  unsigned long long seed;
  long thin;                          /* 0 reads as 1 */
  long block;                         /* iterations per block; 0 reads as 256 */
  const double *prior, *priorlow, *priorup;
  void (*progress)(long iterations, long naccept, void *user);
  void *progress_user;
  long burnin;                        /* rows of global iterations t < burnin enter no test */
  long grcheck;                       /* a test every grcheck iterations and after the last; 0: none */
  double grthreshold;                 /* 0 reads as 1.01 */
  int grexit;                         /* stop at the first test that finds convergence */
  double *grstat;                     /* [ngr][npars], may be NULL */
  long *grwhen;                       /* [ngr], may be NULL */
  int ngr;
  int *ngr_out;                       /* tests made, may be NULL */
  long first;                         /* resume: the global iteration this call starts at */
  const double *start;                /* resume: [nchains][npars] */
  long *done;                         /* iterations of this call the result holds, may be NULL */
  int walk;                           /* 0: as `snooker` says; 2: mrw (BARTRT_WALK_MRW) */
  double esstarget;                   /* effective samples per free parameter; 0: no ESS work at all */
  int essexit;                        /* stop at the first test that reaches esstarget */
  long maxlag;                        /* lags of the autocorrelation; 0 reads as 1024, at most 4096 */
  double *essstat;                    /* [ngr][npars], may be NULL */
  double *esstau;                     /* [ngr][nchains][npars], may be NULL */
} bartrt_mcmc_opts;
int bartrt_mcmc_run_resident(int nchains, int npars, long nsteps, const double *params, const double *pmin,
                             const double *pmax, const double *stepsize, int ndata, const double *data,
                             const double *uncert, const bartrt_mcmc_opts *opts, double *chain, double *chisq,
                             double *models /* NULL */, long *naccept, long *nbad);
/* ENSEMBLES: ngroups INDEPENDENT retrievals ("groups") of one shape -- nchains chains, npars parameters and ndata data
 * each, on the one engine -- advanced in lockstep by one resident loop.  An iteration is one sampler launch, workgroup
 * g advancing group g with chain i of the group on lane i, and ONE batched model evaluation over all ngroups x nchains
 * rows: the launches a ten-chain retrieval leaves half empty are filled by its neighbours.  Nothing else is shared.
 * Group g is bartrt_mcmc_run_resident with groups[g]'s params, pmin, pmax, stepsize (fixed and shared parameters its
 * own), data, uncert, priors (all three or none) and seed, and the opts of this call: its draws are keyed by its seed
 * and its own chain indices 0 .. nchains - 1, its partner chains are drawn among its own, and where the model's
 * launches give a row the same bits in both batches, chain / chisq / models / naccept / nbad of group g are the bytes
 * of that single call.
 *   chain[ngroups][nchains][nkept][npars], chisq[ngroups][nchains][nkept], models (may be NULL)
 *   [ngroups][nchains][nkept][ndata]; naccept[ngroups], nbad[ngroups][4], converged_at[ngroups] (each may be NULL).
 * Set size = sizeof(bartrt_mcmc_group) in EVERY group (fields past `size` read as zero).  opts as above, except that
 * opts->seed, prior, priorlow, priorup and start must be unset (BARTRT_EINVAL): they live in the groups, and that
 * esstarget, essexit, maxlag, essstat and esstau must be unset (BARTRT_EINVAL naming them): the effective-sample-size
 * tests are the single call's.  Limits:
 * ngroups >= 1, nchains >= 1 and ngroups x nchains <= 1024, 64 parameters (BARTRT_EINVAL beyond).  What the single
 * call refuses about a problem is refused here with the group named: "mcmc_run_resident_groups: group 2: stepsize[6] =
 * -7 ...".  walk = BARTRT_WALK_UNIF: BARTRT_EINVAL.
 *   CONVERGENCE TESTS run for every group on its own rows, by the single call's kernels in their fixed summation order:
 * opts->grstat is [ngr][ngroups][npars], grwhen[ngr] as above.  converged_at[g] is the index k of the first test that
 * found group g converged (its iteration count: grwhen[k]), -1 if none did.  grexit stops the call at the first test
 * at which EVERY group is found converged; a group that converged earlier keeps running until then, so its rows up
 * to any iteration are still those of a run of its own.  Stopping point, discarded blocks and *done as above.
 *   RESUME: opts->first = t0 > 0 with start[nchains][npars] in every group, or neither; the guarantee of the single
 * call holds group by group.
 * Sharded engines, LOCKSTEP, chain-service clients and line-by-line engines with a communicator: as for
 * bartrt_mcmc_run_resident. */
typedef struct bartrt_mcmc_group {
  unsigned long size;                 /* sizeof(bartrt_mcmc_group) of the caller */
  const double *params;               /* [npars] the configured point (not read in a resumed call) */
  const double *pmin, *pmax, *stepsize;
  const double *data, *uncert;        /* [ndata] */
  const double *prior, *priorlow, *priorup;   /* [npars], all three or none */
  unsigned long long seed;
  const double *start;                /* resume: [nchains][npars], with opts->first > 0 */
} bartrt_mcmc_group;
int bartrt_mcmc_run_resident_groups(int ngroups, const bartrt_mcmc_group *groups, int nchains, int npars, long nsteps,
                                    int ndata, const bartrt_mcmc_opts *opts, double *chain, double *chisq,
                                    double *models /* NULL */, long *naccept, long *nbad, int *converged_at);
/* Diagnostics: the sampler's draws of chains 0 .. nchains - 1 at iteration t, evaluated ON THE DEVICE (its log, sqrt,
 * sin and cos): out[nchains][9 + npars] = the uniforms of r1, r2, z, gamma and acceptance, log of the acceptance
 * uniform, the partners r1, r2, z (z = -1 with fewer than four chains) and the jitter normal of each parameter.
 * Needs no engine. */
int bartrt_mcmc_draws(unsigned long long seed, unsigned long long t, int nchains, int npars, double *out);
/* Diagnostics: the resident loop's convergence test once ON THE DEVICE, by its own kernels, on a host
 * chain[nchains][nkept][npars], rows [r0, r1) of every chain: psrf[npars] (0 for parameters that are not free:
 * stepsize[j] <= 0), triples[nchains][npars][3] = (n, mean, sum of squared deviations) of every chain and free
 * parameter, *converged as bartrt_mcmc_run_resident decides it (threshold 0 reads as 1.01).  Fewer than two chains
 * or four rows: no test, every output zero.  The bits are those of a host build of bart_amd/csrc/gr_core.hpp.  At
 * most 64 parameters.  Needs no engine. */
int bartrt_mcmc_gr(const double *chain, int nchains, long nkept, int npars, const double *stepsize, long r0, long r1,
                   double threshold, double *psrf, double *triples, int *converged);
/* Diagnostics: the resident loop's effective-sample-size test once ON THE DEVICE, by its own kernels, on a host
 * chain[nchains][nkept][npars], rows [r0, r1) of every chain, n = r1 - r0, K = min(maxlag, n - 1) (maxlag 0 reads as
 * 1024; more than 4096: BARTRT_EINVAL): tau[nchains][npars] the integrated autocorrelation times, ess[npars],
 * truncated[nchains][npars] (1: the sequence ran out at K), acf (may be NULL) [nchains][npars][K + 1] the lagged sums
 * S_k = sum_r (x_r - mean)(x_{r+k} - mean), *reached as bartrt_mcmc_run_resident decides it.  Zeros for parameters
 * that are not free (stepsize[j] <= 0).  Fewer than four rows: no test, every output zero.  One chain is enough.  The
 * bits are those of a host build of bart_amd/csrc/ess_core.hpp.  At most 64 parameters.  Needs no engine. */
int bartrt_mcmc_ess(const double *chain, int nchains, long nkept, int npars, const double *stepsize, long r0, long r1,
                    long maxlag, double esstarget, double *tau, double *ess, int *truncated,
                    double *acf /* NULL */, int *reached);
/* MODEL GRIDS (MC3's `walk = unif`, the reference's way to the training sets of surrogate models,
 * code/makecfg.py:177-190): nsteps iterations of nrows parameter vectors drawn uniformly in [pmin, pmax], each
 * evaluated by the batched model and handed to the caller WITH ITS WHOLE MODEL ROW.  No data, no chi-square, no
 * acceptance.  Sample (t, i) -- global iteration t = first + 0 .. first + nsteps - 1, row i -- has free parameter j
 * at pmin_j + u_j (pmax_j - pmin_j), u_j the uniform of the sampler's jitter slot of parameter j
 * (bart_amd/csrc/grid_core.hpp; mcmc_core.hpp has the table), held to the box; fixed parameters (stepsize 0) keep
 * params[j], shared ones (stepsize -k) copy parameter k - 1.  A sample depends on (seed, t, i) and the box alone:
 * `first` makes any stretch of a grid again, bit for bit.
 * An iteration is three things on the engine's stream, enqueued without a host wait: the draw, the step, and a pack
 * of the model rows into the chunk's slot -- as float with f32, and -1 IN EVERY ENTRY of a row the model rejects
 * (status 1 temperature, 2 abundance, 3 energy balance).  Every `chunk` iterations (0: the whole run in one chunk) the
 * slot is copied to pinned host memory; the host enqueues chunk k + 1, then waits for chunk k and calls
 *     sink(k, t0, niter, params[niter][nrows][npars], status[niter][nrows], rows[niter][nrows][width], user)
 * ON THE CALLING THREAD, once per chunk, k ascending, t0 the chunk's first GLOBAL iteration, width = nfilters
 * (spectra = 0) or the whole grid's sample count (spectra = 1), rows double or (f32) float.  THE BUFFERS ARE VALID
 * DURING THE CALL ONLY.  A non-zero return stops the run: the chunk in flight runs out and is not handed over, and the
 * call returns that value (bartrt_last_error names it; a sink that wants to tell its stop from the library's errors
 * returns a positive value).  nbad (may be NULL): nbad[1..3] rows rejected with status 1, 2, 3 in the chunks handed
 * over.  A chunk costs two device and two pinned host slots of chunk * nrows * (npars * 8 + 4 + width * 4 or 8)
 * bytes each; one that cannot be allocated is BARTRT_EINVAL naming the bytes.
 * BARTRT_EINVAL: nrows outside 1 .. 65535, npars outside 1 .. 64, nsteps < 1, chunk < 0, first < 0, pmin_j > pmax_j on
 * a free parameter, a bad shared parameter, no sink, spectra = 0 without filters, the carry-over of
 * bartrt_step_set_carry switched on.  Sharded engines: WITHOUT a communicator refused (BARTRT_EIO, the step's rule: no
 * rank holds a whole row).  WITH one (bartrt_comm_init) every rank makes the call in LOCKSTEP with the same arguments;
 * in `spectra` mode the step's all-gather leaves the whole spectra on every rank, so EVERY RANK'S sink receives the
 * same whole rows [width = the whole grid], bit for bit -- a caller that writes files lets one rank write.  Line-by-line
 * engines with a communicator and chain-service clients: BARTRT_ENOTSUP. */
typedef struct bartrt_grid_opts {
  unsigned long size;                 /* sizeof(bartrt_grid_opts) of the caller */
  unsigned long long seed;
  long chunk;                         /* iterations per chunk; 0: the whole run */
  long first;                         /* global iteration of this call's first one */
  int spectra;                        /* 0: band fluxes, width = nfilters; 1: whole spectra, width = nwave */
  int f32;                            /* model rows as float */
  int (*sink)(long k, long t0, long niter, const double *params /*[niter][nrows][npars]*/,
              const int *status /*[niter][nrows]*/, const void *rows /*[niter][nrows][width]*/, void *user);
  void *user;
} bartrt_grid_opts;
int bartrt_grid_run(int nrows, int npars, long nsteps, const double *params, const double *pmin,
                    const double *pmax, const double *stepsize, const bartrt_grid_opts *opts, long *nbad);
/* Diagnostics: the samples of iteration t, rows 0 .. nrows - 1, evaluated ON THE DEVICE by the grid's own kernel:
 * out[nrows][npars].  Needs no engine. */
int bartrt_grid_draws(unsigned long long seed, unsigned long long t, int nrows, int npars, const double *params,
                      const double *pmin, const double *pmax, const double *stepsize, double *out);
/* Least-squares fit before the chain (MC3's `leastsq`): nstarts independent Levenberg-Marquardt fits inside the box
 * [pmin, pmax], advanced together on the GPU.  An iteration is two batched model launches -- the nstarts * nfree
 * forward-difference rows of the Jacobians (h_j = fdstep * stepsize_j, the sign flipped at the upper bound), then the
 * nstarts * nrungs trial points of a ladder of dampings lambda 10^(k-1) -- with one small kernel after each (one wave
 * per start; bart_amd/csrc/fit_core.hpp states every decision).  The host waits only every `check` iterations.
 * starts[nstarts][npars]; pmin, pmax, stepsize (0: fixed, -k: a copy of parameter k, as bartrt_mcmc_run_resident),
 * data, uncert as bartrt_mcmc_run.  With the three prior arrays, every parameter with a non-zero priorlow or priorup
 * adds the residual (p_j - prior_j) / width, the width of its side (a zero width does not constrain that side); chisq
 * is the sum of squares of all residuals.  Results: best[nstarts][npars], chisq[nstarts], and (each may be NULL)
 * status[nstarts] (BARTRT_FIT_*), niter[nstarts] iterations made, nbad[4] models rejected with status 1, 2, 3.
 * opts may be NULL; set opts->size = sizeof(bartrt_fit_opts); a zero field reads as its default (maxiter 50: give a
 * negative maxiter for none, nrungs 4 (1 to 8), check 4, fdstep 1e-2, ftol 1e-10, xtol 1e-10, lambda0 1e-3).
 * trace (may be NULL): [nstarts][maxiter + 1][npars + 4] doubles, after the start's own model (record 0) and after
 * every iteration: x, chisq, lambda, the rung taken (-1: none), status.  Records after every start has finished
 * repeat the last.  At most 64 parameters.  Sharded engines and LOCKSTEP as for bartrt_mcmc_run_resident. */
enum { BARTRT_FIT_RUNNING = 0, BARTRT_FIT_CONVERGED = 1, BARTRT_FIT_STALLED = 2, BARTRT_FIT_MAXITER = 3,
       BARTRT_FIT_NO_START = 4 };
typedef struct bartrt_fit_opts {
  unsigned long size;                 /* sizeof(bartrt_fit_opts) of the caller */
  long maxiter;
  int nrungs;
  long check;
  double fdstep, ftol, xtol, lambda0;
  const double *prior, *priorlow, *priorup;
  double *trace;
} bartrt_fit_opts;
int bartrt_fit(int nstarts, int npars, const double *starts, const double *pmin, const double *pmax,
               const double *stepsize, int ndata, const double *data, const double *uncert,
               const bartrt_fit_opts *opts, double *best, double *chisq, int *status, long *niter, long *nbad);
/* Diagnostics: the solve phase of the fit's kernel once ON THE DEVICE, for nstarts starts at x[nstarts][npars] with
 * damping lambda[nstarts] and scaling D[nstarts][npars] (updated in place), from the band fluxes cur[nstarts][ndata]
 * at x and pband[nstarts][nfree][ndata], pstatus[nstarts][nfree] of the forward-difference rows.  Gives
 * trial[nstarts][nrungs][npars] and valid[nstarts] (bit k set: rung k factored).  Of opts it reads nrungs, fdstep and
 * the priors.  Needs no engine. */
int bartrt_fit_probe(int nstarts, int npars, const double *pmin, const double *pmax, const double *stepsize,
                     int ndata, const double *data, const double *uncert, const bartrt_fit_opts *opts,
                     const double *x, const double *lambda, double *D, const double *cur, const double *pband,
                     const int *pstatus, double *trial, int *valid);
/* Device-resident form; d_status and d_spec ([nwalkers][nwave]) may be NULL. */
int bartrt_step_batch_dev(const double *d_params, int nwalkers, int npars,
                          double *d_bandflux, int *d_status, double *d_spec,
                          void *stream);
/* The two converters on their own, for engines sharded by wavenumber block:
 * profiles -> bartrt_run_transit_batch_dev on each shard -> all-gather of the
 * spectra (caller, RCCL) -> bandflux on the reassembled [nwalkers][nwave]. */
int bartrt_step_profiles_dev(const double *d_params, int nwalkers, int npars,
                             double *d_prof, int *d_status, void *stream);
int bartrt_step_bandflux_dev(const double *d_spec_full, int nwalkers,
                             int *d_status, double *d_bandflux, void *stream);
/* The band integration on the ranks' blocks where an all-gather leaves them, for callers that run their own
 * collective (torch, MPI) and for one GPU standing in for any rank count: d_blocks holds nranks slots of
 * nwalkers * wmax doubles (wmax = the largest block), slot r = [nwalkers][W_r] packed rows of block r, which covers
 * samples [Wfull*r/nranks, Wfull*(r+1)/nranks) of the full grid (W_r = Wfull*(r+1)/nranks - Wfull*r/nranks; the
 * split of "--shard r nranks"); a slot's tail past nwalkers * W_r is not read.  Same terms in the same order as
 * bartrt_step_bandflux_dev on the reassembled [nwalkers][Wfull] spectra: the same band fluxes and statuses, bit for
 * bit.  Any engine after bartrt_step_setup, sharded or not; 1 <= nranks <= Wfull.  Asynchronous on `stream`. */
int bartrt_step_bandflux_blocks_dev(const double *d_blocks, int nranks, int nwalkers,
                                    int *d_status, double *d_bandflux, void *stream);

/* ---- the ranks' communicator: the per-step path on sharded engines ----------------------------
 * The library's own RCCL communicator over the ranks of a wavenumber-sharded run ("--shard r n", one GPU per
 * block).  RCCL is opened at run time, not linked: the copy already mapped into the process if there is one (torch
 * ships its own librccl.so; a live torch `nccl` group has it mapped), else BARTRT_RCCL_LIB, else
 * /opt/rocm/lib/librccl.so.1.  Without RCCL every bartrt_comm_* call returns BARTRT_ENOTSUP.
 *
 * Bring-up: rank 0 calls bartrt_comm_get_unique_id (no engine needed), the launcher hands the
 * BARTRT_COMM_ID_BYTES bytes to every rank (torch: bart_amd.engine.comm_init; MPI: MPI_Bcast), and
 * every rank, its engine initialised, calls bartrt_comm_init with the rank and count of its "--shard r n" (an
 * unsharded engine is 0 / 1).  A rank / count that is not the engine's block, a second init, or no engine:
 * BARTRT_EINVAL.  The communicator lives on the engine's device; bartrt_comm_free, bartrt_free_memory and a new
 * bartrt_init destroy it.  Chain-service clients get BARTRT_ENOTSUP.
 *
 * With a communicator attached, bartrt_step_batch, bartrt_step_batch_dev and bartrt_mcmc_run run on sharded engines
 * -- and on an unsharded engine with a communicator of one rank, the same code: the RT launch writes this rank's
 * block straight into its slot of a receive buffer (the layout of bartrt_step_bandflux_blocks_dev), ONE in-place
 * ncclAllGather per call on the call's stream fills the other slots (ordered on the device: no host wait), and the
 * band integration reads the slots in place.  bartrt_step_batch_dev's d_spec, when given, receives the reassembled
 * [nwalkers][Wfull] spectra through one copy kernel.  Every rank makes the same calls with the same parameters:
 * collectives must match across ranks.  Under kernel_by whole (bartrt_set_kernel_by) the band fluxes, statuses and
 * spectra are the unsharded engine's bits; under kernel_by local they agree with them to rounding and agree across
 * ranks bit for bit.
 * LOCKSTEP: bartrt_mcmc_run is host code around that step -- every rank runs the same seeded loop on band fluxes that
 * are the same bits on every rank, so the ranks draw the same proposals, issue the same collectives and write
 * identical chains; give every rank the same arguments.
 * The contribution-function calls (bartrt_cf_setup, _batch, _batch_over, _params and their _dev forms, below) follow
 * the same rule: with a communicator they run on sharded engines, one in-place ncclAllGather per chunk of walkers in
 * the same receive buffer, and every rank gets the same band rows bit for bit.
 * Line-by-line engines: the step with a communicator returns BARTRT_ENOTSUP, and so do the contribution-function
 * calls.  Without a communicator a sharded engine's step and its bartrt_cf_setup fail as before. */
#define BARTRT_COMM_ID_BYTES 128          /* = NCCL_UNIQUE_ID_BYTES */
int bartrt_comm_get_unique_id(void *id);  /* rank 0 calls it; the launcher broadcasts the bytes */
int bartrt_comm_init(const void *id, int rank, int nranks);
int bartrt_comm_free(void);
/* *rank / *nranks of the attached communicator (-1 / 0 without one); *ncollectives: collectives this engine has
 * issued (counted across bartrt_comm_free, reset by bartrt_init).  Pointers may be NULL. */
int bartrt_get_comm(int *rank, int *nranks, unsigned long long *ncollectives);

/* ---- introspection ----------------------------------------------------- */
const char *bartrt_last_error(void);
/* Twelve hex digits: a hash of the CODE the eclipse RT launch is made of (device
 * code objects and host text of the RT translation units), fixed at build time.
 * Never fails, needs no GPU.  Profiler figures under profiles/ carry the id of the
 * library they were measured on; bench.py quotes them only under the same id. */
const char *bartrt_build_id(void);
/* Which eclipse kernel the library's measured table (csrc/kernel_table.inc, written by
 * tools/tune_kernels.py) names for a launch of `columns` 64-sample columns (walkers x
 * ceil(samples / 64)) with `nmol` table molecules under the default conventions (rule 1,
 * `cut slant`, five ray angles): "single", "rows4" / "rows8" / "rows16" / "rows32" (layers per
 * step of the layer-parallel walk), "adj8" / "adj16" (rows on adjacent lanes).  Needs no GPU and
 * no engine; the returned string is static. */
const char *bartrt_kernel_choice(int nmol, long columns);
/* The per-ray thresholds of `cut slant` as the host forms them for every launch (csrc/kernels.hpp, slant_thresholds):
 * for n <= 16 rays with invmu[a] = 1 / cos(theta_a), thr[a] = the largest double t with fl(t * invmu[a]) <= toomuch
 * (so that tau > thr[a] <=> tau * invmu[a] > toomuch, to the bit) and thrb[a] = 2^600 * the next double above thr[a]
 * (+inf where that overflows: the scaled form the single-wave kernel's ray flags add to).  Either output may be NULL.
 * Needs no GPU and no engine. */
int bartrt_slant_thresholds(double toomuch, const double *invmu, int n, double *thr, double *thrb);
/* Diagnostics (tests): the ray quadrature of the initialised eclipse engine as its launches carry it, n =
 * bartrt_get_nangles() entries each, in the order of the `raygrid`: invmu = 1 / cos(theta), wgt = pi (sin^2 hi -
 * sin^2 lo), wq = wgt * invmu, and thr / thrb of bartrt_slant_thresholds for the engine's present `toomuch`.
 * order[s] = the ray in slot s of the specialised kernels' order; *sq = 1 when that order is the square-root one
 * (slot n - 1 holds a ray of exactly twice slot 0's 1 / cos: its transmittance is taken as the square of slot 0's),
 * else 0 and order is the identity.  Any output may be NULL.  Host side only: no kernel runs. */
int bartrt_get_ray_args(int n, double *invmu, double *wgt, double *wq, double *thr, double *thrb, int *order, int *sq);
/* The eclipse kernels the library holds ahead of time, one line each: the kernel's template-id in
 * namespace bartrt with every argument spelled out (the text the run-time compiler is given for a
 * shape that is NOT here), a tab, 1 / 0 -- whether a run-time build of it gets the max-ILP
 * scheduling option --, a tab, the object that holds it.  Needs no GPU and no engine.
 * BARTRT_EINVAL if `buf` is too small; bartrt_last_error() then names the size needed. */
int bartrt_kernel_inventory(char *buf, int buflen);
int bartrt_get_nlayers(void);
int bartrt_get_nspecies(void);
int bartrt_get_nprof(void);                 /* (S+1)*L */
int bartrt_get_local_range(int *lo, int *hi); /* shard's [lo,hi) of the grid */
int bartrt_get_species(char *buf, int buflen); /* space-separated names */
int bartrt_get_pressure(double *out, int n);   /* barye, atm order */
/* optical depth of the latest HOST-buffer call's profile: tau[nwave_local][L], layer
 * index 0 = top (the tau.dat convention read by code/cf.py:68-94); last[i] = the layer
 * where the column of sample i ended.  bartrt_get_tau serves a single-profile call
 * (bartrt_run_transit, the reference's shape); after a batch call it is an ERROR, not the
 * first walker's or an older call's values: name the walker with bartrt_get_tau_of (the
 * profile is re-run with the output enabled).  Device-buffer calls keep no profile. */
int bartrt_get_tau(double *tau, int *last, int nwave, int nlayers);
int bartrt_get_tau_of(int walker, double *tau, int *last, int nwave, int nlayers);

/* Outputs of the standalone run (reference: `transit -c cfg`, code/bestFit.py:421-427,
 * code/cf.py:46-64).  get_atm_profile: the (S+1)*L profile array of the atmosphere
 * file itself.  get_radius: hydrostatic radii (cm, atm order) of the last run's
 * first profile.  get_intensity: I[nangles][nwave_local] of the last
 * single-profile eclipse run (the `outintens` content). */
int bartrt_get_atm_profile(double *prof, int nprof);
int bartrt_get_radius(double *rad, int nlayers);
int bartrt_get_nangles(void);
int bartrt_get_angles(double *deg, int n);
int bartrt_get_intensity(double *intens, int nangles, int nwave);
int bartrt_get_intensity_of(int walker, double *intens, int nangles, int nwave);  /* as bartrt_get_tau_of */

/* Diagnostics (tests): what the preparation of the latest launch wrote for walker `walker` of its batch, copied
 * back from the engine's device buffers -- a host-side copy after a device synchronisation, no kernel runs.  Any
 * output may be NULL.  With M table molecules and C cross-section tables (bartrt_get_prep_shape; a file read under
 * `cia_interp spline` counts twice, its second table holds the curvature terms), layer k counted FROM THE TOP:
 *   coef[L][4 + 2 M + 2 C]   path length r[k-1] - r[k] (cm; 0 on the top layer), c2 / T, per molecule the weights
 *                            rho (1 - f) and rho f of the table's planes j and j + 1, per cross-section table its two
 *                            weights, the Rayleigh term (x wn^4), the grey-cloud extinction;
 *   idx[L][1 + C]            byte offsets: of plane j of the layer's slab in the table ((l Nt + j) M W 8, l the layer
 *                            in atm order), and of each cross-section table's pair plane (16 W bytes each);
 *   kstop                    the last layer of the column (L - 1), or a cloud deck's layer with bit 30 set;
 *   ok                       1, or 0 for a profile the engine cannot evaluate (its records are zeros, c2 / T = 1).
 * BARTRT_EINVAL: no launch yet (or its buffers have been regrown since); a walker index outside the latest batch;
 * the latest launch prepared its walkers inside the RT kernel (one to four walkers under the default conventions:
 * the records lived in LDS and were never written out -- run a larger batch, or with BARTRT_FOLD=0).  After a
 * device-buffer call the flags are read from the caller's buffer, which has to be alive still.  A batch that went
 * out in chunks leaves its last chunk.  Contribution-function calls keep records of their own and leave these alone. */
int bartrt_get_prep_shape(int *nmol, int *ncs);
int bartrt_get_prep_records(int walker, double *coef, long long *idx, int *kstop, unsigned char *ok);

/* Diagnostics (tests), transit geometry: the radii and the chord table the preparation of the latest launch wrote for
 * walker `walker` of its batch -- a host-side copy after a device synchronisation, no kernel runs.  With L layers,
 * layers and chords counted FROM THE TOP:
 *   rtop[L]        the hydrostatic radii, top to bottom (cm);
 *   ds[L][L]       ds[k][j] = s_{j-1} - s_j, s_j = sqrt(r_j^2 - r_k^2): the length inside layer j (between r_{j-1} and
 *                  r_j) of half the chord with impact parameter r_k; 0 for j = 0 and for j > k.  Brought out of the
 *                  order the kernels read into dense rows on the host;
 *   raw            NULL, or 256 ceil(L / 16)^2 doubles: the table as it lies in memory, [row tile kt][step s][lane],
 *                  lane l of step s holding ds[16 kt + l % 16][4 s + l / 16].  Row tile kt is written
 *                  and read up to step 4 kt + 3 (its diagonal tile): there the entries with k >= L, j > k or j = 0
 *                  are 0; the steps behind it are never written nor read (ds reports them as 0).
 * BARTRT_EINVAL: an eclipse engine; rtop or ds NULL; no launch yet (or its buffers have been regrown since); a walker
 * index outside the latest batch.  A batch that went out in chunks leaves its last chunk; bartrt_get_tau_of runs its
 * walker again as a batch of one. */
int bartrt_get_chord_table(int walker, double *rtop, double *ds, double *raw);

/* Band-averaged contribution functions and transmittance of a batch of profiles: BART's
 * post-processing (code/cf.py:114-199, called at BART.py:626-644) on the optical depth
 * bartrt_get_tau_of would return for each walker with `toomuch` infinite -- the engine's
 * own `toomuch` and `cut` have no effect; below a cloud deck's layer the depth repeats.
 * With tau[k] from the top (k = 0 the top layer):
 *   BARTRT_CF_CONTRIB   cf[k] = B(T_k, nu) (exp(-tau[k-1]) - exp(-tau[k])) / (ln p_k - ln p_{k-1}),
 *                       cf[0] = 0 (cf_eq; the vertical depth under the rule in force) --
 *                       eclipse geometry only (BARTRT_ENOTSUP on a transit engine);
 *   BARTRT_CF_TRANSMIT  exp(-tau[k]) (eclipse: vertical depth; transit: chord depth at r_k).
 * Per filter f the band value is trapz(x resp) / trapz(resp) with UNIT spacing over the
 * filter's window (filter_cf: np.trapz without x, half weights at the window's two ends).
 * Normalisation (filt_cf_norm) is left to the caller (bart_amd.engine.contribution).
 *
 * bartrt_cf_setup: the filter windows on the FULL grid (on a sharded engine too): filter f covers samples idx0[f] ..
 * idx0[f] + npts[f] - 1 (at least two, inside the grid) with the filter's response already
 * interpolated onto them, resp = the nfilters windows concatenated (bart_amd.cf.filter_windows
 * builds them as filter_cf does: the samples strictly inside the filter's wavenumber range).
 * Kept until the next setup, bartrt_init or bartrt_free_memory.
 *
 * bartrt_cf_batch: prof[nwalkers][nprof] as bartrt_run_transit_batch ->
 * band[nwalkers][nfilters][nlayers] in atm layer order (what cf.cf / cf.transmittance return,
 * per walker); full[nwalkers][nwave][nlayers] (atm layer order: the per-wavenumber values,
 * cf_eq's array transposed) or NULL.  ok[nwalkers] as bartrt_run_transit_batch (a flagged
 * walker's band rows are NaN); with ok NULL a flagged profile fails the call.
 * bartrt_cf_batch_dev: the same on device buffers, asynchronous on `stream` (NULL: the
 * engine's own); d_ok may be NULL.
 *
 * The engine-wide setters (radius, cloud top, scattering) apply as to run_transit_batch.  A call
 * leaves the engine's other state alone: the profile behind bartrt_get_tau /
 * _get_intensity, a pending bartrt_prefetch_profiles_dev request, the timing and
 * walked-layer records, bartrt_get_radius.  Results are bit-identical from run to run and
 * do not depend on which other walkers share the call.  Internally the walkers go in chunks
 * whose workspace stays under BARTRT_CF_WORKSPACE_BYTES (default 256 MiB).
 * BARTRT_ENOTSUP: line-by-line engines, sharded engines (--shard) WITHOUT a communicator, chain-service clients.
 *
 * Sharded engines (--shard r n) with a communicator attached (bartrt_comm_init): every call of this block is
 * accepted, bartrt_cf_setup included, and bartrt_comm_free brings BARTRT_ENOTSUP back.  The windows are still
 * stated on the FULL grid.  Each rank works on its own block [lo, hi): the windows clipped to it (the half weights of
 * the unit-spacing trapezoid stay at a window's true first and last sample, whichever rank holds them; a sample where
 * the block cuts a window has weight 1; a filter without a sample on a rank contributes 0 there), its sums
 * part[walker][filter][layer] -- layers from the top, added in tile order, not yet divided -- written straight into
 * this rank's slot of the communicator's receive buffer.  Per chunk of walkers ONE in-place ncclAllGather on the
 * call's stream fills the other slots, and one kernel adds the slots in rank order (no atomics), divides by the
 * whole window's trapz(resp) and writes atm layer order.  Every rank makes the same calls with the same arguments
 * and the same BARTRT_CF_WORKSPACE_BYTES (the chunk size follows from the windows and the largest block, never from
 * the rank's own block) and gets the same band rows bit for bit; they agree with the unsharded engine's to the
 * rounding of a differently associated sum.  `full` is the rank's own [nwalkers][hi - lo][nlayers].  The ok flags and
 * the per-walker settings do not depend on wavenumber: every rank flags the same walkers.  An unsharded engine with
 * a communicator of one rank takes the same code and returns the bits it returns without one.  The sharded form has
 * run on one GPU only (ranks one after the other, two processes on one device, RCCL worlds of one): no time is
 * stated for it because none has been measured, and no machine with more than one GPU has run it.
 *
 * For callers that run their own collective, and for one GPU standing in for any rank count (the counterpart of
 * bartrt_step_bandflux_blocks_dev); no communicator needed, any table engine, sharded or not:
 *   bartrt_cf_setup_block    bartrt_cf_setup's arguments and tables for the engine's block, accepted on a sharded
 *                            engine without a communicator (where bartrt_cf_setup keeps refusing).
 *   bartrt_cf_partials_dev   d_prof[nwalkers][nprof] -> this engine's d_part[nwalkers][nfilters][nlayers] as above;
 *                            d_over[nwalkers][3] as bartrt_cf_batch_over_dev or NULL; d_full (the block's own
 *                            [nwalkers][hi - lo][nlayers]) and d_ok may be NULL.  Asynchronous on `stream`.
 *   bartrt_cf_combine_dev    d_slots = nranks slots of nwalkers * nfilters * nlayers doubles, slot r = rank r's
 *                            d_part -> d_band[nwalkers][nfilters][nlayers]; NaN rows where d_ok[w] == 0 (NULL: no
 *                            walker is flagged).  1 <= nranks <= the grid's sample count.  On one slot: the bits
 *                            of bartrt_cf_batch_dev.
 *
 * bartrt_cf_batch_over / _over_dev: the same with every walker under its OWN settings -- a
 * posterior's samples, whose radius, cloud top and scattering are fitted parameters
 * (BARTfunc.py:350-360).  over[nwalkers][3] = {reference radius in km, log10(cloud-top pressure /
 * bar), Rayleigh value}: what bartrt_set_radius, bartrt_set_cloudtop and
 * bartrt_set_scattering(1, value) take.  NaN in a slot = the engine-wide setting for that walker
 * (no cloud top where none is set); a cloud top above the top layer puts the deck on the top
 * layer, as the setter does; the Rayleigh value acts under scattering flag 1 only (flag 2, the
 * polarisability flavour, has no value).  A radius that is not a positive finite number: the host
 * form refuses the call (BARTRT_EINVAL, as bartrt_set_radius does); the _dev form, which cannot
 * look, flags that walker (ok[w] = 0, NaN band rows) and computes the others.  The host form
 * converts the units on the host with the setters' own arithmetic: a walker gets exactly the deck
 * layer the setter would give it.  The _dev form converts on the device, whose 10^x may differ
 * from the host's in the last bit -- visible only for a cloud top that equals a layer's pressure to
 * the bit.  A transit engine's chord depths are those of the walker's own hydrostatic
 * radii.  over == NULL: bartrt_cf_batch's launches, arguments and bits.  The promises above hold:
 * a walker's result depends on its profile and its three values only -- not on the other walkers
 * or their settings, not on the chunking -- and nothing else of the engine changes.
 *
 * bartrt_cf_params / _params_dev: parameters in.  params[nwalkers][npars] as bartrt_step_batch
 * takes them (after bartrt_step_setup and bartrt_cf_setup; BARTRT_EINVAL without either or with
 * another npars) go through the step's own converter -- T(p) model, abundance scaling and
 * renormalisation, bounds -- and the slots declared with bartrt_step_set_extras become the
 * walker's overrides; then as bartrt_cf_batch_over.  The rows of an MC3 output, expanded to full
 * parameter vectors, are this call's input (bart_amd.cf.posterior).
 *   status[w]   0, 1 (temperature) or 2 (abundance), exactly what bartrt_step_batch reports for
 *               the row; 3 (energy balance) is never raised: no spectrum is computed.  May be NULL.
 *   rejected    a sample with status != 0 has NaN in its band rows (its rows of `full` are
 *               undefined); it does not fail the call.
 *   carry       bartrt_step_set_carry has no effect: samples are independent, a parameter set
 *               the T(p) model rejects gets status 1.
 *   scattering  with flag 2 the Rayleigh slot is present and unused, as in the step.
 *   radius      a radius slot that is not a positive finite number leaves status as the step
 *               reports it and NaN in the sample's band rows (the step converts the slots on the
 *               device as well: cloud tops are the step's own, bit for bit).
 * The engine limits and BARTRT_ENOTSUP cases of bartrt_cf_batch apply unchanged. */
#define BARTRT_CF_CONTRIB  0
#define BARTRT_CF_TRANSMIT 1
int bartrt_cf_setup(int nfilters, const int *idx0, const int *npts, const double *resp);
int bartrt_cf_batch(const double *prof, int nwalkers, int nprof, int kind,
                    double *band, double *full, unsigned char *ok);
int bartrt_cf_batch_dev(const double *d_prof, int nwalkers, int kind,
                        double *d_band, double *d_full, unsigned char *d_ok, void *stream);
int bartrt_cf_batch_over(const double *prof, int nwalkers, int nprof, const double *over, int kind,
                         double *band, double *full, unsigned char *ok);
int bartrt_cf_batch_over_dev(const double *d_prof, int nwalkers, const double *d_over, int kind,
                             double *d_band, double *d_full, unsigned char *d_ok, void *stream);
int bartrt_cf_params(const double *params, int nwalkers, int npars, int kind,
                     double *band, double *full, int *status);
int bartrt_cf_params_dev(const double *d_params, int nwalkers, int npars, int kind,
                         double *d_band, double *d_full, int *d_status, void *stream);
int bartrt_cf_setup_block(int nfilters, const int *idx0, const int *npts, const double *resp);
int bartrt_cf_partials_dev(const double *d_prof, int nwalkers, int kind, const double *d_over,
                           double *d_part, double *d_full, unsigned char *d_ok, void *stream);
int bartrt_cf_combine_dev(const double *d_slots, int nranks, int nwalkers, const unsigned char *d_ok,
                          double *d_band, void *stream);

/* Diagnostics (tests): what the contribution-function kernel of the latest call's LAST chunk read for walker `walker`
 * of that chunk, and the filter tables of the latest setup -- the module prepares its walkers into workspaces of its
 * own, which bartrt_get_prep_records and bartrt_get_chord_table do not see.  A host-side copy after a synchronisation
 * of the module's latest stream; no kernel runs.  The call fills the scalar fields first, so a call with walker < 0
 * and every buffer NULL is the shape query (BARTRT_OK once a setup exists); then each buffer that is not NULL:
 *   coef, idx, kstop, ok   as bartrt_get_prep_records.  After a device-buffer call that passed d_ok the flag is read
 *                          from THAT buffer, as bartrt_get_prep_records reads it: the caller keeps it allocated until
 *                          the read-back (the module does not copy flags it was not asked to keep);
 *   rdlp[L]                1 / (ln p_k - ln p_{k-1}), k from the top; [0] is 0 and unused;
 *   rtop[L], ds[L][L]      transit engines only, as bartrt_get_chord_table (BARTRT_EINVAL on an eclipse engine);
 *   tile_ptr[ntiles + 1]   the entries of tile t (64 samples of the engine's block) are tile_ptr[t] .. tile_ptr[t+1]-1,
 *                          one per filter with a sample on the tile, filters ascending;
 *   wt[nent][64]           an entry's weights h_i resp_i on its tile's lanes, 0 outside the window;
 *   f_ptr[nfilters + 1], f_ent[nent]   filter f's entries in tile order: f_ent[f_ptr[f] .. f_ptr[f+1]-1];
 *   trapz[nfilters]        the divisor of each filter's band value;
 *   nwalkers               of the latest chunk (0: none since the latest setup, or its launch was refused);
 *   kernel, lds_bytes      the CF kernel of the latest launch (also of a refused one) and its dynamic LDS.
 * BARTRT_EINVAL: no bartrt_cf_setup; no call since it; a walker outside the latest chunk. */
#define BARTRT_CF_KERNEL_ECLIPSE          0
#define BARTRT_CF_KERNEL_TRANSIT_STAGED   1   /* the layer records staged in LDS */
#define BARTRT_CF_KERNEL_TRANSIT_UNSTAGED 2   /* read where they lie: deep columns */
typedef struct bartrt_cf_records {
  int nlayers, nmol, ncs, transit, nwalkers, nfilters, ntiles, nent, kernel, kstop, ok;   /* transit: 1 on a transit engine */
  long long lds_bytes;
  double *coef;
  long long *idx;
  double *rdlp, *rtop, *ds;
  int *tile_ptr;
  double *wt;
  int *f_ptr, *f_ent;
  double *trapz;
} bartrt_cf_records;
int bartrt_cf_get_records(int walker, bartrt_cf_records *r);

/* ---- exact order statistics, posterior envelopes (csrc/quant.hip, csrc/quant_core.hpp) ----
 * bartrt_colselect_dev: order statistics of the columns of a row-major matrix in device memory.
 *   d_x[nrows][ld]   doubles, of which the first ncols <= ld columns of every row are read
 *   d_ok[nrows]      or NULL: rows with 0 do not exist for the selection
 *   ranks[nranks]    HOST array, 1 <= nranks <= 16, zero-based ranks among the rows that count; any order,
 *                    duplicates allowed
 *   d_out[nranks][ncols]  out[r][c] is the value np.sort(x[ok, c])[ranks[r]] has, bit for bit: the values are
 *                    selected (a radix select on order-preserving 64-bit keys), not computed.  NaNs of
 *                    either sign sort behind +inf and come back with a clear sign bit; -0 sorts before +0.
 * Asynchronous on `stream` (NULL: the engine's own).  The counts are integers added by atomics: the result
 * depends on no launch shape.  It needs an initialised engine for the stream and the scratch buffers, and
 * nothing else from it (any geometry, sharded or not, line-by-line or not).
 *   BARTRT_EINVAL    nranks outside 1..16, a negative rank, ld < ncols, nrows < 1 (or above 2^31 - 1),
 *                    ncols < 0 or above 65535 * 64, a NULL buffer; the message names the argument.
 *   rank too large   the _dev form cannot look at the mask: for a rank at or above the number of rows that count
 *                    it writes NaN into that rank's row of d_out and reports nothing (as
 *                    bartrt_cf_batch_over_dev flags a walker instead of failing).  The host form
 *                    bartrt_colselect (host buffers, the engine's stream, waits) counts the rows first and
 *                    refuses such a rank, and a mask without a row, with BARTRT_EINVAL.
 * bartrt_colselect_slab: *rows = what one workgroup owns of a column (the default, or what
 * bartrt_colselect_set_slab set; 0 restores the default).  For tests: results do not depend on it.
 *
 * bartrt_posterior_tp: the percentile envelope of the temperature profiles of a posterior (reference
 * code/bestFit.py:429-466), after bartrt_step_setup.
 *   params[nsamples][npars]  HOST, rows as bartrt_step_batch takes them; they go through the kernels of
 *                    bartrt_step_profiles_dev in chunks (bartrt_posterior_set_chunk rows, 0: the default;
 *                    the result does not depend on it) and their temperature rows stay on the device
 *   q[nq]            1 <= nq <= 8 percents in [0, 100]
 *   env[nq][L]       HOST: percentile q[i] of every layer (atm order) over the accepted samples (status 0),
 *                    by np.percentile's default linear rule from the two neighbouring order statistics
 *   status[nsamples] 0, 1 (temperature), 2 (abundance) as bartrt_cf_params reports it; bartrt_step_set_carry
 *                    has no effect here either
 *   *ngood           the accepted samples.  None accepted: env is NaN, *ngood = 0, and the call succeeds.
 * bartrt_posterior_tp_order: the order statistics behind the latest envelope, ranks[2 nq] (lo, hi of each
 * percent) and order[2 nq][L]; BARTRT_EINVAL when there is none of that shape.
 * bartrt_percentile_rule / bartrt_percentile_lerp need no engine: the rule's two ranks and weight for n values
 * and percent q, and out[i] = the value between a[i] (rank lo) and b[i] (rank hi) at weight w. */
int bartrt_colselect_dev(const double *d_x, long nrows, int ncols, long ld, const unsigned char *d_ok,
                         int nranks, const long *ranks, double *d_out, void *stream);
int bartrt_colselect(const double *x, long nrows, int ncols, long ld, const unsigned char *ok,
                     int nranks, const long *ranks, double *out);
int bartrt_colselect_slab(long *rows);
int bartrt_colselect_set_slab(long rows);
int bartrt_posterior_tp(const double *params, long nsamples, int npars, int nq, const double *q,
                        double *env, int *status, long *ngood);
int bartrt_posterior_set_chunk(long rows);
int bartrt_posterior_tp_order(int nq, int nlayers, long *ranks, double *order);
int bartrt_percentile_rule(long n, double q, long *lo, long *hi, double *w);
int bartrt_percentile_lerp(const double *a, const double *b, double w, double *out, long n);

/* ---- posterior spectra: the display quantity, spectrum and band-flux envelopes (csrc/specenv.hip,
 * csrc/specenv_core.hpp) ----
 * What the reference's best-fit spectrum figure plots (reference code/bestFit.py:528-688) is the DISPLAY QUANTITY of a
 * model spectrum: for an eclipse gaussian_filter1d(spectrum / sflux * rprs * rprs, 2) (:645-648), for transit and direct
 * geometry gaussian_filter1d(spectrum, 2) (:655, :662).  The rule, stated once for host and device:
 *   value      with a stellar flux y[i] = x[i] / sflux[i] * rprs * rprs, left to right (numpy's bits); without, x[i]
 *   smoothing  scipy.ndimage.correlate1d with the symmetric kernel half[0..r] (half[0] the centre, 0 <= r <= 64) in
 *              mode `reflect` (d c b a | a b c d | d c b a, repeated as often as needed: any row length from 1);
 *              the centre term first, then the pairs (y[l-j] + y[l+j]) half[j] from j = r inwards, no contraction.
 *              r = 0 is the identity.  The library does not compute weights: the caller passes them
 *              (bart_amd.posterior.gauss_half makes SciPy's for a sigma)
 *   stride     >= 1: output column c is grid sample c * stride, Wk = ceil(nwave / stride) columns; the smoothing
 *              always runs on the full grid
 * bartrt_spectrum_display_dev: the kernel alone on device buffers, asynchronous on `stream` (NULL: the engine's own).
 *   d_spec[nrows][ld]  spectra, the first nwave <= ld samples of every row read
 *   d_sflux[nwave]     or NULL
 *   half[r + 1]        HOST
 *   d_out[nrows][ldo]  the first Wk <= ldo columns of every row written, every value by exactly one lane: the result
 *                      depends on no launch shape
 *   BARTRT_EINVAL      r outside 0..64, stride < 1, ld < nwave, ldo < Wk, nrows < 1, nwave < 1, a NULL buffer; the
 *                      message names the argument.  It needs an initialised engine for the stream only.
 * bartrt_spectrum_display_tile: *cols = the kept output columns one workgroup owns for (r, stride) (tests place
 * their shapes around it).
 *
 * bartrt_posterior_spectrum: the percentile envelopes of the display quantity and of the band fluxes of a posterior,
 * after bartrt_step_setup (whose rprs is the one used).
 *   params[nsamples][npars]  HOST, rows as bartrt_step_batch takes them; they go through bartrt_step_batch_dev in
 *                    chunks (bartrt_posterior_set_chunk rows, at most 4096: a larger setting is cut to that, and
 *                    every launch's RT kernel variant is chosen as for 4096 walkers, so the result does not depend
 *                    on the chunk; a one-row call therefore runs the large-batch variant, not the small-batch
 *                    forms bartrt_step_batch_dev would pick), every chunk's spectra through the display kernel
 *                    into one [nsamples][Wk] matrix on the device -- nsamples * Wk * 8 bytes; where that does not
 *                    fit, BARTRT_EINVAL names the bytes: raise stride, or thin the samples -- and its band fluxes
 *                    into one [nsamples][nfilters] matrix
 *   q[nq]            1 <= nq <= 8 percents in [0, 100]
 *   sflux[nwave]     HOST or NULL: the stellar flux on the engine's wavenumber grid (eclipse)
 *   env_spec[nq][Wk], env_band[nq][nfilters]   HOST: percentile q[i] of every column over the accepted samples, by
 *                    np.percentile's default rule from two order statistics selected on the device (bartrt_colselect_dev)
 *   status[nsamples] 0, 1 (temperature), 2 (abundance), 3 (energy balance): every status but 0 drops the sample;
 *                    bartrt_step_set_carry has no effect
 *   *ngood           the accepted samples.  None accepted: both envelopes are NaN, *ngood = 0, the call succeeds.
 *   BARTRT_ENOTSUP   a wavenumber-sharded engine (the spectra are not whole on this GPU).  Line-by-line engines
 *                    are served.
 * bartrt_posterior_spectrum_shape: *Wk = ceil(nwave / stride) and *F = the filters of bartrt_step_setup: the widths
 * of the envelopes a call with that stride writes.
 * bartrt_posterior_spectrum_order: the order statistics behind the latest envelope: ranks[2 nq] (lo, hi of each
 * percent), order_spec[2 nq][Wk], order_band[2 nq][F]; BARTRT_EINVAL when there is none of that shape.
 * bartrt_posterior_spectrum_rows: rows row0 .. row0 + nrows - 1 of the latest sample matrix -> out[nrows][Wk] (HOST),
 * rejected samples' rows included as they lie; BARTRT_EINVAL when there is no matrix or the range is outside it. */
int bartrt_spectrum_display_dev(const double *d_spec, long nrows, int nwave, long ld, const double *d_sflux,
                                double rprs, int r, const double *half, long stride, double *d_out, long ldo,
                                void *stream);
int bartrt_spectrum_display_tile(int r, long stride, long *cols);
int bartrt_posterior_spectrum(const double *params, long nsamples, int npars, int nq, const double *q,
                              const double *sflux, int r, const double *half, long stride, double *env_spec,
                              double *env_band, int *status, long *ngood);
int bartrt_posterior_spectrum_shape(long stride, long *Wk, int *F);
int bartrt_posterior_spectrum_order(int nq, long Wk, int F, long *ranks, double *order_spec, double *order_band);
int bartrt_posterior_spectrum_rows(long row0, long nrows, double *out);

/* ---- posterior marginals: 1-D and pairwise histograms, their range, HPD regions (csrc/hist.hip,
 * csrc/hist_core.hpp) ----
 * The numbers behind MC3's `histogram` and `pairwise` figures (reference code/mc3plots.py:45-82).  NO ENGINE is
 * needed (as for bartrt_mcmc_gr): the calls own their scratch on the current HIP device, so an output.npy can be
 * post-processed without an opacity grid.
 * bartrt_marginals_dev: histograms of selected columns of a row-major matrix in device memory.
 *   d_x[nrows][ld]   doubles, parameters fastest, as a chain lies (and as bartrt_colselect_dev reads it)
 *   d_ok[nrows]      or NULL: rows with 0 do not exist
 *   cols[nsel]       HOST array, 1 <= nsel <= 64 selected columns in [0, ld), any order, not necessarily adjacent
 *   edges[nsel][nbins + 1]  HOST array: per selected column nbins + 1 finite, strictly increasing edges,
 *                    uniform or not.  x is in bin i iff edges[i] <= x < edges[i + 1]; x == edges[nbins] is in
 *                    bin nbins - 1.  The decision is the comparison with the edges themselves, so the counts
 *                    are np.histogram(col, bins=edges)'s and np.histogram2d(a, b, bins=[ea, eb])'s, integer
 *                    for integer -- also for edges = np.linspace(lo, hi, nbins + 1) against numpy's
 *                    bins=nbins, range=(lo, hi).  -0.0 and +0.0 fall in the same bin.
 *   d_h1[nsel][nbins]       the 1-D counts
 *   d_out[nsel][3]   what is in no bin: below edges[0] (-inf included), above edges[nbins] (+inf included), NaN.
 *                    sum(h1[s]) + sum(out[s]) is the number of rows that count, for every s.
 *   d_h2[npairs][nbins][nbins]  or NULL (no pairs wanted).  npairs = nsel (nsel - 1) / 2 pairs of SELECTION
 *                    indices a < b, a-major: (0,1), (0,2), ..., (1,2), ...; the first bin index is a's, so
 *                    h2[p] is np.histogram2d(x[:, cols[a]], x[:, cols[b]], bins=[edges[a], edges[b]])[0].  A row
 *                    counts in a pair iff both values are in range.  nsel == 1: npairs = 0, d_h2 is not touched.
 * All counts are unsigned 64-bit, zeroed by the call and added with integer atomics: they depend on no launch
 * shape, slab or chunk.  Asynchronous on `stream` (NULL: the null stream).  One call at a time uses the
 * scratch: a call first waits, on the host, for the device work of the previous one.
 *   BARTRT_EINVAL    (the message names the argument; the outputs are not touched) nsel outside 1..64; a column
 *                    outside [0, ld), which is also how an ld below the largest selected column + 1 shows;
 *                    nbins outside 1..1024, or above 128 with d_h2 not NULL; an edge that is not finite or not
 *                    above the one before it; nrows < 1 or above 2^31 - 1; a NULL buffer other than d_ok, d_h2.
 * bartrt_marginals: the same from and to host memory.  The matrix goes up in row chunks of bounded size (64 MiB,
 * or bartrt_marginals_set_chunk rows; the whole matrix is never needed in HBM) and the counts add up on the
 * device.  The last row need only reach its last selected column.  Waits.
 * bartrt_marginals_range_dev / bartrt_marginals_range: lohi[nsel][2] the smallest and largest FINITE value of
 * every selected column among the rows that count, nfinite[nsel] their number, bit for bit np.nanmin / np.nanmax
 * over the finite values (minimum and maximum of order-preserving keys: exact in any order; -0.0 orders before
 * +0.0).  No finite value: NaN, NaN, 0.  The same selection arguments and refusals.
 * bartrt_marginals_slab / _set_slab: the rows one workgroup owns (0 restores the default; at most 2^24);
 * bartrt_marginals_chunk / _set_chunk: the rows per upload of the host forms (0: the default, by bytes).  For
 * tests: no result depends on either.
 * bartrt_hpd (host, no device): the highest-density region of a histogram at fraction 0 < p <= 1.  The bins are
 * ordered by descending count, ties by ascending index; the region is the shortest prefix whose cumulative count
 * c has (double)c >= p * (double)N, N = sum(counts).  mask[nbins] (1: included), *threshold the smallest count
 * included, *included the region's total, *nruns its number of maximal runs of bins (2: bimodal).  N == 0: an
 * empty mask and zeros.  This is MC3's credible region taken on the histogram instead of on a kernel density
 * estimate; the estimate itself is bartrt_kde below, and bartrt_hpd_pdf takes the region on it.  BARTRT_EINVAL:
 * nbins < 1, p outside (0, 1], a NULL buffer. */
int bartrt_marginals_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel,
                         const int *cols, int nbins, const double *edges, unsigned long long *d_h1,
                         unsigned long long *d_out, unsigned long long *d_h2, void *stream);
int bartrt_marginals(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols,
                     int nbins, const double *edges, unsigned long long *h1, unsigned long long *out,
                     unsigned long long *h2);
int bartrt_marginals_range_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel,
                               const int *cols, double *d_lohi, unsigned long long *d_nfinite, void *stream);
int bartrt_marginals_range(const double *x, long nrows, long ld, const unsigned char *ok, int nsel,
                           const int *cols, double *lohi, unsigned long long *nfinite);
int bartrt_marginals_slab(long *rows);
int bartrt_marginals_set_slab(long rows);
int bartrt_marginals_chunk(long *rows);
int bartrt_marginals_set_chunk(long rows);
int bartrt_hpd(const unsigned long long *counts, int nbins, double p, unsigned char *mask,
               unsigned long long *threshold, unsigned long long *included, int *nruns);

/* ---- posterior kernel density estimates (csrc/kde.hip; the rule is csrc/kde_core.hpp's) ---------------------
 * The density MC3 thresholds for a parameter's credible region: a Gaussian KDE of the samples of one column,
 * scipy.stats.gaussian_kde(col, bw_method)(grid) for one dimension.  NO ENGINE is needed; the calls own their
 * scratch on the current HIP device.
 * bartrt_kde_dev: densities of selected columns of a row-major matrix in device memory, each on its own grid.
 *   d_x[nrows][ld], d_ok[nrows] or NULL, cols[nsel]   as bartrt_marginals_dev takes them (cols a HOST array,
 *                    1 <= nsel <= 64).  A row counts for a column iff d_ok lets it AND the value is finite.
 *   grid[nsel][ngrid]  HOST array, 1 <= ngrid <= 1024 finite values per selected column, in any order, uniform or
 *                    not.
 *   bw_rule, bw_factor   the bandwidth h = factor * std: 0 Scott's factor n^(-1/5), 1 Silverman's (3 n / 4)^(-1/5),
 *                    2 bw_factor itself (> 0) -- scipy's bw_method = 'scott' | 'silverman' | scalar.
 *   d_pdf[nsel][ngrid]   pdf(g) = sum_i exp(-((g - x_i) / h)^2 / 2) / (n h sqrt(2 pi)) over the rows that count.
 *                    The exponential is the RT kernels' exp_rt, whose formula is within 7e-14 relative of exp
 *                    (its interpolant) plus 2.3e-17 per unit of |argument| / ln 2 (its rounded ln 2), and whose
 *                    fp64 evaluation is within 4e-16 of that formula: a density is within about 1e-13 relative of
 *                    the one taken with exp, not within rounding.  A term whose argument is below -708 is zero.
 *   d_stat[nsel][4]  n (as a double), mean, std (ddof 1), h.  The moments come from tiled (n, mean, M2) triples of
 *                    the values less the column's value in row 0, merged in ascending order: no sum of squares.
 *                    Row 0's value is taken whatever d_ok says of it (0.0 if it is not finite): mean and std are
 *                    as accurate as max |x - x[0]| / std allows, so a first row that holds a wild finite value (a
 *                    sentinel like 1e300), masked or not, takes digits from the std of an otherwise good column.
 *   d_nonfinite[nsel]  unsigned 64-bit: rows d_ok lets through whose value is an infinity or a NaN.  They are
 *                    counted here and otherwise do not exist (scipy would return NaN everywhere).
 * A column with n < 2, or whose std or h is zero or not finite, has h = NaN and a pdf row of NaN; the call
 * succeeds and the other columns are not affected.  The order of every floating-point sum is fixed by the rule
 * (tiles of bartrt_kde_tile consecutive rows of the matrix, rows ascending in a tile, tiles ascending) and there
 * are no floating-point atomics: the bits depend on no launch shape, chunk or schedule.  Asynchronous on
 * `stream` (NULL: the null stream).  One call at a time uses the scratch: a call first waits, on the host, for
 * the device work of the previous one.
 *   BARTRT_EINVAL    (the message names the argument; the outputs are not touched) nsel outside 1..64; a column
 *                    outside [0, ld); ngrid outside 1..1024; a grid value that is not finite; nrows < 1 or above
 *                    2^31 - 1; a NULL buffer other than d_ok; a bw_rule outside 0..2; bw_rule 2 with a bw_factor
 *                    that is not a finite number above 0.
 * bartrt_kde: the same from and to host memory.  The matrix goes up twice in row chunks of whole tiles (64 MiB or
 * one tile of rows, whichever is larger -- one tile is 16 kB times ld, above 64 MiB for ld > 4096 -- or
 * bartrt_kde_set_chunk rows rounded up to a tile), first for the moments, then for the sums; the whole matrix
 * is never needed in HBM.  The last row need only reach its last selected column.  Waits.
 * bartrt_kde_chunk / _set_chunk: the rows per upload of the host form, which also bound the rows one round of
 * launches of either form covers (0: the default, by bytes).  For tests: no result depends on it.
 * bartrt_kde_tile: the rows of a tile, a constant of the rule (tests place their shapes around it).
 * bartrt_hpd_pdf (host, no device): the credible region of a density pdf[n] on a grid at fraction 0 < p <= 1,
 * bartrt_hpd's sibling on doubles.  The points are ordered by descending pdf, ties by ascending index; cumulative
 * sums are formed in that order by plain additions and the total is the last of them; the region is the shortest
 * prefix whose sum c has c >= p * total.  mask[n], *threshold the smallest pdf included, *included the region's
 * sum, *nruns its number of maximal runs.  A NaN or a negative value, or total == 0: an empty mask and zeros.
 * The rule is this project's: MC3's credregion could not be read (the reference's MC3 submodule is empty), so
 * it is stated against SciPy's density and not checked against MC3's source.  BARTRT_EINVAL: n < 1, p outside
 * (0, 1], a NULL buffer. */
int bartrt_kde_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols,
                   int ngrid, const double *grid, int bw_rule, double bw_factor, double *d_pdf, double *d_stat,
                   unsigned long long *d_nonfinite, void *stream);
int bartrt_kde(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int ngrid,
               const double *grid, int bw_rule, double bw_factor, double *pdf, double *stat,
               unsigned long long *nonfinite);
int bartrt_kde_chunk(long *rows);
int bartrt_kde_set_chunk(long rows);
int bartrt_kde_tile(long *rows);
int bartrt_hpd_pdf(const double *pdf, int n, double p, unsigned char *mask, double *threshold, double *included,
                   int *nruns);

/* Line-by-line engines only (cfg has `linedb`, no `opacityfile`): the Voigt
 * extinction of one profile, ext[nlayers][nwave_local] in cm-1, atm layer order. */
int bartrt_get_lbl_extinction(const double *prof, int nprof, double *ext,
                              int nlayers, int nwave);

/* Diagnostics, line-by-line engines only: which accumulation kernel writes each (layer, 256-point tile
 * of the local grid) of bartrt_get_lbl_extinction(prof), owners[nlayers][ntile], ntile =
 * (nwave_local + 255) / 256, decided by the kernels' own predicates on the state vectors the
 * accumulation reads: 0 the tile kernel, 1 the pair kernel, 2 the line-major kernel (oversampled state),
 * 3 the same (BARTRT_MID_REACH), 4 the width-grid kernel, 255 none; bit 7 set: more than one. */
int bartrt_lbl_owners(const double *prof, int nprof, unsigned char *owners, int nlayers, int ntile);

/* Diagnostics, line-by-line engines only, host only: the state vectors the accumulation kernels read, as lbl_states
 * and lbl_smax wrote them for the latest line-by-line call (bartrt_get_lbl_extinction: nstate = nlayers, atm layer
 * order; a batch: walker-major; the opacity-grid generator: the last slab, [layer][temperature]).  Always sets
 * *nstate (0: no call yet), *niso (isotopes over all databases, database order) and *ngroup (databases).  With
 * buffers (either may be null): state[nstate][2 + 3 niso] = T, the oversampling divisor dv, then per isotope the
 * Doppler half-width per unit wavenumber, the Lorentz half-width (cm-1) and pi e^2 / (m_e c^2) * scale (scale:
 * n_i / Z_i(T), or ratio_i / (Z_i(T) m_mol) per gram in the generator); smax[nstate][ngroup] = the largest line
 * strength per (state, database).  BARTRT_EINVAL with buffers before any call, and for smax after
 * bartrt_lbl_owners (which computes no strengths).  No kernel runs. */
int bartrt_lbl_get_states(int *nstate, int *niso, int *ngroup, double *state, double *smax);

/* Diagnostics, no engine needed: the line-by-line kernels' Voigt function
 * K(x, y) = Re w(x + i y) (x >= 0: distance from the line centre in Doppler widths
 * / sqrt(ln 2); y > 0: Lorentz / Doppler width ratio) on n host (x, y) pairs. */
int bartrt_voigt(const double *x, const double *y, double *k, long n);
/* Diagnostics, no engine needed: the exponential integral E_2(x) as the "line" T(p)
 * model's kernels evaluate it (csrc/step.hip, expint_e2) on n host values:
 * x >= 0; 1.0 at 0, 0.0 beyond 709.78 and at +inf, NaN for NaN. */
int bartrt_expint_e2(const double *x, double *out, long n);
/* Diagnostics, no engine needed: one of the RT kernels' elementary functions (csrc/kernels.hpp; exp_rt_fma3:
 * csrc/lbl.hip), evaluated by the device exactly as the kernels call it, on n host values.  The exponentials take
 * -708 <= x <= 700 (exp_core: 709), the reciprocals normal positive numbers; nothing is checked, as in the kernels.
 * BARTRT_EINVAL for a selector that is not in this list. */
enum {
  BARTRT_RT_MATH_EXP_RT = 0,      /* exp_rt(x) */
  BARTRT_RT_MATH_EXP_RT_N4 = 1,   /* exp_rt_n<4> on four consecutive values per lane, every slot written */
  BARTRT_RT_MATH_EXP_RT_FMA3 = 2, /* the line-by-line kernels' copy of exp_rt */
  BARTRT_RT_MATH_EXP_CORE = 3,    /* exp_core(x) */
  BARTRT_RT_MATH_RCP_CORE = 4,    /* rcp_core(x): hardware estimate + two Newton steps */
  BARTRT_RT_MATH_RCP_N1 = 5,      /* rcp_n1(x): hardware estimate + one Newton step */
  BARTRT_RT_MATH_RCP_RAW = 6,     /* the hardware estimate alone */
  BARTRT_RT_MATH_PLANCK_INV = 7,  /* rcp_n1(exp_rt(fmin(x, 700.0)) - 1.0): the Planck term without its numerator */
  /* alive_flags (csrc/rt_eclipse_s1s.hpp), the ray flags of rule 1's `cut slant` kernel: x holds n / 2 pairs (tm, thr)
   * -- a running optical depth and a ray's threshold, 0 < thr < 1.7e308 --, and out[i], i < n / 2, is the flag of pair
   * i (1.0: tm <= thr, the ray is alive; 0.0: it is not); the rest of out is left alone.  The threshold's scaled form
   * is made by the host exactly as for a launch (bartrt_slant_thresholds).  BARTRT_EINVAL for an odd n or a threshold
   * outside that range. */
  BARTRT_RT_MATH_ALIVE_FLAGS = 8
};
int bartrt_rt_math(int which, const double *x, double *out, long n);

/* HIP-event timing of the RT kernel launches (bench.py's roofline leg).
 * begin resets; end returns accumulated device ms and launch count. */
int bartrt_timing_begin(void);
/* the same with events around every stride-th launch only: a pair of event records costs
 * the stream about 5 us, 7 % of a ten-walker step; end returns the sampled launches' sum
 * and their count */
int bartrt_timing_begin_sampled(int stride);
int bartrt_timing_end(double *kernel_ms, int *nlaunch);
/* Diagnostics for the byte model of bench.py: between begin and end every eclipse
 * launch records how many layers each wave walked before all its lanes passed
 * `toomuch`.  end returns the record of the LAST launch: walked[nwalkers][ncolumns]
 * (columns of wn_per_column consecutive wavenumbers, as the launched kernel tiles
 * the grid) and that kernel's name.  A transit launch records its kernel's name only
 * (no walkers, no columns). */
int bartrt_walked_begin(void);
int bartrt_walked_end(int *walked, int cap, int *nwalkers, int *ncolumns, int *wn_per_column,
                      char *kernel, int kernel_len);
/* With the same record (after bartrt_walked_end): restarts[nwalkers], per walker of the last launch the waves that
 * walked their column a second time (bartrt_set_slant_opt; 0 for every other kernel). */
int bartrt_walked_restarts(int *restarts, int cap, int *nwalkers);
/* Shapes outside the ahead-of-time set (seven and more table molecules with two cross-section files under the default
 * spline, nine and more molecules, ten and more ray angles) are instantiated from the same kernel templates when they
 * are first launched (hiprtc; cached under BARTRT_RTC_CACHE, default ~/.cache/bartrt; BARTRT_RTC=0 or a machine without
 * libhiprtc: the generic kernel serves them, 3-10x slower).  *available: a compiler is at hand; kernels compiled /
 * loaded from the disk cache / failed by this process so far, and the seconds spent compiling.  bartrt_walked_end's
 * kernel name carries " [instantiated at run time]" for such a launch (and " [prepares its own walkers]" where a
 * few-walker launch built its layer records in its own prologue instead of a preparation launch: BARTRT_FOLD=0 off;
 * " [table through a moving window]" where a row-per-layer kernel addressed a table of 4 GB or more, or any table under
 * BARTRT_WINDOW, through its per-step window).  Pointers may be NULL. */
int bartrt_get_rtc_stats(int *available, int *compiled, int *from_disk, int *failed, double *compile_seconds);
/* Compiles bartrt::<expr> (a template-id of the kernel headers, e.g. "rt_eclipse_simpson_slant<5, 9, 4, true, 1>")
 * for gfx950 and discards the result: *code_bytes = the code object's size.  Needs no GPU -- a check that the embedded
 * sources and the compiler at hand agree.  BARTRT_ENOTSUP without a compiler or on a compile error (bartrt_last_error). */
int bartrt_rtc_compile(const char *expr, int ilp, long *code_bytes);
/* algorithmic bytes one launch of the RT kernel moves for `nwalkers`
 * (2*L*W*M*8 + 2*L*W*8*ncia + (S+1)*L*8 + W*8 per spectrum) */
double bartrt_algorithmic_bytes(int nwalkers);

#ifdef __cplusplus
}
#endif
#endif
