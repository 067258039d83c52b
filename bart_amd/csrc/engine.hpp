// Host-side engine state: parsed inputs, HBM-resident tables, workspaces.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "devbuf.hpp"
#include "io.hpp"
#include "kernels.hpp"

namespace bartrt {

hipError_t launch_prep(const PrepArgs &a, hipStream_t st);
hipError_t launch_rt(const RtArgs &a, int block, hipStream_t st, RtLaunchInfo *info = nullptr);
hipError_t launch_rt_folded(const RtArgs &a, const PrepArgs &prep, int block, hipStream_t st, RtLaunchInfo *info, bool *folded);
// info (optional): what was launched (its name; window: the matrix-tile kernel read the table through the moving window)
hipError_t launch_transit(const RtArgs &a, hipStream_t st, RtLaunchInfo *info = nullptr);
hipError_t launch_chord_table(const PrepArgs &a, hipStream_t st);  // transit geometry, after launch_prep
hipError_t launch_grid_transpose(const double *src, double *dst, long planes, int M, int W, hipStream_t st);

int parse_integ(const std::string &v);  // "0" / "transmittance", "1" / "simpson", "2" / "trapz_tau"
// what `shareOpacity` means for this process (ShareMode, svc.hpp): cfg key, BARTRT_SHARE_OPACITY, BARTRT_SHARE_MODE,
// BARTRT_SERVICE; no_service: the caller needs the engine in its own process (the service reading becomes IPC)
int resolve_share_mode(const TCfg &cfg, bool no_service);

struct TableShare;  // the opacity grid shared between processes (share.hpp)
struct StepArgs;  // converters around the engine (step.hip)
struct Lbl;       // line-by-line extinction (lbl.hip)
struct Comm;      // the ranks' communicator (comm.hpp)
struct CfState;   // contribution-function tables and workspaces (contrib.hip)
struct QuantState;  // scratch of the order statistics and the posterior envelope (quant.hip)
struct SpecEnvState;  // the display matrix and the scratch of the posterior spectrum envelope (specenv.hip)

// The stream and the timing events, as a base of Engine: a base outlives the members, so every buffer the engine
// owns (DevBuf / PinBuf members, freed by their own destructors) goes before the events, and the stream goes last.
struct EngineStream {
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> ev;
  ~EngineStream();
};

// One set of layer records as prep_profiles writes them; the engine holds two (prefetched preparation, below)
struct RecordSet {
  DevBuf<double> coef;
  DevBuf<idx_t> idx;
  DevBuf<int> kstop;
  DevBuf<unsigned char> ok;
  void reserve(size_t cap, int L, int M, int C) {   // room for cap walkers
    coef.reserve(cap * L * coef_stride(M, C));
    idx.reserve(cap * L * idx_stride(C));
    kstop.reserve(cap);
    ok.reserve(cap);
  }
};

// Everything ONE launch is asked to do (Engine::run).  It travels by const reference from the entry point through the
// chunking down to run_chunk; the engine keeps nothing of it, so no caller has anything to clear afterwards.
struct RunRequest {
  const double *prof;         // [n][(S+1) L] profiles, where the device reads them
  int n;                      // walkers
  double *spec;               // [n][W] spectra
  unsigned char *ok;          // [n] flags; null: the engine's own (rec[0].ok)
  hipStream_t stream;
  bool want_tau = false;      // single walker: optical depths and last layers into d_tau / d_last
  bool want_intens = false;   // single walker, eclipse geometry: intensities per angle into d_intens
  // per-walker radius / cloud-top / scattering overrides [n][3] for the prep launch (NaN: the engine's own value);
  // over_cloud: a cloud top is among them (or among a hook's), so the RT kernels add the deck's surface term
  const double *over = nullptr;
  bool over_cloud = false;
  int sel_walkers = 0;        // > 0: the walker count the kernel variant is chosen for instead of the batch's own (RtArgs::nsel)
  int scat_flag = -1;         // the scattering flag of this launch alone; -1: the engine's
  // when set, run_chunk calls it instead of launch_prep (the per-step path fuses T(p) + abundances into that launch, step.hip)
  hipError_t (*prep_hook)(const PrepArgs &, hipStream_t, void *) = nullptr;
  void *prep_hook_ctx = nullptr;
  // filled in by run() and run_chunks(), not by callers: the batch named for the call after this one (Engine::Pending),
  // and the line-by-line forms -- the chunk's extinction [n][L][W], or the lazy fused kernel
  const double *next_prof = nullptr, *d_ext = nullptr;
  int next_n = 0;
  bool lbl_fused = false;
  RunRequest(const double *prof_, int n_, double *spec_, unsigned char *ok_, hipStream_t st)
      : prof(prof_), n(n_), spec(spec_), ok(ok_), stream(st) {}
};

struct Engine : EngineStream {
  // configuration
  TCfg cfg;
  Atm atm;
  MolInfo mol;
  int L = 0, S = 0, M = 0, Nt = 0, C = 0, A = 0;
  int Wfull = 0, lo = 0, hi = 0;  // this process holds [lo, hi) of the grid
  int W() const { return hi - lo; }
  std::vector<double> wn_full, tgrid, mass, angles;
  std::vector<int> opmol;
  double toomuch = 20.0, gsurf = 0, refpress = 0, refradius = 0;
  int scat_flag = 0, iH2 = -1, iHe = -1, has_cloud = 0;
  int solution = 0;       // 0 eclipse (emergent flux), 1 transit (modulation)
  int integ = 0;          // integration rule of the eclipse geometry (integ.hpp); cfg `integ`, BARTRT_INTEG
  bool cut_slant = false; // cfg `cut slant` / BARTRT_CUT: the toomuch cut per ray angle, on its slant depth (C19)
  // Sharded engines (--shard): is the kernel variant chosen by this block's own columns (true, the default since round 5:
  // a WASP-12b block of 303 samples x 10 walkers takes the layer-parallel kernel, 16 us, instead of the single-wave
  // kernel's latency floor, 52 us; spectra agree with the unsharded run's to 4e-16) or by the WHOLE grid's (false: cfg
  // `kernel_by whole` / BARTRT_KERNEL_BY=whole / bartrt_set_kernel_by -- the blocks then are the unsharded run's bits)
  bool kernel_by_local = true;
  bool cia_spline = false; // cfg `cia_interp spline` / BARTRT_CIA_INTERP: natural cubic splines in wavenumber and T (C20)
  double starrad = 0;     // cm, transit geometry
  double scat_value = 0, cloudtop = 0;
  double cloud_rup = 0, cloud_rdown = 0, cloud_ext = 0;  // radius-ramp cloud (cm, cm, cm-1); 0 = none
  bool transparent = false;                              // transit geometry: no opaque core
  int device = 0;
  // device-resident inputs
  const double *d_kappa = nullptr;    // the table the kernels read: kappa_own's, or kappa_share's mapping
  DevBuf<double> kappa_own, d_cia, d_wn, d_wn_full, d_press, d_mass, d_diam;
  TableShare *kappa_share = nullptr;  // cfg `shareOpacity`: d_kappa is (or is mapped from) another process's allocation
  int share_mode = -1;                // ShareMode (svc.hpp); -1: resolved from the cfg and the environment by setup()
  DevBuf<double> d_prep_consts;  // PrepArgs::consts
  PrepArgs prep{};  // static part filled at init
  RtArgs rt{};
  // workspaces (grown on demand, never inside a timed launch sequence twice)
  int cap_walkers = 0;
  DevBuf<double> d_prof, d_spec;
  RecordSet rec[2];                   // rec[1]: allocated at the first prefetch request (ensure_second_set)
  // The profiles of the latest host-buffer call, which the optical-depth / intensity getters re-run.  They lie in d_prof
  // or in h_pin, and are forgotten when that memory no longer holds them: d_prof regrown (ensure_walkers), h_pin regrown
  // (ensure_pin), h_pin filled with parameters instead (step_run_host); a device-buffer call keeps nothing.
  const double *last_prof = nullptr;
  int last_n = 0;
  void remember_profiles(const double *p, int n) { last_prof = p; last_n = n; }
  void forget_profiles() { last_prof = nullptr; last_n = 0; }
  DevBuf<double> d_rtop, d_ds;  // transit geometry workspaces
  DevBuf<double> d_rad;     // [cap][L] hydrostatic radii of the last run
  DevBuf<double> d_intens;  // [A][W] of the last single-walker run with want_intens
  bool lbl_eager = true;       // full extinction first (default); BARTRT_LBL=lazy: fused kernel
  DevBuf<double> d_tau;  // [W][L] of the last single-walker run
  DevBuf<int> d_last;
  PinBuf<double> h_pin;  // pinned staging
  // Host calls that wait for their result (bartrt_run_transit, bartrt_step_batch): the stream writes a sequence number
  // into a word of pinned host memory behind the kernels and the calling thread polls it -- 5-7 us sooner per call than
  // hipStreamSynchronize wakes up (measured in the chain service: 121 against 128 us per ten-walker call).
  // BARTRT_SYNC=stream: hipStreamSynchronize.
  PinBuf<unsigned int> h_flag;
  unsigned int *d_flag = nullptr;   // h_flag as the device addresses it
  unsigned int flag_seq = 0;
  bool sync_poll = true;
  void wait(hipStream_t st);
  // What two calls of the C ABI leave for a later run: bartrt_step_profiles_dev the walkers' overrides, for the NEXT
  // run (whichever it is); bartrt_prefetch_profiles_dev the batch of the run AFTER the next (prefetched preparation,
  // below).  Written by those two, taken -- and cleared -- in one place, the head of run().
  struct Pending {
    const double *over = nullptr;       // RunRequest::over, ::over_cloud
    bool over_cloud = false;
    const double *next_prof = nullptr;  // RunRequest::next_prof, ::next_n
    int next_n = 0;
  } pending;
  // diagnostics of the next RT launches: layers walked per (walker, kernel column)
  bool want_walked = false;
  DevBuf<int> d_walked;
  int walked_nwalkers = 0;
  size_t walked_restart_off = 0;   // the restarted-wave counts of the last record: d_walked + this, [walked_nwalkers]
  RtLaunchInfo walked_info{};
  // Where the latest launch's preparation left its layer records (bartrt_get_prep_records: a host-side copy for
  // tests).  folded: the RT kernel prepared its own walkers, the records lived in its LDS.  Forgotten when the
  // buffers behind it are regrown.
  struct PrepSeen {
    const double *coef = nullptr;
    const idx_t *idx = nullptr;
    const int *kstop = nullptr;
    const unsigned char *ok = nullptr;
    int n = 0;
    bool folded = false;
  } prep_seen;
  // timing of RT launches
  bool timing = false;
  int timing_stride = 1;     // events bracket every timing_stride-th launch (a pair of event
  long timing_seen = 0;      // records costs the stream ~5 us: bench.py samples)
  int ev_used = 0;
  // Prefetched preparation (bartrt_prefetch_profiles_dev): the caller names the NEXT batch's
  // profile buffer; the RT launch of the current call prepares that batch's layer records in
  // extra workgroups (RtArgs::nprep) into the second set of record buffers, and the next
  // call -- if it is for that buffer -- starts on its RT kernel directly.
  const double *pf_have_prof = nullptr;  // records of this batch are in buffer set pf_have_buf
  int pf_have_n = 0, pf_have_buf = 0;
  // ... built on this stream under these settings (everything of PrepArgs a setter can change)
  struct PrepSettings {
    double refradius, gsurf, cloudtop, scat_value, cloud_rup, cloud_rdown, cloud_ext;
    int has_cloud, scat_flag;
    bool operator==(const PrepSettings &o) const {
      return refradius == o.refradius && gsurf == o.gsurf && cloudtop == o.cloudtop && scat_value == o.scat_value &&
             cloud_rup == o.cloud_rup && cloud_rdown == o.cloud_rdown && cloud_ext == o.cloud_ext &&
             has_cloud == o.has_cloud && scat_flag == o.scat_flag;
    }
  };
  hipStream_t pf_have_stream = nullptr;
  PrepSettings pf_have_set{};
  int cap2 = 0;                          // walkers the second set holds
  DevBuf<char> d_slog;                   // `cut slant`: the single-wave kernels' event log (RtArgs::slog), in bytes
  // per-step converters, line-by-line extinction, contribution functions: owned, null until set up
  StepArgs *step = nullptr;
  Lbl *lbl = nullptr;
  CfState *cf = nullptr;

  ~Engine();
  void init(int argc, const char **argv);
  void setup(const TCfg &cfg_in, int shard_rank, int shard_n);
  // setup()'s stages, in the order it calls them (engine.hip)
  void read_settings();
  void generate_missing_opacity_file(int shard_rank);
  void read_atmosphere();
  void read_grid(OpacityHeader &oh, int shard_rank, int shard_n);
  void read_geometry();
  void open_device();
  void upload_table(const OpacityHeader &oh);
  void resample_cia(std::vector<double> &cia_planes, std::vector<double> &cia_temp);
  void upload_constants(const std::vector<double> &cia_planes, const std::vector<double> &cia_temp);
  void start_workspaces();
  void ensure_walkers(int n);
  void ensure_second_set();
  void ensure_pin(size_t bytes);
  // rq.prof -> rq.spec ([n][W]) on rq.stream, with what `pending` holds; records events when timing
  void run(const RunRequest &rq);
  // host buffers: prof [n][nprof] -> spec [n][nwave] (nwave the block's samples, or the whole grid's: the block goes
  // to its place in each row), flags to ok; without a flag array a walker that is not ok throws
  void run_host(const double *prof, int n, int nprof, double *spec, int nwave, unsigned char *ok);
  // run's chunked form and the parts of run_chunk (engine.hip)
  void run_chunks(const RunRequest &rq, int chunk, bool with_ext);
  void run_chunk(const RunRequest &rq);
  struct Prefetch;
  Prefetch plan_prefetch(bool pf_ok, const RunRequest &rq);
  PrepArgs prep_args(const RunRequest &rq, const RecordSet &records);
  RtArgs rt_args(const RunRequest &rq, const PrepArgs &pa, const Prefetch &pf, bool eclipse_rt, bool timed);

  // bartrt_comm_init: with a communicator the per-step path gathers the ranks' blocks itself (step.hip).  Owned and
  // destroyed by capi.hip (bartrt_comm_free, bartrt_free_memory, a re-bartrt_init) before the engine goes.
  Comm *comm = nullptr;
  unsigned long long ncollectives = 0;  // collectives this engine has issued (kept across bartrt_comm_free)

  QuantState *quant = nullptr;  // owned, null until a selection call (quant_release)
  SpecEnvState *specenv = nullptr;  // owned, null until a posterior_spectrum call (specenv_release)
};

}  // namespace bartrt
