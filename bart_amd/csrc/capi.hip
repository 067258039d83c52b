// extern "C" boundary of libbartrt.so (include/bartrt.h).
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../include/bartrt.h"
#include "comm.hpp"
#include "contrib.hpp"
#include "engine.hpp"
#include "hist.hpp"
#include "kde.hpp"
#include "lbl.hpp"
#include "quant.hpp"
#include "share.hpp"
#include "specenv.hpp"
#include "step.hpp"
#include "rt_launch.hpp"
#include "rtc.hpp"
#include "svc.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>

#include <sys/stat.h>
#include <unistd.h>

using namespace bartrt;

// One of two shapes per process: an engine of its own (g_eng), or -- `shareOpacity` as the chain service,
// svc.hpp -- a client slot (g_cli) of the engine some worker process of the run owns (g_svc set in that one).
static Engine *g_eng = nullptr;
static ChainService *g_svc = nullptr;
static svc::Client *g_cli = nullptr;
static thread_local std::string g_err;

static int fail(int code, const std::string &m) {
  g_err = m;
  return code;
}

// the one ladder from the exception in flight to the code and text the C ABI reports
struct Failure {
  int code;
  std::string msg;
};
static Failure what_failed() {
  try {
    throw;
  } catch (const IoError &e) { return {BARTRT_EIO, e.msg};
  } catch (const HipError &e) { return {BARTRT_ENODEV, std::string(e.what) + ": " + hipGetErrorString(e.e)};
  } catch (const svc::Error &e) { return {e.code, e.msg};
  } catch (const CommError &e) { return {e.code, e.msg};
  } catch (const std::exception &e) { return {BARTRT_EINVAL, e.what()};
  } catch (...) { return {BARTRT_EINVAL, "unknown error"}; }
}

template <class F>
static int guarded(F &&f) {
  try {
    return f();
  } catch (...) {
    const Failure w = what_failed();
    return fail(w.code, w.msg);
  }
}

// func: the entry point's own name, as the refusal to a service client states it
static int need_engine(const char *func) {
  if (g_eng) return BARTRT_OK;
  return g_cli ? fail(BARTRT_ENOTSUP, std::string(func) +
                                          ": this process is a client of the shareOpacity chain service (the engine lives in "
                                          "process " + std::to_string(g_cli->seg.hdr()->owner_pid.load()) +
                                          "); the reference module's eight calls and the plain getters are served -- "
                                          "BARTRT_SHARE_MODE=ipc (or off) gives every process its own engine")
               : fail(BARTRT_EINVAL, "engine not initialised: call bartrt_init first");
}
#define NEED_ENGINE() \
  if (int rc_ = need_engine(__func__)) return rc_
// the stream a device-buffer call runs on: the caller's, or (null) the engine's own
static hipStream_t stream_of(void *stream) { return stream ? (hipStream_t)stream : g_eng->stream; }
// the calls a service client answers itself
#define CLIENT_OR_ENGINE() \
  if (!g_eng && !g_cli) return fail(BARTRT_EINVAL, "engine not initialised: call bartrt_init first")

// ---- start-up: which shape this process takes ---------------------------
namespace {

struct InitArgs {
  std::string cfile;
  int shard_rank = 0, shard_n = 1, device = -1;
  bool no_service = false;
};

InitArgs parse_init_args(int argc, const char **argv) {
  InitArgs a;
  for (int i = 1; i < argc; i++) {
    const std::string s = argv[i];
    if ((s == "-c" || s == "--config_file") && i + 1 < argc) a.cfile = argv[++i];
    else if (s == "--shard" && i + 2 < argc) { a.shard_rank = std::atoi(argv[++i]); a.shard_n = std::atoi(argv[++i]); }
    else if (s == "--device" && i + 1 < argc) a.device = std::atoi(argv[++i]);
    else if (s == "--no-service") a.no_service = true;
  }
  return a;
}

// How many GPUs this process can see, WITHOUT a HIP call (a service client never makes one): the entries of
// HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES if set, else the KFD topology nodes that have SIMDs.  0: unknown.
int visible_gpu_count() {
  for (const char *name : {"HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"}) {
    const char *v = std::getenv(name);
    if (v && *v) {
      int n = 1;
      for (const char *c = v; *c; c++) n += *c == ',';
      return n;
    }
  }
  int n = 0;
  for (int node = 0; node < 256; node++) {
    char path[128];
    std::snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/properties", node);
    FILE *f = std::fopen(path, "r");
    if (!f) break;
    char key[64];
    long long val;
    while (std::fscanf(f, "%63s %lld", key, &val) == 2)
      if (std::strcmp(key, "simd_count") == 0) { n += val > 0; break; }
    std::fclose(f);
  }
  return n;
}

std::string service_key(const InitArgs &a) {
  struct stat st;
  if (stat(a.cfile.c_str(), &st) != 0) throw IoError{"cannot open configuration file '" + a.cfile + "'"};
  char rp[PATH_MAX];
  const std::string real = realpath(a.cfile.c_str(), rp) ? std::string(rp) : a.cfile;
  // (no HIP call here: a client never makes one -- the GPU is named by what selects it, resolved the way
  // Engine::setup resolves it: LOCAL_RANK modulo the visible devices, so that ten workers with ten LOCAL_RANKs on a
  // one-GPU node meet on one engine instead of electing themselves ten times)
  const char *lr = std::getenv("LOCAL_RANK"), *hv = std::getenv("HIP_VISIBLE_DEVICES"), *rv = std::getenv("ROCR_VISIBLE_DEVICES");
  int dev = a.device;
  if (dev < 0) {
    dev = lr ? std::atoi(lr) : 0;
    const int ndev = visible_gpu_count();
    if (ndev > 0) dev %= ndev;
  }
  // (the library's own id: workers on different builds of libbartrt do not share an engine)
  return real + "|" + std::to_string((long long)st.st_size) + "|" + std::to_string((long long)st.st_mtime) + "|" +
         std::to_string((long long)getuid()) + "|dev " + std::to_string(dev) + "|hip " + (hv ? hv : "") + "|rocr " + (rv ? rv : "") +
         "|shard " + std::to_string(a.shard_rank) + "/" + std::to_string(a.shard_n) + "|svc v3|" + bartrt_build_id();
}

void teardown(double wait_s) {
  if (g_cli) {
    g_cli->detach();
    g_cli->seg.unmap();
    delete g_cli;
    g_cli = nullptr;
  }
  if (g_svc) {
    ChainService *s = g_svc;
    g_svc = nullptr;
    s->shutdown(wait_s);
  }
  if (g_eng) {
    (void)hipDeviceSynchronize();
    comm_destroy(g_eng->comm);   // (before the engine's device state goes)
    g_eng->comm = nullptr;
    // (the contribution-function tables and workspaces belong to this engine and go with it)
    delete g_eng;
    g_eng = nullptr;
  }
}

// a process that exits without trm.free_memory(): the dispatcher thread must not outlive the HIP runtime
void at_exit() {
  try { teardown(0.0); } catch (...) {}
}

void start_service(int argc, const char **argv, const InitArgs &ia) {
  const std::string name = svc::hashed_name("bartrt_svc_", service_key(ia));
  svc::Segment seg;
  const bool owner = svc::elect(name, seg);
  auto *cli = new svc::Client;
  try {
    if (owner) {
      Engine *e = new Engine();
      e->share_mode = kShareOff;      // (the grid is this process's own: nobody maps it)
      try {
        e->init(argc, argv);
        g_svc = ChainService::start(std::move(seg), e);
      } catch (...) {
        const std::string why = what_failed().msg;
        svc::retire(seg, why.c_str());
        seg.unmap();
        delete e;
        throw;
      }
      static bool hooked = false;
      if (!hooked) { std::atexit(at_exit); hooked = true; }
      // this process's own calls go through a slot like everybody's (a second mapping of the segment)
      cli->seg.name = name;
      cli->seg.fd = shm_open(name.c_str(), O_RDWR | O_CLOEXEC, 0600);
      if (cli->seg.fd < 0) throw svc::Error{BARTRT_EIO, "shareOpacity: cannot reopen " + name};
      cli->seg.remap(g_svc->seg.hdr()->total_bytes);
      cli->attach(false);
      svc::open_for_clients(g_svc->seg);
    } else {
      cli->seg = seg;
      cli->attach(true);
    }
  } catch (...) {
    cli->detach();
    cli->seg.unmap();
    delete cli;
    if (g_svc) { ChainService *s = g_svc; g_svc = nullptr; s->shutdown(0.0); }
    throw;
  }
  g_cli = cli;
}

// a caller's options struct, maybe an older, shorter one: fields past its size read as zero.  False: size is not set
template <class T>
bool sized_copy(const T *opts, T *o) {
  std::memset(o, 0, sizeof *o);
  if (opts && opts->size < sizeof(opts->size)) return false;
  if (opts) std::memcpy(o, opts, opts->size < sizeof *o ? opts->size : sizeof *o);
  return true;
}

}  // namespace

extern "C" {

const char *bartrt_last_error(void) { return g_err.c_str(); }

int bartrt_init(int argc, const char **argv) {
  if (argc < 1 || !argv) return fail(BARTRT_EINVAL, "bartrt_init: empty argv");
  return guarded([&] {
    teardown(svc::env_num("BARTRT_SHARE_WAIT_S", 60.0));
    (void)slant_opt_guard();   // (a BARTRT_SLANT_OPT that is no guard is refused here, not at the first launch)
    const InitArgs ia = parse_init_args(argc, argv);
    if (ia.cfile.empty()) throw IoError{"transit_init: no '-c <configuration file>' in argv"};
    const int mode = resolve_share_mode(read_tcfg(ia.cfile), ia.no_service);
    if (mode == kShareService) {
      start_service(argc, argv, ia);
      return BARTRT_OK;
    }
    Engine *e = new Engine();
    e->share_mode = mode;
    try {
      e->init(argc, argv);
    } catch (...) {
      delete e;
      throw;
    }
    g_eng = e;
    return BARTRT_OK;
  });
}

int bartrt_free_memory(void) {
  return guarded([&] {
    // (the owner of a chain service keeps serving until the other workers have let go, BARTRT_SHARE_WAIT_S at most)
    teardown(svc::env_num("BARTRT_SHARE_WAIT_S", 60.0));
    return BARTRT_OK;
  });
}

int bartrt_get_no_samples(void) {
  CLIENT_OR_ENGINE();
  return g_cli ? g_cli->info.Wfull : g_eng->Wfull;
}

int bartrt_get_waveno_arr(double *out, int n) {
  CLIENT_OR_ENGINE();
  const std::vector<double> &wn = g_cli ? g_cli->info.wn_full : g_eng->wn_full;
  if (!out || n != (int)wn.size()) return fail(BARTRT_EINVAL, "get_waveno_arr: n must equal get_no_samples()");
  std::memcpy(out, wn.data(), sizeof(double) * n);
  return BARTRT_OK;
}

// (a service client keeps its setters to itself: they ride with each of ITS profiles, per walker of the batch)
int bartrt_set_radius(double r_km) {
  CLIENT_OR_ENGINE();
  if (!(r_km > 0)) return fail(BARTRT_EINVAL, "set_radius: radius must be positive");
  if (g_cli) g_cli->over[0] = r_km * 1e5;
  else g_eng->refradius = r_km * 1e5;
  return BARTRT_OK;
}

int bartrt_set_cloudtop(double logp) {
  CLIENT_OR_ENGINE();
  if (g_cli) { g_cli->over[1] = std::pow(10.0, logp) * 1e6; return BARTRT_OK; }
  g_eng->has_cloud = 1;
  g_eng->cloudtop = std::pow(10.0, logp) * 1e6;
  return BARTRT_OK;
}

int bartrt_set_scattering(int flag, double value) {
  CLIENT_OR_ENGINE();
  if (flag < 0 || flag > 2) return fail(BARTRT_EINVAL, "set_scattering: flag must be 0, 1 or 2");
  if (g_cli) { g_cli->scat_flag = flag; g_cli->over[2] = value; return BARTRT_OK; }
  g_eng->scat_flag = flag;
  g_eng->scat_value = value;
  return BARTRT_OK;
}

int bartrt_set_integ(int rule) {
  NEED_ENGINE();
  if (rule < 0 || rule > 2) return fail(BARTRT_EINVAL, "set_integ: rule must be 0 (transmittance), 1 (simpson) or 2 (trapz_tau)");
  g_eng->integ = rule;
  return BARTRT_OK;
}

int bartrt_set_cut(int slant) {
  NEED_ENGINE();
  if (slant != 0 && slant != 1) return fail(BARTRT_EINVAL, "set_cut: 0 (vertical) or 1 (slant)");
  g_eng->cut_slant = slant != 0;
  return BARTRT_OK;
}

int bartrt_set_slant_opt(double guard) {
  if (!set_slant_opt_guard(guard)) return fail(BARTRT_EINVAL, "set_slant_opt: 0 (off) or a power of two 2^-10 .. 1");
  return BARTRT_OK;
}

int bartrt_get_slant_opt(double *guard) {
  if (!guard) return fail(BARTRT_EINVAL, "get_slant_opt: null output pointer");
  return guarded([&] { *guard = slant_opt_guard(); return BARTRT_OK; });
}

int bartrt_parse_slant_opt(const char *text, double *guard) {
  double g = 0.0;
  if (!parse_slant_opt(text, &g)) return fail(BARTRT_EINVAL, "BARTRT_SLANT_OPT: an integer 0 .. 10 (0: off, n: guard 2^-n)");
  if (guard) *guard = g;
  return BARTRT_OK;
}

int bartrt_set_kernel_by(int local) {
  NEED_ENGINE();
  if (local != 0 && local != 1) return fail(BARTRT_EINVAL, "set_kernel_by: 0 (whole grid) or 1 (local block)");
  g_eng->kernel_by_local = local != 0;
  return BARTRT_OK;
}

int bartrt_get_kernel_by(int *local) {
  NEED_ENGINE();
  if (!local) return fail(BARTRT_EINVAL, "get_kernel_by: null output pointer");
  *local = g_eng->kernel_by_local ? 1 : 0;
  return BARTRT_OK;
}

int bartrt_get_cut(int *slant) {
  CLIENT_OR_ENGINE();
  if (!slant) return fail(BARTRT_EINVAL, "get_cut: null output pointer");
  *slant = g_cli ? g_cli->info.cut_slant : (g_eng->cut_slant ? 1 : 0);
  return BARTRT_OK;
}

int bartrt_get_cia_interp(int *spline) {
  CLIENT_OR_ENGINE();
  if (!spline) return fail(BARTRT_EINVAL, "get_cia_interp: null output pointer");
  *spline = g_cli ? g_cli->info.cia_spline : (g_eng->cia_spline ? 1 : 0);
  return BARTRT_OK;
}

int bartrt_get_share(int *shared, int *owner) {
  CLIENT_OR_ENGINE();
  if (g_cli) {
    if (shared) *shared = 1;
    if (owner) *owner = g_svc ? 1 : 0;
    return BARTRT_OK;
  }
  if (shared) *shared = g_eng->kappa_share ? 1 : 0;
  if (owner) *owner = (g_eng->kappa_share && g_eng->kappa_share->owner) ? 1 : 0;
  return BARTRT_OK;
}

int bartrt_prefetch_profiles_dev(const double *d_prof_next, int nwalkers) {
  NEED_ENGINE();
  if (nwalkers < 0 || (nwalkers > 0 && !d_prof_next)) return fail(BARTRT_EINVAL, "prefetch_profiles_dev: null buffer");
  g_eng->pending.next_prof = nwalkers > 0 ? d_prof_next : nullptr;
  g_eng->pending.next_n = nwalkers;
  return BARTRT_OK;
}

int bartrt_get_integ(int *rule) {
  CLIENT_OR_ENGINE();
  if (!rule) return fail(BARTRT_EINVAL, "get_integ: null output pointer");
  *rule = g_cli ? g_cli->info.integ : g_eng->integ;
  return BARTRT_OK;
}

int bartrt_get_service(int *mode, int *owner_pid, int *slot, int *nclients) {
  CLIENT_OR_ENGINE();
  if (g_cli) {
    const svc::Header *h = g_cli->seg.hdr();
    if (mode) *mode = g_svc ? 2 : 1;
    if (owner_pid) *owner_pid = h->owner_pid.load();
    if (slot) *slot = g_cli->slot;
    if (nclients) {
      int n = 0;
      for (int i = 0; i < h->maxclients; i++) n += g_cli->seg.slot(i)->pid.load() != 0;
      *nclients = n;
    }
  } else {
    if (mode) *mode = 0;
    if (owner_pid) *owner_pid = (int)getpid();
    if (slot) *slot = -1;
    if (nclients) *nclients = 0;
  }
  return BARTRT_OK;
}

int bartrt_get_service_stats(unsigned long long *nlaunches, unsigned long long *nprofiles, unsigned long long *nfull) {
  if (!g_cli) return fail(BARTRT_EINVAL, "get_service_stats: this process is not on a chain service");
  const svc::Header *h = g_cli->seg.hdr();
  if (nlaunches) *nlaunches = h->nbatches.load();
  if (nprofiles) *nprofiles = h->nserved.load();
  if (nfull) *nfull = h->nfull.load();
  return BARTRT_OK;
}

int bartrt_get_service_gathered(unsigned long long *ngathered) {
  if (!g_cli) return fail(BARTRT_EINVAL, "get_service_gathered: this process is not on a chain service");
  if (ngathered) *ngathered = g_cli->seg.hdr()->ngathered.load();
  return BARTRT_OK;
}

int bartrt_get_nlayers(void) { CLIENT_OR_ENGINE(); return g_cli ? g_cli->info.L : g_eng->L; }
int bartrt_get_nspecies(void) { CLIENT_OR_ENGINE(); return g_cli ? g_cli->info.S : g_eng->S; }
int bartrt_get_nprof(void) { CLIENT_OR_ENGINE(); return g_cli ? g_cli->info.nprof() : (g_eng->S + 1) * g_eng->L; }

int bartrt_get_local_range(int *lo, int *hi) {
  CLIENT_OR_ENGINE();
  if (lo) *lo = g_cli ? g_cli->info.lo : g_eng->lo;
  if (hi) *hi = g_cli ? g_cli->info.hi : g_eng->hi;
  return BARTRT_OK;
}

int bartrt_get_species(char *buf, int buflen) {
  CLIENT_OR_ENGINE();
  std::string s;
  if (g_cli) s = g_cli->info.species;
  else for (auto &n : g_eng->atm.species) s += (s.empty() ? "" : " ") + n;
  if (!buf || (int)s.size() + 1 > buflen) return fail(BARTRT_EINVAL, "get_species: buffer too small");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return BARTRT_OK;
}

int bartrt_get_pressure(double *out, int n) {
  CLIENT_OR_ENGINE();
  const std::vector<double> &press = g_cli ? g_cli->info.press : g_eng->atm.press;
  if (!out || n != (int)press.size()) return fail(BARTRT_EINVAL, "get_pressure: n must equal the layer count");
  std::memcpy(out, press.data(), sizeof(double) * n);
  return BARTRT_OK;
}

// trm.run_transit of a chain-service client: the profile goes into this process's slot, the dispatcher of the
// owning process launches it together with the other workers' (svc_core.hpp); a batch from ONE client is posted
// profile by profile (the batched callers own their engine: bart_amd.engine initialises with --no-service)
static int client_run(const double *prof, int nwalkers, int nprof, double *spec, int nwave, unsigned char *ok) {
  svc::Client *c = g_cli;
  if (!prof || !spec || nwalkers < 0) return fail(BARTRT_EINVAL, "run_transit: null buffer");
  if (nprof != c->info.nprof()) return fail(BARTRT_EINVAL, "run_transit: profile length must be (nspecies+1)*nlayers");
  const int Wl = c->info.Wl();
  if (nwave != Wl && nwave != c->info.Wfull)
    return fail(BARTRT_EINVAL, "run_transit: nwave must equal get_no_samples() (or the shard size)");
  return guarded([&] {
    const size_t off = nwave == Wl ? 0 : (size_t)c->info.lo;
    for (int w = 0; w < nwalkers; w++)
      c->call(prof + (size_t)w * nprof, spec + (size_t)w * nwave + off, ok ? ok + w : nullptr);
    return BARTRT_OK;
  });
}

int bartrt_run_transit_batch(const double *prof, int nwalkers, int nprof,
                             double *spec, int nwave, unsigned char *ok) {
  if (g_cli) return client_run(prof, nwalkers, nprof, spec, nwave, ok);
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!prof || !spec || nwalkers < 0) return fail(BARTRT_EINVAL, "run_transit: null buffer");
  if (nprof != (e->S + 1) * e->L)
    return fail(BARTRT_EINVAL, "run_transit: profile length must be (nspecies+1)*nlayers");
  const int Wl = e->W();
  if (nwave != Wl && nwave != e->Wfull)
    return fail(BARTRT_EINVAL, "run_transit: nwave must equal get_no_samples() (or the shard size)");
  return guarded([&] {
    e->run_host(prof, nwalkers, nprof, spec, nwave, ok);
    return BARTRT_OK;
  });
}

int bartrt_run_transit(const double *prof, int nprof, double *spec, int nwave) {
  return bartrt_run_transit_batch(prof, 1, nprof, spec, nwave, nullptr);
}

int bartrt_run_transit_batch_dev(const double *d_prof, int nwalkers, double *d_spec,
                                 unsigned char *d_ok, void *stream) {
  NEED_ENGINE();
  if (!d_prof || !d_spec || nwalkers < 0) return fail(BARTRT_EINVAL, "run_transit_batch_dev: null buffer");
  return guarded([&] {
    hipStream_t st = stream_of(stream);
    // device-buffer calls keep no profile: the optical-depth / intensity getters must not fall
    // back on an older host-buffer call's
    g_eng->forget_profiles();
    g_eng->run(RunRequest(d_prof, nwalkers, d_spec, d_ok, st));
    return BARTRT_OK;
  });
}

// the profile the optical-depth / intensity getters re-run: walker w of the latest host-buffer call
static const double *latest_profile(Engine *e, int walker, const char *who) {
  if (!e->last_prof)
    throw IoError{std::string(who) + ": no host-buffer spectrum has been computed since the engine's buffers were last "
                  "(re)built (device-buffer calls keep no profile: call bartrt_run_transit with the one in question)"};
  if (walker < 0 || walker >= e->last_n)
    throw IoError{std::string(who) + ": walker index outside the latest call's batch"};
  return e->last_prof + (size_t)walker * (e->S + 1) * e->L;
}

int bartrt_get_tau_of(int walker, double *tau, int *last, int nwave, int nlayers) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!tau || nwave != e->W() || nlayers != e->L)
    return fail(BARTRT_EINVAL, "get_tau: shape must be [local samples][nlayers]");
  return guarded([&] {
    // re-run that profile of the latest host-buffer call with the optical-depth output enabled
    RunRequest rq(latest_profile(e, walker, "get_tau"), 1, e->d_spec, e->rec[0].ok, e->stream);
    rq.want_tau = true;
    e->run(rq);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(tau, e->d_tau, sizeof(double) * (size_t)nwave * nlayers, hipMemcpyDeviceToHost));
    if (last) HIPCHK(hipMemcpy(last, e->d_last, sizeof(int) * (size_t)nwave, hipMemcpyDeviceToHost));
    return BARTRT_OK;
  });
}

int bartrt_get_atm_profile(double *prof, int nprof) {
  CLIENT_OR_ENGINE();
  if (g_cli) {
    if (!prof || nprof != g_cli->info.nprof()) return fail(BARTRT_EINVAL, "get_atm_profile: bad length");
    std::memcpy(prof, g_cli->info.atm_prof.data(), sizeof(double) * nprof);
    return BARTRT_OK;
  }
  Engine *e = g_eng;
  if (!prof || nprof != (e->S + 1) * e->L) return fail(BARTRT_EINVAL, "get_atm_profile: bad length");
  for (int l = 0; l < e->L; l++) {
    prof[l] = e->atm.temp[l];
    for (int s = 0; s < e->S; s++) prof[(size_t)(s + 1) * e->L + l] = e->atm.abund[(size_t)l * e->S + s];
  }
  return BARTRT_OK;
}

int bartrt_get_radius(double *rad, int nlayers) {
  NEED_ENGINE();
  if (!rad || nlayers != g_eng->L) return fail(BARTRT_EINVAL, "get_radius: bad length");
  return guarded([&] {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rad, g_eng->d_rad, sizeof(double) * nlayers, hipMemcpyDeviceToHost));
    return BARTRT_OK;
  });
}

int bartrt_get_prep_shape(int *nmol, int *ncs) {
  NEED_ENGINE();
  if (nmol) *nmol = g_eng->M;
  if (ncs) *ncs = g_eng->C;
  return BARTRT_OK;
}

int bartrt_get_prep_records(int walker, double *coef, long long *idx, int *kstop, unsigned char *ok) {
  NEED_ENGINE();
  Engine *e = g_eng;
  const Engine::PrepSeen &s = e->prep_seen;
  if (!s.coef || s.n <= 0) return fail(BARTRT_EINVAL, "get_prep_records: no launch has left layer records to read back");
  if (s.folded)
    return fail(BARTRT_EINVAL, "get_prep_records: the latest launch prepared its walkers inside the RT kernel; the "
                               "records lived in LDS and were never written out");
  if (walker < 0 || walker >= s.n)
    return fail(BARTRT_EINVAL, "get_prep_records: walker " + std::to_string(walker) + " is outside the latest batch of " +
                               std::to_string(s.n));
  return guarded([&] {
    static_assert(sizeof(idx_t) == sizeof(long long), "idx_t is the header's long long");
    const size_t L = (size_t)e->L, NC = (size_t)coef_stride(e->M, e->C), NI = (size_t)idx_stride(e->C);
    HIPCHK(hipDeviceSynchronize());
    if (coef) HIPCHK(hipMemcpy(coef, s.coef + (size_t)walker * L * NC, sizeof(double) * L * NC, hipMemcpyDeviceToHost));
    if (idx) HIPCHK(hipMemcpy(idx, s.idx + (size_t)walker * L * NI, sizeof(idx_t) * L * NI, hipMemcpyDeviceToHost));
    if (kstop) HIPCHK(hipMemcpy(kstop, s.kstop + walker, sizeof(int), hipMemcpyDeviceToHost));
    if (ok) HIPCHK(hipMemcpy(ok, s.ok + walker, 1, hipMemcpyDefault));   // (device memory, or the pinned staging buffer)
    return BARTRT_OK;
  });
}

int bartrt_get_chord_table(int walker, double *rtop, double *ds, double *raw) {
  NEED_ENGINE();
  Engine *e = g_eng;
  const Engine::PrepSeen &s = e->prep_seen;
  if (e->solution != 1) return fail(BARTRT_EINVAL, "get_chord_table: transit geometry only");
  if (!rtop || !ds) return fail(BARTRT_EINVAL, "get_chord_table: rtop and ds must not be null");
  // (the radii and the table live in the engine's own workspaces, regrown -- and prep_seen forgotten -- with the records)
  if (!s.coef || s.n <= 0 || !e->d_rtop.get() || !e->d_ds.get())
    return fail(BARTRT_EINVAL, "get_chord_table: no launch has left a chord table to read back");
  if (walker < 0 || walker >= s.n)
    return fail(BARTRT_EINVAL, "get_chord_table: walker " + std::to_string(walker) + " is outside the latest batch of " +
                               std::to_string(s.n));
  return guarded([&] {
    const int L = e->L;
    const size_t nraw = chord_table_size(L);
    std::vector<double> block(nraw);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(rtop, e->d_rtop.get() + (size_t)walker * L, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(block.data(), e->d_ds.get() + (size_t)walker * nraw, sizeof(double) * nraw, hipMemcpyDeviceToHost));
    // dense [k][j] (chord k, layer j; both from the top) from the row-tile order the kernels read; a row tile ends
    // with its diagonal tile (chord_table_fill), the steps behind it are never written
    for (int k = 0; k < L; k++)
      for (int j = 0; j < L; j++)
        ds[(size_t)k * L + j] = j < 16 * ((k >> 4) + 1) ? block[chord_table_index(L, k, j)] : 0.0;
    if (raw) std::memcpy(raw, block.data(), sizeof(double) * nraw);
    return BARTRT_OK;
  });
}

int bartrt_get_nangles(void) { CLIENT_OR_ENGINE(); return g_cli ? g_cli->info.A : g_eng->A; }

int bartrt_get_tau(double *tau, int *last, int nwave, int nlayers) {
  NEED_ENGINE();
  if (g_eng->last_prof && g_eng->last_n > 1)
    return fail(BARTRT_EINVAL, "get_tau: the latest call was a batch; name the walker with bartrt_get_tau_of()");
  return bartrt_get_tau_of(0, tau, last, nwave, nlayers);
}

int bartrt_get_angles(double *deg, int n) {
  CLIENT_OR_ENGINE();
  const std::vector<double> &ang = g_cli ? g_cli->info.angles : g_eng->angles;
  if (!deg || n != (int)ang.size()) return fail(BARTRT_EINVAL, "get_angles: bad length");
  std::memcpy(deg, ang.data(), sizeof(double) * n);
  return BARTRT_OK;
}

int bartrt_get_intensity(double *intens, int nangles, int nwave) {
  NEED_ENGINE();
  if (g_eng->last_prof && g_eng->last_n > 1)
    return fail(BARTRT_EINVAL, "get_intensity: the latest call was a batch; name the walker with bartrt_get_intensity_of()");
  return bartrt_get_intensity_of(0, intens, nangles, nwave);
}

int bartrt_get_intensity_of(int walker, double *intens, int nangles, int nwave) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (e->solution != 0) return fail(BARTRT_EINVAL, "get_intensity: eclipse geometry only");
  if (!intens || nangles != e->A || nwave != e->W()) return fail(BARTRT_EINVAL, "get_intensity: bad shape");
  return guarded([&] {
    RunRequest rq(latest_profile(e, walker, "get_intensity"), 1, e->d_spec, e->rec[0].ok, e->stream);
    rq.want_intens = true;
    e->run(rq);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(intens, e->d_intens, sizeof(double) * (size_t)nangles * nwave, hipMemcpyDeviceToHost));
    return BARTRT_OK;
  });
}

int bartrt_get_lbl_extinction(const double *prof, int nprof, double *ext, int nlayers, int nwave) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!e->lbl) return fail(BARTRT_EINVAL, "get_lbl_extinction: the engine was not set up with a line list");
  if (!prof || !ext || nprof != (e->S + 1) * e->L || nlayers != e->L || nwave != e->W())
    return fail(BARTRT_EINVAL, "get_lbl_extinction: bad shapes");
  return guarded([&] {
    e->ensure_walkers(1);
    HIPCHK(hipMemcpy(e->d_prof, prof, sizeof(double) * nprof, hipMemcpyHostToDevice));
    lbl_extinction(*e, e->d_prof, 1, e->stream);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(ext, e->lbl->d_ext, sizeof(double) * (size_t)nlayers * nwave, hipMemcpyDeviceToHost));
    return BARTRT_OK;
  });
}

int bartrt_lbl_owners(const double *prof, int nprof, unsigned char *owners, int nlayers, int ntile) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!e->lbl) return fail(BARTRT_EINVAL, "lbl_owners: the engine was not set up with a line list");
  if (!prof || !owners || nprof != (e->S + 1) * e->L || nlayers != e->L || ntile != (e->W() + 255) / 256)
    return fail(BARTRT_EINVAL, "lbl_owners: bad shapes");
  return guarded([&] {
    e->ensure_walkers(1);
    HIPCHK(hipMemcpy(e->d_prof, prof, sizeof(double) * nprof, hipMemcpyHostToDevice));
    lbl_owners(*e, e->d_prof, 1, owners);
    return BARTRT_OK;
  });
}

int bartrt_lbl_get_states(int *nstate, int *niso, int *ngroup, double *state, double *smax) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!e->lbl) return fail(BARTRT_EINVAL, "lbl_get_states: the engine was not set up with a line list");
  if (!nstate || !niso || !ngroup) return fail(BARTRT_EINVAL, "lbl_get_states: null argument");
  return guarded([&] {
    *nstate = (int)lbl_last_nstate(*e);
    *niso = e->lbl->dev.niso;
    *ngroup = e->lbl->dev.ngroup;
    // (lbl_get_states refuses an engine without a call and smax after bartrt_lbl_owners: std::invalid_argument, BARTRT_EINVAL)
    if (state || smax) lbl_get_states(*e, state, smax);
    return BARTRT_OK;
  });
}

int bartrt_voigt(const double *x, const double *y, double *k, long n) {
  if (n < 0 || (n > 0 && (!x || !y || !k))) return fail(BARTRT_EINVAL, "bartrt_voigt: bad arguments");
  return guarded([&] {
    lbl_voigt_probe(x, y, k, n);
    return BARTRT_OK;
  });
}

int bartrt_expint_e2(const double *x, double *out, long n) {
  if (n < 0 || (n > 0 && (!x || !out))) return fail(BARTRT_EINVAL, "bartrt_expint_e2: bad arguments");
  return guarded([&] {
    step_expint_e2_probe(x, out, n);
    return BARTRT_OK;
  });
}

int bartrt_rt_math(int which, const double *x, double *out, long n) {
  if (n < 0 || (n > 0 && (!x || !out))) return fail(BARTRT_EINVAL, "bartrt_rt_math: bad arguments");
  return guarded([&] {
    if (which == BARTRT_RT_MATH_EXP_RT_FMA3) {
      lbl_exp_rt_fma3_probe(x, out, n);
    } else if (!step_rt_math_probe(which, x, out, n)) {
      return fail(BARTRT_EINVAL, "bartrt_rt_math: unknown function selector");
    }
    return BARTRT_OK;
  });
}

int bartrt_timing_begin(void) { return bartrt_timing_begin_sampled(1); }

int bartrt_timing_begin_sampled(int stride) {
  NEED_ENGINE();
  if (stride < 1) return fail(BARTRT_EINVAL, "timing_begin_sampled: stride must be >= 1");
  return guarded([&] {
    // the events of the sampled launches are created here, outside the caller's timed region (created on
    // demand inside it they cost the first window of bench.py 10 us per step: 81 against 71)
    while (g_eng->ev.size() < 4096) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      g_eng->ev.push_back(e);
    }
    g_eng->timing = true;
    g_eng->timing_stride = stride;
    g_eng->timing_seen = 0;
    g_eng->ev_used = 0;
    return BARTRT_OK;
  });
}

int bartrt_timing_end(double *kernel_ms, int *nlaunch) {
  NEED_ENGINE();
  return guarded([&] {
    Engine *e = g_eng;
    double tot = 0.0;
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i + 1 < e->ev_used; i += 2) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
      tot += ms;
    }
    if (kernel_ms) *kernel_ms = tot;
    if (nlaunch) *nlaunch = e->ev_used / 2;
    e->timing = false;
    e->ev_used = 0;
    return BARTRT_OK;
  });
}

int bartrt_walked_begin(void) {
  NEED_ENGINE();
  g_eng->want_walked = true;
  g_eng->walked_nwalkers = 0;
  return BARTRT_OK;
}

int bartrt_walked_end(int *walked, int cap, int *nwalkers, int *ncolumns, int *wn_per_column,
                      char *kernel, int kernel_len) {
  NEED_ENGINE();
  return guarded([&] {
    Engine *e = g_eng;
    e->want_walked = false;
    HIPCHK(hipDeviceSynchronize());
    const int n = e->walked_nwalkers, nc = e->walked_info.ncolumns;
    if (nwalkers) *nwalkers = n;
    if (ncolumns) *ncolumns = nc;
    if (wn_per_column) *wn_per_column = e->walked_info.wn_per_column;
    if (kernel && kernel_len > 0) {
      std::snprintf(kernel, (size_t)kernel_len, "%s%s%s%s", e->walked_info.kernel, e->walked_info.rtc ? " [instantiated at run time]" : "",
                    e->walked_info.prep_folded ? " [prepares its own walkers]" : "",
                    e->walked_info.window ? " [table through a moving window]" : "");
    }
    if (walked && n > 0) {
      if ((size_t)cap < (size_t)n * nc) throw std::invalid_argument("walked_end: buffer too small");
      HIPCHK(hipMemcpy(walked, e->d_walked, sizeof(int) * (size_t)n * nc, hipMemcpyDeviceToHost));
    }
    return BARTRT_OK;
  });
}

int bartrt_walked_restarts(int *restarts, int cap, int *nwalkers) {
  NEED_ENGINE();
  return guarded([&] {
    Engine *e = g_eng;
    HIPCHK(hipDeviceSynchronize());
    const int n = e->walked_nwalkers;
    if (nwalkers) *nwalkers = n;
    if (restarts && n > 0) {
      if (cap < n) throw std::invalid_argument("walked_restarts: buffer too small");
      HIPCHK(hipMemcpy(restarts, e->d_walked.get() + e->walked_restart_off, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return BARTRT_OK;
  });
}

int bartrt_get_rtc_stats(int *available, int *compiled, int *from_disk, int *failed, double *compile_seconds) {
  const RtcStats st = rtc_stats();
  if (available) *available = rtc_available() ? 1 : 0;
  if (compiled) *compiled = st.compiled;
  if (from_disk) *from_disk = st.from_disk;
  if (failed) *failed = st.failed;
  if (compile_seconds) *compile_seconds = st.compile_seconds;
  return BARTRT_OK;
}

int bartrt_rtc_compile(const char *expr, int ilp, long *code_bytes) {
  if (!expr) return fail(BARTRT_EINVAL, "rtc_compile: null expression");
  std::string why;
  const long n = rtc_compile_only(expr, ilp != 0, why);
  if (code_bytes) *code_bytes = n;
  return n < 0 ? fail(BARTRT_ENOTSUP, why) : BARTRT_OK;
}

const char *bartrt_kernel_choice(int nmol, long columns) {
  return kernel_variant_name(slant_simpson_choice(nmol, columns < 0 ? 0 : columns).variant);
}

int bartrt_slant_thresholds(double toomuch, const double *invmu, int n, double *thr, double *thrb) {
  if (!invmu || n < 1 || n > kMaxAngles) return fail(BARTRT_EINVAL, "slant_thresholds: 1 .. 16 rays");
  RtArgs r{};
  r.A = n;
  r.toomuch = toomuch;
  for (int a = 0; a < n; a++) r.invmu[a] = invmu[a];
  slant_thresholds(r);
  for (int a = 0; a < n; a++) {
    if (thr) thr[a] = r.thr[a];
    if (thrb) thrb[a] = r.thrb[a];
  }
  return BARTRT_OK;
}

int bartrt_get_ray_args(int n, double *invmu, double *wgt, double *wq, double *thr, double *thrb, int *order, int *sq) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (e->solution != 0) return fail(BARTRT_EINVAL, "get_ray_args: eclipse geometry only");
  if (n != e->A) return fail(BARTRT_EINVAL, "get_ray_args: bad length");
  RtArgs r = e->rt;
  r.toomuch = e->toomuch;
  slant_thresholds(r);
  for (int a = 0; a < n; a++) {
    if (invmu) invmu[a] = r.invmu[a];
    if (wgt) wgt[a] = r.wgt[a];
    if (wq) wq[a] = r.wq[a];
    if (thr) thr[a] = r.thr[a];
    if (thrb) thrb[a] = r.thrb[a];
  }
  // the specialised kernels' order: the same call their launcher makes, on a copy whose drank carries the slots' origin
  RtArgs b = r;
  for (int a = 0; a < n; a++) b.drank[a] = a;
  const bool is_sq = order_angles_for_square(b);
  for (int a = 0; a < n; a++)
    if (order) order[a] = b.drank[a];
  if (sq) *sq = is_sq ? 1 : 0;
  return BARTRT_OK;
}

int bartrt_kernel_inventory(char *buf, int buflen) {
  std::string s;
  if (!kernel_inventory(s)) return fail(BARTRT_ENOTSUP, "kernel_inventory: a unit lists " + s + " and the ahead-of-time lookup does not reach it");
  if (!buf || buflen < 0 || s.size() + 1 > (size_t)buflen)
    return fail(BARTRT_EINVAL, "kernel_inventory: buffer too small, " + std::to_string(s.size() + 1) + " bytes needed");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return BARTRT_OK;
}

double bartrt_algorithmic_bytes(int nwalkers) {
  if (!g_eng) return 0.0;
  Engine *e = g_eng;
  const double L = e->L, W = e->W(), M = e->M, C = e->C, S = e->S;
  return nwalkers * (2.0 * L * W * M * 8.0 + 2.0 * L * W * C * 8.0 + (S + 1) * L * 8.0 + W * 8.0);
}

// ---- contribution functions / band transmittance (contrib.hip) ----------
// what the batched post-processing does not serve: line-by-line engines, and -- the calls that combine the ranks'
// sums themselves (blocks false) -- sharded engines without a communicator, the rule the step follows (a service
// client never gets here: NEED_ENGINE answers it with BARTRT_ENOTSUP)
static int cf_unsupported(const Engine *e, const char *who, bool blocks) {
  if (e->lbl) return fail(BARTRT_ENOTSUP, std::string(who) + ": line-by-line engines are not supported");
  if (!blocks && !e->comm && (e->lo != 0 || e->hi != e->Wfull))
    return fail(BARTRT_ENOTSUP, std::string(who) + ": sharded engines are not supported without a communicator "
                                                   "(bartrt_comm_init; or bartrt_cf_setup_block / _partials_dev / _combine_dev)");
  return BARTRT_OK;
}

static int cf_setup_any(int nfilters, const int *idx0, const int *npts, const double *resp, const char *who, bool blocks) {
  if (int rc = cf_unsupported(g_eng, who, blocks)) return rc;
  if (nfilters < 1 || !idx0 || !npts || !resp) return fail(BARTRT_EINVAL, std::string(who) + ": null buffer or no filters");
  return guarded([&] {
    cf_setup(*g_eng, nfilters, idx0, npts, resp);
    return BARTRT_OK;
  });
}

int bartrt_cf_setup(int nfilters, const int *idx0, const int *npts, const double *resp) {
  NEED_ENGINE();
  return cf_setup_any(nfilters, idx0, npts, resp, "cf_setup", false);
}

int bartrt_cf_setup_block(int nfilters, const int *idx0, const int *npts, const double *resp) {
  NEED_ENGINE();
  return cf_setup_any(nfilters, idx0, npts, resp, "cf_setup_block", true);
}

// The one gate of the batch calls: a request (contrib.hpp) is checked here, once, and cf_run trusts it.  In order: the
// engine, its limits, the step's setup (parameter calls), kind and geometry, the CF setup, the parameter count, the
// buffers, the stated profile length (nprof; -1 where the ABI takes none).  rq.stream arrives as the caller's handle.
static int cf_call(const char *who, CfRequest rq, int nprof = -1) {
  if (int rc = need_engine(("bartrt_" + std::string(who)).c_str())) return rc;
  Engine *e = g_eng;
  const std::string pre = std::string(who) + ": ";
  if (int rc = cf_unsupported(e, who, rq.partials)) return rc;
  if (rq.from_params && !e->step) return fail(BARTRT_EINVAL, pre + "call bartrt_step_setup first");
  if (rq.kind != BARTRT_CF_CONTRIB && rq.kind != BARTRT_CF_TRANSMIT)
    return fail(BARTRT_EINVAL, pre + "kind must be BARTRT_CF_CONTRIB or BARTRT_CF_TRANSMIT");
  if (rq.kind == BARTRT_CF_CONTRIB && e->solution != 0)
    return fail(BARTRT_ENOTSUP, pre + "contribution functions need the eclipse geometry (transmittance serves transit)");
  if (cf_nfilters(*e) == 0) return fail(BARTRT_EINVAL, pre + "call bartrt_cf_setup first");
  if (rq.from_params && rq.npars != step_npars(*e))
    return fail(BARTRT_EINVAL, pre + "npars must be nPT + (radius, cloud top, scattering parameters "
                                     "declared with step_set_extras) + nmolfit");
  if (!rq.in || !rq.out || rq.n < 0) return fail(BARTRT_EINVAL, pre + "null buffer");
  if (nprof >= 0 && nprof != (e->S + 1) * e->L) return fail(BARTRT_EINVAL, pre + "profile length must be (nspecies+1)*nlayers");
  rq.stream = stream_of(rq.stream);
  return guarded([&] {
    cf_run(*e, rq);
    return BARTRT_OK;
  });
}

// the entry points' arguments as requests: profiles (with overrides or null) and parameter rows; stream null with
// `host`, which runs on the engine's own
static CfRequest cf_profiles(const double *prof, int n, const double *over, int kind, double *out, double *full,
                             unsigned char *ok, bool host, void *stream) {
  CfRequest rq;
  rq.n = n; rq.kind = kind; rq.in = prof; rq.over = over; rq.out = out; rq.full = full; rq.ok = ok;
  rq.host = host; rq.stream = (hipStream_t)stream;
  return rq;
}

static CfRequest cf_params(const double *params, int n, int npars, int kind, double *band, double *full, int *status,
                           bool host, void *stream) {
  CfRequest rq;
  rq.n = n; rq.kind = kind; rq.in = params; rq.from_params = true; rq.npars = npars; rq.out = band; rq.full = full;
  rq.status = status; rq.host = host; rq.stream = (hipStream_t)stream;
  return rq;
}

int bartrt_cf_batch(const double *prof, int nwalkers, int nprof, int kind, double *band, double *full, unsigned char *ok) {
  return cf_call("cf_batch", cf_profiles(prof, nwalkers, nullptr, kind, band, full, ok, true, nullptr), nprof);
}

int bartrt_cf_batch_dev(const double *d_prof, int nwalkers, int kind, double *d_band, double *d_full,
                        unsigned char *d_ok, void *stream) {
  return cf_call("cf_batch_dev", cf_profiles(d_prof, nwalkers, nullptr, kind, d_band, d_full, d_ok, false, stream));
}

int bartrt_cf_batch_over(const double *prof, int nwalkers, int nprof, const double *over, int kind, double *band,
                         double *full, unsigned char *ok) {
  return cf_call("cf_batch_over", cf_profiles(prof, nwalkers, over, kind, band, full, ok, true, nullptr), nprof);
}

int bartrt_cf_batch_over_dev(const double *d_prof, int nwalkers, const double *d_over, int kind, double *d_band,
                             double *d_full, unsigned char *d_ok, void *stream) {
  return cf_call("cf_batch_over_dev", cf_profiles(d_prof, nwalkers, d_over, kind, d_band, d_full, d_ok, false, stream));
}

int bartrt_cf_partials_dev(const double *d_prof, int nwalkers, int kind, const double *d_over, double *d_part,
                           double *d_full, unsigned char *d_ok, void *stream) {
  CfRequest rq = cf_profiles(d_prof, nwalkers, d_over, kind, d_part, d_full, d_ok, false, stream);
  rq.partials = true;   // (this block's sums, no collective: served on a sharded engine without a communicator too)
  return cf_call("cf_partials_dev", rq);
}

// (not a request: the ranks' slots in, no walker runs; the engine limits and the setup as above)
int bartrt_cf_combine_dev(const double *d_slots, int nranks, int nwalkers, const unsigned char *d_ok, double *d_band,
                          void *stream) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (int rc = cf_unsupported(e, "cf_combine_dev", true)) return rc;
  if (cf_nfilters(*e) == 0) return fail(BARTRT_EINVAL, "cf_combine_dev: call bartrt_cf_setup first");
  if (!d_slots || !d_band || nwalkers < 0) return fail(BARTRT_EINVAL, "cf_combine_dev: null buffer");
  return guarded([&] {
    cf_combine_dev(*e, d_slots, nranks, nwalkers, d_ok, d_band, stream_of(stream));
    return BARTRT_OK;
  });
}

// (diagnostics, host code only: the shapes and the latest launch are filled in first, so a call with every buffer
// null is the shape query; the copies need a chunk and a walker inside it)
int bartrt_cf_get_records(int walker, bartrt_cf_records *r) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!r) return fail(BARTRT_EINVAL, "cf_get_records: null argument");
  if (cf_nfilters(*e) == 0) return fail(BARTRT_EINVAL, "cf_get_records: call bartrt_cf_setup first");
  const CfSeen s = cf_seen(*e);
  r->nlayers = e->L; r->nmol = e->M; r->ncs = e->C; r->transit = e->solution == 1; r->nwalkers = s.n; r->nfilters = s.nf; r->ntiles = s.ntiles;
  r->nent = s.nent; r->kernel = s.form; r->lds_bytes = (long long)s.lds; r->kstop = 0; r->ok = 0;
  if (!r->coef && !r->idx && !r->rdlp && !r->rtop && !r->ds && !r->tile_ptr && !r->wt && !r->f_ptr && !r->f_ent && !r->trapz &&
      walker < 0)
    return BARTRT_OK;
  // (cf_get_records refuses a missing chunk and a walker outside it: std::invalid_argument, BARTRT_EINVAL)
  if (e->solution != 1 && (r->rtop || r->ds)) return fail(BARTRT_EINVAL, "cf_get_records: rtop and ds are the transit geometry's");
  return guarded([&] {
    static_assert(sizeof(idx_t) == sizeof(long long), "idx_t is the header's long long");
    const int L = e->L;
    std::vector<double> block(r->ds ? chord_table_size(L) : 0);
    unsigned char ok = 0;
    CfReadback o;
    o.coef = r->coef; o.idx = r->idx; o.kstop = &r->kstop; o.ok = &ok; o.rdlp = r->rdlp; o.rtop = r->rtop;
    o.ds = r->ds ? block.data() : nullptr;
    o.tile_ptr = r->tile_ptr; o.f_ptr = r->f_ptr; o.f_ent = r->f_ent; o.wt = r->wt; o.trapz = r->trapz;
    cf_get_records(*e, walker, o);
    r->ok = ok;
    // dense [k][j] from the row-tile order the kernels read, as bartrt_get_chord_table reports it
    if (r->ds)
      for (int k = 0; k < L; k++)
        for (int j = 0; j < L; j++)
          r->ds[(size_t)k * L + j] = j < 16 * ((k >> 4) + 1) ? block[chord_table_index(L, k, j)] : 0.0;
    return BARTRT_OK;
  });
}

int bartrt_cf_params(const double *params, int nwalkers, int npars, int kind, double *band, double *full, int *status) {
  return cf_call("cf_params", cf_params(params, nwalkers, npars, kind, band, full, status, true, nullptr));
}

int bartrt_cf_params_dev(const double *d_params, int nwalkers, int npars, int kind, double *d_band, double *d_full,
                         int *d_status, void *stream) {
  return cf_call("cf_params_dev", cf_params(d_params, nwalkers, npars, kind, d_band, d_full, d_status, false, stream));
}

// ---- order statistics and posterior envelopes (quant.hip) ----------------
// the arguments both forms of the selection refuse, each named
static int colselect_check(const char *who, const void *x, long nrows, int ncols, long ld, int nranks,
                           const long *ranks, const void *out) {
  const std::string pre = std::string(who) + ": ";
  if (!x || !ranks || !out) return fail(BARTRT_EINVAL, pre + "null buffer");
  if (nranks < 1 || nranks > quant::kMaxRanks)
    return fail(BARTRT_EINVAL, pre + "nranks = " + std::to_string(nranks) + " is outside 1.." + std::to_string(quant::kMaxRanks));
  if (nrows < 1 || nrows > kQuantMaxRows)
    return fail(BARTRT_EINVAL, pre + "nrows = " + std::to_string(nrows) + " is outside 1.." + std::to_string(kQuantMaxRows));
  if (ncols < 0 || ncols > kQuantMaxCols)
    return fail(BARTRT_EINVAL, pre + "ncols = " + std::to_string(ncols) + " is outside 0.." + std::to_string(kQuantMaxCols));
  if (ld < ncols) return fail(BARTRT_EINVAL, pre + "ld = " + std::to_string(ld) + " is below ncols = " + std::to_string(ncols));
  for (int r = 0; r < nranks; r++)
    if (ranks[r] < 0)
      return fail(BARTRT_EINVAL, pre + "ranks[" + std::to_string(r) + "] = " + std::to_string(ranks[r]) + " is negative");
  return BARTRT_OK;
}

int bartrt_colselect_dev(const double *d_x, long nrows, int ncols, long ld, const unsigned char *d_ok, int nranks,
                         const long *ranks, double *d_out, void *stream) {
  NEED_ENGINE();
  if (int rc = colselect_check("colselect_dev", d_x, nrows, ncols, ld, nranks, ranks, d_out)) return rc;
  return guarded([&] {
    colselect_dev(*g_eng, d_x, nrows, ncols, ld, d_ok, nranks, ranks, d_out, stream_of(stream));
    return BARTRT_OK;
  });
}

int bartrt_colselect(const double *x, long nrows, int ncols, long ld, const unsigned char *ok, int nranks,
                     const long *ranks, double *out) {
  NEED_ENGINE();
  if (int rc = colselect_check("colselect", x, nrows, ncols, ld, nranks, ranks, out)) return rc;
  long count = nrows;
  if (ok) {
    count = 0;
    for (long r = 0; r < nrows; r++) count += ok[r] != 0;
  }
  if (count == 0) return fail(BARTRT_EINVAL, "colselect: ok leaves no row");
  for (int r = 0; r < nranks; r++)
    if (ranks[r] >= count)
      return fail(BARTRT_EINVAL, "colselect: ranks[" + std::to_string(r) + "] = " + std::to_string(ranks[r]) +
                                     " is not below the " + std::to_string(count) + " rows that count");
  if (ncols == 0) return BARTRT_OK;
  return guarded([&] {
    colselect_host(*g_eng, x, nrows, ncols, ld, ok, nranks, ranks, out);
    return BARTRT_OK;
  });
}

int bartrt_colselect_slab(long *rows) {
  if (!rows) return fail(BARTRT_EINVAL, "colselect_slab: null buffer");
  *rows = g_eng ? colselect_slab(*g_eng) : kQuantSlabRows;
  return BARTRT_OK;
}

int bartrt_colselect_set_slab(long rows) {
  NEED_ENGINE();
  return guarded([&] {
    colselect_set_slab(*g_eng, rows);
    return BARTRT_OK;
  });
}

int bartrt_posterior_tp(const double *params, long nsamples, int npars, int nq, const double *q, double *env,
                        int *status, long *ngood) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!e->step) return fail(BARTRT_EINVAL, "posterior_tp: call bartrt_step_setup first");
  if (!params || !q || !env || !status || !ngood) return fail(BARTRT_EINVAL, "posterior_tp: null buffer");
  if (nsamples < 1 || nsamples > kQuantMaxRows)
    return fail(BARTRT_EINVAL, "posterior_tp: nsamples = " + std::to_string(nsamples) + " is outside 1.." + std::to_string(kQuantMaxRows));
  if (nq < 1 || nq > quant::kMaxPercents)
    return fail(BARTRT_EINVAL, "posterior_tp: nq = " + std::to_string(nq) + " is outside 1.." + std::to_string(quant::kMaxPercents));
  for (int i = 0; i < nq; i++)
    if (!(q[i] >= 0.0 && q[i] <= 100.0))
      return fail(BARTRT_EINVAL, "posterior_tp: q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is outside 0..100");
  if (npars != step_npars(*e))
    return fail(BARTRT_EINVAL, "posterior_tp: npars must be nPT + (radius, cloud top, scattering parameters declared with "
                               "step_set_extras) + nmolfit");
  return guarded([&] {
    posterior_tp(*e, params, nsamples, npars, nq, q, env, status, ngood);
    return BARTRT_OK;
  });
}

int bartrt_posterior_set_chunk(long rows) {
  NEED_ENGINE();
  return guarded([&] {
    posterior_set_chunk(*g_eng, rows);
    return BARTRT_OK;
  });
}

int bartrt_posterior_tp_order(int nq, int nlayers, long *ranks, double *order) {
  NEED_ENGINE();
  if (!ranks || !order) return fail(BARTRT_EINVAL, "posterior_tp_order: null buffer");
  if (!posterior_tp_order(*g_eng, nq, nlayers, ranks, order))
    return fail(BARTRT_EINVAL, "posterior_tp_order: no envelope of that shape (no bartrt_posterior_tp yet, no accepted "
                               "sample, or another nq / nlayers)");
  return BARTRT_OK;
}

int bartrt_percentile_rule(long n, double q, long *lo, long *hi, double *w) {
  if (!lo || !hi || !w) return fail(BARTRT_EINVAL, "percentile_rule: null buffer");
  if (n < 1) return fail(BARTRT_EINVAL, "percentile_rule: n = " + std::to_string(n) + " is below 1");
  if (!(q >= 0.0 && q <= 100.0)) return fail(BARTRT_EINVAL, "percentile_rule: q = " + std::to_string(q) + " is outside 0..100");
  quant::percentile_rule(n, q, lo, hi, w);
  return BARTRT_OK;
}

int bartrt_percentile_lerp(const double *a, const double *b, double w, double *out, long n) {
  if (!a || !b || !out) return fail(BARTRT_EINVAL, "percentile_lerp: null buffer");
  for (long i = 0; i < n; i++) out[i] = quant::interpolate(a[i], b[i], w);
  return BARTRT_OK;
}

// ---- posterior spectra (specenv.hip, specenv_core.hpp) -------------------
// the display rule's arguments, each refusal named
static int display_check(const std::string &pre, int r, long stride) {
  if (r < 0 || r > specenv::kMaxRadius)
    return fail(BARTRT_EINVAL, pre + "r = " + std::to_string(r) + " is outside 0.." + std::to_string(specenv::kMaxRadius));
  if (stride < 1) return fail(BARTRT_EINVAL, pre + "stride = " + std::to_string(stride) + " is below 1");
  return BARTRT_OK;
}

// what the posterior spectrum calls need of the engine: the whole grid on this GPU, and the step
static int spectrum_needs(const Engine *e, const std::string &pre) {
  if (e->lo != 0 || e->hi != e->Wfull)
    return fail(BARTRT_ENOTSUP, pre + "wavenumber-sharded engines are not supported: the spectra are not whole on this GPU "
                                      "(an engine on the whole grid serves the call)");
  if (!e->step) return fail(BARTRT_EINVAL, pre + "call bartrt_step_setup first");
  return BARTRT_OK;
}

int bartrt_spectrum_display_dev(const double *d_spec, long nrows, int nwave, long ld, const double *d_sflux, double rprs,
                                int r, const double *half, long stride, double *d_out, long ldo, void *stream) {
  NEED_ENGINE();
  const std::string pre = "spectrum_display_dev: ";
  if (int rc = display_check(pre, r, stride)) return rc;
  if (!d_spec || !d_out || !half) return fail(BARTRT_EINVAL, pre + "null buffer (d_spec, half, d_out)");
  if (nrows < 1) return fail(BARTRT_EINVAL, pre + "nrows = " + std::to_string(nrows) + " is below 1");
  if (nwave < 1) return fail(BARTRT_EINVAL, pre + "nwave = " + std::to_string(nwave) + " is below 1");
  if (ld < nwave) return fail(BARTRT_EINVAL, pre + "ld = " + std::to_string(ld) + " is below nwave = " + std::to_string(nwave));
  const long Wk = specenv::kept_columns(nwave, stride);
  if (ldo < Wk) return fail(BARTRT_EINVAL, pre + "ldo = " + std::to_string(ldo) + " is below Wk = " + std::to_string(Wk));
  return guarded([&] {
    spectrum_display_dev(d_spec, nrows, nwave, ld, d_sflux, rprs, r, half, stride, d_out, ldo, stream_of(stream));
    return BARTRT_OK;
  });
}

int bartrt_spectrum_display_tile(int r, long stride, long *cols) {
  if (!cols) return fail(BARTRT_EINVAL, "spectrum_display_tile: null buffer");
  if (int rc = display_check("spectrum_display_tile: ", r, stride)) return rc;
  *cols = spec_tile_out(r, stride);
  return BARTRT_OK;
}

int bartrt_posterior_spectrum(const double *params, long nsamples, int npars, int nq, const double *q, const double *sflux,
                              int r, const double *half, long stride, double *env_spec, double *env_band, int *status,
                              long *ngood) {
  NEED_ENGINE();
  Engine *e = g_eng;
  const std::string pre = "posterior_spectrum: ";
  if (int rc = spectrum_needs(e, pre)) return rc;
  if (int rc = display_check(pre, r, stride)) return rc;
  if (!params || !q || !half || !env_spec || !env_band || !status || !ngood) return fail(BARTRT_EINVAL, pre + "null buffer");
  if (nsamples < 1 || nsamples > kQuantMaxRows)
    return fail(BARTRT_EINVAL, pre + "nsamples = " + std::to_string(nsamples) + " is outside 1.." + std::to_string(kQuantMaxRows));
  if (nq < 1 || nq > quant::kMaxPercents)
    return fail(BARTRT_EINVAL, pre + "nq = " + std::to_string(nq) + " is outside 1.." + std::to_string(quant::kMaxPercents));
  for (int i = 0; i < nq; i++)
    if (!(q[i] >= 0.0 && q[i] <= 100.0))
      return fail(BARTRT_EINVAL, pre + "q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is outside 0..100");
  if (npars != step_npars(*e))
    return fail(BARTRT_EINVAL, pre + "npars must be nPT + (radius, cloud top, scattering parameters declared with "
                                     "step_set_extras) + nmolfit");
  if (specenv::kept_columns(e->Wfull, stride) > kQuantMaxCols)
    return fail(BARTRT_EINVAL, pre + "more than " + std::to_string(kQuantMaxCols) + " kept columns: raise stride");
  return guarded([&] {
    posterior_spectrum(*e, params, nsamples, npars, nq, q, sflux, r, half, stride, env_spec, env_band, status, ngood);
    return BARTRT_OK;
  });
}

int bartrt_posterior_spectrum_shape(long stride, long *Wk, int *F) {
  NEED_ENGINE();
  if (int rc = spectrum_needs(g_eng, "posterior_spectrum_shape: ")) return rc;
  if (int rc = display_check("posterior_spectrum_shape: ", 0, stride)) return rc;
  if (!Wk || !F) return fail(BARTRT_EINVAL, "posterior_spectrum_shape: null buffer");
  *Wk = specenv::kept_columns(g_eng->Wfull, stride);
  *F = g_eng->step->nfilters;
  return BARTRT_OK;
}

int bartrt_posterior_spectrum_order(int nq, long Wk, int F, long *ranks, double *order_spec, double *order_band) {
  NEED_ENGINE();
  if (!ranks || !order_spec || !order_band) return fail(BARTRT_EINVAL, "posterior_spectrum_order: null buffer");
  if (!posterior_spectrum_order(*g_eng, nq, Wk, F, ranks, order_spec, order_band))
    return fail(BARTRT_EINVAL, "posterior_spectrum_order: no envelope of that shape (no bartrt_posterior_spectrum yet, no "
                               "accepted sample, or another nq / Wk / F)");
  return BARTRT_OK;
}

int bartrt_posterior_spectrum_rows(long row0, long nrows, double *out) {
  NEED_ENGINE();
  if (!out) return fail(BARTRT_EINVAL, "posterior_spectrum_rows: null buffer");
  return guarded([&] {
    if (!posterior_spectrum_rows(*g_eng, row0, nrows, out))
      return fail(BARTRT_EINVAL, "posterior_spectrum_rows: rows " + std::to_string(row0) + " .. " + std::to_string(row0 + nrows) +
                                     " are outside the latest sample matrix (no bartrt_posterior_spectrum yet, or another range)");
    return BARTRT_OK;
  });
}

// ---- posterior marginals (hist.hip, hist_core.hpp): no engine ------------
// the selection both calls take, each refusal named
static int marginals_check_sel(const std::string &pre, const void *x, long nrows, long ld, int nsel, const int *cols) {
  if (!x || !cols) return fail(BARTRT_EINVAL, pre + "null buffer (x, cols)");
  if (nsel < 1 || nsel > hist::kMaxSel)
    return fail(BARTRT_EINVAL, pre + "nsel = " + std::to_string(nsel) + " is outside 1.." + std::to_string(hist::kMaxSel));
  if (nrows < 1 || nrows > kHistMaxRows)
    return fail(BARTRT_EINVAL, pre + "nrows = " + std::to_string(nrows) + " is outside 1.." + std::to_string(kHistMaxRows));
  if (ld < 1) return fail(BARTRT_EINVAL, pre + "ld = " + std::to_string(ld) + " is below 1");
  for (int s = 0; s < nsel; s++)
    if (cols[s] < 0 || cols[s] >= ld)
      return fail(BARTRT_EINVAL, pre + "cols[" + std::to_string(s) + "] = " + std::to_string(cols[s]) +
                                     " is outside 0..ld - 1 (ld = " + std::to_string(ld) + ")");
  return BARTRT_OK;
}

static int marginals_check(const char *who, const void *x, long nrows, long ld, int nsel, const int *cols, int nbins,
                           const double *edges, const void *h1, const void *out, const void *h2) {
  const std::string pre = std::string(who) + ": ";
  if (!edges || !h1 || !out) return fail(BARTRT_EINVAL, pre + "null buffer (edges, h1, out)");
  if (int rc = marginals_check_sel(pre, x, nrows, ld, nsel, cols)) return rc;
  if (nbins < 1 || nbins > hist::kMaxBins)
    return fail(BARTRT_EINVAL, pre + "nbins = " + std::to_string(nbins) + " is outside 1.." + std::to_string(hist::kMaxBins));
  if (h2 && nbins > hist::kMaxPairBins)
    return fail(BARTRT_EINVAL, pre + "nbins = " + std::to_string(nbins) + " is above " + std::to_string(hist::kMaxPairBins) +
                                   ", the most with pairs (h2 not NULL)");
  for (int s = 0; s < nsel; s++) {
    const int bad = hist::bad_edge(edges + (size_t)s * (nbins + 1), nbins);
    if (bad >= 0)
      return fail(BARTRT_EINVAL, pre + "edges[" + std::to_string(s) + "][" + std::to_string(bad) +
                                     "] is not finite or not above the edge before it");
  }
  return BARTRT_OK;
}

int bartrt_marginals_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols,
                         int nbins, const double *edges, unsigned long long *d_h1, unsigned long long *d_out,
                         unsigned long long *d_h2, void *stream) {
  if (int rc = marginals_check("marginals_dev", d_x, nrows, ld, nsel, cols, nbins, edges, d_h1, d_out, d_h2)) return rc;
  return guarded([&] {
    marginals_dev(d_x, nrows, ld, d_ok, nsel, cols, nbins, edges, d_h1, d_out, d_h2, (hipStream_t)stream);
    return BARTRT_OK;
  });
}

int bartrt_marginals(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int nbins,
                     const double *edges, unsigned long long *h1, unsigned long long *out, unsigned long long *h2) {
  if (int rc = marginals_check("marginals", x, nrows, ld, nsel, cols, nbins, edges, h1, out, h2)) return rc;
  return guarded([&] {
    marginals_host(x, nrows, ld, ok, nsel, cols, nbins, edges, h1, out, h2);
    return BARTRT_OK;
  });
}

int bartrt_marginals_range_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols,
                               double *d_lohi, unsigned long long *d_nfinite, void *stream) {
  if (!d_lohi || !d_nfinite) return fail(BARTRT_EINVAL, "marginals_range_dev: null buffer (lohi, nfinite)");
  if (int rc = marginals_check_sel("marginals_range_dev: ", d_x, nrows, ld, nsel, cols)) return rc;
  return guarded([&] {
    marginals_range_dev(d_x, nrows, ld, d_ok, nsel, cols, d_lohi, d_nfinite, (hipStream_t)stream);
    return BARTRT_OK;
  });
}

int bartrt_marginals_range(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols,
                           double *lohi, unsigned long long *nfinite) {
  if (!lohi || !nfinite) return fail(BARTRT_EINVAL, "marginals_range: null buffer (lohi, nfinite)");
  if (int rc = marginals_check_sel("marginals_range: ", x, nrows, ld, nsel, cols)) return rc;
  return guarded([&] {
    marginals_range_host(x, nrows, ld, ok, nsel, cols, lohi, nfinite);
    return BARTRT_OK;
  });
}

int bartrt_marginals_slab(long *rows) {
  if (!rows) return fail(BARTRT_EINVAL, "marginals_slab: null buffer");
  *rows = marginals_slab();
  return BARTRT_OK;
}

int bartrt_marginals_set_slab(long rows) {
  return guarded([&] {
    marginals_set_slab(rows);
    return BARTRT_OK;
  });
}

int bartrt_marginals_chunk(long *rows) {
  if (!rows) return fail(BARTRT_EINVAL, "marginals_chunk: null buffer");
  *rows = marginals_chunk();
  return BARTRT_OK;
}

int bartrt_marginals_set_chunk(long rows) {
  return guarded([&] {
    marginals_set_chunk(rows);
    return BARTRT_OK;
  });
}

int bartrt_hpd(const unsigned long long *counts, int nbins, double p, unsigned char *mask, unsigned long long *threshold,
               unsigned long long *included, int *nruns) {
  if (!counts || !mask || !threshold || !included || !nruns) return fail(BARTRT_EINVAL, "hpd: null buffer");
  if (nbins < 1) return fail(BARTRT_EINVAL, "hpd: nbins = " + std::to_string(nbins) + " is below 1");
  if (!(p > 0.0 && p <= 1.0)) return fail(BARTRT_EINVAL, "hpd: p = " + std::to_string(p) + " is outside (0, 1]");
  return guarded([&] {
    uint64_t thr = 0, inc = 0;
    hist::hpd(reinterpret_cast<const uint64_t *>(counts), nbins, p, mask, &thr, &inc, nruns);
    *threshold = thr;
    *included = inc;
    return BARTRT_OK;
  });
}

// ---- posterior kernel density estimates (kde.hip, kde_core.hpp): no engine ----
static int kde_check(const char *who, const void *x, long nrows, long ld, int nsel, const int *cols, int ngrid,
                     const double *grid, int rule, double factor, const void *pdf, const void *stat, const void *nonfinite) {
  const std::string pre = std::string(who) + ": ";
  if (!grid || !pdf || !stat || !nonfinite) return fail(BARTRT_EINVAL, pre + "null buffer (grid, pdf, stat, nonfinite)");
  if (int rc = marginals_check_sel(pre, x, nrows, ld, nsel, cols)) return rc;
  if (ngrid < 1 || ngrid > kde::kMaxGrid)
    return fail(BARTRT_EINVAL, pre + "ngrid = " + std::to_string(ngrid) + " is outside 1.." + std::to_string(kde::kMaxGrid));
  for (int s = 0; s < nsel; s++)
    for (int j = 0; j < ngrid; j++)
      if (!hist::is_finite(grid[(size_t)s * ngrid + j]))
        return fail(BARTRT_EINVAL, pre + "grid[" + std::to_string(s) + "][" + std::to_string(j) + "] is not finite");
  if (rule != kde::kScott && rule != kde::kSilverman && rule != kde::kFactor)
    return fail(BARTRT_EINVAL, pre + "bw_rule = " + std::to_string(rule) + " is none of 0 (Scott), 1 (Silverman), 2 (bw_factor)");
  if (rule == kde::kFactor && !(factor > 0.0 && hist::is_finite(factor)))
    return fail(BARTRT_EINVAL, pre + "bw_factor = " + std::to_string(factor) + " is not a finite number above 0");
  return BARTRT_OK;
}

int bartrt_kde_dev(const double *d_x, long nrows, long ld, const unsigned char *d_ok, int nsel, const int *cols, int ngrid,
                   const double *grid, int bw_rule, double bw_factor, double *d_pdf, double *d_stat,
                   unsigned long long *d_nonfinite, void *stream) {
  if (int rc = kde_check("kde_dev", d_x, nrows, ld, nsel, cols, ngrid, grid, bw_rule, bw_factor, d_pdf, d_stat, d_nonfinite))
    return rc;
  return guarded([&] {
    kde_dev(d_x, nrows, ld, d_ok, nsel, cols, ngrid, grid, bw_rule, bw_factor, d_pdf, d_stat, d_nonfinite, (hipStream_t)stream);
    return BARTRT_OK;
  });
}

int bartrt_kde(const double *x, long nrows, long ld, const unsigned char *ok, int nsel, const int *cols, int ngrid,
               const double *grid, int bw_rule, double bw_factor, double *pdf, double *stat, unsigned long long *nonfinite) {
  if (int rc = kde_check("kde", x, nrows, ld, nsel, cols, ngrid, grid, bw_rule, bw_factor, pdf, stat, nonfinite)) return rc;
  return guarded([&] {
    kde_host(x, nrows, ld, ok, nsel, cols, ngrid, grid, bw_rule, bw_factor, pdf, stat, nonfinite);
    return BARTRT_OK;
  });
}

int bartrt_kde_chunk(long *rows) {
  if (!rows) return fail(BARTRT_EINVAL, "kde_chunk: null buffer");
  *rows = kde_chunk();
  return BARTRT_OK;
}

int bartrt_kde_set_chunk(long rows) {
  return guarded([&] {
    kde_set_chunk(rows);
    return BARTRT_OK;
  });
}

int bartrt_kde_tile(long *rows) {
  if (!rows) return fail(BARTRT_EINVAL, "kde_tile: null buffer");
  *rows = kde::kKdeTileRows;
  return BARTRT_OK;
}

int bartrt_hpd_pdf(const double *pdf, int n, double p, unsigned char *mask, double *threshold, double *included, int *nruns) {
  if (!pdf || !mask || !threshold || !included || !nruns) return fail(BARTRT_EINVAL, "hpd_pdf: null buffer");
  if (n < 1) return fail(BARTRT_EINVAL, "hpd_pdf: n = " + std::to_string(n) + " is below 1");
  if (!(p > 0.0 && p <= 1.0)) return fail(BARTRT_EINVAL, "hpd_pdf: p = " + std::to_string(p) + " is outside (0, 1]");
  return guarded([&] {
    kde::hpd_pdf(pdf, n, p, mask, threshold, included, nruns);
    return BARTRT_OK;
  });
}

// ---- per-step converters (step.hip) ------------------------------------
int bartrt_step_setup(const double *ptargs5, int tint_thorngren, int pttype,
                      double tmin, double tmax,
                      const double *abund, int nmolfit, const int *imol,
                      int nfilters, const int *idx0, const int *npts,
                      const double *nifilter, const double *istarfl,
                      double rprs, int solution) {
  NEED_ENGINE();
  return guarded([&] {
    step_setup(*g_eng, ptargs5, tint_thorngren, pttype, tmin, tmax, abund, nmolfit, imol,
               nfilters, idx0, npts, nifilter, istarfl, rprs, solution);
    return BARTRT_OK;
  });
}

int bartrt_step_set_ebalance(int on, double e_in, double e_fac) {
  NEED_ENGINE();
  return guarded([&] {
    step_set_ebalance(*g_eng, on, e_in, e_fac);
    return BARTRT_OK;
  });
}

int bartrt_step_profiles_dev(const double *d_params, int nwalkers, int npars,
                             double *d_prof, int *d_status, void *stream) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "step_profiles: call bartrt_step_setup first");
  if (!d_params || !d_prof || !d_status) return fail(BARTRT_EINVAL, "step_profiles: null buffer");
  return guarded([&] {
    hipStream_t st = stream_of(stream);
    step_profiles_dev(*g_eng, d_params, nwalkers, npars, d_prof, d_status, st);
    return BARTRT_OK;
  });
}

int bartrt_step_bandflux_dev(const double *d_spec_full, int nwalkers, int *d_status,
                             double *d_bandflux, void *stream) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "step_bandflux: call bartrt_step_setup first");
  if (!d_spec_full || !d_bandflux || !d_status) return fail(BARTRT_EINVAL, "step_bandflux: null buffer");
  return guarded([&] {
    hipStream_t st = stream_of(stream);
    step_bandflux_dev(*g_eng, d_spec_full, nwalkers, d_status, d_bandflux, st);
    return BARTRT_OK;
  });
}

int bartrt_step_batch_dev(const double *d_params, int nwalkers, int npars,
                          double *d_bandflux, int *d_status, double *d_spec,
                          void *stream) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "step_batch: call bartrt_step_setup first");
  return guarded([&] {
    hipStream_t st = stream_of(stream);
    step_run_dev(*g_eng, d_params, nwalkers, npars, d_bandflux, d_status, d_spec, st);
    return BARTRT_OK;
  });
}

int bartrt_step_set_extras(int nrad, int ncloud, int nray) {
  NEED_ENGINE();
  return guarded([&] {
    step_set_extras(*g_eng, nrad, ncloud, nray);
    return BARTRT_OK;
  });
}

int bartrt_step_set_carry(int on) {
  NEED_ENGINE();
  return guarded([&] {
    step_set_carry(*g_eng, on);
    return BARTRT_OK;
  });
}

int bartrt_step_batch(const double *params, int nwalkers, int npars,
                      double *bandflux, int *status) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "step_batch: call bartrt_step_setup first");
  if (!params || !bandflux || nwalkers < 0) return fail(BARTRT_EINVAL, "step_batch: null buffer");
  return guarded([&] {
    step_run_host(*g_eng, params, nwalkers, npars, bandflux, status);
    return BARTRT_OK;
  });
}

// ---- retrievals: the problem arguments of the four calls below travel on as one value (step.hpp) ----
static bool stated(const RetrievalProblem &p) { return p.pmin && p.pmax && p.stepsize && p.data && p.uncert; }
static int null_buffer(const char *who) { return fail(BARTRT_EINVAL, std::string(who) + ": null buffer"); }

int bartrt_mcmc_run(int nchains, int npars, long nsteps, const double *params, const double *pmin,
                    const double *pmax, const double *stepsize, int ndata, const double *data,
                    const double *uncert, int snooker, unsigned long long seed, double *chain,
                    double *chisq, long *naccept, long *nbad) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "mcmc_run: call bartrt_step_setup first");
  const RetrievalProblem p{npars, ndata, 0, pmin, pmax, stepsize, data, uncert};
  if (!stated(p) || !params || !chain || !chisq) return null_buffer("mcmc_run");
  return guarded([&] {
    mcmc_run(*g_eng, p, nchains, nsteps, params, snooker, seed, chain, chisq, naccept, nbad);
    return BARTRT_OK;
  });
}

// the options of the two resident calls (the priors of the single call travel in its problem)
static McmcOpts mcmc_opts_of(const bartrt_mcmc_opts &o) {
  McmcOpts m;
  m.snooker = o.snooker;
  m.seed = o.seed;
  m.thin = o.thin ? o.thin : 1;
  m.block = o.block ? o.block : 256;
  m.progress = o.progress; m.progress_user = o.progress_user;
  m.burnin = o.burnin; m.grcheck = o.grcheck; m.grthreshold = o.grthreshold; m.grexit = o.grexit;
  m.grstat = o.grstat; m.grwhen = o.grwhen; m.ngr = o.ngr; m.ngr_out = o.ngr_out;
  m.first = o.first; m.start = o.start; m.done = o.done;
  m.walk = o.walk;
  m.esstarget = o.esstarget; m.essexit = o.essexit; m.maxlag = o.maxlag; m.essstat = o.essstat; m.esstau = o.esstau;
  return m;
}

int bartrt_mcmc_run_resident(int nchains, int npars, long nsteps, const double *params, const double *pmin,
                             const double *pmax, const double *stepsize, int ndata, const double *data,
                             const double *uncert, const bartrt_mcmc_opts *opts, double *chain, double *chisq,
                             double *models, long *naccept, long *nbad) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "mcmc_run_resident: call bartrt_step_setup first");
  RetrievalProblem p{npars, ndata, 0, pmin, pmax, stepsize, data, uncert};
  if (!stated(p) || !params || !chain || !chisq) return null_buffer("mcmc_run_resident");
  bartrt_mcmc_opts o;
  if (!sized_copy(opts, &o)) return fail(BARTRT_EINVAL, "mcmc_run_resident: set opts->size");
  p.prior = o.prior; p.priorlow = o.priorlow; p.priorup = o.priorup;
  const McmcOpts m = mcmc_opts_of(o);
  return guarded([&] {
    mcmc_run_resident(*g_eng, p, nchains, nsteps, params, m, chain, chisq, models, naccept, nbad);
    return BARTRT_OK;
  });
}

int bartrt_mcmc_run_resident_groups(int ngroups, const bartrt_mcmc_group *groups, int nchains, int npars, long nsteps,
                                    int ndata, const bartrt_mcmc_opts *opts, double *chain, double *chisq,
                                    double *models, long *naccept, long *nbad, int *converged_at) {
  NEED_ENGINE();
  const std::string who = "mcmc_run_resident_groups";
  if (!g_eng->step) return fail(BARTRT_EINVAL, who + ": call bartrt_step_setup first");
  if (ngroups < 1) return fail(BARTRT_EINVAL, who + ": ngroups = " + std::to_string(ngroups) + ": at least one group");
  if (!groups || !chain || !chisq) return null_buffer(who.c_str());
  bartrt_mcmc_opts o;
  if (!sized_copy(opts, &o)) return fail(BARTRT_EINVAL, who + ": set opts->size");
  if (o.seed || o.prior || o.priorlow || o.priorup || o.start)
    return fail(BARTRT_EINVAL, who + ": opts->seed, prior, priorlow, priorup and start are not read here: every group "
                                     "carries its own (bartrt_mcmc_group)");
  // the array's stride is the caller's sizeof(bartrt_mcmc_group): every element says the same
  const unsigned long stride = groups[0].size;
  std::vector<McmcGroup> gs((size_t)ngroups);
  for (int g = 0; g < ngroups; g++) {
    const auto *at = reinterpret_cast<const bartrt_mcmc_group *>(reinterpret_cast<const char *>(groups) + (size_t)g * stride);
    bartrt_mcmc_group c;
    if (stride < sizeof(c.size) || at->size != stride || !sized_copy(at, &c))
      return fail(BARTRT_EINVAL, who + ": group " + std::to_string(g) + ": set size = sizeof(bartrt_mcmc_group) in every group");
    gs[g].p = RetrievalProblem{npars, ndata, 0, c.pmin, c.pmax, c.stepsize, c.data, c.uncert, c.prior, c.priorlow, c.priorup};
    gs[g].params = c.params; gs[g].seed = c.seed; gs[g].start = c.start;
    if (!stated(gs[g].p) || (!c.params && !c.start)) return null_buffer((who + ": group " + std::to_string(g)).c_str());
  }
  const McmcOpts m = mcmc_opts_of(o);
  return guarded([&] {
    mcmc_run_resident_groups(*g_eng, ngroups, gs.data(), nchains, nsteps, m, chain, chisq, models, naccept, nbad,
                             converged_at);
    return BARTRT_OK;
  });
}

int bartrt_mcmc_gr(const double *chain, int nchains, long nkept, int npars, const double *stepsize, long r0, long r1,
                   double threshold, double *psrf, double *triples, int *converged) {
  if (!chain || !stepsize || !psrf || !triples || !converged) return null_buffer("bartrt_mcmc_gr");
  return guarded([&] {
    mcmc_gr_probe(chain, nchains, nkept, npars, stepsize, r0, r1, threshold, psrf, triples, converged);
    return BARTRT_OK;
  });
}

int bartrt_mcmc_ess(const double *chain, int nchains, long nkept, int npars, const double *stepsize, long r0, long r1,
                    long maxlag, double esstarget, double *tau, double *ess, int *truncated, double *acf,
                    int *reached) {
  if (!chain || !stepsize || !tau || !ess || !truncated || !reached) return null_buffer("bartrt_mcmc_ess");
  return guarded([&] {
    mcmc_ess_probe(chain, nchains, nkept, npars, stepsize, r0, r1, maxlag, esstarget, tau, ess, truncated, acf,
                   reached);
    return BARTRT_OK;
  });
}

int bartrt_mcmc_draws(unsigned long long seed, unsigned long long t, int nchains, int npars, double *out) {
  if (!out) return fail(BARTRT_EINVAL, "bartrt_mcmc_draws: null buffer");
  return guarded([&] {
    mcmc_draws_probe(seed, t, nchains, npars, out);
    return BARTRT_OK;
  });
}

int bartrt_grid_run(int nrows, int npars, long nsteps, const double *params, const double *pmin, const double *pmax,
                    const double *stepsize, const bartrt_grid_opts *opts, long *nbad) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "grid_run: call bartrt_step_setup first");
  if (!params || !pmin || !pmax || !stepsize) return null_buffer("grid_run");
  bartrt_grid_opts o;
  if (!opts || !sized_copy(opts, &o)) return fail(BARTRT_EINVAL, "grid_run: opts with opts->size set and a sink");
  GridOpts g;
  g.seed = o.seed; g.chunk = o.chunk; g.first = o.first;
  g.spectra = o.spectra != 0; g.f32 = o.f32 != 0;
  g.sink = o.sink; g.user = o.user;
  return guarded([&] {
    const int rc = grid_run(*g_eng, nrows, npars, nsteps, params, pmin, pmax, stepsize, g, nbad);
    return rc ? fail(rc, "grid_run: the sink stopped the run with " + std::to_string(rc)) : BARTRT_OK;
  });
}

int bartrt_grid_draws(unsigned long long seed, unsigned long long t, int nrows, int npars, const double *params,
                      const double *pmin, const double *pmax, const double *stepsize, double *out) {
  if (!params || !pmin || !pmax || !stepsize || !out) return null_buffer("bartrt_grid_draws");
  return guarded([&] {
    grid_draws_probe(seed, t, nrows, npars, params, pmin, pmax, stepsize, out);
    return BARTRT_OK;
  });
}

// the caller's bartrt_fit_opts as FitOpts, zero fields read as the defaults, and its priors into the problem
static bool fit_opts_of(const bartrt_fit_opts *opts, FitOpts &m, RetrievalProblem &p) {
  bartrt_fit_opts o;
  if (!sized_copy(opts, &o)) return false;
  if (o.maxiter) m.maxiter = o.maxiter < 0 ? 0 : o.maxiter;
  if (o.nrungs) m.nrungs = o.nrungs;
  if (o.check) m.check = o.check;
  if (o.fdstep != 0) m.fdstep = o.fdstep;
  if (o.ftol != 0) m.ftol = o.ftol;
  if (o.xtol != 0) m.xtol = o.xtol;
  if (o.lambda0 != 0) m.lambda0 = o.lambda0;
  p.prior = o.prior; p.priorlow = o.priorlow; p.priorup = o.priorup;
  m.trace = o.trace;
  return true;
}

int bartrt_fit(int nstarts, int npars, const double *starts, const double *pmin, const double *pmax,
               const double *stepsize, int ndata, const double *data, const double *uncert,
               const bartrt_fit_opts *opts, double *best, double *chisq, int *status, long *niter, long *nbad) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "fit: call bartrt_step_setup first");
  RetrievalProblem p{npars, ndata, 0, pmin, pmax, stepsize, data, uncert};
  if (!stated(p) || !starts || !best || !chisq) return null_buffer("fit");
  FitOpts m;
  if (!fit_opts_of(opts, m, p)) return fail(BARTRT_EINVAL, "fit: set opts->size");
  return guarded([&] {
    fit_run(*g_eng, p, nstarts, starts, m, best, chisq, status, niter, nbad);
    return BARTRT_OK;
  });
}

int bartrt_fit_probe(int nstarts, int npars, const double *pmin, const double *pmax, const double *stepsize,
                     int ndata, const double *data, const double *uncert, const bartrt_fit_opts *opts,
                     const double *x, const double *lambda, double *D, const double *cur, const double *pband,
                     const int *pstatus, double *trial, int *valid) {
  RetrievalProblem p{npars, ndata, 0, pmin, pmax, stepsize, data, uncert};
  if (!stated(p) || !x || !lambda || !D || !cur || !pband || !pstatus || !trial || !valid)
    return null_buffer("bartrt_fit_probe");
  FitOpts m;
  if (!fit_opts_of(opts, m, p)) return fail(BARTRT_EINVAL, "bartrt_fit_probe: set opts->size");
  return guarded([&] {
    fit_probe(p, nstarts, m, x, lambda, D, cur, pband, pstatus, trial, valid);
    return BARTRT_OK;
  });
}

// ---- the ranks' communicator (comm.hip) -----------------------------------
int bartrt_comm_get_unique_id(void *id) {
  // (needs no engine: rank 0 may ask before its bartrt_init; a chain-service client gets what every non-reference
  // call gives it)
  if (g_cli && !g_eng)
    return fail(BARTRT_ENOTSUP, "comm_get_unique_id: this process is a client of the shareOpacity chain service");
  if (!id) return fail(BARTRT_EINVAL, "comm_get_unique_id: null buffer");
  return guarded([&] {
    comm_get_unique_id(id);
    return BARTRT_OK;
  });
}

int bartrt_comm_init(const void *id, int rank, int nranks) {
  NEED_ENGINE();
  Engine *e = g_eng;
  if (!id) return fail(BARTRT_EINVAL, "comm_init: null id");
  if (e->comm) return fail(BARTRT_EINVAL, "comm_init: a communicator is already attached (bartrt_comm_free first)");
  // the engine's block must be block `rank` of `nranks` under the engine's split (an unsharded engine is 0 / 1)
  if (nranks < 1 || rank < 0 || rank >= nranks || nranks > e->Wfull ||
      e->lo != (int)((long long)e->Wfull * rank / nranks) || e->hi != (int)((long long)e->Wfull * (rank + 1) / nranks))
    return fail(BARTRT_EINVAL, "comm_init: rank " + std::to_string(rank) + " of " + std::to_string(nranks) +
                                   " is not this engine's --shard (it holds samples [" + std::to_string(e->lo) + ", " +
                                   std::to_string(e->hi) + ") of " + std::to_string(e->Wfull) + ")");
  return guarded([&] {
    e->comm = comm_create(e->device, id, rank, nranks);
    return BARTRT_OK;
  });
}

int bartrt_comm_free(void) {
  NEED_ENGINE();
  return guarded([&] {
    Comm *c = g_eng->comm;
    g_eng->comm = nullptr;
    comm_destroy(c);
    return BARTRT_OK;
  });
}

int bartrt_get_comm(int *rank, int *nranks, unsigned long long *ncollectives) {
  NEED_ENGINE();
  const Comm *c = g_eng->comm;
  if (rank) *rank = c ? c->rank : -1;
  if (nranks) *nranks = c ? c->nranks : 0;
  if (ncollectives) *ncollectives = g_eng->ncollectives;
  return BARTRT_OK;
}

int bartrt_step_bandflux_blocks_dev(const double *d_blocks, int nranks, int nwalkers, int *d_status,
                                    double *d_bandflux, void *stream) {
  NEED_ENGINE();
  if (!g_eng->step) return fail(BARTRT_EINVAL, "step_bandflux_blocks: call bartrt_step_setup first");
  if (!d_blocks || !d_bandflux || !d_status || nwalkers < 0)
    return fail(BARTRT_EINVAL, "step_bandflux_blocks: null buffer");
  return guarded([&] {
    hipStream_t st = stream_of(stream);
    step_bandflux_blocks_dev(*g_eng, d_blocks, nranks, nwalkers, d_status, d_bandflux, st);
    return BARTRT_OK;
  });
}

}  // extern "C"
