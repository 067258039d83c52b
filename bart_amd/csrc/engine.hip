// Host-side engine: reads the transit inputs, places the tables in HBM and
// drives the kernels.  One engine per process (one process per GPU).
#include "engine.hpp"
#include "lbl.hpp"
#include "lds.hpp"
#include "prep.hpp"
#include "contrib.hpp"
#include "quant.hpp"
#include "share.hpp"
#include "specenv.hpp"
#include "step.hpp"
#include "svc.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include <sys/stat.h>
#include <unistd.h>

namespace bartrt {

EngineStream::~EngineStream() {
  for (auto e : ev) (void)hipEventDestroy(e);
  if (stream) (void)hipStreamDestroy(stream);
}

// (the buffers are members: they free themselves after this body, before the events and the stream of the base)
Engine::~Engine() {
  delete step;
  delete lbl;
  cf_release(*this);
  quant_release(*this);
  specenv_release(*this);
  if (kappa_share) { kappa_share->release(); kappa_share = nullptr; }
}

void Engine::init(int argc, const char **argv) {
  std::string cfile;
  int shard_rank = 0, shard_n = 1;
  bool no_service = false;
  device = -1;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    if ((a == "-c" || a == "--config_file") && i + 1 < argc) cfile = argv[++i];
    else if (a == "--shard" && i + 2 < argc) { shard_rank = std::atoi(argv[++i]); shard_n = std::atoi(argv[++i]); }
    else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (a == "--no-service") no_service = true;
  }
  if (cfile.empty()) throw IoError{"transit_init: no '-c <configuration file>' in argv"};
  if (shard_n < 1 || shard_rank < 0 || shard_rank >= shard_n)
    throw IoError{"transit_init: bad --shard rank/nranks"};
  const TCfg c = read_tcfg(cfile);
  if (share_mode < 0) share_mode = resolve_share_mode(c, no_service);
  if (share_mode == kShareService) share_mode = kShareIpc;   // (an engine of its own was asked for: capi.hip runs the service)
  setup(c, shard_rank, shard_n);
}

int resolve_share_mode(const TCfg &cfg, bool no_service) {
  auto truthy = [](const std::string &v) { return v != "0" && v != "no" && v != "false" && v != "False"; };
  // (makeTransit writes the key bare -- code/makecfg.py:106-107: present without a value means yes)
  bool on = false;
  if (auto it = cfg.find("shareOpacity"); it != cfg.end()) on = truthy(it->second);
  if (const char *e = std::getenv("BARTRT_SHARE_OPACITY")) if (*e) on = std::string(e) != "0";
  int mode = kShareService;
  // Fewer than five worker processes: separate HIP contexts overlap their one-walker launches and beat the service's
  // one batched launch (measured, headline grid: three processes 63 against 85 us per call, four 86 / 90, five 89 / 92
  // per call but 2.8e4 / 5.4e4 spectra/s) -- when the launcher says how many chains there are (BARTRT_NCHAINS, set by
  // bart_amd.BARTfunc from the communicator's size; else the MPI world size of the spawned workers) and nothing names a
  // mode, such runs take the IPC reading.
  for (const char *name : {"BARTRT_NCHAINS", "OMPI_COMM_WORLD_SIZE", "PMI_SIZE", "MV2_COMM_WORLD_SIZE"}) {
    const char *e = std::getenv(name);
    if (e && *e) {
      const int n = std::atoi(e);
      if (n >= 1 && n < 5) mode = kShareIpc;
      break;
    }
  }
  if (const char *e = std::getenv("BARTRT_SHARE_MODE")) if (*e) {
    const std::string v = e;
    if (v == "service") mode = kShareService;
    else if (v == "ipc") mode = kShareIpc;
    else if (v == "off" || v == "0" || v == "none") mode = kShareOff;
    else throw IoError{"BARTRT_SHARE_MODE: '" + v + "' is none of service, ipc, off"};
  }
  if (const char *e = std::getenv("BARTRT_SERVICE")) if (*e && std::string(e) != "0") { on = true; mode = kShareService; }
  if (!on) return kShareOff;
  if (mode == kShareService && no_service) mode = kShareIpc;
  return mode;
}

int parse_integ(const std::string &v) {
  if (v == "0" || v == "transmittance") return 0;
  if (v == "1" || v == "simpson") return 1;
  if (v == "2" || v == "trapz_tau" || v == "trapz") return 2;
  throw IoError{"integ: '" + v + "' is not an integration rule (0 transmittance, 1 simpson, 2 trapz_tau)"};
}

static bool file_exists(const std::string &p) {
  FILE *f = std::fopen(p.c_str(), "rb");
  if (f) std::fclose(f);
  return f != nullptr;
}

// Stage 1 (host only): settings from the configuration and the environment.
// Keys of the reference's whitelist (code/makecfg.py:36-52) accepted without
// effect: verb, allowq, rad*, orbpars*, tauiso, outtau, taulevel, modlevel --
// sampling and diagnostic controls of the CPU engine.
void Engine::read_settings() {
  // Radius-ramp cloud (makecfg.py:46-47): `cloudrad <up> <down>` (blank or comma
  // separated, in units of `cloudfct`, default `radfct`, default km) and `cloudext`
  // (cm-1): grey extinction 0 above <up>, rising linearly to cloudext at <down>,
  // cloudext below -- on the radii of each call's own hydrostatic solution.
  if (cfg_has(cfg, "cloudext") && cfg_num(cfg, "cloudext", 0.0) != 0.0) {
    std::string cr = cfg_has(cfg, "cloudrad") ? cfg["cloudrad"] : "";
    for (char &ch : cr) if (ch == ',') ch = ' ';
    TCfg tmp;
    tmp["cloudrad"] = cr;
    const auto v = cfg_list(tmp, "cloudrad");
    const double fct = cfg_num(cfg, "cloudfct", cfg_num(cfg, "radfct", 1e5));
    if (v.size() != 2 || !(v[0] > v[1]) || !(v[1] > 0) || !(fct > 0))
      throw IoError{"transit cfg: cloudext needs `cloudrad <up> <down>` with up > down > 0 (units of cloudfct)"};
    cloud_rup = v[0] * fct;
    cloud_rdown = v[1] * fct;
    cloud_ext = cfg_num(cfg, "cloudext", 0.0);
    if (!(cloud_ext > 0)) throw IoError{"transit cfg: cloudext must be positive"};
  }
  // `transparent` (makecfg.py:44): transit geometry without an opaque core below the
  // last chord; no effect on the eclipse geometry
  transparent = cfg_has(cfg, "transparent") && cfg["transparent"] != "0" && cfg["transparent"] != "no" &&
                cfg["transparent"] != "false";
  if (!cfg_has(cfg, "atm")) throw IoError{"transit cfg: missing 'atm'"};
  if (!cfg_has(cfg, "molfile")) throw IoError{"transit cfg: missing 'molfile'"};
  std::string sol = cfg_has(cfg, "solution") ? cfg["solution"] : "eclipse";
  if (sol == "transit") {
    solution = 1;
    if (!cfg_has(cfg, "starrad"))
      throw IoError{"solution 'transit' needs 'starrad' (stellar radius in solar radii) in the transit cfg"};
    starrad = cfg_num(cfg, "starrad", 0) * 6.96e10;  // Rsun of code/constants.py:11
    if (!(starrad > 0)) throw IoError{"transit cfg: bad 'starrad'"};
  } else if (sol != "eclipse") {
    throw IoError{"unknown solution '" + sol + "' (eclipse or transit)"};
  }
  // a key of this engine's own: the cfg's value (or the default), overridden by a non-empty environment variable
  auto setting = [&](const char *key, const char *env, const char *dflt) {
    std::string v = cfg_has(cfg, key) ? cfg[key] : dflt;
    if (const char *ev = std::getenv(env)) if (*ev) v = ev;
    return v;
  };
  // integration rule of the eclipse geometry (integ.hpp): `integ` in the cfg (this
  // engine's own key: the reference's source, which would settle the rule, is
  // absent), overridden by BARTRT_INTEG; number or name
  // default: rule 1, the integrator SURVEY.md App. A-4 recalls for the reference's engine
  integ = parse_integ(setting("integ", "BARTRT_INTEG", "1"));
  // `voigt exact | grid` (line-by-line evaluation, lbl.hpp / DESIGN.md C18) is checked whether or
  // not this engine ends up reading the lines
  if (cfg_has(cfg, "voigt") && cfg["voigt"] != "exact" && cfg["voigt"] != "grid")
    throw IoError{"voigt: '" + cfg["voigt"] + "' is neither exact nor grid"};
  // `cut vertical | slant`: which optical depth `toomuch` is compared with
  std::string v = setting("cut", "BARTRT_CUT", "slant");
  if (v != "vertical" && v != "slant") throw IoError{"cut: '" + v + "' is neither vertical nor slant"};
  cut_slant = v == "slant";
  v = setting("kernel_by", "BARTRT_KERNEL_BY", "local");
  if (v != "whole" && v != "local") throw IoError{"kernel_by: '" + v + "' is neither whole nor local"};
  kernel_by_local = v == "local";
  // `cia_interp` (BARTRT_CIA_INTERP): spline (default: the reading of the reference believed in,
  // DESIGN.md C20) -- natural cubic splines in wavenumber and temperature -- or linear in both (resample_cia)
  v = setting("cia_interp", "BARTRT_CIA_INTERP", "spline");
  if (v != "linear" && v != "spline") throw IoError{"cia_interp: '" + v + "' is neither linear nor spline"};
  cia_spline = v == "spline";
}

// Stage 2: an opacity file that does not exist yet is generated from the line list
// first (what `transit --justOpacity` does, BART.py:561-565), by a
// temporary line-by-line engine on the same configuration.
void Engine::generate_missing_opacity_file(int shard_rank) {
  if (!cfg_has(cfg, "opacityfile") || file_exists(cfg["opacityfile"])) return;
  if (!cfg_has(cfg, "linedb"))
    throw IoError{"cannot open opacity file '" + cfg["opacityfile"] + "' (and no 'linedb' to build it from)"};
  if (shard_rank != 0) throw IoError{"opacity file missing: generate it on an unsharded engine first"};
  TCfg gcfg = cfg;
  gcfg.erase("opacityfile");
  Engine gen;
  gen.device = device;
  gen.share_mode = kShareOff;
  gen.setup(gcfg, 0, 1);
  std::vector<double> tg;
  const double tlow = cfg_num(cfg, "tlow", 500.0), thigh = cfg_num(cfg, "thigh", 3000.0),
               dt = cfg_num(cfg, "tempdelt", 100.0);
  if (!(dt > 0) || !(thigh > tlow)) throw IoError{"transit cfg: bad tlow/thigh/tempdelt"};
  for (int k = 0; tlow + k * dt <= thigh + 1e-9 * dt; k++) tg.push_back(tlow + k * dt);
  lbl_write_opacity(gen, cfg["opacityfile"], tg);
}

// Stage 3 (host only): atmosphere, molecule file, species masses.
void Engine::read_atmosphere() {
  atm = read_atm(cfg["atm"]);
  mol = read_molfile(cfg["molfile"]);
  L = (int)atm.press.size();
  S = (int)atm.species.size();
  mass.resize(S);
  for (int s = 0; s < S; s++) {
    int j = mol.find_name(atm.species[s]);
    if (j < 0) throw IoError{"species '" + atm.species[s] + "' is not in the molecule file"};
    mass[s] = mol.mass[j];
    if (atm.species[s] == "H2") iH2 = s;
    if (atm.species[s] == "He") iHe = s;
  }
  for (int l = 0; l + 1 < L; l++)
    if (!(atm.press[l] > atm.press[l + 1]))
      throw IoError{"atmosphere file: layers must run bottom -> top (decreasing pressure)"};
}

// Stage 4 (host only): wavenumber grid -- the opacity file's (its header goes to oh) or the cfg's -- and this
// rank's block of it.
void Engine::read_grid(OpacityHeader &oh, int shard_rank, int shard_n) {
  if (cfg_has(cfg, "opacityfile")) {
    oh = read_opacity_header(cfg["opacityfile"]);
    if (oh.nlayer != L) throw IoError{"opacity file: layer count differs from the atmosphere file"};
    for (int l = 0; l < L; l++)
      if (std::fabs(oh.press[l] - atm.press[l]) > 1e-9 * atm.press[l])
        throw IoError{"opacity file: pressure layers differ from the atmosphere file"};
    wn_full = oh.wn;
    tgrid = oh.temp;
    M = (int)oh.nmol;
    Nt = (int)oh.ntemp;
    if (M > kMaxMol) throw IoError{"opacity file: too many molecules"};
    opmol.resize(M);
    for (int m = 0; m < M; m++) {
      int j = mol.find_id(oh.molid[m]);
      if (j < 0) throw IoError{"opacity file: molecule ID not in the molecule file"};
      auto it = std::find(atm.species.begin(), atm.species.end(), mol.name[j]);
      if (it == atm.species.end())
        throw IoError{"opacity file: molecule '" + mol.name[j] + "' is not in the atmosphere file"};
      opmol[m] = (int)(it - atm.species.begin());
    }
  } else {
    double lo_wn, hi_wn;
    double wnfct = cfg_num(cfg, "wnfct", 1.0), wlfct = cfg_num(cfg, "wlfct", 1e-4);
    if (cfg_has(cfg, "wnlow") && cfg_has(cfg, "wnhigh")) {
      lo_wn = cfg_num(cfg, "wnlow", 0) * wnfct;
      hi_wn = cfg_num(cfg, "wnhigh", 0) * wnfct;
    } else if (cfg_has(cfg, "wllow") && cfg_has(cfg, "wlhigh")) {
      lo_wn = 1.0 / (cfg_num(cfg, "wlhigh", 0) * wlfct);
      hi_wn = 1.0 / (cfg_num(cfg, "wllow", 0) * wlfct);
    } else {
      throw IoError{"transit cfg: no spectral range (wnlow/wnhigh or wllow/wlhigh)"};
    }
    double d = cfg_num(cfg, "wndelt", 1.0) * wnfct;
    if (!(d > 0) || !(hi_wn > lo_wn)) throw IoError{"transit cfg: bad spectral sampling"};
    long n = (long)std::floor((hi_wn - lo_wn) / d + 1e-9) + 1;
    wn_full.resize(n);
    for (long i = 0; i < n; i++) wn_full[i] = lo_wn + d * (double)i;
    M = 0; Nt = 2; tgrid = {0.0, 1.0};
  }
  Wfull = (int)wn_full.size();
  lo = (int)((long)Wfull * shard_rank / shard_n);
  hi = (int)((long)Wfull * (shard_rank + 1) / shard_n);
  if (hi <= lo) throw IoError{"--shard leaves this rank without wavenumber samples"};
}

// Stage 5 (host only): ray grid, `toomuch`, hydrostatic keys, cloud top, scattering.
void Engine::read_geometry() {
  angles = cfg_list(cfg, "raygrid");
  if (angles.empty()) angles = {0, 20, 40, 60, 80};
  A = (int)angles.size();
  if (A > kMaxAngles) throw IoError{"raygrid: too many angles"};
  for (int a = 0; a < A; a++)
    if (angles[a] < 0 || angles[a] >= 90 || (a && angles[a] <= angles[a - 1]))
      throw IoError{"raygrid: angles must increase within [0, 90)"};
  toomuch = cfg_num(cfg, "toomuch", 20.0);
  if (!cfg_has(cfg, "gsurf") || !cfg_has(cfg, "refpress") || !cfg_has(cfg, "refradius"))
    throw IoError{"transit cfg: gsurf, refpress and refradius are required"};
  gsurf = cfg_num(cfg, "gsurf", 0);
  refpress = cfg_num(cfg, "refpress", 0) * 1e6;      // bar -> barye
  refradius = cfg_num(cfg, "refradius", 0) * 1e5;    // km -> cm
  if (cfg_has(cfg, "cloudtop")) { has_cloud = 1; cloudtop = std::pow(10.0, cfg_num(cfg, "cloudtop", 0)) * 1e6; }
  if (cfg_has(cfg, "scattering")) { scat_flag = 1; scat_value = cfg_num(cfg, "scattering", 0); }
}

// Stage 6: device, stream, and the pinned word wait() polls.
void Engine::open_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw HipError{hipErrorNoDevice, "no HIP device: libbartrt computes on the GPU only"};
  if (device < 0) {
    const char *lr = std::getenv("LOCAL_RANK");
    device = lr ? std::atoi(lr) % ndev : 0;
  }
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  const char *e = std::getenv("BARTRT_SYNC");
  sync_poll = !(e && std::string(e) == "stream");
  if (!sync_poll) return;
  try {
    void *dv = nullptr;
    h_flag.reserve(16);   // (64 bytes)
    HIPCHK(hipHostGetDevicePointer(&dv, h_flag.get(), 0));
    *h_flag = 0;
    d_flag = static_cast<unsigned int *>(dv);
  } catch (const HipError &) {   // no pinned word: hipStreamSynchronize
    (void)hipGetLastError();
    sync_poll = false;
  }
}

// What names one process's upload of the table to the others of `shareOpacity`: the file (path, size, time), the
// user, the device and this rank's block.
static std::string share_key(const std::string &file, int device, int lo, int hi) {
  struct stat fst;
  if (stat(file.c_str(), &fst) != 0) throw IoError{"opacity file: cannot stat " + file};
  char rp[PATH_MAX];
  const std::string real = realpath(file.c_str(), rp) ? std::string(rp) : file;
  hipDeviceProp_t prop;
  std::string devid = std::to_string(device);
  if (hipGetDeviceProperties(&prop, device) == hipSuccess)
    devid = std::to_string(prop.pciDomainID) + ":" + std::to_string(prop.pciBusID) + ":" + std::to_string(prop.pciDeviceID);
  return real + "|" + std::to_string((long long)fst.st_size) + "|" + std::to_string((long long)fst.st_mtime) +
         "|" + std::to_string((long long)getuid()) + "|dev " + devid + "|wn " + std::to_string(lo) + ":" +
         std::to_string(hi) + "|layout LTWM v1";
}

// Stage 7: the wavenumber grids and the opacity table to HBM.
void Engine::upload_table(const OpacityHeader &oh) {
  const int Wl = W();
  d_wn.upload(wn_full.data() + lo, (size_t)Wl);
  d_wn_full.upload(wn_full);
  if (M == 0) return;
  // The file's order o[L][Nt][M][W] goes up slab by slab -- a bounded number of (layer,
  // temperature) planes through one pinned host buffer and one device staging buffer
  // (256 MB, BARTRT_INIT_SLAB_BYTES) -- and is re-laid out on the device with each
  // wavenumber's molecules contiguous (kernels.hpp, "Table layout"): peak memory during
  // init is the table + one slab, on the device and on the host.
  const size_t n = (size_t)L * Nt * M * Wl;
  const long planes = (long)L * Nt;
  const size_t plane_doubles = (size_t)M * Wl;
  size_t slab_bytes = (size_t)256 << 20;
  if (const char *e = std::getenv("BARTRT_INIT_SLAB_BYTES")) slab_bytes = std::max<size_t>(1, std::strtoull(e, nullptr, 10));
  const long per = std::max<long>(1, std::min<long>(planes, (long)(slab_bytes / (plane_doubles * sizeof(double)))));
  auto upload = [&](double *dst) {
    PinBuf<double> h;
    DevBuf<double> d_stage;
    h.reserve((size_t)per * plane_doubles);
    d_stage.reserve((size_t)per * plane_doubles);
    for (long p0 = 0; p0 < planes; p0 += per) {
      const long np = std::min(per, planes - p0);
      read_opacity_rows(cfg["opacityfile"], oh, lo, hi, p0 * M, np * M, h);
      HIPCHK(hipMemcpyAsync(d_stage, h, (size_t)np * plane_doubles * sizeof(double), hipMemcpyHostToDevice, stream));
      HIPCHK(launch_grid_transpose(d_stage, dst + (size_t)p0 * plane_doubles, np, M, Wl, stream));
      HIPCHK(hipStreamSynchronize(stream));   // the slab buffers are reused
    }
  };
  // `shareOpacity` (code/makecfg.py:106-107: BART's worker processes share ONE opacity grid; a bare key in
  // the cfg makeTransit writes) or BARTRT_SHARE_OPACITY=1: the first process of this (file, device, block)
  // uploads the grid, the others map its HBM allocation through an IPC handle (share.hpp)
  if (share_mode < 0) share_mode = resolve_share_mode(cfg, true);
  if (share_mode == kShareIpc) {
    kappa_share = TableShare::attach(share_key(cfg["opacityfile"], device, lo, hi), n * sizeof(double), upload);
    d_kappa = kappa_share->ptr;
  } else {
    kappa_own.reserve(n);
    upload(kappa_own);
    d_kappa = kappa_own;
  }
}

// second derivatives of the natural cubic spline through (x, y), n points (n < 3: zero)
static void spline_y2(const double *x, const double *y, size_t n, size_t stride, double *y2) {
  for (size_t i = 0; i < n; i++) y2[i * stride] = 0.0;
  if (n < 3) return;
  std::vector<double> u(n, 0.0);
  for (size_t i = 1; i + 1 < n; i++) {
    const double sig = (x[i] - x[i - 1]) / (x[i + 1] - x[i - 1]);
    const double p = sig * y2[(i - 1) * stride] + 2.0;
    y2[i * stride] = (sig - 1.0) / p;
    const double d = (y[(i + 1) * stride] - y[i * stride]) / (x[i + 1] - x[i]) -
                     (y[i * stride] - y[(i - 1) * stride]) / (x[i] - x[i - 1]);
    u[i] = (6.0 * d / (x[i + 1] - x[i - 1]) - sig * u[i - 1]) / p;
  }
  for (size_t k = n - 1; k-- > 1;) y2[k * stride] = y2[k * stride] * y2[(k + 1) * stride] + u[k];
}

// One cross-section file on the grid wn[0..Wl): planes [nt][Wl], zero outside the file; linear in wavenumber, or
// the natural cubic spline through the file's samples
static std::vector<double> cia_on_grid(const Cia &c, const double *wn, int Wl, bool spline) {
  const size_t nw = c.wn.size(), ntc = c.temp.size();
  std::vector<double> planes(ntc * (size_t)Wl), y2w(spline ? nw : 0);
  for (size_t t = 0; t < ntc; t++) {
    const double *al = c.alpha.data() + t * nw;
    if (spline) spline_y2(c.wn.data(), al, nw, 1, y2w.data());
    for (int i = 0; i < Wl; i++) {
      double x = wn[i], v = 0.0;
      if (x >= c.wn.front() && x <= c.wn.back() && nw > 1) {
        size_t j = std::upper_bound(c.wn.begin(), c.wn.end(), x) - c.wn.begin();
        if (j >= nw) j = nw - 1;
        if (j == 0) j = 1;
        double x0 = c.wn[j - 1], x1 = c.wn[j];
        // np.interp form: slope * (x - x0) + y0
        v = (al[j] - al[j - 1]) / (x1 - x0) * (x - x0) + al[j - 1];
        if (x == x1) v = al[j];
        if (spline) {
          const double h = x1 - x0, a = (x1 - x) / h, b = (x - x0) / h;
          v = a * al[j - 1] + b * al[j] + ((a * a * a - a) * y2w[j - 1] + (b * b * b - b) * y2w[j]) * (h * h) / 6.0;
        }
      } else if (nw == 1 && x == c.wn.front()) {
        v = al[0];
      }
      planes[t * Wl + i] = v;
    }
  }
  return planes;
}

// planes [ntc][Wl] -> appended to out as max(ntc - 1, 1) pair planes [Wl][2] = (plane t, plane t + 1) per wavenumber
static void push_pair_planes(const std::vector<double> &pl, size_t ntc, int Wl, std::vector<double> &out) {
  const size_t npair = std::max<size_t>(ntc - 1, 1);
  for (size_t t = 0; t < npair; t++) {
    const size_t hi_t = std::min(t + 1, ntc - 1);
    for (int i = 0; i < Wl; i++) {
      out.push_back(pl[t * Wl + i]);
      out.push_back(pl[hi_t * Wl + i]);
    }
  }
}

// Stage 8 (host only): CIA, resampled on the local grid (zero outside the file) and laid out, per table, as nt-1
// pair planes [W][2] = (alpha_j, alpha_j+1) per wavenumber: one 16-byte load per table and
// layer (kernels.hpp, "Table layout").  Under `cia_interp spline`
// the temperature spline's second derivatives ride as one more table per file, whose
// weights prep_body fills with the spline's curvature terms, so every RT kernel serves it.
void Engine::resample_cia(std::vector<double> &cia_planes, std::vector<double> &cia_temp) {
  if (!cfg_has(cfg, "csfile")) return;
  PrepArgs &pa = prep;
  const int Wl = W();
  auto files = split_file_list(cfg["csfile"]);
  if ((int)files.size() * (cia_spline ? 2 : 1) > kMaxCia)
    throw IoError{cia_spline ? "csfile: too many cross-section files for cia_interp spline (two table slots each)"
                             : "csfile: too many cross-section files"};
  for (auto &fn : files) {
    Cia c = read_cia(fn);
    int cc = C++;
    auto f1 = std::find(atm.species.begin(), atm.species.end(), c.s1);
    auto f2 = std::find(atm.species.begin(), atm.species.end(), c.s2);
    if (f1 == atm.species.end() || f2 == atm.species.end())
      throw IoError{"cross-section file '" + fn + "': species not in the atmosphere file"};
    pa.cia_s1[cc] = (int)(f1 - atm.species.begin());
    pa.cia_s2[cc] = (int)(f2 - atm.species.begin());
    pa.cia_nt[cc] = (int)c.temp.size();
    pa.cia_toff[cc] = (int)cia_temp.size();
    pa.cia_kind[cc] = 0;
    const size_t ntc = c.temp.size();
    // resampled planes [nt][Wl] first, then the (lower, upper) pair planes
    const std::vector<double> planes = cia_on_grid(c, wn_full.data() + lo, Wl, cia_spline);
    pa.cia_poff[cc] = (int)(cia_planes.size() / ((size_t)2 * Wl));
    push_pair_planes(planes, ntc, Wl, cia_planes);
    cia_temp.insert(cia_temp.end(), c.temp.begin(), c.temp.end());
    if (cia_spline) {
      // the second table of the file: second derivatives in T of the resampled planes
      const int c2 = C++;
      pa.cia_s1[c2] = pa.cia_s1[cc]; pa.cia_s2[c2] = pa.cia_s2[cc];
      pa.cia_nt[c2] = pa.cia_nt[cc];
      pa.cia_toff[c2] = (int)cia_temp.size();
      pa.cia_kind[c2] = 1;
      std::vector<double> y2t(planes.size(), 0.0);
      for (int i = 0; i < Wl; i++) spline_y2(c.temp.data(), planes.data() + i, ntc, (size_t)Wl, y2t.data() + i);
      pa.cia_poff[c2] = (int)(cia_planes.size() / ((size_t)2 * Wl));
      push_pair_planes(y2t, ntc, Wl, cia_planes);
      cia_temp.insert(cia_temp.end(), c.temp.begin(), c.temp.end());
    }
  }
}

// hydrostatic reference layer (makeatm.py:229-247)
static void hydrostatic_reference(PrepArgs &pa, const std::vector<double> &press, double refpress) {
  const int L = (int)press.size();
  int ix = 0;
  double best = std::fabs(press[0] - refpress);
  for (int i = 1; i < L; i++) {
    double d = std::fabs(press[i] - refpress);
    if (d < best) { best = d; ix = i; }
  }
  pa.ref_idx = ix;
  pa.ref_exact = press[ix] == refpress;
  pa.ref_ib = ix < L - 1 ? ix : ix - 1;
  pa.ref_f = ix < L - 1 ? 0.0 : 1.0;
  if (L == 1) { pa.ref_ib = 0; pa.ref_f = 0.0; }
  double lp0 = std::log10(refpress);
  for (int i = 0; i + 1 < L; i++) {
    double la = std::log10(press[i]), lb = std::log10(press[i + 1]);
    if ((lp0 <= la && lp0 >= lb) || (lp0 >= la && lp0 <= lb)) {
      pa.ref_ib = i;
      pa.ref_f = (lp0 - la) / (lb - la);
      break;
    }
  }
  pa.ref_lnp = std::log(refpress / press[ix]);
}

// Stage 9: the CIA planes and the per-layer constants to HBM; the static part of PrepArgs and RtArgs.
void Engine::upload_constants(const std::vector<double> &cia_planes, const std::vector<double> &cia_temp) {
  PrepArgs &pa = prep;
  const int Wl = W();
  d_cia.upload(cia_planes);
  std::vector<double> dlnp(std::max(L - 1, 1), 0.0);
  for (int l = 0; l + 1 < L; l++) dlnp[l] = std::log(atm.press[l] / atm.press[l + 1]);
  d_press.upload(atm.press);
  d_mass.upload(mass);
  std::vector<double> diam(S);
  for (int s = 0; s < S; s++) diam[s] = mol.diam[mol.find_name(atm.species[s])] * 1e-8;
  d_diam.upload(diam);
  hydrostatic_reference(pa, atm.press, refpress);
  pa.L = L; pa.S = S; pa.M = M; pa.Nt = Nt; pa.C = C; pa.W = Wl;
  {
    // prep_profiles' constants in one block (layout: kernels.hpp, PrepArgs::consts)
    std::vector<double> blob(atm.press);
    blob.insert(blob.end(), dlnp.begin(), dlnp.end());
    blob.resize(2 * (size_t)L, 0.0);
    blob.insert(blob.end(), mass.begin(), mass.end());
    auto with_inverse_spacing = [&](const double *g, int n) {
      blob.insert(blob.end(), g, g + n);
      for (int j = 0; j < n; j++) blob.push_back(j + 1 < n ? 1.0 / (g[j + 1] - g[j]) : 0.0);
    };
    with_inverse_spacing(tgrid.data(), Nt);
    const size_t at = blob.size();
    blob.insert(blob.end(), cia_temp.begin(), cia_temp.end());
    blob.resize(at + 2 * cia_temp.size(), 0.0);
    for (int c = 0; c < C; c++)
      for (int j = 0; j + 1 < pa.cia_nt[c]; j++) {
        const double *g = cia_temp.data() + pa.cia_toff[c];
        blob[at + cia_temp.size() + pa.cia_toff[c] + j] = 1.0 / (g[j + 1] - g[j]);
      }
    d_prep_consts.upload(blob);
  }
  pa.consts = d_prep_consts;
  if (M > kMaxMol) throw IoError{"more opacity-table molecules than the kernels are built for (16)"};
  for (int m = 0; m < M; m++) pa.opmol[m] = opmol[m];
  pa.ncia_temps = (int)cia_temp.size();
  // the preparation keeps a walker's whole column in LDS (prep.hpp): what cannot fit is refused here, not at the first run
  const size_t prep_lds = sizeof(double) * prep_lds_doubles(L, S, Nt, pa.ncia_temps);
  if (prep_lds > kLdsMax)
    throw IoError{"the column's preparation does not fit in LDS: L = " + std::to_string(L) + " layers and S = " +
                  std::to_string(S) + " species need " + std::to_string(prep_lds) + " bytes of the " +
                  std::to_string(kLdsMax) + " a workgroup has"};
  pa.iH2 = iH2; pa.iHe = iHe;

  RtArgs &r = rt;
  r.L = L; r.M = M; r.Nt = Nt; r.C = C; r.A = A; r.W = Wl; r.Wfull = Wfull;
  r.kappa = d_kappa; r.cia = d_cia; r.wn = d_wn;
  r.kappa_bytes = (unsigned long long)L * Nt * M * Wl * 8ull;
  r.cia_bytes = (unsigned long long)cia_planes.size() * 8ull;
  for (int a = 0; a < A; a++) {
    double lo_a = a == 0 ? 0.0 : 0.5 * (angles[a - 1] + angles[a]);
    double hi_a = a == A - 1 ? 90.0 : 0.5 * (angles[a] + angles[a + 1]);
    double sl = std::sin(lo_a * kPI / 180.0), sh = std::sin(hi_a * kPI / 180.0);
    r.wgt[a] = kPI * (sh * sh - sl * sl);
    r.invmu[a] = 1.0 / std::cos(angles[a] * kPI / 180.0);
    r.wq[a] = r.wgt[a] * r.invmu[a];
    r.mu[a] = std::cos(angles[a] * kPI / 180.0);
  }
}

// Stage 10: the line list (an engine without a table), the first workspaces, and the warm-up launches.
void Engine::start_workspaces() {
  if (!cfg_has(cfg, "opacityfile") && cfg_has(cfg, "linedb")) {
    lbl_init(*this, cfg["linedb"]);
    const char *m = std::getenv("BARTRT_LBL");
    // measured on the config-5 shape (tools/lbl_bench.py): tiles rarely turn opaque
    // as a whole, so the lazy fused kernel (55 ms) loses to the eager two-pass form
    // (43 ms) that exposes all layers as parallel work; BARTRT_LBL=lazy selects it
    // (the fused kernel evaluates the line sums on the output points: no oversampling)
    lbl_eager = !(m && std::string(m) == "lazy") || lbl->dev.osamp > 1 || lbl->dev.voigt_grid;
  }
  d_tau.reserve((size_t)W() * L);
  d_last.reserve((size_t)W());
  ensure_walkers(16);
  // The first launch of a kernel loads its code object (the single-wave kernels' translation unit is 10 MB: 20 ms,
  // seen as ONE 20 ms call among the first of a run -- round 5, three worker processes on the chain service).  The
  // atmosphere file's own profile goes through a one-walker and a twelve-walker launch here, once, so that the
  // first MCMC step does not pay it (BARTRT_WARMUP=0: off).  Table path of the eclipse geometry.
  const char *wv = std::getenv("BARTRT_WARMUP");
  if ((wv && wv[0] == '0') || solution != 0 || lbl || M == 0) return;
  const int nprof = (S + 1) * L, nw = 12;
  std::vector<double> hp((size_t)nw * nprof);
  for (int w = 0; w < nw; w++)
    for (int l = 0; l < L; l++) {
      hp[(size_t)w * nprof + l] = atm.temp[l];
      for (int k = 0; k < S; k++) hp[(size_t)w * nprof + (size_t)(k + 1) * L + l] = atm.abund[(size_t)l * S + k];
    }
  HIPCHK(hipMemcpy(d_prof, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice));
  run(RunRequest(d_prof, 1, d_spec, rec[0].ok, stream));
  run(RunRequest(d_prof, nw, d_spec, rec[0].ok, stream));
  HIPCHK(hipStreamSynchronize(stream));
  forget_profiles();
}

void Engine::setup(const TCfg &cfg_in, int shard_rank, int shard_n) {
  cfg = cfg_in;
  read_settings();
  generate_missing_opacity_file(shard_rank);
  read_atmosphere();
  OpacityHeader oh;
  read_grid(oh, shard_rank, shard_n);
  read_geometry();
  open_device();
  upload_table(oh);
  std::vector<double> cia_planes, cia_temp;
  resample_cia(cia_planes, cia_temp);
  upload_constants(cia_planes, cia_temp);
  start_workspaces();
}

void Engine::ensure_walkers(int n) {
  if (n <= cap_walkers) return;
  int cap = std::max(n, cap_walkers * 2);
  HIPCHK(hipDeviceSynchronize());
  if (last_prof == d_prof) forget_profiles();
  pf_have_prof = nullptr;  // (prefetched records, if any, are dropped with their buffers' sizes)
  prep_seen = PrepSeen{};
  if (cap2) {
    rec[1].reserve((size_t)cap, L, M, C);
    cap2 = cap;
  }
  d_prof.reserve((size_t)cap * (S + 1) * L);
  rec[0].reserve((size_t)cap, L, M, C);
  d_spec.reserve((size_t)cap * W());
  d_rad.reserve((size_t)cap * L);
  if (solution == 1) {
    d_rtop.reserve((size_t)cap * L);
    d_ds.reserve((size_t)cap * chord_table_size(L));
  }
  cap_walkers = cap;
}

// the second set of record buffers, as large as the first (nothing is prefetched into it yet)
void Engine::ensure_second_set() {
  if (cap2 >= cap_walkers) return;
  HIPCHK(hipDeviceSynchronize());
  prep_seen = PrepSeen{};
  rec[1].reserve((size_t)cap_walkers, L, M, C);
  cap2 = cap_walkers;
}

void Engine::wait(hipStream_t st) {
  if (!sync_poll || !h_flag) { HIPCHK(hipStreamSynchronize(st)); return; }
  const unsigned int want = ++flag_seq;
  HIPCHK(hipStreamWriteValue32(st, d_flag, want, 0));
  volatile unsigned int *f = h_flag;
  long spins = 0;
  while (*f != want) {
    __builtin_ia32_pause();
    // (a launch that failed never writes: the stream itself is asked now and then, and reports the error)
    if ((++spins & 0xfffff) == 0 && hipStreamQuery(st) != hipErrorNotReady) { HIPCHK(hipStreamSynchronize(st)); break; }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

void Engine::ensure_pin(size_t bytes) {
  const size_t n = (bytes + sizeof(double) - 1) / sizeof(double);
  if (n <= h_pin.count()) return;
  forget_profiles();
  prep_seen = PrepSeen{};   // (a small host-buffer call keeps its flags in h_pin)
  h_pin.reserve(n);
}

// The walkers of rq in chunks of `chunk`: every chunk is a request of its own rows -- profiles, spectra, flags and
// overrides ([n][3]) -- and the first carries the prefetch request.
// with_ext: the chunk's line-by-line extinction first ([walkers][L][W], lbl_extinction), for run_chunk to read.
void Engine::run_chunks(const RunRequest &rq, int chunk, bool with_ext) {
  const int nprof = (S + 1) * L;
  RunRequest c = rq;
  if (!c.ok) c.ok = rec[0].ok;
  for (int off = 0; off < rq.n; off += chunk) {
    c.n = std::min(chunk, rq.n - off);
    if (with_ext) {
      lbl_extinction(*this, c.prof, c.n, c.stream);
      c.d_ext = lbl->d_ext;
    }
    run_chunk(c);
    c.prof += (size_t)c.n * nprof;
    c.spec += (size_t)c.n * W();
    c.ok += c.n;
    if (c.over) c.over += (size_t)3 * c.n;
    c.next_prof = nullptr;
    c.next_n = 0;
  }
}

void Engine::run(const RunRequest &asked) {
  if (asked.n <= 0) return;
  // what earlier calls left for this one moves into the request here and nowhere else, before anything can throw
  // (a request with overrides or a preparation of its own -- the chain service, the fused step -- keeps those)
  RunRequest rq = asked;
  const Pending left = pending;
  pending = Pending{};
  if (!rq.over && !rq.prep_hook) { rq.over = left.over; rq.over_cloud = left.over_cloud; }
  rq.next_prof = left.next_prof;
  rq.next_n = left.next_n;
  const int n = rq.n;
  // per-walker workspaces (records, flags) are sized by cap_walkers; the caller's profiles and spectra are used in place
  if (n > cap_walkers && rq.prof != d_prof) ensure_walkers(n);
  if (lbl && solution == 0 && !rq.want_tau && !rq.want_intens && !lbl_eager && integ == 0 && !cut_slant) {
    // lazy fused path: layers' line sums are evaluated only as deep as the optical depth requires
    rq.lbl_fused = true;
    run_chunk(rq);
    return;
  }
  if (lbl) {
    // eager path (optical-depth / intensity outputs, transit geometry): [walkers][L][W] extinction first, in chunks
    const size_t per = (size_t)L * W() * sizeof(double);
    size_t cap_bytes = (size_t)2 << 30;
    if (const char *c = std::getenv("BARTRT_LBL_CHUNK_BYTES")) cap_bytes = std::max<size_t>(1, std::strtoull(c, nullptr, 10));
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, cap_bytes / per));
    run_chunks(rq, chunk, true);
    return;
  }
  // `cut slant`, rule 1: the single-wave kernels keep an event log of 100 bytes per (walker, wavenumber) lane
  // (RtArgs::slog) -- 1 MB per walker at W = 1e4.  A batch whose log would pass BARTRT_SLOG_CAP_BYTES (1 GiB) goes
  // out in chunks of walkers (results are per walker: the same bits either way).
  if (cut_slant && integ == 1 && solution == 0 && !rq.prep_hook) {   // (the fused per-step launch addresses its batch whole)
    static const size_t cap = [] {
      const char *c = std::getenv("BARTRT_SLOG_CAP_BYTES");
      return c && *c ? std::max<size_t>(1, std::strtoull(c, nullptr, 10)) : (size_t)1 << 30;
    }();
    const size_t per = std::max<size_t>(1, slant_log_bytes(1, (W() + 63) / 64, 64, A));
    const int chunk = (int)std::max<size_t>(1, cap / per);
    if (n > chunk) {
      run_chunks(rq, chunk, false);
      return;
    }
  }
  run_chunk(rq);
}

// host-buffer calls up to this size skip the staging copies (run_host)
static constexpr size_t kZeroCopyBytes = 512 * 1024;

void Engine::run_host(const double *prof, int n, int nprof, double *spec, int nwave, unsigned char *ok) {
  if (n <= 0) return;
  const int Wl = W();
  ensure_walkers(n);
  const size_t pb = sizeof(double) * (size_t)n * nprof;
  const size_t sb = sizeof(double) * (size_t)n * Wl;
  ensure_pin(pb + sb + n);
  std::memcpy(h_pin, prof, pb);
  double *hs = h_pin + (size_t)n * nprof;
  unsigned char *hok = reinterpret_cast<unsigned char *>(hs + (size_t)n * Wl);
  if (pb + sb <= kZeroCopyBytes) {
    // a walker or a few: the kernels read the profiles from, and write the spectra to, the pinned host buffer
    // themselves (three copy operations cost more than the kernels at this size)
    void *dev = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dev, h_pin, 0));
    double *dp = static_cast<double *>(dev), *ds = dp + (size_t)n * nprof;
    run(RunRequest(dp, n, ds, reinterpret_cast<unsigned char *>(ds + (size_t)n * Wl), stream));
    remember_profiles(dp, n);   // stays valid until the next host-buffer call
  } else {
    remember_profiles(d_prof, n);
    HIPCHK(hipMemcpyAsync(d_prof, h_pin, pb, hipMemcpyHostToDevice, stream));
    run(RunRequest(d_prof, n, d_spec, rec[0].ok, stream));
    HIPCHK(hipMemcpyAsync(hs, d_spec, sb, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(hok, rec[0].ok, n, hipMemcpyDeviceToHost, stream));
  }
  wait(stream);
  const size_t off = nwave == Wl ? 0 : (size_t)lo;
  for (int w = 0; w < n; w++) std::memcpy(spec + (size_t)w * nwave + off, hs + (size_t)w * Wl, sizeof(double) * Wl);
  if (ok) {
    std::memcpy(ok, hok, n);
  } else {
    // no flag array to report through (the reference-shaped single call): refuse loudly
    for (int w = 0; w < n; w++)
      if (!hok[w]) throw std::invalid_argument("run_transit: the profile holds a non-finite or non-positive temperature");
  }
}

// The prefetch decision of one run_chunk call (prefetched preparation, engine.hpp)
struct Engine::Prefetch {
  bool have, want_next;  // the records were prepared by the previous call's RT launch; this one's prepares rq.next_*
  int bset;         // the record set this call's RT kernel reads (the other one takes the next batch's)
  PrepSettings now; // the settings the layer records are built from, as they stand for THIS call
};

Engine::Prefetch Engine::plan_prefetch(bool pf_ok, const RunRequest &rq) {
  bool want_next = pf_ok && rq.next_prof && rq.next_n > 0;
  // the RT launch that carries the next batch's preparation asks for the larger of the two jobs' LDS plus what its form
  // adds (rt_launch.hpp, SpecLaunch: a double per layer in the 16-row forms, the 8.5 kB hand-off ring of
  // rt_eclipse_split) and is not opted in above the 64 kB default (lds.hpp): on a column whose preparation needs that
  // much the request is dropped, the named batch is prepared by its own call
  const size_t pf_lds = sizeof(double) * prep_lds_doubles(L, S, Nt, prep.ncia_temps) + std::max<size_t>(9 * 1024, sizeof(double) * L);
  if (want_next && pf_lds > kLdsDefault) want_next = false;
  if (want_next && rq.next_n > cap_walkers) {
    // the workspaces have to grow for the named batch: not under a call whose own buffers are the
    // engine's (a host-buffer batch: growing frees what it is about to read and write) -- such a
    // request is dropped, the named batch is prepared by its own call
    const bool own = rq.prof == d_prof || rq.spec == d_spec || rq.ok == rec[0].ok;
    if (own) want_next = false;
    else ensure_walkers(rq.next_n);   // (drops prefetched records)
  }
  // records prefetched under other settings (a bartrt_set_radius / _cloudtop / _scattering in between) or on
  // another stream are not used -- the call prepares its own
  const PrepSettings now{refradius, gsurf, cloudtop, scat_value, cloud_rup, cloud_rdown, cloud_ext, has_cloud,
                         rq.scat_flag >= 0 ? rq.scat_flag : scat_flag};
  const bool have = pf_ok && pf_have_prof && pf_have_prof == rq.prof && pf_have_n == rq.n && pf_have_stream == rq.stream &&
                    pf_have_set == now;
  const int bset = have ? pf_have_buf : 0;
  pf_have_prof = nullptr;
  if (want_next) ensure_second_set();   // (first request)
  return Prefetch{have, want_next, bset, now};
}

// PrepArgs of one call: the engine's settings as they stand (the request's scattering flag, if it has one), the
// request's overrides, the records into set `records`
PrepArgs Engine::prep_args(const RunRequest &rq, const RecordSet &records) {
  PrepArgs pa = prep;
  pa.nwalkers = rq.n;
  pa.prof = rq.prof;
  pa.gsurf = gsurf; pa.refradius = refradius;
  pa.scat_flag = rq.scat_flag >= 0 ? rq.scat_flag : scat_flag; pa.scat_value = scat_value;
  pa.has_cloud = has_cloud; pa.cloudtop = cloudtop;
  pa.cloud_rup = cloud_rup; pa.cloud_rdown = cloud_rdown; pa.cloud_ext = cloud_ext;
  pa.coef = records.coef; pa.idx = records.idx; pa.kstop = records.kstop;
  pa.ok = rq.ok ? rq.ok : rec[0].ok.get();
  pa.rad_out = d_rad;
  pa.over = rq.over;
  pa.rtop = solution == 1 ? d_rtop.get() : nullptr;
  pa.ds = solution == 1 ? d_ds.get() : nullptr;
  return pa;
}

// one wave per workgroup at every batch size (measured against 128 and 256 lanes:
// 2-5 % faster from 64 walkers up, finer turnover of the SIMDs' wave slots)
static int rt_block() {
  // A/B runs: 64 (default), 128 or 256 lanes per workgroup
  static const int b = [] { const char *e = std::getenv("BARTRT_BLOCK"); return e ? std::atoi(e) : 64; }();
  return (b == 128 || b == 256) ? b : 64;
}

// RtArgs of one call.  Not a getter: it grows d_intens / d_slog / d_walked when the call needs them (d_slog after a
// device synchronisation), clears d_walked on the stream and, when timed, makes the events and records the fused
// path's first.  eclipse_rt: the launch is launch_rt's (run_chunk)
RtArgs Engine::rt_args(const RunRequest &rq, const PrepArgs &pa, const Prefetch &pf, bool eclipse_rt, bool timed) {
  const int n = rq.n, block = rt_block();
  RtArgs r = rt;
  r.nwalkers = n;
  r.nsel = rq.sel_walkers > n ? rq.sel_walkers : 0;
  if (kernel_by_local) r.Wfull = r.W;
  r.coef = pa.coef; r.idx = pa.idx; r.kstop = pa.kstop;
  r.ext = rq.d_ext;
  r.nprep = 0;
  if (pf.want_next) {
    const RecordSet &next = rec[1 - pf.bset];
    PrepArgs pn = pa;      // same engine settings; the next batch's profiles into the other buffer set
    pn.nwalkers = rq.next_n;
    pn.prof = rq.next_prof;
    pn.coef = next.coef; pn.idx = next.idx; pn.kstop = next.kstop;
    pn.ok = next.ok;
    pn.over = nullptr;
    pn.rad_out = nullptr;   // (bartrt_get_radius: the radii of the batch this call computes)
    r.nprep = rq.next_n;
    r.prep_next = pn;
  }
  r.cloud_on = has_cloud || (rq.over_cloud && (rq.over || rq.prep_hook));
  r.integ = integ;
  r.cut_slant = cut_slant ? 1 : 0;
  r.toomuch = toomuch;
  r.opt_guard = slant_opt_guard();
  if (cut_slant) slant_thresholds(r);
  r.spec = rq.spec;
  r.tau_out = (rq.want_tau && n == 1) ? d_tau.get() : nullptr;
  r.last_out = (rq.want_tau && n == 1) ? d_last.get() : nullptr;
  r.intens_out = nullptr;
  if (rq.want_intens && n == 1 && eclipse_rt) {
    d_intens.reserve((size_t)A * W());
    r.intens_out = d_intens;
  }
  r.ntiles = (r.W + block - 1) / block;
  r.rtop = d_rtop; r.ds = d_ds;
  r.slog = nullptr;
  if (cut_slant && integ == 1 && eclipse_rt) {
    // the event log of rule 1's single-wave `cut slant` kernels (rt_eclipse_s1s.hpp): 100 bytes per lane
    // (rules 0 / 2 -- rt_eclipse_fast<SLANT> -- keep none)
    const size_t need = slant_log_bytes(n, r.ntiles, block, A);
    if (need > d_slog.count()) {
      HIPCHK(hipDeviceSynchronize());   // (an earlier launch on any stream may still write the old log)
      d_slog.reserve(need);
    }
    r.slog = d_slog.get();
  }
  r.inv_starrad2 = solution == 1 ? 1.0 / (starrad * starrad) : 0.0;
  r.transparent = transparent ? 1 : 0;
  // Timing: the RT kernel's own dispatch stamps the two events (BARTRT_RT_LAUNCH) -- no marker
  // packets in the stream; only the fused line-by-line path (several kernels) is bracketed
  // by event records.
  r.ev_start = r.ev_stop = nullptr;
  if (timed) {
    while ((int)ev.size() < ev_used + 2) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      ev.push_back(e);
    }
    if (rq.lbl_fused) HIPCHK(hipEventRecord(ev[ev_used], rq.stream));
    else { r.ev_start = ev[ev_used]; r.ev_stop = ev[ev_used + 1]; }
  }
  r.walked_out = r.restart_out = nullptr;
  if (want_walked && eclipse_rt) {
    // the finest column any eclipse kernel records is ONE wavenumber wide (rt_eclipse_quad with one ray per lane, R = 8);
    // behind the layers walked, per walker: the waves that walked their column twice (RtArgs::restart_out)
    const size_t need = (size_t)n * ((size_t)r.W + 64);
    d_walked.reserve(need + (size_t)n);
    HIPCHK(hipMemsetAsync(d_walked, 0, (need + (size_t)n) * sizeof(int), rq.stream));
    r.walked_out = d_walked;
    r.restart_out = d_walked.get() + need;
    walked_nwalkers = n;
    walked_restart_off = need;
  }
  return r;
}

void Engine::run_chunk(const RunRequest &rq) {
  const int n = rq.n;
  hipStream_t st = rq.stream;
  // coefficient workspaces are sized by cap_walkers; the caller's profile and spectrum buffers are used in place
  if (n > cap_walkers) ensure_walkers(n);
  // What kind of launch this is, worked out once.  eclipse_rt: launch_rt's, from the table or from a chunk's
  // line-by-line extinction (not the lazy fused kernel, not the transit geometry).  plain: ... of the table path with
  // the engine's own preparation and spectra as its only output.  Only a plain launch may have its walkers prepared
  // by the RT kernel itself, and only one without overrides takes part in the prefetched preparation.
  const bool eclipse_rt = solution == 0 && !rq.lbl_fused;
  const bool plain = eclipse_rt && !lbl && !rq.d_ext && !rq.prep_hook && !rq.want_tau && !rq.want_intens;
  const bool pf_ok = plain && !rq.over;
  const Prefetch pf = plan_prefetch(pf_ok, rq);
  const bool use_have = pf.have, want_next = pf.want_next;
  const PrepArgs pa = prep_args(rq, rec[pf.bset]);
  // one to four walkers: the RT kernel may prepare them itself (launch_rt_folded, below)
  const bool try_fold = plain && !use_have && !want_next && std::max(n, rq.sel_walkers) <= 4 && integ == 1 && cut_slant &&
                        A == 5;
  if (use_have) {
    // prepared by the previous call's RT launch; its flags go where this call wants them
    if (rq.ok) HIPCHK(hipMemcpyAsync(rq.ok, rec[pf.bset].ok, (size_t)n, hipMemcpyDeviceToDevice, st));
  } else if (rq.prep_hook) HIPCHK(rq.prep_hook(pa, st, rq.prep_hook_ctx));
  else if (!try_fold) HIPCHK(launch_prep(pa, st));
  if (solution == 1) HIPCHK(launch_chord_table(pa, st));

  // (a call that launches nothing -- no walkers -- takes no event pair: bartrt_timing_end would read unstamped events)
  const bool timed = timing && n > 0 && rt.W > 0 && (timing_seen++ % timing_stride == 0);
  const RtArgs r = rt_args(rq, pa, pf, eclipse_rt, timed);
  bool folded = false;
  if (rq.lbl_fused) lbl_rt_eclipse(*this, rq.prof, n, r, st);
  else if (solution == 1) {
    RtLaunchInfo li;   // (the transit kernels keep no walked-layer record: the name only)
    HIPCHK(launch_transit(r, st, &li));
    if (want_walked) walked_info = li;
  }
  else {
    RtLaunchInfo li;
    if (try_fold) HIPCHK(launch_rt_folded(r, pa, rt_block(), st, &li, &folded));
    if (!folded) {
      if (try_fold) HIPCHK(launch_prep(pa, st));
      li = RtLaunchInfo{};
      HIPCHK(launch_rt(r, rt_block(), st, &li));
    }
    if (want_walked) walked_info = li;
    if (want_next && li.prep_fused) {
      pf_have_prof = rq.next_prof; pf_have_n = rq.next_n; pf_have_buf = 1 - pf.bset;
      pf_have_stream = st; pf_have_set = pf.now;
    }
  }
  // (records prefetched by the previous call's launch: their flags lie in that set unless this call asked for a copy)
  prep_seen = PrepSeen{pa.coef, pa.idx, pa.kstop, use_have && !rq.ok ? rec[pf.bset].ok.get() : pa.ok, n, folded};
  if (timed) {
    if (rq.lbl_fused) HIPCHK(hipEventRecord(ev[ev_used + 1], st));
    ev_used += 2;
  }
}

}  // namespace bartrt
