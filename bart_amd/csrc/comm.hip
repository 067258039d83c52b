// RCCL, opened at run time (include/bartrt.h, bartrt_comm_*).  The library does not link against RCCL: it loads and
// the CPU suite runs where RCCL is absent, and a process that already holds a copy (torch ships its own librccl.so
// under torch/lib; a live torch `nccl` group has it mapped) uses that copy instead of mapping a second one.  Every
// symbol comes from the one handle.
#include "comm.hpp"

#include "../../include/bartrt.h"
#include "engine.hpp"

#include <dlfcn.h>
#include <link.h>

#include <cstdlib>
#include <cstring>
#include <mutex>

namespace bartrt {

namespace {

// the parts of rccl.h the library uses (ABI of NCCL 2.x: ncclResult_t and ncclDataType_t are C enums)
struct NcclId {
  char internal[kCommIdBytes];
};
constexpr int kNcclSuccess = 0;
constexpr int kNcclFloat64 = 8;

struct Rccl {
  void *handle = nullptr;
  std::string path, why;
  int (*get_unique_id)(NcclId *) = nullptr;
  int (*comm_init_rank)(void **, int, NcclId, int) = nullptr;
  int (*comm_destroy)(void *) = nullptr;
  int (*all_gather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  const char *(*error_string)(int) = nullptr;
};

// the path of an RCCL already mapped into this process, or ""
std::string loaded_rccl() {
  std::string found;
  dl_iterate_phdr(
      [](struct dl_phdr_info *info, size_t, void *out) {
        const char *name = info->dlpi_name;
        if (!name || !*name) return 0;
        const char *base = std::strrchr(name, '/');
        base = base ? base + 1 : name;
        if (std::strncmp(base, "librccl.so", 10) == 0) {
          *static_cast<std::string *>(out) = name;
          return 1;
        }
        return 0;
      },
      &found);
  return found;
}

Rccl &rccl() {
  static Rccl r;
  static std::once_flag once;
  // (a copy mapped after the first look -- torch's group brought up later -- is not picked up: one handle per process)
  std::call_once(once, [] {
    std::string tried;
    auto open = [&](const std::string &p, int flags) {
      if (r.handle || p.empty()) return;
      r.handle = dlopen(p.c_str(), flags);
      if (r.handle) {
        r.path = p;
        return;
      }
      const char *err = dlerror();
      tried += (tried.empty() ? "" : "; ") + (err ? std::string(err) : p + ": cannot be opened");
    };
    open(loaded_rccl(), RTLD_NOW | RTLD_NOLOAD);
    if (const char *e = std::getenv("BARTRT_RCCL_LIB")) open(e, RTLD_NOW | RTLD_LOCAL);
    open("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!r.handle) {
      r.why = "RCCL is not available (" + tried + ")";
      return;
    }
    auto sym = [&](const char *name, auto &fn) {
      fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(r.handle, name));
      if (!fn && r.why.empty()) r.why = r.path + " lacks " + name;
    };
    sym("ncclGetUniqueId", r.get_unique_id);
    sym("ncclCommInitRank", r.comm_init_rank);
    sym("ncclCommDestroy", r.comm_destroy);
    sym("ncclAllGather", r.all_gather);
    sym("ncclGetErrorString", r.error_string);
  });
  if (!r.why.empty()) throw CommError{BARTRT_ENOTSUP, r.why};
  return r;
}

void check(int rc, const char *what) {
  if (rc == kNcclSuccess) return;
  const char *s = rccl().error_string ? rccl().error_string(rc) : nullptr;
  throw CommError{BARTRT_ENODEV, std::string(what) + ": " + (s ? s : "RCCL error " + std::to_string(rc))};
}

}  // namespace

void comm_get_unique_id(void *id) {
  NcclId u;
  check(rccl().get_unique_id(&u), "ncclGetUniqueId");
  std::memcpy(id, u.internal, kCommIdBytes);
}

Comm *comm_create(int device, const void *id, int rank, int nranks) {
  Rccl &r = rccl();
  NcclId u;
  std::memcpy(u.internal, id, kCommIdBytes);
  HIPCHK(hipSetDevice(device));
  void *nc = nullptr;
  check(r.comm_init_rank(&nc, nranks, u, rank), "ncclCommInitRank");
  Comm *c = new Comm();
  c->nccl = nc;
  c->rank = rank;
  c->nranks = nranks;
  return c;
}

void comm_destroy(Comm *c) {
  if (!c) return;
  (void)hipDeviceSynchronize();   // (the receive buffer and the communicator may still be in use on a stream)
  if (c->nccl) (void)rccl().comm_destroy(c->nccl);
  if (c->d_recv) (void)hipFree(c->d_recv);
  delete c;
}

double *comm_recv(Comm &c, size_t doubles) {
  if (doubles <= c.recv_doubles) return c.d_recv;
  HIPCHK(hipDeviceSynchronize());
  if (c.d_recv) HIPCHK(hipFree(c.d_recv));
  c.d_recv = nullptr;
  c.recv_doubles = 0;
  HIPCHK(hipMalloc(&c.d_recv, doubles * sizeof(double)));
  c.recv_doubles = doubles;
  return c.d_recv;
}

void comm_allgather_inplace(Comm &c, double *recv, size_t count, hipStream_t st) {
  check(rccl().all_gather(recv + (size_t)c.rank * count, recv, count, kNcclFloat64, c.nccl, st), "ncclAllGather");
}

}  // namespace bartrt
