// The library's own collective (include/bartrt.h, bartrt_comm_*): an RCCL communicator over the ranks of a
// wavenumber-sharded engine, loaded at run time so that the library loads and the CPU suite runs without RCCL.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace bartrt {

constexpr int kCommIdBytes = 128;  // NCCL_UNIQUE_ID_BYTES

// A failure of the communicator layer with the C ABI's code (BARTRT_ENOTSUP: no RCCL; BARTRT_ENODEV: RCCL failed)
struct CommError {
  int code;
  std::string msg;
};

struct Comm {
  void *nccl = nullptr;        // ncclComm_t
  int rank = 0, nranks = 1;
  double *d_recv = nullptr;    // receive buffer of the per-step all-gather: nranks slots
  size_t recv_doubles = 0;
};

void comm_get_unique_id(void *id);
Comm *comm_create(int device, const void *id, int rank, int nranks);
void comm_destroy(Comm *c);
// recv holds c.nranks slots of `count` doubles, slot c.rank already written by this rank: after the call (ordered on
// `st`) every slot holds its rank's data.  One ncclAllGather, in place.
void comm_allgather_inplace(Comm &c, double *recv, size_t count, hipStream_t st);
// the receive buffer, grown to at least `doubles` (device-synchronising when it grows)
double *comm_recv(Comm &c, size_t doubles);

}  // namespace bartrt
