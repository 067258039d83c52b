// Scratch that outlives a call: what the slab-parallel statistics over a row-major matrix x[nrows][ld] (quant.hip,
// hist.hip) share on the host side -- the reuse rule, the host forms' upload and the two settings.
//
// REUSE.  A state serves one call at a time.  Its buffers are touched by the state's own calls only, and every call
// either ends in record() or in a full wait for its stream; so the event stands for all device work on the scratch,
// and a host wait for it (wait()) is enough before a buffer is regrown or pinned staging memory is rewritten -- no
// device-wide synchronise.
#pragma once
#include <stdexcept>
#include <string>

#include "devbuf.hpp"

namespace bartrt {

struct Scratch {
  hipEvent_t done = nullptr;       // the end of the latest call that recorded one (made by the first record())
  bool pending = false;            // ... and the host has not waited for it since
  hipStream_t stream = nullptr;    // that call's stream
  int device = -1;                 // the device the state lives on (on_current_device)
  long slab_rows = 0, chunk_rows = 0;   // rows per workgroup, rows per chunk (0: the feature's default)
  DevBuf<double> x;                // the host forms' matrix and mask
  DevBuf<unsigned char> ok;
  ~Scratch() { if (done) (void)hipEventDestroy(done); }

  // a new call on st comes after the previous one: the same stream orders them itself; for another stream the host
  // waits (not hipStreamWaitEvent: the one run with it died in the runtime, after a call on hipStreamLegacy)
  void after_previous(hipStream_t st) { if (st != stream) wait(); }
  // the host waits for the previous call
  void wait() {
    if (pending) HIPCHK(hipEventSynchronize(done));
    pending = false;
  }
  // the end of a call on st
  void record(hipStream_t st) {
    if (!done) HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HIPCHK(hipEventRecord(done, st));
    pending = true;
    stream = st;
  }
  // room for n elements; the previous call may still read a buffer that has to grow
  template <class T>
  void room(DevBuf<T> &b, size_t n) {
    if (b && n <= b.count()) return;
    wait();
    b.reserve(n);
  }
  // a host matrix through x / ok on st in chunks of `rows` rows, each handed to each(d_x, n, d_ok); `width` columns of
  // a row are read
  template <class F>
  void upload_chunks(const double *hx, long nrows, long ld, long width, const unsigned char *hok, long rows,
                     hipStream_t st, F &&each) {
    room(x, (size_t)(rows - 1) * ld + width);
    if (hok) room(ok, (size_t)rows);
    for (long off = 0; off < nrows; off += rows) {
      const long n = std::min(rows, nrows - off);
      // (the last row is read up to its last column wanted: the caller's array may end there)
      HIPCHK(hipMemcpyAsync(x, hx + (size_t)off * ld, sizeof(double) * ((size_t)(n - 1) * ld + width), hipMemcpyHostToDevice, st));
      if (hok) HIPCHK(hipMemcpyAsync(ok, hok + off, (size_t)n, hipMemcpyHostToDevice, st));
      each(x.get(), n, hok ? ok.get() : nullptr);
    }
  }
  // a setting from its setter `who`: 0 (the default) .. most, or any number from 0 without one
  static void set_rows(long &knob, const char *who, long rows, long most = 0) {
    if (rows < 0 || (most && rows > most))
      throw std::invalid_argument(std::string(who) + ": rows = " + std::to_string(rows) +
                                  (most ? " is outside 0.." + std::to_string(most) : " is negative"));
    knob = rows;
  }
};

// *s for a call on the current device: a state made on another device is waited for and freed, and one with its
// settings starts over here (a state an engine owns lives and dies with the engine's device and needs none of this)
template <class S>
S &on_current_device(S *&s) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev == s->device) return *s;
  s->wait();
  S *fresh = new S;
  fresh->device = dev;
  fresh->slab_rows = s->slab_rows;
  fresh->chunk_rows = s->chunk_rows;
  delete s;
  return *(s = fresh);
}

}  // namespace bartrt
