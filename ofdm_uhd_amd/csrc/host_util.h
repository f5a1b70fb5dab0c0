// host_util.h -- host-side plumbing of the engine: error handling, grow-only device
// buffers, pinned staging, HIP-event profiling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/ofdm_hip.h"

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

// What the ten wideband stream stages (DDC, DDC bank, channeliser, DUC, DUC bank, synthesis bank, both resamplers, both resampler banks)
// share on the host: where the stream stands, the carried history and its double buffer, the host-mode staging buffers
// and the HIP-event pair of the last call.  Each stage's state derives from it and adds its own rates, tables and
// output format; the code that works on these fields is engine_stage.inc.
struct StreamStage {
  bool on = false;
  uint64_t next = 0;  // absolute index of the next input sample
  int cur = 0;        // d_hist[cur] holds the `hist` samples before `next`
  int hist = 0;       // samples of history a call reaches back: ntaps - 1 (DDC, bank), Q = (ntaps - 1) / L (the others)
  DevBuf d_hist[2], d_in, d_out;
  DevBuf d_add;        // the transmit stages: host mode's copy of the band a call adds onto
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  double last_ms = 0.0;
  bool timed = false;  // last_ms is of the stage's last call
  void release() {
    d_hist[0].release();
    d_hist[1].release();
    d_in.release();
    d_out.release();
    d_add.release();
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
    ev_a = ev_b = nullptr;
  }
};

// What the coded-link calls (the K = 7 code with its punctured rates and soft output, the Reed-Solomon outer code, LDPC)
// share on the host: the host-mode staging buffers, the batch's block table on the device, and the HIP-event pair and
// time of the last call (CodecClock: the outer code keeps a second one for ofdm_rs_rel_from_soft).  Each codec's state
// derives from it and adds its own per-block outputs, tables and workspaces; the code that works on these fields is
// engine_codec.inc.
struct CodecClock {
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  double last_ms = 0.0;
  bool timed = false;  // last_ms is of the codec's last call
  void release() {
    if (ev_a) (void)hipEventDestroy(ev_a);
    if (ev_b) (void)hipEventDestroy(ev_b);
    ev_a = ev_b = nullptr;
  }
};
struct CodecStage : CodecClock {
  DevBuf d_in, d_out, d_blk;
  void release() {
    d_in.release();
    d_out.release();
    d_blk.release();
    CodecClock::release();
  }
};

struct ProfSpan {
  int kernel;
  hipEvent_t a, b;
  bool busy;
};

// Per-kernel HIP-event timing.  Spans may sit on different streams (the transmit and receive sides of a handle run
// on their own): collect() takes the spans whose end event has completed and leaves the others for a later call.
struct Profiler {
  bool on = false;
  double total_ms[OFDM_K_COUNT] = {0};
  uint64_t launches[OFDM_K_COUNT] = {0};
  std::vector<ProfSpan> pool;  // events, reused call after call
  int open = -1;               // span begun and not yet ended

  void begin(int k, hipStream_t s) {
    if (!on) return;
    int idx = -1;
    for (size_t i = 0; i < pool.size(); i++)
      if (!pool[i].busy) {
        idx = (int)i;
        break;
      }
    if (idx < 0) {
      ProfSpan sp;
      sp.kernel = k;
      sp.busy = false;
      (void)hipEventCreate(&sp.a);
      (void)hipEventCreate(&sp.b);
      pool.push_back(sp);
      idx = (int)pool.size() - 1;
    }
    pool[idx].kernel = k;
    pool[idx].busy = true;
    (void)hipEventRecord(pool[idx].a, s);
    open = idx;
  }
  void end(hipStream_t s) {
    if (!on || open < 0) return;
    (void)hipEventRecord(pool[open].b, s);
    open = -1;
  }
  void collect() {
    for (size_t i = 0; i < pool.size(); i++) {
      if (!pool[i].busy || (int)i == open) continue;
      if (hipEventQuery(pool[i].b) != hipSuccess) continue;  // still running (another stream): next time
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pool[i].a, pool[i].b) == hipSuccess) {
        total_ms[pool[i].kernel] += (double)ms;
        launches[pool[i].kernel] += 1;
      }
      pool[i].busy = false;
    }
  }
  void reset() {
    for (int i = 0; i < OFDM_K_COUNT; i++) {
      total_ms[i] = 0;
      launches[i] = 0;
    }
    for (auto& sp : pool) sp.busy = false;
    open = -1;
  }
  void destroy() {
    for (auto& sp : pool) {
      (void)hipEventDestroy(sp.a);
      (void)hipEventDestroy(sp.b);
    }
    pool.clear();
    open = -1;
  }
};

// A span that ends where its scope ends, whichever way the function is left; end() closes it earlier.  One span is
// open at a time (Profiler::open): scopes follow each other, they do not nest.
struct ProfScope {
  Profiler& prof;
  hipStream_t stream;
  bool open = true;
  ProfScope(Profiler& p, int kernel, hipStream_t s) : prof(p), stream(s) { prof.begin(kernel, s); }
  ProfScope(const ProfScope&) = delete;
  void end() {
    if (open) prof.end(stream);
    open = false;
  }
  ~ProfScope() { end(); }
};
