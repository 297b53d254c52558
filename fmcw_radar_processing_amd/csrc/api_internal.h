// api_internal.h -- what the host units of libfmcw share (fmcw_api.cpp, api_stft.cpp,
// api_stages.cpp): the error text, the checked-call macros, device and pinned buffers, the
// context, and the chunk / shard helpers of the host-pointer calls.
// Host only: never included by a kernels_*.hip.
#pragma once
#include "../../include/fmcw.h"
#include "fmcw_internal.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace fmcw {

// Sets the calling thread's fmcw_last_error text and returns code (fmcw_api.cpp: the one
// thread-local string of the library).
int fail(int code, const std::string& msg);

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return fail(FMCW_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define CHK(expr)            \
  do {                       \
    int r_ = (expr);         \
    if (r_ != FMCW_OK) return r_; \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  int ensure(size_t bytes) {
    if (bytes <= n && p) return FMCW_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (bytes == 0) bytes = 16;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(FMCW_E_OOM, "hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    n = bytes;
    return FMCW_OK;
  }
  template <typename T> T* as() const { return static_cast<T*>(p); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// Offsets of several arrays packed into one buffer (256-byte aligned).
struct Arena {
  size_t off = 0;
  size_t add(size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

// Page-locked host staging buffer (DMA source / target of the host-pointer calls).
struct PinBuf {
  void* p = nullptr;
  size_t n = 0;
  int ensure(size_t bytes) {
    if (bytes <= n && p) return FMCW_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    if (bytes == 0) bytes = 16;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(FMCW_E_OOM, "hipHostMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    n = bytes;
    return FMCW_OK;
  }
  char* at(size_t off) const { return static_cast<char*>(p) + off; }
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
};

// Host memcpy between the caller's (pageable) arrays and the pinned slots, split over a few
// threads (fmcw_api.cpp).
void par_memcpy(void* dst, const void* src, size_t n);

inline size_t esize(int dtype) { return dtype == FMCW_C32H ? 4 : 8; }

// RCCL, resolved at run time (fmcw_api.cpp): a single-device context never needs it, and a
// process that already holds an RCCL (torch's) shares that copy.
struct Rccl {
  ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*group_start)() = nullptr;
  ncclResult_t (*group_end)() = nullptr;
  const char* (*error_string)(ncclResult_t) = nullptr;
  bool ok = false;
};
const Rccl& rccl();

#define NCCLCHK(expr)                                                                     \
  do {                                                                                    \
    ncclResult_t r_ = (expr);                                                             \
    if (r_ != ncclSuccess) return fail(FMCW_E_HIP, std::string(#expr) + ": " + rccl().error_string(r_)); \
  } while (0)

// contiguous shard [f0, f0 + n) of `total` items for member g of `world` (dist.py shard_range)
inline void shard(int64_t total, int g, int world, int64_t& f0, int64_t& n) {
  const int64_t base = total / world, rem = total % world;
  f0 = g * base + std::min<int64_t>(g, rem);
  n = base + (g < rem ? 1 : 0);
}

constexpr int kStages = 20;  // 0..6 per kernel (see fmcw.h), 7 range+Doppler span per call, 8 k_rdx, 9 render, 10 cfar, 11 cluster, 12 track, 13 mti, 14 aoa, 15 beam, 16 oscfar, 17 ra, 18 music, 19 doa
constexpr int kStagesRead = 19;  // fmcw_timing_read answers for 0..18 only (fmcw.h); fmcw_timing_read_ext for all

}  // namespace fmcw

using namespace fmcw;   // the host units name the above unqualified

struct fmcw_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // software pipeline over chunks: K1 (range) on the caller's stream, K2
  // (Doppler) on sd, K3 (detect) on sx; chunk i's K2 overlaps chunk i+1's K1
  static constexpr int kSlots = 3;
  hipStream_t sd = nullptr, sx = nullptr;
  hipEvent_t ev_k1[kSlots] = {}, ev_k2[kSlots] = {}, ev_k3[kSlots] = {};
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool taps = false;
  fmcw_params p{};
  DevBuf cal, calw, wd, tw_nr, tw_nd;
  std::vector<float> h_wr, h_cal;   // host copies to rebuild calw when IF_scale changes
  float calw_scale = 0.f;
  float2 cal_sum{0.f, 0.f};
  DevBuf scratch_cube, scratch_rd;
  // host-pointer API staging: device slots and page-locked host slots, two of
  // each, so chunk i+1's H2D copy (stream cin) and chunk i-1's D2H copy (cout)
  // run under chunk i's kernels (the caller's data is copied into the pinned
  // slots by host threads meanwhile)
  DevBuf h_iq, h_prof, h_rd;
  PinBuf pin_in, pin_out;
  // small per-call arrays of the host-pointer calls, packed so that they cross PCIe as ONE copy
  // (each pageable copy costs ~20-30 us of latency: six of them were half of a deployed call)
  DevBuf h_small, s_in;
  PinBuf pin_small, pin_sin;
  hipStream_t cin = nullptr, cout = nullptr;
  hipEvent_t ev_h2d[2] = {}, ev_comp[2] = {}, ev_d2h[2] = {};
  DevBuf s_P, s_pmax, s_nseg, s_lidx, s_lw, s_out;
  DevBuf s_cbins, s_segmax, s_tiles;   // fmcw_stft's coarse-to-fine max(P) (stft_coarse_max)
  DevBuf r_q, r_nseg, r_img;                   // spectrogram.png render (device 0)
  // Device scratch kept per stream: device calls on different streams (with different windows,
  // nfft or frame counts) never share one.  At most kPerStream streams per kind (a caller that
  // passes a fresh stream per call does not grow device memory): the least recently used entry is
  // taken over, and the new stream first waits for the event recorded behind the old owner's last
  // readers (done()), so its rewrite cannot overtake them -- the event outlives a destroyed stream.
  struct PerStream {
    struct Entry {
      hipStream_t s = nullptr;
      DevBuf t;
      hipEvent_t done = nullptr;
      uint64_t tick = 0;
      const void* key = nullptr;   // what the contents were built from (STFT tables: the window pointer)
      int64_t key_n = 0;           // and its size (the nfft)
      ~Entry() {
        if (done) (void)hipEventDestroy(done);
      }
    };
    static constexpr size_t kPerStream = 8;
    std::vector<std::unique_ptr<Entry>> es;
    uint64_t tick = 0;
    void* get(hipStream_t st, size_t bytes, int* status, bool* fresh = nullptr) {
      Entry* e = nullptr;
      for (auto& x : es)
        if (x->s == st) e = x.get();
      if (!e && es.size() < kPerStream) {
        es.push_back(std::make_unique<Entry>());
        e = es.back().get();
        e->s = st;
      } else if (!e) {
        e = es[0].get();
        for (auto& x : es)
          if (x->tick < e->tick) e = x.get();
        if (e->done && hipStreamWaitEvent(st, e->done, 0) != hipSuccess) {
          (void)hipGetLastError();
          *status = fail(FMCW_E_HIP, "per-stream scratch: hipStreamWaitEvent failed");
          return nullptr;
        }
        e->s = st;
        e->key = nullptr;
        e->key_n = 0;
      }
      e->tick = ++tick;
      void* before = e->t.p;
      *status = e->t.ensure(bytes);
      if (e->t.p != before) {                  // newly allocated: its contents are undefined
        e->key = nullptr;
        e->key_n = 0;
      }
      if (fresh) *fresh = e->t.p != before;
      last = e;
      return e->t.p;
    }
    Entry* last = nullptr;                     // the entry the last get() returned
    // after the kernels that read stream st's entry are enqueued
    int done(hipStream_t st) {
      for (auto& x : es) {
        if (x->s != st) continue;
        if (!x->done && hipEventCreateWithFlags(&x->done, hipEventDisableTiming | fmcw::kEvDevice) != hipSuccess) {
          (void)hipGetLastError();
          return fail(FMCW_E_HIP, "per-stream scratch: hipEventCreate failed");
        }
        if (hipEventRecord(x->done, st) != hipSuccess) {
          (void)hipGetLastError();
          return fail(FMCW_E_HIP, "per-stream scratch: hipEventRecord failed");
        }
      }
      return FMCW_OK;
    }
  };
  // STFT 20-tap tables W[nfft/2+1][20] + the 20 taps they were built from, one per stream that
  // asked for one (stft_tab, stft_tab64: fmcw_api.cpp)
  PerStream s_tabs;
  static constexpr size_t STFT_TAPS_BYTES = 20 * 4;
  float2* stft_tab(hipStream_t st, size_t bytes, int* status);
  float2* stft_tab64(hipStream_t st, const float* d_win, int nfft, bool* build, int* status);
  int stft_tab_done(hipStream_t st) { return s_tabs.done(st); }
  // K1's per-workgroup profile maxima of fmcw_range_fft_device (config 2), one per stream: two
  // range-only calls on different streams of one context do not write over each other's partials
  PerStream k1_part;
  // k_detect_1p's arrival counter of the fused compaction (fmcw_process_slow_device), one per
  // stream; zeroed when allocated, reset by the kernel's last workgroup
  PerStream det_done;
  // fmcw_cfar_device's per-wave detection lists and counts, one per stream
  PerStream cfar_scr;
  // fmcw_cfar (host pointers): the RD chunk, the per-frame outputs and the mask chunk on the device
  DevBuf cf_in, cf_out, cf_mask;
  // fmcw_sig_device's per-slab column sums, one per stream
  PerStream sig_scr;
  // fmcw_sig (host pointers): the RD chunk, the centres, and both maps with their two maxima on the device
  DevBuf sg_in, sg_ctr, sg_out;
  // fmcw_cluster (host pointers): the chunk's detection lists and the per-frame outputs on the device
  DevBuf cl_in, cl_out;
  // fmcw_aoa (host pointers): the chunk's frames of every channel, the chunk's lists and the per-frame outputs on the device
  DevBuf ao_rd, ao_in, ao_out;
  // fmcw_track (host pointers): the chunk's target rows, the chunk's outputs and the sequences' state on the device
  DevBuf tk_in, tk_out, tk_state;
  // fmcw_mti (host pointers): the chunk's frames (filtered in place) and the sequences' state on the device
  DevBuf mt_rd, mt_bg, mt_seen;
  // fmcw_beam (host pointers): the chunk's frames of every channel and of every output on the device
  DevBuf bm_rd, bm_out;
  // fmcw_ra (host pointers): the chunk's frames of every channel, its covariances and its spectra, and the
  // weight table with the running maximum on the device
  DevBuf ra_rd, ra_cov, ra_out, ra_w;
  // fmcw_music (host pointers): the chunk's covariances, its four outputs, and the weight table with the
  // running maximum on the device
  DevBuf mu_cov, mu_eval, mu_evec, mu_nsrc, mu_out, mu_w;
  // fmcw_doa (host pointers): the chunk's spectra, the grid and the chunk's five outputs
  DevBuf doa_spec, doa_u, doa_count, doa_idx, doa_pow, doa_sin, doa_base;
  int64_t chunk_frames = 0;
  int64_t last_coarse_tiles = -1;     // tiles the last coarse-to-fine max(P) evaluated in full (diagnostics)
  int pipe_mode = FMCW_PIPE_AUTO;
  DevBuf op_rowpk, op_cidx, op_crows;           // single-pass schedule scratch (per chunk)
  DevBuf x_cube, x_ctr, x_err, x_tab;          // XCD-team schedule: hand-off slots, counters, sticky error, XT_* table
  DevBuf x_clk;                                // k_rdx's clock stamps of its last launch (fmcw_rdx_clock)
  int xcd_teams = -1;                          // census of the device: its XCD teams (-1 not run yet, 0 none)
  int8_t xcc_team[16] = {};                    // HW_REG_XCC_ID -> team
  bool xcd_used = false;                       // a k_rdx launch since the last error check
  int x_ctr_set = 0;                           // the counter set (0 / 1) of x_ctr the next k_rdx launch counts in
  bool x_tab_ok = false;                       // x_tab built for the current taps
  // Multi-device context (fmcw_ctx_create with n_devices > 1): this object is
  // device 0 of the context and peers[i] a full context on device i + 1.  The
  // host-pointer calls shard their frames (fmcw_process, fmcw_range_fft) or
  // spectrogram segments (fmcw_stft) over all of them; the device-pointer
  // calls act on device 0.  comms: one RCCL communicator per device
  // (ncclCommInitAll) when the device ids are distinct.
  std::vector<fmcw_ctx*> peers;
  std::vector<ncclComm_t> comms;
  int timing = 0;                    // 0 off, 1 range+Doppler span + STFT launches, 2 + every K1/K2/K3
  struct Pending {
    hipEvent_t a, b;
    int stage;
  };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  double total_ms[kStages] = {};
  int64_t launches[kStages] = {};

  ~fmcw_ctx();

  hipEvent_t get_event() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, fmcw::kEvDevice) != hipSuccess) return nullptr;   // timing pairs
    return e;
  }
};

namespace fmcw {

// Record an event pair around one launch when timing is enabled.
struct StageTimer {
  fmcw_ctx* c;
  int stage;
  hipStream_t s;
  hipEvent_t a = nullptr;
  StageTimer(fmcw_ctx* c_, int st, hipStream_t s_, int level = 1) : c(c_), stage(st), s(s_) {
    // level 3: only the dominant kernels' launches (k_rdx, stage 8; K1 range-only, stage 6):
    // every event pair on the stream costs the step a few microseconds
    const bool on = c->timing == 3 ? (st == 6 || st == 8) : c->timing >= level;
    if (on) {
      a = c->get_event();
      if (a) (void)hipEventRecord(a, s);
    }
  }
  void done() {
    if (a) {
      hipEvent_t b = c->get_event();
      if (b) {
        (void)hipEventRecord(b, s);
        c->pending.push_back({a, b, stage});
      }
      a = nullptr;
    }
  }
};

inline int set_device(fmcw_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  return FMCW_OK;
}

inline hipStream_t pick(fmcw_ctx* c, void* stream) { return stream ? static_cast<hipStream_t>(stream) : c->stream; }

// Frames per host-path chunk: ~64 MiB of input per slot (FMCW_HOST_CHUNK
// overrides, for tests of the chunk seams).
inline int64_t host_chunk(size_t frame_in_bytes, int64_t F) {
  int64_t fc = (int64_t)((64ull << 20) / std::max<size_t>(frame_in_bytes, 1));
  if (const char* e = std::getenv("FMCW_HOST_CHUNK"); e && std::atoll(e) > 0) fc = std::atoll(e);
  return std::max<int64_t>(1, std::min<int64_t>(fc, F));
}

// Run fn(device context, shard index, f0, n) on every device of the context,
// one host thread per device (their H2D copies, kernels and D2H copies then
// overlap), over contiguous shards of `total` items.  The first failing
// device's status and message are returned (the message is the worker thread's own
// fmcw_last_error, copied out before the thread ends).
template <typename Fn>
int over_devices(fmcw_ctx* c, int64_t total, Fn&& fn) {
  const int world = 1 + (int)c->peers.size();
  if (world == 1) return fn(c, 0, (int64_t)0, total);
  std::vector<int> st(world, FMCW_OK);
  std::vector<std::string> msg(world);
  std::vector<std::thread> th;
  for (int g = 0; g < world; ++g) {
    th.emplace_back([&, g] {
      int64_t f0, n;
      shard(total, g, world, f0, n);
      fmcw_ctx* d = g == 0 ? c : c->peers[g - 1];
      st[g] = n > 0 ? fn(d, g, f0, n) : FMCW_OK;
      if (st[g] != FMCW_OK) msg[g] = fmcw_last_error();
    });
  }
  for (auto& t : th) t.join();
  for (int g = 0; g < world; ++g)
    if (st[g] != FMCW_OK) return fail(st[g], "device " + std::to_string(g) + ": " + msg[g]);
  return FMCW_OK;
}

}  // namespace fmcw
