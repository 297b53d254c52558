// kernels_mti.hip -- frame-to-frame clutter filter (MTI) of the range-Doppler map, for gfx950.
//
// Definition (include/fmcw.h, fmcw_mti_params): per sequence a complex float32 background B per RD
// cell and a frame counter `seen`.  One frame step per cell, re and im apart, in float32: x the stored
// value (fp16 storage widened exactly), y = x - B the output (fp16 storage: round to nearest even,
// subnormals kept); then, unless FREEZE, g = RAMP ? max(lambda, 1 / (n + 1)) : lambda with
// n = clamp(seen, 0, 2^30), B = x when g == 1, else t = g * y, B = B + t; n + 1 saturates at 2^30.
// Every operation is rounded on its own: the pragma below keeps the compiler from contracting the
// multiply and the add into one FMA, which rounds once.
//
// k_mti  A streaming kernel: the map is read once and written once.  A lane owns the same 16 bytes
//   (2 complex64 cells, 4 fp16-storage cells) of every frame of its sequence, holds their B in
//   registers for the whole launch -- read once before the first frame, written once after the last
//   -- and walks the F frames in order.  Grid: S x the 256-thread blocks of one frame.
//   The recursion is a dependency chain per cell, the loads are not: frame f + U does not depend on
//   B.  A ring of U 16-byte loads per lane stays in flight; the frames are walked in groups of U with
//   the ring indexed by compile-time constants (a runtime ring index would put it in scratch).  The
//   main loop runs while every prefetch of a group is in range, so its loads are unconditional; behind
//   it the ring is drained (up to U frames) and the last < U frames are loaded and stepped one by one
//   (guarded prefetches in an unrolled tail cost 3x the registers and spilled at U = 8).
//   Loads and stores of the map are nontemporal (touched once, far larger than any cache).
//   In place (out == rd): a lane stores only to addresses it has loaded from before.
//   out == nullptr: only the background is learned.
//   No LDS, no barrier, no atomics.
// k_mti_seen  seen[s] is read by every workgroup of sequence s, so no workgroup of k_mti writes it:
//   this second, tiny launch behind k_mti on the same stream advances it.
//
// Addresses are formed from blockIdx, threadIdx, f and the arguments alone, never from data; a lane
// beyond the frame's last 16 bytes leaves at once.  Frame offsets are 64-bit.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#pragma clang fp contract(off)

namespace fmcw {

namespace {

typedef float mt_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 mt_h8 __attribute__((ext_vector_type(8)));

constexpr int kMtiSeenMax = 1 << 30;

// cells of one 16-byte piece as floats: 4 (complex64) or 8 (fp16 storage)
template <bool H>
struct MtCells {
  static constexpr int N = H ? 8 : 4;
};

template <bool H>
__device__ inline void mt_widen(const mt_f4 v, float (&x)[MtCells<H>::N]) {
  if constexpr (H) {
    const mt_h8 h = __builtin_bit_cast(mt_h8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (float)h[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = v[j];
  }
}

template <bool H>
__device__ inline mt_f4 mt_narrow(const float (&y)[MtCells<H>::N]) {
  if constexpr (H) {
    mt_h8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (_Float16)y[j];   // round to nearest even, subnormals kept
    return __builtin_bit_cast(mt_f4, h);
  } else {
    mt_f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = y[j];
    return v;
  }
}

// OUT: the filtered map is written.  The flags are uniform values folded into selects, so the
// frame step is straight-line code and the waits for the ring's loads can be counted.
template <bool H, int U, bool OUT>
__global__ __launch_bounds__(256) void k_mti(const MtiArgs a) {
  constexpr int N = MtCells<H>::N;
  const unsigned sq = blockIdx.x / (unsigned)a.bpf;
  const int64_t s = sq;
  const int64_t i = (int64_t)(blockIdx.x - sq * (unsigned)a.bpf) * 256 + threadIdx.x;   // this lane's 16-byte piece of a frame
  if (i >= a.n16) return;
  const int64_t F = a.F;
  const int64_t fstride = a.n16;                                         // in 16-byte pieces
  const mt_f4* const src = static_cast<const mt_f4*>(a.rd) + (s * F) * fstride + i;
  mt_f4* const dst = OUT ? static_cast<mt_f4*>(a.out) + (s * F) * fstride + i : nullptr;
  mt_f4* const bgp = reinterpret_cast<mt_f4*>(a.bg) + (s * a.n16 + i) * (N / 4);
  const bool freeze = a.freeze != 0, ramp = a.ramp != 0;
  const float lambda = a.lambda;

  float B[N];
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const mt_f4 v = bgp[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) B[4 * q + j] = v[j];
  }
  int n = min(max(a.seen[s], 0), kMtiSeenMax);

  auto step = [&](const mt_f4 v, int64_t f) {
    float x[N], y[N];
    mt_widen<H>(v, x);
#pragma unroll
    for (int j = 0; j < N; ++j) y[j] = x[j] - B[j];
    if constexpr (OUT) __builtin_nontemporal_store(mt_narrow<H>(y), dst + f * fstride);
    const float r = 1.0f / (float)(n + 1);                 // correctly rounded (hipcc's default for fp32)
    const float g = ramp ? fmaxf(lambda, r) : lambda;
    const bool take = g == 1.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float t = g * y[j];
      const float b = B[j] + t;
      B[j] = freeze ? B[j] : take ? x[j] : b;
    }
    n = min(n + 1, kMtiSeenMax);
  };

  mt_f4 ring[U] = {};
  if (F >= U) {
#pragma unroll
    for (int k = 0; k < U; ++k) ring[k] = __builtin_nontemporal_load(src + (int64_t)k * fstride);
  } else {
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (k < F) ring[k] = __builtin_nontemporal_load(src + (int64_t)k * fstride);
  }

  int64_t f0 = 0;
#pragma unroll 1
  for (; f0 + 2 * U <= F; f0 += U) {                       // every prefetch of the group is in range
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const mt_f4 v = ring[k];
      ring[k] = __builtin_nontemporal_load(src + (f0 + k + U) * fstride);
      step(v, f0 + k);
    }
  }
#pragma unroll
  for (int k = 0; k < U; ++k) {                            // drain the ring
    const int64_t f = f0 + k;
    if (f < F) step(ring[k], f);
  }
#pragma unroll 1
  for (int64_t f = f0 + U; f < F; ++f) step(__builtin_nontemporal_load(src + f * fstride), f);

  if (!freeze) {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      mt_f4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = B[4 * q + j];
      bgp[q] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_mti_seen(int32_t* seen, int64_t S, int64_t F) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const int64_t n = min(max(seen[s], 0), kMtiSeenMax);
  seen[s] = (int32_t)min(n + F, (int64_t)kMtiSeenMax);
}

template <bool H, int U>
void mt_launch(const MtiArgs& a, int64_t blocks, hipStream_t s) {
  if (a.out) hipLaunchKernelGGL((k_mti<H, U, true>), dim3((unsigned)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_mti<H, U, false>), dim3((unsigned)blocks), dim3(256), 0, s, a);
}

template <bool H>
void mt_launch_ring(const MtiArgs& a, int64_t blocks, hipStream_t s) {
  switch (a.ring) {
    case 4: mt_launch<H, 4>(a, blocks, s); break;
    case 8: mt_launch<H, 8>(a, blocks, s); break;
    default: mt_launch<H, 16>(a, blocks, s); break;
  }
}

}  // namespace

bool mti_ring_ok(int ring) { return ring == 4 || ring == 8 || ring == 16; }

hipError_t launch_mti(const MtiArgs& a_in, hipStream_t s) {
  if (a_in.S <= 0 || a_in.F <= 0) return hipSuccess;
  MtiArgs a = a_in;
  if (a.n16 < 1 || !mti_ring_ok(a.ring) || !a.rd || !a.bg || !a.seen || (a.freeze && !a.out)) return hipErrorInvalidValue;
  if (a.n16 > ((int64_t)1 << 30) || a.S > 0x7fffffffLL) return hipErrorInvalidValue;
  a.bpf = (int)((a.n16 + 255) / 256);
  const int64_t blocks = a.S * a.bpf;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (a.h) mt_launch_ring<true>(a, blocks, s);
  else mt_launch_ring<false>(a, blocks, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.freeze) return e;
  hipLaunchKernelGGL(k_mti_seen, dim3((unsigned)((a.S + 255) / 256)), dim3(256), 0, s, a.seen, a.S, a.F);
  return hipGetLastError();
}

}  // namespace fmcw
