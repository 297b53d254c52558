// kernels_beam.hip -- combine the receive channels' range-Doppler maps into beamformed or
// channel-integrated maps, for gfx950.
//
// Definition (include/fmcw.h, fmcw_beam_params): A channel maps in, B maps out, all [F][nr][nd] of one
// dtype.  One cell, in float32, x_a the stored value of channel a (fp16 storage widened exactly),
// w = w[b][a]:  t_a.re = x.re w.re - x.im w.im,  t_a.im = x.re w.im + x.im w.re.
//   coherent   y = t_0, then y.re = y.re + t_a.re, y.im = y.im + t_a.im for a = 1..A-1 in ascending a;
//              out[b] = y (fp16 storage: round to nearest even, subnormals kept, overflow to inf).
//   NCI        with w[0][a]: p = (t_0.re^2 + t_0.im^2), then p = p + (t_a.re^2 + t_a.im^2) in ascending
//              a; out[0].re = sqrtf(p), correctly rounded, out[0].im = +0.
// Every operation is rounded on its own: the pragma below keeps the compiler from contracting a
// multiply and an add into one FMA, which rounds once.
//
// k_beam  A streaming kernel: every map is read once and every output written once.  The F frames of
//   a map follow each other, so a map is one run of F * (frame bytes / 16) 16-byte pieces.  A lane owns
//   the same piece (2 complex64 cells, 4 fp16-storage cells) of all A inputs and all B outputs: it
//   issues its A loads together (they do not depend on each other and are all in flight), widens
//   them, forms the B results one beam after the other and stores B pieces.  Grid: one thread per
//   piece in 256-thread blocks.  Loads and stores of the maps are nontemporal (touched once, far
//   larger than any cache).  The pointers and weights arrive by value in the kernel arguments.  The
//   kernel is templated on A, so the loaded values and the input pointers are indexed by constants;
//   the loop over the possible 8 beams carries a uniform guard, and beam b's weights and output
//   pointer are uniform reads of the kernel arguments into scalar registers: no scratch.
//   No LDS, no barrier, no atomics, no inline assembly; every store is an ordinary vector store.
//
// In place (out[b] == rd[a] for any a, b) is safe by construction: a lane loads its piece of all A
//   inputs before its first store (the maps are not declared restrict, so the compiler keeps that
//   order), and it stores only to the piece index it has itself loaded.  No other lane ever reads or
//   writes that piece index of any map, so no lane can see another's output.  The host refuses every
//   partial overlap, where the same bytes would be different piece indices of two maps.
//
// Addresses are formed from blockIdx, threadIdx, the frame offset of the launch and the arguments
// alone, never from data; a lane past the last piece leaves at once.  Piece offsets are 64-bit.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#pragma clang fp contract(off)

namespace fmcw {

namespace {

typedef float bm_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 bm_h8 __attribute__((ext_vector_type(8)));

// one 16-byte piece as floats: 4 (complex64: 2 cells) or 8 (fp16 storage: 4 cells)
template <bool H>
struct BmCells {
  static constexpr int N = H ? 8 : 4;
};

template <bool H>
__device__ inline void bm_widen(const bm_f4 v, float (&x)[BmCells<H>::N]) {
  if constexpr (H) {
    const bm_h8 h = __builtin_bit_cast(bm_h8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (float)h[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = v[j];
  }
}

template <bool H>
__device__ inline bm_f4 bm_narrow(const float (&y)[BmCells<H>::N]) {
  if constexpr (H) {
    bm_h8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (_Float16)y[j];   // round to nearest even, subnormals kept, overflow to inf
    return __builtin_bit_cast(bm_f4, h);
  } else {
    bm_f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = y[j];
    return v;
  }
}

template <bool H, int A, bool NCI>
__global__ __launch_bounds__(256) void k_beam(const BeamArgs a) {
  constexpr int N = BmCells<H>::N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // this lane's 16-byte piece of the launch
  if (i >= a.n16) return;

  bm_f4 v[A];
#pragma unroll
  for (int ch = 0; ch < A; ++ch) v[ch] = __builtin_nontemporal_load(static_cast<const bm_f4*>(a.rd[ch]) + i);
  float x[A][N];
#pragma unroll
  for (int ch = 0; ch < A; ++ch) bm_widen<H>(v[ch], x[ch]);

  if constexpr (NCI) {
    float y[N];
#pragma unroll
    for (int c = 0; c < N; c += 2) {
      float p = 0.f;
#pragma unroll
      for (int ch = 0; ch < A; ++ch) {
        const float wr = a.w[0][ch][0], wi = a.w[0][ch][1];
        const float xr = x[ch][c], xi = x[ch][c + 1];
        const float tr = xr * wr - xi * wi;
        const float ti = xr * wi + xi * wr;
        const float m = tr * tr + ti * ti;
        p = ch == 0 ? m : p + m;
      }
      y[c] = sqrtf(p);                                       // correctly rounded (hipcc's default for fp32)
      y[c + 1] = 0.f;
    }
    __builtin_nontemporal_store(bm_narrow<H>(y), static_cast<bm_f4*>(a.out[0]) + i);
  } else {
#pragma unroll
    for (int b = 0; b < kBeamMax; ++b) {
      if (b < a.B) {                                           // uniform
        float y[N];
#pragma unroll
        for (int ch = 0; ch < A; ++ch) {
          const float wr = a.w[b][ch][0], wi = a.w[b][ch][1];
#pragma unroll
          for (int c = 0; c < N; c += 2) {
            const float xr = x[ch][c], xi = x[ch][c + 1];
            const float tr = xr * wr - xi * wi;
            const float ti = xr * wi + xi * wr;
            y[c] = ch == 0 ? tr : y[c] + tr;
            y[c + 1] = ch == 0 ? ti : y[c + 1] + ti;
          }
        }
        __builtin_nontemporal_store(bm_narrow<H>(y), static_cast<bm_f4*>(a.out[b]) + i);
      }
    }
  }
}

template <bool H, int A>
void bm_launch(const BeamArgs& a, unsigned blocks, hipStream_t s) {
  if (a.nci) hipLaunchKernelGGL((k_beam<H, A, true>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_beam<H, A, false>), dim3(blocks), dim3(256), 0, s, a);
}

template <bool H>
void bm_launch_chan(const BeamArgs& a, unsigned blocks, hipStream_t s) {
  switch (a.A) {
    case 2: bm_launch<H, 2>(a, blocks, s); break;
    case 3: bm_launch<H, 3>(a, blocks, s); break;
    case 4: bm_launch<H, 4>(a, blocks, s); break;
    case 5: bm_launch<H, 5>(a, blocks, s); break;
    case 6: bm_launch<H, 6>(a, blocks, s); break;
    case 7: bm_launch<H, 7>(a, blocks, s); break;
    default: bm_launch<H, 8>(a, blocks, s); break;
  }
}

}  // namespace

hipError_t launch_beam(const BeamArgs& a, hipStream_t s) {
  if (a.n16 <= 0) return hipSuccess;
  if (a.A < 2 || a.A > kBeamMax || a.B < 1 || a.B > kBeamMax || (a.nci && a.B != 1)) return hipErrorInvalidValue;
  for (int ch = 0; ch < a.A; ++ch)
    if (!a.rd[ch] || (reinterpret_cast<uintptr_t>(a.rd[ch]) & 15)) return hipErrorInvalidValue;
  for (int b = 0; b < a.B; ++b)
    if (!a.out[b] || (reinterpret_cast<uintptr_t>(a.out[b]) & 15)) return hipErrorInvalidValue;
  if (a.n16 > ((int64_t)1 << 31)) return hipErrorInvalidValue;   // the grid stays below 2^32 threads
  const int64_t blocks = (a.n16 + 255) / 256;
  if (a.h) bm_launch_chan<true>(a, (unsigned)blocks, s);
  else bm_launch_chan<false>(a, (unsigned)blocks, s);
  return hipGetLastError();
}

}  // namespace fmcw
