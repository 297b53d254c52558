// kernels_aoa.hip -- angle of arrival from several receive channels of the RD map, for gfx950.
//
// Definition (include/fmcw.h, fmcw_aoa_params): the first n = clamp(det_count[f], 0, max_det) entries
// of frame f's CFAR lists are the cells; cell i is valid iff 1 <= r <= nr and 1 <= d <= nd.  For a
// valid cell, in float32 with every operation rounded on its own (the pragma below keeps the
// compiler from contracting a multiply and an add into one FMA, which rounds once): v_a = x_a w_a,
// x_a the stored value of channel a at (r, d) (fp16 storage widened exactly), then over the adjacent
// pairs p = v_a, q = v_{a+1}: zr += q.re p.re + q.im p.im, zi += q.im p.re - q.re p.im,
// e0 += |p|^2, e1 += |q|^2.  Per cell: z (times scale2), phase = atan2f(zi, zr), sin = clamp(phase
// kinv, -1, 1).  Per target t (the valid cells whose det_label is t, 1 <= t <= max_tgt): the sums of
// (zr, zi, e0, e1) over its cells in ascending list position, phase and sin of the summed z, the
// coherence |z| / (sqrt(e0) sqrt(e1)) cut at 1, and the number of cells.
//
// k_aoa  One workgroup per frame (64 threads when max_det <= 64, else 256), so nothing depends on F.
//   1. Cells.  A thread per list position checks the indices, issues its A loads (8 bytes of a
//      complex64 map, 4 of an fp16-storage one; the lists are sorted by (r, d), so neighbouring lanes
//      often share a line), forms (zr, zi, e0, e1), writes the per-cell outputs and keeps the four
//      sums and the label in LDS.  The channel pointers arrive by value in the arguments and are only
//      ever indexed by compile-time constants (the loop over channels is unrolled), so they stay in
//      scalar registers.
//   2. Targets.  One wave per target walks the list 64 positions at a time, takes the members by a
//      ballot and adds them one by one in ascending position (every lane reads the member's sums from
//      LDS at one address, a broadcast), so the sums are the same bits on every call: no float
//      atomics.
//
// The only addresses formed from list content are those of the map cells, and only after
// 1 <= r <= nr and 1 <= d <= nd held: ((f nr + r - 1) nd + d - 1) elements into a channel of F nr nd
// elements.  Labels are only compared.  Every other address comes from blockIdx, threadIdx and list
// positions < max_det.  All stores are ordinary vector stores.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#include <hip/hip_fp16.h>

#pragma clang fp contract(off)

namespace fmcw {

namespace {

constexpr int kAoaMaxDet = 1024;
constexpr int kAoaMaxTgt = 64;

// the stored value of one channel at element e, as float32
__device__ inline float2 aoa_load(const void* ch, size_t e, bool h) {
  if (h) {
    const __half2 v = static_cast<const __half2*>(ch)[e];
    return make_float2(__low2float(v), __high2float(v));     // exact
  }
  return static_cast<const float2*>(ch)[e];
}

__device__ inline float aoa_phase(float zr, float zi) { return (zr == 0.f && zi == 0.f) ? 0.f : atan2f(zi, zr); }

__device__ inline float aoa_sin(float phase, float kinv) { return fminf(fmaxf(phase * kinv, -1.f), 1.f); }

__global__ __launch_bounds__(256) void k_aoa(const AoaArgs a) {
  extern __shared__ float4 aoa_lds[];
  const int K = a.K;
  float4* const s_z = aoa_lds;                               // [K] {zr, zi, e0, e1}, unscaled
  int* const s_lab = reinterpret_cast<int*>(s_z + K);        // [K] the cell's target 1..M, 0: none

  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t base = (size_t)f * K;
  const size_t fbase = (size_t)f * a.NR * a.ND;
  const int M = a.M;
  int n = a.det_count[f];
  n = __builtin_amdgcn_readfirstlane(min(max(n, 0), K));

  // 1. the cells
  for (int i = tid; i < K; i += nt) {
    float zr = 0.f, zi = 0.f, e0 = 0.f, e1 = 0.f;
    int lab = 0;
    if (i < n) {
      const int r = a.det_ridx[base + i], d = a.det_didx[base + i];
      if ((unsigned)(r - 1) < (unsigned)a.NR && (unsigned)(d - 1) < (unsigned)a.ND) {
        const size_t e = fbase + (size_t)(r - 1) * a.ND + (size_t)(d - 1);
        float2 x[kAoaChan];
#pragma unroll
        for (int c = 0; c < kAoaChan; ++c)
          if (c < a.A) x[c] = aoa_load(a.rd[c], e, a.h != 0);
        float2 p = make_float2(0.f, 0.f);
#pragma unroll
        for (int c = 0; c < kAoaChan; ++c)
          if (c < a.A) {
            const float wr = a.w[2 * c], wi = a.w[2 * c + 1];
            float2 q;
            q.x = x[c].x * wr - x[c].y * wi;
            q.y = x[c].x * wi + x[c].y * wr;
            if (c > 0) {
              zr += (q.x * p.x + q.y * p.y);
              zi += (q.y * p.x - q.x * p.y);
              e0 += (p.x * p.x + p.y * p.y);
              e1 += (q.x * q.x + q.y * q.y);
            }
            p = q;
          }
        if (a.det_label) {
          const int l = a.det_label[base + i];
          lab = (l >= 1 && l <= M) ? l : 0;
        }
      }
    }
    s_z[i] = make_float4(zr, zi, e0, e1);
    s_lab[i] = lab;
    const float ph = aoa_phase(zr, zi);
    if (a.det_zre) a.det_zre[base + i] = zr * a.scale2;
    if (a.det_zim) a.det_zim[base + i] = zi * a.scale2;
    if (a.det_phase) a.det_phase[base + i] = ph;
    if (a.det_sin) a.det_sin[base + i] = aoa_sin(ph, a.kinv);
  }
  if (!a.tgt_any) return;                                    // uniform: no per-target output was asked for
  __syncthreads();

  // 2. the targets: every place 1..M is written, a target without a valid member gets zeros
  const int lane = tid & 63;
  const size_t obase = (size_t)f * M;
  for (int t = tid >> 6; t < M; t += nt >> 6) {
    float zr = 0.f, zi = 0.f, e0 = 0.f, e1 = 0.f;
    int cells = 0;
    for (int b = 0; b < n; b += 64) {
      const int j = b + lane;
      unsigned long long mask = __ballot(j < n && s_lab[j] == t + 1);
      cells += __popcll(mask);
      while (mask) {                                         // the members, in ascending position
        const int src = b + __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const float4 v = s_z[src];
        zr += v.x;
        zi += v.y;
        e0 += v.z;
        e1 += v.w;
      }
    }
    if (lane == 0) {
      const float ph = aoa_phase(zr, zi);
      float coh = 0.f;
      if (e0 != 0.f && e1 != 0.f) coh = fminf(1.f, sqrtf(zr * zr + zi * zi) / (sqrtf(e0) * sqrtf(e1)));
      if (a.tgt_zre) a.tgt_zre[obase + t] = zr * a.scale2;
      if (a.tgt_zim) a.tgt_zim[obase + t] = zi * a.scale2;
      if (a.tgt_e0) a.tgt_e0[obase + t] = e0 * a.scale2;
      if (a.tgt_e1) a.tgt_e1[obase + t] = e1 * a.scale2;
      if (a.tgt_phase) a.tgt_phase[obase + t] = ph;
      if (a.tgt_sin) a.tgt_sin[obase + t] = aoa_sin(ph, a.kinv);
      if (a.tgt_coh) a.tgt_coh[obase + t] = coh;
      if (a.tgt_cells) a.tgt_cells[obase + t] = cells;
    }
  }
}

}  // namespace

hipError_t launch_aoa(const AoaArgs& a, hipStream_t s) {
  if (a.F <= 0) return hipSuccess;
  if (a.K < 1 || a.K > kAoaMaxDet || a.M < 0 || a.M > kAoaMaxTgt || a.A < 2 || a.A > kAoaChan || a.F > 0x7fffffffLL ||
      a.NR < 1 || a.ND < 1 || (a.tgt_any && (a.M < 1 || !a.det_label)))
    return hipErrorInvalidValue;
  const int threads = a.K <= 64 ? 64 : 256;
  const size_t shmem = (size_t)a.K * (sizeof(float4) + sizeof(int));   // 20 KiB at max_det 1024
  hipLaunchKernelGGL(k_aoa, dim3((unsigned)a.F), dim3(threads), shmem, s, a);
  return hipGetLastError();
}

}  // namespace fmcw
