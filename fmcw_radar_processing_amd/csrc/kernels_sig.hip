// kernels_sig.hip -- micro-Doppler (Doppler-time) and range-time signatures of the RD map, for gfx950.
//
// Definition (include/fmcw.h, fmcw_sig_params): with P = |D|^2 and the rows of frame f (the gate, or
// the window centre - h .. centre + h clipped to the gate),
//   doppler_time[f][d] = sum of P[r][d] over the frame's rows,
//   range_time[f][r]   = sum of P[r][d] over the Doppler bins not left out (|d - nd/2| <= dc_half are),
//                        0 for every row that is not one of the frame's.
// Both are sums of non-negative terms by additions only, in an order that depends on
// (nr, nd, dtype, gate, track_half) alone, so the results are bit-identical from call to call and
// do not depend on F.
//
// k_sig   One workgroup of 256 threads owns a slab of consecutive rows of one frame (kSigPasses
//         passes of 4 KiB, 128 KiB of complex64 at most) and reads every row once, 16 bytes per lane
//         (2 complex64 or 4 fp16-storage cells), several passes in flight.  A thread keeps the same
//         cells (columns) in every pass:
//           LPR = lanes per row = nd / cells per lane, TPR = min(LPR, 256) threads per row,
//           RPP = 256 / TPR rows per pass; a thread's cells are those of chunk tid % TPR (and
//           chunk + 256 when LPR = 512), its row in the pass is tid / TPR.
//         Column sums stay in registers over the passes.  At the end the lanes of a wave that hold
//         the same columns (TPR < 64: a wave-load spans 64 / TPR rows) are combined by a butterfly,
//         then the waves (or the RPP row groups) in ascending order through LDS.
//         Row sums: the kept cells of the lane, then a butterfly over the min(TPR, 64) lanes of
//         the row (DPP inside 16 lanes, two shuffles above).  A row shorter than a wave is stored by
//         its first lane at once; a row of one or more waves is parked in lane `pass` of each wave
//         and the waves of a row are combined in ascending order after the loop.  Nothing goes
//         through LDS inside the row loop.
//         One slab per frame: the workgroup writes doppler_time itself.  Several: it writes its
//         column sums to scratch [F][slabs][nd] and
// k_sig_gather  (one workgroup per frame) adds the slabs in ascending order.
// Both raise the maxima by one integer atomic max per workgroup (non-negative floats order as
// their bits), skipped when the value read first is already as large.
// k_sig_db  out = max(10 log10(map / max), floor_db), floor_db where map or max is 0.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#include <hip/hip_fp16.h>

namespace fmcw {

namespace {

constexpr int kSigPasses = 32;       // passes of a slab at most: a row sum per pass fits the lanes of a wave
constexpr int kSigMaxSlabs = 256;

template <int CTRL>
__device__ inline float sig_dpp(float x) {
  const int v = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false));
}

// Sum over the aligned group of W lanes (a power of two, wave-uniform) that holds this lane; every
// lane of the group gets the same bits (a + b == b + a).  After the steps below W = 4 all lanes of
// a quad are equal, so the mirrored lane of the other quad (half row) carries that quad's sum.
__device__ inline float sig_group_sum(float s, int W) {
  if (W > 1) s += sig_dpp<0xB1>(s);      // quad_perm [1,0,3,2]
  if (W > 2) s += sig_dpp<0x4E>(s);      // quad_perm [2,3,0,1]
  if (W > 4) s += sig_dpp<0x141>(s);     // row_half_mirror
  if (W > 8) s += sig_dpp<0x140>(s);     // row_mirror
  if (W > 16) s += __shfl_xor(s, 16);
  if (W > 32) s += __shfl_xor(s, 32);
  return s;
}

__device__ inline float sig_wave_max(float m) {
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
  return m;
}

// max over the workgroup's threads (256), raised into *dst by thread 0
__device__ inline void sig_raise(float m, float* dst, float* wm) {
  m = sig_wave_max(m);
  __syncthreads();                                  // wm may still be read from a previous call
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    int* const p = reinterpret_cast<int*>(dst);
    if (__float_as_int(m) > __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMax(p, __float_as_int(m));
  }
}

// rows [ra, rb) of frame f, 0-based; ra == rb: none
__device__ inline void sig_rows(const SigArgs& a, int64_t f, int& ra, int& rb) {
  ra = a.g0;
  rb = a.g1 + 1;
  if (a.center) {
    const int c = a.center[f * a.cstride];
    if (c < 1 || c > a.NR) {
      ra = rb = 0;
      return;
    }
    ra = max(c - 1 - a.th, a.g0);
    rb = min(c - 1 + a.th, a.g1) + 1;
    if (ra >= rb) ra = rb = 0;
  }
}

template <bool H>
__device__ inline void sig_powers(const uint4& raw, float* pw) {
  if (H) {
    const __half2* hp = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float2 v = __half22float2(hp[i]);
      pw[i] = v.x * v.x + v.y * v.y;
    }
  } else {
    const float4 v = __builtin_bit_cast(float4, raw);
    pw[0] = v.x * v.x + v.y * v.y;
    pw[1] = v.z * v.z + v.w * v.w;
  }
}

}  // namespace

// H: fp16 storage.  NC: 16-byte chunks of a row per thread (2 only for complex64 at nd = 1024).
// FULL: a row fills one wave-load or more (TPR >= 64), so the row sums' butterfly has no branches.
template <bool H, int NC, bool FULL>
__global__ __launch_bounds__(256) void k_sig(SigArgs a) {
  constexpr int CPL = H ? 4 : 2;                   // cells per 16-byte load
  constexpr int NV = NC * CPL;                     // cells of a thread per pass
  constexpr int U = 8 / NC;                        // passes in flight
  __shared__ float colpart[1024];                  // [J][ND] column sums to combine, J * ND <= 1024
  __shared__ float rowpart[kSigPasses * 4];        // [pass][wave] row sums of whole waves
  __shared__ float wm[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int NR = a.NR, ND = a.ND;
  const int TPR = min(ND / CPL, 256);              // threads per row (NC * TPR chunks cover a row)
  const int RPP = 256 / TPR;                       // rows per pass
  const int W = FULL ? 64 : TPR;                   // lanes of a wave on one row
  const int chunk = tid & (TPR - 1), rip = tid / TPR;
  const int64_t f = blockIdx.x / a.slabs;
  const int slab = (int)(blockIdx.x - f * a.slabs);
  int ra, rb;
  sig_rows(a, f, ra, rb);
  const int s0 = ra + slab * a.SR, s1 = min(s0 + a.SR, rb);   // this slab's rows [s0, s1)
  const int npass = s1 > s0 ? (s1 - s0 + RPP - 1) / RPP : 0;
  const bool want_rt = a.rt != nullptr, want_dt = a.dt != nullptr;
  const float sc = a.scale2;
  float* const rt = want_rt ? a.rt + f * NR : nullptr;

  // range-time rows that are not the frame's are zero: the first slab writes them
  if (want_rt && slab == 0)
    for (int i = tid; i < NR; i += 256)
      if (i < ra || i >= rb) rt[i] = 0.f;

  // the Doppler bins of this thread's cells that the row sums keep
  bool keep[NV];
#pragma unroll
  for (int k = 0; k < NC; ++k)
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int d = (chunk + k * 256) * CPL + i, dist = abs(d - ND / 2);
      keep[k * CPL + i] = min(dist, ND - dist) > a.dc;
    }

  const size_t es = H ? 4 : 8;
  const char* const base = static_cast<const char*>(a.rd) + (size_t)f * NR * ND * es + (size_t)chunk * 16;
  float acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.f;
  float rs = 0.f, mrt = 0.f;

  for (int p0 = 0; p0 < npass; p0 += U) {
    uint4 v[U][NC];
    // rows past the slab's end re-read its last row (never a row outside the frame's) and count as zero
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = min(s0 + (p0 + u) * RPP + rip, s1 - 1);
#pragma unroll
      for (int k = 0; k < NC; ++k)
        v[u][k] = *reinterpret_cast<const uint4*>(base + (size_t)row * ND * es + (size_t)k * 4096);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = s0 + (p0 + u) * RPP + rip;
      const bool ok = row < s1;
      float pw[NV];
#pragma unroll
      for (int k = 0; k < NC; ++k) sig_powers<H>(v[u][k], pw + k * CPL);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        pw[i] = ok ? pw[i] : 0.f;
        acc[i] += pw[i];
        s += keep[i] ? pw[i] : 0.f;
      }
      if (want_rt) {
        s = sig_group_sum(s, W);
        if (!FULL) {
          if ((lane & (W - 1)) == 0 && ok) {
            s *= sc;
            rt[row] = s;
            mrt = fmaxf(mrt, s);
          }
        } else {
          rs = lane == p0 + u ? s : rs;
        }
      }
    }
  }

  if (FULL && want_rt) {
    // whole-wave rows: lane p of wave w holds the wave's sum of pass p; the waves of a row in ascending order
    if (lane < npass) rowpart[lane * 4 + w] = rs;
    __syncthreads();
    const int WPR = TPR / 64;                      // waves per row
    if (tid < npass * RPP) {
      const int p = tid / RPP, first = (tid - p * RPP) * WPR, row = s0 + tid;
      float s = rowpart[p * 4 + first];
      for (int i = 1; i < WPR; ++i) s += rowpart[p * 4 + first + i];
      if (row < s1) {
        s *= sc;
        rt[row] = s;
        mrt = fmaxf(mrt, s);
      }
    }
  }
  if (want_rt && a.rt_max) sig_raise(mrt, a.rt_max, wm);

  if (!want_dt) return;
  // column sums: first the lanes of the wave that hold the same chunk (rows rip, rip + 1, ... of a pass)
  if (!FULL)
    for (int o = TPR; o < 64; o <<= 1)
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[i] += __shfl_xor(acc[i], o);
  const int J = FULL ? RPP : 4;                    // partial sums per column: the row groups, or the waves
  const int j = FULL ? rip : w;
  if (FULL || lane < TPR) {
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
      for (int i = 0; i < CPL; ++i) colpart[j * ND + (chunk + k * 256) * CPL + i] = acc[k * CPL + i];
  }
  __syncthreads();
  float mdt = 0.f;
  for (int c = tid; c < ND; c += 256) {
    float s = colpart[c];
    for (int jj = 1; jj < J; ++jj) s += colpart[jj * ND + c];
    s *= sc;
    if (a.slabs == 1) {
      a.dt[f * ND + c] = s;
      mdt = fmaxf(mdt, s);
    } else {
      a.part[((size_t)f * a.slabs + slab) * ND + c] = s;
    }
  }
  if (a.slabs == 1 && a.dt_max) sig_raise(mdt, a.dt_max, wm);
}

__global__ __launch_bounds__(256) void k_sig_gather(SigArgs a) {
  __shared__ float wm[4];
  const int tid = threadIdx.x, ND = a.ND;
  const int64_t f = blockIdx.x;
  const float* const part = a.part + (size_t)f * a.slabs * ND;
  float mdt = 0.f;
  for (int c = tid; c < ND; c += 256) {
    float s = part[c];
    for (int k = 1; k < a.slabs; ++k) s += part[(size_t)k * ND + c];
    a.dt[f * ND + c] = s;
    mdt = fmaxf(mdt, s);
  }
  if (a.dt_max) sig_raise(mdt, a.dt_max, wm);
}

__global__ __launch_bounds__(256) void k_sig_db(const float* __restrict__ map, int64_t n, const float* __restrict__ mx,
                                                float floor_db, float* out) {
  const float m = *mx;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = map[i];
    out[i] = (v == 0.f || m == 0.f) ? floor_db : fmaxf(10.f * log10f(v / m), floor_db);
  }
}

// Slab height and count: functions of (nr, nd, dtype, gate, track_half) only, never of F.
void sig_plan(SigArgs& a) {
  const int cpl = a.h ? 4 : 2, lpr = a.ND / cpl;
  const int tpr = lpr < 256 ? lpr : 256, nc = lpr / tpr, rpp = 256 / tpr;
  a.SR = rpp * (kSigPasses / nc);
  const int gate = a.g1 - a.g0 + 1;
  const int rows = a.center ? (2 * a.th + 1 < gate ? 2 * a.th + 1 : gate) : gate;
  a.slabs = (rows + a.SR - 1) / a.SR;
}

size_t sig_scratch_per_frame(const SigArgs& a) {
  return a.slabs > 1 && a.dt ? (size_t)a.slabs * a.ND * sizeof(float) : 0;
}

hipError_t launch_sig(const SigArgs& a, hipStream_t s) {
  if (a.F <= 0) return hipSuccess;
  const int cpl = a.h ? 4 : 2, lpr = a.ND / cpl, nc = lpr > 256 ? lpr / 256 : 1;
  const int64_t wgs = a.F * a.slabs;
  if (a.ND < 4 || a.ND > 1024 || (a.ND & (a.ND - 1)) || a.NR < 1 || lpr < 1 || nc > 2 || (nc == 2 && a.h) ||
      a.g0 < 0 || a.g1 >= a.NR || a.g0 > a.g1 || a.th < 0 || a.slabs < 1 || a.slabs > kSigMaxSlabs || a.SR < 1 ||
      (size_t)a.slabs * a.SR < (size_t)(a.center ? std::min(2 * a.th + 1, a.g1 - a.g0 + 1) : a.g1 - a.g0 + 1) ||
      a.SR > (256 / (lpr < 256 ? lpr : 256)) * (kSigPasses / nc) || wgs > 0x7fffffffLL || (!a.dt && !a.rt) ||
      (a.center && a.cstride < 1) || (a.slabs > 1 && a.dt && !a.part))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)wgs), block(256);
  const bool full = lpr >= 64;
  if (a.h && full) hipLaunchKernelGGL((k_sig<true, 1, true>), grid, block, 0, s, a);
  else if (a.h) hipLaunchKernelGGL((k_sig<true, 1, false>), grid, block, 0, s, a);
  else if (nc == 2) hipLaunchKernelGGL((k_sig<false, 2, true>), grid, block, 0, s, a);
  else if (full) hipLaunchKernelGGL((k_sig<false, 1, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_sig<false, 1, false>), grid, block, 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.slabs == 1 || !a.dt) return e;
  hipLaunchKernelGGL(k_sig_gather, dim3((unsigned)a.F), block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sig_db(const float* map, int64_t n, const float* mx, float floor_db, float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t wgs = std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_sig_db, dim3((unsigned)wgs), dim3(256), 0, s, map, n, mx, floor_db, out);
  return hipGetLastError();
}

}  // namespace fmcw
