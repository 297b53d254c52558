// kernels_oscfar.hip -- 2-D ordered-statistic CFAR over the range-Doppler map, for gfx950.
//
// Definition (include/fmcw.h, fmcw_oscfar_params): the training set of cell (r, d) is CA-CFAR's;
// with k(r) the rank scaled to the clipped window, the cell is a detection iff at least k(r)
// training powers x have fl(alpha x) < P, which is P > fl(alpha X_(k)).  Every float operation is
// rounded on its own (no contraction), so the outputs equal a float32 reference byte for byte.
//
// k_oscfar  k_cfar's decomposition: one workgroup owns a strip of range rows x a tile of up to 256
//         Doppler columns of one frame and walks the strip row by row.  Every RD row is loaded once
//         (16 bytes per lane, one row ahead) and goes into two LDS rings with a circular halo of Wd
//         columns: P = |D|^2 (the centre cell and the LOCAL_MAX neighbours) and Q = fl(alpha P) (the
//         training cells).  Thread t owns column t: the decision of the centre row (max(Wr, 1) rows
//         behind the newest) is N compares Q < P whose results are counted, an exact integer
//         whatever the order; the LDS reads are independent of each other and issued in batches.
//         Detections go to the per-wave raster-ordered lists of k_cfar, with an empty noise slot,
//         and k_cfar_gather merges them as it does for CA.
// k_oscfar_select  One wave per listed detection (at most max_det per frame): its lanes recompute
//         the window's training powers from the map with the same float operations, at most 18 per
//         lane (the kernel is instantiated for 3, 6, 12 and 18, picked by the window's size), and a
//         31-step radix select over the float bit patterns (non-negative floats order as their
//         integer bits) with wave-wide counts per bit finds X_(k), which lane 0 stores.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#include <hip/hip_fp16.h>

#pragma clang fp contract(off)

namespace fmcw {

namespace {

constexpr int kOsMaxSub = 2048;      // k_cfar_gather's limits
constexpr int kOsMaxStrips = 128;
constexpr int kOsSelPerLane = 18;    // ceil(33 * 33 / 64) window positions per lane at the largest window

struct OsGeom {
  int Wr, Wd, L, PD, HB, PW;
};
__host__ __device__ inline OsGeom os_geom(const CfarArgs& a) {
  OsGeom g;
  g.Wr = a.gr + a.tr;
  g.Wd = a.gd + a.td;
  g.L = g.Wr > 1 ? g.Wr : 1;                   // the centre row lags the newest row by L (row r + 1 is there for LOCAL_MAX)
  g.PD = 2 * g.L + 2;                          // rows r - L .. r + L, and one being written
  g.HB = ((g.Wd > 1 ? g.Wd : 1) + 3) & ~3;     // halo columns on each side, whole 16-byte loads
  g.PW = a.TC + 2 * g.HB;
  return g;
}

// P of one stored cell: fp16 storage is widened exactly and scaled by nr * nd (exact) first
__device__ __forceinline__ float os_power(float re, float im) {
  const float a = re * re, b = im * im;
  return a + b;
}

// training cells N(r) of centre row r and its rank k(r)
__device__ __forceinline__ int os_rank(const OsCfarArgs& o, int Wr, int Wd, int r, int& lo, int& hi, int& glo, int& ghi) {
  const CfarArgs& a = o.c;
  lo = max(-Wr, -r);
  hi = min(Wr, a.NR - 1 - r);
  glo = max(lo, -a.gr);
  ghi = min(hi, a.gr);
  const int nside = ghi - glo + 1, nfull = hi - lo + 1 - nside;
  const int N = nside * 2 * a.td + nfull * (2 * Wd + 1);
  return o.nfull > 1 ? 1 + ((o.rank - 1) * (N - 1)) / (o.nfull - 1) : 1;
}

// cnt + #{dd in [lo, hi] : q[dd] < P}, the reads four at a time (eight at a time measured slower)
__device__ __forceinline__ int os_count(const float* q, int lo, int hi, float P, int cnt) {
  int dd = lo;
  for (; dd + 3 <= hi; dd += 4) {
    const float x0 = q[dd], x1 = q[dd + 1], x2 = q[dd + 2], x3 = q[dd + 3];
    cnt += (x0 < P) + (x1 < P) + (x2 < P) + (x3 < P);
  }
  for (; dd <= hi; ++dd) cnt += q[dd] < P;
  return cnt;
}

}  // namespace

__global__ __launch_bounds__(256) void k_oscfar(OsCfarArgs o) {
  extern __shared__ float lds[];
  const CfarArgs& a = o.c;
  const OsGeom g = os_geom(a);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int NR = a.NR, ND = a.ND, TC = a.TC, PW = g.PW, HB = g.HB, L = g.L;
  const int WPF = a.strips * a.tiles;
  const int64_t f = blockIdx.x / WPF;
  const int wi = (int)(blockIdx.x - f * WPF);
  const int strip = wi / a.tiles, tile = wi - strip * a.tiles;
  float* const Pr = lds;                       // [PD][PW]  |D|^2, entry i = column (c0 - HB + i) mod ND
  float* const Qr = Pr + g.PD * PW;            // [PD][PW]  fl(alpha |D|^2)
  const int s0 = a.g0 + strip * a.RS;
  const int s1 = min(s0 + a.RS, a.g1 + 1);     // centre rows [s0, s1)
  const int c0 = tile * TC, c = tid;
  const bool colv = c < TC;
  // one 16-byte load per lane and row: 2 complex64 or 4 fp16-storage cells
  const int cpl = a.h ? 4 : 2;
  const bool ldv = tid < PW / cpl;
  const int gcol = (c0 - HB + tid * cpl) & (ND - 1);
  const size_t es = a.h ? 4 : 8;
  const char* const fbase = static_cast<const char*>(a.rd) + (size_t)f * NR * ND * es + (size_t)gcol * es;
  auto load = [&](int row) { return *reinterpret_cast<const uint4*>(fbase + (size_t)row * ND * es); };
  const float sc = a.scale, alpha = a.alpha;
  auto put = [&](const uint4& raw, int slot) {
    float* const dp = Pr + slot * PW + tid * cpl;
    float* const dq = Qr + slot * PW + tid * cpl;
    if (a.h) {
      const __half2* hp = reinterpret_cast<const __half2*>(&raw);
      float4 p;
      float2 v = __half22float2(hp[0]); p.x = os_power(v.x * sc, v.y * sc);
      v = __half22float2(hp[1]); p.y = os_power(v.x * sc, v.y * sc);
      v = __half22float2(hp[2]); p.z = os_power(v.x * sc, v.y * sc);
      v = __half22float2(hp[3]); p.w = os_power(v.x * sc, v.y * sc);
      *reinterpret_cast<float4*>(dp) = p;
      *reinterpret_cast<float4*>(dq) = make_float4(alpha * p.x, alpha * p.y, alpha * p.z, alpha * p.w);
    } else {
      const float4 v = __builtin_bit_cast(float4, raw);
      const float p0 = os_power(v.x, v.y), p1 = os_power(v.z, v.w);
      *reinterpret_cast<float2*>(dp) = make_float2(p0, p1);
      *reinterpret_cast<float2*>(dq) = make_float2(alpha * p0, alpha * p1);
    }
  };

  // mask rows outside the gate are zero: the first strip clears the rows before it, the last the rows after
  if (a.mask) {
    uint8_t* const m = a.mask + (size_t)f * NR * ND + c0;
    if (strip == 0)
      for (int i = tid; i < a.g0 * TC; i += blockDim.x) m[(size_t)(i / TC) * ND + (i % TC)] = 0;
    if (strip == a.strips - 1)
      for (int i = tid; i < (NR - 1 - a.g1) * TC; i += blockDim.x) m[(size_t)(a.g1 + 1 + i / TC) * ND + (i % TC)] = 0;
  }

  const int j0 = max(0, s0 - L), j1 = s1 - 1 + L;
  int jp = j0 % g.PD;                          // ring slot of row j
  if (ldv) put(load(j0), jp);
  int wcount = 0;                              // detections of this wave so far (wave-uniform)
  const int sub = wi * a.waves + w;
  float4* const list = a.sub_list + ((size_t)f * WPF * a.waves + sub) * a.K;

  for (int j = j0; j <= j1; ++j) {
    const bool more = j + 1 <= j1 && j + 1 < NR;
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (more && ldv) nxt = load(j + 1);        // in flight under this row's compares
    __syncthreads();                           // row j's powers are in LDS
    const int r = j - L;
    if (r >= s0 && r < s1) {
      int lo, hi, glo, ghi;
      const int k = os_rank(o, g.Wr, g.Wd, r, lo, hi, glo, ghi);
      bool det = false;
      float P = 0.f;
      int rp = jp - L;                         // ring slot of row r
      if (rp < 0) rp += g.PD;
      if (colv) {
        const float* p = Pr + rp * PW + HB + c;
        P = p[0];
        int q = rp + lo;                       // ring slot of row r + lo
        if (q < 0) q += g.PD;
        int cnt = 0;
        for (int dr = lo; dr <= hi; ++dr) {
          const float* x = Qr + q * PW + HB + c;
          if (dr >= glo && dr <= ghi) {
            cnt = os_count(x, -g.Wd, -a.gd - 1, P, cnt);
            cnt = os_count(x, a.gd + 1, g.Wd, P, cnt);
          } else {
            cnt = os_count(x, -g.Wd, g.Wd, P, cnt);
          }
          if (++q == g.PD) q = 0;
        }
        det = cnt >= k;
        if (det && a.local_max) {
          bool top = P > p[-1] && P >= p[1];
          if (r > 0) {
            const float* u = Pr + (rp == 0 ? g.PD - 1 : rp - 1) * PW + HB + c;
            top = top && P > u[-1] && P > u[0] && P > u[1];
          }
          if (r + 1 < NR) {
            const float* d = Pr + (rp + 1 == g.PD ? 0 : rp + 1) * PW + HB + c;
            top = top && P >= d[-1] && P >= d[0] && P >= d[1];
          }
          det = top;
        }
        if (a.mask) a.mask[((size_t)f * NR + r) * ND + c0 + c] = det ? 1 : 0;
      }
      const unsigned long long bal = __ballot(det);
      if (bal) {
        const int pos = wcount + __popcll(bal & ((1ull << lane) - 1ull));
        if (det && pos < a.K) list[pos] = make_float4(__int_as_float(r * ND + c0 + c), P, 0.f, 0.f);
        wcount += __popcll(bal);
      }
    }
    if (more && ldv) put(nxt, jp + 1 == g.PD ? 0 : jp + 1);   // that slot's row (j + 1 - PD) is below every row read above
    if (++jp == g.PD) jp = 0;
  }
  if (lane == 0) a.sub_count[(size_t)f * WPF * a.waves + sub] = wcount;
}

// MP: window positions per lane, (2 Wr + 1)(2 Wd + 1) <= 64 MP
template <int MP>
__global__ __launch_bounds__(256) void k_oscfar_select(OsCfarArgs o) {
  const CfarArgs& a = o.c;
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int K = a.K;
  const int64_t f = wid / K;
  const int i = (int)(wid - f * K);
  if (f >= a.F || i >= min(a.det_count[f], K)) return;       // wave-uniform
  const int NR = a.NR, ND = a.ND, Wr = a.gr + a.tr, Wd = a.gd + a.td;
  const int r = a.det_ridx[f * K + i] - 1, d = a.det_didx[f * K + i] - 1;
  int lo, hi, glo, ghi;
  int k = os_rank(o, Wr, Wd, r, lo, hi, glo, ghi);
  const int cols = 2 * Wd + 1, cells = (2 * Wr + 1) * cols;
  const size_t es = a.h ? 4 : 8;
  const char* const fbase = static_cast<const char*>(a.rd) + (size_t)f * NR * ND * es;
  const float sc = a.scale;
  uint32_t v[MP];                              // bit patterns of this lane's training powers; all ones: no cell
#pragma unroll
  for (int m = 0; m < MP; ++m) {
    const int t = lane + 64 * m;
    const int dr = t / cols - Wr, dd = t - (t / cols) * cols - Wd;
    uint32_t bits = 0xffffffffu;
    if (t < cells && dr >= lo && dr <= hi && !(dr >= -a.gr && dr <= a.gr && dd >= -a.gd && dd <= a.gd)) {
      const char* const cell = fbase + ((size_t)(r + dr) * ND + ((d + dd) & (ND - 1))) * es;
      float P;
      if (a.h) {
        const float2 z = __half22float2(*reinterpret_cast<const __half2*>(cell));
        P = os_power(z.x * sc, z.y * sc);
      } else {
        const float2 z = *reinterpret_cast<const float2*>(cell);
        P = os_power(z.x, z.y);
      }
      bits = __float_as_uint(P);
    }
    v[m] = bits;
  }
  // the k-th smallest pattern, bit by bit from the top: the k valid cells sought all have bit 31 clear
  uint32_t prefix = 0;
  for (int b = 30; b >= 0; --b) {
    const uint32_t above = ~((2u << b) - 1u);
    int zeros = 0;                             // candidates (equal to prefix above bit b) whose bit b is clear
#pragma unroll
    for (int m = 0; m < MP; ++m)
      zeros += __popcll(__ballot((v[m] & above) == prefix && !((v[m] >> b) & 1u)));
    if (k > zeros) {
      k -= zeros;
      prefix |= 1u << b;
    }
  }
  if (lane == 0) a.det_noise[f * K + i] = __uint_as_float(prefix);
}

hipError_t launch_oscfar(const OsCfarArgs& o, hipStream_t s) {
  const CfarArgs& a = o.c;
  if (a.F <= 0) return hipSuccess;
  const OsGeom g = os_geom(a);
  const int64_t wgs = a.F * a.strips * a.tiles;
  const int64_t sel = (a.F * a.K + 3) / 4;
  const int nfull = (2 * g.Wr + 1) * (2 * g.Wd + 1) - (2 * a.gr + 1) * (2 * a.gd + 1);
  if (a.strips < 1 || a.strips > kOsMaxStrips || a.strips * a.tiles * a.waves > kOsMaxSub || wgs > 0x7fffffffLL ||
      sel > 0x7fffffffLL || a.TC * a.tiles != a.ND || a.waves * 64 < a.TC || a.waves > 4 ||
      g.PW / (a.h ? 4 : 2) > a.waves * 64 || g.Wd > g.HB || g.Wr > 16 || g.Wd > 16 || 2 * g.Wd + 1 > a.ND ||
      2 * g.Wr + 1 > a.NR || a.g0 < 0 || a.g1 >= a.NR || a.g0 > a.g1 ||
      (a.g1 - a.g0 + 1 + a.RS - 1) / a.RS != a.strips || a.K < 1 || o.nfull != nfull || o.rank < 1 || o.rank > nfull ||
      (2 * g.Wr + 1) * (2 * g.Wd + 1) > 64 * kOsSelPerLane)
    return hipErrorInvalidValue;
  const size_t shmem = 2 * (size_t)g.PD * g.PW * sizeof(float);
  if (shmem > 160 * 1024) return hipErrorInvalidValue;
  if (shmem > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_oscfar),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_oscfar, dim3((unsigned)wgs), dim3(a.waves * 64), shmem, s, o);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_cfar_gather(a, s);
  if (e != hipSuccess) return e;
  const int cells = (2 * g.Wr + 1) * (2 * g.Wd + 1);
  if (cells <= 64 * 3) hipLaunchKernelGGL(k_oscfar_select<3>, dim3((unsigned)sel), dim3(256), 0, s, o);
  else if (cells <= 64 * 6) hipLaunchKernelGGL(k_oscfar_select<6>, dim3((unsigned)sel), dim3(256), 0, s, o);
  else if (cells <= 64 * 12) hipLaunchKernelGGL(k_oscfar_select<12>, dim3((unsigned)sel), dim3(256), 0, s, o);
  else hipLaunchKernelGGL(k_oscfar_select<kOsSelPerLane>, dim3((unsigned)sel), dim3(256), 0, s, o);
  return hipGetLastError();
}

}  // namespace fmcw
