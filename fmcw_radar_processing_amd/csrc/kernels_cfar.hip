// kernels_cfar.hip -- 2-D cell-averaging CFAR over the range-Doppler map, for gfx950.
//
// Definition (include/fmcw.h, fmcw_cfar_params): the training set of cell (r, d) is the window
// |dr| <= Wr, |dd| <= Wd without the guard box |dr| <= guard_r, |dd| <= guard_d, circular in
// Doppler and clipped in range; the cell is a detection iff P > alpha * S / N.
//
// k_cfar  One workgroup owns a strip of range rows x a tile of up to 256 Doppler columns of one
//         frame and walks the strip row by row.  Every RD row is loaded once (16 bytes per lane)
//         and turned into |D|^2, which goes into a small ring of power rows in LDS (with a
//         circular halo of Wd columns on each side).  Thread t owns column t of the tile: from the
//         newest power row it forms the two horizontal sums of the separable form,
//           H_full over the 2 Wd + 1 columns, H_side over the 2 train_d columns outside the guard,
//         and keeps them in two LDS rings of its own (Wr + max(Wr, 1) + 1 rows deep).  The sum of
//         the training cells of the centre row (max(Wr, 1) rows behind the newest) is then the
//         vertical sum of H_full over the rows outside the guard rows and of H_side over the guard
//         rows: additions of non-negative terms only, in one fixed order (no box differences and no
//         running sum, whose subtractions would leave u * P_target behind next to a strong target),
//         so a cell's result does not depend on the strip it fell into.
//         Detections are appended in raster order per wave (a wave owns 64 columns; a ballot gives
//         the positions), each wave to its own list of at most max_det entries, and counted in full.
// k_cfar_gather  One workgroup per frame merges the frame's lists into the raster-ordered output:
//         the position of an entry is the number of detections in the strips before its own, plus its
//         rank among its strip's lists (binary searches on the cell index).  A list that was cut at
//         max_det entries only lacks entries whose rank is >= max_det anyway.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#include <hip/hip_fp16.h>

namespace fmcw {

namespace {

constexpr int kCfarTile = 256;       // Doppler columns per workgroup (one thread per column)
constexpr int kCfarMaxSub = 2048;    // lists per frame: 128 strips x 4 tiles x 4 waves at most
constexpr int kCfarMaxStrips = 128;

struct CfarGeom {
  int Wr, Wd, L, HD, PD, HB, PW;
};
__host__ __device__ inline CfarGeom cfar_geom(const CfarArgs& a) {
  CfarGeom g;
  g.Wr = a.gr + a.tr;
  g.Wd = a.gd + a.td;
  g.L = g.Wr > 1 ? g.Wr : 1;                   // the centre row lags the newest row by L (row r + 1 is there for LOCAL_MAX)
  g.HD = g.Wr + g.L + 1;                       // rows of the H rings
  g.PD = g.L + 3;                              // rows of the power ring: r - 1 .. r + L, and one being written
  g.HB = ((g.Wd > 1 ? g.Wd : 1) + 3) & ~3;     // halo columns on each side, whole 16-byte loads
  g.PW = a.TC + 2 * g.HB;
  return g;
}

}  // namespace

__global__ __launch_bounds__(256) void k_cfar(CfarArgs a) {
  extern __shared__ float lds[];
  const CfarGeom g = cfar_geom(a);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int NR = a.NR, ND = a.ND, TC = a.TC, PW = g.PW, HB = g.HB, L = g.L;
  const int WPF = a.strips * a.tiles;
  const int64_t f = blockIdx.x / WPF;
  const int wi = (int)(blockIdx.x - f * WPF);
  const int strip = wi / a.tiles, tile = wi - strip * a.tiles;
  float* const Pr = lds;                       // [PD][PW]  |D|^2, entry i = column (c0 - HB + i) mod ND
  float* const Hf = Pr + g.PD * PW;            // [HD][TC]  H_full
  float* const Hs = Hf + g.HD * TC;            // [HD][TC]  H_side
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
  const float sc = a.scale;
  auto put = [&](const uint4& raw, int slot) {
    float* dst = Pr + slot * PW + tid * cpl;
    if (a.h) {
      const __half2* hp = reinterpret_cast<const __half2*>(&raw);
      float4 p;
      float2 v = __half22float2(hp[0]); v.x *= sc; v.y *= sc; p.x = v.x * v.x + v.y * v.y;
      v = __half22float2(hp[1]); v.x *= sc; v.y *= sc; p.y = v.x * v.x + v.y * v.y;
      v = __half22float2(hp[2]); v.x *= sc; v.y *= sc; p.z = v.x * v.x + v.y * v.y;
      v = __half22float2(hp[3]); v.x *= sc; v.y *= sc; p.w = v.x * v.x + v.y * v.y;
      *reinterpret_cast<float4*>(dst) = p;
    } else {
      const float4 v = __builtin_bit_cast(float4, raw);
      *reinterpret_cast<float2*>(dst) = make_float2(v.x * v.x + v.y * v.y, v.z * v.z + v.w * v.w);
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
  int jp = j0 % g.PD, jh = j0 % g.HD;          // ring slots of row j
  if (ldv) put(load(j0), jp);
  int wcount = 0;                              // detections of this wave so far (wave-uniform)
  const int sub = (int)(blockIdx.x % WPF) * a.waves + w;
  float4* const list = a.sub_list + ((size_t)f * WPF * a.waves + sub) * a.K;
  const int side_rows = a.td > 0 ? 1 : 0;

  for (int j = j0; j <= j1; ++j) {
    const bool more = j + 1 <= j1 && j + 1 < NR;
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (more && ldv) nxt = load(j + 1);        // in flight under this row's sums
    __syncthreads();                           // row j's powers are in LDS
    if (j < NR && colv) {
      const float* p = Pr + jp * PW + HB + c;
      float side = 0.f, mid = 0.f;
      for (int dd = -g.Wd; dd < -a.gd; ++dd) side += p[dd];
      for (int dd = a.gd + 1; dd <= g.Wd; ++dd) side += p[dd];
      for (int dd = -a.gd; dd <= a.gd; ++dd) mid += p[dd];
      Hs[jh * TC + c] = side;
      Hf[jh * TC + c] = side + mid;
    }
    const int r = j - L;
    if (r >= s0 && r < s1) {
      const int lo = max(-g.Wr, -r), hi = min(g.Wr, NR - 1 - r);
      const int glo = max(lo, -a.gr), ghi = min(hi, a.gr);
      const int nside = ghi - glo + 1, nfull = hi - lo + 1 - nside;
      const int N = nside * 2 * a.td + nfull * (2 * g.Wd + 1);
      bool det = false;
      float P = 0.f, S = 0.f;
      int rp = jp - L;                         // power-ring slot of row r
      if (rp < 0) rp += g.PD;
      if (colv) {
        int q = jh - L + lo;                   // H-ring slot of row r + lo
        if (q < 0) q += g.HD;
        for (int dr = lo; dr < glo; ++dr) {
          S += Hf[q * TC + c];
          if (++q == g.HD) q = 0;
        }
        for (int dr = glo; dr <= ghi; ++dr) {
          if (side_rows) S += Hs[q * TC + c];
          if (++q == g.HD) q = 0;
        }
        for (int dr = ghi + 1; dr <= hi; ++dr) {
          S += Hf[q * TC + c];
          if (++q == g.HD) q = 0;
        }
        const float* p = Pr + rp * PW + HB + c;
        P = p[0];
        det = P > S * (a.alpha / (float)N);
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
        if (det && pos < a.K)
          list[pos] = make_float4(__int_as_float(r * ND + c0 + c), P, S / (float)N, 0.f);
        wcount += __popcll(bal);
      }
    }
    if (more && ldv) put(nxt, jp + 1 == g.PD ? 0 : jp + 1);   // that slot's row (j + 1 - PD) is below every row read above
    if (++jp == g.PD) jp = 0;
    if (++jh == g.HD) jh = 0;
  }
  if (lane == 0) a.sub_count[(size_t)f * WPF * a.waves + sub] = wcount;
}

__global__ __launch_bounds__(256) void k_cfar_gather(CfarArgs a) {
  __shared__ int cnt[kCfarMaxSub];
  __shared__ int sbase[kCfarMaxStrips + 1];
  const int tid = threadIdx.x, K = a.K;
  const int64_t f = blockIdx.x;
  const int NQ = a.tiles * a.waves, NSUB = a.strips * NQ;
  for (int i = tid; i < NSUB; i += 256) cnt[i] = a.sub_count[f * NSUB + i];
  __syncthreads();
  // detections of each strip (thread s), then the exclusive prefix over the at most 128 strips:
  // an inclusive wave scan, the second wave offset by the first one's total
  int mine = 0;
  if (tid < a.strips)
    for (int q = 0; q < NQ; ++q) mine += cnt[tid * NQ + q];
  int incl = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if ((tid & 63) >= o) incl += t;
  }
  if (tid == 63) sbase[kCfarMaxStrips] = incl;           // wave 0's total, parked in the last slot
  __syncthreads();
  const int w0 = sbase[kCfarMaxStrips];
  __syncthreads();
  if (tid < a.strips) sbase[tid] = incl - mine + (tid >= 64 ? w0 : 0);
  if (tid == a.strips - 1) {
    sbase[a.strips] = incl + (tid >= 64 ? w0 : 0);
    a.det_count[f] = incl + (tid >= 64 ? w0 : 0);
  }
  __syncthreads();
  const int total = sbase[a.strips];
  for (int i = min(total, K) + tid; i < K; i += 256) {
    a.det_ridx[f * K + i] = 0;
    a.det_didx[f * K + i] = 0;
    a.det_power[f * K + i] = 0.f;
    a.det_noise[f * K + i] = 0.f;
  }
  const float4* const lists = a.sub_list + (size_t)f * NSUB * K;
  int shift = 0;
  while ((1 << shift) < a.ND) ++shift;
  for (int s = 0; s < a.strips && sbase[s] < K; ++s) {
    if (sbase[s + 1] == sbase[s]) continue;
    for (int q = 0; q < NQ; ++q) {
      const int n = min(cnt[s * NQ + q], K);
      for (int i = tid; i < n; i += 256) {
        const float4 e = lists[(size_t)(s * NQ + q) * K + i];
        const int key = __float_as_int(e.x);
        int rank = sbase[s] + i;
        for (int q2 = 0; q2 < NQ; ++q2) {
          if (q2 == q) continue;
          const float4* const o = lists + (size_t)(s * NQ + q2) * K;
          int lo = 0, hi = min(cnt[s * NQ + q2], K);          // entries of list q2 before this cell
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (__float_as_int(o[mid].x) < key) lo = mid + 1;
            else hi = mid;
          }
          rank += lo;
        }
        if (rank < K) {
          a.det_ridx[f * K + rank] = (key >> shift) + 1;
          a.det_didx[f * K + rank] = (key & (a.ND - 1)) + 1;
          a.det_power[f * K + rank] = e.y;
          a.det_noise[f * K + rank] = e.z;
        }
      }
    }
  }
}

// Strip height and tiling of a launch over F frames: the tallest strip (least halo re-read) that
// still gives the device a few thousand workgroups.  The outputs do not depend on it.
void cfar_plan(CfarArgs& a, int64_t F) {
  a.TC = a.ND < kCfarTile ? a.ND : kCfarTile;
  a.tiles = a.ND / a.TC;
  a.waves = (a.TC + 63) / 64;
  const int G = a.g1 - a.g0 + 1;
  for (int rs = 128;; rs >>= 1) {
    a.RS = rs;
    a.strips = (G + rs - 1) / rs;
    if (rs == 16 || F * a.strips * a.tiles >= 2048) break;
  }
}

size_t cfar_scratch_per_frame(const CfarArgs& a) {
  const size_t nsub = (size_t)a.strips * a.tiles * a.waves;
  return nsub * ((size_t)a.K * sizeof(float4) + sizeof(int32_t));
}

hipError_t launch_cfar(const CfarArgs& a, hipStream_t s) {
  if (a.F <= 0) return hipSuccess;
  const CfarGeom g = cfar_geom(a);
  const int64_t wgs = a.F * a.strips * a.tiles;
  if (a.strips < 1 || a.strips > kCfarMaxStrips || a.strips * a.tiles * a.waves > kCfarMaxSub || wgs > 0x7fffffffLL ||
      a.TC * a.tiles != a.ND || a.waves * 64 < a.TC || a.waves > 4 || g.PW / (a.h ? 4 : 2) > a.waves * 64 ||
      g.Wd > g.HB || 2 * g.Wd + 1 > a.ND || 2 * g.Wr + 1 > a.NR || a.g0 < 0 || a.g1 >= a.NR || a.g0 > a.g1 ||
      (a.g1 - a.g0 + 1 + a.RS - 1) / a.RS != a.strips || a.K < 1)
    return hipErrorInvalidValue;
  const size_t shmem = ((size_t)g.PD * g.PW + 2 * (size_t)g.HD * a.TC) * sizeof(float);
  if (shmem > 160 * 1024) return hipErrorInvalidValue;
  if (shmem > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_cfar),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cfar, dim3((unsigned)wgs), dim3(a.waves * 64), shmem, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cfar_gather, dim3((unsigned)a.F), dim3(256), 0, s, a);
  return hipGetLastError();
}

// k_cfar_gather alone, over lists another kernel wrote in k_cfar's format under a cfar_plan that
// the caller checked as launch_cfar does (kernels_oscfar.hip)
hipError_t launch_cfar_gather(const CfarArgs& a, hipStream_t s) {
  if (a.F <= 0) return hipSuccess;
  if (a.strips < 1 || a.strips > kCfarMaxStrips || a.strips * a.tiles * a.waves > kCfarMaxSub || a.F > 0x7fffffffLL)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cfar_gather, dim3((unsigned)a.F), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace fmcw
