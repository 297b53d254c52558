// kernels_ra.hip -- range-angle maps from several receive channels' RD maps, for gfx950: the spatial
// covariance of the channels per range row, and the Bartlett and Capon angular spectra taken from it.
//
// Definition (include/fmcw.h, fmcw_ra_params): A channel maps [F][nr][nd] of one dtype in.
//   cov[f][r][t] = R_ab = sum over the kept Doppler bins d of x_a[r][d] conj(x_b[r][d]), a <= b,
//                  t = a A - a (a - 1) / 2 + (b - a), (re, im) float32; a diagonal entry has im = +0;
//                  rows outside the gate are zero; fp16 storage: the sums times ((float)nr (float)nd)^2.
//   ra[f][r][k]  = the power of look direction k, from the float32 cov bytes and w[k][a] alone, by the
//                  steps of the header: every operation rounded on its own, in the order written.
//
// k_cov  A streaming kernel: every input byte is read once, 16 bytes per lane (2 complex64 or 4
//   fp16-storage cells), the same piece of all A channels loaded together (nontemporal: touched once).
//   A wave owns whole rows, so nothing crosses waves: no LDS, no barrier, no atomics, no scratch.
//     LPR = nd / cells per lane = 16-byte pieces of a row.
//     FULL (LPR >= 64): a row is LPR / 64 wave-loads of one wave (a wave takes rpw consecutive rows, one
//       after the other); a lane adds the products of its cells into the row's 2T sums (real and
//       imaginary parts in two register arrays, so that two neighbouring entries make one packed
//       multiply-add; diagonal im a constant 0) in ascending chunk and cell order.  The row reduction
//       goes top down, four values at a time, in the row's memory order: a 16-lane
//       swap of (v0, v1) and of (v2, v3) with one add each leaves two registers whose 16-lane rows
//       alternate between the two values, a 32-lane swap of those with one add leaves ONE register
//       whose row rho holds the partial sums of value rho, and the four DPP levels (xor 1, xor 2,
//       half mirror and mirror on group-uniform values) finish all four at once: 10 instructions for
//       four values where a butterfly per value takes 40.  Every pairing is symmetric (a + b == b + a),
//       so all 16 lanes of a row end with the same bits.  Lane (rho, j) then picks register j and
//       stores float 4 j + rho of the row: one coalesced store of 64 floats (two at A = 8).
//     narrow rows (LPR < 64): a wave-load spans 64 / LPR consecutive rows (they follow each other
//       in memory, across frames too); the LPR lanes of a row are combined by k_sig's butterfly per
//       value and the row's first lane stores it.  A row that is not the launch's or not in the gate
//       has its cells selected to 0, so it sums to +0.
//   The left-out Doppler band is a per-lane predicate that selects the cell's values to 0 before the
//   products (never a subtraction), so a non-finite value there or outside the gate touches nothing.
//   The order of every sum is a function of (A, nd, dtype) alone: the bytes do not depend on F, on
//   the launch cut or on the call.
//
// k_ra   A workgroup of 256 threads owns 64 consecutive rows.  Their packed R, which is contiguous,
//   is copied to LDS in one coalesced pass.  Capon: a THREAD per row factors M = R + delta I
//   (Cholesky, in registers: the kernel is templated on A, every index is a constant) and writes L
//   over R, so a row is factored once and not once per lane.  Then a wave per row and a lane per look
//   direction (directions l, l + 64, ...): what depends on the direction alone (Bartlett's
//   c = w_a conj(w_b), Capon's u and e) is formed once and kept in registers over the wave's 16
//   rows, whose R or L is read from LDS at a wave-uniform address (a broadcast); per row and
//   direction that leaves Bartlett's T products and sums, or Capon's forward substitution and one
//   divide.  The operations and their order are those of the header, whoever executes them.  Rows
//   outside the gate and degenerate rows write zeros.  The maximum is raised by one integer atomic
//   max per workgroup on the float's bits, skipped when the value read first is already as large.
//
// Addresses are formed from blockIdx, threadIdx and the arguments alone, never from data; offsets
// are 64-bit.  No inline assembly; every store is an ordinary vector store.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#pragma clang fp contract(off)

namespace fmcw {

namespace {

typedef float ra_f4 __attribute__((ext_vector_type(4)));
typedef float ra_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 ra_h8 __attribute__((ext_vector_type(8)));

// DPP lane read; old = 0 with bound_ctrl lets the compiler fuse the move into the consuming add
// (every control used here reads a lane of the same row, so no lane reads the old value)
template <int CTRL>
__device__ inline float ra_dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// (r0, r1) of v_permlane16_swap / v_permlane32_swap on (x, y): the odd 16-lane rows (the upper 32
// lanes) of x trade places with the even rows (the lower 32 lanes) of y
template <int H>
__device__ inline float ra_swap_sum(float x, float y) {
  if constexpr (H == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
}

// the four DPP levels of a 16-lane row: every lane of the row ends with the row's sum
__device__ inline float ra_row_sum(float s) {
  s += ra_dpp<0xB1>(s);      // quad_perm [1,0,3,2]
  s += ra_dpp<0x4E>(s);      // quad_perm [2,3,0,1]
  s += ra_dpp<0x141>(s);     // row_half_mirror: quads are uniform, so this is xor 4
  s += ra_dpp<0x140>(s);     // row_mirror: 8-lane groups are uniform, so this is xor 8
  return s;
}

// k_sig's butterfly over the aligned group of W <= 32 lanes (a power of two, wave-uniform)
__device__ inline float ra_group_sum(float s, int W) {
  if (W > 1) s += ra_dpp<0xB1>(s);
  if (W > 2) s += ra_dpp<0x4E>(s);
  if (W > 4) s += ra_dpp<0x141>(s);
  if (W > 8) s += ra_dpp<0x140>(s);
  if (W > 16) s = ra_swap_sum<16>(s, s);
  return s;
}

// one 16-byte piece as (re, im) floats of its cells
template <bool H>
__device__ inline void ra_widen(const ra_f4 v, float* x) {
  if constexpr (H) {
    const ra_h8 h = __builtin_bit_cast(ra_h8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (float)h[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = v[j];
  }
}

constexpr int ra_tri(int A, int a, int b) { return a * A - a * (a - 1) / 2 + (b - a); }

// The row's sums in registers, shaped for packed multiply-adds.  Entry (p, q), p <= q, lives in the
// pair of columns (q & ~1, q | 1) of row p: re[p][q / 2] and im[p][q / 2] hold both columns, the
// channels' values come as the same column pairs, and the factor of channel p is one value for both
// halves.  The two entries of a row whose pair would straddle its start -- re (p, p) for odd p,
// im (p, p + 1) for even p -- are kept as scalars.
template <int A>
struct RaSums {
  static constexpr int P2 = (A + 1) / 2;
  ra_f2 re[A][P2], im[A][P2];
  float re1[A], im1[A];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int p = 0; p < A; ++p) {
      re1[p] = im1[p] = 0.f;
#pragma unroll
      for (int k = 0; k < P2; ++k) re[p][k] = im[p][k] = ra_f2{0.f, 0.f};
    }
  }
  // the products of one cell: xr2 / xi2 the channels' real / imaginary parts in column pairs
  __device__ __forceinline__ void add(const ra_f2 (&xr2)[P2], const ra_f2 (&xi2)[P2]) {
#pragma unroll
    for (int p = 0; p < A; ++p) {
      const float xr = xr2[p / 2][p & 1], xi = xi2[p / 2][p & 1];
      const ra_f2 rp = {xr, xr}, ip = {xi, xi};
      if (p & 1) {
        re1[p] = fmaf(xr, xr, re1[p]);
        re1[p] = fmaf(xi, xi, re1[p]);
      } else if (p + 1 < A) {
        im1[p] = fmaf(xi, xr2[p / 2][1], im1[p]);
        im1[p] = fmaf(-xr, xi2[p / 2][1], im1[p]);
      }
#pragma unroll
      for (int k = (p + 1) / 2; k < P2; ++k) {
        re[p][k] = __builtin_elementwise_fma(rp, xr2[k], re[p][k]);
        re[p][k] = __builtin_elementwise_fma(ip, xi2[k], re[p][k]);
      }
#pragma unroll
      for (int k = p / 2 + 1; k < P2; ++k) {
        im[p][k] = __builtin_elementwise_fma(ip, xr2[k], im[p][k]);
        im[p][k] = __builtin_elementwise_fma(-rp, xi2[k], im[p][k]);
      }
    }
  }
  // the row's output in memory order: entry t of the packed upper triangle at val[2 t] (re), val[2 t + 1] (im)
  __device__ __forceinline__ void flat(float (&val)[A * (A + 1)]) const {
#pragma unroll
    for (int p = 0; p < A; ++p)
#pragma unroll
      for (int q = p; q < A; ++q) {
        const int t = ra_tri(A, p, q);
        val[2 * t] = ((p & 1) && q == p) ? re1[p] : re[p][q / 2][q & 1];
        val[2 * t + 1] = q == p ? 0.f : (!(p & 1) && q == p + 1) ? im1[p] : im[p][q / 2][q & 1];
      }
  }
  template <typename F>
  __device__ __forceinline__ void each(F&& f) {               // x = f(x) for every sum that is not a constant 0
#pragma unroll
    for (int p = 0; p < A; ++p) {
      if (p & 1) re1[p] = f(re1[p]);
      else if (p + 1 < A) im1[p] = f(im1[p]);
#pragma unroll
      for (int k = (p + 1) / 2; k < P2; ++k) {
        re[p][k].x = f(re[p][k].x);
        if (2 * k + 1 < A) re[p][k].y = f(re[p][k].y);
      }
#pragma unroll
      for (int k = p / 2 + 1; k < P2; ++k) {
        im[p][k].x = f(im[p][k].x);
        if (2 * k + 1 < A) im[p][k].y = f(im[p][k].y);
      }
    }
  }
};

// The cells of one 16-byte piece of every channel, the left-out ones selected to 0 on the stored
// words (one word per fp16-storage cell, two per complex64 cell), into the row's sums.
template <bool H, int A>
__device__ __forceinline__ void ra_piece(const ra_f4 (&v)[A], const bool (&keep)[H ? 4 : 2], RaSums<A>& sums) {
  constexpr int CPL = H ? 4 : 2, P2 = (A + 1) / 2;
  typedef unsigned ra_u4 __attribute__((ext_vector_type(4)));
  float x[A][2 * CPL];
#pragma unroll
  for (int ch = 0; ch < A; ++ch) {
    ra_u4 u = __builtin_bit_cast(ra_u4, v[ch]);
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = keep[H ? k : k / 2] ? u[k] : 0u;
    ra_widen<H>(__builtin_bit_cast(ra_f4, u), x[ch]);
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    ra_f2 xr2[P2], xi2[P2];
#pragma unroll
    for (int k = 0; k < P2; ++k) {
      xr2[k] = ra_f2{x[2 * k][2 * j], 2 * k + 1 < A ? x[2 * k + 1 < A ? 2 * k + 1 : 0][2 * j] : 0.f};
      xi2[k] = ra_f2{x[2 * k][2 * j + 1], 2 * k + 1 < A ? x[2 * k + 1 < A ? 2 * k + 1 : 0][2 * j + 1] : 0.f};
    }
    sums.add(xr2, xi2);
  }
}

template <bool H, int A, bool FULL>
__global__ __launch_bounds__(256) void k_cov(const CovArgs a) {
  constexpr int CPL = H ? 4 : 2;                   // cells per 16-byte piece
  constexpr int T = A * (A + 1) / 2;
  constexpr int NV = 2 * T;                        // floats of one row of cov
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
  const int ND = a.ND, LPR = ND / CPL;

  if constexpr (FULL) {
    const int nch = LPR >> 6;
    for (int rw = 0; rw < a.rpw; ++rw) {
      const int64_t row = unit * a.rpw + rw;       // wave-uniform
      if (row >= a.rows) return;
      float* const out = a.cov + row * NV;
      const int r = (int)(row & (a.NR - 1));
      if (r < a.g0 || r > a.g1) {
        for (int i = lane; i < NV; i += 64) out[i] = 0.f;
        continue;
      }
      RaSums<A> sums;
      sums.clear();
      const int64_t rowoff = row * LPR * 16;       // wave-uniform byte offset of the row in every map
      for (int c = 0; c < nch; ++c) {
        const unsigned off = (unsigned)(c * 64 + lane) * 16u;
        ra_f4 v[A];
#pragma unroll
        for (int ch = 0; ch < A; ++ch)
          v[ch] = __builtin_nontemporal_load(reinterpret_cast<const ra_f4*>(static_cast<const char*>(a.rd[ch]) + rowoff + off));
        bool keep[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          const int d = (c * 64 + lane) * CPL + j, dist = abs(d - ND / 2);
          keep[j] = min(dist, ND - dist) > a.dc;
        }
        ra_piece<H, A>(v, keep, sums);
      }
      // four values per register, in the row's memory order:
      // 16-lane swaps, a 32-lane swap, then the four DPP levels
      constexpr int Q = (NV + 3) / 4;
      float val[NV], red[Q];
      sums.flat(val);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float v0 = val[4 * q], v1 = val[4 * q + 1];
        const float v2 = 4 * q + 2 < NV ? val[4 * q + 2] : 0.f, v3 = 4 * q + 3 < NV ? val[4 * q + 3] : 0.f;
        const float s01 = ra_swap_sum<16>(v0, v1);   // rows: v0, v1, v0, v1
        const float s23 = ra_swap_sum<16>(v2, v3);
        red[q] = ra_row_sum(ra_swap_sum<32>(s01, s23));   // row rho: value 4 q + rho
      }
      const int j = lane & 15, rho = lane >> 4;
#pragma unroll
      for (int q0 = 0; q0 < Q; q0 += 16) {
        float s = 0.f;
#pragma unroll
        for (int q = q0; q < Q && q < q0 + 16; ++q) s = j == q - q0 ? red[q] : s;
        const int i = 4 * (q0 + j) + rho;
        if (i < NV) out[i] = s * a.scale2;
      }
    }
  } else {
    // LPR < 64: the wave-load holds 64 / LPR rows, lane group g = row, piece index = unit * 64 + lane
    const int W = LPR, lw = __builtin_ctz(W);
    const int64_t row = (unit * 64 + lane) >> lw;
    const bool ok = row < a.rows;
    const int r = (int)(row & (a.NR - 1));
    const bool live = ok && r >= a.g0 && r <= a.g1;
    const int jl = lane & (W - 1);
    // a lane past the launch's rows re-reads the last piece (never a byte outside the maps) and counts as zero
    const int64_t p = min(unit * 64 + lane, a.rows * W - 1);
    ra_f4 v[A];
#pragma unroll
    for (int ch = 0; ch < A; ++ch) v[ch] = __builtin_nontemporal_load(static_cast<const ra_f4*>(a.rd[ch]) + p);
    bool keep[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int d = jl * CPL + j, dist = abs(d - ND / 2);
      keep[j] = live && min(dist, ND - dist) > a.dc;
    }
    RaSums<A> sums;
    sums.clear();
    ra_piece<H, A>(v, keep, sums);
    sums.each([&](float x) { return ra_group_sum(x, W); });
    if (jl == 0 && ok) {
      float2* const out = reinterpret_cast<float2*>(a.cov + row * NV);
      float val[NV];
      sums.flat(val);
#pragma unroll
      for (int t = 0; t < T; ++t) out[t] = make_float2(val[2 * t] * a.scale2, val[2 * t + 1] * a.scale2);
    }
  }
}

__device__ inline int ra_wave_max(int m) {
  for (int o = 1; o < 64; o <<= 1) m = max(m, __shfl_xor(m, o));
  return m;
}

constexpr int kRaRows = 64;            // rows of one workgroup of k_ra

template <int A, bool CAPON>
__global__ __launch_bounds__(256) void k_ra(const RaArgs a) {
  constexpr int T = A * (A + 1) / 2, NV = 2 * T;
  __shared__ float sR[kRaRows * NV];     // the rows' packed R (re, im); Capon: overwritten by the factor L
  __shared__ int sZero[kRaRows];         // the row writes zeros: outside the gate, or degenerate
  __shared__ int wm[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * kRaRows;
  const int nrows = (int)min((int64_t)kRaRows, a.rows - row0);   // a multiple of 16: rows is one of NR >= 16

  // the workgroup's rows of cov follow each other: one coalesced copy
  {
    const float4* const src = reinterpret_cast<const float4*>(a.cov + row0 * NV);
    for (int i = tid; i < nrows * NV / 4; i += 256) reinterpret_cast<float4*>(sR)[i] = src[i];
  }
  __syncthreads();
  // a thread per row: the gate, and Capon's Cholesky factor L of M = R + delta I in place of R
  // (lower triangular, L[i][j] at packed index i (i + 1) / 2 + j; every index is a constant)
  if (tid < nrows) {
    const int r = (int)((row0 + tid) & (a.NR - 1));
    bool zero = r < a.g0 || r > a.g1;
    if constexpr (CAPON) {
      float2* const mine = reinterpret_cast<float2*>(sR + tid * NV);
      float Rr[T], Ri[T], Lr[T], Li[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float2 v = mine[t];
        Rr[t] = v.x;
        Ri[t] = v.y;
      }
      float tr = 0.f;
#pragma unroll
      for (int i = 0; i < A; ++i) tr = tr + Rr[ra_tri(A, i, i)];
      const float delta = a.load * (tr / (float)A);
      bool bad = false;
#pragma unroll
      for (int i = 0; i < A; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          float sr, si;
          if (i == j) {
            sr = Rr[ra_tri(A, i, i)] + delta;
            si = 0.f;
          } else {
            sr = Rr[ra_tri(A, j, i)];
            si = -Ri[ra_tri(A, j, i)];
          }
#pragma unroll
          for (int k = 0; k < j; ++k) {
            const float ar = Lr[i * (i + 1) / 2 + k], ai = Li[i * (i + 1) / 2 + k];
            const float br = Lr[j * (j + 1) / 2 + k], bi = Li[j * (j + 1) / 2 + k];
            sr = sr - (ar * br + ai * bi);
            si = si - (ai * br - ar * bi);
          }
          if (i == j) {
            bad = bad || !(sr > 0.f && sr <= 3.402823466e38f);
            Lr[i * (i + 1) / 2 + i] = sqrtf(sr);
            Li[i * (i + 1) / 2 + i] = 0.f;
          } else {
            const float d = Lr[j * (j + 1) / 2 + j];
            Lr[i * (i + 1) / 2 + j] = sr / d;
            Li[i * (i + 1) / 2 + j] = si / d;
          }
        }
      }
      zero = zero || bad;
#pragma unroll
      for (int t = 0; t < T; ++t) mine[t] = make_float2(Lr[t], Li[t]);
    }
    sZero[tid] = zero ? 1 : 0;
  }
  __syncthreads();

  // a lane per look direction, a wave per row (rows wv, wv + 4, ...): what depends on the direction
  // alone is formed once and kept over the wave's rows; the row's R or L is read at a uniform address
  int mx = 0;                                                // bits of the largest value written (>= +0)
  for (int k = lane; k < a.n_ang; k += 64) {
    float wr[A], wi[A];
#pragma unroll
    for (int i = 0; i < A; ++i) {
      const float2 v = reinterpret_cast<const float2*>(a.w)[(int64_t)k * A + i];
      wr[i] = v.x;
      wi[i] = v.y;
    }
    [[maybe_unused]] float cr[T], ci[T];                     // Bartlett: c = w_p conj(w_q)
    [[maybe_unused]] float e = 0.f;                          // Capon: sum |u_a|^2
    if constexpr (!CAPON) {
#pragma unroll
      for (int p = 0; p < A; ++p)
#pragma unroll
        for (int q = p; q < A; ++q) {
          cr[ra_tri(A, p, q)] = wr[p] * wr[q] + wi[p] * wi[q];
          ci[ra_tri(A, p, q)] = wi[p] * wr[q] - wr[p] * wi[q];
        }
    } else {
#pragma unroll
      for (int p = 0; p < A; ++p) {
        const float ur = wr[p], ui = -wi[p];
        e = e + (ur * ur + ui * ui);
      }
    }
    for (int rr = wv; rr < nrows; rr += 4) {
      const float2* const row = reinterpret_cast<const float2*>(sR + rr * NV);
      float res;
      if constexpr (!CAPON) {
        float acc = 0.f;
#pragma unroll
        for (int p = 0; p < A; ++p)
#pragma unroll
          for (int q = p; q < A; ++q) {
            const float2 R = row[ra_tri(A, p, q)];
            // a diagonal entry is real (its im is not read) and its c.im is w.im w.re - w.re w.im = +0:
            // c.re R.re - (+0)(+0) is c.re R.re
            const float t = p == q ? cr[ra_tri(A, p, p)] * R.x : cr[ra_tri(A, p, q)] * R.x - ci[ra_tri(A, p, q)] * R.y;
            acc = p == q ? acc + t : acc + (t + t);
          }
        res = acc;
      } else {
        float yr[A], yi[A];
        float qq = 0.f;
#pragma unroll
        for (int p = 0; p < A; ++p) {
          float sr = wr[p], si = -wi[p];
#pragma unroll
          for (int b = 0; b < p; ++b) {
            const float2 L = row[p * (p + 1) / 2 + b];
            sr = sr - (L.x * yr[b] - L.y * yi[b]);
            si = si - (L.x * yi[b] + L.y * yr[b]);
          }
          const float d = row[p * (p + 1) / 2 + p].x;
          yr[p] = sr / d;
          yi[p] = si / d;
          qq = qq + (yr[p] * yr[p] + yi[p] * yi[p]);
        }
        res = qq == 0.f ? 0.f : (e * e) / qq;
      }
      if (sZero[rr]) res = 0.f;
      a.ra[(row0 + rr) * a.n_ang + k] = res;
      mx = max(mx, __float_as_int(res));
    }
  }
  if (a.ra_max) {                                            // uniform
    mx = ra_wave_max(mx);
    if (lane == 0) wm[wv] = mx;
    __syncthreads();
    if (tid == 0) {
      mx = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
      int* const p = reinterpret_cast<int*>(a.ra_max);
      if (mx > __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMax(p, mx);
    }
  }
}

template <bool H, int A>
void cov_launch(const CovArgs& a, unsigned blocks, bool full, hipStream_t s) {
  if (full) hipLaunchKernelGGL((k_cov<H, A, true>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_cov<H, A, false>), dim3(blocks), dim3(256), 0, s, a);
}

template <bool H>
void cov_launch_chan(const CovArgs& a, unsigned blocks, bool full, hipStream_t s) {
  switch (a.A) {
    case 2: cov_launch<H, 2>(a, blocks, full, s); break;
    case 3: cov_launch<H, 3>(a, blocks, full, s); break;
    case 4: cov_launch<H, 4>(a, blocks, full, s); break;
    case 5: cov_launch<H, 5>(a, blocks, full, s); break;
    case 6: cov_launch<H, 6>(a, blocks, full, s); break;
    case 7: cov_launch<H, 7>(a, blocks, full, s); break;
    default: cov_launch<H, 8>(a, blocks, full, s); break;
  }
}

template <int A>
void ra_launch(const RaArgs& a, unsigned blocks, hipStream_t s) {
  if (a.capon) hipLaunchKernelGGL((k_ra<A, true>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_ra<A, false>), dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace

// Rows a wave takes where a row is one wave-load or more: two when a row is a single wave-load (a
// wave then moves as many bytes as with two wave-loads per row), else one.  A function of (nd, dtype)
// alone; the bytes written do not depend on it.
int cov_rows_per_wave(int nd, int h) { return nd / (h ? 4 : 2) / 64 >= 2 ? 1 : 2; }

hipError_t launch_cov(const CovArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  const int cpl = a.h ? 4 : 2;
  if (a.A < 2 || a.A > kRaChan || a.ND < 4 || a.ND > 1024 || (a.ND & (a.ND - 1)) || a.NR < 1 || (a.NR & (a.NR - 1)) ||
      (a.rows & (a.NR - 1)) || a.rows > kRaRowsMax || a.g0 < 0 || a.g1 >= a.NR || a.g0 > a.g1 || a.dc < -1 ||
      2 * a.dc + 1 >= a.ND || !a.cov || (reinterpret_cast<uintptr_t>(a.cov) & 7))
    return hipErrorInvalidValue;
  for (int ch = 0; ch < a.A; ++ch)
    if (!a.rd[ch] || (reinterpret_cast<uintptr_t>(a.rd[ch]) & 15)) return hipErrorInvalidValue;
  const int lpr = a.ND / cpl;
  const bool full = lpr >= 64;
  // waves: one per row, or one per 64 pieces of the rows that follow each other
  if (full && a.rpw != 1 && a.rpw != 2) return hipErrorInvalidValue;   // rpw divides NR
  const int64_t units = full ? a.rows / a.rpw : (a.rows * lpr + 63) / 64;
  const int64_t blocks = (units + 3) / 4;
  if (a.h) cov_launch_chan<true>(a, (unsigned)blocks, full, s);
  else cov_launch_chan<false>(a, (unsigned)blocks, full, s);
  return hipGetLastError();
}

hipError_t launch_ra(const RaArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.A < 2 || a.A > kRaChan || a.n_ang < 1 || a.n_ang > kRaAngMax || a.NR < 1 || (a.NR & (a.NR - 1)) ||
      (a.rows & (a.NR - 1)) || a.rows > kRaRowsMax || a.g0 < 0 || a.g1 >= a.NR || a.g0 > a.g1 || !a.cov || !a.w || !a.ra ||
      (reinterpret_cast<uintptr_t>(a.cov) & 15) || (reinterpret_cast<uintptr_t>(a.w) & 7) || (reinterpret_cast<uintptr_t>(a.ra) & 3) ||
      (reinterpret_cast<uintptr_t>(a.ra_max) & 3))
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((a.rows + kRaRows - 1) / kRaRows);
  switch (a.A) {
    case 2: ra_launch<2>(a, blocks, s); break;
    case 3: ra_launch<3>(a, blocks, s); break;
    case 4: ra_launch<4>(a, blocks, s); break;
    case 5: ra_launch<5>(a, blocks, s); break;
    case 6: ra_launch<6>(a, blocks, s); break;
    case 7: ra_launch<7>(a, blocks, s); break;
    default: ra_launch<8>(a, blocks, s); break;
  }
  return hipGetLastError();
}

}  // namespace fmcw
