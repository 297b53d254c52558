// kernels_music.hip -- MUSIC angular spectra from the range rows' spatial covariance, for gfx950: the
// eigen-decomposition of the A x A Hermitian covariance of every range row by a cyclic Jacobi method
// with a fixed number of sweeps, a source count, and the MUSIC pseudo-spectrum on the look
// directions of a fmcw_ra_steer table.
//
// Definition (include/fmcw.h, fmcw_music_params): cov [rows][T][2] float32 in, exactly what k_cov
// writes or a caller's own; eval [rows][A], evec [rows][A][A][2], nsrc [rows], music [rows][n_ang]
// out.  Everything is float32, every operation rounded on its own in the order the header writes
// (no contraction; divides and square roots correctly rounded), so every byte equals a float32
// numpy evaluation of the same steps (tests/music_reference.py).
//
// k_music  One wave (a workgroup of 64 threads) owns 64 consecutive rows.
//   Phase 1, a LANE per row: the row's matrix lives in registers as its upper triangle (diagonal re,
//   off-diagonal re and im: A^2 floats; M_ba is read as conj(M_ab), which is the header's rule) with
//   V beside it (2 A^2 floats): 192 floats at A = 8.  The kernel is templated on A and the p, q, k
//   loops are unrolled, so every index is a constant and nothing goes to scratch.  The rotation's
//   scalars (g, ph, tau, t, c, s: four divides and three square roots) are formed once per row and
//   pair, not once per lane of a lane group; a pair with g == 0 is skipped under the lane's own
//   predicate.  The sweep loop is not unrolled.
//   The eigenpairs leave the registers in ascending order through LDS: lane i's value of rank r
//   goes to slot r of the lane's LDS row (the rank is counted by A (A - 1) compares with constant
//   register indices; the LDS address is the only thing formed from data, and a rank lies in
//   0 .. A - 1 whatever the compares say, NaN included).  The LDS row's stride is odd in floats, so
//   the 64 lanes' stores to one slot fall in 64 different banks.  RB rows are staged at a time (64,
//   or 32 at A >= 6: half the LDS, so that LDS does not hold the waves per SIMD below what the
//   registers allow); the other half's eigenpairs wait in their registers.
//   The estimated count reads the row's sorted eigenvalues back from its own LDS slots.
//   eval, evec and nsrc are then copied LDS -> memory by the whole wave, coalesced.
//   Phase 2, a lane per look direction (directions l, l + 64, ...) over the staged rows: the
//   direction's weights and e are kept in registers, the row's eigenvectors are read from LDS at a
//   wave-uniform address (a broadcast), the noise-subspace loop j < A - n is wave-uniform.
//   The maximum is raised by one integer atomic max per wave on the float's bits, skipped when the
//   value read first is already as large.  No float atomics.
//
// Every global address is formed from blockIdx, threadIdx and the arguments alone; offsets are
// 64-bit.  No inline assembly; every store is an ordinary vector store.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#pragma clang fp contract(off)

namespace fmcw {

namespace {

constexpr int mu_tri(int A, int a, int b) { return a * A - a * (a - 1) / 2 + (b - a); }

__device__ inline int mu_wave_max(int m) {
  for (int o = 1; o < 64; o <<= 1) m = max(m, __shfl_xor(m, o));
  return m;
}

// (c x - conj(sp) y, sp x + c y): four real products per complex product, each pair's sum or
// difference rounded, then combined with the c term
__device__ __forceinline__ void mu_rot(float& xr, float& xi, float& yr, float& yi, float c, float sr, float si) {
  const float nxr = c * xr - (sr * yr + si * yi);
  const float nxi = c * xi - (sr * yi - si * yr);
  const float nyr = (sr * xr - si * xi) + c * yr;
  const float nyi = (sr * xi + si * xr) + c * yi;
  xr = nxr; xi = nxi; yr = nyr; yi = nyi;
}

constexpr int kMuRows = 64;            // rows of one workgroup (one wave) of k_music

template <int A>
struct MuShape {
  static constexpr int T = A * (A + 1) / 2;
  static constexpr int EV = 2 * A * A;                         // floats of one row's eigenvectors
  static constexpr int ST = (EV + A) | 1;                      // floats of one LDS row: evec, eval; odd
  static constexpr int RB = A >= 6 ? 32 : 64;                  // rows staged in LDS at a time
};

template <int A>
__global__ __launch_bounds__(64) void k_music(const MusicArgs a) {
  using S = MuShape<A>;
  constexpr int T = S::T, EV = S::EV, ST = S::ST, RB = S::RB;
  __shared__ float sE[RB * ST];          // per staged row: evec[j][a] (re, im) ascending in j, then eval[j]
  __shared__ int sN[RB];                 // the row's source count; -1: outside the gate (writes zeros)
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kMuRows;
  const int nrows = (int)min((int64_t)kMuRows, a.rows - row0);   // a multiple of 16: rows is one of NR >= 16
  const bool mine = lane < nrows;
  const int r = (int)((row0 + lane) & (a.NR - 1));
  const bool gated = mine && r >= a.g0 && r <= a.g1;

  // ---- phase 1: a lane per row ----
  float Mr[T], Mi[T];                    // the upper triangle; Mi of a diagonal entry is never read
  float Vr[A][A], Vi[A][A];
#pragma unroll
  for (int t = 0; t < T; ++t) Mr[t] = Mi[t] = 0.f;
  if (gated) {
    const float2* const src = reinterpret_cast<const float2*>(a.cov) + (row0 + lane) * T;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float2 v = src[t];
      Mr[t] = v.x;
      Mi[t] = v.y;
    }
  }
#pragma unroll
  for (int i = 0; i < A; ++i) Mi[mu_tri(A, i, i)] = 0.f;
  if (a.fb) {                            // uniform: forward-backward averaging from the original R
    float Fr[T], Fi[T];
#pragma unroll
    for (int p = 0; p < A; ++p)
#pragma unroll
      for (int q = p; q < A; ++q) {
        const int t = mu_tri(A, p, q), u = mu_tri(A, A - 1 - q, A - 1 - p);
        Fr[t] = 0.5f * (Mr[t] + Mr[u]);
        Fi[t] = p == q ? 0.f : 0.5f * (Mi[t] + Mi[u]);
      }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      Mr[t] = Fr[t];
      Mi[t] = Fi[t];
    }
  }
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int j = 0; j < A; ++j) {
      Vr[i][j] = i == j ? 1.f : 0.f;
      Vi[i][j] = 0.f;
    }

#pragma nounroll
  for (int sw = 0; sw < a.sweeps; ++sw) {
#pragma unroll
    for (int p = 0; p < A - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < A; ++q) {
        const int tpq = mu_tri(A, p, q), tpp = mu_tri(A, p, p), tqq = mu_tri(A, q, q);
        const float hr = Mr[tpq], hi = Mi[tpq];
        const float g = sqrtf(hr * hr + hi * hi);
        if (g != 0.f) {
          const float phr = hr / g, phi = hi / g;
          const float da = Mr[tpp], db = Mr[tqq];
          const float tau = (db - da) / (2.f * g);
          const float at = fabsf(tau);
          float t = 1.f / (at + sqrtf(1.f + at * at));
          t = tau < 0.f ? -t : t;
          const float c = 1.f / sqrtf(1.f + t * t);
          const float s = t * c;
          const float sr = s * phr, si = s * phi;
#pragma unroll
          for (int k = 0; k < A; ++k) {
            if (k == p || k == q) continue;
            // x = M_kp, y = M_kq: the stored entry, or the conjugate of its mirror
            const int ix = k < p ? mu_tri(A, k, p) : mu_tri(A, p, k);
            const int iy = k < q ? mu_tri(A, k, q) : mu_tri(A, q, k);
            float xr = Mr[ix], xi = k < p ? Mi[ix] : -Mi[ix];
            float yr = Mr[iy], yi = k < q ? Mi[iy] : -Mi[iy];
            mu_rot(xr, xi, yr, yi, c, sr, si);
            Mr[ix] = xr;
            Mi[ix] = k < p ? xi : -xi;
            Mr[iy] = yr;
            Mi[iy] = k < q ? yi : -yi;
          }
          const float tg = t * g;
          Mr[tpp] = da - tg;
          Mr[tqq] = db + tg;
          Mr[tpq] = 0.f;
          Mi[tpq] = 0.f;
#pragma unroll
          for (int k = 0; k < A; ++k) mu_rot(Vr[k][p], Vi[k][p], Vr[k][q], Vi[k][q], c, sr, si);
        }
      }
  }

  // the rank of every eigenvalue: ascending, ties by original index
  float lam[A];
  int rk[A];
#pragma unroll
  for (int i = 0; i < A; ++i) lam[i] = Mr[mu_tri(A, i, i)];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < A; ++j) {
      if (j < i) n += lam[j] <= lam[i] ? 1 : 0;
      if (j > i) n += lam[j] < lam[i] ? 1 : 0;
    }
    rk[i] = n;
  }

  int mx = 0;                                                  // bits of the largest value written (>= +0)
#pragma unroll 1
  for (int b0 = 0; b0 < nrows; b0 += RB) {                     // uniform
    const int nb = min(RB, nrows - b0);
    const int lr = lane - b0;                                  // the lane's staged row
    if (lr >= 0 && lr < nb) {
      float* const me = sE + lr * ST;
      int n = -1;
      if (gated) {
#pragma unroll
        for (int i = 0; i < A; ++i) {
          me[EV + rk[i]] = lam[i];
#pragma unroll
          for (int k = 0; k < A; ++k) {
            me[(rk[i] * A + k) * 2] = Vr[k][i];
            me[(rk[i] * A + k) * 2 + 1] = Vi[k][i];
          }
        }
        if (a.n_src) {
          n = a.n_src;
        } else {                                               // the sorted eigenvalues, from the lane's own slots
          const int nn = A - a.max_src;
          float nu = 0.f;
#pragma unroll
          for (int j = 0; j < A; ++j)
            if (j < nn) nu = nu + me[EV + j];
          nu = nu / (float)nn;
          const float thr = a.src_thr * nu;
          int cnt = 0;
#pragma unroll
          for (int j = 0; j < A; ++j) cnt += me[EV + j] > thr ? 1 : 0;
          n = min(a.max_src, cnt);
        }
      } else {
#pragma unroll
        for (int i = 0; i < EV + A; ++i) me[i] = 0.f;
      }
      sN[lr] = n;
    }
    __syncthreads();

    // coalesced copies of what was asked for
    const int64_t rb = row0 + b0;
    if (a.evec)
      for (int i = lane; i < nb * EV; i += 64) a.evec[rb * EV + i] = sE[(i / EV) * ST + i % EV];
    if (a.eval)
      for (int i = lane; i < nb * A; i += 64) a.eval[rb * A + i] = sE[(i / A) * ST + EV + i % A];
    if (a.nsrc && lane < nb) a.nsrc[rb + lane] = max(sN[lane], 0);

    // ---- phase 2: a lane per look direction, the staged rows one after the other ----
    if (a.music) {
      for (int k = lane; k < a.n_ang; k += 64) {
        float wr[A], wi[A];
        float e = 0.f;
#pragma unroll
        for (int i = 0; i < A; ++i) {
          const float2 v = reinterpret_cast<const float2*>(a.w)[(int64_t)k * A + i];
          wr[i] = v.x;
          wi[i] = v.y;
          e = e + (wr[i] * wr[i] + wi[i] * wi[i]);
        }
        for (int rr = 0; rr < nb; ++rr) {
          const float* const row = sE + rr * ST;
          const int n = sN[rr];                                // uniform
          float den = 0.f;
#pragma unroll
          for (int j = 0; j < A; ++j) {
            if (j < A - n) {
              float pr = 0.f, pi = 0.f;
#pragma unroll
              for (int i = 0; i < A; ++i) {
                const float vr = row[(j * A + i) * 2], vi = row[(j * A + i) * 2 + 1];
                pr = pr + (wr[i] * vr - wi[i] * vi);
                pi = pi + (wr[i] * vi + wi[i] * vr);
              }
              den = den + (pr * pr + pi * pi);
            }
          }
          float res = den == 0.f ? 3.402823466e38f : e / den;
          if (n < 0) res = 0.f;
          a.music[(rb + rr) * a.n_ang + k] = res;
          mx = max(mx, __float_as_int(res));
        }
      }
    }
    __syncthreads();                                           // the next batch writes over the staged rows
  }
  if (a.music && a.music_max) {                                // uniform
    mx = mu_wave_max(mx);
    if (lane == 0) {
      int* const p = reinterpret_cast<int*>(a.music_max);
      if (mx > __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMax(p, mx);
    }
  }
}

}  // namespace

hipError_t launch_music(const MusicArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.A < 2 || a.A > kRaChan || a.NR < 16 || (a.NR & (a.NR - 1)) || (a.rows & (a.NR - 1)) || a.rows > kRaRowsMax || a.g0 < 0 ||
      a.g1 >= a.NR || a.g0 > a.g1 || a.n_src < 0 || a.n_src >= a.A || (a.n_src == 0 && (a.max_src < 1 || a.max_src >= a.A)) ||
      a.sweeps < 1 || a.sweeps > 16 || !a.cov || (reinterpret_cast<uintptr_t>(a.cov) & 7) ||
      !(a.eval || a.evec || a.nsrc || a.music) ||
      ((reinterpret_cast<uintptr_t>(a.eval) | reinterpret_cast<uintptr_t>(a.evec) | reinterpret_cast<uintptr_t>(a.nsrc) |
        reinterpret_cast<uintptr_t>(a.music) | reinterpret_cast<uintptr_t>(a.music_max)) & 3))
    return hipErrorInvalidValue;
  if (a.music && (!a.w || (reinterpret_cast<uintptr_t>(a.w) & 7) || a.n_ang < 1 || a.n_ang > kRaAngMax)) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((a.rows + kMuRows - 1) / kMuRows);
  switch (a.A) {
    case 2: hipLaunchKernelGGL((k_music<2>), dim3(blocks), dim3(64), 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_music<3>), dim3(blocks), dim3(64), 0, s, a); break;
    case 4: hipLaunchKernelGGL((k_music<4>), dim3(blocks), dim3(64), 0, s, a); break;
    case 5: hipLaunchKernelGGL((k_music<5>), dim3(blocks), dim3(64), 0, s, a); break;
    case 6: hipLaunchKernelGGL((k_music<6>), dim3(blocks), dim3(64), 0, s, a); break;
    case 7: hipLaunchKernelGGL((k_music<7>), dim3(blocks), dim3(64), 0, s, a); break;
    default: hipLaunchKernelGGL((k_music<8>), dim3(blocks), dim3(64), 0, s, a); break;
  }
  return hipGetLastError();
}

}  // namespace fmcw
