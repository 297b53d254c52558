// kernels_doa.hip -- directions of arrival for gfx950: the peaks of an angular spectrum per range
// row (Bartlett, Capon, MUSIC or a caller's own), thinned by an absolute, a relative and a
// prominence rule, ordered by power, each with a sub-grid direction from a parabola through the
// peak and its two neighbours.
//
// Definition (include/fmcw.h, fmcw_doa_params): spec [rows][K] float32 and the grid u [K] in; count
// [rows], idx, pow, sin, base [rows][max_pk] out.  Everything is float32, every operation rounded on
// its own in the order the header writes (no contraction; divides correctly rounded), so every byte
// equals the plain-loop evaluation of the same steps (tests/doa_reference.py).
//
// k_doa<NP>  A wave owns whole rows: a workgroup is four waves, a wave takes kDoaRows consecutive
//   rows one after the other and shares nothing with the other waves (no LDS, no barrier).
//   Element e of the row sits in lane e % 64 as value e / 64 ("plane" j of NP = ceil(K / 64) <= 4), so
//   that a ballot over plane j is word j of a K-bit set in index order.  Every spectrum value is
//   loaded once (a coalesced 4-byte load per lane and plane); the grid is loaded once per wave.
//   Step 0: a wave maximum and minimum by compares.
//   Step 1: neighbours by a lane rotation, the plane seam patched from the next plane; two ballots
//   per plane give the sets D (s[e+1] < s[e]) and NE (s[e+1] != s[e]), with the mode's rule at the two
//   ends.  Element e is a peak iff s[e-1] < s[e] and the first NE bit at or after e (cyclic under WRAP)
//   is a D bit: every lane finds that bit for its own elements with a count of trailing zeros on at
//   most NP words, so a flat top costs no walk.
//   Step 3's three cheap rules thin the candidates.
//   Step 2, for one candidate at a time, wave-uniform: the value is broadcast, one ballot per plane
//   marks the larger values, the nearest marked bit either side of k bounds the two walks, and the
//   two minima are one masked wave minimum each.  With min_prom > 0 every candidate needs it (at most
//   K / 2 rounds: peaks are not adjacent); with min_prom = 0 only the written peaks do, and only
//   when base was asked for.
//   Step 4: at most max_pk rounds of a wave maximum over the kept values and a ballot of the lanes that
//   hold it, whose lowest bit is the peak (ties by ascending k).  Round i's result stays in lane i.
//   Step 5 runs on wave-uniform values in the same round.
//   The results leave by one store per output from lanes 0 .. max_pk - 1 (lane 0 also stores count).
//
// Every global address is formed from blockIdx, threadIdx and the arguments alone (an index taken
// from the data only selects a lane and a register); offsets are 64-bit.  No inline assembly, no
// atomics, no scratch; every store is an ordinary vector store.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#pragma clang fp contract(off)

namespace fmcw {

namespace {

constexpr int kDoaWaves = 4;           // waves of one workgroup of k_doa
constexpr int kDoaRows = 4;            // consecutive rows of one wave
constexpr float kDoaInf = __builtin_huge_valf();

// element e (wave-uniform) of a row held as planes: value e / 64 of lane e % 64
template <int NP>
__device__ __forceinline__ float doa_pick(const float (&v)[NP], int e) {
  e = __builtin_amdgcn_readfirstlane(e);
  // one lane read per plane and a scalar select: a select among the planes first would be turned
  // into an indexed array, which the compiler then moves out of the registers
  int x = __builtin_amdgcn_readlane(__float_as_int(v[0]), e & 63);
#pragma unroll
  for (int j = 1; j < NP; ++j) {
    const int t = __builtin_amdgcn_readlane(__float_as_int(v[j]), e & 63);
    x = (e >> 6) == j ? t : x;
  }
  return __int_as_float(x);
}

// x of the lane a DPP pattern names: 0xB1 / 0x4E swap lanes 1 / 2 apart inside a quad, 0x141 mirrors a
// group of 8, 0x140 a row of 16; every pattern reads a live lane
template <int CTRL>
__device__ __forceinline__ float doa_dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), CTRL, 0xf, 0xf, false));
}

// Wave minimum and maximum by compares, wave-uniform: four DPP steps leave every row of 16 lanes with
// its own result, one lane read per row and three scalar compares join the four rows.
__device__ __forceinline__ float doa_wave_min(float m) {
  float t;
  t = doa_dpp<0xB1>(m); m = t < m ? t : m;
  t = doa_dpp<0x4E>(m); m = t < m ? t : m;
  t = doa_dpp<0x141>(m); m = t < m ? t : m;
  t = doa_dpp<0x140>(m); m = t < m ? t : m;
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 48));
  const float a = r1 < r0 ? r1 : r0, b = r3 < r2 ? r3 : r2;
  return b < a ? b : a;
}

__device__ __forceinline__ float doa_wave_max(float m) {
  float t;
  t = doa_dpp<0xB1>(m); m = t > m ? t : m;
  t = doa_dpp<0x4E>(m); m = t > m ? t : m;
  t = doa_dpp<0x141>(m); m = t > m ? t : m;
  t = doa_dpp<0x140>(m); m = t > m ? t : m;
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 48));
  const float a = r1 > r0 ? r1 : r0, b = r3 > r2 ? r3 : r2;
  return b > a ? b : a;
}

// Step 2 for the peak k of value c (both wave-uniform): the larger of the two sides' minima.
template <int NP>
__device__ __forceinline__ float doa_base(const float (&v)[NP], int K, int lane, bool wrap, int k, float c) {
  k = __builtin_amdgcn_readfirstlane(k);
  unsigned long long G[NP];
  bool any = false;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    G[j] = __ballot(64 * j + lane < K && v[j] > c);
    any = any || G[j] != 0;
  }
  const int kw = k >> 6, kb = k & 63;
  int la = -1, rb = -1, top = -1, bot = -1;    // nearest larger value below / above k; the highest / lowest of all
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const unsigned long long below = j < kw ? G[j] : j == kw ? G[j] & ((1ull << kb) - 1ull) : 0ull;
    if (below) la = 64 * j + 63 - __builtin_clzll(below);
    if (G[j]) top = 64 * j + 63 - __builtin_clzll(G[j]);
  }
#pragma unroll
  for (int j = NP - 1; j >= 0; --j) {
    const unsigned long long above = j > kw ? G[j] : j == kw ? (kb == 63 ? 0ull : G[j] & (~0ull << (kb + 1))) : 0ull;
    if (above) rb = 64 * j + __builtin_ctzll(above);
    if (G[j]) bot = 64 * j + __builtin_ctzll(G[j]);
  }
  // left: la < e < k, or under WRAP with nothing larger below k: e < k or e > la (la: the highest
  // larger value, or k itself when nothing is larger: every other element).  right likewise.
  bool lw = false, rw = false;
  if (la < 0 && wrap) {
    lw = true;
    la = any ? top : k;
  }
  if (rb < 0) {
    if (wrap) {
      rw = true;
      rb = any ? bot : k;
    } else {
      rb = K;
    }
  }
  const int nl = lw ? k + (K - 1 - la) : k - 1 - la;
  const int nr = rw ? (K - 1 - k) + rb : rb - 1 - k;
  float lmin = kDoaInf, rmin = kDoaInf;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int e = 64 * j + lane;
    const bool ok = e < K;
    const bool inl = ok && (lw ? (e < k || e > la) : (e > la && e < k));
    const bool inr = ok && (rw ? (e > k || e < rb) : (e > k && e < rb));
    if (inl) lmin = v[j] < lmin ? v[j] : lmin;
    if (inr) rmin = v[j] < rmin ? v[j] : rmin;
  }
  lmin = doa_wave_min(lmin);
  rmin = doa_wave_min(rmin);
  float base = nl > 0 ? lmin : rmin;
  if (nl > 0 && nr > 0) base = lmin > rmin ? lmin : rmin;
  return base + 0.f;                             // a zero base is +0
}

// Step 5 for the written peak k of value c (wave-uniform): its sub-grid direction.
template <int NP>
__device__ __forceinline__ float doa_refine(const float (&v)[NP], const float (&u)[NP], int K, bool wrap, bool inv, int k, float c) {
  int kl = k - 1, kr = k + 1;
  if (wrap) {
    kl = kl < 0 ? K - 1 : kl;
    kr = kr == K ? 0 : kr;
  }
  const float uk = doa_pick(u, k);
  if (kl < 0 || kr >= K) return uk;              // a neighbour is missing
  float l = doa_pick(v, kl), r = doa_pick(v, kr);
  float delta = 0.f;
  bool ok = true;
  if (inv) {
    if (l > 0.f && r > 0.f) {
      l = 1.f / l;
      c = 1.f / c;
      r = 1.f / r;
    } else {
      ok = false;
    }
  }
  if (ok) {
    const float den = (l - c) + (r - c);
    const float num = 0.5f * (l - r);
    if (den != 0.f && fabsf(den) < kDoaInf && fabsf(num) < kDoaInf) delta = num / den;
  }
  delta = delta < -0.5f ? -0.5f : delta > 0.5f ? 0.5f : delta;
  const float ul = doa_pick(u, kl), ur = doa_pick(u, kr);
  float step;
  if (delta >= 0.f) step = kr < k ? uk - ul : ur - uk;
  else step = kl > k ? ur - uk : uk - ul;
  return uk + delta * step;
}

template <int NP>
__global__ __launch_bounds__(64 * kDoaWaves) void k_doa(const DoaArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = a.K;
  const bool edges = (a.flags & FMCW_DOA_EDGES) != 0, wrap = (a.flags & FMCW_DOA_WRAP) != 0, inv = (a.flags & FMCW_DOA_INV) != 0;
  const bool all_bases = a.min_prom > 0.f;       // min_prom = 0: s[k] > 0 >= 0 * base, the rule is off
  float u[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) u[j] = 64 * j + lane < K ? a.u[64 * j + lane] : 0.f;
  const int64_t first = ((int64_t)blockIdx.x * kDoaWaves + wave) * kDoaRows;

#pragma unroll 1
  for (int it = 0; it < kDoaRows; ++it) {
    const int64_t row = first + it;
    if (row >= a.rows) break;                    // uniform
    const int r = (int)(row & (a.NR - 1));
    int n_kept = 0;
    int o_idx = -1;                              // lane i: slot i of the row
    float o_pow = 0.f, o_sin = 0.f, o_base = 0.f;
    if (r >= a.g0 && r <= a.g1) {                // uniform
      const float* const src = a.spec + row * K;
      float v[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) v[j] = 64 * j + lane < K ? src[64 * j + lane] : 0.f;
      // ---- step 0 ----
      float hi = -kDoaInf, lo = kDoaInf;
#pragma unroll
      for (int j = 0; j < NP; ++j)
        if (64 * j + lane < K) {
          hi = v[j] > hi ? v[j] : hi;
          lo = v[j] < lo ? v[j] : lo;
        }
      hi = doa_wave_max(hi);
      lo = doa_wave_min(lo);
      if (hi > lo && hi > 0.f) {                 // uniform
        // ---- step 1 ----
        const float s_first = doa_pick(v, 0), s_last = doa_pick(v, K - 1);
        unsigned long long MD[NP], MNE[NP];
        bool cand[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          const int e = 64 * j + lane;
          const bool ok = e < K;
          float p = __shfl(v[j], (lane + 63) & 63);
          if (j > 0) {
            const float q = __shfl(v[j - 1], 63);
            p = lane == 0 ? q : p;
          }
          float n = __shfl(v[j], (lane + 1) & 63);
          if (j + 1 < NP) {
            const float q = __shfl(v[j + 1], 0);
            n = lane == 63 ? q : n;
          }
          bool has_l = e > 0, has_r = e < K - 1;
          if (wrap) {
            p = e == 0 ? s_last : p;
            n = e == K - 1 ? s_first : n;
            has_l = has_r = true;
          }
          cand[j] = ok && (has_l ? p < v[j] : edges);
          const bool d = ok && (has_r ? n < v[j] : edges);
          const bool up = ok && has_r && n > v[j];
          MD[j] = __ballot(d);
          MNE[j] = __ballot(d || up);
        }
        const float t_rel = a.min_rel * hi;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          // the first NE bit at or after e, cyclic under WRAP; -1: the walk reaches the end
          int pos = -1;
#pragma unroll
          for (int w = j; w < NP; ++w) {
            const unsigned long long word = w == j ? MNE[w] & (~0ull << lane) : MNE[w];
            if (pos < 0 && word) pos = 64 * w + __builtin_ctzll(word);
          }
          if (wrap) {
#pragma unroll
            for (int w = 0; w <= j; ++w)
              if (pos < 0 && MNE[w]) pos = 64 * w + __builtin_ctzll(MNE[w]);
          }
          bool falls = false;
#pragma unroll
          for (int w = 0; w < NP; ++w)
            if ((pos >> 6) == w) falls = (MD[w] >> (pos & 63)) & 1ull;
          // ---- step 3, the cheap rules ----
          cand[j] = cand[j] && falls && v[j] > 0.f && v[j] >= a.min_abs && v[j] >= t_rel;
        }
        // ---- steps 2 and 3: the prominence rule, one candidate at a time ----
        float bs[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) bs[j] = 0.f;
        if (all_bases) {
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            unsigned long long m = __ballot(cand[j]);
            while (m) {                          // uniform; at most 32 rounds per plane
              const int b = __builtin_ctzll(m);
              m &= m - 1;
              const float c = doa_pick(v, 64 * j + b);
              const float base = doa_base(v, K, lane, wrap, 64 * j + b, c);
              const bool keep = c >= a.min_prom * base;
              if (lane == b) {
                bs[j] = base;
                cand[j] = keep;
              }
            }
          }
        }
        // ---- step 4 ----
#pragma unroll
        for (int j = 0; j < NP; ++j) n_kept += __popcll(__ballot(cand[j]));
        const int rounds = min(n_kept, a.max_pk);
#pragma unroll 1
        for (int i = 0; i < rounds; ++i) {
          // the largest kept value (kept peaks are positive), then the lowest index that holds it
          float best = 0.f;
#pragma unroll
          for (int j = 0; j < NP; ++j)
            if (cand[j] && v[j] > best) best = v[j];
          const float c = doa_wave_max(best);
          int k = -1;
#pragma unroll
          for (int j = NP - 1; j >= 0; --j) {
            const unsigned long long eq = __ballot(cand[j] && v[j] == c);
            if (eq) k = 64 * j + __builtin_ctzll(eq);
          }
#pragma unroll
          for (int j = 0; j < NP; ++j)
            if (64 * j + lane == k) cand[j] = false;
          float base = 0.f, sn = 0.f;
          if (all_bases) base = doa_pick(bs, k);
          else if (a.base) base = doa_base(v, K, lane, wrap, k, c);
          if (a.sn) sn = doa_refine(v, u, K, wrap, inv, k, c);
          if (lane == i) {
            o_idx = k;
            o_pow = c;
            o_sin = sn;
            o_base = base;
          }
        }
      }
    }
    if (lane < a.max_pk) {
      const int64_t o = row * a.max_pk + lane;
      if (a.idx) a.idx[o] = o_idx;
      if (a.pw) a.pw[o] = o_pow;
      if (a.sn) a.sn[o] = o_sin;
      if (a.base) a.base[o] = o_base;
    }
    if (lane == 0 && a.count) a.count[row] = n_kept;
  }
}

}  // namespace

hipError_t launch_doa(const DoaArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.K < 1 || a.K > kRaAngMax || a.NR < 16 || (a.NR & (a.NR - 1)) || (a.rows & (a.NR - 1)) || a.rows > kRaRowsMax || a.g0 < 0 ||
      a.g1 >= a.NR || a.g0 > a.g1 || a.max_pk < 1 || a.max_pk > kDoaPkMax || !a.spec || !a.u ||
      (a.flags & ~(FMCW_DOA_EDGES | FMCW_DOA_WRAP | FMCW_DOA_INV)) || ((a.flags & FMCW_DOA_EDGES) && (a.flags & FMCW_DOA_WRAP)) ||
      ((a.flags & FMCW_DOA_WRAP) && a.K < 3) || !(a.count || a.idx || a.pw || a.sn || a.base) ||
      ((reinterpret_cast<uintptr_t>(a.spec) | reinterpret_cast<uintptr_t>(a.u) | reinterpret_cast<uintptr_t>(a.count) |
        reinterpret_cast<uintptr_t>(a.idx) | reinterpret_cast<uintptr_t>(a.pw) | reinterpret_cast<uintptr_t>(a.sn) |
        reinterpret_cast<uintptr_t>(a.base)) & 3))
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)kDoaWaves * kDoaRows;
  const unsigned blocks = (unsigned)((a.rows + per - 1) / per);
  const dim3 block(64 * kDoaWaves);
  switch ((a.K + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_doa<1>), dim3(blocks), block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_doa<2>), dim3(blocks), block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_doa<3>), dim3(blocks), block, 0, s, a); break;
    default: hipLaunchKernelGGL((k_doa<4>), dim3(blocks), block, 0, s, a); break;
  }
  return hipGetLastError();
}

}  // namespace fmcw
