// kernels_track.hip -- tracks the per-frame targets across frames, for gfx950.
//
// Definition (include/fmcw.h, fmcw_track_params): per sequence max_trk slots carry id, status, hits,
// misses, age, r, v, d, power from frame to frame.  One frame step: predict rp = r + v; the cost
// c = (er*er)*wr + (x*x)*wd of every (live slot, valid measurement) pair, x the Doppler difference
// wrapped into [-nd/2, nd/2); greedy association of the admissible pairs (c <= 1) in ascending order
// of (tentative, bits of c, slot, measurement); alpha-beta update of the range, alpha update of the
// circular Doppler, coasting and freeing; births of the unassigned measurements into the free slots.
// Every float operation is rounded on its own, in the order the definition writes it: the pragma
// below keeps the compiler from contracting a multiply and an add into one FMA, which rounds once.
//
// k_track  The step is a dependency chain over the frames of a sequence: frame f + 1 needs the state
//   frame f leaves.  The parallelism is across sequences (one 64-thread workgroup, i.e. one wave, per
//   sequence) and across the slots and measurements of one frame (lane k holds slot k in registers,
//   lane j holds measurement j of the current frame), never across frames.  No LDS, no barrier, no
//   atomics, nothing passes between workgroups.
//   Cost loop: j runs over 0 .. n-1 and the measurement is read from lane j (j is the same in every
//     lane, so this is a read-lane, not a permute); each lane keeps its smallest key over the
//     measurements not yet taken.
//   Association: at most min(n, max_trk) rounds, each the wave-wide minimum of the 64-bit key
//     {tentative bit, cost bits, k, j} by a cross-lane butterfly; only the lanes whose best
//     measurement was just taken scan again.  Taking the smallest key among the pairs whose slot and
//     measurement are both still free, over and over, is the greedy pass over the sorted pairs.
//   Births: a ballot of the unassigned valid measurements and a ballot of the free slots, matched by
//     rank (the popcount below the lane).
//   Loads: the rows of frame f + 1 are loaded before the step of frame f -- they do not depend on the
//     state.  One coalesced row store per output array.
//
// Why it ends, whatever the input and state bytes hold: every loop bound comes from an argument.
//   frames         f < F                            (argument)
//   cost loop      j < n, n = clamp(tgt_count, 0, max_tgt): the data can only shorten it
//   rounds         it < min(n, max_trk); the early exit (no admissible pair left) only shortens it
//   rank search    6 halving steps
// Addresses are formed from blockIdx, f, the lane and the arguments alone: a slot index is a lane
// index (< max_trk), a measurement index is a lane index or a loop counter (< n <= max_tgt <= 64), and
// the values of range / doppler / peak_power and of the state block are only compared and copied.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

#pragma clang fp contract(off)

namespace fmcw {

namespace {

__device__ inline float tk_lane_f(float v, int j) {        // v of lane j, j the same in every lane
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

__device__ inline unsigned long long tk_wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}

// position of the q-th (0-based) set bit of m; q < popcount(m)
__device__ inline int tk_nth_set(unsigned long long m, int q) {
  int pos = 0;
  for (int w = 32; w > 0; w >>= 1) {
    const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
    if (q >= c) {
      q -= c;
      pos += w;
    }
  }
  return pos;
}

constexpr unsigned long long kNoKey = ~0ull;

__global__ __launch_bounds__(64) void k_track(const TrackArgs a) {
  const int lane = threadIdx.x;
  const int T = a.T, M = a.M;
  const bool slot = lane < T, meas = lane < M;
  const int64_t row0 = (int64_t)blockIdx.x * a.F;
  uint32_t* const st = a.state + (size_t)blockIdx.x * track_state_words(T);
  const float nd_f = (float)a.ND, half = (float)(a.ND / 2), nhalf = -half;
  const float nd05 = (float)a.ND + 0.5f, nr05 = (float)a.NR + 0.5f;
  const unsigned long long below = (1ull << lane) - 1ull;

  // the slot of this lane; a free slot is all zero
  int id = 0, status = 0, hits = 0, misses = 0, age = 0;
  float r = 0.f, v = 0.f, d = 0.f, pw = 0.f;
  if (slot) {
    const int s_in = (int)st[T + lane];
    if (s_in != 0) {
      status = s_in == 1 ? 1 : 2;
      id = (int)st[lane];
      hits = (int)st[2 * T + lane];
      misses = (int)st[3 * T + lane];
      age = (int)st[4 * T + lane];
      r = __uint_as_float(st[5 * T + lane]);
      v = __uint_as_float(st[6 * T + lane]);
      d = __uint_as_float(st[7 * T + lane]);
      pw = __uint_as_float(st[8 * T + lane]);
    }
  }
  unsigned counter = st[kTrackFields * T];

  int n_cnt = 0;
  float n_zr = 0.f, n_zd = 0.f, n_zp = 0.f;
  if (a.F > 0) {
    n_cnt = a.tgt_count[row0];
    if (meas) {
      n_zr = a.range[(size_t)row0 * M + lane];
      n_zd = a.doppler[(size_t)row0 * M + lane];
      n_zp = a.power[(size_t)row0 * M + lane];
    }
  }

  for (int64_t f = 0; f < a.F; ++f) {
    const int64_t row = row0 + f;
    const int cnt = n_cnt;
    const float zr = n_zr, zd = n_zd, zp = n_zp;
    if (f + 1 < a.F) {                                     // the next frame's rows: independent of the state
      n_cnt = a.tgt_count[row + 1];
      if (meas) {
        n_zr = a.range[(size_t)(row + 1) * M + lane];
        n_zd = a.doppler[(size_t)(row + 1) * M + lane];
        n_zp = a.power[(size_t)(row + 1) * M + lane];
      }
    }
    const int n = __builtin_amdgcn_readfirstlane(min(max(cnt, 0), M));
    const bool valid = lane < n && isfinite(zr) && isfinite(zd) && zr >= 0.5f && zr < nr05 && zd >= 0.5f && zd < nd05;

    // 1. predict
    const bool live = status != 0;
    const float rp = r + v;
    const unsigned long long tent = status == 1 ? 1ull << 46 : 0ull;
    const int id_in = id;

    // 2. the smallest key of this lane's slot over the measurements in `avail`
    auto best_of = [&](unsigned long long avail) {
      unsigned long long best = kNoKey;
      for (int j = 0; j < n; ++j) {
        if (!((avail >> j) & 1ull)) continue;
        const float er = tk_lane_f(zr, j) - rp;
        float x = tk_lane_f(zd, j) - d;
        if (x >= half) x = x - nd_f;
        else if (x < nhalf) x = x + nd_f;
        float c = er * er;
        c = c * a.wr;
        float c2 = x * x;
        c2 = c2 * a.wd;
        c = c + c2;
        if (c <= 1.0f) {                                   // c >= +0 here, so its bits order as c does
          const unsigned long long key =
              tent | ((unsigned long long)__float_as_uint(c) << 14) | ((unsigned long long)lane << 7) | (unsigned)j;
          best = key < best ? key : best;
        }
      }
      return best;
    };

    // 3. greedy association
    unsigned long long avail = __ballot(valid);
    unsigned long long best = best_of(avail);
    if (!live) best = kNoKey;
    int my_j = -1;                                         // slot lane: the measurement it was given
    int my_k = -1;                                         // measurement lane: the slot it went to
    const int rounds = min(n, T);
    for (int it = 0; it < rounds; ++it) {
      const unsigned long long m = tk_wave_min(my_j < 0 ? best : kNoKey);
      const unsigned m_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)m);
      const unsigned m_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(m >> 32));
      if ((m_lo & m_hi) == 0xffffffffu) break;             // no admissible pair is left
      const int ks = (int)((m_lo >> 7) & 127u), js = (int)(m_lo & 127u);
      if (lane == ks) my_j = js;
      if (lane == js) my_k = ks;
      avail &= ~(1ull << js);
      const bool again = my_j < 0 && best != kNoKey && (int)((unsigned)best & 127u) == js;
      if (__ballot(again)) {
        const unsigned long long nb = best_of(avail);
        if (again) best = nb;
      }
    }

    // 4. update
    const bool hit = live && my_j >= 0;
    const int src = hit ? my_j : 0;
    const float zr_j = __shfl(zr, src), zd_j = __shfl(zd, src), zp_j = __shfl(zp, src);
    if (hit) {
      const float er = zr_j - rp;
      float x = zd_j - d;
      if (x >= half) x = x - nd_f;
      else if (x < nhalf) x = x + nd_f;
      if (hits == 1) {                                     // two-point start
        r = zr_j;
        v = er;
        d = zd_j;
      } else {
        float t = a.alpha_r * er;
        r = rp + t;
        t = a.beta_r * er;
        v = v + t;
        t = a.alpha_d * x;
        float dn = d + t;
        if (dn >= nd05) dn = dn - nd_f;
        if (dn < 0.5f) dn = dn + nd_f;
        d = dn;
      }
      pw = zp_j;
      hits = (int)((unsigned)hits + 1u);
      misses = 0;
      age = (int)((unsigned)age + 1u);
      if (status == 1 && hits >= a.confirm_hits) status = 2;
    } else if (live) {
      r = rp;
      misses = (int)((unsigned)misses + 1u);
      age = (int)((unsigned)age + 1u);
      if (status == 1 || misses > a.max_coast) status = 0;
    }
    if (live && !(r >= 0.5f && r < nr05)) status = 0;     // also a NaN range
    if (status == 0) {
      id = hits = misses = age = 0;
      r = v = d = pw = 0.f;
    }

    // 5. births, matched by rank
    const bool is_free = slot && status == 0;
    const bool orphan = valid && my_k < 0;
    const unsigned long long fm = __ballot(is_free), bm = __ballot(orphan);
    const int n_new = min(__popcll(fm), __popcll(bm));
    const int s_rank = __popcll(fm & below), m_rank = __popcll(bm & below);
    const bool take = is_free && s_rank < n_new;
    const int bsrc = take ? tk_nth_set(bm, s_rank) : 0;
    const float zr_b = __shfl(zr, bsrc), zd_b = __shfl(zd, bsrc), zp_b = __shfl(zp, bsrc);
    if (take) {
      id = (int)(counter + (unsigned)s_rank + 1u);
      status = a.confirm_hits == 1 ? 2 : 1;
      hits = 1;
      misses = 0;
      age = 1;
      r = zr_b;
      v = 0.f;
      d = zd_b;
      pw = zp_b;
    }
    int tt = __shfl(id_in, my_k >= 0 ? my_k : 0);
    if (my_k < 0) tt = orphan && m_rank < n_new ? (int)(counter + (unsigned)m_rank + 1u) : 0;
    counter += (unsigned)n_new;

    // 6. outputs
    const int n_conf = __popcll(__ballot(status == 2));
    if (lane == 0) a.trk_count[row] = n_conf;
    if (slot) {
      const size_t o = (size_t)row * T + lane;
      if (a.trk_id) a.trk_id[o] = id;
      if (a.trk_status) a.trk_status[o] = status;
      if (a.trk_age) a.trk_age[o] = age;
      if (a.trk_misses) a.trk_misses[o] = misses;
      if (a.trk_range) a.trk_range[o] = r;
      if (a.trk_rate) a.trk_rate[o] = v;
      if (a.trk_doppler) a.trk_doppler[o] = d;
      if (a.trk_power) a.trk_power[o] = pw;
    }
    if (meas && a.tgt_track) a.tgt_track[(size_t)row * M + lane] = tt;
  }

  if (slot) {
    st[lane] = (uint32_t)id;
    st[T + lane] = (uint32_t)status;
    st[2 * T + lane] = (uint32_t)hits;
    st[3 * T + lane] = (uint32_t)misses;
    st[4 * T + lane] = (uint32_t)age;
    st[5 * T + lane] = __float_as_uint(r);
    st[6 * T + lane] = __float_as_uint(v);
    st[7 * T + lane] = __float_as_uint(d);
    st[8 * T + lane] = __float_as_uint(pw);
  }
  if (lane == 0) st[kTrackFields * T] = counter;
}

}  // namespace

hipError_t launch_track(const TrackArgs& a, hipStream_t s) {
  if (a.S <= 0 || a.F <= 0) return hipSuccess;
  if (a.T < 1 || a.T > kTrackMax || a.M < 1 || a.M > kTrackMax || a.S > 0x7fffffffLL || a.ND < 4 || a.NR < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_track, dim3((unsigned)a.S), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace fmcw
