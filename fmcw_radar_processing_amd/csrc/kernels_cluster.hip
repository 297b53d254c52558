// kernels_cluster.hip -- groups the CFAR detection lists into targets, for gfx950.
//
// Definition (include/fmcw.h, fmcw_cluster_params): the first n = clamp(det_count[f], 0, max_det)
// entries of frame f's lists are the cells; cells i, j are linked iff |r_i - r_j| <= link_r and the
// circular Doppler distance min(|d_i - d_j|, nd - |d_i - d_j|) <= link_d; a cluster is a connected
// component, its label the smallest list index in it.  Per cluster: the member count, the peak (the
// largest power, ties to the smallest index), the power sum, the power-weighted centroid relative to
// the peak, the extents; clusters of fewer than min_cells cells are dropped, the rest ordered by
// peak power descending (ties: label ascending).
//
// k_cluster  One workgroup per frame (64 threads when max_det <= 64, else 256), so nothing depends
//   on F.  The list (r, d, P) and the labels live in LDS.  Indices read from the lists are only ever
//   compared: every LDS or global address is formed from list positions < n, so no list content can
//   send an access out of bounds.
//   1. Candidates.  The lists are sorted by (r, d): the cells that can link to cell i are the
//      contiguous positions of the rows r_i - link_r .. r_i + link_r, found once by two binary
//      searches and kept in registers (a thread owns the positions tid, tid + T, ...).
//   2. Labels, min-label propagation with one pointer jump: lab[i] starts at i; a sweep sets lab[i]
//      to lab[m], m the smallest label among i and its linked candidates.  Only the owner writes
//      lab[i], labels only fall and always name a position of the same component, so the unordered
//      reads inside a sweep are harmless: after k sweeps lab[i] is at most the smallest position
//      within k links of i.  The sweep that changes nothing ends the loop (__syncthreads_or makes the
//      flag the same in every thread before anybody leaves); the loop is bounded by n sweeps
//      whatever the lists hold (a component's diameter is at most n - 1).  At the fixed point every
//      cell of a component carries its smallest position, whichever order the sweeps ran in.
//   3. Counts and peaks by integer LDS atomics (add; 64-bit max of {power bits, ~position}:
//      non-negative floats order as their bits, and of equal powers the smallest position wins), so
//      they do not depend on the order of arrival.
//   4. Order by counting: the kept roots are appended to a compact list (in any order), and the rank
//      of a root is the number of kept roots that come before it -- a function of the set alone.
//   5. Sums.  One wave per written target walks the list 64 positions at a time, takes the members
//      by a ballot and adds them one by one in ascending position, so power and the centroids are
//      the same bits on every call: no float atomics.
#include "fmcw_internal.h"
#include "../../include/fmcw.h"

namespace fmcw {

namespace {

constexpr int kClMaxDet = 1024;
constexpr int kClMaxTgt = 64;
constexpr int kClOwn = 4;            // positions per thread at most: 1024 / 256

__device__ inline unsigned cl_absdiff(int a, int b) {
  return a > b ? (unsigned)a - (unsigned)b : (unsigned)b - (unsigned)a;
}

__device__ inline bool cl_linked(int ri, int di, int rj, int dj, unsigned lr, unsigned ld, unsigned nd) {
  const unsigned dd = cl_absdiff(di, dj);
  return cl_absdiff(ri, rj) <= lr && min(dd, nd - dd) <= ld;
}

// first position in [0, n) whose row is >= v (or_equal false) / > v (or_equal true)
__device__ inline int cl_bound(const int* s_r, int n, long long v, bool or_equal) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const long long r = s_r[mid];
    if (or_equal ? r <= v : r < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_cluster(const ClusterArgs a) {
  extern __shared__ int cl_lds[];
  const int K = a.K;
  int* const s_r = cl_lds;
  int* const s_d = s_r + K;
  float* const s_p = reinterpret_cast<float*>(s_d + K);
  volatile int* const s_lab = s_d + 2 * K;
  int* const s_cnt = s_d + 3 * K;                          // members of the component of root i
  int* const s_pos = s_d + 4 * K;                          // 1-based place of root i among the targets, 0: dropped
  int2* const s_kept = reinterpret_cast<int2*>(s_d + 5 * K);                     // {root, peak power bits}
  unsigned long long* const s_key = reinterpret_cast<unsigned long long*>(s_d + 7 * K);
  int* const s_troot = s_d + 9 * K;                        // [kClMaxTgt] root of the target at each place
  int* const s_nk = s_troot + kClMaxTgt;

  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t base = (size_t)f * K;
  const unsigned nd = (unsigned)a.ND;
  int n = a.det_count[f];
  n = __builtin_amdgcn_readfirstlane(min(max(n, 0), K));

  for (int i = tid; i < n; i += nt) {
    s_r[i] = a.det_ridx[base + i];
    s_d[i] = a.det_didx[base + i];
    s_p[i] = a.det_power[base + i];
    s_lab[i] = i;
    s_cnt[i] = 0;
    s_pos[i] = 0;
    s_key[i] = 0ull;
  }
  if (tid < kClMaxTgt) s_troot[tid] = 0;
  if (tid == 0) *s_nk = 0;
  __syncthreads();

  // 1. candidate positions of the cells this thread owns
  int lo[kClOwn], hi[kClOwn];
#pragma unroll
  for (int k = 0; k < kClOwn; ++k) {
    const int i = tid + k * nt;
    lo[k] = hi[k] = 0;
    if (i < n) {
      const long long r = s_r[i];
      lo[k] = cl_bound(s_r, n, r - a.link_r, false);
      hi[k] = cl_bound(s_r, n, r + a.link_r, true);
    }
  }

  // 2. labels: at most n sweeps, each one monotone
  for (int it = 0; it < n; ++it) {
    int changed = 0;
#pragma unroll
    for (int k = 0; k < kClOwn; ++k) {
      const int i = tid + k * nt;
      if (i < n) {
        const int ri = s_r[i], di = s_d[i];
        const int m0 = s_lab[i];
        int m = m0;
        for (int j = lo[k]; j < hi[k]; ++j)
          if (cl_linked(ri, di, s_r[j], s_d[j], (unsigned)a.link_r, (unsigned)a.link_d, nd)) m = min(m, s_lab[j]);
        m = s_lab[m];
        if (m < m0) {
          s_lab[i] = m;
          changed = 1;
        }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }

  // 3. members and peak of every component, kept at its root
  for (int i = tid; i < n; i += nt) {
    const int L = s_lab[i];
    atomicAdd(&s_cnt[L], 1);
    const unsigned long long key =
        ((unsigned long long)__float_as_uint(s_p[i] + 0.f) << 32) | (unsigned long long)(unsigned)~i;
    atomicMax(&s_key[L], key);
  }
  __syncthreads();

  // 4. the kept roots, then the place of each by counting
  for (int i = tid; i < n; i += nt)
    if (s_lab[i] == i && s_cnt[i] >= a.min_cells) {
      const int e = atomicAdd(s_nk, 1);
      s_kept[e] = make_int2(i, (int)(unsigned)(s_key[i] >> 32));
    }
  __syncthreads();
  const int nk = __builtin_amdgcn_readfirstlane(*s_nk);
  for (int e = tid; e < nk; e += nt) {
    const int2 me = s_kept[e];
    int rank = 0;
    for (int e2 = 0; e2 < nk; ++e2) {
      const int2 o = s_kept[e2];
      rank += ((unsigned)o.y > (unsigned)me.y || (o.y == me.y && o.x < me.x)) ? 1 : 0;
    }
    s_pos[me.x] = rank + 1;
    if (rank < a.max_tgt) s_troot[rank] = me.x;
  }
  if (tid == 0) a.tgt_count[f] = nk;
  __syncthreads();

  if (a.det_label)
    for (int i = tid; i < K; i += nt) a.det_label[base + i] = i < n ? s_pos[s_lab[i]] : 0;

  // 5. the written targets: unused places are 0 in every array
  const int M = a.max_tgt;
  const int T = min(nk, M);
  const size_t obase = (size_t)f * M;
  for (int t = T + tid; t < M; t += nt) {
    if (a.cells) a.cells[obase + t] = 0;
    if (a.pk_ridx) a.pk_ridx[obase + t] = 0;
    if (a.pk_didx) a.pk_didx[obase + t] = 0;
    if (a.ext_r) a.ext_r[obase + t] = 0;
    if (a.ext_d) a.ext_d[obase + t] = 0;
    if (a.pk_power) a.pk_power[obase + t] = 0.f;
    if (a.pk_noise) a.pk_noise[obase + t] = 0.f;
    if (a.power) a.power[obase + t] = 0.f;
    if (a.range) a.range[obase + t] = 0.f;
    if (a.doppler) a.doppler[obase + t] = 0.f;
  }
  const int lane = tid & 63;
  for (int t = tid >> 6; t < T; t += nt >> 6) {
    const int root = __builtin_amdgcn_readfirstlane(s_troot[t]);
    const int pk = (int)~(unsigned)s_key[root];            // a member's position, so < n
    const int rpk = s_r[pk], dpk = s_d[pk];
    float sP = 0.f, sR = 0.f, sD = 0.f;
    int rmin = 0x7fffffff, rmax = (int)0x80000000, dmin = 0x7fffffff, dmax = (int)0x80000000;
    for (int b = root & ~63; b < n; b += 64) {
      const int j = b + lane;
      const bool mem = j < n && s_lab[j] == root;
      float p = 0.f;
      int rj = 0, dl = 0;
      if (mem) {
        p = s_p[j];
        rj = s_r[j];
        dl = (int)(((unsigned)s_d[j] - (unsigned)dpk + nd / 2) & (nd - 1)) - (int)(nd / 2);
      }
      unsigned long long mask = __ballot(mem);
      while (mask) {                                       // the members, in ascending position
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const float pp = __shfl(p, src);
        const int rr = __shfl(rj, src), dd = __shfl(dl, src);
        sP += pp;
        sR += pp * (float)(int)((unsigned)rr - (unsigned)rpk);
        sD += pp * (float)dd;
        rmin = min(rmin, rr);
        rmax = max(rmax, rr);
        dmin = min(dmin, dd);
        dmax = max(dmax, dd);
      }
    }
    if (lane == 0) {
      float rc = (float)rpk, dc = (float)dpk;
      if (sP > 0.f) {                                      // all powers 0: the centroid is the peak
        rc += sR / sP;
        dc += sD / sP;
      }
      if (dc < 0.5f) dc += (float)nd;                      // may round up to nd + 0.5: folded back below
      if (dc >= (float)nd + 0.5f) dc -= (float)nd;
      if (a.cells) a.cells[obase + t] = s_cnt[root];
      if (a.pk_ridx) a.pk_ridx[obase + t] = rpk;
      if (a.pk_didx) a.pk_didx[obase + t] = dpk;
      if (a.ext_r) a.ext_r[obase + t] = (int)((unsigned)rmax - (unsigned)rmin + 1u);
      if (a.ext_d) a.ext_d[obase + t] = dmax - dmin + 1;
      if (a.pk_power) a.pk_power[obase + t] = s_p[pk];
      if (a.pk_noise) a.pk_noise[obase + t] = a.det_noise ? a.det_noise[base + pk] : 0.f;
      if (a.power) a.power[obase + t] = sP;
      if (a.range) a.range[obase + t] = rc;
      if (a.doppler) a.doppler[obase + t] = dc;
    }
  }
}

}  // namespace

hipError_t launch_cluster(const ClusterArgs& a, hipStream_t s) {
  if (a.F <= 0) return hipSuccess;
  if (a.K < 1 || a.K > kClMaxDet || a.max_tgt < 1 || a.max_tgt > kClMaxTgt || a.F > 0x7fffffffLL || a.ND < 1 ||
      (a.ND & (a.ND - 1)) || a.link_r < 0 || a.link_d < 0)
    return hipErrorInvalidValue;
  const int threads = a.K <= 64 ? 64 : 256;               // kClOwn positions per thread cover max_det
  if (threads * kClOwn < a.K) return hipErrorInvalidValue;
  const size_t shmem = ((size_t)10 * a.K + kClMaxTgt + 1) * sizeof(int);   // 40.3 KiB at max_det 1024
  hipLaunchKernelGGL(k_cluster, dim3((unsigned)a.F), dim3(threads), shmem, s, a);
  return hipGetLastError();
}

}  // namespace fmcw
