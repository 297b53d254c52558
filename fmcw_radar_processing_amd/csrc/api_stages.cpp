// api_stages.cpp -- the RD-map stages of the libfmcw C-ABI (include/fmcw.h): 2-D CA-CFAR and OS-CFAR,
// Doppler-time / range-time signatures, clustering, angle of arrival, tracking, the MTI clutter
// filter, the combination of the receive channels' maps into beams and the range-angle maps.
// Every stage has a host-only fmcw_*_check, a device-pointer entry and a host-pointer entry that
// shards over the context's devices and walks its shard in chunks; the two entries share the
// stage's *_entry check.  The rules every stage states alike take the stage's message prefix.
#include "api_internal.h"

#include <cmath>
#include <cstring>

namespace {

int check_rd_shape(const std::string& stage, int32_t nr, int32_t nd) {   // nd: narrower than the frame pipeline's [2, 1024]
  if (nr < 16 || nr > 2048 || (nr & (nr - 1))) return fail(FMCW_E_ARG, stage + ": nr must be a power of two in [16, 2048]");
  if (nd < 4 || nd > 1024 || (nd & (nd - 1))) return fail(FMCW_E_ARG, stage + ": nd must be a power of two in [4, 1024]");
  return FMCW_OK;
}

int check_rd_dtype(int32_t dtype) {
  return dtype == FMCW_C64 || dtype == FMCW_C32H ? FMCW_OK : fail(FMCW_E_ARG, "bad rd_dtype");
}

// the range gate r_lo..r_hi, 1-based and inclusive; 0, 0 stands for all rows
int check_gate(const std::string& stage, int32_t r_lo, int32_t r_hi, int32_t nr) {
  if (r_lo > r_hi) return fail(FMCW_E_ARG, stage + ": r_lo > r_hi");
  if (!(r_lo == 0 && r_hi == 0) && (r_lo < 1 || r_hi > nr))
    return fail(FMCW_E_ARG, stage + ": the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)");
  return FMCW_OK;
}

// a checked gate as 0-based inclusive rows
void gate_rows(int32_t r_lo, int32_t r_hi, int32_t nr, int& g0, int& g1) {
  g0 = r_lo == 0 ? 0 : r_lo - 1;
  g1 = r_hi == 0 ? nr - 1 : r_hi - 1;
}

// S sequences of F frames each
int check_seq_sizes(const std::string& stage, int64_t S, int64_t F) {
  if (F < 0 || S < 0) return fail(FMCW_E_ARG, "S < 0 or F < 0");
  if (S > 0x7fffffffLL || F > ((int64_t)1 << 40) / std::max<int64_t>(S, 1))
    return fail(FMCW_E_ARG, stage + ": S must be below 2^31 and S * F at most 2^40");
  return FMCW_OK;
}

template <typename T> T* shifted(T* p, int64_t n) { return p ? p + n : nullptr; }   // NULL (optional) stays NULL

// t moved on by `rows` frames of M targets
fmcw_targets offset(const fmcw_targets& t, int64_t rows, int64_t M) {
  const int64_t n = rows * M;
  fmcw_targets o{};
  o.tgt_count = shifted(t.tgt_count, rows);
  o.cells = shifted(t.cells, n);
  o.peak_range_idx = shifted(t.peak_range_idx, n); o.peak_doppler_idx = shifted(t.peak_doppler_idx, n);
  o.extent_r = shifted(t.extent_r, n); o.extent_d = shifted(t.extent_d, n);
  o.peak_power = shifted(t.peak_power, n); o.peak_noise = shifted(t.peak_noise, n);
  o.power = shifted(t.power, n); o.range = shifted(t.range, n); o.doppler = shifted(t.doppler, n);
  return o;
}

// t moved on by `rows` frames of T tracks
fmcw_tracks offset(const fmcw_tracks& t, int64_t rows, int64_t T) {
  const int64_t n = rows * T;
  fmcw_tracks o{};
  o.trk_count = shifted(t.trk_count, rows);
  o.trk_id = shifted(t.trk_id, n); o.trk_status = shifted(t.trk_status, n);
  o.trk_age = shifted(t.trk_age, n); o.trk_misses = shifted(t.trk_misses, n);
  o.trk_range = shifted(t.trk_range, n); o.trk_range_rate = shifted(t.trk_range_rate, n);
  o.trk_doppler = shifted(t.trk_doppler, n); o.trk_power = shifted(t.trk_power, n);
  return o;
}

// Rows [f0, f0 + nf) of every one of S sequences, between a host array of F rows per sequence
// and a dense device array of nf rows per sequence: one copy, 2-D where the sequences' host
// rows do not follow each other.
int seq_rows(void* dev, void* host, int64_t S, int64_t F, int64_t f0, int64_t nf, size_t rowbytes, bool to_device,
             hipStream_t s) {
  void* const h = static_cast<char*>(host) + (size_t)f0 * rowbytes;
  void* const dst = to_device ? dev : h;
  const void* const src = to_device ? h : dev;
  const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  const size_t hp = (size_t)F * rowbytes, dp = (size_t)nf * rowbytes;   // bytes from one sequence to the next
  if (nf == F || S == 1) HIPCHK(hipMemcpyAsync(dst, src, (size_t)S * dp, kind, s));
  else HIPCHK(hipMemcpy2DAsync(dst, to_device ? dp : hp, src, to_device ? hp : dp, dp, (size_t)S, kind, s));
  return FMCW_OK;
}

// the device copy, at arena offset `off` of `base`, of an output the caller may have left out
template <typename T> T* dev_of(T* host, char* base, size_t off) {
  return host ? reinterpret_cast<T*>(base + off) : nullptr;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// 2-D CA-CFAR over the RD map (kernels_cfar.hip)
// ---------------------------------------------------------------------------
int fmcw_cfar_check(const fmcw_cfar_params* q, int32_t nr, int32_t nd, int32_t* n_train_full) {
  if (!q) return fail(FMCW_E_ARG, "cfar params is NULL");
  CHK(check_rd_shape("cfar", nr, nd));
  if (q->guard_r < 0 || q->guard_d < 0 || q->train_r < 0 || q->train_d < 0)
    return fail(FMCW_E_ARG, "cfar: guard and training half-widths must be >= 0");
  if (q->guard_r > 16 || q->guard_d > 16 || q->train_r > 16 || q->train_d > 16 || q->guard_r + q->train_r > 16 ||
      q->guard_d + q->train_d > 16)
    return fail(FMCW_E_ARG, "cfar: guard + train must be <= 16 in range (Wr) and in Doppler (Wd)");
  if (q->train_r + q->train_d < 1) return fail(FMCW_E_ARG, "cfar: train_r + train_d must be >= 1");
  const int Wr = q->guard_r + q->train_r, Wd = q->guard_d + q->train_d;
  if (2 * Wd + 1 > nd) return fail(FMCW_E_ARG, "cfar: the Doppler window 2 Wd + 1 exceeds nd");
  if (2 * Wr + 1 > nr) return fail(FMCW_E_ARG, "cfar: the range window 2 Wr + 1 exceeds nr");
  if (!(q->alpha > 0.f) || !std::isfinite(q->alpha)) return fail(FMCW_E_ARG, "cfar: alpha must be finite and > 0");
  CHK(check_gate("cfar", q->r_lo, q->r_hi, nr));
  if (q->max_det < 1 || q->max_det > 1024) return fail(FMCW_E_ARG, "cfar: max_det must be in [1, 1024]");
  if (q->flags & ~FMCW_CFAR_LOCAL_MAX) return fail(FMCW_E_ARG, "cfar: unknown flag bits");
  if (n_train_full) *n_train_full = (2 * Wr + 1) * (2 * Wd + 1) - (2 * q->guard_r + 1) * (2 * q->guard_d + 1);
  return FMCW_OK;
}

// what both CFAR entries check before they look at F == 0 and the pointers
static int cfar_entry(fmcw_ctx* c, const fmcw_cfar_params* q, int32_t rd_dtype, int64_t F, int32_t nr, int32_t nd) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_cfar_check(q, nr, nd, nullptr));
  CHK(check_rd_dtype(rd_dtype));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  return FMCW_OK;
}

int fmcw_cfar_alpha(int32_t n_train, double pfa, float* alpha) {
  if (!alpha) return fail(FMCW_E_ARG, "alpha is NULL");
  if (n_train < 1) return fail(FMCW_E_ARG, "cfar: n_train must be >= 1");
  if (!(pfa > 0.0 && pfa < 1.0)) return fail(FMCW_E_ARG, "cfar: pfa must be in (0, 1)");
  *alpha = (float)((double)n_train * std::expm1(-std::log(pfa) / (double)n_train));   // N (pfa^(-1/N) - 1)
  return FMCW_OK;
}

int fmcw_cfar_device(fmcw_ctx* c, const fmcw_cfar_params* q, const void* d_rd, int32_t rd_dtype, int64_t F, int32_t nr,
                     int32_t nd, int32_t* d_count, int32_t* d_ridx, int32_t* d_didx, float* d_power, float* d_noise,
                     uint8_t* d_mask, void* stream) {
  CHK(cfar_entry(c, q, rd_dtype, F, nr, nd));
  if (F == 0) return FMCW_OK;
  if (!d_rd || !d_count || !d_ridx || !d_didx || !d_power || !d_noise) return fail(FMCW_E_ARG, "required pointer is NULL");
  if (reinterpret_cast<uintptr_t>(d_rd) & 15) return fail(FMCW_E_ARG, "cfar: d_rd must be 16-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::CfarArgs a{};
  a.h = rd_dtype == FMCW_C32H;
  a.scale = a.h ? (float)nr * (float)nd : 1.f;
  a.NR = nr; a.ND = nd;
  a.gr = q->guard_r; a.gd = q->guard_d; a.tr = q->train_r; a.td = q->train_d;
  gate_rows(q->r_lo, q->r_hi, nr, a.g0, a.g1);
  a.K = q->max_det;
  a.local_max = (q->flags & FMCW_CFAR_LOCAL_MAX) ? 1 : 0;
  a.alpha = q->alpha;
  fmcw::cfar_plan(a, F);
  // frames per launch pair: at most 256 MiB of list scratch (the lists hold max_det entries per wave;
  // FMCW_CFAR_SCRATCH, in bytes, overrides, for tests of the launch seams)
  const size_t per = fmcw::cfar_scratch_per_frame(a);
  size_t budget = (size_t)256 << 20;
  if (const char* e = std::getenv("FMCW_CFAR_SCRATCH"); e && std::atoll(e) > 0) budget = (size_t)std::atoll(e);
  const int64_t Fc = std::max<int64_t>(1, std::min<int64_t>({F, (int64_t)(budget / per), (int64_t)32768}));
  const size_t nsub = (size_t)a.strips * a.tiles * a.waves;
  const size_t list_bytes = (size_t)Fc * nsub * a.K * sizeof(float4);
  int st = FMCW_OK;
  char* scr = static_cast<char*>(c->cfar_scr.get(s, list_bytes + (size_t)Fc * nsub * 4, &st));
  CHK(st);
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.F = std::min(Fc, F - f0);
    a.rd = static_cast<const char*>(d_rd) + (size_t)f0 * fin;
    a.sub_list = reinterpret_cast<float4*>(scr);
    a.sub_count = reinterpret_cast<int32_t*>(scr + list_bytes);
    a.det_count = d_count + f0;
    a.det_ridx = d_ridx + f0 * a.K;
    a.det_didx = d_didx + f0 * a.K;
    a.det_power = d_power + f0 * a.K;
    a.det_noise = d_noise + f0 * a.K;
    a.mask = d_mask ? d_mask + (size_t)f0 * nr * nd : nullptr;
    StageTimer tm(c, 10, s);
    HIPCHK(fmcw::launch_cfar(a, s));
    tm.done();
  }
  CHK(c->cfar_scr.done(s));
  return FMCW_OK;
}

// os: the OS-CFAR parameters whose window q is (fmcw_oscfar), or nullptr for CA-CFAR
static int cfar_host_one(fmcw_ctx* c, const fmcw_cfar_params* q, const fmcw_oscfar_params* os, const char* rd,
                         int32_t dtype, int64_t F, int32_t nr, int32_t nd, int32_t* count, int32_t* ridx, int32_t* didx,
                         float* power, float* noise, uint8_t* mask) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const int K = q->max_det;
  const size_t fin = (size_t)nr * nd * esize(dtype), fmask = (size_t)nr * nd;
  const int64_t Fc = host_chunk(fin, F);
  // the shard's lists in the context's cf_out
  void* const host[5] = {count, ridx, didx, power, noise};
  Arena ar;
  size_t oo[5], obytes[5];
  for (int i = 0; i < 5; ++i) oo[i] = ar.add(obytes[i] = (size_t)F * 4 * (i == 0 ? 1 : K));
  CHK(c->cf_out.ensure(ar.off));
  CHK(c->cf_in.ensure((size_t)Fc * fin));
  if (mask) CHK(c->cf_mask.ensure((size_t)Fc * fmask));
  char* const o = c->cf_out.as<char>();
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    HIPCHK(hipMemcpyAsync(c->cf_in.p, rd + (size_t)f0 * fin, (size_t)nf * fin, hipMemcpyHostToDevice, s));
    int32_t* const dc = reinterpret_cast<int32_t*>(o + oo[0]) + f0;
    int32_t* const dri = reinterpret_cast<int32_t*>(o + oo[1]) + f0 * K;
    int32_t* const ddi = reinterpret_cast<int32_t*>(o + oo[2]) + f0 * K;
    float* const dpw = reinterpret_cast<float*>(o + oo[3]) + f0 * K;
    float* const dnz = reinterpret_cast<float*>(o + oo[4]) + f0 * K;
    uint8_t* const dm = mask ? c->cf_mask.as<uint8_t>() : nullptr;
    if (os) CHK(fmcw_oscfar_device(c, os, c->cf_in.p, dtype, nf, nr, nd, dc, dri, ddi, dpw, dnz, dm, s));
    else CHK(fmcw_cfar_device(c, q, c->cf_in.p, dtype, nf, nr, nd, dc, dri, ddi, dpw, dnz, dm, s));
    if (mask) HIPCHK(hipMemcpyAsync(mask + (size_t)f0 * fmask, c->cf_mask.p, (size_t)nf * fmask, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  for (int i = 0; i < 5; ++i) HIPCHK(hipMemcpyAsync(host[i], o + oo[i], obytes[i], hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_cfar(fmcw_ctx* c, const fmcw_cfar_params* q, const void* rd, int32_t rd_dtype, int64_t F, int32_t nr, int32_t nd,
              int32_t* count, int32_t* ridx, int32_t* didx, float* power, float* noise, uint8_t* mask) {
  CHK(cfar_entry(c, q, rd_dtype, F, nr, nd));
  if (F == 0) return FMCW_OK;
  if (!rd || !count || !ridx || !didx || !power || !noise) return fail(FMCW_E_ARG, "required pointer is NULL");
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  const int K = q->max_det;
  // frames are independent: contiguous shards, each written in place
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    return cfar_host_one(d, q, nullptr, static_cast<const char*>(rd) + (size_t)f0 * fin, rd_dtype, n, nr, nd, count + f0,
                         ridx + f0 * K, didx + f0 * K, power + f0 * K, noise + f0 * K, shifted(mask, f0 * nr * nd));
  });
}

// ---------------------------------------------------------------------------
// 2-D OS-CFAR over the RD map (kernels_oscfar.hip)
// ---------------------------------------------------------------------------
int fmcw_oscfar_check(const fmcw_oscfar_params* q, int32_t nr, int32_t nd, int32_t* n_train_full) {
  if (!q) return fail(FMCW_E_ARG, "oscfar params is NULL");
  int32_t n = 0;
  CHK(fmcw_cfar_check(&q->win, nr, nd, &n));
  if (q->rank < 1 || q->rank > n)
    return fail(FMCW_E_ARG, "oscfar: rank must be in [1, " + std::to_string(n) + "], the full window's training cells");
  if (n_train_full) *n_train_full = n;
  return FMCW_OK;
}

// what both OS-CFAR entries check before they look at F == 0 and the pointers
static int oscfar_entry(fmcw_ctx* c, const fmcw_oscfar_params* q, int32_t rd_dtype, int64_t F, int32_t nr, int32_t nd,
                        int32_t* n_train_full) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_oscfar_check(q, nr, nd, n_train_full));
  CHK(check_rd_dtype(rd_dtype));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  return FMCW_OK;
}

int fmcw_oscfar_alpha(int32_t n_train, int32_t rank, double pfa, float* alpha) {
  if (!alpha) return fail(FMCW_E_ARG, "alpha is NULL");
  if (n_train < 1) return fail(FMCW_E_ARG, "oscfar: n_train must be >= 1");
  if (rank < 1 || rank > n_train) return fail(FMCW_E_ARG, "oscfar: rank must be in [1, n_train]");
  if (!(pfa > 0.0 && pfa < 1.0)) return fail(FMCW_E_ARG, "oscfar: pfa must be in (0, 1)");
  // -ln Pfa(alpha) = sum_{i < k} log1p(alpha / (N - i)) rises with alpha: bracket, then bisect
  const double want = -std::log(pfa);
  auto g = [&](double a) {
    double s = 0.0;
    for (int i = 0; i < rank; ++i) s += std::log1p(a / (double)(n_train - i));
    return s;
  };
  double lo = 0.0, hi = 1.0;
  while (g(hi) < want) {
    lo = hi;
    hi *= 2.0;
  }
  for (int it = 0; it < 200 && hi - lo > 0.0; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;
    if (g(mid) < want) lo = mid;
    else hi = mid;
  }
  *alpha = (float)(0.5 * (lo + hi));
  return FMCW_OK;
}

int fmcw_oscfar_device(fmcw_ctx* c, const fmcw_oscfar_params* q, const void* d_rd, int32_t rd_dtype, int64_t F,
                       int32_t nr, int32_t nd, int32_t* d_count, int32_t* d_ridx, int32_t* d_didx, float* d_power,
                       float* d_noise, uint8_t* d_mask, void* stream) {
  int32_t nfull = 0;
  CHK(oscfar_entry(c, q, rd_dtype, F, nr, nd, &nfull));
  if (F == 0) return FMCW_OK;
  if (!d_rd || !d_count || !d_ridx || !d_didx || !d_power || !d_noise) return fail(FMCW_E_ARG, "required pointer is NULL");
  if (reinterpret_cast<uintptr_t>(d_rd) & 15) return fail(FMCW_E_ARG, "oscfar: d_rd must be 16-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::OsCfarArgs o{};
  fmcw::CfarArgs& a = o.c;
  o.rank = q->rank;
  o.nfull = nfull;
  a.h = rd_dtype == FMCW_C32H;
  a.scale = a.h ? (float)nr * (float)nd : 1.f;
  a.NR = nr; a.ND = nd;
  a.gr = q->win.guard_r; a.gd = q->win.guard_d; a.tr = q->win.train_r; a.td = q->win.train_d;
  gate_rows(q->win.r_lo, q->win.r_hi, nr, a.g0, a.g1);
  a.K = q->win.max_det;
  a.local_max = (q->win.flags & FMCW_CFAR_LOCAL_MAX) ? 1 : 0;
  a.alpha = q->win.alpha;
  fmcw::cfar_plan(a, F);
  // frames per launch group: CA-CFAR's list scratch, budget and override (fmcw_cfar_device)
  const size_t per = fmcw::cfar_scratch_per_frame(a);
  size_t budget = (size_t)256 << 20;
  if (const char* e = std::getenv("FMCW_CFAR_SCRATCH"); e && std::atoll(e) > 0) budget = (size_t)std::atoll(e);
  const int64_t Fc = std::max<int64_t>(1, std::min<int64_t>({F, (int64_t)(budget / per), (int64_t)32768}));
  const size_t nsub = (size_t)a.strips * a.tiles * a.waves;
  const size_t list_bytes = (size_t)Fc * nsub * a.K * sizeof(float4);
  int st = FMCW_OK;
  char* scr = static_cast<char*>(c->cfar_scr.get(s, list_bytes + (size_t)Fc * nsub * 4, &st));
  CHK(st);
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.F = std::min(Fc, F - f0);
    a.rd = static_cast<const char*>(d_rd) + (size_t)f0 * fin;
    a.sub_list = reinterpret_cast<float4*>(scr);
    a.sub_count = reinterpret_cast<int32_t*>(scr + list_bytes);
    a.det_count = d_count + f0;
    a.det_ridx = d_ridx + f0 * a.K;
    a.det_didx = d_didx + f0 * a.K;
    a.det_power = d_power + f0 * a.K;
    a.det_noise = d_noise + f0 * a.K;
    a.mask = d_mask ? d_mask + (size_t)f0 * nr * nd : nullptr;
    StageTimer tm(c, 16, s);
    HIPCHK(fmcw::launch_oscfar(o, s));
    tm.done();
  }
  CHK(c->cfar_scr.done(s));
  return FMCW_OK;
}

int fmcw_oscfar(fmcw_ctx* c, const fmcw_oscfar_params* q, const void* rd, int32_t rd_dtype, int64_t F, int32_t nr,
                int32_t nd, int32_t* count, int32_t* ridx, int32_t* didx, float* power, float* noise, uint8_t* mask) {
  CHK(oscfar_entry(c, q, rd_dtype, F, nr, nd, nullptr));
  if (F == 0) return FMCW_OK;
  if (!rd || !count || !ridx || !didx || !power || !noise) return fail(FMCW_E_ARG, "required pointer is NULL");
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  const int K = q->win.max_det;
  // frames are independent: contiguous shards, each written in place
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    return cfar_host_one(d, &q->win, q, static_cast<const char*>(rd) + (size_t)f0 * fin, rd_dtype, n, nr, nd, count + f0,
                         ridx + f0 * K, didx + f0 * K, power + f0 * K, noise + f0 * K, shifted(mask, f0 * nr * nd));
  });
}

// ---------------------------------------------------------------------------
// Doppler-time and range-time signatures of the RD map (kernels_sig.hip)
// ---------------------------------------------------------------------------
int fmcw_sig_check(const fmcw_sig_params* q, int32_t nr, int32_t nd) {
  if (!q) return fail(FMCW_E_ARG, "sig params is NULL");
  CHK(check_rd_shape("sig", nr, nd));
  CHK(check_gate("sig", q->r_lo, q->r_hi, nr));
  if (q->track_half < 0 || q->track_half > 64) return fail(FMCW_E_ARG, "sig: track_half must be in [0, 64]");
  if (q->dc_half < -1) return fail(FMCW_E_ARG, "sig: dc_half must be >= -1 (-1 leaves no Doppler bin out)");
  if (2 * (int64_t)q->dc_half + 1 >= nd) return fail(FMCW_E_ARG, "sig: 2 dc_half + 1 must be < nd");
  if (q->flags & ~FMCW_SIG_DB) return fail(FMCW_E_ARG, "sig: unknown flag bits");
  if (!(q->floor_db < 0.f) || !std::isfinite(q->floor_db)) return fail(FMCW_E_ARG, "sig: floor_db must be finite and < 0");
  return FMCW_OK;
}

// what both signature entries check before they look at F == 0 and the RD pointer
static int sig_entry(fmcw_ctx* c, const fmcw_sig_params* q, int32_t rd_dtype, int64_t F, int32_t nr, int32_t nd,
                     const int32_t* center, int32_t center_stride, const float* doppler_time, const float* range_time) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_sig_check(q, nr, nd));
  CHK(check_rd_dtype(rd_dtype));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (!doppler_time && !range_time) return fail(FMCW_E_ARG, "sig: both maps are NULL");
  if (center && center_stride < 1) return fail(FMCW_E_ARG, "sig: center_stride must be >= 1");
  return FMCW_OK;
}

int fmcw_sig_device(fmcw_ctx* c, const fmcw_sig_params* q, const void* d_rd, int32_t rd_dtype, int64_t F, int32_t nr,
                    int32_t nd, const int32_t* d_center, int32_t center_stride, float* d_doppler_time,
                    float* d_range_time, float* d_dt_max, float* d_rt_max, void* stream) {
  CHK(sig_entry(c, q, rd_dtype, F, nr, nd, d_center, center_stride, d_doppler_time, d_range_time));
  if (F == 0) return FMCW_OK;
  if (!d_rd) return fail(FMCW_E_ARG, "required pointer is NULL");
  if (reinterpret_cast<uintptr_t>(d_rd) & 15) return fail(FMCW_E_ARG, "sig: d_rd must be 16-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::SigArgs a{};
  a.h = rd_dtype == FMCW_C32H;
  a.scale2 = a.h ? ((float)nr * (float)nd) * ((float)nr * (float)nd) : 1.f;
  a.NR = nr; a.ND = nd;
  gate_rows(q->r_lo, q->r_hi, nr, a.g0, a.g1);
  a.th = q->track_half;
  a.dc = q->dc_half;
  a.center = d_center;
  a.cstride = d_center ? center_stride : 0;
  a.dt = d_doppler_time; a.rt = d_range_time;
  a.dt_max = d_doppler_time ? d_dt_max : nullptr;
  a.rt_max = d_range_time ? d_rt_max : nullptr;
  fmcw::sig_plan(a);
  // frames per launch: at most 256 MiB of column-sum scratch (the results do not depend on the cut)
  const size_t per = fmcw::sig_scratch_per_frame(a);
  const int64_t Fc = std::max<int64_t>(1, std::min<int64_t>({F, per ? (int64_t)(((size_t)256 << 20) / per) : F,
                                                             (int64_t)0x7fffffff / 256}));
  if (per) {
    int st = FMCW_OK;
    a.part = static_cast<float*>(c->sig_scr.get(s, (size_t)Fc * per, &st));
    CHK(st);
  }
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.F = std::min(Fc, F - f0);
    a.rd = static_cast<const char*>(d_rd) + (size_t)f0 * fin;
    a.center = shifted(d_center, f0 * center_stride);
    a.dt = shifted(d_doppler_time, f0 * nd);
    a.rt = shifted(d_range_time, f0 * nr);
    HIPCHK(fmcw::launch_sig(a, s));
  }
  if (per) CHK(c->sig_scr.done(s));
  return FMCW_OK;
}

int fmcw_sig_db_device(fmcw_ctx* c, const float* d_map, int64_t n, const float* d_max, float floor_db, float* d_out,
                       void* stream) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (n < 0) return fail(FMCW_E_ARG, "n < 0");
  if (!(floor_db < 0.f) || !std::isfinite(floor_db)) return fail(FMCW_E_ARG, "sig: floor_db must be finite and < 0");
  if (n == 0) return FMCW_OK;
  if (!d_map || !d_max || !d_out) return fail(FMCW_E_ARG, "required pointer is NULL");
  CHK(set_device(c));
  HIPCHK(fmcw::launch_sig_db(d_map, n, d_max, floor_db, d_out, pick(c, stream)));
  return FMCW_OK;
}

// byte offsets of one shard's maps and two maxima in the context's sg_out: [F][nd], [F][nr], 2 floats
namespace {
struct SigOut {
  size_t o_dt, o_rt, o_max, bytes;
  SigOut(int64_t F, int nr, int nd) {
    Arena ar;
    o_dt = ar.add((size_t)F * nd * 4);
    o_rt = ar.add((size_t)F * nr * 4);
    o_max = ar.add(8);
    bytes = ar.off;
  }
};
}  // namespace

// One shard of fmcw_sig: both maps and both maxima of frames [0, F) into sg_out, chunk by chunk.
// The maps stay there for sig_host_finish.
static int sig_host_one(fmcw_ctx* c, const fmcw_sig_params* q, const char* rd, int32_t dtype, int64_t F, int32_t nr,
                        int32_t nd, const int32_t* center, int32_t cstride, float* mx) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const size_t fin = (size_t)nr * nd * esize(dtype);
  const int64_t Fc = host_chunk(fin, F);
  const SigOut so(F, nr, nd);
  CHK(c->sg_out.ensure(so.bytes));
  CHK(c->sg_in.ensure((size_t)Fc * fin));
  char* const o = c->sg_out.as<char>();
  float* const d_mx = reinterpret_cast<float*>(o + so.o_max);
  HIPCHK(hipMemsetAsync(d_mx, 0, 8, s));
  if (center) {
    CHK(c->sg_ctr.ensure((size_t)F * cstride * 4));
    HIPCHK(hipMemcpyAsync(c->sg_ctr.p, center, (size_t)F * cstride * 4, hipMemcpyHostToDevice, s));
  }
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    HIPCHK(hipMemcpyAsync(c->sg_in.p, rd + (size_t)f0 * fin, (size_t)nf * fin, hipMemcpyHostToDevice, s));
    CHK(fmcw_sig_device(c, q, c->sg_in.p, dtype, nf, nr, nd, center ? c->sg_ctr.as<int32_t>() + f0 * cstride : nullptr,
                        cstride, reinterpret_cast<float*>(o + so.o_dt) + f0 * nd,
                        reinterpret_cast<float*>(o + so.o_rt) + f0 * nr, d_mx, d_mx + 1, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffer is reused by the next chunk
  }
  HIPCHK(hipMemcpyAsync(mx, d_mx, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

// The shard's maps to the host, in dB relative to the global maxima gmx when db.
static int sig_host_finish(fmcw_ctx* c, int64_t F, int32_t nr, int32_t nd, bool db, const float* gmx, float floor_db,
                           float* dt, float* rt) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const SigOut so(F, nr, nd);
  char* const o = c->sg_out.as<char>();
  float* const d_dt = reinterpret_cast<float*>(o + so.o_dt);
  float* const d_rt = reinterpret_cast<float*>(o + so.o_rt);
  float* const d_mx = reinterpret_cast<float*>(o + so.o_max);
  if (db) {
    HIPCHK(hipMemcpyAsync(d_mx, gmx, 8, hipMemcpyHostToDevice, s));
    if (dt) CHK(fmcw_sig_db_device(c, d_dt, F * nd, d_mx, floor_db, d_dt, s));
    if (rt) CHK(fmcw_sig_db_device(c, d_rt, F * nr, d_mx + 1, floor_db, d_rt, s));
  }
  if (dt) HIPCHK(hipMemcpyAsync(dt, d_dt, (size_t)F * nd * 4, hipMemcpyDeviceToHost, s));
  if (rt) HIPCHK(hipMemcpyAsync(rt, d_rt, (size_t)F * nr * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_sig(fmcw_ctx* c, const fmcw_sig_params* q, const void* rd, int32_t rd_dtype, int64_t F, int32_t nr, int32_t nd,
             const int32_t* center, int32_t center_stride, float* doppler_time, float* range_time, float* dt_max,
             float* rt_max) {
  CHK(sig_entry(c, q, rd_dtype, F, nr, nd, center, center_stride, doppler_time, range_time));
  if (F == 0) {
    if (dt_max) *dt_max = 0.f;
    if (rt_max) *rt_max = 0.f;
    return FMCW_OK;
  }
  if (!rd) return fail(FMCW_E_ARG, "required pointer is NULL");
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  const int world = 1 + (int)c->peers.size();
  std::vector<float> mx(2 * (size_t)world, 0.f);
  // frames are independent: contiguous shards; every shard forms both maps on its device
  CHK(over_devices(c, F, [&](fmcw_ctx* d, int g, int64_t f0, int64_t n) {
    return sig_host_one(d, q, static_cast<const char*>(rd) + (size_t)f0 * fin, rd_dtype, n, nr, nd,
                        shifted(center, f0 * center_stride), center_stride, &mx[2 * (size_t)g]);
  }));
  float gmx[2] = {0.f, 0.f};                   // a maximum of non-negative floats does not depend on order
  for (int g = 0; g < world; ++g) {
    gmx[0] = std::max(gmx[0], mx[2 * (size_t)g]);
    gmx[1] = std::max(gmx[1], mx[2 * (size_t)g + 1]);
  }
  if (dt_max) *dt_max = gmx[0];
  if (rt_max) *rt_max = gmx[1];
  // second pass, after the maxima are combined (:282-283): dB relative to the global maximum, then home
  const bool db = (q->flags & FMCW_SIG_DB) != 0;
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    return sig_host_finish(d, n, nr, nd, db, gmx, q->floor_db, shifted(doppler_time, f0 * nd), shifted(range_time, f0 * nr));
  });
}

// ---------------------------------------------------------------------------
// Targets from the CFAR detection lists (kernels_cluster.hip)
// ---------------------------------------------------------------------------
int fmcw_cluster_check(const fmcw_cluster_params* q, int32_t nr, int32_t nd, int32_t max_det) {
  if (!q) return fail(FMCW_E_ARG, "cluster params is NULL");
  CHK(check_rd_shape("cluster", nr, nd));
  if (q->link_r < 0 || q->link_r > 8 || q->link_d < 0 || q->link_d > 8)
    return fail(FMCW_E_ARG, "cluster: link_r and link_d must be in [0, 8]");
  if (2 * q->link_d + 1 > nd) return fail(FMCW_E_ARG, "cluster: the Doppler link 2 link_d + 1 exceeds nd");
  if (q->min_cells < 1 || q->min_cells > 1024) return fail(FMCW_E_ARG, "cluster: min_cells must be in [1, 1024]");
  if (q->max_tgt < 1 || q->max_tgt > 64) return fail(FMCW_E_ARG, "cluster: max_tgt must be in [1, 64]");
  if (max_det < 1 || max_det > 1024) return fail(FMCW_E_ARG, "cluster: max_det must be in [1, 1024]");
  if (q->flags != 0) return fail(FMCW_E_ARG, "cluster: unknown flag bits");
  return FMCW_OK;
}

// what both clustering entries check before they look at F == 0 and the pointers
static int cluster_entry(fmcw_ctx* c, const fmcw_cluster_params* q, int64_t F, int32_t nr, int32_t nd, int32_t max_det) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_cluster_check(q, nr, nd, max_det));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  return FMCW_OK;
}

int fmcw_cluster_device(fmcw_ctx* c, const fmcw_cluster_params* q, int64_t F, int32_t nr, int32_t nd, int32_t max_det,
                        const int32_t* d_count, const int32_t* d_ridx, const int32_t* d_didx, const float* d_power,
                        const float* d_noise, const fmcw_targets* d_out, int32_t* d_label, void* stream) {
  CHK(cluster_entry(c, q, F, nr, nd, max_det));
  if (F == 0) return FMCW_OK;
  if (!d_count || !d_ridx || !d_didx || !d_power || !d_out || !d_out->tgt_count)
    return fail(FMCW_E_ARG, "required pointer is NULL");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::ClusterArgs a{};
  a.ND = nd;
  a.K = max_det;
  a.link_r = q->link_r; a.link_d = q->link_d; a.min_cells = q->min_cells; a.max_tgt = q->max_tgt;
  const int64_t K = max_det, M = q->max_tgt;
  // one workgroup per frame: at most 2^20 frames per launch (the results do not depend on the cut)
  const int64_t Fc = (int64_t)1 << 20;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.F = std::min(Fc, F - f0);
    a.det_count = d_count + f0;
    a.det_ridx = d_ridx + f0 * K;
    a.det_didx = d_didx + f0 * K;
    a.det_power = d_power + f0 * K;
    a.det_noise = shifted(d_noise, f0 * K);
    const fmcw_targets t = offset(*d_out, f0, M);
    a.tgt_count = t.tgt_count; a.cells = t.cells;
    a.pk_ridx = t.peak_range_idx; a.pk_didx = t.peak_doppler_idx; a.ext_r = t.extent_r; a.ext_d = t.extent_d;
    a.pk_power = t.peak_power; a.pk_noise = t.peak_noise; a.power = t.power; a.range = t.range; a.doppler = t.doppler;
    a.det_label = shifted(d_label, f0 * K);
    StageTimer tm(c, 11, s);
    HIPCHK(fmcw::launch_cluster(a, s));
    tm.done();
  }
  return FMCW_OK;
}

static int cluster_host_one(fmcw_ctx* c, const fmcw_cluster_params* q, int64_t F, int32_t nr, int32_t nd, int32_t K,
                            const int32_t* count, const int32_t* ridx, const int32_t* didx, const float* power,
                            const float* noise, const fmcw_targets& out, int32_t* label) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const int M = q->max_tgt;
  const size_t flist = (size_t)K * 4;
  const int64_t Fc = host_chunk(4 + 4 * flist, F);
  // the shard's outputs in the context's cl_out: the fmcw_targets members in declaration order, then det_label
  void* const host[12] = {out.tgt_count, out.cells, out.peak_range_idx, out.peak_doppler_idx, out.extent_r, out.extent_d,
                          out.peak_power, out.peak_noise, out.power, out.range, out.doppler, label};
  Arena in, ou;
  size_t oo[12], obytes[12];
  for (int i = 0; i < 12; ++i) oo[i] = ou.add(obytes[i] = (size_t)F * 4 * (i == 0 ? 1 : i == 11 ? K : M));
  const size_t i_count = in.add((size_t)Fc * 4), i_ridx = in.add((size_t)Fc * flist), i_didx = in.add((size_t)Fc * flist),
               i_pow = in.add((size_t)Fc * flist), i_noise = in.add((size_t)Fc * flist);
  CHK(c->cl_out.ensure(ou.off));
  CHK(c->cl_in.ensure(in.off));
  char* const o = c->cl_out.as<char>();
  char* const di = c->cl_in.as<char>();
  const fmcw_targets dev{dev_of(out.tgt_count, o, oo[0]), dev_of(out.cells, o, oo[1]), dev_of(out.peak_range_idx, o, oo[2]),
                         dev_of(out.peak_doppler_idx, o, oo[3]), dev_of(out.extent_r, o, oo[4]),
                         dev_of(out.extent_d, o, oo[5]), dev_of(out.peak_power, o, oo[6]), dev_of(out.peak_noise, o, oo[7]),
                         dev_of(out.power, o, oo[8]), dev_of(out.range, o, oo[9]), dev_of(out.doppler, o, oo[10])};
  int32_t* const dev_label = dev_of(label, o, oo[11]);
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    HIPCHK(hipMemcpyAsync(di + i_count, count + f0, (size_t)nf * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(di + i_ridx, ridx + f0 * K, (size_t)nf * flist, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(di + i_didx, didx + f0 * K, (size_t)nf * flist, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(di + i_pow, power + f0 * K, (size_t)nf * flist, hipMemcpyHostToDevice, s));
    if (noise) HIPCHK(hipMemcpyAsync(di + i_noise, noise + f0 * K, (size_t)nf * flist, hipMemcpyHostToDevice, s));
    const fmcw_targets d = offset(dev, f0, M);
    CHK(fmcw_cluster_device(c, q, nf, nr, nd, K, reinterpret_cast<int32_t*>(di + i_count),
                            reinterpret_cast<int32_t*>(di + i_ridx), reinterpret_cast<int32_t*>(di + i_didx),
                            reinterpret_cast<float*>(di + i_pow), noise ? reinterpret_cast<float*>(di + i_noise) : nullptr,
                            &d, shifted(dev_label, f0 * K), s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  for (int i = 0; i < 12; ++i)
    if (host[i]) HIPCHK(hipMemcpyAsync(host[i], o + oo[i], obytes[i], hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_cluster(fmcw_ctx* c, const fmcw_cluster_params* q, int64_t F, int32_t nr, int32_t nd, int32_t max_det,
                 const int32_t* count, const int32_t* ridx, const int32_t* didx, const float* power, const float* noise,
                 const fmcw_targets* out, int32_t* label) {
  CHK(cluster_entry(c, q, F, nr, nd, max_det));
  if (F == 0) return FMCW_OK;
  if (!count || !ridx || !didx || !power || !out || !out->tgt_count) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int64_t K = max_det, M = q->max_tgt;
  // frames are independent: contiguous shards, each written in place
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    return cluster_host_one(d, q, n, nr, nd, max_det, count + f0, ridx + f0 * K, didx + f0 * K, power + f0 * K,
                            shifted(noise, f0 * K), offset(*out, f0, M), shifted(label, f0 * K));
  });
}

// ---------------------------------------------------------------------------
// Angle of arrival from several receive channels of the RD map (kernels_aoa.hip)
// ---------------------------------------------------------------------------
int fmcw_aoa_check(const fmcw_aoa_params* q, int32_t nr, int32_t nd, int32_t max_det) {
  if (!q) return fail(FMCW_E_ARG, "aoa params is NULL");
  CHK(check_rd_shape("aoa", nr, nd));
  if (q->n_chan < 2 || q->n_chan > fmcw::kAoaChan) return fail(FMCW_E_ARG, "aoa: n_chan must be in [2, 8]");
  if (q->max_tgt < 0 || q->max_tgt > 64) return fail(FMCW_E_ARG, "aoa: max_tgt must be 0 or in [1, 64]");
  if (max_det < 1 || max_det > 1024) return fail(FMCW_E_ARG, "aoa: max_det must be in [1, 1024]");
  if (q->flags != 0) return fail(FMCW_E_ARG, "aoa: unknown flag bits");
  if (!std::isfinite(q->spacing) || !(std::fabs(q->spacing) >= 0.01f && std::fabs(q->spacing) <= 16.f))
    return fail(FMCW_E_ARG, "aoa: spacing must be finite with 0.01 <= |spacing| <= 16");
  for (int i = 0; i < 2 * q->n_chan; ++i)
    if (!std::isfinite(q->w[i])) return fail(FMCW_E_ARG, "aoa: the weights must be finite");
  return FMCW_OK;
}

}  // extern "C"

namespace {

constexpr int kAoaDet = 4, kAoaOut = 12;   // fmcw_angles: the first kAoaDet members are per cell, the rest per target

// the members of an fmcw_angles in declaration order
void aoa_members(const fmcw_angles& t, void* (&m)[kAoaOut]) {
  void* const v[kAoaOut] = {t.det_zre, t.det_zim, t.det_phase, t.det_sin, t.tgt_zre, t.tgt_zim,
                            t.tgt_e0,  t.tgt_e1,  t.tgt_phase, t.tgt_sin, t.tgt_coh, t.tgt_cells};
  for (int i = 0; i < kAoaOut; ++i) m[i] = v[i];
}

// t moved on by `rows` frames of K cells and M targets
fmcw_angles offset(const fmcw_angles& t, int64_t rows, int64_t K, int64_t M) {
  const int64_t k = rows * K, m = rows * M;
  fmcw_angles o{};
  o.det_zre = shifted(t.det_zre, k); o.det_zim = shifted(t.det_zim, k);
  o.det_phase = shifted(t.det_phase, k); o.det_sin = shifted(t.det_sin, k);
  o.tgt_zre = shifted(t.tgt_zre, m); o.tgt_zim = shifted(t.tgt_zim, m);
  o.tgt_e0 = shifted(t.tgt_e0, m); o.tgt_e1 = shifted(t.tgt_e1, m);
  o.tgt_phase = shifted(t.tgt_phase, m); o.tgt_sin = shifted(t.tgt_sin, m);
  o.tgt_coh = shifted(t.tgt_coh, m); o.tgt_cells = shifted(t.tgt_cells, m);
  return o;
}

// what both angle entries check before they look at F == 0 and the input pointers
int aoa_entry(fmcw_ctx* c, const fmcw_aoa_params* q, int32_t rd_dtype, int64_t F, int32_t nr, int32_t nd, int32_t max_det,
              const int32_t* label, const fmcw_angles* out) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_aoa_check(q, nr, nd, max_det));
  CHK(check_rd_dtype(rd_dtype));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (!out) return fail(FMCW_E_ARG, "aoa: the output struct is NULL");
  void* m[kAoaOut];
  aoa_members(*out, m);
  bool any = false, tgt = false;
  for (int i = 0; i < kAoaOut; ++i) {
    any = any || m[i];
    tgt = tgt || (i >= kAoaDet && m[i]);
  }
  if (!any) return fail(FMCW_E_ARG, "aoa: every output is NULL");
  if (tgt && !label) return fail(FMCW_E_ARG, "aoa: a per-target output needs det_label");
  if (tgt && q->max_tgt == 0) return fail(FMCW_E_ARG, "aoa: a per-target output needs max_tgt >= 1");
  return FMCW_OK;
}

}  // namespace

extern "C" {

int fmcw_aoa_device(fmcw_ctx* c, const fmcw_aoa_params* q, const void* const* d_rd_ch, int32_t rd_dtype, int64_t F,
                    int32_t nr, int32_t nd, int32_t max_det, const int32_t* d_count, const int32_t* d_ridx,
                    const int32_t* d_didx, const int32_t* d_label, const fmcw_angles* d_out, void* stream) {
  CHK(aoa_entry(c, q, rd_dtype, F, nr, nd, max_det, d_label, d_out));
  if (F == 0) return FMCW_OK;
  if (!d_rd_ch || !d_count || !d_ridx || !d_didx) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int A = q->n_chan;
  for (int ch = 0; ch < A; ++ch) {
    if (!d_rd_ch[ch]) return fail(FMCW_E_ARG, "required pointer is NULL");
    if (reinterpret_cast<uintptr_t>(d_rd_ch[ch]) & 15) return fail(FMCW_E_ARG, "aoa: every channel's d_rd must be 16-byte aligned");
  }
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::AoaArgs a{};
  a.NR = nr; a.ND = nd;
  a.K = max_det;
  a.A = A;
  a.M = q->max_tgt;
  a.h = rd_dtype == FMCW_C32H;
  a.scale2 = a.h ? ((float)nr * (float)nd) * ((float)nr * (float)nd) : 1.f;
  a.kinv = (float)(1.0 / (2.0 * 3.14159265358979323846 * (double)q->spacing));
  for (int i = 0; i < 2 * A; ++i) a.w[i] = q->w[i];
  a.tgt_any = d_out->tgt_zre || d_out->tgt_zim || d_out->tgt_e0 || d_out->tgt_e1 || d_out->tgt_phase ||
              d_out->tgt_sin || d_out->tgt_coh || d_out->tgt_cells;
  const int64_t K = max_det, M = q->max_tgt;
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  // one workgroup per frame: at most 2^20 frames per launch (the results do not depend on the cut)
  const int64_t Fc = (int64_t)1 << 20;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.F = std::min(Fc, F - f0);
    for (int ch = 0; ch < A; ++ch) a.rd[ch] = static_cast<const char*>(d_rd_ch[ch]) + (size_t)f0 * fin;
    a.det_count = d_count + f0;
    a.det_ridx = d_ridx + f0 * K;
    a.det_didx = d_didx + f0 * K;
    a.det_label = shifted(d_label, f0 * K);
    const fmcw_angles t = offset(*d_out, f0, K, M);
    a.det_zre = t.det_zre; a.det_zim = t.det_zim; a.det_phase = t.det_phase; a.det_sin = t.det_sin;
    a.tgt_zre = t.tgt_zre; a.tgt_zim = t.tgt_zim; a.tgt_e0 = t.tgt_e0; a.tgt_e1 = t.tgt_e1;
    a.tgt_phase = t.tgt_phase; a.tgt_sin = t.tgt_sin; a.tgt_coh = t.tgt_coh; a.tgt_cells = t.tgt_cells;
    StageTimer tm(c, 14, s);
    HIPCHK(fmcw::launch_aoa(a, s));
    tm.done();
  }
  return FMCW_OK;
}

static int aoa_host_one(fmcw_ctx* c, const fmcw_aoa_params* q, const char* const* rd_ch, int32_t dtype, int64_t F, int32_t nr,
                        int32_t nd, int32_t K, const int32_t* count, const int32_t* ridx, const int32_t* didx,
                        const int32_t* label, const fmcw_angles& out) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const int A = q->n_chan, M = q->max_tgt;
  const size_t fin = (size_t)nr * nd * esize(dtype), flist = (size_t)K * 4;
  // all A channels of a chunk are staged
  const int64_t Fc = host_chunk((size_t)A * fin, F);
  // the shard's outputs in the context's ao_out: the fmcw_angles members in declaration order
  void* host[kAoaOut];
  aoa_members(out, host);
  Arena in, ou;
  size_t oo[kAoaOut], obytes[kAoaOut];
  for (int i = 0; i < kAoaOut; ++i) oo[i] = ou.add(obytes[i] = (size_t)F * 4 * (i < kAoaDet ? K : M));
  const size_t i_count = in.add((size_t)Fc * 4), i_ridx = in.add((size_t)Fc * flist), i_didx = in.add((size_t)Fc * flist),
               i_label = in.add((size_t)Fc * flist);
  CHK(c->ao_out.ensure(ou.off));
  CHK(c->ao_in.ensure(in.off));
  CHK(c->ao_rd.ensure((size_t)A * Fc * fin));
  char* const o = c->ao_out.as<char>();
  char* const di = c->ao_in.as<char>();
  char* const dr = c->ao_rd.as<char>();
  const void* d_ch[fmcw::kAoaChan] = {};
  for (int ch = 0; ch < A; ++ch) d_ch[ch] = dr + (size_t)ch * Fc * fin;   // a multiple of 256 bytes apart
  const fmcw_angles dev{dev_of(out.det_zre, o, oo[0]), dev_of(out.det_zim, o, oo[1]), dev_of(out.det_phase, o, oo[2]),
                        dev_of(out.det_sin, o, oo[3]), dev_of(out.tgt_zre, o, oo[4]), dev_of(out.tgt_zim, o, oo[5]),
                        dev_of(out.tgt_e0, o, oo[6]), dev_of(out.tgt_e1, o, oo[7]), dev_of(out.tgt_phase, o, oo[8]),
                        dev_of(out.tgt_sin, o, oo[9]), dev_of(out.tgt_coh, o, oo[10]), dev_of(out.tgt_cells, o, oo[11])};
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    for (int ch = 0; ch < A; ++ch)
      HIPCHK(hipMemcpyAsync(dr + (size_t)ch * Fc * fin, rd_ch[ch] + (size_t)f0 * fin, (size_t)nf * fin, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(di + i_count, count + f0, (size_t)nf * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(di + i_ridx, ridx + f0 * K, (size_t)nf * flist, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(di + i_didx, didx + f0 * K, (size_t)nf * flist, hipMemcpyHostToDevice, s));
    if (label) HIPCHK(hipMemcpyAsync(di + i_label, label + f0 * K, (size_t)nf * flist, hipMemcpyHostToDevice, s));
    const fmcw_angles d = offset(dev, f0, K, M);
    CHK(fmcw_aoa_device(c, q, d_ch, dtype, nf, nr, nd, K, reinterpret_cast<int32_t*>(di + i_count),
                        reinterpret_cast<int32_t*>(di + i_ridx), reinterpret_cast<int32_t*>(di + i_didx),
                        label ? reinterpret_cast<int32_t*>(di + i_label) : nullptr, &d, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  for (int i = 0; i < kAoaOut; ++i)
    if (host[i]) HIPCHK(hipMemcpyAsync(host[i], o + oo[i], obytes[i], hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_aoa(fmcw_ctx* c, const fmcw_aoa_params* q, const void* const* rd_ch, int32_t rd_dtype, int64_t F, int32_t nr,
             int32_t nd, int32_t max_det, const int32_t* count, const int32_t* ridx, const int32_t* didx,
             const int32_t* label, const fmcw_angles* out) {
  CHK(aoa_entry(c, q, rd_dtype, F, nr, nd, max_det, label, out));
  if (F == 0) return FMCW_OK;
  if (!rd_ch || !count || !ridx || !didx) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int A = q->n_chan;
  for (int ch = 0; ch < A; ++ch)
    if (!rd_ch[ch]) return fail(FMCW_E_ARG, "required pointer is NULL");
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  const int64_t K = max_det, M = q->max_tgt;
  // frames are independent: contiguous shards, each written in place
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    const char* ch0[fmcw::kAoaChan] = {};
    for (int ch = 0; ch < A; ++ch) ch0[ch] = static_cast<const char*>(rd_ch[ch]) + (size_t)f0 * fin;
    return aoa_host_one(d, q, ch0, rd_dtype, n, nr, nd, max_det, count + f0, ridx + f0 * K, didx + f0 * K,
                        shifted(label, f0 * K), offset(*out, f0, K, M));
  });
}

// ---------------------------------------------------------------------------
// Tracks from the per-frame targets (kernels_track.hip)
// ---------------------------------------------------------------------------
int fmcw_track_check(const fmcw_track_params* q, int32_t nr, int32_t nd, int32_t max_tgt) {
  if (!q) return fail(FMCW_E_ARG, "track params is NULL");
  CHK(check_rd_shape("track", nr, nd));
  if (max_tgt < 1 || max_tgt > fmcw::kTrackMax) return fail(FMCW_E_ARG, "track: max_tgt must be in [1, 64]");
  if (!(std::isfinite(q->gate_r) && q->gate_r > 0.f)) return fail(FMCW_E_ARG, "track: gate_r must be finite and > 0");
  if (!(std::isfinite(q->gate_d) && q->gate_d > 0.f)) return fail(FMCW_E_ARG, "track: gate_d must be finite and > 0");
  if (!(q->gate_d < (float)(nd / 2))) return fail(FMCW_E_ARG, "track: gate_d must be below nd/2");
  if (!(q->alpha_r > 0.f && q->alpha_r <= 1.f)) return fail(FMCW_E_ARG, "track: alpha_r must be in (0, 1]");
  if (!(q->alpha_d > 0.f && q->alpha_d <= 1.f)) return fail(FMCW_E_ARG, "track: alpha_d must be in (0, 1]");
  if (!(q->beta_r >= 0.f && q->beta_r <= 1.f)) return fail(FMCW_E_ARG, "track: beta_r must be in [0, 1]");
  if (q->confirm_hits < 1 || q->confirm_hits > 255) return fail(FMCW_E_ARG, "track: confirm_hits must be in [1, 255]");
  if (q->max_coast < 0 || q->max_coast > 255) return fail(FMCW_E_ARG, "track: max_coast must be in [0, 255]");
  if (q->max_trk < 1 || q->max_trk > fmcw::kTrackMax) return fail(FMCW_E_ARG, "track: max_trk must be in [1, 64]");
  if (q->flags != 0) return fail(FMCW_E_ARG, "track: unknown flag bits");
  return FMCW_OK;
}

// what both tracking entries check before they look at F == 0, S == 0 and the pointers
static int track_entry(fmcw_ctx* c, const fmcw_track_params* q, int64_t S, int64_t F, int32_t nr, int32_t nd,
                       int32_t max_tgt) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_track_check(q, nr, nd, max_tgt));
  return check_seq_sizes("track", S, F);
}

int32_t fmcw_track_state_bytes(int32_t max_trk) {
  if (max_trk < 1 || max_trk > fmcw::kTrackMax) return fail(FMCW_E_ARG, "track: max_trk must be in [1, 64]");
  return fmcw::track_state_words(max_trk) * 4;
}

int fmcw_track_device(fmcw_ctx* c, const fmcw_track_params* q, int64_t S, int64_t F, int32_t nr, int32_t nd, int32_t max_tgt,
                      const int32_t* d_count, const float* d_range, const float* d_doppler, const float* d_power,
                      void* d_state, const fmcw_tracks* d_out, int32_t* d_tgt_track, void* stream) {
  CHK(track_entry(c, q, S, F, nr, nd, max_tgt));
  if (F == 0 || S == 0) return FMCW_OK;
  if (!d_count || !d_range || !d_doppler || !d_power || !d_state || !d_out || !d_out->trk_count)
    return fail(FMCW_E_ARG, "required pointer is NULL");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::TrackArgs a{};
  a.S = S; a.F = F; a.NR = nr; a.ND = nd; a.M = max_tgt; a.T = q->max_trk;
  a.wr = (float)(1.0 / ((double)q->gate_r * q->gate_r));
  a.wd = (float)(1.0 / ((double)q->gate_d * q->gate_d));
  a.alpha_r = q->alpha_r; a.alpha_d = q->alpha_d; a.beta_r = q->beta_r;
  a.confirm_hits = q->confirm_hits; a.max_coast = q->max_coast;
  a.tgt_count = d_count; a.range = d_range; a.doppler = d_doppler; a.power = d_power;
  a.state = static_cast<uint32_t*>(d_state);
  a.trk_count = d_out->trk_count;
  a.trk_id = d_out->trk_id; a.trk_status = d_out->trk_status; a.trk_age = d_out->trk_age; a.trk_misses = d_out->trk_misses;
  a.trk_range = d_out->trk_range; a.trk_rate = d_out->trk_range_rate; a.trk_doppler = d_out->trk_doppler;
  a.trk_power = d_out->trk_power;
  a.tgt_track = d_tgt_track;
  StageTimer tm(c, 12, s);
  HIPCHK(fmcw::launch_track(a, s));
  tm.done();
  return FMCW_OK;
}

static int track_host_one(fmcw_ctx* c, const fmcw_track_params* q, int64_t S, int64_t F, int32_t nr, int32_t nd, int32_t M,
                          const int32_t* count, const float* range, const float* doppler, const float* power, void* state,
                          const fmcw_tracks& out, int32_t* tgt_track) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const int T = q->max_trk;
  const size_t sbytes = (size_t)fmcw::track_state_words(T) * 4;
  const size_t frow = (size_t)M * 4, trow = (size_t)T * 4;
  // frames per chunk: a chunk holds that many frames of every sequence of the shard
  const int64_t Fc = host_chunk((size_t)S * (4 + 3 * frow), F);
  // the chunk's outputs in the context's tk_out: the fmcw_tracks members in declaration order, then tgt_track
  void* const host[10] = {out.trk_count, out.trk_id, out.trk_status, out.trk_age, out.trk_misses,
                          out.trk_range, out.trk_range_rate, out.trk_doppler, out.trk_power, tgt_track};
  Arena in, ou;
  size_t oo[10], orow[10];
  for (int i = 0; i < 10; ++i) oo[i] = ou.add((size_t)S * Fc * (orow[i] = i == 0 ? 4 : i == 9 ? frow : trow));
  const size_t i_count = in.add((size_t)S * Fc * 4), i_r = in.add((size_t)S * Fc * frow), i_d = in.add((size_t)S * Fc * frow),
               i_p = in.add((size_t)S * Fc * frow);
  CHK(c->tk_in.ensure(in.off));
  CHK(c->tk_out.ensure(ou.off));
  CHK(c->tk_state.ensure((size_t)S * sbytes));
  char* const di = c->tk_in.as<char>();
  char* const o = c->tk_out.as<char>();
  if (state) HIPCHK(hipMemcpyAsync(c->tk_state.p, state, (size_t)S * sbytes, hipMemcpyHostToDevice, s));
  else HIPCHK(hipMemsetAsync(c->tk_state.p, 0, (size_t)S * sbytes, s));
  const fmcw_tracks d{dev_of(out.trk_count, o, oo[0]), dev_of(out.trk_id, o, oo[1]), dev_of(out.trk_status, o, oo[2]),
                      dev_of(out.trk_age, o, oo[3]), dev_of(out.trk_misses, o, oo[4]), dev_of(out.trk_range, o, oo[5]),
                      dev_of(out.trk_range_rate, o, oo[6]), dev_of(out.trk_doppler, o, oo[7]), dev_of(out.trk_power, o, oo[8])};
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    CHK(seq_rows(di + i_count, const_cast<int32_t*>(count), S, F, f0, nf, 4, true, s));
    CHK(seq_rows(di + i_r, const_cast<float*>(range), S, F, f0, nf, frow, true, s));
    CHK(seq_rows(di + i_d, const_cast<float*>(doppler), S, F, f0, nf, frow, true, s));
    CHK(seq_rows(di + i_p, const_cast<float*>(power), S, F, f0, nf, frow, true, s));
    CHK(fmcw_track_device(c, q, S, nf, nr, nd, M, reinterpret_cast<int32_t*>(di + i_count),
                          reinterpret_cast<float*>(di + i_r), reinterpret_cast<float*>(di + i_d),
                          reinterpret_cast<float*>(di + i_p), c->tk_state.p, &d, dev_of(tgt_track, o, oo[9]), s));
    for (int i = 0; i < 10; ++i)
      if (host[i]) CHK(seq_rows(o + oo[i], host[i], S, F, f0, nf, orow[i], false, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  if (state) HIPCHK(hipMemcpyAsync(state, c->tk_state.p, (size_t)S * sbytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_track(fmcw_ctx* c, const fmcw_track_params* q, int64_t S, int64_t F, int32_t nr, int32_t nd, int32_t max_tgt,
               const int32_t* count, const float* range, const float* doppler, const float* power, void* state,
               const fmcw_tracks* out, int32_t* tgt_track) {
  CHK(track_entry(c, q, S, F, nr, nd, max_tgt));
  if (F == 0 || S == 0) return FMCW_OK;
  if (!count || !range || !doppler || !power || !out || !out->trk_count) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int64_t M = max_tgt, T = q->max_trk;
  const size_t sbytes = (size_t)fmcw::track_state_words(q->max_trk) * 4;
  // the frames of a sequence depend on each other, the sequences do not: contiguous shards of sequences
  return over_devices(c, S, [&](fmcw_ctx* d, int, int64_t s0, int64_t n) {
    const int64_t r0 = s0 * F;
    return track_host_one(d, q, n, F, nr, nd, max_tgt, count + r0, range + r0 * M, doppler + r0 * M, power + r0 * M,
                          shifted(static_cast<char*>(state), s0 * (int64_t)sbytes), offset(*out, r0, T),
                          shifted(tgt_track, r0 * M));
  });
}

// ---------------------------------------------------------------------------
// Frame-to-frame clutter filter of the RD map (kernels_mti.hip)
// ---------------------------------------------------------------------------
int fmcw_mti_check(const fmcw_mti_params* q, int32_t nr, int32_t nd) {
  if (!q) return fail(FMCW_E_ARG, "mti params is NULL");
  CHK(check_rd_shape("mti", nr, nd));
  if (!(std::isfinite(q->lambda) && q->lambda > 0.f && q->lambda <= 1.f))
    return fail(FMCW_E_ARG, "mti: lambda must be finite and in (0, 1]");
  if (q->flags & ~(FMCW_MTI_RAMP | FMCW_MTI_FREEZE)) return fail(FMCW_E_ARG, "mti: unknown flag bits");
  return FMCW_OK;
}

// what both MTI entries check before they look at F == 0, S == 0 and the pointers
static int mti_entry(fmcw_ctx* c, const fmcw_mti_params* q, int32_t rd_dtype, int64_t S, int64_t F, int32_t nr, int32_t nd,
                     const void* out) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_mti_check(q, nr, nd));
  CHK(check_rd_dtype(rd_dtype));
  CHK(check_seq_sizes("mti", S, F));
  if ((q->flags & FMCW_MTI_FREEZE) && !out) return fail(FMCW_E_ARG, "mti: FREEZE without an output leaves nothing to do");
  return FMCW_OK;
}

// frames per lane in flight: the shipped depth of the dtype (FMCW_MTI_RING, one of 4 8 16,
// overrides, for the measurement of tools/bench_mti.py)
int32_t fmcw_mti_ring(int32_t rd_dtype) {
  CHK(check_rd_dtype(rd_dtype));
  if (const char* e = std::getenv("FMCW_MTI_RING"); e && fmcw::mti_ring_ok(std::atoi(e))) return std::atoi(e);
  return rd_dtype == FMCW_C32H ? fmcw::kMtiRingC32H : fmcw::kMtiRingC64;
}

int fmcw_mti_device(fmcw_ctx* c, const fmcw_mti_params* q, const void* d_rd, int32_t rd_dtype, int64_t S, int64_t F,
                    int32_t nr, int32_t nd, float* d_bg, int32_t* d_seen, void* d_out, void* stream) {
  CHK(mti_entry(c, q, rd_dtype, S, F, nr, nd, d_out));
  if (F == 0 || S == 0) return FMCW_OK;
  if (!d_rd || !d_bg || !d_seen) return fail(FMCW_E_ARG, "required pointer is NULL");
  const uintptr_t pr = reinterpret_cast<uintptr_t>(d_rd), po = reinterpret_cast<uintptr_t>(d_out);
  if ((pr | po | reinterpret_cast<uintptr_t>(d_bg) | reinterpret_cast<uintptr_t>(d_seen)) & 15)
    return fail(FMCW_E_ARG, "mti: d_rd, d_out, d_bg and d_seen must be 16-byte aligned");
  const size_t fin = (size_t)nr * nd * esize(rd_dtype), total = (size_t)S * F * fin;
  if (d_out && po != pr && po < pr + total && pr < po + total)
    return fail(FMCW_E_ARG, "mti: d_out must be d_rd itself or not overlap it");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::MtiArgs a{};
  a.rd = d_rd; a.out = d_out; a.bg = d_bg; a.seen = d_seen;
  a.S = S; a.F = F;
  a.n16 = (int64_t)(fin / 16);
  a.h = rd_dtype == FMCW_C32H;
  a.ring = fmcw_mti_ring(rd_dtype);
  a.lambda = q->lambda;
  a.ramp = (q->flags & FMCW_MTI_RAMP) ? 1 : 0;
  a.freeze = (q->flags & FMCW_MTI_FREEZE) ? 1 : 0;
  StageTimer tm(c, 13, s);
  HIPCHK(fmcw::launch_mti(a, s));
  tm.done();
  return FMCW_OK;
}

static int mti_host_one(fmcw_ctx* c, const fmcw_mti_params* q, const char* rd, int32_t dtype, int64_t S, int64_t F, int32_t nr,
                        int32_t nd, float* bg, int32_t* seen, char* out) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const size_t fin = (size_t)nr * nd * esize(dtype), bbytes = (size_t)nr * nd * 8;
  // frames per chunk: a chunk holds that many frames of every sequence of the shard
  const int64_t Fc = host_chunk((size_t)S * fin, F);
  CHK(c->mt_rd.ensure((size_t)S * Fc * fin));
  CHK(c->mt_bg.ensure((size_t)S * bbytes));
  CHK(c->mt_seen.ensure((size_t)S * 4));
  if (bg) {
    HIPCHK(hipMemcpyAsync(c->mt_bg.p, bg, (size_t)S * bbytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->mt_seen.p, seen, (size_t)S * 4, hipMemcpyHostToDevice, s));
  } else {
    HIPCHK(hipMemsetAsync(c->mt_bg.p, 0, (size_t)S * bbytes, s));
    HIPCHK(hipMemsetAsync(c->mt_seen.p, 0, (size_t)S * 4, s));
  }
  char* const d = c->mt_rd.as<char>();
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    CHK(seq_rows(d, const_cast<char*>(rd), S, F, f0, nf, fin, true, s));
    CHK(fmcw_mti_device(c, q, d, dtype, S, nf, nr, nd, c->mt_bg.as<float>(), c->mt_seen.as<int32_t>(), out ? d : nullptr, s));
    if (out) CHK(seq_rows(d, out, S, F, f0, nf, fin, false, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffer is reused by the next chunk
  }
  if (bg) {
    HIPCHK(hipMemcpyAsync(bg, c->mt_bg.p, (size_t)S * bbytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(seen, c->mt_seen.p, (size_t)S * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_mti(fmcw_ctx* c, const fmcw_mti_params* q, const void* rd, int32_t rd_dtype, int64_t S, int64_t F, int32_t nr,
             int32_t nd, float* bg, int32_t* seen, void* out) {
  CHK(mti_entry(c, q, rd_dtype, S, F, nr, nd, out));
  if ((bg == nullptr) != (seen == nullptr)) return fail(FMCW_E_ARG, "mti: bg and seen must both be given or both be NULL");
  if (F == 0 || S == 0) return FMCW_OK;
  if (!rd) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int64_t fin = (int64_t)nr * nd * (int64_t)esize(rd_dtype), cells2 = (int64_t)nr * nd * 2;
  // the frames of a sequence depend on each other, the sequences do not: contiguous shards of sequences
  return over_devices(c, S, [&](fmcw_ctx* d, int, int64_t s0, int64_t n) {
    return mti_host_one(d, q, static_cast<const char*>(rd) + s0 * F * fin, rd_dtype, n, F, nr, nd,
                        shifted(bg, s0 * cells2), shifted(seen, s0), shifted(static_cast<char*>(out), s0 * F * fin));
  });
}

// ---------------------------------------------------------------------------
// The receive channels' RD maps combined into beams or one integrated map (kernels_beam.hip)
// ---------------------------------------------------------------------------
int fmcw_beam_check(const fmcw_beam_params* q, int32_t nr, int32_t nd) {
  if (!q) return fail(FMCW_E_ARG, "beam params is NULL");
  CHK(check_rd_shape("beam", nr, nd));
  if (q->n_chan < 2 || q->n_chan > fmcw::kBeamMax) return fail(FMCW_E_ARG, "beam: n_chan must be in [2, 8]");
  if (q->n_beam < 1 || q->n_beam > fmcw::kBeamMax) return fail(FMCW_E_ARG, "beam: n_beam must be in [1, 8]");
  if (q->flags & ~FMCW_BEAM_NCI) return fail(FMCW_E_ARG, "beam: unknown flag bits");
  if ((q->flags & FMCW_BEAM_NCI) && q->n_beam != 1) return fail(FMCW_E_ARG, "beam: FMCW_BEAM_NCI needs n_beam == 1");
  for (int b = 0; b < q->n_beam; ++b)
    for (int a = 0; a < q->n_chan; ++a)
      if (!std::isfinite(q->w[b][a][0]) || !std::isfinite(q->w[b][a][1]))
        return fail(FMCW_E_ARG, "beam: the weights must be finite");
  return FMCW_OK;
}

// The weights of n_dir look directions of a uniform line of n_chan elements, flat [n_dir][n_chan][2]:
// what fmcw_beam_steer and fmcw_ra_steer both are (one formula, one rounding, one set of argument
// rules; `stage` prefixes the messages, `count` names the number of directions, at most max_dir).
static int steer_table(const std::string& stage, const char* count, int max_dir, int32_t n_chan, int32_t n_dir, float spacing,
                       const float* sin_theta, const float* cal, const float* taper, int32_t normalize, std::vector<float>& w) {
#pragma clang fp contract(off)
  if (n_chan < 2 || n_chan > fmcw::kBeamMax) return fail(FMCW_E_ARG, stage + ": n_chan must be in [2, 8]");
  if (n_dir < 1 || n_dir > max_dir)
    return fail(FMCW_E_ARG, stage + ": " + count + " must be in [1, " + std::to_string(max_dir) + "]");
  if (!std::isfinite(spacing) || !(std::fabs(spacing) >= 0.01f && std::fabs(spacing) <= 16.f))
    return fail(FMCW_E_ARG, stage + ": spacing must be finite with 0.01 <= |spacing| <= 16");
  if (!sin_theta) return fail(FMCW_E_ARG, stage + ": sin_theta is NULL");
  for (int b = 0; b < n_dir; ++b)
    if (!(sin_theta[b] >= -1.f && sin_theta[b] <= 1.f)) return fail(FMCW_E_ARG, stage + ": every sin_theta must be in [-1, 1]");
  if (cal)
    for (int i = 0; i < 2 * n_chan; ++i)
      if (!std::isfinite(cal[i])) return fail(FMCW_E_ARG, stage + ": cal must be finite");
  double norm = normalize ? (double)n_chan : 1.0;
  if (taper) {
    double sum = 0.0;
    for (int a = 0; a < n_chan; ++a) {
      if (!std::isfinite(taper[a])) return fail(FMCW_E_ARG, stage + ": taper must be finite");
      sum = sum + (double)taper[a];
    }
    if (normalize && sum == 0.0) return fail(FMCW_E_ARG, stage + ": normalize needs a taper whose sum is not 0");
    if (normalize) norm = sum;
  }
  w.assign((size_t)n_dir * n_chan * 2, 0.f);
  for (int b = 0; b < n_dir; ++b)
    for (int a = 0; a < n_chan; ++a) {
      // the phase -2 pi spacing a sin(theta) in turns, reduced to [-1/2, 1/2], then split into k whole
      // quarter turns and a rest f in [-1/2, 1/2] of a quarter turn: f = 0 gives exactly 1 and 0
      double t = -((double)spacing * (double)a * (double)sin_theta[b]);
      t = t - std::nearbyint(t);
      const double q4 = 4.0 * t;
      const double k = std::nearbyint(q4);
      const double ang = (q4 - k) * 1.5707963267948966;
      const double c = std::cos(ang), s = std::sin(ang);
      double er, ei;
      switch (((int)k + 4) & 3) {
        case 0: er = c; ei = s; break;
        case 1: er = 0.0 - s; ei = c; break;
        case 2: er = 0.0 - c; ei = 0.0 - s; break;
        default: er = s; ei = 0.0 - c; break;
      }
      const double g = (taper ? (double)taper[a] : 1.0) / norm;
      const double gr = (cal ? (double)cal[2 * a] : 1.0) * g, gi = (cal ? (double)cal[2 * a + 1] : 0.0) * g;
      float* const o = &w[((size_t)b * n_chan + a) * 2];
      o[0] = (float)(gr * er - gi * ei);
      o[1] = (float)(gr * ei + gi * er);
      if (!std::isfinite(o[0]) || !std::isfinite(o[1])) return fail(FMCW_E_ARG, stage + ": a weight does not fit float32");
    }
  return FMCW_OK;
}

int fmcw_beam_steer(int32_t n_chan, int32_t n_beam, float spacing, const float* sin_theta, const float* cal,
                    const float* taper, int32_t normalize, fmcw_beam_params* q) {
  if (!q) return fail(FMCW_E_ARG, "beam params is NULL");
  std::vector<float> t;
  CHK(steer_table("beam", "n_beam", fmcw::kBeamMax, n_chan, n_beam, spacing, sin_theta, cal, taper, normalize, t));
  float w[fmcw::kBeamMax][fmcw::kBeamMax][2] = {};
  for (int b = 0; b < n_beam; ++b)
    for (int a = 0; a < n_chan; ++a) {
      w[b][a][0] = t[((size_t)b * n_chan + a) * 2];
      w[b][a][1] = t[((size_t)b * n_chan + a) * 2 + 1];
    }
  q->n_chan = n_chan;
  q->n_beam = n_beam;
  q->flags = 0;
  std::memcpy(q->w, w, sizeof(w));
  return FMCW_OK;
}

// what both beam entries check: everything but the alignment, which only the device call asks for
static int beam_entry(fmcw_ctx* c, const fmcw_beam_params* q, const void* const* rd, int32_t rd_dtype, int64_t F, int32_t nr,
                      int32_t nd, void* const* out) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_beam_check(q, nr, nd));
  CHK(check_rd_dtype(rd_dtype));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F > ((int64_t)1 << 40)) return fail(FMCW_E_ARG, "beam: F must be at most 2^40");
  if (F == 0) return FMCW_OK;
  if (!rd || !out) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int A = q->n_chan, B = q->n_beam;
  for (int a = 0; a < A; ++a)
    if (!rd[a]) return fail(FMCW_E_ARG, "required pointer is NULL");
  for (int b = 0; b < B; ++b)
    if (!out[b]) return fail(FMCW_E_ARG, "required pointer is NULL");
  const uintptr_t total = (uintptr_t)F * nr * nd * esize(rd_dtype);
  for (int b = 0; b < B; ++b) {
    const uintptr_t po = reinterpret_cast<uintptr_t>(out[b]);
    for (int a = 0; a < A; ++a) {
      const uintptr_t pa = reinterpret_cast<uintptr_t>(rd[a]);
      if (po != pa && po < pa + total && pa < po + total)
        return fail(FMCW_E_ARG, "beam: an output must be one of the inputs itself or not overlap it");
    }
    for (int b2 = 0; b2 < b; ++b2) {
      const uintptr_t p2 = reinterpret_cast<uintptr_t>(out[b2]);
      if (po == p2) return fail(FMCW_E_ARG, "beam: two outputs at the same address");
      if (po < p2 + total && p2 < po + total) return fail(FMCW_E_ARG, "beam: the outputs must not overlap each other");
    }
  }
  return FMCW_OK;
}

int fmcw_beam_device(fmcw_ctx* c, const fmcw_beam_params* q, const void* const* d_rd_ch, int32_t rd_dtype, int64_t F,
                     int32_t nr, int32_t nd, void* const* d_out, void* stream) {
  CHK(beam_entry(c, q, d_rd_ch, rd_dtype, F, nr, nd, d_out));
  if (F == 0) return FMCW_OK;
  const int A = q->n_chan, B = q->n_beam;
  for (int a = 0; a < A; ++a)
    if (reinterpret_cast<uintptr_t>(d_rd_ch[a]) & 15) return fail(FMCW_E_ARG, "beam: every channel's d_rd must be 16-byte aligned");
  for (int b = 0; b < B; ++b)
    if (reinterpret_cast<uintptr_t>(d_out[b]) & 15) return fail(FMCW_E_ARG, "beam: every d_out must be 16-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::BeamArgs a{};
  a.A = A; a.B = B;
  a.h = rd_dtype == FMCW_C32H;
  a.nci = (q->flags & FMCW_BEAM_NCI) ? 1 : 0;
  for (int b = 0; b < B; ++b)
    for (int ch = 0; ch < A; ++ch) {
      a.w[b][ch][0] = q->w[b][ch][0];
      a.w[b][ch][1] = q->w[b][ch][1];
    }
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  const int64_t f16 = (int64_t)(fin / 16);
  // one thread per 16-byte piece: at most 2^31 pieces per launch, a grid of fewer than 2^32 threads
  // (the results do not depend on the cut)
  const int64_t Fc = ((int64_t)1 << 31) / f16;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.n16 = std::min(Fc, F - f0) * f16;
    for (int ch = 0; ch < A; ++ch) a.rd[ch] = static_cast<const char*>(d_rd_ch[ch]) + (size_t)f0 * fin;
    for (int b = 0; b < B; ++b) a.out[b] = static_cast<char*>(d_out[b]) + (size_t)f0 * fin;
    StageTimer tm(c, 15, s);
    HIPCHK(fmcw::launch_beam(a, s));
    tm.done();
  }
  return FMCW_OK;
}

static int beam_host_one(fmcw_ctx* c, const fmcw_beam_params* q, const char* const* rd_ch, int32_t dtype, int64_t F, int32_t nr,
                         int32_t nd, char* const* out) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const int A = q->n_chan, B = q->n_beam;
  const size_t fin = (size_t)nr * nd * esize(dtype);
  // all A channels and all B outputs of a chunk are staged
  const int64_t Fc = host_chunk((size_t)(A + B) * fin, F);
  CHK(c->bm_rd.ensure((size_t)A * Fc * fin));
  CHK(c->bm_out.ensure((size_t)B * Fc * fin));
  char* const dr = c->bm_rd.as<char>();
  char* const dout = c->bm_out.as<char>();
  const void* d_ch[fmcw::kBeamMax] = {};
  void* d_o[fmcw::kBeamMax] = {};
  for (int ch = 0; ch < A; ++ch) d_ch[ch] = dr + (size_t)ch * Fc * fin;   // a multiple of 256 bytes apart
  for (int b = 0; b < B; ++b) d_o[b] = dout + (size_t)b * Fc * fin;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    for (int ch = 0; ch < A; ++ch)
      HIPCHK(hipMemcpyAsync(dr + (size_t)ch * Fc * fin, rd_ch[ch] + (size_t)f0 * fin, (size_t)nf * fin, hipMemcpyHostToDevice, s));
    CHK(fmcw_beam_device(c, q, d_ch, dtype, nf, nr, nd, d_o, s));
    // an output may be one of the inputs: every channel of the chunk is on the device before this
    for (int b = 0; b < B; ++b)
      HIPCHK(hipMemcpyAsync(out[b] + (size_t)f0 * fin, dout + (size_t)b * Fc * fin, (size_t)nf * fin, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  return FMCW_OK;
}

int fmcw_beam(fmcw_ctx* c, const fmcw_beam_params* q, const void* const* rd_ch, int32_t rd_dtype, int64_t F, int32_t nr,
              int32_t nd, void* const* out) {
  CHK(beam_entry(c, q, rd_ch, rd_dtype, F, nr, nd, out));
  if (F == 0) return FMCW_OK;
  const int A = q->n_chan, B = q->n_beam;
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  // frames are independent: contiguous shards, each written in place
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    const char* ch0[fmcw::kBeamMax] = {};
    char* o0[fmcw::kBeamMax] = {};
    for (int ch = 0; ch < A; ++ch) ch0[ch] = static_cast<const char*>(rd_ch[ch]) + (size_t)f0 * fin;
    for (int b = 0; b < B; ++b) o0[b] = static_cast<char*>(out[b]) + (size_t)f0 * fin;
    return beam_host_one(d, q, ch0, rd_dtype, n, nr, nd, o0);
  });
}

// ---------------------------------------------------------------------------
// Range-angle maps: the channels' spatial covariance per range row and its Bartlett / Capon
// spectra (kernels_ra.hip)
// ---------------------------------------------------------------------------
// the rules of fmcw_ra_params; fmcw_ra_device has no nd to hold dc_half against
static int ra_rules(const fmcw_ra_params* q, int32_t nr, int32_t nd, bool have_nd) {
  if (!q) return fail(FMCW_E_ARG, "ra params is NULL");
  CHK(check_rd_shape("ra", nr, have_nd ? nd : 4));
  CHK(check_gate("ra", q->r_lo, q->r_hi, nr));
  if (q->n_chan < 2 || q->n_chan > fmcw::kRaChan) return fail(FMCW_E_ARG, "ra: n_chan must be in [2, 8]");
  if (q->n_ang < 1 || q->n_ang > fmcw::kRaAngMax) return fail(FMCW_E_ARG, "ra: n_ang must be in [1, 256]");
  if (q->dc_half < -1) return fail(FMCW_E_ARG, "ra: dc_half must be >= -1 (-1 leaves no Doppler bin out)");
  if (have_nd && 2 * (int64_t)q->dc_half + 1 >= nd) return fail(FMCW_E_ARG, "ra: 2 dc_half + 1 must be < nd");
  if (q->flags & ~FMCW_RA_CAPON) return fail(FMCW_E_ARG, "ra: unknown flag bits");
  if (!(std::isfinite(q->load) && q->load >= 0.f)) return fail(FMCW_E_ARG, "ra: load must be finite and >= 0");
  return FMCW_OK;
}

int fmcw_ra_check(const fmcw_ra_params* q, int32_t nr, int32_t nd) { return ra_rules(q, nr, nd, true); }

int fmcw_ra_steer(int32_t n_chan, int32_t n_ang, float spacing, const float* sin_theta, const float* cal, const float* taper,
                  int32_t normalize, float* w) {
  if (!w) return fail(FMCW_E_ARG, "ra: w is NULL");
  std::vector<float> t;
  CHK(steer_table("ra", "n_ang", fmcw::kRaAngMax, n_chan, n_ang, spacing, sin_theta, cal, taper, normalize, t));
  std::memcpy(w, t.data(), t.size() * sizeof(float));
  return FMCW_OK;
}

// what the three calls check before they look at F == 0 and the pointers
static int ra_entry(fmcw_ctx* c, const fmcw_ra_params* q, int64_t F, int32_t nr, int32_t nd, bool have_nd) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(ra_rules(q, nr, nd, have_nd));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F > ((int64_t)1 << 40)) return fail(FMCW_E_ARG, "ra: F must be at most 2^40");
  return FMCW_OK;
}

int fmcw_cov_device(fmcw_ctx* c, const fmcw_ra_params* q, const void* const* d_rd_ch, int32_t rd_dtype, int64_t F, int32_t nr,
                    int32_t nd, float* d_cov, void* stream) {
  CHK(ra_entry(c, q, F, nr, nd, true));
  CHK(check_rd_dtype(rd_dtype));
  if (F == 0) return FMCW_OK;
  if (!d_rd_ch || !d_cov) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int A = q->n_chan;
  for (int a = 0; a < A; ++a)
    if (!d_rd_ch[a]) return fail(FMCW_E_ARG, "required pointer is NULL");
  for (int a = 0; a < A; ++a)
    if (reinterpret_cast<uintptr_t>(d_rd_ch[a]) & 15) return fail(FMCW_E_ARG, "ra: every channel's d_rd must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_cov) & 15) return fail(FMCW_E_ARG, "ra: d_cov must be 16-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::CovArgs a{};
  a.A = A; a.NR = nr; a.ND = nd;
  a.h = rd_dtype == FMCW_C32H;
  a.scale2 = a.h ? ((float)nr * (float)nd) * ((float)nr * (float)nd) : 1.f;
  gate_rows(q->r_lo, q->r_hi, nr, a.g0, a.g1);
  a.dc = q->dc_half;
  a.rpw = fmcw::cov_rows_per_wave(nd, a.h);
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  const size_t T = (size_t)A * (A + 1) / 2;
  // at most kRaRowsMax rows per launch (the results do not depend on the cut)
  const int64_t Fc = fmcw::kRaRowsMax / nr;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.rows = std::min(Fc, F - f0) * nr;
    for (int ch = 0; ch < A; ++ch) a.rd[ch] = static_cast<const char*>(d_rd_ch[ch]) + (size_t)f0 * fin;
    a.cov = d_cov + (size_t)f0 * nr * T * 2;
    StageTimer tm(c, 17, s);
    HIPCHK(fmcw::launch_cov(a, s));
    tm.done();
  }
  return FMCW_OK;
}

int fmcw_ra_device(fmcw_ctx* c, const fmcw_ra_params* q, const float* d_cov, int64_t F, int32_t nr, const float* d_w,
                   float* d_ra, float* d_ra_max, void* stream) {
  CHK(ra_entry(c, q, F, nr, 0, false));
  if (F == 0) return FMCW_OK;
  if (!d_cov || !d_w || !d_ra) return fail(FMCW_E_ARG, "required pointer is NULL");
  if ((reinterpret_cast<uintptr_t>(d_cov) | reinterpret_cast<uintptr_t>(d_w) | reinterpret_cast<uintptr_t>(d_ra)) & 15)
    return fail(FMCW_E_ARG, "ra: d_cov, d_w and d_ra must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_ra_max) & 3) return fail(FMCW_E_ARG, "ra: d_ra_max must be 4-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::RaArgs a{};
  a.A = q->n_chan; a.NR = nr; a.n_ang = q->n_ang;
  gate_rows(q->r_lo, q->r_hi, nr, a.g0, a.g1);
  a.capon = (q->flags & FMCW_RA_CAPON) ? 1 : 0;
  a.load = q->load;
  a.w = d_w;
  a.ra_max = d_ra_max;
  const size_t T = (size_t)a.A * (a.A + 1) / 2;
  const int64_t Fc = fmcw::kRaRowsMax / nr;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.rows = std::min(Fc, F - f0) * nr;
    a.cov = d_cov + (size_t)f0 * nr * T * 2;
    a.ra = d_ra + (size_t)f0 * nr * a.n_ang;
    StageTimer tm(c, 17, s);
    HIPCHK(fmcw::launch_ra(a, s));
    tm.done();
  }
  return FMCW_OK;
}

// One shard of fmcw_ra, chunk by chunk: the chunk's frames of every channel in, cov and ra out.
static int ra_host_one(fmcw_ctx* c, const fmcw_ra_params* q, const char* const* rd_ch, int32_t dtype, int64_t F, int32_t nr,
                       int32_t nd, const float* w, float* cov, float* ra, float* mx) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const int A = q->n_chan, K = q->n_ang;
  const size_t fin = (size_t)nr * nd * esize(dtype);
  const size_t covf = (size_t)nr * A * (A + 1), raf = (size_t)nr * K;   // floats per frame
  const int64_t Fc = host_chunk((size_t)A * fin, F);
  Arena ar;
  const size_t o_w = ar.add((size_t)K * A * 8), o_mx = ar.add(4);
  CHK(c->ra_rd.ensure((size_t)A * Fc * fin));
  CHK(c->ra_cov.ensure((size_t)Fc * covf * 4));
  char* const dr = c->ra_rd.as<char>();
  const void* d_ch[fmcw::kRaChan] = {};
  for (int ch = 0; ch < A; ++ch) d_ch[ch] = dr + (size_t)ch * Fc * fin;   // a multiple of 256 bytes apart
  // the spectra's buffers only where the spectra are asked for
  float* d_w = nullptr;
  float* d_mx = nullptr;
  if (ra) {
    CHK(c->ra_out.ensure((size_t)Fc * raf * 4));
    CHK(c->ra_w.ensure(ar.off));
    d_w = reinterpret_cast<float*>(c->ra_w.as<char>() + o_w);
    d_mx = reinterpret_cast<float*>(c->ra_w.as<char>() + o_mx);
    HIPCHK(hipMemsetAsync(d_mx, 0, 4, s));
    HIPCHK(hipMemcpyAsync(d_w, w, (size_t)K * A * 8, hipMemcpyHostToDevice, s));
  }
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    for (int ch = 0; ch < A; ++ch)
      HIPCHK(hipMemcpyAsync(dr + (size_t)ch * Fc * fin, rd_ch[ch] + (size_t)f0 * fin, (size_t)nf * fin, hipMemcpyHostToDevice, s));
    CHK(fmcw_cov_device(c, q, d_ch, dtype, nf, nr, nd, c->ra_cov.as<float>(), s));
    if (ra) CHK(fmcw_ra_device(c, q, c->ra_cov.as<float>(), nf, nr, d_w, c->ra_out.as<float>(), d_mx, s));
    if (cov) HIPCHK(hipMemcpyAsync(cov + (size_t)f0 * covf, c->ra_cov.p, (size_t)nf * covf * 4, hipMemcpyDeviceToHost, s));
    if (ra) HIPCHK(hipMemcpyAsync(ra + (size_t)f0 * raf, c->ra_out.p, (size_t)nf * raf * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  *mx = 0.f;
  if (ra) HIPCHK(hipMemcpyAsync(mx, d_mx, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_ra(fmcw_ctx* c, const fmcw_ra_params* q, const void* const* rd_ch, int32_t rd_dtype, int64_t F, int32_t nr, int32_t nd,
            const float* w, float* cov, float* ra, float* ra_max) {
  CHK(ra_entry(c, q, F, nr, nd, true));
  CHK(check_rd_dtype(rd_dtype));
  if (!cov && !ra) return fail(FMCW_E_ARG, "ra: cov and ra are both NULL");
  if (F == 0) {
    if (ra_max) *ra_max = 0.f;
    return FMCW_OK;
  }
  if (!rd_ch || (ra && !w)) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int A = q->n_chan;
  for (int ch = 0; ch < A; ++ch)
    if (!rd_ch[ch]) return fail(FMCW_E_ARG, "required pointer is NULL");
  const size_t fin = (size_t)nr * nd * esize(rd_dtype);
  const int64_t covf = (int64_t)nr * A * (A + 1), raf = (int64_t)nr * q->n_ang;
  const int world = 1 + (int)c->peers.size();
  std::vector<float> mx((size_t)world, 0.f);
  // frames are independent: contiguous shards, each written in place
  CHK(over_devices(c, F, [&](fmcw_ctx* d, int g, int64_t f0, int64_t n) {
    const char* ch0[fmcw::kRaChan] = {};
    for (int ch = 0; ch < A; ++ch) ch0[ch] = static_cast<const char*>(rd_ch[ch]) + (size_t)f0 * fin;
    return ra_host_one(d, q, ch0, rd_dtype, n, nr, nd, w, shifted(cov, f0 * covf), shifted(ra, f0 * raf), &mx[(size_t)g]);
  }));
  float gmx = 0.f;                             // a maximum of non-negative floats does not depend on order
  for (int g = 0; g < world; ++g) gmx = std::max(gmx, mx[(size_t)g]);
  if (ra_max) *ra_max = gmx;
  return FMCW_OK;
}

// ---------------------------------------------------------------------------
// MUSIC: per range row the eigen-decomposition of its covariance, a source count and the MUSIC
// pseudo-spectrum (kernels_music.hip)
// ---------------------------------------------------------------------------
int fmcw_music_check(const fmcw_music_params* q, int32_t nr) {
  if (!q) return fail(FMCW_E_ARG, "music params is NULL");
  CHK(check_rd_shape("music", nr, 4));
  CHK(check_gate("music", q->r_lo, q->r_hi, nr));
  if (q->n_chan < 2 || q->n_chan > fmcw::kRaChan) return fail(FMCW_E_ARG, "music: n_chan must be in [2, 8]");
  if (q->n_ang < 1 || q->n_ang > fmcw::kRaAngMax) return fail(FMCW_E_ARG, "music: n_ang must be in [1, 256]");
  if (q->n_src < 0 || q->n_src >= q->n_chan) return fail(FMCW_E_ARG, "music: n_src must be in [0, n_chan - 1] (0 estimates it)");
  if (q->n_src == 0 && (q->max_src < 1 || q->max_src >= q->n_chan))
    return fail(FMCW_E_ARG, "music: max_src must be in [1, n_chan - 1] when n_src is 0");
  if (q->sweeps < 1 || q->sweeps > 16) return fail(FMCW_E_ARG, "music: sweeps must be in [1, 16]");
  if (q->flags & ~FMCW_MUSIC_FB) return fail(FMCW_E_ARG, "music: unknown flag bits");
  if (!(std::isfinite(q->src_thr) && q->src_thr > 0.f)) return fail(FMCW_E_ARG, "music: src_thr must be finite and > 0");
  return FMCW_OK;
}

static int music_entry(fmcw_ctx* c, const fmcw_music_params* q, int64_t F, int32_t nr) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_music_check(q, nr));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F > ((int64_t)1 << 40)) return fail(FMCW_E_ARG, "music: F must be at most 2^40");
  return FMCW_OK;
}

int fmcw_music_device(fmcw_ctx* c, const fmcw_music_params* q, const float* d_cov, int64_t F, int32_t nr, const float* d_w,
                      float* d_eval, float* d_evec, int32_t* d_nsrc, float* d_music, float* d_music_max, void* stream) {
  CHK(music_entry(c, q, F, nr));
  if (!d_eval && !d_evec && !d_nsrc && !d_music) return fail(FMCW_E_ARG, "music: every output is NULL");
  if (F == 0) return FMCW_OK;
  if (!d_cov || (d_music && !d_w)) return fail(FMCW_E_ARG, "required pointer is NULL");
  if ((reinterpret_cast<uintptr_t>(d_cov) | reinterpret_cast<uintptr_t>(d_w) | reinterpret_cast<uintptr_t>(d_eval) |
       reinterpret_cast<uintptr_t>(d_evec) | reinterpret_cast<uintptr_t>(d_nsrc) | reinterpret_cast<uintptr_t>(d_music)) & 15)
    return fail(FMCW_E_ARG, "music: d_cov, d_w, d_eval, d_evec, d_nsrc and d_music must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_music_max) & 3) return fail(FMCW_E_ARG, "music: d_music_max must be 4-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::MusicArgs a{};
  a.A = q->n_chan; a.NR = nr; a.n_ang = q->n_ang;
  gate_rows(q->r_lo, q->r_hi, nr, a.g0, a.g1);
  a.n_src = q->n_src;
  a.max_src = q->n_src ? 1 : q->max_src;
  a.sweeps = q->sweeps;
  a.fb = (q->flags & FMCW_MUSIC_FB) ? 1 : 0;
  a.src_thr = q->src_thr;
  a.w = d_music ? d_w : nullptr;
  a.music_max = d_music ? d_music_max : nullptr;
  const size_t A = (size_t)a.A, T = A * (A + 1) / 2;
  // at most kRaRowsMax rows per launch (the results do not depend on the cut)
  const int64_t Fc = fmcw::kRaRowsMax / nr;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.rows = std::min(Fc, F - f0) * nr;
    const size_t r0 = (size_t)f0 * nr;
    a.cov = d_cov + r0 * T * 2;
    a.eval = shifted(d_eval, (int64_t)(r0 * A));
    a.evec = shifted(d_evec, (int64_t)(r0 * A * A * 2));
    a.nsrc = shifted(d_nsrc, (int64_t)r0);
    a.music = shifted(d_music, (int64_t)(r0 * a.n_ang));
    StageTimer tm(c, 18, s);
    HIPCHK(fmcw::launch_music(a, s));
    tm.done();
  }
  return FMCW_OK;
}

// One shard of fmcw_music, chunk by chunk: the chunk's covariances in, what was asked for out.
static int music_host_one(fmcw_ctx* c, const fmcw_music_params* q, const float* cov, int64_t F, int32_t nr, const float* w,
                          float* eval, float* evec, int32_t* nsrc, float* music, float* mx) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const size_t A = (size_t)q->n_chan, K = (size_t)q->n_ang;
  const size_t covf = (size_t)nr * A * (A + 1), evf = (size_t)nr * A, vecf = (size_t)nr * A * A * 2, muf = (size_t)nr * K;   // per frame
  const int64_t Fc = host_chunk(covf * 4, F);
  Arena ar;
  const size_t o_w = ar.add(K * A * 8), o_mx = ar.add(4);
  CHK(c->mu_cov.ensure((size_t)Fc * covf * 4));
  if (eval) CHK(c->mu_eval.ensure((size_t)Fc * evf * 4));
  if (evec) CHK(c->mu_evec.ensure((size_t)Fc * vecf * 4));
  if (nsrc) CHK(c->mu_nsrc.ensure((size_t)Fc * nr * 4));
  float* d_w = nullptr;
  float* d_mx = nullptr;
  if (music) {
    CHK(c->mu_out.ensure((size_t)Fc * muf * 4));
    CHK(c->mu_w.ensure(ar.off));
    d_w = reinterpret_cast<float*>(c->mu_w.as<char>() + o_w);
    d_mx = reinterpret_cast<float*>(c->mu_w.as<char>() + o_mx);
    HIPCHK(hipMemsetAsync(d_mx, 0, 4, s));
    HIPCHK(hipMemcpyAsync(d_w, w, K * A * 8, hipMemcpyHostToDevice, s));
  }
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    HIPCHK(hipMemcpyAsync(c->mu_cov.p, cov + (size_t)f0 * covf, (size_t)nf * covf * 4, hipMemcpyHostToDevice, s));
    CHK(fmcw_music_device(c, q, c->mu_cov.as<float>(), nf, nr, d_w, eval ? c->mu_eval.as<float>() : nullptr,
                          evec ? c->mu_evec.as<float>() : nullptr, nsrc ? c->mu_nsrc.as<int32_t>() : nullptr,
                          music ? c->mu_out.as<float>() : nullptr, d_mx, s));
    if (eval) HIPCHK(hipMemcpyAsync(eval + (size_t)f0 * evf, c->mu_eval.p, (size_t)nf * evf * 4, hipMemcpyDeviceToHost, s));
    if (evec) HIPCHK(hipMemcpyAsync(evec + (size_t)f0 * vecf, c->mu_evec.p, (size_t)nf * vecf * 4, hipMemcpyDeviceToHost, s));
    if (nsrc) HIPCHK(hipMemcpyAsync(nsrc + (size_t)f0 * nr, c->mu_nsrc.p, (size_t)nf * nr * 4, hipMemcpyDeviceToHost, s));
    if (music) HIPCHK(hipMemcpyAsync(music + (size_t)f0 * muf, c->mu_out.p, (size_t)nf * muf * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  *mx = 0.f;
  if (music) HIPCHK(hipMemcpyAsync(mx, d_mx, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int fmcw_music(fmcw_ctx* c, const fmcw_music_params* q, const float* cov, int64_t F, int32_t nr, const float* w, float* eval,
               float* evec, int32_t* nsrc, float* music, float* music_max) {
  CHK(music_entry(c, q, F, nr));
  if (!eval && !evec && !nsrc && !music) return fail(FMCW_E_ARG, "music: every output is NULL");
  if (F == 0) {
    if (music_max) *music_max = 0.f;
    return FMCW_OK;
  }
  if (!cov || (music && !w)) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int64_t A = q->n_chan;
  const int64_t covf = (int64_t)nr * A * (A + 1), evf = (int64_t)nr * A, vecf = (int64_t)nr * A * A * 2, muf = (int64_t)nr * q->n_ang;
  const int world = 1 + (int)c->peers.size();
  std::vector<float> mx((size_t)world, 0.f);
  // frames are independent: contiguous shards, each written in place
  CHK(over_devices(c, F, [&](fmcw_ctx* d, int g, int64_t f0, int64_t n) {
    return music_host_one(d, q, cov + f0 * covf, n, nr, w, shifted(eval, f0 * evf), shifted(evec, f0 * vecf),
                          shifted(nsrc, f0 * nr), shifted(music, f0 * muf), &mx[(size_t)g]);
  }));
  float gmx = 0.f;                             // a maximum of non-negative floats does not depend on order
  for (int g = 0; g < world; ++g) gmx = std::max(gmx, mx[(size_t)g]);
  if (music_max) *music_max = gmx;
  return FMCW_OK;
}

// ---------------------------------------------------------------------------
// Directions of arrival: per range row the peaks of its angular spectrum (kernels_doa.hip)
// ---------------------------------------------------------------------------
int fmcw_doa_check(const fmcw_doa_params* q, int32_t nr) {
  if (!q) return fail(FMCW_E_ARG, "doa params is NULL");
  CHK(check_rd_shape("doa", nr, 4));
  CHK(check_gate("doa", q->r_lo, q->r_hi, nr));
  if (q->n_ang < 1 || q->n_ang > fmcw::kRaAngMax) return fail(FMCW_E_ARG, "doa: n_ang must be in [1, 256]");
  if (q->max_pk < 1 || q->max_pk > fmcw::kDoaPkMax) return fail(FMCW_E_ARG, "doa: max_pk must be in [1, 8]");
  if (q->flags & ~(FMCW_DOA_EDGES | FMCW_DOA_WRAP | FMCW_DOA_INV)) return fail(FMCW_E_ARG, "doa: unknown flag bits");
  if ((q->flags & FMCW_DOA_EDGES) && (q->flags & FMCW_DOA_WRAP))
    return fail(FMCW_E_ARG, "doa: FMCW_DOA_EDGES and FMCW_DOA_WRAP exclude each other");
  if ((q->flags & FMCW_DOA_WRAP) && q->n_ang < 3) return fail(FMCW_E_ARG, "doa: FMCW_DOA_WRAP needs n_ang >= 3");
  if (!(std::isfinite(q->min_abs) && q->min_abs >= 0.f)) return fail(FMCW_E_ARG, "doa: min_abs must be finite and >= 0");
  if (!(q->min_rel >= 0.f && q->min_rel <= 1.f)) return fail(FMCW_E_ARG, "doa: min_rel must be in [0, 1]");
  if (!(std::isfinite(q->min_prom) && q->min_prom >= 0.f)) return fail(FMCW_E_ARG, "doa: min_prom must be finite and >= 0");
  return FMCW_OK;
}

static int doa_entry(fmcw_ctx* c, const fmcw_doa_params* q, int64_t F, int32_t nr) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(fmcw_doa_check(q, nr));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F > ((int64_t)1 << 40)) return fail(FMCW_E_ARG, "doa: F must be at most 2^40");
  return FMCW_OK;
}

int fmcw_doa_device(fmcw_ctx* c, const fmcw_doa_params* q, const float* d_spec, int64_t F, int32_t nr, const float* d_sin_theta,
                    int32_t* d_count, int32_t* d_idx, float* d_pow, float* d_sin, float* d_base, void* stream) {
  CHK(doa_entry(c, q, F, nr));
  if (!d_count && !d_idx && !d_pow && !d_sin && !d_base) return fail(FMCW_E_ARG, "doa: every output is NULL");
  if (F == 0) return FMCW_OK;
  if (!d_spec || !d_sin_theta) return fail(FMCW_E_ARG, "required pointer is NULL");
  if ((reinterpret_cast<uintptr_t>(d_spec) | reinterpret_cast<uintptr_t>(d_sin_theta) | reinterpret_cast<uintptr_t>(d_count) |
       reinterpret_cast<uintptr_t>(d_idx) | reinterpret_cast<uintptr_t>(d_pow) | reinterpret_cast<uintptr_t>(d_sin) |
       reinterpret_cast<uintptr_t>(d_base)) & 15)
    return fail(FMCW_E_ARG, "doa: d_spec, d_sin_theta, d_count, d_idx, d_pow, d_sin and d_base must be 16-byte aligned");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::DoaArgs a{};
  a.K = q->n_ang; a.NR = nr; a.max_pk = q->max_pk; a.flags = q->flags;
  gate_rows(q->r_lo, q->r_hi, nr, a.g0, a.g1);
  a.min_abs = q->min_abs; a.min_rel = q->min_rel; a.min_prom = q->min_prom;
  a.u = d_sin_theta;
  // at most kRaRowsMax rows per launch (the results do not depend on the cut)
  const int64_t Fc = fmcw::kRaRowsMax / nr;
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    a.rows = std::min(Fc, F - f0) * nr;
    const int64_t r0 = f0 * nr;
    a.spec = d_spec + r0 * a.K;
    a.count = shifted(d_count, r0);
    a.idx = shifted(d_idx, r0 * a.max_pk);
    a.pw = shifted(d_pow, r0 * a.max_pk);
    a.sn = shifted(d_sin, r0 * a.max_pk);
    a.base = shifted(d_base, r0 * a.max_pk);
    StageTimer tm(c, 19, s);
    HIPCHK(fmcw::launch_doa(a, s));
    tm.done();
  }
  return FMCW_OK;
}

// One shard of fmcw_doa, chunk by chunk: the chunk's spectra in, what was asked for out.
static int doa_host_one(fmcw_ctx* c, const fmcw_doa_params* q, const float* spec, int64_t F, int32_t nr, const float* u,
                        int32_t* count, int32_t* idx, float* pw, float* sn, float* base) {
  CHK(set_device(c));
  hipStream_t s = c->stream;
  const size_t K = (size_t)q->n_ang, P = (size_t)q->max_pk;
  const size_t specf = (size_t)nr * K, pkf = (size_t)nr * P;            // per frame
  const int64_t Fc = c->chunk_frames > 0 ? std::min<int64_t>(c->chunk_frames, F) : host_chunk(specf * 4, F);
  CHK(c->doa_spec.ensure((size_t)Fc * specf * 4));
  CHK(c->doa_u.ensure(K * 4));
  if (count) CHK(c->doa_count.ensure((size_t)Fc * nr * 4));
  if (idx) CHK(c->doa_idx.ensure((size_t)Fc * pkf * 4));
  if (pw) CHK(c->doa_pow.ensure((size_t)Fc * pkf * 4));
  if (sn) CHK(c->doa_sin.ensure((size_t)Fc * pkf * 4));
  if (base) CHK(c->doa_base.ensure((size_t)Fc * pkf * 4));
  HIPCHK(hipMemcpyAsync(c->doa_u.p, u, K * 4, hipMemcpyHostToDevice, s));
  for (int64_t f0 = 0; f0 < F; f0 += Fc) {
    const int64_t nf = std::min(Fc, F - f0);
    HIPCHK(hipMemcpyAsync(c->doa_spec.p, spec + (size_t)f0 * specf, (size_t)nf * specf * 4, hipMemcpyHostToDevice, s));
    CHK(fmcw_doa_device(c, q, c->doa_spec.as<float>(), nf, nr, c->doa_u.as<float>(), count ? c->doa_count.as<int32_t>() : nullptr,
                        idx ? c->doa_idx.as<int32_t>() : nullptr, pw ? c->doa_pow.as<float>() : nullptr,
                        sn ? c->doa_sin.as<float>() : nullptr, base ? c->doa_base.as<float>() : nullptr, s));
    if (count) HIPCHK(hipMemcpyAsync(count + (size_t)f0 * nr, c->doa_count.p, (size_t)nf * nr * 4, hipMemcpyDeviceToHost, s));
    if (idx) HIPCHK(hipMemcpyAsync(idx + (size_t)f0 * pkf, c->doa_idx.p, (size_t)nf * pkf * 4, hipMemcpyDeviceToHost, s));
    if (pw) HIPCHK(hipMemcpyAsync(pw + (size_t)f0 * pkf, c->doa_pow.p, (size_t)nf * pkf * 4, hipMemcpyDeviceToHost, s));
    if (sn) HIPCHK(hipMemcpyAsync(sn + (size_t)f0 * pkf, c->doa_sin.p, (size_t)nf * pkf * 4, hipMemcpyDeviceToHost, s));
    if (base) HIPCHK(hipMemcpyAsync(base + (size_t)f0 * pkf, c->doa_base.p, (size_t)nf * pkf * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));           // the chunk buffers are reused by the next chunk
  }
  return FMCW_OK;
}

int fmcw_doa(fmcw_ctx* c, const fmcw_doa_params* q, const float* spec, int64_t F, int32_t nr, const float* sin_theta,
             int32_t* count, int32_t* idx, float* pw, float* sn, float* base) {
  CHK(doa_entry(c, q, F, nr));
  if (!count && !idx && !pw && !sn && !base) return fail(FMCW_E_ARG, "doa: every output is NULL");
  if (F == 0) return FMCW_OK;
  if (!spec || !sin_theta) return fail(FMCW_E_ARG, "required pointer is NULL");
  const int64_t specf = (int64_t)nr * q->n_ang, pkf = (int64_t)nr * q->max_pk;
  // frames are independent: contiguous shards, each written in place
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    return doa_host_one(d, q, spec + f0 * specf, n, nr, sin_theta, shifted(count, f0 * nr), shifted(idx, f0 * pkf),
                        shifted(pw, f0 * pkf), shifted(sn, f0 * pkf), shifted(base, f0 * pkf));
  });
}

}  // extern "C"
