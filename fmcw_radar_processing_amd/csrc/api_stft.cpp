// api_stft.cpp -- the slow-time STFT and the spectrogram render of the libfmcw C-ABI
// (include/fmcw.h): the STFT size rules of :273/:276, the logspace/interp1 bin table of
// :293-299, max(P) at a large nfft (stft_coarse_max), and fmcw_stft / fmcw_stft_png over the
// devices of a context.
#include "api_internal.h"

#include <cmath>
#include <cstdio>
#include <cstring>

extern "C" {

static int check_stft_shape(int32_t wlen, int32_t noverlap, int32_t nfft) {
  if (wlen < 1 || wlen > 256) return fail(FMCW_E_ARG, "wlen must be in [1, 256]");
  if (noverlap < 0 || noverlap >= wlen) return fail(FMCW_E_ARG, "noverlap must be in [0, wlen)");
  if (nfft < wlen || (nfft % 2) != 0) return fail(FMCW_E_ARG, "nfft must be even and >= wlen");
  return FMCW_OK;
}

int fmcw_stft_power_device(fmcw_ctx* c, const float* d_slow, const int32_t* d_list, const int64_t* d_len,
                           int32_t pn, const float* d_halo, int32_t n_halo, const int64_t* d_halo_len,
                           const float* d_win, int32_t wlen,
                           int32_t noverlap, int32_t nfft, double fs, int64_t max_seg, float* d_P, float* d_pmax,
                           int64_t* d_nseg, void* stream) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(check_stft_shape(wlen, noverlap, nfft));
  if (pn < 1 || n_halo < 0 || max_seg < 0 || !(fs > 0)) return fail(FMCW_E_ARG, "bad pn / n_halo / max_seg / fs");
  if (!d_slow || !d_list || !d_len || !d_win || !d_pmax || !d_nseg || (n_halo > 0 && !d_halo))
    return fail(FMCW_E_ARG, "NULL device pointer");   // d_P may be NULL: max(P) only
  // the shard split of the slow-time signal (dist.py) starts every shard's segment grid at its own
  // sample 0 and takes wlen-1 samples of right halo: that is the global grid only for hop 1
  if (n_halo > 0 && wlen - noverlap != 1)
    return fail(FMCW_E_ARG, "a halo (sharded STFT) needs hop 1, i.e. noverlap = wlen - 1");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::StftArgs a{};
  a.slow_mag = d_slow; a.frame_list = d_list; a.len = d_len; a.pn = pn;
  a.halo = d_halo; a.n_halo = n_halo; a.halo_len = d_halo_len;
  a.win = d_win; a.wlen = wlen; a.hop = wlen - noverlap; a.nfft = nfft;
  a.inv_fs = (float)(1.0 / fs);
  a.max_seg = max_seg; a.P = d_P; a.pmax = d_pmax; a.nseg_out = d_nseg;
  StageTimer tm(c, 4, s);
  if (fmcw::stft_fast_path(wlen, a.hop)) {        // the reference's 20-tap window: W table + k_stft20
    int st = FMCW_OK;
    bool build = true;
    // the cached nfft-64 table only for the forms that tolerate a stale one; the table form (any other nfft,
    // an unaligned d_P, FMCW_STFT_MFMA=0) gets a table built from this call's window (stft_tab clears the key)
    const int mode = d_P ? 0 : 1;
    float2* tab = fmcw::stft_form(a, mode, nullptr) != fmcw::STFT_FORM_TABLE
                      ? c->stft_tab64(s, d_win, nfft, &build, &st)
                      : c->stft_tab(s, (size_t)(nfft / 2 + 1) * 20 * 8, &st);
    CHK(st);
    if (build) HIPCHK(fmcw::launch_stft_table(d_win, nfft, tab, s));
    // device API: d_P is the caller's [max_seg][nfft/2+1] (fmcw.h), the table this stream's
    HIPCHK(fmcw::launch_stft20(a, tab, mode, nullptr, s, max_seg * (int64_t)(nfft / 2 + 1),
                               (int64_t)(nfft / 2 + 1) * 20));
    CHK(c->stft_tab_done(s));
  } else {
    HIPCHK(fmcw::launch_stft_power(a, s));
  }
  tm.done();
  return FMCW_OK;
}

int fmcw_stft_db_direct_device(fmcw_ctx* c, const float* d_slow, const int32_t* d_list, const int64_t* d_len,
                               int32_t pn, const float* d_halo, int32_t n_halo, const int64_t* d_halo_len,
                               const float* d_win, int32_t wlen, int32_t noverlap, int32_t nfft, double fs,
                               int64_t max_seg, const float* d_pmax, float* d_out, void* stream) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(check_stft_shape(wlen, noverlap, nfft));
  if (pn < 1 || n_halo < 0 || max_seg < 0 || !(fs > 0)) return fail(FMCW_E_ARG, "bad pn / n_halo / max_seg / fs");
  if (!d_slow || !d_list || !d_len || !d_win || !d_pmax || !d_out || (n_halo > 0 && !d_halo))
    return fail(FMCW_E_ARG, "NULL device pointer");
  if (!fmcw::stft_fast_path(wlen, wlen - noverlap))
    return fail(FMCW_E_ARG, "the direct dB STFT needs the 20-tap window and hop <= 4");
  if (n_halo > 0 && wlen - noverlap != 1)
    return fail(FMCW_E_ARG, "a halo (sharded STFT) needs hop 1, i.e. noverlap = wlen - 1");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  fmcw::StftArgs a{};
  a.slow_mag = d_slow; a.frame_list = d_list; a.len = d_len; a.pn = pn;
  a.halo = d_halo; a.n_halo = n_halo; a.halo_len = d_halo_len;
  a.win = d_win; a.wlen = wlen; a.hop = wlen - noverlap; a.nfft = nfft;
  a.inv_fs = (float)(1.0 / fs);
  a.max_seg = max_seg; a.P = nullptr; a.pmax = const_cast<float*>(d_pmax); a.nseg_out = nullptr;
  StageTimer tm(c, 5, s);
  int st = FMCW_OK;
  bool build = true;
  // as fmcw_stft_power_device: an unaligned d_out takes the table form, which must not see a cached table
  float2* tab = fmcw::stft_form(a, 2, d_out) != fmcw::STFT_FORM_TABLE
                    ? c->stft_tab64(s, d_win, nfft, &build, &st)
                    : c->stft_tab(s, (size_t)(nfft / 2 + 1) * 20 * 8, &st);
  CHK(st);
  if (build) HIPCHK(fmcw::launch_stft_table(d_win, nfft, tab, s));
  HIPCHK(fmcw::launch_stft20(a, tab, 2, d_out, s, max_seg * (int64_t)(nfft / 2 + 1), (int64_t)(nfft / 2 + 1) * 20));
  CHK(c->stft_tab_done(s));
  tm.done();
  return FMCW_OK;
}

// logspace(log10(fs/nfft), log10(fs/2), n) located on F = (0:nfft/2)*fs/nfft
static void log_table(int nfft, double fs, int n, std::vector<int32_t>& idx, std::vector<float>& wt,
                      std::vector<double>* fq_out) {
  const int nb = nfft / 2 + 1;
  const double df = fs / nfft;
  const double a = std::log10(df), b = std::log10((nb - 1) * df);
  idx.resize(n);
  wt.resize(n);
  if (fq_out) fq_out->resize(n);
  for (int j = 0; j < n; ++j) {
    const double e = (n == 1) ? b : (j == n - 1 ? b : a + j * (b - a) / (n - 1));
    const double fq = std::pow(10.0, e);
    int i0 = (int)std::floor(fq / df);
    if (i0 < 0) i0 = 0;
    if (i0 > nb - 2) i0 = nb - 2;
    idx[j] = i0;
    wt[j] = (float)((fq - i0 * df) / df);
    if (fq_out) (*fq_out)[j] = fq;
  }
}

int fmcw_stft_db_device(fmcw_ctx* c, const float* d_P, const int64_t* d_nseg, int64_t max_seg, int32_t nfft,
                        double fs, const float* d_pmax, int32_t n_log_bins, float* d_out, void* stream) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (nfft < 2 || (nfft % 2) != 0 || n_log_bins < 0 || max_seg < 0 || !(fs > 0))
    return fail(FMCW_E_ARG, "bad nfft / n_log_bins / max_seg / fs");
  if (!d_P || !d_nseg || !d_pmax || !d_out) return fail(FMCW_E_ARG, "NULL device pointer");
  if (n_log_bins > 0 && d_out == d_P) return fail(FMCW_E_ARG, "d_out may alias d_P only without resampling");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  if (n_log_bins > 0) {
    std::vector<int32_t> idx;
    std::vector<float> wt;
    log_table(nfft, fs, n_log_bins, idx, wt, nullptr);
    CHK(c->s_lidx.ensure(idx.size() * 4));
    CHK(c->s_lw.ensure(wt.size() * 4));
    HIPCHK(hipMemcpyAsync(c->s_lidx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->s_lw.p, wt.data(), wt.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // host vectors go out of scope
  }
  fmcw::StftDbArgs a{};
  a.P = d_P; a.nseg = d_nseg; a.max_seg = max_seg; a.nbins_in = nfft / 2 + 1;
  a.pmax = d_pmax; a.nlog = n_log_bins;
  a.lidx = n_log_bins > 0 ? c->s_lidx.as<int32_t>() : nullptr;
  a.lw = n_log_bins > 0 ? c->s_lw.as<float>() : nullptr;
  a.out = d_out;
  StageTimer tm(c, 5, s);
  HIPCHK(fmcw::launch_stft_db(a, s));
  tm.done();
  return FMCW_OK;
}

int fmcw_stft_sizes(int64_t L, int32_t wlen, int32_t noverlap, int32_t nfft, int32_t n_log_bins, int64_t* nseg,
                    int32_t* nfft_used, int32_t* nbins_out) {
  if (L < 0 || n_log_bins < 0) return fail(FMCW_E_ARG, "L < 0 or n_log_bins < 0");
  int32_t nf = nfft;
  if (nf == 0) {                       // :273 nfft_stft = 2^nextpow2(length(iq_data(:)))
    int64_t v = 1;
    while (v < L) v <<= 1;
    if (v > (1 << 26)) return fail(FMCW_E_ARG, "2^nextpow2(L) too large");
    nf = (int32_t)v;
  }
  if (wlen < 1 || noverlap < 0 || noverlap >= wlen) return fail(FMCW_E_ARG, "need 0 <= noverlap < wlen");
  const int hop = wlen - noverlap;
  const int64_t ns = (L - noverlap) >= 0 ? (L - noverlap) / hop : 0;   // fix((nx-noverlap)/(nwind-noverlap))
  if (nseg) *nseg = ns;
  if (nfft_used) *nfft_used = nf;
  if (nbins_out) *nbins_out = n_log_bins > 0 ? n_log_bins : nf / 2 + 1;
  if (ns < 1) return fail(FMCW_E_DATA, "spectrogram: signal length " + std::to_string(L) + " is shorter than the window");
  CHK(check_stft_shape(wlen, noverlap, nf));
  return FMCW_OK;
}

int fmcw_render_spectrogram_device(fmcw_ctx* c, const float* d_Q, int32_t nq, const int64_t* d_nseg,
                                   const float* d_pmax, int32_t nfft, double fs, double t0, double dt, int32_t width,
                                   int32_t height, uint8_t* d_img, void* stream) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (!d_Q || !d_nseg || !d_pmax || !d_img) return fail(FMCW_E_ARG, "NULL device pointer");
  if (nfft < 2 || (nfft % 2) != 0 || nq < 1 || nq > nfft / 2 || !(fs > 0) || !(dt > 0))
    return fail(FMCW_E_ARG, "bad nfft / nq / fs / dt");
  if (width < 1 || height < 1 || width > 65536 || height > 65535) return fail(FMCW_E_ARG, "bad image size");
  CHK(set_device(c));
  fmcw::RenderArgs a{};
  a.Q = d_Q; a.nq = nq; a.nseg = d_nseg; a.pmax = d_pmax;
  a.nb = nfft / 2 + 1; a.nfft = nfft; a.seam = a.nb - a.nb / 2 - 1;
  a.fs = fs; a.t0 = t0; a.dt = dt;
  a.fmax = FMCW_PNG_FMAX_HZ; a.cmin = FMCW_PNG_CMIN_DB; a.cmax = FMCW_PNG_CMAX_DB;
  a.W = width; a.H = height; a.img = d_img;
  hipStream_t s = pick(c, stream);
  StageTimer tm(c, 9, s);
  HIPCHK(fmcw::launch_render(a, s));
  tm.done();
  return FMCW_OK;
}

// A large device -> pageable-host copy on stream s, through the two pinned out slots of the
// context: the DMA of piece i overlaps the host threads copying piece i-1 to the caller (and
// taking its first-touch page faults in parallel). Returns once dst holds every byte.
static int d2h_big(fmcw_ctx* c, void* dst, const void* d_src, size_t bytes, hipStream_t s) {
  constexpr size_t kPiece = 32u << 20;
  if (bytes < 2 * kPiece) {
    HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return FMCW_OK;
  }
  CHK(c->pin_out.ensure(2 * kPiece));
  const size_t n = (bytes + kPiece - 1) / kPiece;
  auto piece = [&](size_t i) { return std::min(kPiece, bytes - i * kPiece); };
  for (size_t i = 0; i <= n; ++i) {
    if (i < n) {
      const int b = (int)(i & 1);
      HIPCHK(hipMemcpyAsync(c->pin_out.at(b * kPiece), static_cast<const char*>(d_src) + i * kPiece, piece(i),
                            hipMemcpyDeviceToHost, s));
      HIPCHK(hipEventRecord(c->ev_d2h[b], s));
    }
    if (i >= 1) {   // piece i-1 is in its pinned slot once its event fires; slot (i-1)&1 is reused by piece i+1
      const int b = (int)((i - 1) & 1);
      HIPCHK(hipEventSynchronize(c->ev_d2h[b]));
      par_memcpy(static_cast<char*>(dst) + (i - 1) * kPiece, c->pin_out.at(b * kPiece), piece(i - 1));
    }
  }
  return FMCW_OK;
}

// max(P) of :282-283 over every bin of a large nfft without evaluating every bin of every segment.
// |X_s(w)| of a 20-tap segment is a trigonometric polynomial of degree 19, so (Bernstein) within one
// coarse step h = 2 pi / K of its peak it is at least (1 - 19 h) of the peak.  Pass 1 takes each
// segment's max over the coarse bins k = m nfft / K (exact P values of the fine grid, so their
// maximum G is a lower bound of max(P)); a segment whose coarse max is below G (1 - 19 h)^2 cannot
// hold max(P).  Pass 2 takes the max over every bin of the 256-segment tiles that hold a
// candidate: the same P values the full pass would compare, so the result is the same bits.
static int stft_coarse_max(fmcw_ctx* d, const fmcw::StftArgs& a0, hipStream_t s) {
  // The bound below holds for the 20-tap window only (a degree-19 trigonometric polynomial per
  // segment; any sign of the samples) and for a power-of-two nfft of at least 2^16, so that the
  // coarse grid (every D-th bin) holds DC, Nyquist and an interior bin within h of any peak.
  if (!fmcw::stft_fast_path(a0.wlen, a0.hop)) return fail(FMCW_E_ARG, "stft_coarse_max: not the 20-tap fast path");
  if (a0.nfft < (1 << 16) || (a0.nfft & (a0.nfft - 1))) return fail(FMCW_E_ARG, "stft_coarse_max: nfft must be a power of two >= 2^16");
  const int nf = a0.nfft, K = std::min(16384, nf / 8), D = nf / K, nc = K / 2 + 1;   // nf >= 2^16
  const int64_t ns = a0.max_seg;
  if (ns < 1 || ns > 0x7fffffffLL) return fail(FMCW_E_ARG, "stft_coarse_max: bad segment count");
  std::vector<int32_t> cb(nc);
  for (int m = 0; m < nc; ++m) cb[m] = D * m;
  CHK(d->s_cbins.ensure((size_t)nc * 4));
  CHK(d->s_segmax.ensure((size_t)ns * 4));
  int st = FMCW_OK;
  float2* tab = d->stft_tab(s, (size_t)(nf / 2 + 1) * 20 * 8, &st);
  CHK(st);
  HIPCHK(hipMemcpyAsync(d->s_cbins.p, cb.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
  HIPCHK(fmcw::launch_stft_table(a0.win, nf, tab, s));
  fmcw::StftArgs a = a0;
  a.bins = d->s_cbins.as<int32_t>();
  a.ncol = nc;
  // mode 4 writes one float per segment: s_segmax holds ns (launch_stft20 checks the capacity)
  HIPCHK(fmcw::launch_stft20(a, tab, 4, d->s_segmax.as<float>(), s, (int64_t)(d->s_segmax.n / 4),
                             (int64_t)(nf / 2 + 1) * 20));
  std::vector<float> sm((size_t)ns);
  HIPCHK(hipMemcpyAsync(sm.data(), d->s_segmax.p, (size_t)ns * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float G = 0.f;
  for (float v : sm) G = std::max(G, v);
  const double f = 1.0 - (double)(a0.wlen - 1) * 2.0 * M_PI / K;   // degree wlen - 1 (the 20-tap fast path)
  const float thr = (float)((double)G * f * f * (1.0 - 1e-3));   // margin for the fp32 rounding of P
  std::vector<int32_t> tiles;
  for (int64_t t = 0; t * 256 < ns; ++t) {
    const int64_t e = std::min<int64_t>(ns, (t + 1) * 256);
    for (int64_t i = t * 256; i < e; ++i)
      if (sm[(size_t)i] >= thr) { tiles.push_back((int32_t)t); break; }
  }
  CHK(d->s_tiles.ensure(tiles.size() * 4));
  HIPCHK(hipMemcpyAsync(d->s_tiles.p, tiles.data(), tiles.size() * 4, hipMemcpyHostToDevice, s));
  a = a0;
  a.tiles = d->s_tiles.as<int32_t>();
  a.ntiles = (int)tiles.size();
  HIPCHK(fmcw::launch_stft20(a, tab, 1, nullptr, s, 0, (int64_t)(nf / 2 + 1) * 20));
  CHK(d->stft_tab_done(s));
  HIPCHK(hipStreamSynchronize(s));   // tiles / cb leave scope
  d->last_coarse_tiles = (int64_t)tiles.size();
  if (const char* e = std::getenv("FMCW_STFT_DEBUG"); e && e[0] == '1')
    std::fprintf(stderr, "stft_coarse_max: nfft %d, %lld segments, %zu of %lld tiles in full\n", nf, (long long)ns,
                 tiles.size(), (long long)((ns + 255) / 256));
  return FMCW_OK;
}

static int stft_impl(fmcw_ctx* c, const float* x, int64_t L, const float* win, int32_t wlen, int32_t noverlap,
                     int32_t nfft, double fs, int32_t n_log_bins, float* T, float* freq, float* intensity,
                     const char* png_path, int32_t width, int32_t height, int64_t* png_bytes) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if ((!x && L > 0) || !win || !T || !freq || !intensity) return fail(FMCW_E_ARG, "NULL pointer");
  if (!(fs > 0)) return fail(FMCW_E_ARG, "fs must be > 0");
  if (L > 0x7fffffffLL) return fail(FMCW_E_ARG, "L too large for the host API");
  int64_t nseg = 0;
  int32_t nf = 0, nbo = 0;
  CHK(fmcw_stft_sizes(L, wlen, noverlap, nfft, n_log_bins, &nseg, &nf, &nbo));   // nfft rule on the whole signal
  const int hop = wlen - noverlap;
  const int nb = nf / 2 + 1;
  const int world = 1 + (int)c->peers.size();
  auto dev = [&](int g) { return g == 0 ? c : c->peers[g - 1]; };
  const double df = fs / nf;
  const int nq = png_path ? (int)std::min<int64_t>(nb - 1, (int64_t)std::floor(FMCW_PNG_FMAX_HZ / df) + 2) : 0;
  // With the log-frequency output (:286-299) and the 20-tap window, P is formed only for the
  // bins interp1 and the picture read: a max(P)-only pass over every bin, then those columns
  // ([seg][ncolP], ascending bins). Otherwise every bin ([seg][nb]).
  const bool sel_mode = n_log_bins > 0 && fmcw::stft_fast_path(wlen, hop);
  std::vector<int32_t> bins, lidx;
  std::vector<float> lw;
  if (sel_mode) {
    log_table(nf, fs, n_log_bins, lidx, lw, nullptr);
    std::vector<int32_t> pos(nb, 0);
    for (int32_t i0 : lidx) pos[i0] = pos[i0 + 1] = 1;
    for (int k = 0; k < nq; ++k) pos[k] = 1;
    if (png_path) pos[nb - 1] = 1;
    for (int k = 0; k < nb; ++k)
      if (pos[k]) { pos[k] = (int32_t)bins.size(); bins.push_back(k); }
    for (auto& i0 : lidx) i0 = pos[i0];   // i0 and i0+1 are both listed, so they are adjacent columns
  }
  const int ncolP = sel_mode ? (int)bins.size() : nb;
  // per device, the call's inputs (its samples, the one-entry frame list, the length, the window,
  // the listed bins and the interp1 table) in one arena: one pinned H2D copy instead of seven
  struct InOff { size_t x, list, len, win, bins, lidx, lw; };
  std::vector<InOff> io(world);
  // Segments are sharded contiguously over the devices; device g takes the
  // samples its segments cover (its halo is simply the next samples of x).
  // 1) P and the local max(P) per device
  for (int g = 0; g < world; ++g) {
    fmcw_ctx* d = dev(g);
    int64_t s0, ns;
    shard(nseg, g, world, s0, ns);
    CHK(set_device(d));
    hipStream_t s = d->stream;
    const int64_t Ld = ns > 0 ? (ns - 1) * hop + wlen : 0;
    CHK(d->s_P.ensure((size_t)std::max<int64_t>(ns, 1) * ncolP * 4));
    CHK(d->s_pmax.ensure(4));
    CHK(d->s_nseg.ensure(8));
    CHK(d->s_out.ensure((size_t)std::max<int64_t>(ns, 1) * nbo * 4));
    HIPCHK(hipMemsetAsync(d->s_pmax.p, 0, 4, s));
    if (ns == 0) continue;
    Arena ar;
    InOff& o = io[g];
    o.x = ar.add((size_t)Ld * 4); o.list = ar.add(4); o.len = ar.add(8); o.win = ar.add((size_t)wlen * 4);
    o.bins = ar.add(bins.size() * 4); o.lidx = ar.add(lidx.size() * 4); o.lw = ar.add(lw.size() * 4);
    CHK(d->s_in.ensure(ar.off));
    CHK(d->pin_sin.ensure(ar.off));
    {
      char* h = d->pin_sin.at(0);
      par_memcpy(h + o.x, x + s0 * hop, (size_t)Ld * 4);
      const int32_t zero = 0;
      std::memcpy(h + o.list, &zero, 4);
      std::memcpy(h + o.len, &Ld, 8);
      std::memcpy(h + o.win, win, (size_t)wlen * 4);
      if (!bins.empty()) std::memcpy(h + o.bins, bins.data(), bins.size() * 4);
      if (!lidx.empty()) std::memcpy(h + o.lidx, lidx.data(), lidx.size() * 4);
      if (!lw.empty()) std::memcpy(h + o.lw, lw.data(), lw.size() * 4);
    }
    HIPCHK(hipMemcpyAsync(d->s_in.p, d->pin_sin.p, ar.off, hipMemcpyHostToDevice, s));
    char* const di = d->s_in.as<char>();
    float* const d_x = reinterpret_cast<float*>(di + o.x);
    int32_t* const d_list = reinterpret_cast<int32_t*>(di + o.list);
    int64_t* const d_len = reinterpret_cast<int64_t*>(di + o.len);
    float* const d_win = reinterpret_cast<float*>(di + o.win);
    // the shard's samples are one "frame" of Ld samples in the compaction indirection
    const char* ce = std::getenv("FMCW_STFT_COARSE");   // 0: every bin of every segment (tests, A/B)
    const char* me = std::getenv("FMCW_STFT_MFMA");
    const bool coarse_ok = !(ce && ce[0] == '0') && !(me && me[0] == '0');
    if (sel_mode && coarse_ok && nf >= (1 << 16)) {   // max(P) only, over a large nfft: coarse-to-fine
      fmcw::StftArgs a{};
      a.slow_mag = d_x; a.frame_list = d_list; a.len = d_len; a.pn = (int32_t)Ld;
      a.win = d_win; a.wlen = wlen; a.hop = hop; a.nfft = nf; a.inv_fs = (float)(1.0 / fs);
      a.max_seg = ns; a.P = nullptr; a.pmax = d->s_pmax.as<float>(); a.nseg_out = d->s_nseg.as<int64_t>();
      StageTimer tm(d, 4, s);
      CHK(stft_coarse_max(d, a, s));
      tm.done();
    } else if (sel_mode) {   // max(P) only, in the table form the listed-bins pass below uses (at nfft 64
                             // too: P / max(P) of the listed bins then peaks at exactly 0 dB, as in MATLAB)
      fmcw::StftArgs a{};
      a.slow_mag = d_x; a.frame_list = d_list; a.len = d_len; a.pn = (int32_t)Ld;
      a.win = d_win; a.wlen = wlen; a.hop = hop; a.nfft = nf; a.inv_fs = (float)(1.0 / fs);
      a.max_seg = ns; a.P = nullptr; a.pmax = d->s_pmax.as<float>(); a.nseg_out = d->s_nseg.as<int64_t>();
      a.table_form = 1;
      StageTimer tm(d, 4, s);
      int st = FMCW_OK;
      float2* tab = d->stft_tab(s, (size_t)(nf / 2 + 1) * 20 * 8, &st);
      CHK(st);
      HIPCHK(fmcw::launch_stft_table(d_win, nf, tab, s));
      HIPCHK(fmcw::launch_stft20(a, tab, 1, nullptr, s, 0, (int64_t)(nf / 2 + 1) * 20));
      CHK(d->stft_tab_done(s));
      tm.done();
    } else {
      CHK(fmcw_stft_power_device(d, d_x, d_list, d_len, (int32_t)Ld, nullptr, 0, nullptr, d_win, wlen, noverlap, nf, fs, ns,
                                 d->s_P.as<float>(), d->s_pmax.as<float>(), d->s_nseg.as<int64_t>(), s));
    }
    if (sel_mode) {   // second pass: P of the listed bins (the W table the first pass built on s is reused)
      fmcw::StftArgs a{};
      a.slow_mag = d_x; a.frame_list = d_list; a.len = d_len;
      a.pn = (int32_t)Ld; a.win = d_win; a.wlen = wlen; a.hop = hop; a.nfft = nf;
      a.inv_fs = (float)(1.0 / fs); a.max_seg = ns; a.bins = reinterpret_cast<int32_t*>(di + o.bins); a.ncol = ncolP;
      StageTimer tm(d, 4, s);
      int st = FMCW_OK;
      float2* tab = d->stft_tab(s, (size_t)(nf / 2 + 1) * 20 * 8, &st);   // the first pass's table on s (both
      CHK(st);                                                             // first-pass forms built it for d_win)
      HIPCHK(fmcw::launch_stft20(a, tab, 3, d->s_P.as<float>(), s, (int64_t)(d->s_P.n / 4), (int64_t)(nf / 2 + 1) * 20));
      CHK(d->stft_tab_done(s));
      tm.done();
    }
    if (world > 1) HIPCHK(hipStreamSynchronize(s));   // local max(P) final (step 2 may read it through the host)
  }
  // 2) the global max(P) of :282-283: RCCL all_reduce(max) across the devices
  if (world > 1) {
    if (!c->comms.empty()) {
      NCCLCHK(rccl().group_start());
      for (int g = 0; g < world; ++g) {
        fmcw_ctx* d = dev(g);
        CHK(set_device(d));
        NCCLCHK(rccl().all_reduce(d->s_pmax.p, d->s_pmax.p, 1, ncclFloat32, ncclMax, c->comms[g], d->stream));
      }
      NCCLCHK(rccl().group_end());
    } else {   // several contexts on ONE device (no communicator can span them): 4 bytes through the host
      float m = 0.f;
      for (int g = 0; g < world; ++g) {
        float v = 0.f;
        CHK(set_device(dev(g)));
        HIPCHK(hipMemcpy(&v, dev(g)->s_pmax.p, 4, hipMemcpyDeviceToHost));
        m = std::max(m, v);
      }
      for (int g = 0; g < world; ++g) {
        CHK(set_device(dev(g)));
        HIPCHK(hipMemcpy(dev(g)->s_pmax.p, &m, 4, hipMemcpyHostToDevice));
      }
    }
  }
  // 2b) spectrogram.png (:331-348) from the linear-bin P before it is overwritten:
  //     the bins below ylim plus the Nyquist bin of every segment, gathered to device 0
  std::vector<uint8_t> img;
  if (png_path) {
    std::vector<float> q((size_t)std::max<int64_t>(nseg, 1) * (nq + 1));
    for (int g = 0; g < world; ++g) {
      fmcw_ctx* d = dev(g);
      int64_t s0, ns;
      shard(nseg, g, world, s0, ns);
      if (ns == 0) continue;
      CHK(set_device(d));
      // bins 0..nq-1 are the first nq columns of P and the Nyquist bin its last, in both layouts
      HIPCHK(hipMemcpy2DAsync(q.data() + s0 * (nq + 1), (nq + 1) * 4, d->s_P.p, (size_t)ncolP * 4, (size_t)nq * 4, ns,
                              hipMemcpyDeviceToHost, d->stream));
      HIPCHK(hipMemcpy2DAsync(q.data() + s0 * (nq + 1) + nq, (nq + 1) * 4, d->s_P.as<float>() + (ncolP - 1),
                              (size_t)ncolP * 4, 4, ns, hipMemcpyDeviceToHost, d->stream));
    }
    for (int g = 0; g < world; ++g) {
      CHK(set_device(dev(g)));
      HIPCHK(hipStreamSynchronize(dev(g)->stream));
    }
    CHK(set_device(c));
    hipStream_t s = c->stream;
    CHK(c->r_q.ensure(q.size() * 4));
    CHK(c->r_nseg.ensure(8));
    CHK(c->r_img.ensure((size_t)height * (width + 1)));
    HIPCHK(hipMemcpyAsync(c->r_q.p, q.data(), q.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->r_nseg.p, &nseg, 8, hipMemcpyHostToDevice, s));
    CHK(fmcw_render_spectrogram_device(c, c->r_q.as<float>(), nq, c->r_nseg.as<int64_t>(), c->s_pmax.as<float>(), nf, fs,
                                       (wlen / 2.0) / fs, hop / fs, width, height, c->r_img.as<uint8_t>(), s));
    img.resize((size_t)height * (width + 1));
    HIPCHK(hipMemcpyAsync(img.data(), c->r_img.p, img.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  // 3) dB (+ log-frequency resampling) and the rows back into intensity
  for (int g = 0; g < world; ++g) {
    fmcw_ctx* d = dev(g);
    int64_t s0, ns;
    shard(nseg, g, world, s0, ns);
    if (ns == 0) continue;
    CHK(set_device(d));
    hipStream_t s = d->stream;
    if (sel_mode) {   // interp1 over the listed columns (lidx holds column positions; uploaded in step 1)
      fmcw::StftDbArgs a{};
      a.P = d->s_P.as<float>(); a.nseg = d->s_nseg.as<int64_t>(); a.max_seg = ns; a.nbins_in = ncolP;
      a.pmax = d->s_pmax.as<float>(); a.nlog = n_log_bins;
      a.lidx = reinterpret_cast<int32_t*>(d->s_in.as<char>() + io[g].lidx);
      a.lw = reinterpret_cast<float*>(d->s_in.as<char>() + io[g].lw); a.out = d->s_out.as<float>();
      StageTimer tm(d, 5, s);
      HIPCHK(fmcw::launch_stft_db(a, s));
      tm.done();
    } else {
      CHK(fmcw_stft_db_device(d, d->s_P.as<float>(), d->s_nseg.as<int64_t>(), ns, nf, fs, d->s_pmax.as<float>(),
                              n_log_bins, n_log_bins > 0 ? d->s_out.as<float>() : d->s_P.as<float>(), s));
    }
    const float* res = n_log_bins > 0 ? d->s_out.as<float>() : d->s_P.as<float>();
    CHK(d2h_big(d, intensity + s0 * nbo, res, (size_t)ns * nbo * 4, s));
  }
  for (int g = 0; g < world; ++g) {
    CHK(set_device(dev(g)));
    HIPCHK(hipStreamSynchronize(dev(g)->stream));
  }
  if (png_path) CHK(fmcw::png_write_indexed(png_path, img.data(), width, height, 1, 0, png_bytes));
  for (int64_t i = 0; i < nseg; ++i) T[i] = (float)(((double)i * hop + wlen / 2.0) / fs);   // spectrogram T
  if (n_log_bins > 0) {
    std::vector<int32_t> idx;
    std::vector<float> wt;
    std::vector<double> fq;
    log_table(nf, fs, n_log_bins, idx, wt, &fq);
    for (int j = 0; j < n_log_bins; ++j) freq[j] = (float)fq[j];
  } else {
    for (int j = 0; j < nb; ++j) freq[j] = (float)(j * fs / nf);
  }
  return FMCW_OK;
}

int fmcw_stft(fmcw_ctx* c, const float* x, int64_t L, const float* win, int32_t wlen, int32_t noverlap, int32_t nfft,
              double fs, int32_t n_log_bins, float* T, float* freq, float* intensity) {
  return stft_impl(c, x, L, win, wlen, noverlap, nfft, fs, n_log_bins, T, freq, intensity, nullptr, 0, 0, nullptr);
}

int fmcw_stft_png(fmcw_ctx* c, const float* x, int64_t L, const float* win, int32_t wlen, int32_t noverlap,
                  int32_t nfft, double fs, int32_t n_log_bins, float* T, float* freq, float* intensity,
                  const char* png_path, int32_t width, int32_t height, int64_t* png_bytes) {
  if (!png_path) return fail(FMCW_E_ARG, "png_path is NULL");
  return stft_impl(c, x, L, win, wlen, noverlap, nfft, fs, n_log_bins, T, freq, intensity, png_path,
                   width > 0 ? width : FMCW_PNG_DEFAULT_W, height > 0 ? height : FMCW_PNG_DEFAULT_H, png_bytes);
}

}  // extern "C"
