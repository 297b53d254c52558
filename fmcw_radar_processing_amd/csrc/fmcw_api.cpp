// fmcw_api.cpp -- libfmcw C-ABI (include/fmcw.h) on top of the gfx950 kernels: the context
// and the per-frame pipeline.  The STFT and render path is api_stft.cpp, the RD-map stages
// (CFAR, signatures, clustering, tracking, MTI, beams) are api_stages.cpp; api_internal.h holds what
// the three share.
//
// Host responsibilities kept here, mirroring what radar_processing.m does
// around the loop: argument validation (MATLAB would raise), twiddle tables,
// scratch management for the per-chunk range cube and the chunked launch
// sequence K1 -> K2 -> K3.
#include "api_internal.h"
#include "xcd_ctr_plan.h"

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>

namespace {
thread_local std::string g_err;   // the library's one error text (fmcw_last_error)
}  // namespace

namespace fmcw {

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int set_error(int code, const char* msg) { return fail(code, msg); }

// one core copies ~10 GB/s, PCIe Gen5 x16 takes ~50
void par_memcpy(void* dst, const void* src, size_t n) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const unsigned T = n >= (8u << 20) ? std::min(8u, hw) : 1u;
  if (T == 1) {
    std::memcpy(dst, src, n);
    return;
  }
  const size_t per = ((n + T - 1) / T + 4095) & ~(size_t)4095;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; ++t) {
    const size_t o = (size_t)t * per;
    if (o >= n) break;
    th.emplace_back([=] { std::memcpy(static_cast<char*>(dst) + o, static_cast<const char*>(src) + o, std::min(per, n - o)); });
  }
  for (auto& x : th) x.join();
}

const Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
      if (h) break;
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return x;
    x.comm_init_all = reinterpret_cast<decltype(x.comm_init_all)>(dlsym(h, "ncclCommInitAll"));
    x.comm_destroy = reinterpret_cast<decltype(x.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
    x.all_reduce = reinterpret_cast<decltype(x.all_reduce)>(dlsym(h, "ncclAllReduce"));
    x.group_start = reinterpret_cast<decltype(x.group_start)>(dlsym(h, "ncclGroupStart"));
    x.group_end = reinterpret_cast<decltype(x.group_end)>(dlsym(h, "ncclGroupEnd"));
    x.error_string = reinterpret_cast<decltype(x.error_string)>(dlsym(h, "ncclGetErrorString"));
    x.ok = x.comm_init_all && x.comm_destroy && x.all_reduce && x.group_start && x.group_end && x.error_string;
    return x;
  }();
  return r;
}

}  // namespace fmcw

fmcw_ctx::~fmcw_ctx() {
  for (ncclComm_t m : comms) (void)rccl().comm_destroy(m);
  for (fmcw_ctx* q : peers) delete q;
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  for (auto& pd : pending) { (void)hipEventDestroy(pd.a); (void)hipEventDestroy(pd.b); }
  for (auto e : pool) (void)hipEventDestroy(e);
  for (int i = 0; i < kSlots; ++i)
    for (hipEvent_t e : {ev_k1[i], ev_k2[i], ev_k3[i]})
      if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {ev_fork, ev_join, ev_h2d[0], ev_h2d[1], ev_comp[0], ev_comp[1], ev_d2h[0], ev_d2h[1]})
    if (e) (void)hipEventDestroy(e);
  for (hipStream_t x : {sd, sx, cin, cout})
    if (x) { (void)hipStreamSynchronize(x); (void)hipStreamDestroy(x); }
  if (stream) (void)hipStreamDestroy(stream);
}

// a table the caller rewrites (any nfft): the entry no longer holds what a cached nfft-64 key
// says it holds, so the key is cleared (a later stft_tab64 with the same window rebuilds)
float2* fmcw_ctx::stft_tab(hipStream_t st, size_t bytes, int* status) {
  float2* t = static_cast<float2*>(s_tabs.get(st, bytes + STFT_TAPS_BYTES, status));
  if (t) {
    s_tabs.last->key = nullptr;
    s_tabs.last->key_n = 0;
  }
  return t;
}

// The device calls at nfft 64 (the bench's config-4 STFT, two passes per step) keep the
// stream's table while the window pointer and nfft are unchanged: k_stft64m compares the 20
// taps stored behind the table with the call's window and forms its W entries itself when they
// differ (a window rewritten in place), so the table is rebuilt once, not every pass.
// *build: the caller must launch k_stft_table into the returned table.
float2* fmcw_ctx::stft_tab64(hipStream_t st, const float* d_win, int nfft, bool* build, int* status) {
  float2* t = static_cast<float2*>(s_tabs.get(st, (size_t)(nfft / 2 + 1) * 20 * 8 + STFT_TAPS_BYTES, status));
  if (!t) return nullptr;
  PerStream::Entry* e = s_tabs.last;
  *build = !(e->key == d_win && e->key_n == nfft);
  e->key = d_win;
  e->key_n = nfft;
  return t;
}

namespace {

int check_params(const fmcw_params* p) {
  if (!p) return fail(FMCW_E_ARG, "params is NULL");
  if (p->nts < 1 || p->nts > 65536) return fail(FMCW_E_ARG, "nts out of range [1, 65536]");
  if (p->pn < 1 || p->pn > 65536) return fail(FMCW_E_ARG, "pn out of range [1, 65536]");
  if (!fmcw::range_size_supported(p->nr)) return fail(FMCW_E_ARG, "nr must be a power of two in [16, 2048]");
  if (!fmcw::doppler_size_supported(p->nd)) return fail(FMCW_E_ARG, "nd must be a power of two in [2, 1024]");
  if (p->max_targets < 1 || p->max_targets > 8) return fail(FMCW_E_ARG, "max_targets must be in [1, 8]");
  if (!(p->dist_per_bin > 0.f)) return fail(FMCW_E_ARG, "dist_per_bin must be > 0");
  return FMCW_OK;
}

// {cal.re, cal.im, IF_scale*w, w} per sample: one 16-byte load per sample in K1
int build_calw(fmcw_ctx* c, float if_scale, hipStream_t s) {
  const size_t n = c->h_wr.size();
  std::vector<float> t(4 * n);
  for (size_t i = 0; i < n; ++i) {
    t[4 * i] = c->h_cal[2 * i];
    t[4 * i + 1] = c->h_cal[2 * i + 1];
    t[4 * i + 2] = (float)((double)if_scale * c->h_wr[i]);
    t[4 * i + 3] = c->h_wr[i];
  }
  CHK(c->calw.ensure(t.size() * 4));
  HIPCHK(hipMemcpyAsync(c->calw.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  c->calw_scale = if_scale;
  return FMCW_OK;
}

int check_ctx(fmcw_ctx* c, const fmcw_params* p) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(check_params(p));
  if (!c->taps) return fail(FMCW_E_STATE, "fmcw_set_taps has not been called");
  if (p->nts != c->p.nts || p->pn != c->p.pn || p->nr != c->p.nr || p->nd != c->p.nd)
    return fail(FMCW_E_STATE, "nts/pn/nr/nd differ from the ones given to fmcw_set_taps");
  CHK(set_device(c));
  if (p->if_scale != c->calw_scale) {   // queued work on any stream may still read the old table
    HIPCHK(hipDeviceSynchronize());
    CHK(build_calw(c, p->if_scale, c->stream));
  }
  return FMCW_OK;
}

int upload_twiddles(DevBuf& buf, int n, hipStream_t s) {
  std::vector<float> tw(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const double a = -2.0 * M_PI * (double)i / (double)n;
    tw[2 * i] = (float)std::cos(a);
    tw[2 * i + 1] = (float)std::sin(a);
  }
  CHK(buf.ensure(tw.size() * sizeof(float)));
  HIPCHK(hipMemcpyAsync(buf.p, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return FMCW_OK;
}

int64_t default_chunk(const fmcw_params* p) {
  // The range cube of one chunk is the only intermediate.  Measured on MI355X
  // (tools/mall_probe.hip): re-reading a freshly written buffer is no faster
  // from the Infinity Cache than from HBM, so the chunk is sized for launch
  // efficiency (long kernels, few boundaries): 256 MiB per slot, 3 slots.
  const int64_t per_frame = (int64_t)p->pn * p->nr * 8;
  int64_t c = (256ll << 20) / std::max<int64_t>(per_frame, 1);
  return std::max<int64_t>(c, 1);
}

// Chirps per K1 team: long enough streams for the next-chirp prefetch, while
// keeping >= ~2048 workgroups per launch to fill 256 CUs.
int range_cpt(int nr, int64_t nchirps) {
  const int T = nr >= 16 ? nr / 16 : 1;
  const int teams = T >= 256 ? 1 : 256 / T;
  const int64_t c = nchirps / ((int64_t)teams * 2048);
  return (int)std::max<int64_t>(1, std::min<int64_t>(8, c));
}


}  // namespace

extern "C" {

int32_t fmcw_abi_version(void) { return FMCW_ABI_VERSION; }

const char* fmcw_last_error(void) { return g_err.c_str(); }

int fmcw_device_count(int32_t* n) {
  if (!n) return fail(FMCW_E_ARG, "n is NULL");
  int d = 0;
  hipError_t e = hipGetDeviceCount(&d);
  if (e != hipSuccess) {
    *n = 0;
    return fail(FMCW_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *n = d;
  return FMCW_OK;
}

int fmcw_default_devices(int32_t cap, int32_t* ids, int32_t* n) {
  if (!ids || !n || cap < 1) return fail(FMCW_E_ARG, "ids/n NULL or cap < 1");
  *n = 0;
  const char* env = std::getenv("FMCW_DEVICES");
  std::string v = env ? env : "";
  v.erase(std::remove_if(v.begin(), v.end(), [](char ch) { return ch == ' ' || ch == '\t'; }), v.end());
  std::vector<long> want;                      // the list is parsed before any device is asked about
  if (!v.empty() && v != "all") {
    size_t pos = 0;
    while (pos <= v.size()) {
      const size_t end = std::min(v.find(',', pos), v.size());
      const std::string tok = v.substr(pos, end - pos);
      char* stop = nullptr;
      const long id = tok.empty() ? -1 : std::strtol(tok.c_str(), &stop, 10);
      if (tok.empty() || *stop != '\0' || id < 0) return fail(FMCW_E_ARG, "FMCW_DEVICES: malformed list '" + v + "'");
      want.push_back(id);
      pos = end + 1;
    }
    if ((int64_t)want.size() > cap) return fail(FMCW_E_ARG, "FMCW_DEVICES: more ids than cap");
  }
  int nd = 0;
  hipError_t e = hipGetDeviceCount(&nd);
  if (e != hipSuccess) return fail(FMCW_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  if (want.empty()) {
    if (nd < 1) return fail(FMCW_E_HIP, "no HIP device present");
    const int m = std::min<int>(nd, cap);
    for (int i = 0; i < m; ++i) ids[i] = i;
    *n = m;
    return FMCW_OK;
  }
  for (size_t i = 0; i < want.size(); ++i) {
    if (want[i] >= nd)
      return fail(FMCW_E_ARG, "FMCW_DEVICES: device " + std::to_string(want[i]) + " not present (" +
                                  std::to_string(nd) + " devices)");
    ids[i] = (int32_t)want[i];
  }
  *n = (int32_t)want.size();
  return FMCW_OK;
}

static int ctx_create_one(int32_t device_id, fmcw_ctx** out) {
  *out = nullptr;
  int nd = 0;
  HIPCHK(hipGetDeviceCount(&nd));
  if (device_id < 0 || device_id >= nd)
    return fail(FMCW_E_HIP, "device " + std::to_string(device_id) + " not present (" + std::to_string(nd) + " devices)");
  HIPCHK(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_id));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(FMCW_E_HIP, std::string("libfmcw is built for gfx950, device is ") + prop.gcnArchName);
  auto* c = new fmcw_ctx();
  c->device = device_id;
  bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->sd, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->sx, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->cin, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->cout, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; i < 2; ++i)
    for (hipEvent_t* e : {&c->ev_h2d[i], &c->ev_comp[i], &c->ev_d2h[i]})
      ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  for (int i = 0; i < fmcw_ctx::kSlots; ++i)   // the streams schedule's joins: device scope
    for (hipEvent_t* e : {&c->ev_k1[i], &c->ev_k2[i], &c->ev_k3[i]})
      ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming | fmcw::kEvDevice) == hipSuccess;
  for (hipEvent_t* e : {&c->ev_fork, &c->ev_join})
    ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming | fmcw::kEvDevice) == hipSuccess;
  if (!ok) {
    delete c;
    return fail(FMCW_E_HIP, "stream/event creation failed");
  }
  *out = c;
  return FMCW_OK;
}

int fmcw_ctx_create(int32_t n_devices, const int32_t* device_ids, fmcw_ctx** out) {
  if (!out) return fail(FMCW_E_ARG, "out is NULL");
  *out = nullptr;
  if (n_devices < 1 || n_devices > 64) return fail(FMCW_E_ARG, "n_devices must be in [1, 64]");
  std::vector<int> ids(n_devices);
  for (int i = 0; i < n_devices; ++i) ids[i] = device_ids ? device_ids[i] : i;
  fmcw_ctx* c = nullptr;
  CHK(ctx_create_one(ids[0], &c));
  for (int i = 1; i < n_devices; ++i) {
    fmcw_ctx* q = nullptr;
    const int st = ctx_create_one(ids[i], &q);
    if (st != FMCW_OK) {
      delete c;
      return st;
    }
    c->peers.push_back(q);
  }
  std::vector<int> sorted = ids;
  std::sort(sorted.begin(), sorted.end());
  const bool distinct = std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
  if (n_devices > 1 && distinct) {   // one communicator per device, one process
    if (!rccl().ok) {
      delete c;
      return fail(FMCW_E_HIP, "RCCL (librccl.so.1) not found: needed for a context over several devices");
    }
    c->comms.assign(n_devices, nullptr);
    const ncclResult_t r = rccl().comm_init_all(c->comms.data(), n_devices, ids.data());
    if (r != ncclSuccess) {
      c->comms.clear();
      const std::string msg = std::string("ncclCommInitAll: ") + rccl().error_string(r);
      delete c;
      return fail(FMCW_E_HIP, msg);
    }
  }
  *out = c;
  return FMCW_OK;
}

int fmcw_ctx_devices(fmcw_ctx* c, int32_t* n_devices, int32_t* device_ids, int32_t* rccl_comms) {
  if (!c || !n_devices) return fail(FMCW_E_ARG, "NULL argument");
  *n_devices = 1 + (int32_t)c->peers.size();
  if (device_ids) {
    device_ids[0] = c->device;
    for (size_t i = 0; i < c->peers.size(); ++i) device_ids[i + 1] = c->peers[i]->device;
  }
  if (rccl_comms) *rccl_comms = c->comms.empty() ? 0 : 1;
  return FMCW_OK;
}

int fmcw_ctx_destroy(fmcw_ctx* c) {
  if (!c) return FMCW_OK;
  delete c;
  return FMCW_OK;
}

int fmcw_set_taps(fmcw_ctx* c, const fmcw_params* p, const float* range_win, const float* doppler_win,
                  const float* calib) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(check_params(p));
  if (!range_win || !doppler_win || !calib) return fail(FMCW_E_ARG, "taps pointer is NULL");
  CHK(set_device(c));
  hipStream_t s = c->stream;
  // the taps are read by work on the caller's streams, which the context's stream does not
  // order against: let queued work finish with the old taps, and finish the copies before
  // returning, so that a call on any stream afterwards reads the new ones
  HIPCHK(hipDeviceSynchronize());
  CHK(c->wd.ensure((size_t)p->pn * 4));
  CHK(c->cal.ensure((size_t)p->nts * 8));
  HIPCHK(hipMemcpyAsync(c->wd.p, doppler_win, (size_t)p->pn * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->cal.p, calib, (size_t)p->nts * 8, hipMemcpyHostToDevice, s));
  c->h_wr.assign(range_win, range_win + p->nts);
  c->h_cal.assign(calib, calib + 2 * (size_t)p->nts);
  double sr = 0, si = 0;
  for (int n = 0; n < p->nts; ++n) { sr += calib[2 * n]; si += calib[2 * n + 1]; }
  c->cal_sum = make_float2((float)sr, (float)si);
  CHK(build_calw(c, p->if_scale, s));
  CHK(upload_twiddles(c->tw_nr, p->nr, s));
  CHK(upload_twiddles(c->tw_nd, p->nd, s));
  c->p = *p;
  c->taps = true;
  c->x_tab_ok = false;
  HIPCHK(hipStreamSynchronize(s));
  for (fmcw_ctx* q : c->peers) CHK(fmcw_set_taps(q, p, range_win, doppler_win, calib));
  return FMCW_OK;
}

int fmcw_set_chunk_frames(fmcw_ctx* c, int64_t frames) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (frames < 0) return fail(FMCW_E_ARG, "frames < 0");
  c->chunk_frames = frames;
  for (fmcw_ctx* q : c->peers) q->chunk_frames = frames;
  return FMCW_OK;
}

int fmcw_set_pipeline(fmcw_ctx* c, int32_t mode) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (mode != FMCW_PIPE_AUTO && mode != FMCW_PIPE_STREAMS && mode != FMCW_PIPE_ONEPASS && mode != FMCW_PIPE_XCD)
    return fail(FMCW_E_ARG, "bad pipeline mode");
  c->pipe_mode = mode;
  for (fmcw_ctx* q : c->peers) q->pipe_mode = mode;
  return FMCW_OK;
}

// The XCD-team schedule's sticky error word (kernels_xcd.hip): read after the
// stream is idle; a set bit means the outputs of some k_rdx launch are invalid.
static int xcd_check(fmcw_ctx* c) {
  if (!c->xcd_used) return FMCW_OK;
  unsigned e = 0;
  HIPCHK(hipMemcpy(&e, c->x_err.p, sizeof(e), hipMemcpyDeviceToHost));
  c->xcd_used = false;
  if (!e) return FMCW_OK;
  HIPCHK(hipMemset(c->x_err.p, 0, sizeof(e)));
  return fail(FMCW_E_HIP, (e & 2) ? "XCD schedule: an XCD received more than 32 workgroups (outputs invalid)"
                                  : "XCD schedule: a range-cube hand-off timed out (outputs invalid)");
}

int fmcw_rdx_clock(fmcw_ctx* c, double* mhz, double* us) {
  if (!c || !mhz) return fail(FMCW_E_ARG, "ctx / mhz is NULL");
  *mhz = 0.0;
  if (us) *us = 0.0;
  CHK(set_device(c));
  if (!c->x_clk.p) return FMCW_OK;             // no k_rdx launch yet
  unsigned long long h[4] = {};
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h, c->x_clk.p, sizeof(h), hipMemcpyDeviceToHost));
  if (h[3] > h[1] && h[2] > h[0]) {
    *mhz = (double)(h[2] - h[0]) / (double)(h[3] - h[1]) * 100.0;   // s_memrealtime: 100 MHz
    if (us) *us = (double)(h[3] - h[1]) / 100.0;
  }
  return FMCW_OK;
}

int fmcw_copy_device(fmcw_ctx* c, const void* d_src, void* d_dst, int64_t bytes, void* stream) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (!d_src || !d_dst || bytes < 0) return fail(FMCW_E_ARG, "bad copy arguments");
  CHK(set_device(c));
  HIPCHK(fmcw::launch_copy16(d_src, d_dst, bytes, pick(c, stream)));
  return FMCW_OK;
}

int fmcw_synchronize(fmcw_ctx* c) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(set_device(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  return xcd_check(c);
}

int fmcw_timing_enable(fmcw_ctx* c, int32_t enable) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (enable < 0 || enable > 3) return fail(FMCW_E_ARG, "timing level must be 0, 1, 2 or 3");
  c->timing = enable;
  return FMCW_OK;   // device 0 only: the timers are the device-pointer calls' (benches)
}

static int timing_collect(fmcw_ctx* c) {
  for (auto& pd : c->pending) {
    HIPCHK(hipEventSynchronize(pd.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, pd.a, pd.b));
    c->total_ms[pd.stage] += ms;
    c->launches[pd.stage] += 1;
    c->pool.push_back(pd.a);
    c->pool.push_back(pd.b);
  }
  c->pending.clear();
  return FMCW_OK;
}

static int timing_read(fmcw_ctx* c, int32_t stage, int32_t stages, double* total_ms, int64_t* launches) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (stage < 0 || stage >= stages) return fail(FMCW_E_ARG, "stage out of range");
  CHK(set_device(c));
  CHK(timing_collect(c));
  if (total_ms) *total_ms = c->total_ms[stage];
  if (launches) *launches = c->launches[stage];
  return FMCW_OK;
}

int fmcw_timing_read(fmcw_ctx* c, int32_t stage, double* total_ms, int64_t* launches) {
  return timing_read(c, stage, kStagesRead, total_ms, launches);
}

int fmcw_timing_read_ext(fmcw_ctx* c, int32_t stage, double* total_ms, int64_t* launches) {
  return timing_read(c, stage, kStages, total_ms, launches);
}

int fmcw_timing_reset(fmcw_ctx* c) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  CHK(set_device(c));
  CHK(timing_collect(c));
  for (int i = 0; i < kStages; ++i) { c->total_ms[i] = 0; c->launches[i] = 0; }
  return FMCW_OK;
}

// ---------------------------------------------------------------------------
// per-frame stages
// ---------------------------------------------------------------------------
// Twiddle table of the XCD-team schedule (kernels_xcd.hip, XT_* sections, lane order [..][64]),
// built in float64 and rounded once; it depends only on NR, so it is built once per context.
static int build_xcd_tab(fmcw_ctx* c, hipStream_t s) {
  const int NR = c->p.nr;
  std::vector<double> cr(NR), ci(NR);
  for (int i = 0; i < NR; ++i) {
    const double a = -2.0 * M_PI * (double)i / (double)NR;
    cr[i] = std::cos(a);
    ci[i] = std::sin(a);
  }
  std::vector<float> xt(2 * (size_t)fmcw::XT_SIZE);
  auto xput = [&](int idx, int e1024) { xt[2 * idx] = (float)cr[e1024 & (NR - 1)]; xt[2 * idx + 1] = (float)ci[e1024 & (NR - 1)]; };
  for (int l = 0; l < 64; ++l) {
    for (int k1 = 1; k1 < 8; ++k1)
      for (int e = 0; e < 2; ++e) xput(fmcw::XT_R1 + (2 * (k1 - 1) + e) * 64 + l, (2 * l + e) * k1);   // W1024^(a k1)
    for (int s1 = 1; s1 < 16; ++s1) xput(fmcw::XT_R2 + (s1 - 1) * 64 + l, 8 * ((l & 7) * s1));      // W128^(a0 s1)
    for (int d0 = 1; d0 < 16; ++d0) xput(fmcw::XT_D1 + (d0 - 1) * 64 + l, 4 * ((l & 15) * d0));     // W256^(q d0)
  }
  CHK(c->x_tab.ensure(xt.size() * 4));
  HIPCHK(hipMemcpyAsync(c->x_tab.p, xt.data(), xt.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  c->x_tab_ok = true;
  return FMCW_OK;
}

// fp16 storage on the single pass: the 128-bin blocks of the range cube that hold no bin able
// to become a detection or slow-time candidate (k_rdx's key test: 1 <= r <= NR - 2 and
// min_d <= r * dist_per_bin <= max_d, with two bins of margin each side for the local-maximum
// test's neighbours) are handed between the CUs as c32h; the others stay c64, so the slow-time
// rows and the profile around a target come from fp32 values.  FMCW_S16=0 keeps every block c64.
static unsigned host_s16mask(const fmcw_params* p, int NR) {
  {
    const char* e = std::getenv("FMCW_S16");
    if (e && e[0] == '0') return 0u;
  }
  const double dpb = p->dist_per_bin;
  if (!(dpb > 0.0) || !std::isfinite(dpb) || !std::isfinite(p->min_d) || !std::isfinite(p->max_d)) return 0u;
  const double lo_d = std::floor((double)p->min_d / dpb) - 2, hi_d = std::ceil((double)p->max_d / dpb) + 2;
  const int lo = (int)std::max(0.0, std::min((double)NR, lo_d));
  const int hi = (int)std::max(-1.0, std::min((double)NR - 1, hi_d));
  unsigned m = 0;
  for (int b = 0; b < NR / 128; ++b)
    if (hi < lo || 128 * b + 127 < lo || 128 * b > hi) m |= 1u << b;
  return m;
}

// The slow-time leg's start, fused into the detection (fmcw_process_slow_device): the
// compaction of :257-260 (frame list, L) and the reset of the STFT's running max(P).
struct SlowLeg {
  int32_t* list;
  int64_t* len;
  float* pmax;   // may be NULL
};

// Single-pass schedule (kernels_xcd.hip): k_rdx computes range FFT, profile,
// Doppler FFT and the slow-time candidate rows of each frame, the range cube
// handed between the CUs of one XCD; k_detect_1p runs the detection (and
// recomputes the rare slow-time row that was not among a group's candidates).
// Chunks bound the candidate scratch (XCD_TILES * XCD_CAND rows of PN floats per
// frame).  The hand-off is one 2 MiB slot per XCD, rewritten in place every frame.
static int process_onepass(fmcw_ctx* c, const fmcw_params* p, const void* d_iq, int h, int64_t F, float* d_prof,
                           int32_t* d_count, int32_t* d_ridx, float* d_rmag, int32_t* d_didx, float* d_slow,
                           void* d_rd, int64_t probe_column, float* d_probe, const SlowLeg* leg, hipStream_t s) {
  const int C = p->pn, S = p->nts, NR = p->nr, ND = p->nd, M = p->max_targets;
  const int64_t chunk = std::min<int64_t>(F, c->chunk_frames > 0 ? c->chunk_frames : 8192);
  const int tiles = fmcw::XCD_TILES, ncand = fmcw::XCD_CAND;
  const int TC = tiles * ncand;
  const int slots = 1;   // one in-place hand-off slot per XCD (xcd_place, fmcw_internal.h)
  {
#ifdef FMCW_XCUBE_PAD_AB   // A/B (tools/place_probe.py slots): the slot ring FMCW_XCUBE_PAD bytes into a larger buffer
    CHK(c->x_cube.ensure((size_t)8 * slots * fmcw::XCD_TILES * C * 32 * 8 + ((size_t)1 << 30)));
#else
    CHK(c->x_cube.ensure((size_t)8 * slots * fmcw::XCD_TILES * C * 32 * 8));
#endif
    if (!c->x_ctr.p) {                         // two counter sets, both zero before the first launch
      CHK(c->x_ctr.ensure(sizeof(unsigned) * 2 * fmcw::XCD_CTR_WORDS));
      HIPCHK(hipMemsetAsync(c->x_ctr.p, 0, sizeof(unsigned) * 2 * fmcw::XCD_CTR_WORDS, s));
      c->x_ctr_set = 0;
    }
    if (!c->x_clk.p) {
      CHK(c->x_clk.ensure(4 * sizeof(unsigned long long)));
      HIPCHK(hipMemsetAsync(c->x_clk.p, 0, 4 * sizeof(unsigned long long), s));
    }
    if (!c->x_err.p) {
      CHK(c->x_err.ensure(sizeof(unsigned)));
      HIPCHK(hipMemsetAsync(c->x_err.p, 0, sizeof(unsigned), s));
    }
  }
  CHK(c->op_rowpk.ensure((size_t)chunk * NR * 8));
  CHK(c->op_cidx.ensure((size_t)chunk * TC * 4));
  CHK(c->op_crows.ensure((size_t)chunk * TC * C * 4));
  int32_t* det_done = nullptr;
  if (leg) {
    int st = FMCW_OK;
    bool fresh = false;
    det_done = static_cast<int32_t*>(c->det_done.get(s, 9 * 128, &st, &fresh));   // 8 shards + top, 128 B apart
    CHK(st);
    if (fresh) HIPCHK(hipMemsetAsync(det_done, 0, 9 * 128, s));
  }
  const int64_t pframe = probe_column > 0 ? (probe_column - 1) / C : -1;
  const int pchirp = probe_column > 0 ? (int)((probe_column - 1) % C) : 0;
  if (!c->x_tab_ok) CHK(build_xcd_tab(c, s));
  if (pframe >= 0 && d_probe) {                // :410-411 fft_data column: one chirp by a direct DFT
    fmcw::ProbeArgs pa{};
    pa.iq = d_iq; pa.h = h;
    pa.frame = pframe; pa.chirp = pchirp; pa.C = C; pa.S = S; pa.NR = NR;
    pa.calw = c->calw.as<float4>(); pa.tw_nr = c->tw_nr.as<float2>(); pa.probe_mag = d_probe;
    HIPCHK(fmcw::launch_probe(pa, s));
  }
  StageTimer span(c, 7, s, 1);
  for (int64_t f0 = 0; f0 < F; f0 += chunk) {
    const int64_t nf = std::min(chunk, F - f0);
    fmcw::OnePassArgs a{};
    a.iq = static_cast<const char*>(d_iq) + (size_t)f0 * C * S * (h ? 4 : 8);
    a.h = h;
    a.rd_scale = h ? 1.0f / ((float)NR * ND) : 1.0f;
    a.F = nf; a.C = C; a.S = S;
    a.calw = c->calw.as<float4>();
    a.tw_nr = c->tw_nr.as<float2>(); a.tw_nd = c->tw_nd.as<float2>(); a.wd = c->wd.as<float>();
    a.rd = d_rd ? static_cast<char*>(d_rd) + (size_t)f0 * NR * ND * (h ? 4 : 8) : nullptr;
    a.profile = d_prof + f0 * NR;
    a.rowpk = c->op_rowpk.as<int2>();
    a.cand_idx = c->op_cidx.as<int32_t>();
    a.cand_rows = c->op_crows.as<float>();
    a.range_thr = p->range_thr; a.min_d = p->min_d; a.max_d = p->max_d; a.dist_per_bin = p->dist_per_bin;
    // counter sets: this launch counts in set x_ctr_set and zeroes the other one for the next launch (launches
    // of a device run one at a time, launch_xcd's chain); FMCW_XCD_MEMSET=1 (read per launch) adds a memset of
    // the counting set and changes nothing else, so the knob may differ from one launch to the next
    // (xcd_ctr_plan.h holds the rule, tests/native/xcd_ctr_plan.cpp checks it over every knob sequence)
    const bool xmemset = [] { const char* e = std::getenv("FMCW_XCD_MEMSET"); return e && e[0] == '1'; }();
    const fmcw::XcdCtrPlan xp = fmcw::xcd_ctr_plan(c->x_ctr_set, xmemset);
    a.xcube = c->x_cube.as<float2>(); a.xerr = c->x_err.as<unsigned>();
    a.xctr = c->x_ctr.as<unsigned>() + xp.count_set * fmcw::XCD_CTR_WORDS;
    a.xclr = xp.clear_set < 0 ? nullptr : c->x_ctr.as<unsigned>() + xp.clear_set * fmcw::XCD_CTR_WORDS;
    a.xmemset = xp.memset_first ? 1 : 0;
#ifdef FMCW_XCUBE_PAD_AB
    if (const char* e = std::getenv("FMCW_XCUBE_PAD")) {
      const size_t pad = std::min<size_t>((size_t)std::strtoull(e, nullptr, 0), (size_t)1 << 30) & ~(size_t)255;
      a.xcube = reinterpret_cast<float2*>(c->x_cube.as<char>() + pad);
    }
#endif
    a.slots = slots; a.xtab = c->x_tab.as<float2>(); a.cal_sum = c->cal_sum;
    a.clk = c->x_clk.as<unsigned long long>();
    a.s16mask = h ? host_s16mask(p, NR) : 0u;
    a.nteams = c->xcd_teams > 0 ? c->xcd_teams : 0;
    std::memcpy(a.xcc_team, c->xcc_team, sizeof(a.xcc_team));
    {
      const char* e = std::getenv("FMCW_ONEPASS_FORCE_FIX");
      a.force_fix = (e && e[0] == '1') ? 1 : 0;
    }
#if defined(XK_STAMPS) || defined(XK_SKEW)
    static unsigned long long* xdbg = nullptr;
    if (!xdbg) HIPCHK(hipMalloc(&xdbg, (size_t)1 << 20));
    a.dbg = xdbg;
#endif
    {
      StageTimer tm(c, 8, s, 2);
      {
        HIPCHK(fmcw::launch_xcd(a, s));
        c->xcd_used = true;
        if (nf > 0) c->x_ctr_set = xp.next_set;    // the next launch counts in the set this one zeroed
#ifdef XK_SKEW
        {   // diagnostic build: the team's skew.  Per XCD and step j: the spread of the 32 members' publish
            // times of R(j - 1), and how long after the last publish each member's poll of it returned
            // (100 MHz realtime clock, steps 8 .. 247 of the launch); which member published last how often
          constexpr int ST = 256;
          const int nblk = 32 * a.nteams;
          std::vector<unsigned long long> hh((size_t)nblk * 2 * ST);
          HIPCHK(hipStreamSynchronize(s));
          HIPCHK(hipMemcpy(hh.data(), a.dbg, hh.size() * 8, hipMemcpyDeviceToHost));
          double spread = 0, lag_min = 0, lag_max = 0, lag_mean = 0, pub_to_first_poll = 0;
          long n = 0;
          std::vector<long> last(32, 0), first(32, 0);
          for (int xx = 0; xx < a.nteams; ++xx)
            for (int j = 8; j < ST - 8; ++j) {
              unsigned long long pmin = ~0ull, pmax = 0, qmin = ~0ull, qmax = 0;
              double qs = 0;
              int kl = 0, kf = 0;
              for (int kk = 0; kk < 32; ++kk) {
                const unsigned long long p_ = hh[((size_t)(xx * 32 + kk)) * 2 * ST + 2 * j];
                const unsigned long long q_ = hh[((size_t)(xx * 32 + kk)) * 2 * ST + 2 * j + 1];
                if (p_ > pmax) { pmax = p_; kl = kk; }
                if (p_ < pmin) { pmin = p_; kf = kk; }
                qmin = std::min(qmin, q_); qmax = std::max(qmax, q_);
                qs += (double)q_;
              }
              if (!pmin || !qmin) continue;
              spread += (double)(pmax - pmin);
              lag_min += (double)qmin - (double)pmax;
              lag_max += (double)qmax - (double)pmax;
              lag_mean += qs / 32 - (double)pmax;
              pub_to_first_poll += (double)qmin - (double)pmin;
              ++last[kl]; ++first[kf]; ++n;
            }
          if (n) {
            std::fprintf(stderr, "xk-skew (us, %ld team-steps): publish spread %.2f | poll return after the last publish: "
                         "first %.2f mean %.2f last %.2f\n", n, spread / n / 100, lag_min / n / 100, lag_mean / n / 100,
                         lag_max / n / 100);
            std::fprintf(stderr, "xk-skew last publisher by member:");
            for (int kk = 0; kk < 32; ++kk) std::fprintf(stderr, " %ld", last[kk]);
            std::fprintf(stderr, "\nxk-skew first publisher by member:");
            for (int kk = 0; kk < 32; ++kk) std::fprintf(stderr, " %ld", first[kk]);
            std::fprintf(stderr, "\n");
          }
        }
#endif
#ifdef XK_STAMPS
        {   // diagnostic build: per-step phase times of k_rdx (100 MHz realtime clock), averaged over blocks
          const int nblk = 32 * a.nteams;
          std::vector<unsigned long long> hh(nblk * 32);
          HIPCHK(hipStreamSynchronize(s));
          HIPCHK(hipMemcpy(hh.data(), a.dbg, hh.size() * 8, hipMemcpyDeviceToHost));
          static const char* nm[10] = {"B1", "stage", "B2", "rows", "pubwait+B3", "cand", "R1+ld+D3",
                                       "poll+grp", "TD..R3", "RD"};
          for (int wv = 0; wv < 2; ++wv) {
            double ph[10] = {}, steps = 0;
            for (int bb = 0; bb < nblk; ++bb) {
              for (int q = 0; q < 10; ++q) ph[q] += (double)hh[(bb * 2 + wv) * 16 + q];
              steps += (double)hh[(bb * 2 + wv) * 16 + 15];
            }
            double tot = 0;
            std::fprintf(stderr, "xk-stamps wave %d (us/step):", wv * 4);
            for (int q = 0; q < 10; ++q) { std::fprintf(stderr, " %s %.2f |", nm[q], ph[q] / steps / 100); tot += ph[q]; }
            double cyc = 0, rt = 0;
            for (int bb = 0; bb < nblk; ++bb) { cyc += (double)hh[(bb * 2 + wv) * 16 + 13]; rt += (double)hh[(bb * 2 + wv) * 16 + 14]; }
            std::fprintf(stderr, " sum %.2f | clock %.3f GHz\n", tot / steps / 100, rt > 0 ? cyc / rt * 0.1 : 0.0);
          }
        }
#endif
      }
      tm.done();
    }
    fmcw::Detect1pArgs k{};
    k.profile = a.profile; k.rowpk = a.rowpk; k.rd = a.rd; k.ND = ND; k.rd_h = h; k.cand_idx = a.cand_idx; k.cand_rows = a.cand_rows;
    k.tiles = tiles; k.ncand = ncand;
    k.nframes = (int)nf; k.NR = NR; k.C = C; k.M = M;
    k.det.ND = ND; k.det.C = C; k.det.M = M;
    k.det.range_thr = p->range_thr; k.det.doppler_thr = p->doppler_thr;
    k.det.min_d = p->min_d; k.det.max_d = p->max_d; k.det.dist_per_bin = p->dist_per_bin;
    k.det.fallback = p->doppler_fallback_idx;
    k.det.cube_unscale = 1.0f; k.det.rd_unscale = 1.0f / a.rd_scale;
    k.count = d_count + f0; k.ridx = d_ridx + f0 * M; k.rmag = d_rmag + f0 * M; k.didx = d_didx + f0 * M;
    k.slow_mag = d_slow + f0 * C;
    k.iq = a.iq; k.h = h; k.S = S; k.calw = a.calw; k.tw_nr = a.tw_nr;
    if (leg && f0 + nf == F) {   // the last chunk's detection also compacts every frame of the call
      k.done = det_done; k.count_all = d_count; k.F_all = F; k.pn = C;
      k.list = leg->list; k.len = leg->len; k.pmax_reset = leg->pmax;
    }
    {
      StageTimer tm(c, 2, s, 2);
      HIPCHK(fmcw::launch_detect_1p(k, s));
      tm.done();
    }
  }
  if (leg) CHK(c->det_done.done(s));
  span.done();
  return FMCW_OK;
}

static int process_device_impl(fmcw_ctx* c, const fmcw_params* p, const void* d_iq, int32_t in_dtype, int64_t F,
                               float* d_prof, int32_t* d_count, int32_t* d_ridx, float* d_rmag, int32_t* d_didx,
                               float* d_slow, void* d_cube, void* d_rd, int32_t out_dtype, int64_t probe_column,
                               float* d_probe, const SlowLeg* leg, void* stream) {
  CHK(check_ctx(c, p));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F == 0) return FMCW_OK;
  if (in_dtype != FMCW_C64 && in_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad in_dtype");
  if (out_dtype != FMCW_C64 && out_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad out_dtype");
  if (!d_iq || !d_prof || !d_count || !d_ridx || !d_rmag || !d_didx || !d_slow)
    return fail(FMCW_E_ARG, "required device pointer is NULL");
  const int S = p->nts, C = p->pn, NR = p->nr, ND = p->nd, M = p->max_targets;
  if (probe_column < 0 || probe_column > F * (int64_t)C) return fail(FMCW_E_ARG, "probe_column out of range");
  hipStream_t s = pick(c, stream);
  // the single pass keeps one storage type end to end: c64 in / c64 RD, or
  // fp16 storage (c32h in / c32h RD); the RD dtype is free when RD is not asked for
  const bool onepass_ok = !d_cube && (!d_rd || out_dtype == in_dtype) && fmcw::onepass_supported(S, C, NR, ND);
  // the XCD-team single pass (k_rdx) wherever it applies: half the HBM bytes of the streams
  // schedule (no range cube) and faster on MI355X; FMCW_PIPE_ONEPASS is
  // the same schedule (the 8-tile single pass of ABI 2 is retired); AUTO falls back to the
  // streams schedule where the geometry or the device does not allow it
  const bool want = c->pipe_mode == FMCW_PIPE_ONEPASS || c->pipe_mode == FMCW_PIPE_XCD;
  if (want || (c->pipe_mode == FMCW_PIPE_AUTO && onepass_ok)) {
    if (!onepass_ok)
      return fail(FMCW_E_ARG, "single-pass schedule: needs nr 1024, pn == nd == 256, even nts <= nr, "
                              "the RD map in the IQ dtype and no range cube");
    if (c->xcd_teams < 0) {
      int n = 0;
      HIPCHK(fmcw::xcd_census(&n, c->xcc_team));
      const char* e = std::getenv("FMCW_NO_XCD");
      c->xcd_teams = (e && e[0] == '1') ? 0 : n;
    }
    if (c->xcd_teams > 0)
      return process_onepass(c, p, d_iq, in_dtype == FMCW_C32H ? 1 : 0, F, d_prof, d_count, d_ridx, d_rmag, d_didx,
                             d_slow, d_rd, probe_column, d_probe, leg, s);
    if (want)
      return fail(FMCW_E_ARG, "XCD schedule: needs 32 CUs per XCD and a grid of one workgroup per CU dealt 32 per XCD");
  }
  const int64_t chunk = c->chunk_frames > 0 ? c->chunk_frames : default_chunk(p);
  const int cube_dt = d_cube ? out_dtype : FMCW_C64;
  const int rd_dt = d_rd ? out_dtype : FMCW_C64;
  // fp16 storage keeps MATLAB's values divided by the FFT sizes applied so far
  // (exact powers of two): |X|/Nr and |D|/(Nr*Nd) stay inside the fp16 range
  const float cube_scale = cube_dt == FMCW_C32H ? 1.0f / NR : 1.0f;
  const float rd_scale = rd_dt == FMCW_C32H ? 1.0f / ((float)NR * ND) : 1.0f;
  const int64_t cf = std::min(chunk, F);
  const size_t cube_slot = (size_t)cf * C * NR * 8, rd_slot = (size_t)cf * NR * ND * 8;
  constexpr int NS = fmcw_ctx::kSlots;
  // NS scratch slots: while K3(i-1) and K2(i) read slots (i-1)%NS and i%NS,
  // K1(i+1) fills slot (i+1)%NS
  if (!d_cube) CHK(c->scratch_cube.ensure(NS * cube_slot));
  if (!d_rd) CHK(c->scratch_rd.ensure(NS * rd_slot));
  const int64_t pframe = probe_column > 0 ? (probe_column - 1) / C : -1;
  const int pchirp = probe_column > 0 ? (int)((probe_column - 1) % C) : 0;
  hipStream_t sd = c->sd, sx = c->sx;
  // one chunk: K1 -> K2 -> K3 have nothing to overlap with, so they go on the caller's stream
  // without the fork / join events (a deployed 115-frame call: 9 event calls fewer)
  if (F <= chunk) sd = sx = s;
  if (const char* e = std::getenv("FMCW_ONE_STREAM"); e && e[0] == '1') sd = sx = s;   // A/B probe
  const bool split = sd != s || sx != s;
  StageTimer span(c, 7, s, 1);     // range+Doppler span: before K1(0) on s ... after the last K2 on sd
  if (split) {
    HIPCHK(hipEventRecord(c->ev_fork, s));
    HIPCHK(hipStreamWaitEvent(sd, c->ev_fork, 0));
    HIPCHK(hipStreamWaitEvent(sx, c->ev_fork, 0));
  }

  int64_t i = 0;
  for (int64_t f0 = 0; f0 < F; f0 += chunk, ++i) {
    const int b = (int)(i % NS);
    const int64_t nf = std::min(chunk, F - f0);
    if (split && i >= NS) HIPCHK(hipStreamWaitEvent(s, c->ev_k3[b], 0));   // WAR: K2/K3(i-NS) done with slot b
    char* cube = d_cube ? static_cast<char*>(d_cube) + (size_t)f0 * C * NR * esize(cube_dt)
                        : c->scratch_cube.as<char>() + b * cube_slot;
    char* rd = d_rd ? static_cast<char*>(d_rd) + (size_t)f0 * NR * ND * esize(rd_dt)
                    : c->scratch_rd.as<char>() + b * rd_slot;

    fmcw::RangeArgs ra{};
    ra.iq = static_cast<const char*>(d_iq) + (size_t)f0 * C * S * esize(in_dtype);
    ra.in_dtype = in_dtype;
    ra.nchirps = nf * C;
    ra.C = C; ra.S = S; ra.NR = NR;
    ra.calw = c->calw.as<float4>();
    ra.cal_sum = c->cal_sum;
    ra.if_scale = p->if_scale;
    ra.tw = c->tw_nr.as<float2>();
    ra.cube = cube;
    ra.cube_dtype = cube_dt;
    ra.cube_scale = cube_scale;
    ra.profile = nullptr;
    ra.cpt = range_cpt(NR, ra.nchirps);
    {
      StageTimer tm(c, 0, s, 2);
      HIPCHK(fmcw::launch_range(ra, s));
      tm.done();
    }
    if (split) {
      HIPCHK(hipEventRecord(c->ev_k1[b], s));
      HIPCHK(hipStreamWaitEvent(sd, c->ev_k1[b], 0));
    }

    fmcw::DopplerArgs da{};
    da.cube = cube; da.cube_dtype = cube_dt;
    da.cube_unscale = 1.0f / cube_scale; da.rd_scale = rd_scale;
    da.nframes = (int)nf; da.C = C; da.NR = NR; da.ND = ND;
    da.wd = c->wd.as<float>();
    da.tw = c->tw_nd.as<float2>();
    da.rd = rd; da.rd_dtype = rd_dt;
    da.profile = d_prof + f0 * NR;
    {
      StageTimer tm(c, 1, sd, 2);
      HIPCHK(fmcw::launch_doppler(da, sd));
      tm.done();
    }
    if (split) {
      HIPCHK(hipEventRecord(c->ev_k2[b], sd));
      HIPCHK(hipStreamWaitEvent(sx, c->ev_k2[b], 0));
    }

    fmcw::DetectArgs ka{};
    ka.profile = d_prof + f0 * NR;
    ka.rd = rd; ka.rd_dtype = rd_dt;
    ka.cube = cube; ka.cube_dtype = cube_dt;
    ka.cube_unscale = 1.0f / cube_scale; ka.rd_unscale = 1.0f / rd_scale;
    ka.nframes = (int)nf; ka.NR = NR; ka.ND = ND; ka.C = C; ka.M = M;
    ka.range_thr = p->range_thr; ka.doppler_thr = p->doppler_thr;
    ka.min_d = p->min_d; ka.max_d = p->max_d; ka.dist_per_bin = p->dist_per_bin;
    ka.fallback = p->doppler_fallback_idx;
    ka.count = d_count + f0;
    ka.ridx = d_ridx + f0 * M;
    ka.rmag = d_rmag + f0 * M;
    ka.didx = d_didx + f0 * M;
    ka.slow_mag = d_slow + f0 * C;
    ka.probe_frame = (pframe >= f0 && pframe < f0 + nf) ? pframe - f0 : -1;
    ka.probe_chirp = pchirp;
    ka.probe_mag = d_probe;
    {
      StageTimer tm(c, 2, sx, 2);
      HIPCHK(fmcw::launch_detect(ka, sx));
      tm.done();
    }
    if (split) HIPCHK(hipEventRecord(c->ev_k3[b], sx));
  }
  span.s = sd;
  span.done();
  // join: the caller's stream waits for the last detect (which follows every K2)
  if (split) {
    HIPCHK(hipEventRecord(c->ev_join, sx));
    HIPCHK(hipStreamWaitEvent(s, c->ev_join, 0));
  }
  if (leg) {   // the streams schedule: the slow-time leg's start as launches of its own
    HIPCHK(fmcw::launch_compact(d_count, F, C, leg->list, leg->len, s));
    if (leg->pmax) HIPCHK(hipMemsetAsync(leg->pmax, 0, 4, s));
  }
  return FMCW_OK;
}

int fmcw_process_device(fmcw_ctx* c, const fmcw_params* p, const void* d_iq, int32_t in_dtype, int64_t F,
                        float* d_prof, int32_t* d_count, int32_t* d_ridx, float* d_rmag, int32_t* d_didx,
                        float* d_slow, void* d_cube, void* d_rd, int32_t out_dtype, int64_t probe_column,
                        float* d_probe, void* stream) {
  return process_device_impl(c, p, d_iq, in_dtype, F, d_prof, d_count, d_ridx, d_rmag, d_didx, d_slow, d_cube, d_rd,
                             out_dtype, probe_column, d_probe, nullptr, stream);
}

int fmcw_process_slow_device(fmcw_ctx* c, const fmcw_params* p, const void* d_iq, int32_t in_dtype, int64_t F,
                             float* d_prof, int32_t* d_count, int32_t* d_ridx, float* d_rmag, int32_t* d_didx,
                             float* d_slow, void* d_rd, int32_t out_dtype, int32_t* d_frame_list, int64_t* d_len,
                             float* d_pmax, void* stream) {
  if (!d_frame_list || !d_len) return fail(FMCW_E_ARG, "d_frame_list / d_len is NULL");
  if (F == 0 && c) {   // nothing to detect: the leg still starts (L = 0, max(P) = 0)
    CHK(check_ctx(c, p));
    hipStream_t s = pick(c, stream);
    HIPCHK(hipMemsetAsync(d_len, 0, 8, s));
    if (d_pmax) HIPCHK(hipMemsetAsync(d_pmax, 0, 4, s));
    return FMCW_OK;
  }
  const SlowLeg leg{d_frame_list, d_len, d_pmax};
  return process_device_impl(c, p, d_iq, in_dtype, F, d_prof, d_count, d_ridx, d_rmag, d_didx, d_slow, nullptr, d_rd,
                             out_dtype, 0, nullptr, &leg, stream);
}

int fmcw_range_fft_device(fmcw_ctx* c, const fmcw_params* p, const void* d_iq, int32_t in_dtype, int64_t F,
                          void* d_cube, int32_t out_dtype, float* d_prof, void* stream) {
  CHK(check_ctx(c, p));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F == 0) return FMCW_OK;
  if (!d_iq || !d_cube || !d_prof) return fail(FMCW_E_ARG, "required device pointer is NULL");
  if (in_dtype != FMCW_C64 && in_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad in_dtype");
  if (out_dtype != FMCW_C64 && out_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad out_dtype");
  hipStream_t s = pick(c, stream);
  HIPCHK(hipMemsetAsync(d_prof, 0, (size_t)F * p->nr * 4, s));   // 0.0f: identity of max over |.|
  fmcw::RangeArgs ra{};
  ra.iq = d_iq; ra.in_dtype = in_dtype;
  ra.nchirps = F * p->pn;
  ra.C = p->pn; ra.S = p->nts; ra.NR = p->nr;
  ra.calw = c->calw.as<float4>(); ra.cal_sum = c->cal_sum; ra.if_scale = p->if_scale;
  ra.tw = c->tw_nr.as<float2>();
  ra.cube = d_cube; ra.cube_dtype = out_dtype;
  ra.cube_scale = out_dtype == FMCW_C32H ? 1.0f / p->nr : 1.0f;
  ra.profile = d_prof;
  int cpt = 8;      // config 2: 2 workgroups per frame (771-782 us vs 786-787 at 16; profiles/r04_k1_profile_combine.txt)
  if (const char* e = std::getenv("FMCW_K1_CPT")) cpt = std::max(1, std::min(64, std::atoi(e)));   // A/B
  while (cpt > 1 && (p->pn % cpt) != 0) cpt >>= 1;
  ra.cpt = cpt;
  // workgroups of TEAMS teams x cpt chirps: when several share a frame evenly, their profile
  // maxima go to per-workgroup slots (plain stores) and one reduction pass forms the profile
  const int T = p->nr >= 16 ? p->nr / 16 : 1;
  const int teams = T >= 256 ? 1 : 256 / T;
  const int64_t per_wg = (int64_t)teams * cpt;
  ra.parts = (per_wg < p->pn && p->pn % per_wg == 0) ? (int)(p->pn / per_wg) : 0;
  if (ra.parts > 1) {
    int st = FMCW_OK;
    ra.prof_part = static_cast<float*>(c->k1_part.get(s, (size_t)F * ra.parts * p->nr * 4, &st));
    CHK(st);
  }
  StageTimer tm(c, 6, s);
  HIPCHK(fmcw::launch_range(ra, s));
  if (ra.parts > 1) {
    HIPCHK(fmcw::launch_profile_reduce(ra.prof_part, ra.parts, F, p->nr, d_prof, s));
    CHK(c->k1_part.done(s));
  }
  tm.done();
  return FMCW_OK;
}

// ---------------------------------------------------------------------------
// slow time (the STFT on it: api_stft.cpp)
// ---------------------------------------------------------------------------
int fmcw_compact_device(fmcw_ctx* c, const int32_t* d_count, int64_t F, int32_t pn, int32_t* d_list,
                        int64_t* d_len, void* stream) {
  if (!c) return fail(FMCW_E_ARG, "ctx is NULL");
  if (F < 0 || pn < 1) return fail(FMCW_E_ARG, "bad F / pn");
  if (!d_count || !d_list || !d_len) return fail(FMCW_E_ARG, "NULL device pointer");
  CHK(set_device(c));
  hipStream_t s = pick(c, stream);
  StageTimer tm(c, 3, s);
  HIPCHK(fmcw::launch_compact(d_count, F, pn, d_list, d_len, s));
  tm.done();
  return FMCW_OK;
}

// ---------------------------------------------------------------------------
// host-pointer per-frame API
// ---------------------------------------------------------------------------
}  // extern "C"

// The host-pointer calls as a two-slot pipeline over chunks of frames:
//   host:  caller's iq chunk i -> pinned slot i%2 (once the H2D of chunk i-2 has left it)
//   cin:   pinned slot -> device slot (after chunk i-2's kernels released the device slot)
//   s:     the device-pointer call on the chunk (small outputs written in place at f0)
//   cout:  the chunk's large outputs (range cube, RD map) -> pinned out slot; the host
//          copies chunk i-2's rows to the caller before that slot is reused
// The small per-frame outputs stay on the device for all F and come back once.
// `run(d_in, f0, nf, d_big[2])` enqueues the device call for one chunk on s.
struct BigOut {
  char* host;        // caller's [F][...] array or nullptr
  size_t fbytes;     // bytes per frame
};
template <typename Run>
static int host_pipeline(fmcw_ctx* c, const void* iq, int64_t F, size_t fin, const BigOut (&big)[2], Run&& run) {
  hipStream_t s = c->stream;
  const int64_t Fc = host_chunk(fin, F);
  const size_t slot_in = (size_t)Fc * fin;
  size_t slot_big[2], off_big[2] = {0, 0}, slot_out = 0;
  bool any = false;
  for (int q = 0; q < 2; ++q) {
    slot_big[q] = big[q].host ? (size_t)Fc * big[q].fbytes : 0;
    off_big[q] = slot_out;
    slot_out += slot_big[q];
    any = any || big[q].host;
  }
  CHK(c->h_iq.ensure(2 * slot_in));
  CHK(c->pin_in.ensure(2 * slot_in));
  if (any) {
    CHK(c->h_rd.ensure(2 * slot_out));
    CHK(c->pin_out.ensure(2 * slot_out));
  }
  const int64_t n = (F + Fc - 1) / Fc;
  auto drain = [&](int64_t j) -> int {          // chunk j's large outputs: pinned slot -> caller
    const int b = (int)(j & 1);
    const int64_t f0 = j * Fc, nf = std::min(Fc, F - f0);
    HIPCHK(hipEventSynchronize(c->ev_d2h[b]));
    for (int q = 0; q < 2; ++q)
      if (big[q].host)
        par_memcpy(big[q].host + (size_t)f0 * big[q].fbytes, c->pin_out.at(b * slot_out + off_big[q]),
                   (size_t)nf * big[q].fbytes);
    return FMCW_OK;
  };
  // one chunk: its H2D copy has nothing to overlap with and goes on s (no fork / join events)
  const bool single = n == 1;
  hipStream_t cin = single ? s : c->cin;
  if (!single) {
    HIPCHK(hipEventRecord(c->ev_fork, s));          // the device buffers are free once earlier work on s is done
    HIPCHK(hipStreamWaitEvent(c->cin, c->ev_fork, 0));
  }
  for (int64_t i = 0; i < n; ++i) {
    const int b = (int)(i & 1);
    const int64_t f0 = i * Fc, nf = std::min(Fc, F - f0);
    if (i >= 2) HIPCHK(hipEventSynchronize(c->ev_h2d[b]));   // pinned slot b: chunk i-2's H2D has read it
    par_memcpy(c->pin_in.at(b * slot_in), static_cast<const char*>(iq) + (size_t)f0 * fin, (size_t)nf * fin);
    if (i >= 2) HIPCHK(hipStreamWaitEvent(c->cin, c->ev_comp[b], 0));   // device slot b: chunk i-2's kernels are done
    HIPCHK(hipMemcpyAsync(c->h_iq.as<char>() + b * slot_in, c->pin_in.at(b * slot_in), (size_t)nf * fin,
                          hipMemcpyHostToDevice, cin));
    if (!single) {
      HIPCHK(hipEventRecord(c->ev_h2d[b], c->cin));
      HIPCHK(hipStreamWaitEvent(s, c->ev_h2d[b], 0));
    }
    if (any && i >= 2) {                          // device out slot b: chunk i-2's D2H has read it
      HIPCHK(hipStreamWaitEvent(s, c->ev_d2h[b], 0));
      CHK(drain(i - 2));                          // and its rows go to the caller (pinned slot b is reused below)
    }
    char* d_big[2];
    for (int q = 0; q < 2; ++q) d_big[q] = big[q].host ? c->h_rd.as<char>() + b * slot_out + off_big[q] : nullptr;
    CHK(run(c->h_iq.as<char>() + b * slot_in, f0, nf, d_big));
    HIPCHK(hipEventRecord(c->ev_comp[b], s));
    if (any) {
      HIPCHK(hipStreamWaitEvent(c->cout, c->ev_comp[b], 0));
      for (int q = 0; q < 2; ++q)
        if (big[q].host)
          HIPCHK(hipMemcpyAsync(c->pin_out.at(b * slot_out + off_big[q]), d_big[q], (size_t)nf * big[q].fbytes,
                                hipMemcpyDeviceToHost, c->cout));
      HIPCHK(hipEventRecord(c->ev_d2h[b], c->cout));
    }
  }
  if (any)
    for (int64_t j = std::max<int64_t>(0, n - 2); j < n; ++j) CHK(drain(j));
  return FMCW_OK;
}

extern "C" {

static int process_host_one(fmcw_ctx* c, const fmcw_params* p, const void* iq, int32_t in_dtype, int64_t F,
                            float* prof, int32_t* count, int32_t* ridx, float* rmag, int32_t* didx, float* slow,
                            float* cube, float* rd, int64_t probe_column, float* probe) {
  CHK(check_ctx(c, p));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F == 0) return FMCW_OK;
  if (!iq || !prof || !count || !ridx || !rmag || !didx || !slow) return fail(FMCW_E_ARG, "required pointer is NULL");
  if (in_dtype != FMCW_C64 && in_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad in_dtype");
  const int S = p->nts, C = p->pn, NR = p->nr, ND = p->nd, M = p->max_targets;
  hipStream_t s = c->stream;
  // the small outputs in one device arena, back through one pinned copy
  Arena ar;
  const size_t o_prof = ar.add((size_t)F * NR * 4), o_count = ar.add((size_t)F * 4), o_ridx = ar.add((size_t)F * M * 4),
               o_rmag = ar.add((size_t)F * M * 4), o_didx = ar.add((size_t)F * M * 4), o_slow = ar.add((size_t)F * C * 4),
               o_probe = ar.add(probe ? (size_t)NR * 4 : 0);
  CHK(c->h_small.ensure(ar.off));
  CHK(c->pin_small.ensure(ar.off));
  char* const hs = c->h_small.as<char>();
  auto at = [&](size_t o) { return reinterpret_cast<float*>(hs + o); };
  auto ati = [&](size_t o) { return reinterpret_cast<int32_t*>(hs + o); };
  const size_t fin = (size_t)C * S * esize(in_dtype);
  const BigOut big[2] = {{reinterpret_cast<char*>(cube), (size_t)C * NR * 8}, {reinterpret_cast<char*>(rd), (size_t)NR * ND * 8}};
  CHK(host_pipeline(c, iq, F, fin, big, [&](char* d_in, int64_t f0, int64_t nf, char* const* d_big) {
    const int64_t pc = probe && probe_column > f0 * C && probe_column <= (f0 + nf) * C ? probe_column - f0 * C : 0;
    return fmcw_process_device(c, p, d_in, in_dtype, nf, at(o_prof) + f0 * NR, ati(o_count) + f0, ati(o_ridx) + f0 * M,
                               at(o_rmag) + f0 * M, ati(o_didx) + f0 * M, at(o_slow) + f0 * C, d_big[0], d_big[1], FMCW_C64,
                               pc, pc ? at(o_probe) : nullptr, s);
  }));
  HIPCHK(hipMemcpyAsync(c->pin_small.p, hs, ar.off, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipStreamSynchronize(c->cout));
  const char* ps = c->pin_small.at(0);
  par_memcpy(prof, ps + o_prof, (size_t)F * NR * 4);
  std::memcpy(count, ps + o_count, (size_t)F * 4);
  std::memcpy(ridx, ps + o_ridx, (size_t)F * M * 4);
  std::memcpy(rmag, ps + o_rmag, (size_t)F * M * 4);
  std::memcpy(didx, ps + o_didx, (size_t)F * M * 4);
  par_memcpy(slow, ps + o_slow, (size_t)F * C * 4);
  if (probe) std::memcpy(probe, ps + o_probe, (size_t)NR * 4);
  return xcd_check(c);
}

static int range_fft_host_one(fmcw_ctx* c, const fmcw_params* p, const void* iq, int32_t in_dtype, int64_t F,
                              float* cube, float* prof) {
  CHK(check_ctx(c, p));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (F == 0) return FMCW_OK;
  if (!iq || !cube || !prof) return fail(FMCW_E_ARG, "required pointer is NULL");
  if (in_dtype != FMCW_C64 && in_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad in_dtype");
  const int S = p->nts, C = p->pn, NR = p->nr;
  hipStream_t s = c->stream;
  CHK(c->h_prof.ensure((size_t)F * NR * 4));
  const BigOut big[2] = {{reinterpret_cast<char*>(cube), (size_t)C * NR * 8}, {nullptr, 0}};
  CHK(host_pipeline(c, iq, F, (size_t)C * S * esize(in_dtype), big, [&](char* d_in, int64_t f0, int64_t nf, char* const* d_big) {
    return fmcw_range_fft_device(c, p, d_in, in_dtype, nf, d_big[0], FMCW_C64, c->h_prof.as<float>() + f0 * NR, s);
  }));
  HIPCHK(hipMemcpyAsync(prof, c->h_prof.p, (size_t)F * NR * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipStreamSynchronize(c->cout));
  return FMCW_OK;
}

}  // extern "C"

extern "C" {

int fmcw_process(fmcw_ctx* c, const fmcw_params* p, const void* iq, int32_t in_dtype, int64_t F, float* prof,
                 int32_t* count, int32_t* ridx, float* rmag, int32_t* didx, float* slow, float* cube, float* rd,
                 int64_t probe_column, float* probe) {
  CHK(check_ctx(c, p));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (in_dtype != FMCW_C64 && in_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad in_dtype");
  if (probe_column < 0 || probe_column > F * (int64_t)p->pn) return fail(FMCW_E_ARG, "probe_column out of range");
  const int C = p->pn, S = p->nts, NR = p->nr, ND = p->nd, M = p->max_targets;
  const size_t fin = (size_t)C * S * esize(in_dtype);
  // frames are independent: each device takes a contiguous shard and writes its
  // rows of every output in place (the range_speed concatenation of :386-389 is
  // the frame order itself); the probed column lives on one shard
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    const int64_t pc = probe_column > f0 * C && probe_column <= (f0 + n) * C ? probe_column - f0 * C : 0;
    return process_host_one(d, p, static_cast<const char*>(iq) + f0 * fin, in_dtype, n, prof + f0 * NR, count + f0,
                            ridx + f0 * M, rmag + f0 * M, didx + f0 * M, slow + f0 * C,
                            cube ? cube + f0 * (size_t)C * NR * 2 : nullptr, rd ? rd + f0 * (size_t)NR * ND * 2 : nullptr,
                            pc, pc ? probe : nullptr);
  });
}

int fmcw_range_fft(fmcw_ctx* c, const fmcw_params* p, const void* iq, int32_t in_dtype, int64_t F, float* cube,
                   float* prof) {
  CHK(check_ctx(c, p));
  if (F < 0) return fail(FMCW_E_ARG, "F < 0");
  if (in_dtype != FMCW_C64 && in_dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad in_dtype");
  const size_t fin = (size_t)p->pn * p->nts * esize(in_dtype);
  return over_devices(c, F, [&](fmcw_ctx* d, int, int64_t f0, int64_t n) {
    return range_fft_host_one(d, p, static_cast<const char*>(iq) + f0 * fin, in_dtype, n,
                              cube + f0 * (size_t)p->pn * p->nr * 2, prof + f0 * p->nr);
  });
}

int fmcw_synth_device(fmcw_ctx* c, const fmcw_params* p, int64_t frame0, int64_t F, void* d_iq, int32_t dtype,
                      void* stream) {
  CHK(check_ctx(c, p));
  if (F < 0 || frame0 < 0) return fail(FMCW_E_ARG, "F / frame0 < 0");
  if (!d_iq) return fail(FMCW_E_ARG, "d_iq is NULL");
  if (dtype != FMCW_C64 && dtype != FMCW_C32H) return fail(FMCW_E_ARG, "bad dtype");
  fmcw::SynthArgs a{};
  a.iq = d_iq; a.dtype = dtype; a.frame0 = frame0; a.nframes = F;
  a.C = p->pn; a.S = p->nts; a.NR = p->nr; a.ND = p->nd;
  a.dist_per_bin = p->dist_per_bin;
  a.cal = c->cal.as<float2>();
  HIPCHK(fmcw::launch_synth(a, pick(c, stream)));
  return FMCW_OK;
}

}  // extern "C"
