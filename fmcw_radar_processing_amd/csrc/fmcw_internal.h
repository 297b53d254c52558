// fmcw_internal.h -- launch wrappers shared by kernels_*.hip and fmcw_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xcd_place.h"   // k_rdx's hand-off place map (no HIP types: tests/native/xcd_place.cpp reads it on the host)

namespace fmcw {

// Flags of the events that only order work on one device (stream joins, per-stream scratch
// reuse, k_rdx's launch chain, the timing pairs read after a device synchronise): no system-scope
// release when they are recorded.  A default event's release makes the queue write the L2s back
// before the next packet runs; behind k_rdx (whose hand-off slots leave dirty lines in every XCD's
// L2) that showed as 6-19 us of idle GPU after every recorded event (profiles/r06_gaps.txt).
// The host-pointer path's copy events keep the default (the host reads what they guard).
// -DFMCW_EV_SYSFENCE restores the default flags (A/B).
#ifndef FMCW_EV_SYSFENCE
constexpr unsigned kEvDevice = hipEventDisableSystemFence;
#else
constexpr unsigned kEvDevice = 0;
#endif

struct RangeArgs {
  const void* iq;          // [nchirps][S] complex, dtype in_dtype
  int in_dtype;            // FMCW_C64 / FMCW_C32H
  int64_t nchirps;         // chirps in this launch (= frames * C)
  int C, S, NR;
  const float4* calw;      // [S] {cal.re, cal.im, if_scale*w, w}  (w = 2*blackman)
  float2 cal_sum;          // sum_n cal[n] over all S samples
  float if_scale;
  const float2* tw;        // [NR]
  void* cube;              // [nchirps][NR], dtype cube_dtype
  int cube_dtype;
  float cube_scale;        // stored value = X * cube_scale (1, or 1/NR for fp16)
  float* profile;          // [frames][NR] (max over chirps) or nullptr
  int cpt;                 // chirps per team (divides C when profile != nullptr)
  float* prof_part;        // [frames][parts][NR] per-workgroup maxima when a workgroup holds 1/parts of
  int parts;               // a frame (parts > 1), reduced by launch_profile_reduce; else nullptr / 0
};

struct DopplerArgs {
  const void* cube;        // [frames][C][NR]
  int cube_dtype;
  float cube_unscale;      // 1/cube_scale
  float rd_scale;          // stored value = D * rd_scale (1, or 1/(NR*ND) for fp16)
  int nframes, C, NR, ND;
  const float* wd;         // [C]
  const float2* tw;        // [ND]
  void* rd;                // [frames][NR][ND]
  int rd_dtype;
  float* profile;          // [frames][NR]
};

struct DetectArgs {
  const float* profile;    // [frames][NR]
  const void* rd;          // [frames][NR][ND]
  int rd_dtype;
  const void* cube;        // [frames][C][NR]
  int cube_dtype;
  float cube_unscale, rd_unscale;
  int nframes, NR, ND, C, M;
  float range_thr, doppler_thr, min_d, max_d, dist_per_bin;
  int fallback;
  int32_t* count;          // [frames]
  int32_t* ridx;           // [frames][M]
  float* rmag;             // [frames][M]
  int32_t* didx;           // [frames][M]
  float* slow_mag;         // [frames][C]
  int64_t probe_frame;     // frame within this launch, -1 = none
  int probe_chirp;
  float* probe_mag;        // [NR]
};

// detection constants shared by k_detect and k_detect_1p (frame_ops.h)
struct DetectParams {
  int ND, C, M;
  float range_thr, doppler_thr, min_d, max_d, dist_per_bin;
  int fallback;
  float cube_unscale, rd_unscale;
};

// Single-pass range+Doppler (kernels_xcd.hip, k_rdx): the range cube never
// reaches HBM; k_detect_1p / k_probe (kernels_detect.hip) finish
// the per-frame outputs.
struct OnePassArgs {
  const void* iq;          // [F][C][S] c64, or c32h when h
  int h;                   // fp16 storage (FMCW_C32H): c32h IQ in, c32h RD out holding D / (NR ND)
  float rd_scale;          // 1 / (NR ND) when h, else 1
  int64_t F;
  int C, S;                // NR = 1024, ND = C (kernel template)
  const float4* calw;      // [S] {cal.re, cal.im, IF_scale*w, w}
  const float2* tw_nr;     // [NR]
  const float2* tw_nd;     // [ND]
  const float* wd;         // [C]
  void* rd;                // [F][NR][ND] c64 (c32h when h), or nullptr (then only the row peaks are kept)
  float* profile;          // [F][NR]
  int2* rowpk;             // [F][NR] {float bits of max_d |D[r,d]|, first argmax d (fftshift-ed, 0-based)}; only when rd is nullptr
  int32_t* cand_idx;       // [F][XCD_TILES][XCD_CAND] 0-based bin or -1
  float* cand_rows;        // [F][XCD_TILES][XCD_CAND][C] |X[bin, k]|^2
  float range_thr, min_d, max_d, dist_per_bin;
  int force_fix;           // test knob (FMCW_ONEPASS_FORCE_FIX=1): keep no candidates, so every
                           // slow-time row goes through k_slow_fix
  unsigned long long* dbg; // diagnostic builds only (-DXK_STAMPS): [blocks][8] s_memrealtime stamps
  unsigned long long* clk; // or nullptr: {shader clock, 100 MHz clock} at the start and the end of team 0's
                           // member 0 (k_rdx's effective clock, fmcw_rdx_clock)
  // XCD-team schedule (k_rdx) only:
  float2* xcube;           // [8 XCDs][slots] hand-off slots of 32 x 32 places (xcd_place.h), 2 MiB each
  unsigned* xctr;          // [8 XCDs][2: ready, (unused)][XCD_MAX_SLOTS][32] + [8][32] tickets + the abort word:
                           // one 128-byte line per counter, XCD_CTR_WORDS in all (zero when a launch starts)
  unsigned* xclr;          // the context's other counter set (launches alternate between two): k_rdx's block 0
                           // zeroes its first XCD_IDLE words for the next launch, which saves a memset packet per
                           // launch; nullptr: launch_xcd zeroes xctr before the launch
  unsigned* xerr;          // sticky, reported by fmcw_synchronize: bit 0 a hand-off wait timed out, bit 1 an XCD
                           // got more than 32 blocks (the launch's own abort word lets its grid drain; a later
                           // launch starts with a clear one)
  int slots;               // hand-off slots allocated per XCD (1: k_rdx rewrites one slot in place)
  unsigned s16mask;        // fp16 storage only: bit b set = range bins 128 b .. 128 b + 127 (groups 4 b .. 4 b + 3)
                           // are handed over as c32h (X / NR): no bin of the block can become a detection or
                           // slow-time candidate (host_s16mask in fmcw_api.cpp); 0 = every group c64
  int nteams;              // XCDs of the device (teams of 32 CUs): 8 in SPX mode, 1-4 in the partition modes
  int xmemset;             // host only: 1 = launch_xcd zeroes xctr before the launch even though the previous
                           // launch zeroed it (FMCW_XCD_MEMSET=1, xcd_ctr_plan.h)
  int8_t xcc_team[16];     // HW_REG_XCC_ID -> team index 0..nteams-1, -1 for an XCC not in the device
  const float2* xtab;      // XT_* sections (host, float64, lane order)
  float2 cal_sum;          // sum_{n < S} cal[n]
};

// XCD-team schedule (kernels_xcd.hip): the 32 CUs of an XCD share each of its
// frames, split by chirps for the range FFT and by range-bin groups for the
// Doppler FFT; the range cube moves between them through the XCD's L2.
constexpr int XCD_TILES = 32;        // range-bin groups per frame (one per team member)
constexpr int XCD_CAND = 2;          // slow-time candidate rows kept per group
constexpr int XCD_MAX_SLOTS = 4;
constexpr int XCD_GRID = 256;        // at most 8 XCDs x 32 CUs, one persistent workgroup per CU
constexpr int XCD_TICKETS = 8 * 2 * 32 * XCD_MAX_SLOTS;   // xctr offset of the 8 per-XCD member tickets (128-byte lines)
constexpr int XCD_ABORT = XCD_TICKETS + 8 * 32;           // xctr offset of the launch's abort word (own line)
constexpr int XCD_IDLE = XCD_ABORT + 32;                  // xctr offset of [256 CUs][32] words the non-publishing
                                                          // waves add 0 to (kernels_xcd.hip, publish)
constexpr int XCD_CTR_WORDS = XCD_IDLE + 256 * 32;
// (where a chunk of the cube lives in the hand-off slot: xcd_place(j, r, w) of xcd_place.h, included above)
// table sections (float2, [..][64 lanes])
constexpr int XT_R1 = 0;             // [14]: W1024^((2l + e) k1), index 2 (k1 - 1) + e
constexpr int XT_R2 = 14 * 64;       // [15]: W128^((l & 7) s1), s1 = 1..15
constexpr int XT_D1 = 29 * 64;       // [15]: W256^((l & 15) d0), d0 = 1..15
constexpr int XT_SIZE = 44 * 64;
// group g, position p (0..31) <-> range bin: r = k1 + 16 h + 8 e + 128 s2 with
// k1 = (p >> 3) + 4 (g & 1), h = p & 7, e = (g >> 1) & 1, s2 = g >> 2
__host__ __device__ inline int xcd_bin(int g, int p) {
  return (p >> 3) + 4 * (g & 1) + 8 * ((g >> 1) & 1) + 16 * (p & 7) + 128 * (g >> 2);
}
__host__ __device__ inline int xcd_group(int r) { return ((r >> 2) & 1) | (((r >> 3) & 1) << 1) | ((r >> 7) << 2); }
__host__ __device__ inline int xcd_pos(int r) { return ((r & 3) << 3) | ((r >> 4) & 7); }

struct Detect1pArgs {
  const float* profile;    // [F][NR]
  const int2* rowpk;       // [F][NR] (used when rd is nullptr)
  const void* rd;          // [F][NR][ND] c64 (c32h when rd_h, holding D * det.rd_unscale^-1) or nullptr
  int ND, rd_h;
  const int32_t* cand_idx; // [F][tiles][ncand]
  const float* cand_rows;  // [F][tiles][ncand][C] |X|^2
  int tiles, ncand;        // XCD_TILES (tile = xcd_group) / XCD_CAND
  int nframes, NR, C, M;
  DetectParams det;
  int32_t* count;
  int32_t* ridx;
  float* rmag;
  int32_t* didx;
  float* slow_mag;         // [F][C]
  // the rare target row that was not a group candidate: its slow-time row (:257-259) recomputed
  // by the frame's own wave, a direct DFT of every chirp at that bin (was the k_slow_fix launch)
  const void* iq;          // [F][C][S] c64, or c32h when h
  int h, S;
  const float4* calw;
  const float2* tw_nr;
  // fused compaction (:257-260, as k_compact), when list != nullptr: every workgroup stores its
  // counts write-through and adds 1 to *done; the last one scans count_all[0..F_all) (the call's
  // earlier chunks included), writes list / *len, zeroes *pmax_reset (if set: the running max(P)
  // of the STFT passes that follow, :276 / :282) and resets *done for the next launch
  int32_t* done;           // device counters, 0 before the first launch: 8 shards + the top, 32 words apart
  const int32_t* count_all;
  int64_t F_all;
  int pn;
  int32_t* list;
  int64_t* len;
  float* pmax_reset;
};

hipError_t launch_detect_1p(const Detect1pArgs& a, hipStream_t s);
hipError_t launch_xcd(const OnePassArgs& a, hipStream_t s);
// The device's XCD teams: *nteams = its XCDs (0 when the XCD-team schedule cannot run: a CU count
// that is not 32 per XCD, or a grid of one workgroup per CU not dealt 32 per XCD), xcc_team[16]
// the team index of each HW_REG_XCC_ID.
hipError_t xcd_census(int* nteams, int8_t* xcc_team);

struct ProbeArgs {          // fft_data column (:410-411) for the single-pass schedule
  const void* iq;          // [F][C][S] of the launch, c64 or c32h (h)
  int h;
  int64_t frame;
  int chirp, C, S, NR;
  const float4* calw;
  const float2* tw_nr;
  float* probe_mag;        // [NR]
};
hipError_t launch_probe(const ProbeArgs& a, hipStream_t s);
bool onepass_supported(int nts, int pn, int nr, int nd);

struct StftArgs {
  const float* slow_mag;   // [*][pn]
  const int32_t* frame_list;
  const int64_t* len;      // device scalar L
  int pn;
  const float* halo;
  int n_halo;
  const int64_t* halo_len;  // device, or nullptr -> n_halo
  const float* win;        // device [wlen]
  int wlen, hop, nfft;
  float inv_fs;            // 1/fs; the 'psd' scale 1/(fs*sum(win^2)) is formed in-kernel
  int64_t max_seg;
  float* P;                // [max_seg][nfft/2+1]
  float* pmax;
  int64_t* nseg_out;
  const int32_t* bins;     // k_stft20 mode 3 / 4: the ascending bin list of the columns (device), else nullptr
  int ncol;                // k_stft20 mode 3 / 4: columns in `bins`
  const int32_t* tiles;    // k_stft_mfma mode 1: the 256-segment tiles to cover (device), nullptr = all
  int ntiles;
  int table_form;          // 1: the table-based k_stft_mfma / k_stft20 even at nfft 64 (the host call's
                           // max(P) pass, so that it forms P exactly as its listed-bins pass does)
};

// 20-tap fast path (kernels_stft.hip k_stft20): W table [nfft/2+1][20] from the window,
// then mode 0 P + max, 1 max only, 2 dB written to dst (given max), 3 P of the bins
// a.bins[0..a.ncol) only, written to dst as [seg][ncol], 4 each segment's max of P over the bins
// a.bins written to dst[seg] (matrix-core form only)
bool stft_fast_path(int wlen, int hop);
// the nfft-64 matrix-core kernel (k_stft64m) serves this nfft (not disabled by FMCW_STFT_MFMA=0);
// it verifies a cached W table against the call's window
bool stft64_form(int nfft);
// The kernel form launch_stft20 runs for (a, mode, dst): the nfft-64 kernels -- k_stft64f never reads the W
// table, k_stft64m verifies it against the call's window, so both may be given a table cached from an earlier
// call -- or the table form (k_stft_mfma / k_stft20), which trusts the table: its caller builds the table for
// this call.  nfft-64 form, mode <= 2, no tiles, no table_form, a 16-byte aligned output (mode 1 has none);
// FMCW_STFT64_FOLD=0 picks k_stft64m.
enum StftForm { STFT_FORM_TABLE = 0, STFT_FORM_64F = 1, STFT_FORM_64M = 2 };
StftForm stft_form(const StftArgs& a, int mode, const float* dst);
hipError_t launch_stft_table(const float* win, int nfft, float2* tab, hipStream_t s);
// dst_cap: floats available at dst (mode 0: at a.P), tab_cap: float2 entries of tab; a launch
// whose writes would not fit returns hipErrorInvalidValue before anything is enqueued
hipError_t launch_stft20(const StftArgs& a, const float2* tab, int mode, float* dst, hipStream_t s, int64_t dst_cap,
                         int64_t tab_cap);


struct StftDbArgs {
  const float* P;
  const int64_t* nseg;
  int64_t max_seg;
  int nbins_in;            // nfft/2+1
  const float* pmax;
  int nlog;                // 0 = no resampling
  const int32_t* lidx;     // [nlog]
  const float* lw;         // [nlog]
  float* out;
};

struct SynthArgs {
  void* iq;
  int dtype;
  int64_t frame0, nframes;
  int C, S, NR, ND;
  float dist_per_bin;
  const float2* cal;
};

hipError_t launch_range(const RangeArgs& a, hipStream_t s);
// profile[f][b] = max over parts of prof_part[f][part][b] (K1's per-workgroup maxima)
hipError_t launch_profile_reduce(const float* part, int parts, int64_t frames, int nr, float* profile, hipStream_t s);
hipError_t launch_doppler(const DopplerArgs& a, hipStream_t s);
hipError_t launch_detect(const DetectArgs& a, hipStream_t s);
hipError_t launch_compact(const int32_t* count, int64_t F, int pn, int32_t* frame_list, int64_t* len,
                          hipStream_t s);
hipError_t launch_stft_power(const StftArgs& a, hipStream_t s);
hipError_t launch_stft_db(const StftDbArgs& a, hipStream_t s);
hipError_t launch_synth(const SynthArgs& a, hipStream_t s);
hipError_t launch_fill_u32(uint32_t* p, uint32_t v, int64_t n, hipStream_t s);
// kernels_util.hip: the bench's HBM copy ceiling (16-byte nontemporal loads and stores)
hipError_t launch_copy16(const void* src, void* dst, int64_t bytes, hipStream_t s);


// 2-D CA-CFAR over the RD map (kernels_cfar.hip): k_cfar + k_cfar_gather
struct CfarArgs {
  const void* rd;          // [F][NR][ND] c64, or c32h (h) holding D / (NR ND); 16-byte aligned
  int h;
  float scale;             // NR * ND when h, else 1: powers come out in the units of |D|^2
  int64_t F;
  int NR, ND;
  int gr, gd, tr, td;      // guard / training half-widths
  int g0, g1;              // gated rows, 0-based, inclusive
  int K, local_max;
  float alpha;
  int RS, strips;          // rows per strip, strips over [g0, g1]          (cfar_plan)
  int TC, tiles, waves;    // columns per tile, tiles per row, waves per workgroup
  int32_t* sub_count;      // scratch [F][strips * tiles * waves] detections of each wave's cells
  float4* sub_list;        // scratch [F][strips * tiles * waves][K] {cell index bits, P, S / N, 0}
  int32_t* det_count;      // [F]
  int32_t* det_ridx;       // [F][K]
  int32_t* det_didx;       // [F][K]
  float* det_power;        // [F][K]
  float* det_noise;        // [F][K]
  uint8_t* mask;           // [F][NR][ND] or nullptr
};
void cfar_plan(CfarArgs& a, int64_t F);
size_t cfar_scratch_per_frame(const CfarArgs& a);
hipError_t launch_cfar(const CfarArgs& a, hipStream_t s);
hipError_t launch_cfar_gather(const CfarArgs& a, hipStream_t s);

// 2-D OS-CFAR over the RD map (kernels_oscfar.hip): k_oscfar + k_cfar_gather + k_oscfar_select.
// c is planned by cfar_plan and uses CA's scratch layout; its list entries' noise slot stays 0.
struct OsCfarArgs {
  CfarArgs c;
  int rank;                // 1..nfull, the caller's rank in the full window
  int nfull;               // training cells of the full window
};
hipError_t launch_oscfar(const OsCfarArgs& a, hipStream_t s);

// Doppler-time / range-time signatures of the RD map (kernels_sig.hip): k_sig + k_sig_gather, k_sig_db
struct SigArgs {
  const void* rd;          // [F][NR][ND] c64, or c32h (h) holding D / (NR ND); 16-byte aligned
  int h;
  float scale2;            // (NR * ND)^2 when h, else 1: the sums come out in the units of |D|^2
  int64_t F;
  int NR, ND;
  int g0, g1;              // gated rows, 0-based, inclusive
  int th;                  // track_half (used with center)
  int dc;                  // dc_half, -1 = keep every Doppler bin
  const int32_t* center;   // [F * cstride] 1-based row of the frame's window centre, or nullptr: the gate
  int64_t cstride;
  int SR, slabs;           // rows per slab, slabs per frame                 (sig_plan)
  float* part;             // scratch [F][slabs][ND] column sums, when slabs > 1 and dt
  float* dt;               // [F][ND] or nullptr
  float* rt;               // [F][NR] or nullptr
  float* dt_max;           // running maxima or nullptr
  float* rt_max;
};
void sig_plan(SigArgs& a);
size_t sig_scratch_per_frame(const SigArgs& a);
hipError_t launch_sig(const SigArgs& a, hipStream_t s);
hipError_t launch_sig_db(const float* map, int64_t n, const float* mx, float floor_db, float* out, hipStream_t s);

// Clustering of the CFAR detection lists into targets (kernels_cluster.hip): k_cluster
struct ClusterArgs {
  int64_t F;
  int ND;                  // Doppler ring length (a power of two)
  int K;                   // max_det: entries per frame of the lists
  int link_r, link_d, min_cells, max_tgt;
  const int32_t* det_count;        // [F]
  const int32_t* det_ridx;         // [F][K]
  const int32_t* det_didx;         // [F][K]
  const float* det_power;          // [F][K]
  const float* det_noise;          // [F][K] or nullptr
  int32_t* tgt_count;              // [F]
  // [F][max_tgt] each, any may be nullptr
  int32_t* cells; int32_t* pk_ridx; int32_t* pk_didx; int32_t* ext_r; int32_t* ext_d;
  float* pk_power; float* pk_noise; float* power; float* range; float* doppler;
  int32_t* det_label;              // [F][K] or nullptr
};
hipError_t launch_cluster(const ClusterArgs& a, hipStream_t s);

// Angle of arrival from several receive channels' RD maps at the CFAR cells (kernels_aoa.hip): k_aoa
constexpr int kAoaChan = 8;            // channels at most
struct AoaArgs {
  int64_t F;
  int NR, ND;
  int K;                   // max_det: entries per frame of the lists
  int A;                   // channels, 2..kAoaChan
  int M;                   // max_tgt, 0: no per-target outputs
  int h;                   // fp16 storage
  int tgt_any;             // some per-target output is asked for (then det_label is set and M >= 1)
  float scale2;            // (NR * ND)^2 when h, else 1: z, e0, e1 come out in the units of |D|^2
  float kinv;              // 1 / (2 pi spacing)
  float w[2 * kAoaChan];   // the channels' complex weights (re, im)
  const void* rd[kAoaChan];        // channel a: [F][NR][ND] c64, or c32h (h) holding D / (NR ND)
  const int32_t* det_count;        // [F]
  const int32_t* det_ridx;         // [F][K]
  const int32_t* det_didx;         // [F][K]
  const int32_t* det_label;        // [F][K] or nullptr
  // [F][K] each, any may be nullptr
  float* det_zre; float* det_zim; float* det_phase; float* det_sin;
  // [F][M] each, any may be nullptr
  float* tgt_zre; float* tgt_zim; float* tgt_e0; float* tgt_e1; float* tgt_phase; float* tgt_sin; float* tgt_coh;
  int32_t* tgt_cells;
};
hipError_t launch_aoa(const AoaArgs& a, hipStream_t s);

// Tracking of the per-frame targets across frames (kernels_track.hip): k_track
// One sequence's state block: kTrackFields arrays of T = max_trk 32-bit words (id, status, hits,
// misses, age as int32; r, v, d, power as float32), then the id counter, padded to 16 bytes.
constexpr int kTrackFields = 9;
constexpr int kTrackMax = 64;          // max_trk and max_tgt at most: a slot / a measurement per lane
constexpr int track_state_words(int max_trk) { return (kTrackFields * max_trk + 1 + 3) & ~3; }
struct TrackArgs {
  int64_t S, F;                    // sequences, frames per sequence
  int NR, ND;
  int M, T;                        // max_tgt, max_trk
  float wr, wd;                    // 1 / gate_r^2, 1 / gate_d^2
  float alpha_r, alpha_d, beta_r;
  int confirm_hits, max_coast;
  const int32_t* tgt_count;        // [S*F]
  const float* range;              // [S*F][M]
  const float* doppler;            // [S*F][M]
  const float* power;              // [S*F][M]
  uint32_t* state;                 // [S][track_state_words(T)]
  int32_t* trk_count;              // [S*F]
  // [S*F][T] each, any may be nullptr
  int32_t* trk_id; int32_t* trk_status; int32_t* trk_age; int32_t* trk_misses;
  float* trk_range; float* trk_rate; float* trk_doppler; float* trk_power;
  int32_t* tgt_track;              // [S*F][M] or nullptr
};
hipError_t launch_track(const TrackArgs& a, hipStream_t s);

// Frame-to-frame clutter filter of the RD map (kernels_mti.hip): k_mti + k_mti_seen
constexpr int kMtiRingC64 = 4;     // frames a lane keeps in flight ahead of the recursion
constexpr int kMtiRingC32H = 8;
struct MtiArgs {
  const void* rd;          // [S*F][NR][ND] c64 or c32h; 16-byte aligned
  void* out;               // the same shape and dtype, == rd (in place), or nullptr: learn only
  float* bg;               // [S][NR][ND] complex float32, read and (unless freeze) rewritten
  int32_t* seen;           // [S], advanced by k_mti_seen (unless freeze)
  int64_t S, F;
  int64_t n16;             // 16-byte pieces of one frame
  int bpf;                 // 256-thread blocks of one frame (set by launch_mti)
  int h;                   // fp16 storage
  int ring;                // 4, 8 or 16
  float lambda;
  int ramp, freeze;
};
bool mti_ring_ok(int ring);
hipError_t launch_mti(const MtiArgs& a, hipStream_t s);

// The receive channels' RD maps combined into beamformed or channel-integrated maps (kernels_beam.hip): k_beam
constexpr int kBeamMax = 8;            // channels and beams at most
struct BeamArgs {
  const void* rd[kBeamMax];        // channel a: the launch's frames, [F][NR][ND] c64 or c32h; 16-byte aligned
  void* out[kBeamMax];             // beam b: the same shape and dtype; may be one of rd (in place)
  int64_t n16;                     // 16-byte pieces of one map of the launch: F * (frame bytes / 16)
  int A, B;                        // channels 2..kBeamMax, beams 1..kBeamMax (1 when nci)
  int h;                           // fp16 storage
  int nci;                         // non-coherent integration: out[0] = (sqrt(sum |t_a|^2), +0)
  float w[kBeamMax][kBeamMax][2];  // (re, im) per (beam, channel)
};
hipError_t launch_beam(const BeamArgs& a, hipStream_t s);

// Range-angle maps (kernels_ra.hip): k_cov (the channels' spatial covariance per range row) and
// k_ra (the Bartlett / Capon spectrum of every row)
constexpr int kRaChan = 8;             // channels at most
constexpr int kRaAngMax = 256;         // look directions at most
constexpr int64_t kRaRowsMax = (int64_t)1 << 30;   // rows (frames * NR) of one launch at most
struct CovArgs {
  const void* rd[kRaChan];         // channel a: the launch's frames, [rows][ND] c64 or c32h; 16-byte aligned
  float* cov;                      // [rows][T][2], T = A (A + 1) / 2; 8-byte aligned
  int64_t rows;                    // frames * NR of the launch
  int A, NR, ND;
  int h;                           // fp16 storage
  int g0, g1;                      // gated rows, 0-based, inclusive
  int dc;                          // dc_half, -1 = keep every Doppler bin
  int rpw;                         // rows a wave takes one after the other where a row fills a wave-load (cov_rows_per_wave)
  float scale2;                    // (NR * ND)^2 when h, else 1
};
int cov_rows_per_wave(int nd, int h);
hipError_t launch_cov(const CovArgs& a, hipStream_t s);
struct RaArgs {
  const float* cov;                // [rows][T][2]
  const float* w;                  // [n_ang][A][2]
  float* ra;                       // [rows][n_ang]
  float* ra_max;                   // running maximum or nullptr
  int64_t rows;
  int A, NR, n_ang;
  int g0, g1;
  int capon;
  float load;
};
hipError_t launch_ra(const RaArgs& a, hipStream_t s);

// MUSIC (kernels_music.hip): k_music (per range row the eigen-decomposition of its covariance, a
// source count and the MUSIC pseudo-spectrum)
struct MusicArgs {
  const float* cov;                // [rows][T][2]; 8-byte aligned
  const float* w;                  // [n_ang][A][2]; read only with music
  float* eval;                     // [rows][A] or nullptr
  float* evec;                     // [rows][A][A][2] or nullptr
  int32_t* nsrc;                   // [rows] or nullptr
  float* music;                    // [rows][n_ang] or nullptr
  float* music_max;                // running maximum or nullptr
  int64_t rows;
  int A, NR, n_ang;
  int g0, g1;
  int n_src, max_src;              // n_src 0: estimated, at most max_src
  int sweeps;
  int fb;                          // forward-backward averaging
  float src_thr;
};
hipError_t launch_music(const MusicArgs& a, hipStream_t s);

// Directions of arrival (kernels_doa.hip): k_doa (per range row the peaks of its angular spectrum,
// thinned, ordered by power, each with a sub-grid direction)
constexpr int kDoaPkMax = 8;           // written peaks of a row at most
struct DoaArgs {
  const float* spec;               // [rows][K]
  const float* u;                  // [K]: the grid, sin(theta) of every look direction
  int32_t* count;                  // [rows] or nullptr
  int32_t* idx;                    // [rows][max_pk] or nullptr
  float* pw;                       // [rows][max_pk] or nullptr
  float* sn;                       // [rows][max_pk] or nullptr
  float* base;                     // [rows][max_pk] or nullptr
  int64_t rows;
  int K, NR;
  int g0, g1;
  int max_pk;
  int flags;                       // FMCW_DOA_*
  float min_abs, min_rel, min_prom;
};
hipError_t launch_doa(const DoaArgs& a, hipStream_t s);

bool range_size_supported(int nr);
bool doppler_size_supported(int nd);

// spectrogram.png of :331-348 (kernels_render.hip)
struct RenderArgs {
  const float* Q;          // [nseg][nq + 1]: P of bins 0 .. nq-1, then the Nyquist bin nb-1
  int nq;
  const int64_t* nseg;     // device scalar
  const float* pmax;       // device scalar: max(P(:)) (:282-283)
  int nb, nfft, seam;      // one-sided bins, FFT size, the bin m whose face (m, m+1) fftshift drops
  double fs, t0, dt;       // sample rate, T(1), T(2) - T(1)
  double fmax, cmin, cmax; // ylim([0 fmax]), clim([cmin cmax])
  int W, H;                // pixels
  uint8_t* img;            // [H][1 + W] palette indices, PNG filter byte first
};
hipError_t launch_render(const RenderArgs& a, hipStream_t s);

}  // namespace fmcw

#include "host_io.h"   // png_write_indexed, jet_palette, set_error
