/*
 * fmcw.h -- C-ABI of libfmcw, the MI355X (gfx950) FMCW radar DSP path.
 *
 * Drop-in boundary for the per-frame fast-time / slow-time / STFT loop of
 * alepnabil/fmcw_radar_processing, radar-etl-pipeline/radar_processing.m
 * (function radar_processing(process_animal_activity), :56).  The reference
 * has no FFI layer of its own: every step is a MATLAB built-in call inside
 * one serial loop.  The entry points below replace exactly these lines, and
 * are what a MEX gateway (mex/fmcw_mex.c) binds; INTEGRATION.md shows the
 * MATLAB-side call sequence and a ctypes binding.
 *
 *   fmcw_set_taps      <- :121/:136 IF_scale, :138-139 window taps, :166-174 calib_rx1
 *   fmcw_process       <- :197-261 per-frame loop ('no' branch) + :265 range_tx1rx1_max_abs
 *                         (:457-498 per-frame part of the 'yes' branch is the same math)
 *   fmcw_range_fft     <- :203-205 + :207 + :210 only (range cube + profile; config 2)
 *   fmcw_stft          <- :270-299 (|slow|, nextpow2, spectrogram, fftshift, 20log10,
 *                         logspace + interp1)
 *
 * Conventions
 *   - Plain C types only.  Complex data is interleaved (re, im) float32, which
 *     is MATLAB's interleaved-complex `single` layout (-R2018a API).
 *   - Array shapes are written C-style, last index fastest.  Every one of them
 *     is also the memory layout of the MATLAB array named next to it, so a MEX
 *     gateway hands MATLAB buffers through without copies or transposes.
 *   - Return value: FMCW_OK (0) or a negative fmcw_status; the message of the
 *     last failure on the calling thread is in fmcw_last_error().
 *   - A context is NOT thread-safe: one per host thread (MEX keeps one static).
 *   - The caller owns every I/O buffer; the library never returns memory.
 *   - There is no CPU fallback: on a host without a usable gfx950 device
 *     fmcw_ctx_create fails with FMCW_E_HIP.
 */
#ifndef FMCW_H_
#define FMCW_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: FMCW_PIPE_ONEPASS names the XCD-team schedule (E_ARG where the XCD census fails),
 *    fmcw_default_devices, FMCW_JSON_BOOL
 * 4: + the CFAR entry points (fmcw_cfar_check, fmcw_cfar_alpha, fmcw_cfar_device, fmcw_cfar)
 *    and timing stage 10, added within ABI 4: nothing that existed changed
 *    + the signature entry points (fmcw_sig_check, fmcw_sig_device, fmcw_sig_db_device,
 *    fmcw_sig), added within ABI 4 in the same way
 *    + the clustering entry points (fmcw_cluster_check, fmcw_cluster_device, fmcw_cluster), the
 *    structs fmcw_cluster_params / fmcw_targets and timing stage 11, added within ABI 4 in the
 *    same way
 *    + the tracking entry points (fmcw_track_check, fmcw_track_state_bytes, fmcw_track_device,
 *    fmcw_track), the structs fmcw_track_params / fmcw_tracks and timing stage 12, added within
 *    ABI 4 in the same way
 *    + the clutter-filter entry points (fmcw_mti_check, fmcw_mti_ring, fmcw_mti_device, fmcw_mti),
 *    the struct fmcw_mti_params and timing stage 13, added within ABI 4 in the same way
 *    + the angle-of-arrival entry points (fmcw_aoa_check, fmcw_aoa_device, fmcw_aoa), the structs
 *    fmcw_aoa_params / fmcw_angles and timing stage 14, added within ABI 4 in the same way
 *    + the channel-combining entry points (fmcw_beam_check, fmcw_beam_steer, fmcw_beam_device,
 *    fmcw_beam), the struct fmcw_beam_params and timing stage 15, added within ABI 4 in the same way
 *    + the ordered-statistic CFAR entry points (fmcw_oscfar_check, fmcw_oscfar_alpha,
 *    fmcw_oscfar_device, fmcw_oscfar), the struct fmcw_oscfar_params and timing stage 16, added
 *    within ABI 4 in the same way
 *    + the range-angle entry points (fmcw_ra_check, fmcw_ra_steer, fmcw_cov_device, fmcw_ra_device,
 *    fmcw_ra), the struct fmcw_ra_params and timing stage 17, added within ABI 4 in the same way
 *    + the MUSIC entry points (fmcw_music_check, fmcw_music_device, fmcw_music), the struct
 *    fmcw_music_params and timing stage 18, added within ABI 4 in the same way
 *    + the direction-of-arrival entry points (fmcw_doa_check, fmcw_doa_device, fmcw_doa), the struct
 *    fmcw_doa_params, timing stage 19 and its reader fmcw_timing_read_ext, added within ABI 4 in the
 *    same way */
#define FMCW_ABI_VERSION 4

typedef enum fmcw_status {
  FMCW_OK = 0,
  FMCW_E_ARG = -1,          /* bad argument / unsupported size                */
  FMCW_E_HIP = -2,          /* HIP runtime failure (no device, launch, copy)   */
  FMCW_E_OOM = -3,          /* device allocation failed                        */
  FMCW_E_STATE = -4,        /* call order (e.g. fmcw_set_taps not called)      */
  FMCW_E_DATA = -5          /* data-dependent failure MATLAB would raise, e.g.
                               spectrogram of a signal shorter than the window */
} fmcw_status;

/* Element type of IQ input and of complex outputs. */
typedef enum fmcw_dtype {
  FMCW_C64 = 0,             /* complex float32, 8 B per sample                 */
  FMCW_C32H = 1             /* complex float16, 4 B per sample (storage only;
                               all arithmetic is float32).  fp16 OUTPUTS hold
                               MATLAB's values divided by the FFT sizes applied
                               so far (exact powers of two, to stay inside the
                               fp16 range): range cube X/nr, RD map D/(nr*nd) */
} fmcw_dtype;

/* Algorithm parameters: radar_processing.m:117-154 (a1 in SURVEY.md 8a). */
typedef struct fmcw_params {
  int32_t nts;                  /* NTS, ADC samples per chirp            :109 */
  int32_t pn;                   /* PN, chirps per frame                  :112 */
  int32_t nr;                   /* range_fft_size (power of 2, 16..2048) :118 */
  int32_t nd;                   /* Doppler_fft_size (power of 2, 2..1024):119 */
  int32_t max_targets;          /* max_num_targets (1..8)                :129 */
  int32_t doppler_fallback_idx; /* 1-based; the literal 9 of :234 in parity
                                   mode, nd/2+1 in throughput mode            */
  float if_scale;               /* IF_scale                          :121/136 */
  float range_thr;              /* range_threshold                       :123 */
  float doppler_thr;            /* Doppler_threshold                     :124 */
  float min_d;                  /* min_distance [m]                      :126 */
  float max_d;                  /* max_distance [m]                      :127 */
  float dist_per_bin;           /* dist_per_bin [m]                      :147 */
} fmcw_params;

typedef struct fmcw_ctx fmcw_ctx;

int32_t     fmcw_abi_version(void);
const char* fmcw_last_error(void);
int         fmcw_device_count(int32_t* n);
/* The devices a caller that names none should use ("device choice
 * comes from an env var or an explicit id"): the comma-separated ids of the
 * environment variable FMCW_DEVICES (e.g. "0,1,2,3"), or every visible device
 * when it is unset, empty or "all".  Writes up to cap ids to ids[], their count
 * to *n.  FMCW_E_ARG for a malformed list or an id that is not present.  The
 * MEX gateway's fmcw_mex('init') (no ids) and matlab/radar_processing.m use it,
 * so one MATLAB call drives every GPU of the node (radar_processing_with_azure.m:50
 * -> radar_processing.m:197). */
int         fmcw_default_devices(int32_t cap, int32_t* ids, int32_t* n);

/* Bind a context to n_devices HIP devices (device_ids[n_devices], or NULL for
 * 0 .. n_devices-1), each with its own streams, scratch and tables, all in the
 * calling process.  With several distinct devices the context also holds one
 * RCCL communicator per device (ncclCommInitAll; RCCL is loaded
 * at run time).  The host-pointer calls (fmcw_process, fmcw_range_fft,
 * fmcw_stft) then split their work over the devices -- contiguous frame
 * shards, each written back in place (the range_speed concatenation of
 * :386-389 is the frame order), and contiguous spectrogram segment shards with
 * the global max(P) of :282-283 taken by an RCCL all_reduce(max) -- so one MEX
 * call from the serial loop's caller (radar_processing_with_azure.m:50 ->
 * radar_processing.m:197) drives every GPU.  The device-pointer calls act on
 * the first device (one process per GPU for torch.distributed drivers).
 * Results do not depend on the number of devices (bit-identical shards). */
int fmcw_ctx_create(int32_t n_devices, const int32_t* device_ids, fmcw_ctx** out);
int fmcw_ctx_destroy(fmcw_ctx* ctx);
/* n_devices, device_ids[n_devices] (may be NULL), rccl_comms: 1 if RCCL communicators exist. */
int fmcw_ctx_devices(fmcw_ctx* ctx, int32_t* n_devices, int32_t* device_ids, int32_t* rccl_comms);

/* Window taps and calibration (radar_processing.m:138, :139, :174):
 *   range_win   [nts]        = 2*blackman(NTS)
 *   doppler_win [pn]         = 2*chebwin(PN)
 *   calib       [nts] c64    = calib_rx1
 * Those are the reference's taps; the taps themselves are arbitrary: no kernel assumes a
 * symmetric window, zero end points, or a calibration vector of constant modulus, linear phase
 * or zero mean (tests/test_gpu_taps.py runs windows and a calibration with none of these).
 * Also builds the twiddle tables for nr and nd.  Must precede processing and
 * be repeated whenever nts/pn/nr/nd change.  Synchronous with the device: work
 * queued before it (on any stream) finishes with the old taps, and calls after it
 * (on any stream) see the new ones. */
int fmcw_set_taps(fmcw_ctx* ctx, const fmcw_params* p, const float* range_win,
                  const float* doppler_win, const float* calib);

/* ---------------------------------------------------------------------------
 * Host-pointer API (MEX / ctypes).  Data are staged through device memory
 * owned by the context; the call returns when the outputs are on the host.
 * ------------------------------------------------------------------------- */

/* Per-frame stages a5-a11 + a13 of SURVEY 8a over F frames
 * (radar_processing.m:199-239, :257-259, :265).
 *   iq              [F][pn][nts]  in_dtype   cat(3, frame.Chirp(:,:,1))
 *   range_profile   [F][nr]  f32   range_tx1rx1_max_abs (:265, Nr x F)
 *   tgt_count       [F]      i32   num_of_targets (:213)
 *   tgt_range_idx   [F][M]   i32   tgt_range_idx, 1-based, 0 where j >= count
 *   tgt_range_mag   [F][M]   f32   tgt_range_mag
 *   tgt_doppler_idx [F][M]   i32   tgt_doppler_idx (:227-239), 1-based
 *   slow_mag        [F][pn]  f32   abs(range_tx1rx1_complete(ridx(1),:,fr)),
 *                                  the slow-time samples appended at :259 and
 *                                  made real at :270; zero where count == 0
 *   range_cube      [F][pn][nr] c64 or NULL   range_tx1rx1_complete (:207)
 *   rd_map          [F][nr][nd] c64 or NULL   range_Doppler_tx1rx1 (:219) for
 *                                  EVERY range row (the reference fills only the
 *                                  target rows; each row is the same row op).
 *                                  Note the per-frame transpose vs MATLAB's Nr x Nd.
 *   probe_column    1-based linear column of the Nr x (pn*F) view of the cube
 *                   (:410-411 uses 100), 0 = none
 *   probe_mag       [nr] f32 or NULL  abs(range_tx1rx1_complete(:, probe_column))
 */
int fmcw_process(fmcw_ctx* ctx, const fmcw_params* p, const void* iq, int32_t in_dtype,
                 int64_t F, float* range_profile, int32_t* tgt_count, int32_t* tgt_range_idx,
                 float* tgt_range_mag, int32_t* tgt_doppler_idx, float* slow_mag,
                 float* range_cube, float* rd_map, int64_t probe_column, float* probe_mag);

/* Range stage only (config 2): :203-205, :207, :210 -> cube + profile. */
int fmcw_range_fft(fmcw_ctx* ctx, const fmcw_params* p, const void* iq, int32_t in_dtype,
                   int64_t F, float* range_cube, float* range_profile);

/* STFT + dB + optional log-frequency resampling (:270-299).
 *   x [L] f32        iq_data = abs(slow_time_signal_all_frames)
 *   win [wlen]       kaiser(20,3) (:276) in parity mode
 *   noverlap         19 (:179); hop = wlen - noverlap
 *   nfft             0 = the reference rule 2^nextpow2(L) (:273)
 *   fs               1/PRT
 *   n_log_bins       1024 (:293) -> intensity is interp1 onto logspace bins;
 *                    0 -> intensity is 20log10(P/max P) on the nfft/2+1 bins
 *   out: T [nseg], freq [n_log_bins or nfft/2+1], intensity [nseg][nbins_out]
 *        (MATLAB's nbins_out x nseg matrix), nseg = fix((L-noverlap)/hop)
 *   Query sizes first with fmcw_stft_sizes.  Fails with FMCW_E_DATA when
 *   nseg < 1 (MATLAB's spectrogram raises on such input). */
int fmcw_stft_sizes(int64_t L, int32_t wlen, int32_t noverlap, int32_t nfft,
                    int32_t n_log_bins, int64_t* nseg, int32_t* nfft_used, int32_t* nbins_out);
int fmcw_stft(fmcw_ctx* ctx, const float* x, int64_t L, const float* win, int32_t wlen,
              int32_t noverlap, int32_t nfft, double fs, int32_t n_log_bins, float* T,
              float* freq, float* intensity);

/* ---------------------------------------------------------------------------
 * Device-pointer API (benches, multi-GPU driver).  All pointers are device
 * pointers on the context's device; `stream` is a hipStream_t (NULL = the
 * context's own stream).  Calls are asynchronous on that stream.
 * ------------------------------------------------------------------------- */
int fmcw_process_device(fmcw_ctx* ctx, const fmcw_params* p, const void* d_iq, int32_t in_dtype,
                        int64_t F, float* d_range_profile, int32_t* d_tgt_count,
                        int32_t* d_tgt_range_idx, float* d_tgt_range_mag,
                        int32_t* d_tgt_doppler_idx, float* d_slow_mag, void* d_range_cube,
                        void* d_rd_map, int32_t out_dtype, int64_t probe_column,
                        float* d_probe_mag, void* stream);

/* Placement (a performance note, not a requirement): the range kernel reads d_iq and writes
 * d_range_cube at the same time, and on MI355X its time depends on where the two streams sit
 * relative to each other in HBM -- 748-860 us per 4096 frames of 128 x 512 for 18 byte gaps between
 * the end of d_iq and the start of d_range_cube (profiles/r06_k1_place.txt).  Carving both from one
 * allocation with the cube 64 KiB (or 4-16 MiB) past the input's end measured at the fast end. */
int fmcw_range_fft_device(fmcw_ctx* ctx, const fmcw_params* p, const void* d_iq, int32_t in_dtype,
                          int64_t F, void* d_range_cube, int32_t out_dtype, float* d_range_profile,
                          void* stream);

/* fmcw_process_device (no range cube, no probe column) followed by the start of the slow-time
 * leg, in one call (ABI 4): the compaction of :257-260 -- d_frame_list / *d_len exactly as
 * fmcw_compact_device(d_tgt_count, F, pn, ...) -- and *d_pmax = 0 (when d_pmax != NULL) for the
 * STFT passes that follow (fmcw_stft_power_device's running max(P), :276 / :282).  On the
 * single-pass schedule both run inside the detection kernel (its last workgroup), so the leg
 * costs no launches of its own (the reference's :257-260 append and the spectrogram call
 * `radar_processing.m:259`, `:276`). */
int fmcw_process_slow_device(fmcw_ctx* ctx, const fmcw_params* p, const void* d_iq, int32_t in_dtype,
                             int64_t F, float* d_range_profile, int32_t* d_tgt_count,
                             int32_t* d_tgt_range_idx, float* d_tgt_range_mag,
                             int32_t* d_tgt_doppler_idx, float* d_slow_mag, void* d_rd_map,
                             int32_t out_dtype, int32_t* d_frame_list, int64_t* d_len, float* d_pmax,
                             void* stream);

/* Slow-time compaction (:257-260): exclusive scan of (tgt_count>0) over F
 * frames.  Writes d_frame_list[i] = i-th frame with a target, *d_len = L
 * (= pn * #frames with a target, int64, device). */
int fmcw_compact_device(fmcw_ctx* ctx, const int32_t* d_tgt_count, int64_t F, int32_t pn,
                        int32_t* d_frame_list, int64_t* d_len, void* stream);

/* Power spectrogram of the compacted |slow| signal, segments [0, nseg) with
 * nseg = fix((L + H - noverlap)/hop) clipped to max_seg (all on device):
 * sample q < L is slow_mag[frame_list[q/pn]][q%pn], q >= L is d_halo[q-L].
 * H = *d_halo_len when d_halo_len != NULL (device int64, <= n_halo), else
 * n_halo.  The halo carries the first samples of the following shards in the
 * multi-GPU split of the concatenated slow-time signal (:259).
 *   d_P [max_seg][nfft/2+1]  MATLAB P (psd scaling, one-sided); NULL: only max(P) is formed
 *   d_pmax                   running max of P (float, atomically raised;
 *                            initialise to 0 before the first call)
 *   d_nseg                   int64 device: segments actually written */
int fmcw_stft_power_device(fmcw_ctx* ctx, const float* d_slow_mag, const int32_t* d_frame_list,
                           const int64_t* d_len, int32_t pn, const float* d_halo, int32_t n_halo,
                           const int64_t* d_halo_len, const float* d_win, int32_t wlen, int32_t noverlap, int32_t nfft,
                           double fs, int64_t max_seg, float* d_P, float* d_pmax,
                           int64_t* d_nseg, void* stream);

/* psd = 20*log10(P / pmax) (:282-283), optionally resampled onto n_log_bins
 * logspace bins (:293-299).  d_out [max_seg][n_log_bins or nfft/2+1]; may
 * alias d_P when n_log_bins == 0. */
int fmcw_stft_db_device(fmcw_ctx* ctx, const float* d_P, const int64_t* d_nseg, int64_t max_seg,
                        int32_t nfft, double fs, const float* d_pmax, int32_t n_log_bins,
                        float* d_out, void* stream);

/* Second pass of the two-pass STFT without a stored P (20-tap window, hop <= 4,
 * linear bins only): recomputes P of every segment and writes
 * psd = 20*log10(P / max) (:283) to d_out [max_seg][nfft/2+1].  With
 * fmcw_stft_power_device(..., d_P = NULL, ...) as the first pass (max(P) only)
 * the P map is never written to or read back from HBM.  Same inputs as the power
 * call; d_pmax is the (all-reduced) max. */
int fmcw_stft_db_direct_device(fmcw_ctx* ctx, const float* d_slow, const int32_t* d_list, const int64_t* d_len,
                               int32_t pn, const float* d_halo, int32_t n_halo, const int64_t* d_halo_len,
                               const float* d_win, int32_t wlen, int32_t noverlap, int32_t nfft, double fs,
                               int64_t max_seg, const float* d_pmax, float* d_out, void* stream);

/* Synthetic IQ frames of SURVEY 8d (seed 0xF3C0 ^ global frame index),
 * generated in place in HBM: d_iq [F][pn][nts] of dtype.  Bench input only. */
int fmcw_synth_device(fmcw_ctx* ctx, const fmcw_params* p, int64_t frame0, int64_t F,
                      void* d_iq, int32_t dtype, void* stream);

/* Per-stage device timing with HIP events on the launching streams.
 * enable: 0 off; 1 = the range+Doppler span of each fmcw_process_device call
 * (stage 7: event before the first range launch .. event after the last
 * Doppler launch; the chunks run as a 3-stream software pipeline) and one pair
 * per STFT-side launch (stages 3-6); 2 = additionally one pair per K1/K2/K3; 3 = only the
 * dominant kernel's launches (stage 8 k_rdx, stage 6 range-only K1), the cheapest form for a
 * timed run (each event pair costs the stream a few microseconds).
 * stage: 0 range, 1 doppler, 2 detect, 3 compact, 4 stft_power, 5 stft_db,
 *        6 range_only, 7 range+Doppler span, 8 k_rdx (single-pass schedule,
 *        level 2), 9 render (spectrogram.png), 10 cfar (one pair per k_cfar + k_cfar_gather
 *        launch pair of fmcw_cfar_device), 11 cluster (one pair per k_cluster launch of
 *        fmcw_cluster_device), 12 track (one pair per k_track launch of fmcw_track_device),
 *        13 mti (one pair per fmcw_mti_device call's k_mti + k_mti_seen launches), 14 aoa (one pair
 *        per k_aoa launch of fmcw_aoa_device), 15 beam (one pair per k_beam launch of
 *        fmcw_beam_device), 16 oscfar (one pair per k_oscfar + k_cfar_gather + k_oscfar_select
 *        launch group of fmcw_oscfar_device), 17 ra (one pair per k_cov launch of fmcw_cov_device
 *        and one per k_ra launch of fmcw_ra_device), 18 music (one pair per k_music launch of
 *        fmcw_music_device), 19 doa (one pair per k_doa launch of fmcw_doa_device).
 *        fmcw_timing_read synchronises.  It answers for the stages 0..18 and keeps returning FMCW_E_ARG
 *        for any other, 19 included: callers written against stage 18 as the last one see no change.
 *        fmcw_timing_read_ext is the same call for every stage, 0..19.  fmcw_timing_reset clears all. */
int fmcw_timing_enable(fmcw_ctx* ctx, int32_t enable);
int fmcw_timing_read(fmcw_ctx* ctx, int32_t stage, double* total_ms, int64_t* launches);
int fmcw_timing_read_ext(fmcw_ctx* ctx, int32_t stage, double* total_ms, int64_t* launches);
int fmcw_timing_reset(fmcw_ctx* ctx);

/* Frames per range/Doppler chunk of the 3-stream pipeline (the range cube of
 * one chunk is its only intermediate; default 256 MiB of cube per chunk).
 * 0 restores the default. */
int fmcw_set_chunk_frames(fmcw_ctx* ctx, int64_t frames);

/* Schedule of fmcw_process_device / fmcw_process (the two agree to fp32 rounding):
 *  FMCW_PIPE_AUTO    the single-pass XCD-team schedule where it applies (geometry
 *                    and device below, no range cube requested), else the streams
 *                    schedule;
 *  FMCW_PIPE_STREAMS K1 | K2 | K3 kernels as a 3-stream chunk pipeline, the
 *                    range cube of each chunk round-trips through HBM;
 *  FMCW_PIPE_XCD     the XCD-team single pass (kernels_xcd.hip): the 32 CUs of each
 *                    XCD share a frame (range FFT split by chirps, Doppler FFT by
 *                    range-bin groups, the cube handed over in the XCD's L2), so
 *                    every input byte is read once and the range cube never goes
 *                    to HBM.  Needs nr 1024, pn == nd == 256, even nts <= nr, the RD
 *                    map (if any) in the IQ dtype (complex64 or fp16 storage), no
 *                    range cube (else E_ARG).  One persistent workgroup per CU: needs
 *                    32 CUs per XCD and a grid of one workgroup per CU dealt 32 per
 *                    XCD -- any XCD count, so the SPX mode (8 XCDs) and the DPX /
 *                    QPX / CPX partition modes (4 / 2 / 1 XCDs per device) alike;
 *                    checked once per context by a census, else E_ARG.  A hand-off
 *                    that does not complete within ~1 s is reported by
 *                    fmcw_synchronize (and the host-pointer calls) as FMCW_E_HIP.
 *  FMCW_PIPE_ONEPASS the same as FMCW_PIPE_XCD (ABI 2's 8-tile single pass, which
 *                    re-read every frame from L2 8 times, is retired).
 * (Value 2 is retired: the persistent "fused" schedule of ABI 1, slower than both.) */
enum { FMCW_PIPE_AUTO = 0, FMCW_PIPE_STREAMS = 1, FMCW_PIPE_ONEPASS = 3, FMCW_PIPE_XCD = 4 };
int fmcw_set_pipeline(fmcw_ctx* ctx, int32_t mode);

int fmcw_synchronize(fmcw_ctx* ctx);

/* Measurement helpers of the bench line (ABI 4; no part of the reference's path).
 * fmcw_rdx_clock: the effective shader clock (MHz) of the context's last k_rdx launch, from the
 *   shader-clock and 100 MHz stamps one member takes at its start and its end (*us: that span);
 *   0 when no launch ran.  Synchronises the device.
 * fmcw_copy_device: a 16-byte nontemporal copy of `bytes` (a multiple of 16, 16-byte aligned
 *   pointers), asynchronous on `stream`: the HBM copy ceiling of k_rdx's bytes (bench.py). */
int fmcw_rdx_clock(fmcw_ctx* ctx, double* mhz, double* us);
int fmcw_copy_device(fmcw_ctx* ctx, const void* d_src, void* d_dst, int64_t bytes, void* stream);

/* ---------------------------------------------------------------------------
 * 2-D cell-averaging CFAR over the range-Doppler map (added within ABI 4; beyond the
 * reference, whose only consumer of the map is the one-peak rule of :211 / :233).
 * Indices below are 0-based; every index the calls return is 1-based.
 *   rd [F][nr][nd]   the layout fmcw_process* writes: FMCW_C64, or FMCW_C32H (values
 *                    D/(nr*nd)); nr a power of two in 16..2048, nd one in 4..1024.
 *                    P[r][d] = re^2 + im^2 of the stored value.
 *   Training set of cell (r, d), with Wr = guard_r + train_r, Wd = guard_d + train_d:
 *     the cells (r + dr, (d + dd) mod nd) with |dr| <= Wr, |dd| <= Wd, not
 *     (|dr| <= guard_r and |dd| <= guard_d), and 0 <= r + dr < nr.  Doppler is circular,
 *     range is clipped: N(r) cells remain, S is the sum of P over them (formed by
 *     additions only, so relative error <= (N - 1) 2^-24).
 *   Test: a gated cell is a detection iff P > alpha * S / N.
 *   FMCW_CFAR_LOCAL_MAX: it must also be the maximum of its 3 x 3 neighbourhood (circular
 *     in Doppler, clipped in range, gated or not): P > the four neighbours before it in
 *     raster order, P >= the four after it, so a two-cell plateau keeps one cell.
 *   Constraints: guards, trains >= 0; train_r + train_d >= 1; Wr, Wd <= 16;
 *     2 Wr + 1 <= nr; 2 Wd + 1 <= nd; alpha > 0; 1 <= r_lo <= r_hi <= nr or r_lo = r_hi = 0
 *     (all rows); max_det in 1..1024.
 *   Outputs per frame (K = max_det):
 *     det_count [F] i32          detections found; may exceed K (the list was cut)
 *     det_range_idx, det_doppler_idx [F][K] i32   1-based, ascending (range, doppler); the
 *                                first K in that order; 0 where unused
 *     det_power, det_noise [F][K] f32   P and S/N in the units of |range_Doppler_tx1rx1|^2
 *                                (fp16 storage: times (nr*nd)^2, exact); 0 where unused
 *     mask [F][nr][nd] u8 or NULL   1 where a cell is a detection; not cut at K
 *   Results are bit-identical from call to call and do not depend on F.
 * ------------------------------------------------------------------------- */
enum { FMCW_CFAR_LOCAL_MAX = 1 };
typedef struct fmcw_cfar_params {
  int32_t guard_r, guard_d, train_r, train_d;
  int32_t r_lo, r_hi;      /* 1-based inclusive gate, 0/0 = all rows */
  int32_t max_det;         /* 1..1024 */
  int32_t flags;           /* FMCW_CFAR_LOCAL_MAX */
  float   alpha;           /* linear power ratio, > 0 */
} fmcw_cfar_params;

/* Host only, no context.  fmcw_cfar_check: FMCW_E_ARG (with a message) for any violation of
 * the constraints above; on success *n_train_full (may be NULL) = the full window's
 * training-cell count (2Wr+1)(2Wd+1) - (2 guard_r+1)(2 guard_d+1).
 * fmcw_cfar_alpha: alpha = N (pfa^(-1/N) - 1), the cell-averaging rule for exponentially
 * distributed noise power; FMCW_E_ARG unless 0 < pfa < 1 and n_train >= 1. */
int fmcw_cfar_check(const fmcw_cfar_params* q, int32_t nr, int32_t nd, int32_t* n_train_full);
int fmcw_cfar_alpha(int32_t n_train, double pfa, float* alpha);

/* Device pointers (d_rd 16-byte aligned), asynchronous on `stream`; needs no fmcw_set_taps.
 * Acts on the context's first device. */
int fmcw_cfar_device(fmcw_ctx* ctx, const fmcw_cfar_params* q, const void* d_rd, int32_t rd_dtype,
                     int64_t F, int32_t nr, int32_t nd, int32_t* d_det_count,
                     int32_t* d_det_range_idx, int32_t* d_det_doppler_idx, float* d_det_power,
                     float* d_det_noise, uint8_t* d_mask, void* stream);

/* Host pointers: staged through context memory, frames sharded over the context's devices
 * (bit-identical shards); returns when the outputs are on the host. */
int fmcw_cfar(fmcw_ctx* ctx, const fmcw_cfar_params* q, const void* rd, int32_t rd_dtype, int64_t F,
              int32_t nr, int32_t nd, int32_t* det_count, int32_t* det_range_idx,
              int32_t* det_doppler_idx, float* det_power, float* det_noise, uint8_t* mask);

/* ---------------------------------------------------------------------------
 * 2-D ordered-statistic CFAR (OS-CFAR) over the range-Doppler map (added within ABI 4).  The
 * cell-averaging threshold above is the window's mean, so one strong return in a neighbour's
 * window lifts that neighbour's threshold by P_strong / N and hides a weak target next to it; an
 * order statistic of the window does not move.  Window, gate, flags, list format and mask are
 * fmcw_cfar's (`win`, under fmcw_cfar_check's constraints).  Indices below are 0-based; every
 * index the calls return is 1-based.
 *   Power: P[r][d] = fl(fl(re re) + fl(im im)) of the stored value in float32, every operation
 *     rounded on its own (no fused multiply-add).  fp16 storage is widened exactly and multiplied
 *     by (float)nr (float)nd (a power of two, exact) before squaring.  k_cfar may contract its
 *     multiply-add, so these powers may differ from fmcw_cfar's det_power in the last bit.
 *   Training set: exactly fmcw_cfar's.  N_full is the full window's count, N(r) row r's clipped one.
 *   Rank: `rank` in 1..N_full.  Row r uses k(r) = 1 + ((rank - 1) (N(r) - 1)) / (N_full - 1) by
 *     integer division (k = 1 when N_full = 1): 1 -> 1, N_full -> N(r), a clipped window keeps the
 *     same quantile.
 *   Test: a gated cell is a detection iff #{training cells x : fl(alpha x) < P} >= k(r).  fl(alpha .)
 *     is monotone, so this is exactly P > fl(alpha X_(k)), X_(k) the k-th smallest training power
 *     (ties counted): compares only, no sort and no float sum.
 *   FMCW_CFAR_LOCAL_MAX keeps its meaning.
 *   Outputs as for fmcw_cfar: det_count, the lists (ascending (range, doppler), cut at max_det
 *     while the count is full, 0 where unused) and the optional mask (not cut).  det_power = P;
 *     det_noise = X_(k), one of the input powers bit for bit.  The lists feed fmcw_cluster*,
 *     fmcw_aoa* and the rest unchanged.
 *   With finite input every output byte equals a float32 evaluation of the rules above, for any F
 *   and however a host call is sharded or chunked.  A non-finite stored value makes the outcome of
 *   the cells whose window holds it unspecified and touches nothing else.
 *   Measured on one MI355X: DESIGN.md 4.11 (profiles/oscfar_bench.json).
 * ------------------------------------------------------------------------- */
typedef struct fmcw_oscfar_params {
  fmcw_cfar_params win;    /* window, gate, max_det, flags and alpha, under fmcw_cfar's rules */
  int32_t rank;            /* 1..N_full */
} fmcw_oscfar_params;

/* Host only, no context.  fmcw_oscfar_check: fmcw_cfar_check on `win`, then 1 <= rank <= N_full;
 * FMCW_E_ARG with a message for any violation; on success *n_train_full (may be NULL) = N_full.
 * fmcw_oscfar_alpha: for exponentially distributed noise power the k-th of N training powers gives
 * Pfa = prod_{i=0}^{k-1} (N - i) / (N - i + alpha); solved for alpha in double precision (bisection
 * on ln Pfa) and returned as float.  FMCW_E_ARG unless 0 < pfa < 1 and 1 <= rank <= n_train. */
int fmcw_oscfar_check(const fmcw_oscfar_params* q, int32_t nr, int32_t nd, int32_t* n_train_full);
int fmcw_oscfar_alpha(int32_t n_train, int32_t rank, double pfa, float* alpha);

/* Device pointers (d_rd 16-byte aligned), asynchronous on `stream`; needs no fmcw_set_taps.  Acts
 * on the context's first device.  F = 0 is a no-op.  The call is cut into launch groups by
 * fmcw_cfar_device's list-scratch budget. */
int fmcw_oscfar_device(fmcw_ctx* ctx, const fmcw_oscfar_params* q, const void* d_rd, int32_t rd_dtype,
                       int64_t F, int32_t nr, int32_t nd, int32_t* d_det_count,
                       int32_t* d_det_range_idx, int32_t* d_det_doppler_idx, float* d_det_power,
                       float* d_det_noise, uint8_t* d_mask, void* stream);

/* Host pointers: staged, sharded over the context's devices and chunked as fmcw_cfar is
 * (bit-identical shards and chunks); returns when the outputs are on the host. */
int fmcw_oscfar(fmcw_ctx* ctx, const fmcw_oscfar_params* q, const void* rd, int32_t rd_dtype, int64_t F,
                int32_t nr, int32_t nd, int32_t* det_count, int32_t* det_range_idx,
                int32_t* det_doppler_idx, float* det_power, float* det_noise, uint8_t* mask);

/* ---------------------------------------------------------------------------
 * Doppler-time (micro-Doppler) and range-time signatures of the RD map (added within ABI 4;
 * beyond the reference, whose spectrogram of abs(slow_time) at one range bin, :258-270, loses
 * the sign of the velocity and joins chirps of different frames).  Indices below are 0-based;
 * every index argument is 1-based.
 *   rd [F][nr][nd]   as for fmcw_cfar_device (same dtypes, size limits and 16-byte alignment).
 *                    P[r][d] = re^2 + im^2 of the stored value; fp16 storage: times (nr*nd)^2
 *                    (exact), so the outputs are in the units of |range_Doppler_tx1rx1|^2.
 *   Rows of frame f: without a centre array, the gate r_lo..r_hi.  With one,
 *     c = d_center[f * center_stride] is a 1-based row (0: the frame has no target):
 *     the rows c-1-track_half .. c-1+track_half intersected with the gate; c = 0, an empty
 *     intersection or a c outside 0..nr (never read through): no rows.  d_tgt_range_idx of
 *     fmcw_process* with center_stride = max_targets follows the strongest target (:258).
 *   doppler_time [F][nd]   sum of P[r][d] over the frame's rows
 *   range_time   [F][nr]   sum of P[r][d] over the Doppler bins d that are not left out
 *                          (circular |d - nd/2| <= dc_half is left out: zero Doppler sits at
 *                          bin nd/2 after the fftshift of :219), for the frame's rows; 0 for
 *                          every other row.  A frame with no rows gives zeros in both.
 *   Either map may be NULL, not both.
 *   Every output is a sum of non-negative terms by additions only (no guard band is
 *   subtracted from a full sum): within (N + 8) 2^-24 relative of the exact sum of the
 *   stored values, N the number of cells summed.  Results are bit-identical from call to
 *   call and do not depend on F or on how a host call is sharded or chunked.
 *   d_dt_max / d_rt_max (device floats or NULL): running maxima of everything written to
 *   the corresponding map, raised atomically; the caller zeroes them first.
 *   Constraints: 1 <= r_lo <= r_hi <= nr or r_lo = r_hi = 0 (all rows); track_half in
 *     0..64; dc_half >= -1 (-1 leaves no bin out) and 2 dc_half + 1 < nd; floor_db finite
 *     and < 0; no unknown flag bits.
 *   Measured on one MI355X over 4096 frames of 1024 x 256, every row, both maps
 *   (profiles/sig_bench.json, 2026-10-19): 1.50 ms for FMCW_C64 and 0.77 ms for FMCW_C32H,
 *   beside 2.63 / 1.32 ms for fmcw_copy_device on the same RD bytes in the same run
 *   (DESIGN.md 4.5).
 * ------------------------------------------------------------------------- */
enum { FMCW_SIG_DB = 1 };           /* host call only: outputs in dB, see fmcw_sig */
typedef struct fmcw_sig_params {
  int32_t r_lo, r_hi;      /* 1-based inclusive range gate, 0/0 = all rows */
  int32_t track_half;      /* used only with a centre array; 0..64 */
  int32_t dc_half;         /* range-time map: Doppler bins left out around nd/2; -1 = none */
  int32_t flags;           /* FMCW_SIG_DB */
  float   floor_db;        /* < 0, finite; lower clamp of the dB outputs */
} fmcw_sig_params;

/* Host only, no context: FMCW_E_ARG (with a message) for any violation of the constraints. */
int fmcw_sig_check(const fmcw_sig_params* q, int32_t nr, int32_t nd);

/* Device pointers (d_rd 16-byte aligned), asynchronous on `stream`; needs no fmcw_set_taps.
 * Acts on the context's first device.  FMCW_SIG_DB is ignored here.  F = 0 is a no-op. */
int fmcw_sig_device(fmcw_ctx* ctx, const fmcw_sig_params* q, const void* d_rd, int32_t rd_dtype,
                    int64_t F, int32_t nr, int32_t nd, const int32_t* d_center, int32_t center_stride,
                    float* d_doppler_time, float* d_range_time, float* d_dt_max, float* d_rt_max,
                    void* stream);

/* out[i] = max(10 log10(map[i] / *d_max), floor_db) with log10f; floor_db where map[i] == 0
 * or *d_max == 0.  d_out may alias d_map. */
int fmcw_sig_db_device(fmcw_ctx* ctx, const float* d_map, int64_t n, const float* d_max, float floor_db,
                       float* d_out, void* stream);

/* Host pointers: staged, sharded over the context's devices and chunked as fmcw_cfar is
 * (bit-identical).  center: a host array or NULL.  *dt_max / *rt_max (may be NULL) always
 * receive the global maxima of the two linear maps.  With FMCW_SIG_DB both maps come back in
 * dB relative to their global maximum (a second pass after the maxima are combined, the order
 * of :282-283), clamped at floor_db. */
int fmcw_sig(fmcw_ctx* ctx, const fmcw_sig_params* q, const void* rd, int32_t rd_dtype, int64_t F,
             int32_t nr, int32_t nd, const int32_t* center, int32_t center_stride, float* doppler_time,
             float* range_time, float* dt_max, float* rt_max);

/* ---------------------------------------------------------------------------
 * Targets from the CFAR detection lists: clustering, centroids, extents (added within ABI 4;
 * the reference's product is one range and one speed per target and frame, range_speed of
 * :241-252 / :385-389, which it takes from the one-peak rule; this stage forms it from the CFAR
 * cells).  It works on the lists fmcw_cfar* wrote, never on the RD map or the mask: O(F max_det)
 * bytes, no RD dtype.  Every index is 1-based.
 *   Input of frame f: the first n = clamp(det_count[f], 0, max_det) entries of det_range_idx,
 *     det_doppler_idx, det_power [F][max_det] and, optionally, det_noise, exactly as fmcw_cfar*
 *     writes them: ascending (range, Doppler), powers finite and >= 0.  det_count[f] > max_det
 *     means the list was cut: the targets are those of its first max_det cells.  On input that
 *     breaks this the result is unspecified, but nothing is read or written out of bounds (the
 *     indices are only ever compared, never used as addresses) and the call still ends.
 *   Linking: cells i, j are linked iff |r_i - r_j| <= link_r and
 *     min(|d_i - d_j|, nd - |d_i - d_j|) <= link_d (Doppler is circular, range is not, as in
 *     CFAR).  (1, 1) is 8-connectivity; (0, 0) makes every cell its own cluster.  A cluster is a
 *     connected component of this graph; its label is the smallest list index in it.
 *   Per cluster, every sum in ascending list order, delta_i = ((d_i - d_pk + nd/2) mod nd) - nd/2:
 *     cells             the member count
 *     peak_range_idx, peak_doppler_idx, peak_power, peak_noise
 *                       the member with the largest det_power (ties: the smallest list index);
 *                       peak_noise is its det_noise, 0 without that array
 *     power             sum of P_i
 *     range             r_pk + sum P_i (r_i - r_pk) / power          (r_pk where power is 0)
 *     doppler           d_pk + sum P_i delta_i / power, brought into [0.5, nd + 0.5) by +- nd
 *     extent_r          r_max - r_min + 1
 *     extent_d          max delta - min delta + 1
 *   Clusters with cells < min_cells are dropped; the rest are ordered by peak_power descending,
 *   ties by label ascending.  tgt_count[f] is their full number (it may exceed max_tgt); the first
 *   max_tgt are written, unused entries are 0 in every array.
 *   det_label [F][max_det] i32 (optional): entry i < n gets the 1-based place of its target in
 *   that order (it may exceed max_tgt), 0 when its cluster was dropped; unused entries get 0.
 *   Constraints: link_r, link_d in 0..8; 2 link_d + 1 <= nd; min_cells in 1..1024; max_tgt in
 *     1..64; max_det in 1..1024; nr, nd within CFAR's limits; flags 0 (no bit is defined).
 *   Results are bit-identical from call to call and do not depend on F or on how a host call is
 *   sharded or chunked: integer steps decide the partition, the peak and the order, and the sums
 *   are formed one member after the other in list order (no float atomics).  power is within
 *   (n + 8) 2^-24 relative of the exact sum, n the cluster's cell count.
 *   Measured on one MI355X on the CFAR lists of 4096 frames of 1024 x 256, link (1, 1), min_cells 2,
 *   max_tgt 16 (profiles/cluster_bench.json, 2026-10-19, tree 72a1213+): 0.018 ms at 12.5 cells per
 *   frame (pfa 1e-6, max_det 64) and 0.208 ms at 476 cells per frame (pfa 1e-3, max_det 1024), beside
 *   8.36 / 10.17 ms for the fmcw_cfar_device call that wrote the lists and 0.005 / 0.014 ms for
 *   fmcw_copy_device over the bytes the stage reads and writes, in the same run.
 * ------------------------------------------------------------------------- */
typedef struct fmcw_cluster_params {
  int32_t link_r, link_d;  /* 0..8 */
  int32_t min_cells;       /* 1..1024 */
  int32_t max_tgt;         /* 1..64 */
  int32_t flags;           /* 0 */
} fmcw_cluster_params;

/* Output pointers, [F][max_tgt] each but tgt_count [F]; any member except tgt_count may be NULL. */
typedef struct fmcw_targets {
  int32_t* tgt_count;
  int32_t* cells;
  int32_t* peak_range_idx;
  int32_t* peak_doppler_idx;
  int32_t* extent_r;
  int32_t* extent_d;
  float*   peak_power;
  float*   peak_noise;
  float*   power;
  float*   range;
  float*   doppler;
} fmcw_targets;

/* Host only, no context: FMCW_E_ARG (with a message) for any violation of the constraints. */
int fmcw_cluster_check(const fmcw_cluster_params* q, int32_t nr, int32_t nd, int32_t max_det);

/* Device pointers (the members of *d_out are device pointers, the struct itself is read on the host),
 * asynchronous on `stream`; needs no fmcw_set_taps.  Acts on the context's first device.  F = 0 is a
 * no-op.  FMCW_E_ARG is returned before any launch: the outputs are then untouched.  d_det_noise and
 * d_det_label may be NULL. */
int fmcw_cluster_device(fmcw_ctx* ctx, const fmcw_cluster_params* q, int64_t F, int32_t nr, int32_t nd,
                        int32_t max_det, const int32_t* d_det_count, const int32_t* d_det_range_idx,
                        const int32_t* d_det_doppler_idx, const float* d_det_power, const float* d_det_noise,
                        const fmcw_targets* d_out, int32_t* d_det_label, void* stream);

/* Host pointers: staged, sharded over the context's devices and chunked as fmcw_cfar is
 * (bit-identical shards); returns when the outputs are on the host. */
int fmcw_cluster(fmcw_ctx* ctx, const fmcw_cluster_params* q, int64_t F, int32_t nr, int32_t nd, int32_t max_det,
                 const int32_t* det_count, const int32_t* det_range_idx, const int32_t* det_doppler_idx,
                 const float* det_power, const float* det_noise, const fmcw_targets* out, int32_t* det_label);

/* ---------------------------------------------------------------------------
 * Angle of arrival from several receive channels of the RD map (added within ABI 4; beyond the
 * reference, which parses numAntennasRx, :103, and keeps only frame.Chirp(:,:,1), :202).  For the
 * cells CFAR found and the targets clustering formed it takes the same cells from every channel's RD
 * map and turns the inter-channel phase into an angle.  The caller runs fmcw_set_taps + fmcw_process*
 * once per receive plane (each plane has its own calib_rx); RD -> MTI -> CFAR -> clusters are linear
 * or work on lists, so the phase relation between the planes' maps survives them.
 *   Input: A channel maps rd[a], a = 0..A-1, A in 2..8, each [F][nr][nd] in the layout fmcw_process*
 *     writes, all of one dtype, FMCW_C64 or FMCW_C32H; nr, nd within CFAR's limits.  The maps are
 *     given as a host array of A pointers (for the device call: device pointers; the array itself is
 *     read on the host, as fmcw_targets is), each 16-byte aligned; separate allocations or slices of
 *     one.  The detection lists exactly as fmcw_cfar* writes them: det_count [F], det_range_idx,
 *     det_doppler_idx [F][max_det], 1-based, max_det in 1..1024; optionally det_label [F][max_det]
 *     from fmcw_cluster*.  n = clamp(det_count[f], 0, max_det).
 *     Unlike clustering, the indices ARE used as addresses here: cell i < n is valid iff
 *     1 <= r <= nr and 1 <= d <= nd.  An invalid cell is never read through, gives zeros and joins no
 *     target.  Labels are only compared: a valid cell belongs to target t iff det_label == t with
 *     1 <= t <= max_tgt; a label of 0, a negative one or one above max_tgt belongs to no target.
 *   Parameters: n_chan = A; max_tgt 0 (no per-target outputs) or 1..64; flags 0; spacing, the element
 *     spacing in wavelengths, signed (the sign sets which side is positive), finite,
 *     0.01 <= |spacing| <= 16; w[16], a complex weight (re, im) per channel, finite, which absorbs the
 *     receive paths' phase and gain mismatch ((1, 0): none; entries of channels >= A are ignored).
 *     The host forms kinv = (float)(1.0 / (2 pi (double)spacing)).
 *   One cell, in float32, every operation rounded on its own in the order written (no fused
 *   multiply-add):
 *   1. x_a is the stored value of channel a at (r, d); fp16 storage is widened exactly.
 *      v_a.re = x.re w.re - x.im w.im;  v_a.im = x.re w.im + x.im w.re.
 *   2. From zr = zi = e0 = e1 = 0, for a = 0..A-2 with p = v_a, q = v_{a+1}:
 *      zr += (q.re p.re + q.im p.im);  zi += (q.im p.re - q.re p.im);
 *      e0 += (p.re^2 + p.im^2);        e1 += (q.re^2 + q.im^2).
 *      So z = sum v_{a+1} conj(v_a), the lag-1 spatial correlation: phase-comparison monopulse for
 *      A = 2, the power-weighted single-source estimator for a uniform line of A elements.
 *   3. Per-cell outputs [F][max_det], each optional:
 *      det_zre, det_zim   zr, zi times scale2, scale2 = ((float)nr (float)nd)^2 for FMCW_C32H and 1
 *                         otherwise (an exact power of two: the units of |range_Doppler|^2, as fmcw_sig)
 *      det_phase          atan2f(zi, zr) in (-pi, pi]; 0 when both are 0
 *      det_sin            clamp(det_phase kinv, -1, 1): sin(theta).  Bearings are unambiguous for
 *                         |sin(theta)| <= 1 / (2 |spacing|).
 *   One target: per-target outputs [F][max_tgt], each optional; they need det_label (a per-target
 *   output without det_label, or with max_tgt = 0, is FMCW_E_ARG).  Z = (sum zr, sum zi, sum e0,
 *   sum e1) over the target's valid cells in ascending list position, one cell after the other (no
 *   float atomics: the bits do not depend on the call, on F, on sharding or on chunking).
 *      tgt_zre, tgt_zim, tgt_e0, tgt_e1   the sums times scale2
 *      tgt_phase, tgt_sin                 as above, from the unscaled sums
 *      tgt_coh     min(1, sqrt(zr zr + zi zi) / (sqrt(e0) sqrt(e1))), 0 when e0 or e1 is 0; sqrt and
 *                  the divide correctly rounded
 *      tgt_cells   i32: the number of valid member cells
 *   A target with no valid member gets zeros.  Unused and invalid entries are 0 in every array.  At
 *   least one output must be non-NULL.
 *   A non-finite stored value or weight makes that cell's outputs, and its target's, unspecified; it
 *   touches nothing else and nothing out of bounds.  The call ends for any list, label and count
 *   bytes.
 *   The device's atan2f: the largest error seen on one MI355X over every value the tests and the bench
 *   compare is 1.93 ulp of the float32 result, against float64 atan2 of the same inputs.
 *   Measured on one MI355X on the CFAR lists of 4096 frames of 1024 x 256, labels from link (1, 1),
 *   min_cells 2, max_tgt 16, every output written (profiles/aoa_bench.json, 2026-10-20, tree d65bf9b+), A = 2 /
 *   A = 4: at 12.5 cells per frame (pfa 1e-6, max_det 64) 0.018 / 0.022 ms complex64 and 0.019 / 0.022 ms fp16
 *   storage; at 476 cells per frame (pfa 1e-3, max_det 1024) 0.113 / 0.174 ms complex64 and 0.113 / 0.187 ms
 *   fp16 storage; beside 8.35 / 10.18 ms for the fmcw_cfar_device call and 0.018 / 0.208 ms for the
 *   fmcw_cluster_device call that produced the lists and labels, and 0.005 / 0.034-0.049 ms for
 *   fmcw_copy_device over the bytes the stage reads and writes, in the same run: 2.9 to 4.8 times the copy's
 *   time, so the stage MISSES the copy-time yardstick; its time follows the number of gathered values, not
 *   their bytes.
 * ------------------------------------------------------------------------- */
typedef struct fmcw_aoa_params {
  int32_t n_chan;          /* 2..8 */
  int32_t max_tgt;         /* 0, or 1..64 */
  int32_t flags;           /* 0 */
  float   spacing;         /* wavelengths, signed; 0.01 <= |spacing| <= 16 */
  float   w[16];           /* (re, im) per channel */
} fmcw_aoa_params;

/* Output pointers: det_* [F][max_det], tgt_* [F][max_tgt]; any may be NULL, not all. */
typedef struct fmcw_angles {
  float*   det_zre;
  float*   det_zim;
  float*   det_phase;
  float*   det_sin;
  float*   tgt_zre;
  float*   tgt_zim;
  float*   tgt_e0;
  float*   tgt_e1;
  float*   tgt_phase;
  float*   tgt_sin;
  float*   tgt_coh;
  int32_t* tgt_cells;
} fmcw_angles;

/* Host only, no context: FMCW_E_ARG (with a message) for any violation of the constraints. */
int fmcw_aoa_check(const fmcw_aoa_params* q, int32_t nr, int32_t nd, int32_t max_det);

/* Device pointers (d_rd_ch[a] and the members of *d_out are device pointers; the array and the struct
 * themselves are read on the host), asynchronous on `stream`; needs no fmcw_set_taps.  Acts on the
 * context's first device.  F = 0 is a no-op.  FMCW_E_ARG is returned before any launch: the outputs
 * are then untouched.  d_det_label may be NULL. */
int fmcw_aoa_device(fmcw_ctx* ctx, const fmcw_aoa_params* q, const void* const* d_rd_ch, int32_t rd_dtype,
                    int64_t F, int32_t nr, int32_t nd, int32_t max_det, const int32_t* d_det_count,
                    const int32_t* d_det_range_idx, const int32_t* d_det_doppler_idx, const int32_t* d_det_label,
                    const fmcw_angles* d_out, void* stream);

/* Host pointers: staged (all A channels of a chunk), sharded over the context's devices and chunked
 * as fmcw_cfar is (bit-identical shards); returns when the outputs are on the host. */
int fmcw_aoa(fmcw_ctx* ctx, const fmcw_aoa_params* q, const void* const* rd_ch, int32_t rd_dtype, int64_t F,
             int32_t nr, int32_t nd, int32_t max_det, const int32_t* det_count, const int32_t* det_range_idx,
             const int32_t* det_doppler_idx, const int32_t* det_label, const fmcw_angles* out);

/* ---------------------------------------------------------------------------
 * Tracks from the per-frame targets: association, alpha-beta filter, ids (added within ABI 4; the
 * reference's deliverable range_speed, :241-252 / :385-389, is a time series of one range and one
 * speed per target, which needs to know which target of one frame is which target of the next).
 * Every index and id is 1-based, 0 means "none".
 *   Input: what fmcw_cluster* writes, never the RD map or the detection lists.  A call covers S
 *     independent sequences of F consecutive frames each; frame f of sequence s is row s*F + f of
 *     tgt_count [S*F] and of range, doppler, peak_power [S*F][max_tgt] (range, doppler: the cluster
 *     centroids in bins, float32).  n = clamp(tgt_count, 0, max_tgt).  Measurement j < n is valid iff
 *     range and doppler are finite, 0.5 <= range < nr + 0.5 and 0.5 <= doppler < nd + 0.5; an invalid
 *     measurement is ignored as if absent.  Measurement values are only compared and copied, never
 *     used as addresses.
 *   Parameters: gate_r, gate_d (bins) finite and > 0, gate_d < nd/2; alpha_r, alpha_d in (0, 1];
 *     beta_r in [0, 1]; confirm_hits in 1..255; max_coast in 0..255; max_trk in 1..64; flags 0;
 *     nr, nd within CFAR's limits; max_tgt in 1..64.  The host forms
 *     wr = float(1.0 / ((double)gate_r * gate_r)) and wd likewise.
 *   State: per sequence max_trk slots -- id, status (0 free, 1 tentative, 2 confirmed), hits,
 *     misses, age, r, v (bins per frame), d, power -- and an id counter, in
 *     fmcw_track_state_bytes(max_trk) bytes.  The layout is private, with two guarantees: an
 *     all-zero block is a fresh sequence, and a freed slot is all zero.  Gains may change between
 *     calls, max_trk may not.
 *   One frame step, in float32, every operation rounded on its own in the order written (no fused
 *   multiply-add):
 *   1. Predict.  For every live slot k: rp = r + v.  Doppler is not extrapolated.
 *   2. Cost.  For every pair (live slot k, valid measurement j): er = zr_j - rp_k; x = zd_j - d_k,
 *      then x -= nd if x >= nd/2, else x += nd if x < -nd/2; c = (er*er)*wr + (x*x)*wd.  The pair is
 *      admissible iff c <= 1.0f (NaN never is).
 *   3. Associate (greedy).  The admissible pairs in ascending order of the tuple (tentative slot ?
 *      1 : 0, bits of c, k, j); a pair is taken iff neither its slot nor its measurement is taken
 *      yet.  So confirmed tracks choose first, and ties go to the lower slot, then the lower j.
 *   4. Update.  A slot assigned to measurement j: if its hits are 1 (two-point start) r = zr_j,
 *      v = er, d = zd_j; otherwise r = rp + alpha_r*er, v = v + beta_r*er, dn = d + alpha_d*x, then
 *      one conditional dn -= nd if dn >= nd + 0.5 followed by one conditional dn += nd if dn < 0.5,
 *      d = dn.  In both cases power = zp_j, hits + 1, misses = 0, age + 1, and a tentative slot with
 *      hits >= confirm_hits becomes confirmed.  A live slot with no measurement: r = rp, misses + 1,
 *      age + 1; a tentative one is freed at once, a confirmed one when misses > max_coast.  A live
 *      slot whose r has left [0.5, nr + 0.5) is freed.
 *   5. Births.  The valid unassigned measurements, in ascending j, take the free slots in ascending
 *      k (slots freed in step 4 count).  The new slot: id = the sequence's counter pre-incremented
 *      (first id 1), tentative (confirmed when confirm_hits == 1), hits 1, misses 0, age 1, r = zr_j,
 *      v = 0, d = zd_j, power = zp_j.  With no slot free the measurement is dropped.
 *   6. Outputs of the frame, taken after step 5 (fmcw_tracks; [S*F][max_trk] each but trk_count
 *      [S*F]; any member but trk_count may be NULL): trk_count the number of confirmed slots;
 *      trk_id, trk_status, trk_age, trk_misses (i32) and trk_range, trk_range_rate, trk_doppler,
 *      trk_power (f32) the slot values, 0 for a free slot.  A track keeps its slot for life, so a
 *      column is a trajectory.  tgt_track [S*F][max_tgt] i32 (optional): the id of the track that
 *      measurement j updated or started, 0 if it was dropped, invalid or unused.
 *   Results are bit-identical from call to call.  A sequence's results do not depend on S or on
 *   which other sequences share the call.  F frames in one call equal any split into consecutive
 *   calls with the state carried, byte for byte, in every output and in the final state block.  For
 *   any input bytes and any state bytes the call ends and touches nothing out of bounds (a slot
 *   index is a lane index, n is clamped).
 *   Measured on one MI355X on the cluster outputs of 4096 frames of 1024 x 256, max_tgt 16, max_trk 16
 *   (profiles/track_bench.json, 2026-10-20, tree 0e93d61+): a frame step costs 1.3 us at 1.6 targets per
 *   frame and 2.9 us at 16, alone or with 63 other sequences beside it -- one sequence of 4096 frames
 *   5.36 / 11.73 ms, 64 sequences of 64 frames 0.090 / 0.190 ms -- beside 8.41 / 10.18 ms for the
 *   fmcw_cfar_device call and 0.018 / 0.205 ms for the fmcw_cluster_device call of the same run, and
 *   0.005-0.007 ms for fmcw_copy_device over the bytes the stage reads and writes: a dependency chain
 *   over frames, bound by latency, not by bytes.
 * ------------------------------------------------------------------------- */
typedef struct fmcw_track_params {
  float   gate_r, gate_d;  /* bins; finite, > 0; gate_d < nd/2 */
  float   alpha_r, alpha_d;/* (0, 1] */
  float   beta_r;          /* [0, 1] */
  int32_t confirm_hits;    /* 1..255 */
  int32_t max_coast;       /* 0..255 */
  int32_t max_trk;         /* 1..64 */
  int32_t flags;           /* 0 */
} fmcw_track_params;

/* Output pointers, [S*F][max_trk] each but trk_count [S*F]; any member except trk_count may be NULL. */
typedef struct fmcw_tracks {
  int32_t* trk_count;
  int32_t* trk_id;
  int32_t* trk_status;
  int32_t* trk_age;
  int32_t* trk_misses;
  float*   trk_range;
  float*   trk_range_rate;
  float*   trk_doppler;
  float*   trk_power;
} fmcw_tracks;

/* Host only, no context.  fmcw_track_check: FMCW_E_ARG (with a message) for any violation of the
 * constraints.  fmcw_track_state_bytes: the bytes of one sequence's state block (a multiple of 16,
 * growing with max_trk), or FMCW_E_ARG for a max_trk outside 1..64. */
int fmcw_track_check(const fmcw_track_params* q, int32_t nr, int32_t nd, int32_t max_tgt);
int32_t fmcw_track_state_bytes(int32_t max_trk);

/* Device pointers (the members of *d_out are device pointers, the struct itself is read on the host),
 * asynchronous on `stream`; needs no fmcw_set_taps.  Acts on the context's first device.
 * d_state [S][fmcw_track_state_bytes(max_trk)], 16-byte aligned, is read and rewritten in place.
 * F = 0 or S = 0 is a no-op.  FMCW_E_ARG is returned before any launch: the outputs and the state are
 * then untouched.  d_tgt_track may be NULL. */
int fmcw_track_device(fmcw_ctx* ctx, const fmcw_track_params* q, int64_t S, int64_t F, int32_t nr, int32_t nd,
                      int32_t max_tgt, const int32_t* d_tgt_count, const float* d_range, const float* d_doppler,
                      const float* d_peak_power, void* d_state, const fmcw_tracks* d_out, int32_t* d_tgt_track,
                      void* stream);

/* Host pointers.  state [S][fmcw_track_state_bytes(max_trk)] is read and rewritten, or NULL: the
 * sequences start fresh and their state is discarded.  Sequences, never frames, are sharded
 * contiguously over the context's devices; the frames are staged in chunks with the state kept on the
 * device between chunks (bit-identical, by the split guarantee above).  Returns when the outputs are
 * on the host. */
int fmcw_track(fmcw_ctx* ctx, const fmcw_track_params* q, int64_t S, int64_t F, int32_t nr, int32_t nd,
               int32_t max_tgt, const int32_t* tgt_count, const float* range, const float* doppler,
               const float* peak_power, void* state, const fmcw_tracks* out, int32_t* tgt_track);

/* ---------------------------------------------------------------------------
 * Frame-to-frame clutter filter (MTI) of the range-Doppler map (added within ABI 4; beyond the
 * reference, which has no moving-target step: the Doppler mean removal of :217-218 cancels only
 * what is constant within one frame).  A complex background per RD cell is learned recursively and
 * subtracted coherently: whatever repeats from frame to frame -- walls, rails, feeders and their
 * leakage into every Doppler bin -- goes, whatever changes its phase from frame to frame stays.
 * The output is an RD map in the layout and dtype of the input, so fmcw_cfar*, fmcw_sig* and
 * everything behind them take it unchanged.
 *   Input: rd [S*F][nr][nd] in the layout fmcw_process* writes, FMCW_C64 or FMCW_C32H: S
 *     independent sequences of F consecutive frames each; frame f of sequence s is frame s*F + f, as
 *     in fmcw_track.  nr, nd within CFAR's limits.
 *   State per sequence, public layout, always float32:
 *     bg   [S][nr][nd] complex64 interleaved: the background B, in the units of the stored values
 *          (fp16 storage: D/(nr*nd)).
 *     seen [S] int32: the number of frames absorbed.
 *     An all-zero bg with seen = 0 is a fresh sequence.  A caller may save the state, reload it and
 *     inspect it (which is why the layout is public, unlike the tracker's).
 *   Parameters: lambda finite, in (0, 1]; no unknown flag bit; FMCW_MTI_FREEZE together with a NULL
 *     output is FMCW_E_ARG (there would be nothing to do); RAMP with FREEZE is allowed, RAMP is then
 *     moot.
 *   One frame step for every cell, re and im handled separately, in float32, every operation rounded
 *   on its own in the order written (no fused multiply-add):
 *   1. x is the stored value; fp16 storage is widened exactly to float32.
 *   2. y = x - B.  The output cell of this frame is y; for FMCW_C32H it is converted with IEEE
 *      round-to-nearest-even, subnormals kept (exactly numpy's astype(float16)).
 *   3. Update, unless FMCW_MTI_FREEZE is set: n = clamp(seen, 0, 2^30); with FMCW_MTI_RAMP
 *      g = max(lambda, 1.0f / (float)(n + 1)), without it g = lambda; if g == 1.0f then B = x,
 *      otherwise t = g*y, then B = B + t.
 *   4. After the frame seen = min(n + 1, 2^30).  With FREEZE, B and seen are not touched.
 *   So lambda = 1 is the exact two-frame canceller D_f - D_{f-1}; RAMP starts as the running mean of
 *   the frames so far and goes over to the exponential average after about 1/lambda frames (from a
 *   fresh state frame 0 passes unchanged and B becomes frame 0 exactly); FREEZE subtracts a learned
 *   background without touching it ("learn the empty pen, then watch").
 *   Results are bit-identical from call to call.  A sequence's results do not depend on S or on which
 *   other sequences share the call.  F frames in one call equal any split into consecutive calls with
 *   bg / seen carried, byte for byte, in the output and in the final state.  For finite input every
 *   output and state bit equals the numpy float32 evaluation of the steps above (g has the bits of
 *   float32(1)/float32(n+1): a correctly rounded division).  A non-finite input value makes that
 *   cell's output and background unspecified from then on (NaN payloads differ between hosts and the
 *   GPU); it touches no other cell and nothing out of bounds.
 *   Measured on one MI355X over 4096 frames of 1024 x 256, S = 1 (profiles/mti_bench.json, 2026-10-20,
 *   tree ad9069a+), beside fmcw_copy_device over the same RD bytes in the same run (2.64 ms FMCW_C64,
 *   1.31 ms FMCW_C32H), which reads and writes what the filter with an output reads and writes: to a
 *   second buffer 3.43 / 1.56 ms (1.30x / 1.19x the copy), in place 3.17 / 1.57 ms (1.20x / 1.20x), 64
 *   sequences of 64 frames 3.28 / 1.50 ms (1.24x / 1.14x): with an output the stage MISSES the
 *   copy-time yardstick by 14-30 %.  Learning only (no output, half the bytes) takes 1.40 / 0.65 ms,
 *   0.53x / 0.50x the copy against a goal of 0.5: it meets it in fp16 storage and misses it by 6 % in
 *   complex64 (what was tried, and what the evidence excludes as the bound).
 * ------------------------------------------------------------------------- */
enum { FMCW_MTI_RAMP = 1, FMCW_MTI_FREEZE = 2 };
typedef struct fmcw_mti_params {
  float   lambda;          /* (0, 1], finite */
  int32_t flags;           /* FMCW_MTI_RAMP | FMCW_MTI_FREEZE */
} fmcw_mti_params;

/* Host only, no context.  fmcw_mti_check: FMCW_E_ARG (with a message) for a lambda or flags outside
 * the rules above or nr / nd outside CFAR's limits.  fmcw_mti_ring: the number of frames U a lane of
 * k_mti keeps in flight ahead of the recursion for that dtype (the frame counts at which the kernel
 * changes path are U and 2U), or FMCW_E_ARG for an unknown dtype. */
int fmcw_mti_check(const fmcw_mti_params* q, int32_t nr, int32_t nd);
int32_t fmcw_mti_ring(int32_t rd_dtype);

/* Device pointers, each 16-byte aligned; asynchronous on `stream`; needs no fmcw_set_taps.  Acts on
 * the context's first device.  d_bg [S][nr][nd] complex64 and d_seen [S] are read and rewritten in
 * place.  d_out has the dtype of d_rd; d_out == d_rd (in place) is allowed (a lane writes only the
 * addresses it has already read), a partial overlap is FMCW_E_ARG; d_out == NULL learns the
 * background and writes no map.  F = 0 or S = 0 is a no-op.  FMCW_E_ARG is returned before any
 * launch: the outputs and the state are then untouched. */
int fmcw_mti_device(fmcw_ctx* ctx, const fmcw_mti_params* q, const void* d_rd, int32_t rd_dtype,
                    int64_t S, int64_t F, int32_t nr, int32_t nd, float* d_bg, int32_t* d_seen,
                    void* d_out, void* stream);

/* Host pointers.  bg and seen are both given (read and rewritten) or both NULL: the sequences start
 * fresh and the state is discarded.  out may be NULL (learn only).  Sequences, never frames, are
 * sharded contiguously over the context's devices (S = 1 runs on the first device); the frames are
 * staged in chunks with bg / seen kept on the device between chunks (bit-identical, by the split
 * guarantee above).  Returns when the outputs are on the host. */
int fmcw_mti(fmcw_ctx* ctx, const fmcw_mti_params* q, const void* rd, int32_t rd_dtype,
             int64_t S, int64_t F, int32_t nr, int32_t nd, float* bg, int32_t* seen, void* out);

/* ---------------------------------------------------------------------------
 * Receive channels combined: beamformed and channel-integrated RD maps (added within ABI 4; beyond
 * the reference, which parses numAntennasRx, :103, and keeps only frame.Chirp(:,:,1), :202).  The A
 * channels' maps become B maps to detect on: B steered beams (coherent), or one map of the summed
 * channel power (non-coherent integration).  Every output is an RD map in the layout and dtype of the
 * input, so fmcw_mti*, fmcw_cfar*, fmcw_sig*, clustering, fmcw_aoa* and tracking take it unchanged.
 *   Input: A channel maps rd[a], a = 0..A-1, A in 2..8, each [F][nr][nd] in the layout fmcw_process*
 *     writes, all of one dtype, FMCW_C64 or FMCW_C32H; nr, nd within CFAR's limits.  The maps are
 *     given as a host array of A pointers (for the device call: device pointers, each 16-byte
 *     aligned; the array itself is read on the host); separate allocations or slices of one, exactly
 *     as fmcw_aoa takes them.
 *   Output: B maps out[b], b = 0..B-1, B in 1..8, of the same shape and dtype, given as a host array
 *     of B pointers.  out[b] may be exactly one of the rd[a] (in place); any partial overlap of an
 *     output with an input or with another output, and two outputs at the same address, are
 *     FMCW_E_ARG.
 *   Parameters: n_chan = A, n_beam = B; flags 0 (coherent) or FMCW_BEAM_NCI, which needs n_beam == 1;
 *     an unknown flag bit is FMCW_E_ARG; w[b][a], a complex float32 weight (re, im) per (beam,
 *     channel), finite; entries with a >= A or b >= B are ignored.
 *   One cell, coherent, in float32, every operation rounded on its own in the order written (no fused
 *   multiply-add).  For every beam b:
 *   1. x_a is the stored value of channel a; fp16 storage is widened exactly.
 *      t_a.re = x.re w.re - x.im w.im;  t_a.im = x.re w.im + x.im w.re,  with w = w[b][a].
 *   2. y = t_0; then y.re = y.re + t_a.re, y.im = y.im + t_a.im for a = 1..A-1, in ascending a.
 *   3. out[b] = y; for FMCW_C32H it is converted with IEEE round-to-nearest-even, subnormals kept,
 *      overflow to +-inf (exactly numpy's astype(float16)).
 *   One cell, FMCW_BEAM_NCI: t_a as above with w[0][a]; p = (t_0.re^2 + t_0.im^2), then
 *   p = p + (t_a.re^2 + t_a.im^2) in ascending a; out[0].re = sqrtf(p), correctly rounded,
 *   out[0].im = +0.  This is an amplitude map: CFAR's |.|^2 of it is the summed channel power to
 *   within rounding.  (It stays in the RD layout so that every later stage takes it; the unused
 *   imaginary half of the one written map is the price.)
 *   Results are bit-identical from call to call and do not depend on F, on sharding or on chunking.  A
 *   non-finite stored value or weight makes that cell's outputs unspecified; it touches nothing else.
 *   Measured on one MI355X over 4096 frames of 1024 x 256 per map, channel a = one RD map turned by
 *   0.6 a rad (profiles/beam_bench.json, 2026-10-21, tree e759450+), beside fmcw_copy_device over
 *   (A + B) / 2 maps' bytes in the same run, which reads and writes exactly the bytes the stage reads
 *   and writes; stage / copy in ms, complex64 then fp16 storage: (A, B) = (2, 1) 3.94 / 3.95 and
 *   1.94 / 1.96, (2, 1) NCI 3.93 / 3.94 and 1.94 / 1.96, (4, 4) 10.42 / 10.48 (complex64) MEET the
 *   copy-time yardstick, as does (2, 1) in place in fp16 storage, 1.95 / 1.96; (2, 1) in place in
 *   complex64 3.98 / 3.95, (4, 1) 6.77 / 6.49 and 3.40 / 3.27, (4, 4) fp16 5.32 / 5.22, (8, 1) 12.90 /
 *   11.86 and 6.35 / 5.86, (8, 8) complex64 21.41 / 20.95 MISS it by 1-9 %, and (8, 8) in fp16 storage
 *   14.92 / 10.55 MISSES it by 41 %: there the arithmetic, not HBM, sets the time.
 * ------------------------------------------------------------------------- */
enum { FMCW_BEAM_NCI = 1 };
typedef struct fmcw_beam_params {
  int32_t n_chan;          /* A, 2..8 */
  int32_t n_beam;          /* B, 1..8; 1 with FMCW_BEAM_NCI */
  int32_t flags;           /* 0 or FMCW_BEAM_NCI */
  float   w[8][8][2];      /* w[b][a]: (re, im) of beam b, channel a */
} fmcw_beam_params;

/* Host only, no context: FMCW_E_ARG (with a message) for any violation of the constraints. */
int fmcw_beam_check(const fmcw_beam_params* q, int32_t nr, int32_t nd);

/* Host only, no context: the weights of n_beam beams of a uniform line of n_chan elements, in the
 * convention of fmcw_aoa: channel a of a source at sin(theta) carries the phase
 * +2 pi spacing a sin(theta).  spacing as fmcw_aoa_params.spacing (wavelengths, signed, finite,
 * 0.01 <= |spacing| <= 16); sin_theta [n_beam], each in [-1, 1]; cal [n_chan][2] (re, im), the
 * per-channel calibration weights a caller gives fmcw_aoa, finite, or NULL (1); taper [n_chan], real,
 * finite, or NULL (1); normalize != 0 divides by sum taper_a (which must then not be 0), or by n_chan
 * without a taper, so that a plane wave from the look direction comes out at channel amplitude and
 * fp16 storage does not overflow.
 *   w[b][a] = cal_a (taper_a / norm) exp(-j 2 pi spacing a sin(theta_b)),
 * formed in double and rounded once to float32: t = -((double)spacing a sin_theta_b) in turns,
 * t = t - nearbyint(t), k = nearbyint(4 t), phi = (4 t - k) pi/2, e = (cos phi, sin phi) turned by k
 * exact quarter turns; g = cal_a (taper_a / norm); w = (g.re e.re - g.im e.im, g.re e.im + g.im e.re).
 * So every phase that is a whole number of quarter turns gives exactly 0 and +-1.
 * Sets q->n_chan, q->n_beam, q->flags = 0 and all of q->w (unused entries 0).  FMCW_E_ARG (with a
 * message, q untouched) for any violated constraint or a weight that does not fit float32. */
int fmcw_beam_steer(int32_t n_chan, int32_t n_beam, float spacing, const float* sin_theta, const float* cal,
                    const float* taper, int32_t normalize, fmcw_beam_params* q);

/* Device pointers (d_rd_ch[a] and d_out[b] are device pointers, each 16-byte aligned; the two arrays
 * and *q are read on the host), asynchronous on `stream`; needs no fmcw_set_taps.  Acts on the
 * context's first device.  F = 0 is a no-op.  FMCW_E_ARG is returned before any launch: the outputs
 * are then untouched.  In place is safe: a lane of k_beam stores only to the 16 bytes it has itself
 * loaded from every input. */
int fmcw_beam_device(fmcw_ctx* ctx, const fmcw_beam_params* q, const void* const* d_rd_ch, int32_t rd_dtype,
                     int64_t F, int32_t nr, int32_t nd, void* const* d_out, void* stream);

/* Host pointers (no alignment asked for): staged (all A channels and B outputs of a chunk), frames
 * sharded over the context's devices and chunked as fmcw_cfar is (bit-identical shards and chunks);
 * returns when the outputs are on the host. */
int fmcw_beam(fmcw_ctx* ctx, const fmcw_beam_params* q, const void* const* rd_ch, int32_t rd_dtype, int64_t F,
              int32_t nr, int32_t nd, void* const* out);

/* ---------------------------------------------------------------------------
 * Range-angle maps: the spatial covariance of the receive channels per range row, and the Bartlett
 * and Capon (MVDR) angular power spectra taken from it (added within ABI 4; beyond the reference).
 * fmcw_aoa* gives one angle per detection and fmcw_beam* at most eight fixed beams; this stage gives
 * an angular spectrum for every range row on a grid of up to 256 look directions, and the covariance
 * itself, which is the input of any subspace method (fmcw_music* below is one).  Indices below are 0-based; the gate is 1-based
 * as everywhere else.
 *   Input: A channel maps rd[a], A in 2..8, each [F][nr][nd], all FMCW_C64 or all FMCW_C32H, given as
 *     a host array of A pointers exactly as fmcw_beam takes them (device call: each 16-byte aligned);
 *     nr, nd within CFAR's limits.
 *   Stage 1, covariance.  For every frame f and every gated row r,
 *       R_ab = sum over d of x_a[r][d] conj(x_b[r][d])
 *     over the Doppler bins that are not left out: a bin is left out when circular
 *     |d - nd/2| <= dc_half, exactly fmcw_sig's rule (dc_half = -1 keeps every bin); N = bins kept.
 *     cov [F][nr][T][2] float32, T = A (A + 1) / 2: the packed upper triangle, entry (a, b), a <= b,
 *     at index a A - a (a - 1) / 2 + (b - a), each (re, im); a diagonal entry has im = +0.  Rows
 *     outside the gate r_lo..r_hi are all zero (0, 0: all rows).  fp16 storage: the stored values
 *     are widened exactly and the written sums are multiplied by ((float)nr (float)nd)^2, an exact
 *     power of two (the scale of fmcw_sig and fmcw_aoa).
 *     Accuracy: the order of the sum and the contraction of multiply-adds are the kernel's own.
 *     Every component of every entry is within (N + 8) 2^-24 sqrt(R_aa R_bb) of the exact sum of
 *     the stored values: a product term has at most 3 roundings of relative size 2^-24 against
 *     |x_a| |x_b|, a sum of N terms in any order adds (N - 1) 2^-24 sum |x_a| |x_b|, and
 *     sum_d |x_a| |x_b| <= sqrt(R_aa R_bb) (Cauchy-Schwarz); the 8 is fmcw_sig's margin.  For a
 *     diagonal entry, a sum of non-negative terms, this is fmcw_sig's relative bound.
 *     Determinism: the order is fixed by (A, nr, nd, dtype, dc_half, gate) alone and no float atomics
 *     are used, so the bytes do not depend on the call, on F, on sharding or on chunking.
 *   Stage 2, spectra, from the float32 cov bytes and a weight table w [n_ang][A][2], n_ang in 1..256:
 *     w[k] holds the beam weights of look direction k in fmcw_beam_steer's convention
 *     (w = conj(steering) / norm).  ra [F][nr][n_ang] float32, a power in the units of cov; rows
 *     outside the gate are zero.  Everything is float32, every operation rounded on its own in the
 *     order written (no fused multiply-add), divides and square roots correctly rounded: every
 *     output byte equals a float32 numpy evaluation of the same steps on the same cov bytes.
 *     Bartlett (flags 0): acc = 0; for a = 0..A-1, for b = a..A-1:
 *       c.re = wa.re wb.re + wa.im wb.im;  c.im = wa.im wb.re - wa.re wb.im;
 *       t = c.re R_ab.re - c.im R_ab.im;   acc = acc + t when a == b, else acc = acc + (t + t).
 *       ra = acc.  This is sum_d |sum_a w_a x_a|^2: the power of fmcw_beam's beam k summed over the
 *       kept Doppler bins.
 *     Capon (FMCW_RA_CAPON), once per row:
 *       tr = sum_a R_aa.re in ascending a (from 0);  delta = load (tr / (float)A).
 *       The Cholesky factor L (lower triangular, real diagonal) of M, M_ii = R_ii.re + delta and,
 *       for i > j, M_ij = (R_ji.re, -R_ji.im): for i = 0..A-1, for j = 0..i: s = M_ij; for
 *       k = 0..j-1: s.re -= (Lik.re Ljk.re + Lik.im Ljk.im), s.im -= (Lik.im Ljk.re - Lik.re Ljk.im);
 *       i == j: L_ii = sqrtf(s.re), and the row is DEGENERATE unless s.re > 0 and s.re is finite;
 *       i > j: L_ij = (s.re / L_jj, s.im / L_jj).
 *       Per direction: u_a = (w_a.re, -w_a.im); q = 0, e = 0; in ascending a: s = u_a; for
 *       b = 0..a-1: s.re -= (Lab.re yb.re - Lab.im yb.im), s.im -= (Lab.re yb.im + Lab.im yb.re);
 *       y_a = (s.re / L_aa, s.im / L_aa); q += (y_a.re^2 + y_a.im^2); e += (u_a.re^2 + u_a.im^2).
 *       ra = (e e) / q; ra = 0 for a degenerate row or q == 0.
 *       With w = conj(a) / A this is 1 / (a^H M^-1 a), the usual MVDR power, on the scale of the
 *       Bartlett value: both estimate a lone source's summed power.
 *     d_ra_max: an optional running maximum of everything written to ra, raised as an integer
 *     atomic maximum on the float's bits as fmcw_sig does (so a negative value, which rounding can
 *     leave in a Bartlett null, never raises it); the caller zeroes it first.  fmcw_sig_db_device
 *     turns ra into dB.
 *   A non-finite stored value or weight makes the outputs of the rows that hold it unspecified; it
 *   touches nothing else and nothing out of bounds.
 *   Parameters: n_chan = A in 2..8; n_ang in 1..256; r_lo, r_hi as fmcw_cfar_params; dc_half >= -1
 *     with 2 dc_half + 1 < nd; flags 0 or FMCW_RA_CAPON (an unknown bit is FMCW_E_ARG); load finite
 *     and >= 0, used only by Capon.
 *   Measured times and the copy-time yardsticks: DESIGN.md 4.12, profiles/ra_bench.json.
 * ------------------------------------------------------------------------- */
enum { FMCW_RA_CAPON = 1 };
typedef struct fmcw_ra_params {
  int32_t n_chan;          /* A, 2..8 */
  int32_t n_ang;           /* look directions, 1..256 */
  int32_t r_lo, r_hi;      /* range gate, 1-based inclusive; 0, 0: all rows */
  int32_t dc_half;         /* Doppler bins |d - nd/2| <= dc_half (circular) are left out; -1: none */
  int32_t flags;           /* 0 (Bartlett) or FMCW_RA_CAPON */
  float   load;            /* Capon's diagonal loading, relative to the mean diagonal; >= 0 */
} fmcw_ra_params;

/* Host only, no context: FMCW_E_ARG (with a message) for any violation of the constraints. */
int fmcw_ra_check(const fmcw_ra_params* q, int32_t nr, int32_t nd);

/* Host only, no context: the weights of n_ang look directions, w [n_ang][n_chan][2] flat.  The
 * formula, the argument rules and the rounding are fmcw_beam_steer's (one function forms both):
 * direction k of this table equals beam k % 8 of fmcw_beam_steer over sin_theta[8 (k / 8) ..].
 * FMCW_E_ARG (with a message, w untouched) for any violated constraint. */
int fmcw_ra_steer(int32_t n_chan, int32_t n_ang, float spacing, const float* sin_theta, const float* cal,
                  const float* taper, int32_t normalize, float* w);

/* Stage 1 on device pointers (d_rd_ch[a] device pointers, each 16-byte aligned, as is d_cov; the
 * array and *q are read on the host; d_cov must not overlap a map), asynchronous on `stream`; needs
 * no fmcw_set_taps.  Acts on the context's first device.  F = 0 is a no-op.  FMCW_E_ARG is returned
 * before any launch: d_cov is then untouched.  n_ang, flags and load are checked but not used. */
int fmcw_cov_device(fmcw_ctx* ctx, const fmcw_ra_params* q, const void* const* d_rd_ch, int32_t rd_dtype,
                    int64_t F, int32_t nr, int32_t nd, float* d_cov, void* stream);

/* Stage 2 on device pointers: d_cov [F][nr][T][2] is what fmcw_cov_device wrote, or a caller's own
 * covariance (the imaginary part of a diagonal entry is not read); d_w [n_ang][n_chan][2]; d_ra
 * [F][nr][n_ang]; all three 16-byte aligned; d_ra_max one float or NULL.  dc_half is checked
 * against -1 only (the call has no nd).  The rest as fmcw_cov_device. */
int fmcw_ra_device(fmcw_ctx* ctx, const fmcw_ra_params* q, const float* d_cov, int64_t F, int32_t nr,
                   const float* d_w, float* d_ra, float* d_ra_max, void* stream);

/* Host pointers (no alignment asked for): both stages, staged (all A channels of a chunk), frames
 * sharded over the context's devices and chunked as fmcw_beam is (bit-identical shards and chunks);
 * returns when the outputs are on the host.  cov or ra may be NULL, not both; w may be NULL without
 * ra; *ra_max (may be NULL) is the maximum over all shards, 0 without ra. */
int fmcw_ra(fmcw_ctx* ctx, const fmcw_ra_params* q, const void* const* rd_ch, int32_t rd_dtype, int64_t F,
            int32_t nr, int32_t nd, const float* w, float* cov, float* ra, float* ra_max);

/* ---------------------------------------------------------------------------
 * MUSIC angular spectra: per range row the eigen-decomposition of its spatial covariance, a source
 * count and the MUSIC pseudo-spectrum (added within ABI 4; beyond the reference).  Bartlett cannot
 * separate two returns closer than the array's beamwidth and Capon only sometimes; the noise
 * subspace of the covariance can, and with forward-backward averaging it also separates two
 * returns of one Doppler bin (coherent ones) on a uniform line.
 *   Input: cov [F][nr][T][2] float32, T = A (A + 1) / 2, A in 2..8: exactly what fmcw_cov_device
 *     writes, or a caller's own covariance in that layout; nr within CFAR's limits.
 *   Outputs, all float32 but nsrc; rows outside the gate r_lo..r_hi are zero in every one of them:
 *     eval [F][nr][A]          the eigenvalues, ascending;
 *     evec [F][nr][A][A][2]    evec[j][a] = component a of the eigenvector of eval[j], (re, im);
 *     nsrc [F][nr] int32       the source count n;
 *     music [F][nr][n_ang]     the pseudo-spectrum on the look directions of a weight table
 *                              w [n_ang][A][2] of fmcw_ra_steer, n_ang in 1..256.
 *   Everything is float32, every operation rounded on its own in the order written (no fused
 *   multiply-add), divides and square roots correctly rounded: every output byte equals a float32
 *   numpy evaluation of the steps below on the same cov bytes, for any F and any sharding or
 *   chunking, and does not depend on which other outputs were asked for.
 *   1. Matrix.  The state is the upper triangle: M_ab, a <= b, is the packed entry; a diagonal
 *      entry's imaginary part is not read (it is taken as +0).  Wherever M_ba, b > a, is read it is
 *      conj(M_ab), and where it is written M_ab becomes its conjugate: there is one copy of every pair.
 *      With FMCW_MUSIC_FB (forward-backward averaging, for a uniform line) every upper entry is first
 *      replaced from the ORIGINAL R by 0.5f (R_ab + R_a'b'), a' = A-1-b, b' = A-1-a (also an upper
 *      entry: no conjugate), re and im each on its own; a diagonal entry's im stays +0.
 *   2. Cyclic Jacobi, `sweeps` sweeps, no data-dependent stopping (the call ends for any bytes).
 *      V = I.  sweeps times: for p = 0..A-2, for q = p+1..A-1:
 *        h = M_pq;  g = sqrtf(h.re h.re + h.im h.im);  the pair is SKIPPED iff g == 0;
 *        ph = (h.re / g, h.im / g);  a = M_pp.re, b = M_qq.re;
 *        tau = (b - a) / (2 g);  at = |tau|;  t = 1 / (at + sqrtf(1 + at at)), negated when tau < 0;
 *        c = 1 / sqrtf(1 + t t);  s = t c;  sp = (s ph.re, s ph.im).
 *        For every k other than p and q, with x = M_kp, y = M_kq:
 *          M_kp = (c x.re - (sp.re y.re + sp.im y.im),  c x.im - (sp.re y.im - sp.im y.re))
 *          M_kq = ((sp.re x.re - sp.im x.im) + c y.re,  (sp.re x.im + sp.im x.re) + c y.im)
 *        (c x - conj(sp) y and sp x + c y, four real products per complex product, each pair's sum
 *        or difference rounded, then combined with the c term), and M_pk = conj(M_kp),
 *        M_qk = conj(M_kq).  Then M_pp = a - t g, M_qq = b + t g (one product t g), M_pq = (+0, +0).
 *        The same two expressions update V_kp, V_kq for EVERY k = 0..A-1.
 *        tau = +-inf gives t = 0: overflow needs no special case.
 *   3. Order.  lambda_j: the diagonal entries ascending, ties by original index; e_j the matching
 *      column of V.
 *   4. Source count.  n_src in 1..A-1: n = n_src.  n_src = 0: nu = (lambda_0 + ... +
 *      lambda_{A-max_src-1}, added ascending from 0) / (float)(A - max_src);
 *      n = min(max_src, #{j : lambda_j > src_thr nu}), in 0..max_src.
 *   5. MUSIC, per direction k, w = w[k]:  e = sum_a (w_a.re w_a.re + w_a.im w_a.im), ascending from 0;
 *      den = 0; for j = 0..A-n-1: p = (0, 0); for a ascending, v = e_j[a]:
 *        p.re += (w_a.re v.re - w_a.im v.im);  p.im += (w_a.re v.im + w_a.im v.re);
 *      den += (p.re p.re + p.im p.im).  music = e / den, FLT_MAX when den == 0.
 *      With w = conj(a) / A this is the usual a^H a / (a^H E_n E_n^H a).
 *   6. d_music_max: an optional running maximum of everything written to music, kept exactly as
 *      fmcw_ra_device's d_ra_max (an integer atomic maximum on the float's bits; the caller zeroes it).
 *   A zero row skips every rotation: lambda = 0, V = I; an estimated n is then 0 and music is 1.
 *   A non-finite input makes that row's outputs unspecified; it touches nothing else and nothing out
 *   of bounds.
 *   Accuracy against a float64 eigh, the rows where it is lost (equal diagonal entries under an
 *   off-diagonal entry whose square is denormal), the default of sweeps and the measured times:
 *   DESIGN.md 4.13, profiles/music_bench.json.
 *   Parameters: n_chan = A in 2..8; n_ang in 1..256; r_lo, r_hi as fmcw_cfar_params; n_src in
 *     0..A-1 (0: estimated); max_src in 1..A-1, read only when n_src = 0; sweeps in 1..16; flags 0 or
 *     FMCW_MUSIC_FB (an unknown bit is FMCW_E_ARG); src_thr finite and > 0.
 * ------------------------------------------------------------------------- */
enum { FMCW_MUSIC_FB = 1 };
typedef struct fmcw_music_params {
  int32_t n_chan;          /* A, 2..8 */
  int32_t n_ang;           /* look directions, 1..256 */
  int32_t r_lo, r_hi;      /* range gate, 1-based inclusive; 0, 0: all rows */
  int32_t n_src;           /* sources, 1..A-1; 0: estimated per row */
  int32_t max_src;         /* the estimate's upper limit, 1..A-1 (read only when n_src = 0) */
  int32_t sweeps;          /* Jacobi sweeps, 1..16 */
  int32_t flags;           /* 0 or FMCW_MUSIC_FB */
  float   src_thr;         /* the estimate's threshold over the mean of the smallest eigenvalues; > 0 */
} fmcw_music_params;

/* Host only, no context: FMCW_E_ARG (with a message) for any violation of the constraints. */
int fmcw_music_check(const fmcw_music_params* q, int32_t nr);

/* Device pointers (every one given 16-byte aligned; *q is read on the host), asynchronous on
 * `stream`; needs no fmcw_set_taps.  Acts on the context's first device.  d_cov [F][nr][T][2];
 * d_w [n_ang][n_chan][2], needed only with d_music; d_eval, d_evec, d_nsrc, d_music as above, any of
 * them NULL (not written) but not all; d_music_max one float or NULL, raised only with d_music.
 * F = 0 is a no-op.  FMCW_E_ARG is returned before any launch: the outputs are then untouched. */
int fmcw_music_device(fmcw_ctx* ctx, const fmcw_music_params* q, const float* d_cov, int64_t F, int32_t nr,
                      const float* d_w, float* d_eval, float* d_evec, int32_t* d_nsrc, float* d_music,
                      float* d_music_max, void* stream);

/* Host pointers (no alignment asked for): staged, frames sharded over the context's devices and
 * chunked as fmcw_ra is (bit-identical shards and chunks); returns when the outputs are on the host.
 * Any output may be NULL, not all; w may be NULL without music; *music_max (may be NULL) is the
 * maximum over all shards, 0 without music. */
int fmcw_music(fmcw_ctx* ctx, const fmcw_music_params* q, const float* cov, int64_t F, int32_t nr, const float* w,
               float* eval, float* evec, int32_t* nsrc, float* music, float* music_max);

/* ---------------------------------------------------------------------------
 * Directions of arrival: the peaks of an angular spectrum per range row, thinned, ordered by power,
 * each with a sub-grid direction (added within ABI 4; beyond the reference).  fmcw_ra* and
 * fmcw_music* end in a spectrum [F][nr][n_ang]; this stage turns it into what a caller wants from
 * it: how many returns a row holds, in which directions and how strong, as a fixed-size record per
 * row in the form of the CFAR lists.
 *   Input: spec [F][nr][K] float32, K = n_ang in 1..256: what fmcw_ra_device or fmcw_music_device
 *     wrote, or a caller's own spectrum; sin_theta [K] float32, the grid u the weight table was
 *     formed on (the table does not carry it); nr within CFAR's limits.
 *   Outputs; unused slots and every row outside the gate r_lo..r_hi hold idx -1, floats +0, count 0:
 *     count [F][nr] int32          the peaks kept; it may exceed max_pk (as CFAR's count may max_det);
 *     idx   [F][nr][max_pk] int32  the grid point k of every written peak;
 *     pow, sin, base [F][nr][max_pk] float32: s[k], the sub-grid direction, the peak's reference level.
 *   Everything is float32, every operation rounded on its own in the order written (no fused
 *   multiply-add), divides correctly rounded: every output byte equals the plain-loop evaluation of
 *   the steps below (tests/doa_reference.py) on the same bytes, for any F and any sharding or
 *   chunking, and does not depend on which other outputs were asked for.  Per gated row s[0..K-1]:
 *   0. Extremes.  hi = max s, lo = min s, by compares.  Unless hi > lo and hi > 0 the row has no peak.
 *   1. Peak test.  For k let L = k - 1 and R the first index right of k with s[R] != s[k]; k is a
 *      peak iff s[L] < s[k] and s[R] < s[k]: of a flat top only its first point qualifies, and a
 *      flat stretch that then rises is no peak.  Default: if L or R does not exist (k = 0, or the
 *      walk reaches the end) k is no peak, as MATLAB's findpeaks treats end points.
 *      FMCW_DOA_EDGES: a missing neighbour counts as lower.  FMCW_DOA_WRAP: indices are taken modulo
 *      K (hi > lo: R exists).
 *   2. Base, the reference level of findpeaks' prominence.  Walk left from k over the indices j with
 *      s[j] <= s[k]; stop before the first s[j] > s[k], or at the end, or after K - 1 steps under
 *      WRAP.  lmin: the minimum over the visited j (k itself is not among them); rmin the same to the
 *      right; base = max(lmin, rmin) + 0.0f (a zero base is +0).  A side with nothing visited does
 *      not take part (only at an end under EDGES).
 *   3. Keep k iff s[k] > 0 and s[k] >= min_abs and s[k] >= fl(min_rel hi) and s[k] >= fl(min_prom
 *      base).  The prominence rule is a ratio because MUSIC's pseudo-spectrum has no absolute scale;
 *      min_prom = 0 switches it off.
 *   4. Order.  Kept peaks by descending s[k], ties by ascending k; count = the number kept; the first
 *      max_pk are written: pow = s[k], base as above.
 *   5. Sub-grid direction of every written peak.  kl = k - 1, kr = k + 1, modulo K under WRAP.  If a
 *      neighbour is missing sin = u[k], the grid value itself.  Otherwise (l, c, r) = (s[kl], s[k],
 *      s[kr]) and delta = 0; with FMCW_DOA_INV the parabola is laid through the reciprocals, which
 *      suits Capon and MUSIC (one over a quadratic form that is smooth at its minimum): if l > 0 and
 *      r > 0 the three become 1/l, 1/c, 1/r, otherwise delta stays 0 and the next line is skipped.
 *        den = (l - c) + (r - c);  num = 0.5f (l - r);  delta = num / den when den is finite and
 *        not 0 and num is finite.
 *      delta is then clamped to [-0.5, 0.5] (in exact arithmetic a peak's |delta| is at most 0.5; the
 *      halving in num rounds when l - r is an odd number of denormal units, e.g. 0.5f * 3u = 2u over
 *      den = 3u).  delta >= 0: sin = u[k] + delta (u[kr] - u[k]);
 *      delta < 0: sin = u[k] + delta (u[k] - u[kl]).  Across the seam under WRAP the grid step on the
 *      other side of k is used: k = K-1 with delta >= 0: u[k] - u[kl]; k = 0 with delta < 0:
 *      u[kr] - u[k].  The result is not folded back into [-1, 1].
 *   6. A non-finite s or u makes that row's outputs unspecified; it touches nothing else and nothing
 *      out of bounds.
 *   Measured errors of the sub-grid direction and the measured times: DESIGN.md 4.14,
 *   profiles/doa_bench.json.
 *   Parameters: n_ang = K in 1..256; r_lo, r_hi as fmcw_cfar_params; max_pk in 1..8; flags a subset
 *     of FMCW_DOA_EDGES, FMCW_DOA_WRAP, FMCW_DOA_INV (EDGES with WRAP, or an unknown bit, is
 *     FMCW_E_ARG; WRAP needs n_ang >= 3); min_abs finite and >= 0; min_rel in [0, 1]; min_prom finite
 *     and >= 0.
 * ------------------------------------------------------------------------- */
enum { FMCW_DOA_EDGES = 1, FMCW_DOA_WRAP = 2, FMCW_DOA_INV = 4 };
typedef struct fmcw_doa_params {
  int32_t n_ang;           /* K, look directions, 1..256 */
  int32_t r_lo, r_hi;      /* range gate, 1-based inclusive; 0, 0: all rows */
  int32_t max_pk;          /* written peaks per row, 1..8 */
  int32_t flags;           /* FMCW_DOA_* */
  float   min_abs;         /* keep s[k] >= min_abs; >= 0 */
  float   min_rel;         /* keep s[k] >= min_rel * the row's maximum; 0..1 */
  float   min_prom;        /* keep s[k] >= min_prom * base; >= 0, 0: off */
} fmcw_doa_params;

/* Host only, no context: FMCW_E_ARG (with a message) for any violation of the constraints. */
int fmcw_doa_check(const fmcw_doa_params* q, int32_t nr);

/* Device pointers (every one given 16-byte aligned; *q is read on the host), asynchronous on
 * `stream`; needs no fmcw_set_taps.  Acts on the context's first device.  d_spec [F][nr][n_ang];
 * d_sin_theta [n_ang]; d_count, d_idx, d_pow, d_sin, d_base as above, any of them NULL (not written)
 * but not all.  F = 0 is a no-op.  FMCW_E_ARG is returned before any launch: the outputs are then
 * untouched. */
int fmcw_doa_device(fmcw_ctx* ctx, const fmcw_doa_params* q, const float* d_spec, int64_t F, int32_t nr,
                    const float* d_sin_theta, int32_t* d_count, int32_t* d_idx, float* d_pow, float* d_sin,
                    float* d_base, void* stream);

/* Host pointers (no alignment asked for): staged, frames sharded over the context's devices and
 * chunked as fmcw_music is (fmcw_set_chunk_frames, when set, gives the frames of a chunk;
 * bit-identical shards and chunks); returns when the outputs are on the host.  Any output may be
 * NULL, not all. */
int fmcw_doa(fmcw_ctx* ctx, const fmcw_doa_params* q, const float* spec, int64_t F, int32_t nr, const float* sin_theta,
             int32_t* count, int32_t* idx, float* pow, float* sin, float* base);

/* ---------------------------------------------------------------------------
 * spectrogram.png, replacing radar_processing.m:331-348:
 *   surf(T, fftshift(F), fftshift(psd,1), 'EdgeColor','none'); view(0,90);
 *   axis tight; ylim([0 150]); clim([-40 0]); axis off; colormap(jet);
 *   exportgraphics(fig, 'spectrogram.png', 'Resolution', 600)
 * rendered on the GPU (kernels_render.hip states the rules: the fftshift-ed
 * one-sided axis folds the surface; the depth test of the top view; flat
 * faces coloured by their first vertex through jet(256) on [-40 0] dB) and
 * written as an 8-bit palette PNG.  Default size 2906 x 2038: the default
 * axes box of a 600 x 400 figure (0.775 x 0.815 of it) at 600/96 px per
 * screen pixel, which is what exportgraphics crops to with the axis off.
 * MATLAB graphics cannot run here: the pixels are unpinned against it.
 * ------------------------------------------------------------------------- */
#define FMCW_PNG_FMAX_HZ 150.0
#define FMCW_PNG_CMIN_DB (-40.0)
#define FMCW_PNG_CMAX_DB 0.0
#define FMCW_PNG_DEFAULT_W 2906
#define FMCW_PNG_DEFAULT_H 2038

/* fmcw_stft (:270-299) plus the PNG of :331-348 written to png_path
 * (width/height 0: the defaults above); png_bytes may be NULL. */
int fmcw_stft_png(fmcw_ctx* ctx, const float* x, int64_t L, const float* win, int32_t wlen, int32_t noverlap,
                  int32_t nfft, double fs, int32_t n_log_bins, float* T, float* freq, float* intensity,
                  const char* png_path, int32_t width, int32_t height, int64_t* png_bytes);

/* Device call: palette indices img[height][1 + width] (PNG filter byte 0 first)
 * from Q[nseg][nq + 1] = the one-sided P (:276) of bins 0 .. nq-1 followed by
 * bin nfft/2 (for a full P row of nfft/2 + 1 bins: nq = nfft/2, Q = P), the
 * global max(P) (:282), T(1) = t0, T(2) - T(1) = dt. */
int fmcw_render_spectrogram_device(fmcw_ctx* ctx, const float* d_Q, int32_t nq, const int64_t* d_nseg,
                                   const float* d_pmax, int32_t nfft, double fs, double t0, double dt, int32_t width,
                                   int32_t height, uint8_t* d_img, void* stream);

/* ---------------------------------------------------------------------------
 * Output files: native jsonencode(struct, 'PrettyPrint', true).
 * Replaces the jsonencode + fprintf of radar_processing.m:313-321
 * (spectrogram_data.json), :362-369 (<file>_range_fft_data.json), :390-398
 * (<file>_range_speed_data.json), :424-431 (<file>_fft_data.json) and :590-593
 * (the 'yes' branch's batch JSONs).  One field per struct member, in order:
 *   FMCW_JSON_STRING  data = NUL-terminated char*, rows/cols ignored
 *   FMCW_JSON_F32/F64/I32  a rows x cols MATLAB array; element (i, j) at
 *     data[i * row_stride + j * col_stride] (so a [nseg][nbins] device-layout
 *     intensity is written as MATLAB's nbins x nseg without a transpose).
 *   FMCW_JSON_BOOL    the same with uint8 elements (0 / non-0): a MATLAB logical
 *     array, written as true / false.
 * jsonencode's shape rules: 1x1 -> number, 1xN / Nx1 -> flat array, MxN ->
 * array of M rows, empty -> []; NaN/Inf -> null; numbers as "%.15g" (integers
 * without a fraction).  threads <= 0: up to 16 host threads format in parallel.
 * No device work; no context needed.
 * ------------------------------------------------------------------------- */
enum { FMCW_JSON_STRING = 0, FMCW_JSON_F32 = 1, FMCW_JSON_F64 = 2, FMCW_JSON_I32 = 3, FMCW_JSON_BOOL = 4 };
typedef struct {
  const char* name;
  int32_t kind;
  const void* data;
  int64_t rows, cols, row_stride, col_stride;
} fmcw_json_field;
int fmcw_json_write(const char* path, const fmcw_json_field* fields, int32_t n_fields, int32_t pretty,
                    int32_t threads, int64_t* bytes_written);

#ifdef __cplusplus
}
#endif
#endif /* FMCW_H_ */
