/*
 * fmcw_mex.c -- MATLAB MEX gateway onto libfmcw (include/fmcw.h).
 *
 * Binds the C-ABI for matlab/radar_processing.m, which keeps the signature
 * radar_processing(process_animal_activity) of the reference
 * (radar-etl-pipeline/radar_processing.m:56) and calls:
 *
 *   fmcw_mex('init' [, device_ids])                              -> fmcw_ctx_create (once; mexLock);
 *                                        device_ids: vector; without it fmcw_default_devices (the env
 *                                        var FMCW_DEVICES, else every visible GPU); several ids = one
 *                                        context over several GPUs (frames and STFT segments sharded,
 *                                        RCCL max)
 *   ids = fmcw_mex('devices')                                    -> fmcw_ctx_devices (the ids in use)
 *   fmcw_mex('taps', P, range_win, doppler_win, calib_rx1)       -> fmcw_set_taps       (:138-139, :174)
 *   [prof, cnt, ridx, rmag, didx, slow, probe] =
 *       fmcw_mex('process', P, iq, probe_column)                  -> fmcw_process        (:197-261, :265, :410)
 *   [T, freq, intensity] =
 *       fmcw_mex('stft', x, win, noverlap, nfft, fs, n_log_bins)  -> fmcw_stft           (:270-299)
 *   [T, freq, intensity] =
 *       fmcw_mex('stft_png', x, win, noverlap, nfft, fs, n_log_bins, png_path)
 *                                                                 -> fmcw_stft_png  (:270-299 + :331-348)
 *   bytes = fmcw_mex('json', path, s)                             -> fmcw_json_write (:313-321 and the other
 *                                        jsonencode(s, 'PrettyPrint', true) + fprintf writes); s: a scalar
 *                                        struct of char rows and double / single / int32 arrays
 *   [cnt, ridx, didx, power, noise] = fmcw_mex('cfar', Q, rd)     -> fmcw_cfar: 2-D CA-CFAR over an RD map
 *                                        (beyond the reference); Q: a struct with the fields of
 *                                        fmcw_cfar_params; rd: single complex Nd x Nr x F (the C array
 *                                        [F][Nr][Nd]: permute(range_Doppler, [2 1 3])); ridx ... noise are
 *                                        max_det x F
 *   [cnt, ridx, didx, power, noise] = fmcw_mex('oscfar', Q, rd)   -> fmcw_oscfar: 2-D ordered-statistic CFAR over
 *                                        an RD map; Q: the fields of 'cfar' plus rank (1..N_full); rd and the
 *                                        outputs as for 'cfar', noise holding the order statistic X_(k)
 *   [dt, rt, dt_max, rt_max] = fmcw_mex('signature', Q, rd[, center])  -> fmcw_sig: Doppler-time (micro-Doppler)
 *                                        and range-time signatures of an RD map (beyond the reference); Q: a
 *                                        struct with the fields of fmcw_sig_params; rd as for 'cfar'; center:
 *                                        int32, one 1-based range row per frame (0: no target), e.g.
 *                                        ridx(1, :) of 'process', or absent / empty for the fixed gate; dt is
 *                                        Nd x F, rt Nr x F (in dB when Q.flags has FMCW_SIG_DB), the maxima
 *                                        are those of the linear maps
 *   [tcnt, cells, pk_ridx, pk_didx, ext_r, ext_d, pk_power, pk_noise, power, range, doppler, label] =
 *       fmcw_mex('cluster', Q, cnt, ridx, didx, power, noise, nr, nd)  -> fmcw_cluster: the detection lists of
 *                                        'cfar' grouped into targets (beyond the reference, whose range_speed of
 *                                        :241-252 holds one range and one speed per target); Q: a struct with the
 *                                        fields of fmcw_cluster_params; cnt 1 x F, ridx ... noise max_det x F as
 *                                        'cfar' returns them (noise may be []); tcnt is 1 x F, label max_det x F,
 *                                        the others max_tgt x F; range and doppler are the 1-based power-weighted
 *                                        centroids.  Outputs that are not asked for are not computed.
 *   [zre, zim, phase, sn, tzre, tzim, te0, te1, tphase, tsn, tcoh, tcells] =
 *       fmcw_mex('aoa', Q, rd4, cnt, ridx, didx[, label])           -> fmcw_aoa: the angle of arrival at the cells
 *                                        of 'cfar' and the targets of 'cluster' from several receive planes (beyond
 *                                        the reference, which keeps frame.Chirp(:,:,1) alone); Q: a struct with the
 *                                        fields max_tgt, flags, spacing of fmcw_aoa_params and, optionally, w: a
 *                                        double array of 2 A values (re, im per plane; absent: no weighting); rd4:
 *                                        single complex Nd x Nr x F x A, cat(4, ...) of the planes' RD maps, each
 *                                        as for 'cfar' (A = size(rd4, 4) is n_chan); cnt 1 x F, ridx, didx max_det
 *                                        x F as 'cfar' returns them; label max_det x F as 'cluster' returns it, or
 *                                        absent / [] (then only the first four outputs exist); zre ... sn are
 *                                        max_det x F, tzre ... tcells max_tgt x F; sn and tsn are sin(theta).
 *                                        Outputs that are not asked for are not computed.
 *   [kcnt, id, status, age, misses, range, rate, doppler, power, tgt_track, state] =
 *       fmcw_mex('track', Q, tcnt, range, doppler, power, nr, nd, nseq[, state])  -> fmcw_track: the targets of
 *                                        'cluster' tracked across frames (the per-target time series range_speed
 *                                        of :385-389 needs to know which target is which); Q: a struct with the
 *                                        fields of fmcw_track_params; tcnt 1 x (nseq*F), range, doppler, power
 *                                        max_tgt x (nseq*F) as 'cluster' returns them (sequence s in the columns
 *                                        s*F+1 .. s*F+F); state: int32, fmcw_track_state_bytes(max_trk)/4 x nseq, as
 *                                        an earlier call returned it, or absent / [] for fresh sequences; kcnt is
 *                                        1 x (nseq*F), tgt_track max_tgt x (nseq*F), the others max_trk x (nseq*F):
 *                                        a row is the trajectory of one slot.  Outputs not asked for are not computed.
 *   [out, bg, seen] = fmcw_mex('mti', Q, rd, nseq[, bg, seen])    -> fmcw_mti: the frame-to-frame clutter filter
 *                                        of an RD map (beyond the reference): a complex background per cell,
 *                                        learned recursively and subtracted coherently; Q: a struct with the fields
 *                                        of fmcw_mti_params (lambda, flags); rd as for 'cfar', Nd x Nr x (nseq*F)
 *                                        (sequence s in the frames s*F+1 .. s*F+F); bg: single complex Nd x Nr x
 *                                        nseq and seen: int32 1 x nseq as an earlier call returned them, or both
 *                                        absent / [] for fresh sequences; out is (Nd*Nr) x (nseq*F) and bg (Nd*Nr) x
 *                                        nseq, single complex (reshape(out, Nd, Nr, []) feeds 'cfar' and 'signature'
 *                                        unchanged), seen 1 x nseq.  With FMCW_MTI_FREEZE in Q.flags bg and seen
 *                                        come back as they went in.
 *   out = fmcw_mex('beam', Q, rd4)                                -> fmcw_beam: the receive planes' RD maps combined
 *                                        into B maps to detect on (beyond the reference): steered beams, or with
 *                                        FMCW_BEAM_NCI in Q.flags one map of the summed plane power; Q: a struct with
 *                                        the fields flags and w, a real double array of 2 x A x B values (re, im;
 *                                        plane; beam), e.g. what 'beam_steer' returns; rd4 as for 'aoa', single
 *                                        complex Nd x Nr x F x A; out is (Nd*Nr*F) x B, single complex:
 *                                        reshape(out, Nd, Nr, F, B) is the 4-D array Nd x Nr x F x B, and
 *                                        out4(:, :, :, b) feeds 'mti', 'cfar' and 'signature' unchanged
 *   w = fmcw_mex('beam_steer', n_chan, spacing, sin_theta[, cal, taper, normalize])
 *                                                                 -> fmcw_beam_steer (needs no context): the weights of
 *                                        one beam per entry of sin_theta for a uniform line, in the sign convention
 *                                        of 'aoa'; cal: 2 A doubles (re, im per plane) or [], taper: A doubles or [],
 *                                        normalize: 0 / 1 (default 1); w is (2*A) x B, double, the layout of Q.w
 *   [ra, cov, ra_max] = fmcw_mex('ra', Q, rd4, w)                 -> fmcw_ra: range-angle maps (beyond the reference): the
 *                                        receive planes' spatial covariance per range row and its Bartlett or, with
 *                                        FMCW_RA_CAPON in Q.flags, Capon spectrum over the look directions of w; Q: a
 *                                        struct with the fields r_lo, r_hi, dc_half, flags, load; rd4 as for 'aoa',
 *                                        single complex Nd x Nr x F x A; w: a real double array of 2 x A x K values (re,
 *                                        im; plane; direction), e.g. what 'ra_steer' returns; ra is K x (Nr*F) single
 *                                        (a power; reshape(ra, K, Nr, F)), cov (2*T) x (Nr*F) single with T =
 *                                        A (A + 1) / 2 (reshape(cov, 2, T, Nr, F): the packed upper triangle, re and
 *                                        im), ra_max a double
 *   w = fmcw_mex('ra_steer', n_chan, spacing, sin_theta[, cal, taper, normalize])
 *                                                                 -> fmcw_ra_steer (needs no context): 'beam_steer' for up
 *                                        to 256 look directions; w is (2*A) x K, double
 *   [music, nsrc, eval, evec, music_max] = fmcw_mex('music', Q, cov, nr, w)
 *                                                                 -> fmcw_music: MUSIC angular spectra (beyond the
 *                                        reference) from the covariance 'ra' returns: per range row the
 *                                        eigen-decomposition, a source count and the pseudo-spectrum over the look
 *                                        directions of w; Q: a struct with the fields r_lo, r_hi, n_src, max_src,
 *                                        sweeps, flags (FMCW_MUSIC_FB = 1), src_thr; cov: real single (2*T) x (Nr*F),
 *                                        T = A (A + 1) / 2, A in 2..8; nr: the rows of one frame; w as for 'ra';
 *                                        music is K x (Nr*F) single (reshape(music, K, Nr, F)), nsrc 1 x (Nr*F) int32,
 *                                        eval A x (Nr*F) single (ascending), evec (2*A*A) x (Nr*F) single
 *                                        (reshape(evec, 2, A, A, Nr, F): re and im; component; eigenvector), music_max
 *                                        a double
 *   [idx, count, pow, sn, base] = fmcw_mex('doa', Q, spec, nr, sin_theta)
 *                                                                 -> fmcw_doa: directions of arrival (beyond the
 *                                        reference), the peaks of an angular spectrum per range row; Q: a struct with
 *                                        the fields r_lo, r_hi, max_pk, flags (FMCW_DOA_EDGES = 1, FMCW_DOA_WRAP = 2,
 *                                        FMCW_DOA_INV = 4), min_abs, min_rel, min_prom; spec: real single K x (Nr*F),
 *                                        what 'ra' or 'music' returns, K in 1..256; nr: the rows of one frame;
 *                                        sin_theta: the K grid values the weight table was formed on; idx is
 *                                        max_pk x (Nr*F) int32, 0-based grid points by descending power, -1 in unused
 *                                        slots; count 1 x (Nr*F) int32 (it may exceed max_pk); pow, sn (the sub-grid
 *                                        sin(theta)) and base max_pk x (Nr*F) single
 *   fmcw_mex('close')                                            -> fmcw_ctx_destroy
 *
 * P is a struct with the fields of fmcw_params (nts, pn, nr, nd, max_targets,
 * doppler_fallback_idx, if_scale, range_thr, doppler_thr, min_d, max_d,
 * dist_per_bin).  iq is a single complex NTS x PN x F array (interleaved
 * complex API: build with `mex -R2018a`), which is the C array [F][PN][NTS]
 * of the ABI -- no copy.  Outputs come back in MATLAB layout: prof Nr x F
 * (= range_tx1rx1_max_abs), ridx/rmag/didx M x F, slow PN x F, probe Nr x 1,
 * intensity nbins x nseg.
 *
 * Errors: a non-zero fmcw status becomes mexErrMsgIdAndTxt("fmcw:<status>",
 * fmcw_last_error()), i.e. a MATLAB exception that the unchanged try/catch of
 * radar_processing_with_azure.m:48-66 records in its steps struct.
 *
 * Build (MATLAB R2018a+):  mex -R2018a -I../include fmcw_mex.c -L../fmcw_radar_processing_amd -lfmcw
 * This file is compile-checked only where mex.h exists (not in this container).
 */
#include "mex.h"

#include <stdio.h>
#include <string.h>

#include "fmcw.h"

static fmcw_ctx* g_ctx = NULL;

static void at_exit(void) {
  if (g_ctx) fmcw_ctx_destroy(g_ctx);
  g_ctx = NULL;
}

static void check(int st) {
  if (st != FMCW_OK) {
    char id[32];
    const char* name = st == FMCW_E_ARG ? "arg" : st == FMCW_E_HIP ? "hip" : st == FMCW_E_OOM ? "oom"
                     : st == FMCW_E_STATE ? "state" : st == FMCW_E_DATA ? "data" : "error";
    snprintf(id, sizeof id, "fmcw:%s", name);
    mexErrMsgIdAndTxt(id, "%s", fmcw_last_error());
  }
}

static double field(const mxArray* s, const char* name) {
  const mxArray* f = mxGetField(s, 0, name);
  if (!f || !mxIsNumeric(f) || mxGetNumberOfElements(f) != 1) mexErrMsgIdAndTxt("fmcw:arg", "P.%s missing", name);
  return mxGetScalar(f);
}

static fmcw_params params_of(const mxArray* s) {
  fmcw_params p;
  if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "P must be a struct");
  p.nts = (int32_t)field(s, "nts");
  p.pn = (int32_t)field(s, "pn");
  p.nr = (int32_t)field(s, "nr");
  p.nd = (int32_t)field(s, "nd");
  p.max_targets = (int32_t)field(s, "max_targets");
  p.doppler_fallback_idx = (int32_t)field(s, "doppler_fallback_idx");
  p.if_scale = (float)field(s, "if_scale");
  p.range_thr = (float)field(s, "range_thr");
  p.doppler_thr = (float)field(s, "doppler_thr");
  p.min_d = (float)field(s, "min_d");
  p.max_d = (float)field(s, "max_d");
  p.dist_per_bin = (float)field(s, "dist_per_bin");
  return p;
}

static float* single_real(const mxArray* a, mwSize n, const char* what) {
  if (!mxIsSingle(a) || mxIsComplex(a) || mxGetNumberOfElements(a) != n)
    mexErrMsgIdAndTxt("fmcw:arg", "%s must be a real single array of %d elements", what, (int)n);
  return mxGetSingles(a);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  char cmd[16];
  if (nrhs < 1 || mxGetString(prhs[0], cmd, sizeof cmd)) mexErrMsgIdAndTxt("fmcw:arg", "first argument: command");

  if (!strcmp(cmd, "init")) {
    if (!g_ctx) {
      int32_t ids[64] = {0};
      int32_t n = 1;
      if (nrhs < 2) {
        check(fmcw_default_devices(64, ids, &n));
      } else {
        const mxArray* a = prhs[1];
        if (!mxIsDouble(a) || mxIsComplex(a) || mxGetNumberOfElements(a) < 1 || mxGetNumberOfElements(a) > 64)
          mexErrMsgIdAndTxt("fmcw:arg", "init: device_ids must be a real double vector of 1..64 ids");
        n = (int32_t)mxGetNumberOfElements(a);
        for (int32_t i = 0; i < n; ++i) ids[i] = (int32_t)mxGetDoubles(a)[i];
      }
      check(fmcw_ctx_create(n, ids, &g_ctx));
      mexLock();
      mexAtExit(at_exit);
    }
    return;
  }
  if (!strcmp(cmd, "devices")) {            /* ids = fmcw_mex('devices'): the context's device ids */
    if (!g_ctx) mexErrMsgIdAndTxt("fmcw:state", "call fmcw_mex('init') first");
    int32_t ids[64], n = 0, rc = 0;
    check(fmcw_ctx_devices(g_ctx, &n, ids, &rc));
    plhs[0] = mxCreateDoubleMatrix(1, n, mxREAL);
    for (int32_t i = 0; i < n; ++i) mxGetDoubles(plhs[0])[i] = ids[i];
    return;
  }
  if (!strcmp(cmd, "close")) {
    if (g_ctx) { fmcw_ctx_destroy(g_ctx); g_ctx = NULL; mexUnlock(); }
    return;
  }
  if (!strcmp(cmd, "json")) {               /* bytes = fmcw_mex('json', path, s): needs no context */
    if (nrhs != 3 || !mxIsChar(prhs[1]) || !mxIsStruct(prhs[2]) || mxGetNumberOfElements(prhs[2]) != 1)
      mexErrMsgIdAndTxt("fmcw:arg", "json: path, scalar struct");
    char path[4096];
    if (mxGetString(prhs[1], path, sizeof path)) mexErrMsgIdAndTxt("fmcw:arg", "json: path too long");
    const int nf = mxGetNumberOfFields(prhs[2]);
    fmcw_json_field* fl = (fmcw_json_field*)mxCalloc(nf > 0 ? nf : 1, sizeof(fmcw_json_field));
    for (int k = 0; k < nf; ++k) {
      const mxArray* v = mxGetFieldByNumber(prhs[2], 0, k);
      fl[k].name = mxGetFieldNameByNumber(prhs[2], k);
      if (!v) mexErrMsgIdAndTxt("fmcw:arg", "json: field %s is empty", fl[k].name);
      if (mxIsChar(v)) {
        fl[k].kind = FMCW_JSON_STRING;
        fl[k].data = mxArrayToUTF8String(v);          /* freed with the MEX call's memory */
        continue;
      }
      if (mxIsComplex(v) || mxGetNumberOfDimensions(v) > 2)
        mexErrMsgIdAndTxt("fmcw:arg", "json: field %s must be a real vector or matrix", fl[k].name);
      fl[k].kind = mxIsDouble(v) ? FMCW_JSON_F64 : mxIsSingle(v) ? FMCW_JSON_F32 : mxIsInt32(v) ? FMCW_JSON_I32 : -1;
      if (fl[k].kind < 0) mexErrMsgIdAndTxt("fmcw:arg", "json: field %s: double, single, int32 or char", fl[k].name);
      fl[k].data = mxGetData(v);
      fl[k].rows = (int64_t)mxGetM(v);
      fl[k].cols = (int64_t)mxGetN(v);
      fl[k].row_stride = 1;                          /* MATLAB column-major */
      fl[k].col_stride = (int64_t)mxGetM(v);
    }
    int64_t bytes = 0;
    check(fmcw_json_write(path, fl, nf, 1, 0, &bytes));
    if (nlhs > 0) plhs[0] = mxCreateDoubleScalar((double)bytes);
    return;
  }
  if (!strcmp(cmd, "beam_steer")) {         /* w = fmcw_mex('beam_steer', n_chan, spacing, sin_theta[, cal, taper, normalize]): needs no context */
    if (nrhs < 4 || nrhs > 7) mexErrMsgIdAndTxt("fmcw:arg", "beam_steer: n_chan, spacing, sin_theta[, cal, taper, normalize]");
    const int32_t A = (int32_t)mxGetScalar(prhs[1]);
    const mwSize B = mxGetNumberOfElements(prhs[3]);
    if (A < 2 || A > 8 || B < 1 || B > 8 || !mxIsDouble(prhs[3]) || mxIsComplex(prhs[3]))
      mexErrMsgIdAndTxt("fmcw:arg", "beam_steer: n_chan in 2..8 and sin_theta a real double vector of 1..8 values");
    float st[8], cal[16], taper[8];
    const float* pc = NULL;
    const float* pt = NULL;
    for (mwSize b = 0; b < B; ++b) st[b] = (float)mxGetDoubles(prhs[3])[b];
    if (nrhs > 4 && mxGetNumberOfElements(prhs[4]) > 0) {
      if (!mxIsDouble(prhs[4]) || mxIsComplex(prhs[4]) || mxGetNumberOfElements(prhs[4]) != (mwSize)(2 * A))
        mexErrMsgIdAndTxt("fmcw:arg", "beam_steer: cal must be a real double array of 2 A values (re, im per plane)");
      for (int i = 0; i < 2 * A; ++i) cal[i] = (float)mxGetDoubles(prhs[4])[i];
      pc = cal;
    }
    if (nrhs > 5 && mxGetNumberOfElements(prhs[5]) > 0) {
      if (!mxIsDouble(prhs[5]) || mxIsComplex(prhs[5]) || mxGetNumberOfElements(prhs[5]) != (mwSize)A)
        mexErrMsgIdAndTxt("fmcw:arg", "beam_steer: taper must be a real double array of A values");
      for (int i = 0; i < A; ++i) taper[i] = (float)mxGetDoubles(prhs[5])[i];
      pt = taper;
    }
    fmcw_beam_params q;
    check(fmcw_beam_steer(A, (int32_t)B, (float)mxGetScalar(prhs[2]), st, pc, pt, nrhs > 6 ? mxGetScalar(prhs[6]) != 0 : 1, &q));
    plhs[0] = mxCreateDoubleMatrix((mwSize)(2 * A), B, mxREAL);
    for (mwSize b = 0; b < B; ++b)
      for (int i = 0; i < 2 * A; ++i) mxGetDoubles(plhs[0])[b * (mwSize)(2 * A) + i] = q.w[b][i / 2][i % 2];
    return;
  }
  if (!strcmp(cmd, "ra_steer")) {           /* w = fmcw_mex('ra_steer', n_chan, spacing, sin_theta[, cal, taper, normalize]): needs no context */
    if (nrhs < 4 || nrhs > 7) mexErrMsgIdAndTxt("fmcw:arg", "ra_steer: n_chan, spacing, sin_theta[, cal, taper, normalize]");
    const int32_t A = (int32_t)mxGetScalar(prhs[1]);
    const mwSize K = mxGetNumberOfElements(prhs[3]);
    if (A < 2 || A > 8 || K < 1 || K > 256 || !mxIsDouble(prhs[3]) || mxIsComplex(prhs[3]))
      mexErrMsgIdAndTxt("fmcw:arg", "ra_steer: n_chan in 2..8 and sin_theta a real double vector of 1..256 values");
    float st[256], cal[16], taper[8], wf[256 * 8 * 2];
    const float* pc = NULL;
    const float* pt = NULL;
    for (mwSize k = 0; k < K; ++k) st[k] = (float)mxGetDoubles(prhs[3])[k];
    if (nrhs > 4 && mxGetNumberOfElements(prhs[4]) > 0) {
      if (!mxIsDouble(prhs[4]) || mxIsComplex(prhs[4]) || mxGetNumberOfElements(prhs[4]) != (mwSize)(2 * A))
        mexErrMsgIdAndTxt("fmcw:arg", "ra_steer: cal must be a real double array of 2 A values (re, im per plane)");
      for (int i = 0; i < 2 * A; ++i) cal[i] = (float)mxGetDoubles(prhs[4])[i];
      pc = cal;
    }
    if (nrhs > 5 && mxGetNumberOfElements(prhs[5]) > 0) {
      if (!mxIsDouble(prhs[5]) || mxIsComplex(prhs[5]) || mxGetNumberOfElements(prhs[5]) != (mwSize)A)
        mexErrMsgIdAndTxt("fmcw:arg", "ra_steer: taper must be a real double array of A values");
      for (int i = 0; i < A; ++i) taper[i] = (float)mxGetDoubles(prhs[5])[i];
      pt = taper;
    }
    check(fmcw_ra_steer(A, (int32_t)K, (float)mxGetScalar(prhs[2]), st, pc, pt, nrhs > 6 ? mxGetScalar(prhs[6]) != 0 : 1, wf));
    plhs[0] = mxCreateDoubleMatrix((mwSize)(2 * A), K, mxREAL);
    for (mwSize i = 0; i < K * (mwSize)(2 * A); ++i) mxGetDoubles(plhs[0])[i] = wf[i];
    return;
  }
  if (!g_ctx) mexErrMsgIdAndTxt("fmcw:state", "call fmcw_mex('init') first");

  if (!strcmp(cmd, "taps")) {               /* fmcw_mex('taps', P, range_win, doppler_win, calib_rx1) */
    if (nrhs != 5) mexErrMsgIdAndTxt("fmcw:arg", "taps: P, range_win, doppler_win, calib");
    fmcw_params p = params_of(prhs[1]);
    const float* wr = single_real(prhs[2], p.nts, "range_win");
    const float* wd = single_real(prhs[3], p.pn, "doppler_win");
    if (!mxIsSingle(prhs[4]) || !mxIsComplex(prhs[4]) || mxGetNumberOfElements(prhs[4]) != (mwSize)p.nts)
      mexErrMsgIdAndTxt("fmcw:arg", "calib must be single complex, NTS elements");
    check(fmcw_set_taps(g_ctx, &p, wr, wd, (const float*)mxGetComplexSingles(prhs[4])));
    return;
  }

  if (!strcmp(cmd, "process")) {            /* fmcw_mex('process', P, iq, probe_column) */
    if (nrhs != 4) mexErrMsgIdAndTxt("fmcw:arg", "process: P, iq, probe_column");
    fmcw_params p = params_of(prhs[1]);
    const mxArray* iq = prhs[2];
    if (!mxIsSingle(iq) || !mxIsComplex(iq)) mexErrMsgIdAndTxt("fmcw:arg", "iq must be single complex NTS x PN x F");
    const mwSize nd = mxGetNumberOfDimensions(iq);
    const mwSize* dims = mxGetDimensions(iq);
    if (dims[0] != (mwSize)p.nts || dims[1] != (mwSize)p.pn) mexErrMsgIdAndTxt("fmcw:arg", "iq must be NTS x PN x F");
    const int64_t F = nd >= 3 ? (int64_t)dims[2] : 1;
    const int64_t probe = (int64_t)mxGetScalar(prhs[3]);
    const mwSize M = (mwSize)p.max_targets;
    plhs[0] = mxCreateNumericMatrix(p.nr, F, mxSINGLE_CLASS, mxREAL);   /* range_tx1rx1_max_abs */
    plhs[1] = mxCreateNumericMatrix(1, F, mxINT32_CLASS, mxREAL);
    plhs[2] = mxCreateNumericMatrix(M, F, mxINT32_CLASS, mxREAL);
    plhs[3] = mxCreateNumericMatrix(M, F, mxSINGLE_CLASS, mxREAL);
    plhs[4] = mxCreateNumericMatrix(M, F, mxINT32_CLASS, mxREAL);
    plhs[5] = mxCreateNumericMatrix(p.pn, F, mxSINGLE_CLASS, mxREAL);
    plhs[6] = mxCreateNumericMatrix(p.nr, 1, mxSINGLE_CLASS, mxREAL);
    check(fmcw_process(g_ctx, &p, mxGetComplexSingles(iq), FMCW_C64, F, mxGetSingles(plhs[0]),
                       mxGetInt32s(plhs[1]), mxGetInt32s(plhs[2]), mxGetSingles(plhs[3]), mxGetInt32s(plhs[4]),
                       mxGetSingles(plhs[5]), NULL, NULL, probe, probe > 0 ? mxGetSingles(plhs[6]) : NULL));
    return;
  }

  if (!strcmp(cmd, "stft") || !strcmp(cmd, "stft_png")) {
    /* fmcw_mex('stft', x, win, noverlap, nfft, fs, n_log_bins [, png_path]) */
    const int png = !strcmp(cmd, "stft_png");
    if (nrhs != 7 + png) mexErrMsgIdAndTxt("fmcw:arg", "stft: x, win, noverlap, nfft, fs, n_log_bins[, png_path]");
    char png_path[4096] = {0};
    if (png && (!mxIsChar(prhs[7]) || mxGetString(prhs[7], png_path, sizeof png_path)))
      mexErrMsgIdAndTxt("fmcw:arg", "stft_png: png_path must be a char row");
    const int64_t L = (int64_t)mxGetNumberOfElements(prhs[1]);
    const float* x = single_real(prhs[1], (mwSize)L, "x");
    const int32_t wlen = (int32_t)mxGetNumberOfElements(prhs[2]);
    const float* w = single_real(prhs[2], (mwSize)wlen, "win");
    const int32_t nov = (int32_t)mxGetScalar(prhs[3]), nfft = (int32_t)mxGetScalar(prhs[4]);
    const double fs = mxGetScalar(prhs[5]);
    const int32_t nlog = (int32_t)mxGetScalar(prhs[6]);
    int64_t nseg = 0;
    int32_t nf = 0, nb = 0;
    check(fmcw_stft_sizes(L, wlen, nov, nfft, nlog, &nseg, &nf, &nb));
    plhs[0] = mxCreateNumericMatrix(1, nseg, mxSINGLE_CLASS, mxREAL);   /* T */
    plhs[1] = mxCreateNumericMatrix(1, nb, mxSINGLE_CLASS, mxREAL);     /* log_freq_bins / F */
    plhs[2] = mxCreateNumericMatrix(nb, nseg, mxSINGLE_CLASS, mxREAL);  /* interp_intensity */
    if (png)
      check(fmcw_stft_png(g_ctx, x, L, w, wlen, nov, nfft, fs, nlog, mxGetSingles(plhs[0]), mxGetSingles(plhs[1]),
                          mxGetSingles(plhs[2]), png_path, 0, 0, NULL));
    else
      check(fmcw_stft(g_ctx, x, L, w, wlen, nov, nfft, fs, nlog, mxGetSingles(plhs[0]), mxGetSingles(plhs[1]),
                      mxGetSingles(plhs[2])));
    return;
  }
  const int os = !strcmp(cmd, "oscfar");    /* 'oscfar': the outputs of 'cfar', Q with the field rank besides */
  if (os || !strcmp(cmd, "cfar")) {         /* [cnt, ridx, didx, power, noise] = fmcw_mex('cfar', Q, rd) */
    if (nrhs != 3) mexErrMsgIdAndTxt("fmcw:arg", os ? "oscfar: Q, rd" : "cfar: Q, rd");
    const mxArray* s = prhs[1];
    const mxArray* rd = prhs[2];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    fmcw_cfar_params q;
    q.guard_r = (int32_t)field(s, "guard_r");
    q.guard_d = (int32_t)field(s, "guard_d");
    q.train_r = (int32_t)field(s, "train_r");
    q.train_d = (int32_t)field(s, "train_d");
    q.r_lo = (int32_t)field(s, "r_lo");
    q.r_hi = (int32_t)field(s, "r_hi");
    q.max_det = (int32_t)field(s, "max_det");
    q.flags = (int32_t)field(s, "flags");
    q.alpha = (float)field(s, "alpha");
    if (!mxIsSingle(rd) || !mxIsComplex(rd) || mxGetNumberOfDimensions(rd) < 2)
      mexErrMsgIdAndTxt("fmcw:arg", "rd must be single complex Nd x Nr x F");
    const mwSize* dims = mxGetDimensions(rd);
    const int64_t F = mxGetNumberOfDimensions(rd) >= 3 ? (int64_t)dims[2] : 1;
    const int32_t nd = (int32_t)dims[0], nr = (int32_t)dims[1];
    fmcw_oscfar_params qo;
    qo.win = q;
    qo.rank = os ? (int32_t)field(s, "rank") : 1;
    check(os ? fmcw_oscfar_check(&qo, nr, nd, NULL) : fmcw_cfar_check(&q, nr, nd, NULL));   /* before max_det sizes the outputs */
    const mwSize K = (mwSize)q.max_det;
    plhs[0] = mxCreateNumericMatrix(1, F, mxINT32_CLASS, mxREAL);    /* detections found per frame */
    plhs[1] = mxCreateNumericMatrix(K, F, mxINT32_CLASS, mxREAL);    /* range index, 1-based, 0 = unused */
    plhs[2] = mxCreateNumericMatrix(K, F, mxINT32_CLASS, mxREAL);    /* Doppler index */
    plhs[3] = mxCreateNumericMatrix(K, F, mxSINGLE_CLASS, mxREAL);   /* |D|^2 of the cell */
    plhs[4] = mxCreateNumericMatrix(K, F, mxSINGLE_CLASS, mxREAL);   /* noise estimate S / N ('oscfar': X_(k)) */
    if (os)
      check(fmcw_oscfar(g_ctx, &qo, mxGetComplexSingles(rd), FMCW_C64, F, nr, nd, mxGetInt32s(plhs[0]),
                        mxGetInt32s(plhs[1]), mxGetInt32s(plhs[2]), mxGetSingles(plhs[3]), mxGetSingles(plhs[4]), NULL));
    else
      check(fmcw_cfar(g_ctx, &q, mxGetComplexSingles(rd), FMCW_C64, F, nr, nd, mxGetInt32s(plhs[0]), mxGetInt32s(plhs[1]),
                      mxGetInt32s(plhs[2]), mxGetSingles(plhs[3]), mxGetSingles(plhs[4]), NULL));
    return;
  }
  if (!strcmp(cmd, "signature")) {          /* [dt, rt, dt_max, rt_max] = fmcw_mex('signature', Q, rd[, center]) */
    if (nrhs != 3 && nrhs != 4) mexErrMsgIdAndTxt("fmcw:arg", "signature: Q, rd[, center]");
    const mxArray* s = prhs[1];
    const mxArray* rd = prhs[2];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    fmcw_sig_params q;
    q.r_lo = (int32_t)field(s, "r_lo");
    q.r_hi = (int32_t)field(s, "r_hi");
    q.track_half = (int32_t)field(s, "track_half");
    q.dc_half = (int32_t)field(s, "dc_half");
    q.flags = (int32_t)field(s, "flags");
    q.floor_db = (float)field(s, "floor_db");
    if (!mxIsSingle(rd) || !mxIsComplex(rd) || mxGetNumberOfDimensions(rd) < 2)
      mexErrMsgIdAndTxt("fmcw:arg", "rd must be single complex Nd x Nr x F");
    const mwSize* dims = mxGetDimensions(rd);
    const int64_t F = mxGetNumberOfDimensions(rd) >= 3 ? (int64_t)dims[2] : 1;
    const int32_t nd = (int32_t)dims[0], nr = (int32_t)dims[1];
    check(fmcw_sig_check(&q, nr, nd));
    const int32_t* center = NULL;
    if (nrhs == 4 && mxGetNumberOfElements(prhs[3]) > 0) {
      if (!mxIsInt32(prhs[3]) || (int64_t)mxGetNumberOfElements(prhs[3]) != F)
        mexErrMsgIdAndTxt("fmcw:arg", "center must be int32 with one entry per frame");
      center = mxGetInt32s(prhs[3]);
    }
    float dmx = 0.f, rmx = 0.f;
    plhs[0] = mxCreateNumericMatrix((mwSize)nd, (mwSize)F, mxSINGLE_CLASS, mxREAL);   /* Doppler-time map */
    plhs[1] = mxCreateNumericMatrix((mwSize)nr, (mwSize)F, mxSINGLE_CLASS, mxREAL);   /* range-time map */
    check(fmcw_sig(g_ctx, &q, mxGetComplexSingles(rd), FMCW_C64, F, nr, nd, center, 1, mxGetSingles(plhs[0]),
                   mxGetSingles(plhs[1]), &dmx, &rmx));
    plhs[2] = mxCreateDoubleScalar((double)dmx);
    plhs[3] = mxCreateDoubleScalar((double)rmx);
    return;
  }
  if (!strcmp(cmd, "cluster")) {            /* [tcnt, cells, ...] = fmcw_mex('cluster', Q, cnt, ridx, didx, power, noise, nr, nd) */
    if (nrhs != 9) mexErrMsgIdAndTxt("fmcw:arg", "cluster: Q, cnt, ridx, didx, power, noise, nr, nd");
    const mxArray* s = prhs[1];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    fmcw_cluster_params q;
    q.link_r = (int32_t)field(s, "link_r");
    q.link_d = (int32_t)field(s, "link_d");
    q.min_cells = (int32_t)field(s, "min_cells");
    q.max_tgt = (int32_t)field(s, "max_tgt");
    q.flags = (int32_t)field(s, "flags");
    const int32_t nr = (int32_t)mxGetScalar(prhs[7]), nd = (int32_t)mxGetScalar(prhs[8]);
    if (!mxIsInt32(prhs[2]) || !mxIsInt32(prhs[3]) || !mxIsInt32(prhs[4]))
      mexErrMsgIdAndTxt("fmcw:arg", "cnt, ridx and didx must be int32");
    const int64_t F = (int64_t)mxGetNumberOfElements(prhs[2]);
    const mwSize K = mxGetM(prhs[3]);
    check(fmcw_cluster_check(&q, nr, nd, (int32_t)K));   /* before max_tgt sizes the outputs */
    const mwSize n = K * (mwSize)F, M = (mwSize)q.max_tgt;
    if (mxGetNumberOfElements(prhs[3]) != n || mxGetNumberOfElements(prhs[4]) != n)
      mexErrMsgIdAndTxt("fmcw:arg", "ridx and didx must be max_det x F");
    const float* power = single_real(prhs[5], n, "power");
    const float* noise = mxGetNumberOfElements(prhs[6]) > 0 ? single_real(prhs[6], n, "noise") : NULL;
    /* outputs past nlhs do not exist: their pointers stay NULL and the library leaves them out */
    const int want = nlhs > 1 ? nlhs : 1;
    void* o[12] = {0};
    for (int i = 0; i < 12 && i < want; ++i) {
      const int is_f = i >= 6 && i <= 10;
      plhs[i] = mxCreateNumericMatrix(i == 0 ? 1 : i == 11 ? K : M, (mwSize)F, is_f ? mxSINGLE_CLASS : mxINT32_CLASS, mxREAL);
      o[i] = is_f ? (void*)mxGetSingles(plhs[i]) : (void*)mxGetInt32s(plhs[i]);
    }
    fmcw_targets t;
    t.tgt_count = (int32_t*)o[0];
    t.cells = (int32_t*)o[1];
    t.peak_range_idx = (int32_t*)o[2];
    t.peak_doppler_idx = (int32_t*)o[3];
    t.extent_r = (int32_t*)o[4];
    t.extent_d = (int32_t*)o[5];
    t.peak_power = (float*)o[6];
    t.peak_noise = (float*)o[7];
    t.power = (float*)o[8];
    t.range = (float*)o[9];
    t.doppler = (float*)o[10];
    check(fmcw_cluster(g_ctx, &q, F, nr, nd, (int32_t)K, mxGetInt32s(prhs[2]), mxGetInt32s(prhs[3]), mxGetInt32s(prhs[4]),
                       power, noise, &t, (int32_t*)o[11]));
    return;
  }
  if (!strcmp(cmd, "aoa")) {                /* [zre, zim, phase, sn, tzre, ...] = fmcw_mex('aoa', Q, rd4, cnt, ridx, didx[, label]) */
    if (nrhs != 6 && nrhs != 7) mexErrMsgIdAndTxt("fmcw:arg", "aoa: Q, rd4, cnt, ridx, didx[, label]");
    const mxArray* s = prhs[1];
    const mxArray* rd = prhs[2];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    if (!mxIsSingle(rd) || !mxIsComplex(rd) || mxGetNumberOfDimensions(rd) != 4)
      mexErrMsgIdAndTxt("fmcw:arg", "rd4 must be single complex Nd x Nr x F x A");
    const mwSize* dims = mxGetDimensions(rd);
    const int32_t nd = (int32_t)dims[0], nr = (int32_t)dims[1];
    const int64_t F = (int64_t)dims[2];
    fmcw_aoa_params q;
    memset(&q, 0, sizeof q);
    q.n_chan = (int32_t)dims[3];
    q.max_tgt = (int32_t)field(s, "max_tgt");
    q.flags = (int32_t)field(s, "flags");
    q.spacing = (float)field(s, "spacing");
    for (int i = 0; i < 8; ++i) q.w[2 * i] = 1.f;
    const mxArray* w = mxGetField(s, 0, "w");
    if (w && mxGetNumberOfElements(w) > 0) {
      if (!mxIsDouble(w) || mxIsComplex(w) || q.n_chan < 1 || q.n_chan > 8 || mxGetNumberOfElements(w) != (mwSize)(2 * q.n_chan))
        mexErrMsgIdAndTxt("fmcw:arg", "Q.w must be a real double array of 2 A values (re, im per plane)");
      for (int i = 0; i < 2 * q.n_chan; ++i) q.w[i] = (float)mxGetDoubles(w)[i];
    }
    if (!mxIsInt32(prhs[3]) || !mxIsInt32(prhs[4]) || !mxIsInt32(prhs[5]))
      mexErrMsgIdAndTxt("fmcw:arg", "cnt, ridx and didx must be int32");
    const mwSize K = mxGetM(prhs[4]);
    check(fmcw_aoa_check(&q, nr, nd, (int32_t)K));   /* before max_tgt and n_chan size anything */
    const mwSize n = K * (mwSize)F, M = (mwSize)q.max_tgt;
    if ((int64_t)mxGetNumberOfElements(prhs[3]) != F || mxGetNumberOfElements(prhs[4]) != n || mxGetNumberOfElements(prhs[5]) != n)
      mexErrMsgIdAndTxt("fmcw:arg", "cnt must be 1 x F, ridx and didx max_det x F");
    const int32_t* label = NULL;
    if (nrhs == 7 && mxGetNumberOfElements(prhs[6]) > 0) {
      if (!mxIsInt32(prhs[6]) || mxGetNumberOfElements(prhs[6]) != n) mexErrMsgIdAndTxt("fmcw:arg", "label must be int32 max_det x F");
      label = mxGetInt32s(prhs[6]);
    }
    const void* chan[8] = {0};
    for (int a = 0; a < q.n_chan; ++a) chan[a] = mxGetComplexSingles(rd) + (size_t)a * (size_t)F * (size_t)nr * (size_t)nd;
    /* outputs past nlhs do not exist: their pointers stay NULL and the library leaves them out; the
     * per-target ones need the labels and max_tgt >= 1 */
    const int most = label && M > 0 ? 12 : 4;
    if (nlhs > most) mexErrMsgIdAndTxt("fmcw:arg", "aoa: the per-target outputs need label and max_tgt >= 1");
    const int want = nlhs > 1 ? nlhs : 1;
    void* o[12] = {0};
    for (int i = 0; i < want; ++i) {
      plhs[i] = mxCreateNumericMatrix(i < 4 ? K : M, (mwSize)F, i == 11 ? mxINT32_CLASS : mxSINGLE_CLASS, mxREAL);
      o[i] = i == 11 ? (void*)mxGetInt32s(plhs[i]) : (void*)mxGetSingles(plhs[i]);
    }
    fmcw_angles t;
    t.det_zre = (float*)o[0];
    t.det_zim = (float*)o[1];
    t.det_phase = (float*)o[2];
    t.det_sin = (float*)o[3];
    t.tgt_zre = (float*)o[4];
    t.tgt_zim = (float*)o[5];
    t.tgt_e0 = (float*)o[6];
    t.tgt_e1 = (float*)o[7];
    t.tgt_phase = (float*)o[8];
    t.tgt_sin = (float*)o[9];
    t.tgt_coh = (float*)o[10];
    t.tgt_cells = (int32_t*)o[11];
    check(fmcw_aoa(g_ctx, &q, chan, FMCW_C64, F, nr, nd, (int32_t)K, mxGetInt32s(prhs[3]), mxGetInt32s(prhs[4]),
                   mxGetInt32s(prhs[5]), label, &t));
    return;
  }
  if (!strcmp(cmd, "track")) {              /* [kcnt, id, ...] = fmcw_mex('track', Q, tcnt, range, doppler, power, nr, nd, nseq[, state]) */
    if (nrhs != 9 && nrhs != 10) mexErrMsgIdAndTxt("fmcw:arg", "track: Q, tcnt, range, doppler, power, nr, nd, nseq[, state]");
    const mxArray* s = prhs[1];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    fmcw_track_params q;
    q.gate_r = (float)field(s, "gate_r");
    q.gate_d = (float)field(s, "gate_d");
    q.alpha_r = (float)field(s, "alpha_r");
    q.alpha_d = (float)field(s, "alpha_d");
    q.beta_r = (float)field(s, "beta_r");
    q.confirm_hits = (int32_t)field(s, "confirm_hits");
    q.max_coast = (int32_t)field(s, "max_coast");
    q.max_trk = (int32_t)field(s, "max_trk");
    q.flags = (int32_t)field(s, "flags");
    const int32_t nr = (int32_t)mxGetScalar(prhs[6]), nd = (int32_t)mxGetScalar(prhs[7]);
    const int64_t S = (int64_t)mxGetScalar(prhs[8]);
    if (!mxIsInt32(prhs[2])) mexErrMsgIdAndTxt("fmcw:arg", "tcnt must be int32");
    const int64_t rows = (int64_t)mxGetNumberOfElements(prhs[2]);
    const mwSize M = mxGetM(prhs[3]);
    check(fmcw_track_check(&q, nr, nd, (int32_t)M));     /* before max_trk sizes the outputs */
    if (S < 1 || rows % S) mexErrMsgIdAndTxt("fmcw:arg", "nseq must divide the number of frames");
    const int64_t F = rows / S;
    const mwSize n = M * (mwSize)rows, T = (mwSize)q.max_trk;
    const float* range = single_real(prhs[3], n, "range");
    const float* doppler = single_real(prhs[4], n, "doppler");
    const float* power = single_real(prhs[5], n, "power");
    const mwSize sw = (mwSize)fmcw_track_state_bytes(q.max_trk) / 4;   /* a multiple of 16 bytes: int32 words */
    /* the state comes back as output 11: a copy of the input state carried on, or a fresh (zero) one;
       MATLAB frees the array itself when it is not returned */
    mxArray* st = NULL;
    const int carried = nrhs == 10 && mxGetNumberOfElements(prhs[9]) > 0;
    if (carried && (!mxIsInt32(prhs[9]) || mxGetNumberOfElements(prhs[9]) != sw * (mwSize)S))
      mexErrMsgIdAndTxt("fmcw:arg", "state must be int32, fmcw_track_state_bytes(max_trk)/4 x nseq");
    if (carried || nlhs > 10) st = mxCreateNumericMatrix(sw, (mwSize)S, mxINT32_CLASS, mxREAL);
    if (carried) memcpy(mxGetInt32s(st), mxGetInt32s(prhs[9]), sw * (size_t)S * 4);
    /* outputs past nlhs do not exist: their pointers stay NULL and the library leaves them out */
    const int want = nlhs > 1 ? nlhs : 1;
    void* o[10] = {0};
    for (int i = 0; i < 10 && i < want; ++i) {
      const int is_f = i >= 5 && i <= 8;
      plhs[i] = mxCreateNumericMatrix(i == 0 ? 1 : i == 9 ? M : T, (mwSize)rows, is_f ? mxSINGLE_CLASS : mxINT32_CLASS, mxREAL);
      o[i] = is_f ? (void*)mxGetSingles(plhs[i]) : (void*)mxGetInt32s(plhs[i]);
    }
    fmcw_tracks t;
    t.trk_count = (int32_t*)o[0];
    t.trk_id = (int32_t*)o[1];
    t.trk_status = (int32_t*)o[2];
    t.trk_age = (int32_t*)o[3];
    t.trk_misses = (int32_t*)o[4];
    t.trk_range = (float*)o[5];
    t.trk_range_rate = (float*)o[6];
    t.trk_doppler = (float*)o[7];
    t.trk_power = (float*)o[8];
    check(fmcw_track(g_ctx, &q, S, F, nr, nd, (int32_t)M, mxGetInt32s(prhs[2]), range, doppler, power,
                     st ? (void*)mxGetInt32s(st) : NULL, &t, (int32_t*)o[9]));
    if (nlhs > 10) plhs[10] = st;
    return;
  }
  if (!strcmp(cmd, "mti")) {                /* [out, bg, seen] = fmcw_mex('mti', Q, rd, nseq[, bg, seen]) */
    if (nrhs != 4 && nrhs != 6) mexErrMsgIdAndTxt("fmcw:arg", "mti: Q, rd, nseq[, bg, seen]");
    const mxArray* s = prhs[1];
    const mxArray* rd = prhs[2];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    fmcw_mti_params q;
    q.lambda = (float)field(s, "lambda");
    q.flags = (int32_t)field(s, "flags");
    if (!mxIsSingle(rd) || !mxIsComplex(rd) || mxGetNumberOfDimensions(rd) < 2)
      mexErrMsgIdAndTxt("fmcw:arg", "rd must be single complex Nd x Nr x (nseq*F)");
    const mwSize* dims = mxGetDimensions(rd);
    const int64_t rows = mxGetNumberOfDimensions(rd) >= 3 ? (int64_t)dims[2] : 1;
    const int32_t nd = (int32_t)dims[0], nr = (int32_t)dims[1];
    const int64_t S = (int64_t)mxGetScalar(prhs[3]);
    check(fmcw_mti_check(&q, nr, nd));
    if (S < 1 || rows % S) mexErrMsgIdAndTxt("fmcw:arg", "nseq must divide the number of frames");
    const mwSize cells = (mwSize)nd * (mwSize)nr;
    /* the state comes back as outputs 2 and 3: a copy of the input state carried on, or a fresh (zero) one */
    const int carried = nrhs == 6 && mxGetNumberOfElements(prhs[4]) > 0;
    if (carried && (!mxIsSingle(prhs[4]) || !mxIsComplex(prhs[4]) || mxGetNumberOfElements(prhs[4]) != cells * (mwSize)S ||
                    !mxIsInt32(prhs[5]) || mxGetNumberOfElements(prhs[5]) != (mwSize)S))
      mexErrMsgIdAndTxt("fmcw:arg", "bg must be single complex Nd x Nr x nseq and seen int32 with nseq entries");
    plhs[0] = mxCreateNumericMatrix(cells, (mwSize)rows, mxSINGLE_CLASS, mxCOMPLEX);
    mxArray* bg = mxCreateNumericMatrix(cells, (mwSize)S, mxSINGLE_CLASS, mxCOMPLEX);
    mxArray* seen = mxCreateNumericMatrix(1, (mwSize)S, mxINT32_CLASS, mxREAL);
    if (carried) {
      memcpy(mxGetComplexSingles(bg), mxGetComplexSingles(prhs[4]), cells * (size_t)S * sizeof(mxComplexSingle));
      memcpy(mxGetInt32s(seen), mxGetInt32s(prhs[5]), (size_t)S * 4);
    }
    check(fmcw_mti(g_ctx, &q, mxGetComplexSingles(rd), FMCW_C64, S, rows / S, nr, nd, (float*)mxGetComplexSingles(bg),
                   mxGetInt32s(seen), mxGetComplexSingles(plhs[0])));
    if (nlhs > 1) plhs[1] = bg;
    if (nlhs > 2) plhs[2] = seen;
    return;
  }
  if (!strcmp(cmd, "beam")) {               /* out = fmcw_mex('beam', Q, rd4) */
    if (nrhs != 3) mexErrMsgIdAndTxt("fmcw:arg", "beam: Q, rd4");
    const mxArray* s = prhs[1];
    const mxArray* rd = prhs[2];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    if (!mxIsSingle(rd) || !mxIsComplex(rd) || mxGetNumberOfDimensions(rd) != 4)
      mexErrMsgIdAndTxt("fmcw:arg", "rd4 must be single complex Nd x Nr x F x A");
    const mwSize* dims = mxGetDimensions(rd);
    const int32_t nd = (int32_t)dims[0], nr = (int32_t)dims[1];
    const int64_t F = (int64_t)dims[2];
    const mwSize A = dims[3];
    const mxArray* w = mxGetField(s, 0, "w");
    if (A < 2 || A > 8 || !w || !mxIsDouble(w) || mxIsComplex(w) || mxGetNumberOfElements(w) == 0 ||
        mxGetNumberOfElements(w) % (2 * A) || mxGetNumberOfElements(w) > 16 * A)
      mexErrMsgIdAndTxt("fmcw:arg", "A must be in 2..8 and Q.w a real double array of 2 x A x B values (re, im; plane; beam), B in 1..8");
    fmcw_beam_params q;
    memset(&q, 0, sizeof q);
    q.n_chan = (int32_t)A;
    q.n_beam = (int32_t)(mxGetNumberOfElements(w) / (2 * A));
    q.flags = (int32_t)field(s, "flags");
    for (int b = 0; b < q.n_beam; ++b)
      for (mwSize i = 0; i < 2 * A; ++i) q.w[b][i / 2][i % 2] = (float)mxGetDoubles(w)[(mwSize)b * 2 * A + i];
    check(fmcw_beam_check(&q, nr, nd));
    const size_t map = (size_t)F * (size_t)nr * (size_t)nd;
    plhs[0] = mxCreateNumericMatrix((mwSize)map, (mwSize)q.n_beam, mxSINGLE_CLASS, mxCOMPLEX);
    const void* chan[8] = {0};
    void* out[8] = {0};
    for (mwSize a = 0; a < A; ++a) chan[a] = mxGetComplexSingles(rd) + a * map;
    for (int b = 0; b < q.n_beam; ++b) out[b] = mxGetComplexSingles(plhs[0]) + (size_t)b * map;
    check(fmcw_beam(g_ctx, &q, chan, FMCW_C64, F, nr, nd, out));
    return;
  }
  if (!strcmp(cmd, "ra")) {                 /* [ra, cov, ra_max] = fmcw_mex('ra', Q, rd4, w) */
    if (nrhs != 4) mexErrMsgIdAndTxt("fmcw:arg", "ra: Q, rd4, w");
    const mxArray* s = prhs[1];
    const mxArray* rd = prhs[2];
    const mxArray* w = prhs[3];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    if (!mxIsSingle(rd) || !mxIsComplex(rd) || mxGetNumberOfDimensions(rd) != 4)
      mexErrMsgIdAndTxt("fmcw:arg", "rd4 must be single complex Nd x Nr x F x A");
    const mwSize* dims = mxGetDimensions(rd);
    const int32_t nd = (int32_t)dims[0], nr = (int32_t)dims[1];
    const int64_t F = (int64_t)dims[2];
    const mwSize A = dims[3];
    if (A < 2 || A > 8 || !mxIsDouble(w) || mxIsComplex(w) || mxGetNumberOfElements(w) == 0 ||
        mxGetNumberOfElements(w) % (2 * A) || mxGetNumberOfElements(w) > 512 * A)
      mexErrMsgIdAndTxt("fmcw:arg", "A must be in 2..8 and w a real double array of 2 x A x K values (re, im; plane; direction), K in 1..256");
    fmcw_ra_params q;
    memset(&q, 0, sizeof q);
    q.n_chan = (int32_t)A;
    q.n_ang = (int32_t)(mxGetNumberOfElements(w) / (2 * A));
    q.r_lo = (int32_t)field(s, "r_lo");
    q.r_hi = (int32_t)field(s, "r_hi");
    q.dc_half = (int32_t)field(s, "dc_half");
    q.flags = (int32_t)field(s, "flags");
    q.load = (float)field(s, "load");
    check(fmcw_ra_check(&q, nr, nd));
    float* wf = (float*)mxCalloc(mxGetNumberOfElements(w), sizeof(float));   /* freed with the MEX call's memory */
    for (mwSize i = 0; i < mxGetNumberOfElements(w); ++i) wf[i] = (float)mxGetDoubles(w)[i];
    const size_t map = (size_t)F * (size_t)nr * (size_t)nd;
    const mwSize T = A * (A + 1) / 2;
    plhs[0] = mxCreateNumericMatrix((mwSize)q.n_ang, (mwSize)nr * (mwSize)F, mxSINGLE_CLASS, mxREAL);
    mxArray* cov = mxCreateNumericMatrix(2 * T, (mwSize)nr * (mwSize)F, mxSINGLE_CLASS, mxREAL);
    const void* chan[8] = {0};
    for (mwSize a = 0; a < A; ++a) chan[a] = mxGetComplexSingles(rd) + a * map;
    float mx = 0.f;
    check(fmcw_ra(g_ctx, &q, chan, FMCW_C64, F, nr, nd, wf, mxGetSingles(cov), mxGetSingles(plhs[0]), &mx));
    if (nlhs > 1) plhs[1] = cov;
    if (nlhs > 2) plhs[2] = mxCreateDoubleScalar((double)mx);
    return;
  }
  if (!strcmp(cmd, "music")) {              /* [music, nsrc, eval, evec, music_max] = fmcw_mex('music', Q, cov, nr, w) */
    if (nrhs != 5) mexErrMsgIdAndTxt("fmcw:arg", "music: Q, cov, nr, w");
    const mxArray* s = prhs[1];
    const mxArray* cov = prhs[2];
    const mxArray* w = prhs[4];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    if (!mxIsSingle(cov) || mxIsComplex(cov) || mxGetNumberOfDimensions(cov) != 2)
      mexErrMsgIdAndTxt("fmcw:arg", "cov must be real single (2*T) x (Nr*F)");
    mwSize A = 0;
    for (mwSize a = 2; a <= 8; ++a)
      if (mxGetM(cov) == a * (a + 1)) A = a;
    const int32_t nr = (int32_t)mxGetScalar(prhs[3]);
    if (A == 0 || nr < 1 || mxGetN(cov) % (mwSize)nr)
      mexErrMsgIdAndTxt("fmcw:arg", "cov must have A (A + 1) rows, A in 2..8, and a multiple of nr columns");
    const int64_t F = (int64_t)(mxGetN(cov) / (mwSize)nr);
    if (!mxIsDouble(w) || mxIsComplex(w) || mxGetNumberOfElements(w) == 0 || mxGetNumberOfElements(w) % (2 * A) ||
        mxGetNumberOfElements(w) > 512 * A)
      mexErrMsgIdAndTxt("fmcw:arg", "w must be a real double array of 2 x A x K values (re, im; plane; direction), K in 1..256");
    fmcw_music_params q;
    memset(&q, 0, sizeof q);
    q.n_chan = (int32_t)A;
    q.n_ang = (int32_t)(mxGetNumberOfElements(w) / (2 * A));
    q.r_lo = (int32_t)field(s, "r_lo");
    q.r_hi = (int32_t)field(s, "r_hi");
    q.n_src = (int32_t)field(s, "n_src");
    q.max_src = (int32_t)field(s, "max_src");
    q.sweeps = (int32_t)field(s, "sweeps");
    q.flags = (int32_t)field(s, "flags");
    q.src_thr = (float)field(s, "src_thr");
    check(fmcw_music_check(&q, nr));
    float* wf = (float*)mxCalloc(mxGetNumberOfElements(w), sizeof(float));   /* freed with the MEX call's memory */
    for (mwSize i = 0; i < mxGetNumberOfElements(w); ++i) wf[i] = (float)mxGetDoubles(w)[i];
    const mwSize rows = mxGetN(cov);
    plhs[0] = mxCreateNumericMatrix((mwSize)q.n_ang, rows, mxSINGLE_CLASS, mxREAL);
    mxArray* nsrc = mxCreateNumericMatrix(1, rows, mxINT32_CLASS, mxREAL);
    mxArray* eval = mxCreateNumericMatrix(A, rows, mxSINGLE_CLASS, mxREAL);
    mxArray* evec = mxCreateNumericMatrix(2 * A * A, rows, mxSINGLE_CLASS, mxREAL);
    float mx = 0.f;
    check(fmcw_music(g_ctx, &q, mxGetSingles(cov), F, nr, wf, mxGetSingles(eval), mxGetSingles(evec), mxGetInt32s(nsrc),
                     mxGetSingles(plhs[0]), &mx));
    if (nlhs > 1) plhs[1] = nsrc;
    if (nlhs > 2) plhs[2] = eval;
    if (nlhs > 3) plhs[3] = evec;
    if (nlhs > 4) plhs[4] = mxCreateDoubleScalar((double)mx);
    return;
  }
  if (!strcmp(cmd, "doa")) {                /* [idx, count, pow, sn, base] = fmcw_mex('doa', Q, spec, nr, sin_theta) */
    if (nrhs != 5) mexErrMsgIdAndTxt("fmcw:arg", "doa: Q, spec, nr, sin_theta");
    const mxArray* s = prhs[1];
    const mxArray* spec = prhs[2];
    const mxArray* st = prhs[4];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("fmcw:arg", "Q must be a struct");
    if (!mxIsSingle(spec) || mxIsComplex(spec) || mxGetNumberOfDimensions(spec) != 2)
      mexErrMsgIdAndTxt("fmcw:arg", "spec must be real single K x (Nr*F)");
    const mwSize K = mxGetM(spec);
    const int32_t nr = (int32_t)mxGetScalar(prhs[3]);
    if (K < 1 || K > 256 || nr < 1 || mxGetN(spec) % (mwSize)nr)
      mexErrMsgIdAndTxt("fmcw:arg", "spec must have K rows, K in 1..256, and a multiple of nr columns");
    const int64_t F = (int64_t)(mxGetN(spec) / (mwSize)nr);
    if (!mxIsDouble(st) || mxIsComplex(st) || mxGetNumberOfElements(st) != K)
      mexErrMsgIdAndTxt("fmcw:arg", "sin_theta must be a real double array of K values");
    fmcw_doa_params q;
    memset(&q, 0, sizeof q);
    q.n_ang = (int32_t)K;
    q.r_lo = (int32_t)field(s, "r_lo");
    q.r_hi = (int32_t)field(s, "r_hi");
    q.max_pk = (int32_t)field(s, "max_pk");
    q.flags = (int32_t)field(s, "flags");
    q.min_abs = (float)field(s, "min_abs");
    q.min_rel = (float)field(s, "min_rel");
    q.min_prom = (float)field(s, "min_prom");
    check(fmcw_doa_check(&q, nr));
    float* u = (float*)mxCalloc(K, sizeof(float));                          /* freed with the MEX call's memory */
    for (mwSize i = 0; i < K; ++i) u[i] = (float)mxGetDoubles(st)[i];
    const mwSize rows = mxGetN(spec);
    plhs[0] = mxCreateNumericMatrix((mwSize)q.max_pk, rows, mxINT32_CLASS, mxREAL);
    mxArray* count = mxCreateNumericMatrix(1, rows, mxINT32_CLASS, mxREAL);
    mxArray* pw = mxCreateNumericMatrix((mwSize)q.max_pk, rows, mxSINGLE_CLASS, mxREAL);
    mxArray* sn = mxCreateNumericMatrix((mwSize)q.max_pk, rows, mxSINGLE_CLASS, mxREAL);
    mxArray* base = mxCreateNumericMatrix((mwSize)q.max_pk, rows, mxSINGLE_CLASS, mxREAL);
    check(fmcw_doa(g_ctx, &q, mxGetSingles(spec), F, nr, u, mxGetInt32s(count), mxGetInt32s(plhs[0]), mxGetSingles(pw),
                   mxGetSingles(sn), mxGetSingles(base)));
    if (nlhs > 1) plhs[1] = count;
    if (nlhs > 2) plhs[2] = pw;
    if (nlhs > 3) plhs[3] = sn;
    if (nlhs > 4) plhs[4] = base;
    return;
  }
  mexErrMsgIdAndTxt("fmcw:arg", "unknown command '%s'", cmd);
}
