"""Python handle on one libfmcw context (one HIP device, one stream).

Two call styles, both straight through the C-ABI of include/fmcw.h:

* host arrays (numpy) -- the same sequence a MEX gateway performs for MATLAB
  (``process``, ``range_fft``, ``stft``);
* device buffers (torch tensors used purely as HBM allocations, plus the
  torch stream) -- ``process_device`` and friends, for benches and the
  multi-GPU driver.
"""
from __future__ import annotations

import contextlib
import ctypes as ct

import numpy as np

from . import _lib
from ._lib import DOA_STAGE, FMCW_C32H, FMCW_C64, MUSIC_STAGE, STAGES, FmcwError, check
from .params import (AoaConfig, BeamConfig, CfarConfig, ClusterConfig, DoaConfig, FmcwConfig, MtiConfig, MusicConfig, OsCfarConfig,
                     RaConfig, SigConfig, TrackConfig)


def _ptr(a) -> ct.c_void_p:
    if a is None:
        return ct.c_void_p(0)
    if isinstance(a, np.ndarray):
        return ct.c_void_p(a.ctypes.data)
    return ct.c_void_p(int(a.data_ptr()))      # torch tensor (device pointer)


def _host_iq(iq: np.ndarray):
    """complex64 [F][C][S]  or  float16 [F][C][S][2] -> (array, dtype code)."""
    if iq.dtype == np.complex64:
        return np.ascontiguousarray(iq), FMCW_C64
    if iq.dtype == np.float16 and iq.shape[-1] == 2:
        return np.ascontiguousarray(iq), FMCW_C32H
    if np.iscomplexobj(iq):
        return np.ascontiguousarray(iq.astype(np.complex64)), FMCW_C64
    raise TypeError("iq must be complex64 [F][C][S] or float16 [F][C][S][2]")


def _host_rd(rd: np.ndarray, lead: str):
    """complex64 [lead][nr][nd]  or  float16 [lead][nr][nd][2] -> (contiguous array, dtype code)."""
    if rd.dtype == np.complex64 and rd.ndim == 3:
        return np.ascontiguousarray(rd), FMCW_C64
    if rd.dtype == np.float16 and rd.ndim == 4 and rd.shape[-1] == 2:
        return np.ascontiguousarray(rd), FMCW_C32H
    raise TypeError(f"rd must be complex64 [{lead}][nr][nd] or float16 [{lead}][nr][nd][2]")


class Engine:
    """fmcw_ctx on HIP device ``device`` -- an int, or a list of device ids for
    one context over several GPUs (the host-array calls then shard their work
    over them; include/fmcw.h fmcw_ctx_create).  No CPU fallback: raises if a
    device is absent."""

    def __init__(self, device: int | list | tuple | None = 0):
        self.lib = _lib.load()
        if device is None:                       # FMCW_DEVICES, else every visible device
            device = default_devices()
        ids = [int(device)] if isinstance(device, int) else [int(d) for d in device]
        arr = (ct.c_int32 * len(ids))(*ids)
        h = ct.c_void_p()
        check(self.lib.fmcw_ctx_create(len(ids), arr, ct.byref(h)))
        self.h = h
        self.device = ids[0]
        self.devices = ids
        self.cfg: FmcwConfig | None = None
        self.p = None

    def device_info(self) -> dict:
        """{'devices': [...], 'rccl': bool} of this context."""
        n, rc = ct.c_int32(), ct.c_int32()
        ids = (ct.c_int32 * 64)()
        check(self.lib.fmcw_ctx_devices(self.h, ct.byref(n), ids, ct.byref(rc)))
        return {"devices": list(ids[: n.value]), "rccl": bool(rc.value)}

    def close(self):
        if getattr(self, "h", None):
            self.lib.fmcw_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup ---------------------------------------------------------------
    def set_taps(self, cfg: FmcwConfig, cal: np.ndarray, range_win: np.ndarray | None = None,
                 doppler_win: np.ndarray | None = None) -> None:
        """radar_processing.m:138-139 windows and :174 calib_rx1 to the device."""
        wr = np.ascontiguousarray(cfg.range_window() if range_win is None else range_win, np.float32)
        wd = np.ascontiguousarray(cfg.doppler_window() if doppler_win is None else doppler_win, np.float32)
        c = np.ascontiguousarray(np.asarray(cal, np.complex128).astype(np.complex64))
        if wr.shape != (cfg.nts,) or wd.shape != (cfg.pn,) or c.shape != (cfg.nts,):
            raise ValueError("taps have the wrong length")
        self.cfg, self.p = cfg, cfg.abi()
        check(self.lib.fmcw_set_taps(self.h, ct.byref(self.p), _ptr(wr), _ptr(wd), _ptr(c)))

    def set_chunk_frames(self, n: int) -> None:
        check(self.lib.fmcw_set_chunk_frames(self.h, int(n)))

    def set_pipeline(self, mode: int) -> None:
        """FMCW_PIPE_AUTO / _STREAMS / _ONEPASS (include/fmcw.h)."""
        check(self.lib.fmcw_set_pipeline(self.h, int(mode)))

    # ---- host-array API --------------------------------------------------------
    def process(self, iq: np.ndarray, want_cube: bool = False, want_rd: bool = False,
                probe_column: int = 0) -> dict:
        """Per-frame stages (:197-261, :265) over iq[F][C][S]."""
        cfg = self._need()
        iq, dt = _host_iq(iq)
        F = iq.shape[0]
        if iq.shape[1:3] != (cfg.pn, cfg.nts):
            raise ValueError(f"iq must be [F][{cfg.pn}][{cfg.nts}]")
        M = cfg.max_targets
        out = dict(profile=np.empty((F, cfg.nr), np.float32), tgt_count=np.empty(F, np.int32),
                   tgt_range_idx=np.empty((F, M), np.int32), tgt_range_mag=np.empty((F, M), np.float32),
                   tgt_doppler_idx=np.empty((F, M), np.int32), slow_mag=np.empty((F, cfg.pn), np.float32))
        cube = np.empty((F, cfg.pn, cfg.nr), np.complex64) if want_cube else None
        rd = np.empty((F, cfg.nr, cfg.nd), np.complex64) if want_rd else None
        probe = np.empty(cfg.nr, np.float32) if probe_column else None
        check(self.lib.fmcw_process(self.h, ct.byref(self.p), _ptr(iq), dt, F, _ptr(out["profile"]),
                                    _ptr(out["tgt_count"]), _ptr(out["tgt_range_idx"]), _ptr(out["tgt_range_mag"]),
                                    _ptr(out["tgt_doppler_idx"]), _ptr(out["slow_mag"]), _ptr(cube), _ptr(rd),
                                    int(probe_column), _ptr(probe)))
        if want_cube:
            out["cube"] = cube
        if want_rd:
            out["rd"] = rd
        if probe is not None:
            out["probe_mag"] = probe
        return out

    def range_fft(self, iq: np.ndarray):
        """Config-2 range stage: (cube [F][C][Nr] complex64, profile [F][Nr])."""
        cfg = self._need()
        iq, dt = _host_iq(iq)
        F = iq.shape[0]
        cube = np.empty((F, cfg.pn, cfg.nr), np.complex64)
        prof = np.empty((F, cfg.nr), np.float32)
        check(self.lib.fmcw_range_fft(self.h, ct.byref(self.p), _ptr(iq), dt, F, _ptr(cube), _ptr(prof)))
        return cube, prof

    def stft_sizes(self, L: int, wlen: int, noverlap: int, nfft: int = 0, n_log_bins: int = 1024):
        ns, nf, nb = ct.c_int64(), ct.c_int32(), ct.c_int32()
        check(self.lib.fmcw_stft_sizes(int(L), int(wlen), int(noverlap), int(nfft), int(n_log_bins),
                                       ct.byref(ns), ct.byref(nf), ct.byref(nb)))
        return ns.value, nf.value, nb.value

    def stft(self, x: np.ndarray, win: np.ndarray, noverlap: int, fs: float, nfft: int = 0,
             n_log_bins: int = 1024) -> dict:
        """:270-299 on the device; returns time [nseg], frequency, intensity [nseg][nbins]."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        w = np.ascontiguousarray(win, np.float32)
        nseg, nf, nb = self.stft_sizes(len(x), len(w), noverlap, nfft, n_log_bins)
        T = np.empty(nseg, np.float32)
        Fq = np.empty(nb, np.float32)
        inten = np.empty((nseg, nb), np.float32)
        check(self.lib.fmcw_stft(self.h, _ptr(x), len(x), _ptr(w), len(w), int(noverlap), int(nfft), float(fs),
                                 int(n_log_bins), _ptr(T), _ptr(Fq), _ptr(inten)))
        return dict(time=T, frequency=Fq, intensity=inten, nfft=nf)

    def stft_png(self, x: np.ndarray, win: np.ndarray, noverlap: int, fs: float, png_path: str, nfft: int = 0,
                 n_log_bins: int = 1024, width: int = 0, height: int = 0) -> dict:
        """:270-299 as ``stft`` plus spectrogram.png (:331-348) rendered on the device."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        w = np.ascontiguousarray(win, np.float32)
        nseg, nf, nb = self.stft_sizes(len(x), len(w), noverlap, nfft, n_log_bins)
        T = np.empty(nseg, np.float32)
        Fq = np.empty(nb, np.float32)
        inten = np.empty((nseg, nb), np.float32)
        nbytes = ct.c_int64()
        check(self.lib.fmcw_stft_png(self.h, _ptr(x), len(x), _ptr(w), len(w), int(noverlap), int(nfft), float(fs),
                                     int(n_log_bins), _ptr(T), _ptr(Fq), _ptr(inten), str(png_path).encode(),
                                     int(width), int(height), ct.byref(nbytes)))
        return dict(time=T, frequency=Fq, intensity=inten, nfft=nf, png_bytes=nbytes.value)

    def render_spectrogram_device(self, d_Q, nq: int, d_nseg, d_pmax, nfft: int, fs: float, t0: float, dt: float,
                                  width: int, height: int, d_img, stream=None) -> None:
        with _sided(stream) as hs:
            check(self.lib.fmcw_render_spectrogram_device(self.h, _ptr(d_Q), int(nq), _ptr(d_nseg), _ptr(d_pmax),
                                                          int(nfft), float(fs), float(t0), float(dt), int(width),
                                                          int(height), _ptr(d_img), hs))

    # ---- device API (torch tensors as HBM buffers) -------------------------------
    def process_device(self, d_iq, F: int, in_dtype: int, outs: dict, d_cube=None, d_rd=None,
                       out_dtype: int = FMCW_C64, probe_column: int = 0, stream=None) -> None:
        self._need()
        with _sided(stream) as hs:
            check(self.lib.fmcw_process_device(
                self.h, ct.byref(self.p), _ptr(d_iq), in_dtype, int(F), _ptr(outs["profile"]),
                _ptr(outs["tgt_count"]), _ptr(outs["tgt_range_idx"]), _ptr(outs["tgt_range_mag"]),
                _ptr(outs["tgt_doppler_idx"]), _ptr(outs["slow_mag"]), _ptr(d_cube), _ptr(d_rd), out_dtype,
                int(probe_column), _ptr(outs.get("probe_mag")), hs))

    def process_slow_device(self, d_iq, F: int, in_dtype: int, outs: dict, d_list, d_len, d_pmax=None, d_rd=None,
                            out_dtype: int = FMCW_C64, stream=None) -> None:
        """process_device + compact_device (+ d_pmax = 0) in one call (fmcw_process_slow_device): on
        the single-pass schedule the compaction runs in the detection kernel's last workgroup."""
        self._need()
        with _sided(stream) as hs:
            check(self.lib.fmcw_process_slow_device(
                self.h, ct.byref(self.p), _ptr(d_iq), in_dtype, int(F), _ptr(outs["profile"]),
                _ptr(outs["tgt_count"]), _ptr(outs["tgt_range_idx"]), _ptr(outs["tgt_range_mag"]),
                _ptr(outs["tgt_doppler_idx"]), _ptr(outs["slow_mag"]), _ptr(d_rd), out_dtype, _ptr(d_list),
                _ptr(d_len), _ptr(d_pmax), hs))

    def range_fft_device(self, d_iq, F: int, in_dtype: int, d_cube, d_prof, out_dtype: int = FMCW_C64,
                         stream=None) -> None:
        self._need()
        with _sided(stream) as hs:
            check(self.lib.fmcw_range_fft_device(self.h, ct.byref(self.p), _ptr(d_iq), in_dtype, int(F), _ptr(d_cube),
                                                 out_dtype, _ptr(d_prof), hs))

    def compact_device(self, d_count, F: int, d_list, d_len, stream=None) -> None:
        cfg = self._need()
        with _sided(stream) as hs:
            check(self.lib.fmcw_compact_device(self.h, _ptr(d_count), int(F), cfg.pn, _ptr(d_list), _ptr(d_len),
                                               hs))

    def stft_power_device(self, d_slow, d_list, d_len, pn: int, d_win, wlen: int, noverlap: int, nfft: int,
                          fs: float, max_seg: int, d_P, d_pmax, d_nseg, d_halo=None, n_halo: int = 0,
                          d_halo_len=None, stream=None) -> None:
        with _sided(stream) as hs:
            check(self.lib.fmcw_stft_power_device(self.h, _ptr(d_slow), _ptr(d_list), _ptr(d_len), int(pn),
                                                  _ptr(d_halo), int(n_halo), _ptr(d_halo_len), _ptr(d_win),
                                                  int(wlen), int(noverlap),
                                                  int(nfft), float(fs), int(max_seg), _ptr(d_P), _ptr(d_pmax),
                                                  _ptr(d_nseg), hs))

    def stft_db_direct_device(self, d_slow, d_list, d_len, pn: int, d_win, wlen: int, noverlap: int, nfft: int,
                              fs: float, max_seg: int, d_pmax, d_out, d_halo=None, n_halo: int = 0, d_halo_len=None,
                              stream=None) -> None:
        with _sided(stream) as hs:
            check(self.lib.fmcw_stft_db_direct_device(self.h, _ptr(d_slow), _ptr(d_list), _ptr(d_len), int(pn),
                                                      _ptr(d_halo), int(n_halo), _ptr(d_halo_len), _ptr(d_win),
                                                      int(wlen), int(noverlap), int(nfft), float(fs), int(max_seg),
                                                      _ptr(d_pmax), _ptr(d_out), hs))

    def stft_db_device(self, d_P, d_nseg, max_seg: int, nfft: int, fs: float, d_pmax, n_log_bins: int, d_out,
                       stream=None) -> None:
        with _sided(stream) as hs:
            check(self.lib.fmcw_stft_db_device(self.h, _ptr(d_P), _ptr(d_nseg), int(max_seg), int(nfft), float(fs),
                                               _ptr(d_pmax), int(n_log_bins), _ptr(d_out), hs))

    def synth_device(self, d_iq, frame0: int, F: int, dtype: int = FMCW_C64, stream=None) -> None:
        self._need()
        with _sided(stream) as hs:
            check(self.lib.fmcw_synth_device(self.h, ct.byref(self.p), int(frame0), int(F), _ptr(d_iq), dtype,
                                             hs))

    # ---- 2-D CA-CFAR over the RD map (include/fmcw.h, fmcw_cfar_params) ---------
    def cfar(self, rd: np.ndarray, q: CfarConfig | OsCfarConfig, want_mask: bool = False) -> dict:
        """Detections of rd (fmcw_cfar, or fmcw_oscfar for an OsCfarConfig): complex64 [F][nr][nd],
        or float16 [F][nr][nd][2] holding D / (nr nd).
        Host arrays, sharded over the context's devices.  Returns det_count [F], det_range_idx,
        det_doppler_idx, det_power, det_noise [F][max_det] (1-based indices, 0 where unused) and,
        once set_taps has given the geometry's scales, range_m / speed_mps of every listed
        detection (NaN where unused); `mask` [F][nr][nd] uint8 when asked for."""
        rd, dt = _host_rd(rd, "F")
        F, nr, nd = rd.shape[:3]
        K = int(q.max_det)
        out = dict(det_count=np.zeros(F, np.int32), det_range_idx=np.zeros((F, max(K, 0)), np.int32),
                   det_doppler_idx=np.zeros((F, max(K, 0)), np.int32), det_power=np.zeros((F, max(K, 0)), np.float32),
                   det_noise=np.zeros((F, max(K, 0)), np.float32))
        mask = np.zeros((F, nr, nd), np.uint8) if want_mask else None
        qa = q.abi()
        call = self.lib.fmcw_oscfar if isinstance(q, OsCfarConfig) else self.lib.fmcw_cfar
        check(call(self.h, ct.byref(qa), _ptr(rd), dt, F, nr, nd, _ptr(out["det_count"]),
                   _ptr(out["det_range_idx"]), _ptr(out["det_doppler_idx"]), _ptr(out["det_power"]),
                   _ptr(out["det_noise"]), _ptr(mask)))
        if mask is not None:
            out["mask"] = mask
        if self.cfg is not None and (self.cfg.nr, self.cfg.nd) == (nr, nd):
            used = out["det_range_idx"] > 0
            out["range_m"] = np.where(used, self.cfg.range_m(out["det_range_idx"]), np.nan)
            out["speed_mps"] = np.where(used, self.cfg.speed(out["det_doppler_idx"]), np.nan)
        return out

    def cfar_device(self, q: CfarConfig | OsCfarConfig, d_rd, rd_dtype: int, F: int, nr: int, nd: int, outs: dict,
                    d_mask=None, stream=None) -> None:
        """fmcw_cfar_device (fmcw_oscfar_device for an OsCfarConfig): d_rd [F][nr][nd] of rd_dtype on
        the device; outs holds the device
        buffers det_count [F] int32, det_range_idx / det_doppler_idx [F][max_det] int32 and
        det_power / det_noise [F][max_det] float32.  Asynchronous on `stream`."""
        qa = q.abi()
        call = self.lib.fmcw_oscfar_device if isinstance(q, OsCfarConfig) else self.lib.fmcw_cfar_device
        with _sided(stream) as hs:
            check(call(self.h, ct.byref(qa), _ptr(d_rd), int(rd_dtype), int(F), int(nr), int(nd),
                       _ptr(outs["det_count"]), _ptr(outs["det_range_idx"]), _ptr(outs["det_doppler_idx"]),
                       _ptr(outs["det_power"]), _ptr(outs["det_noise"]), _ptr(d_mask), hs))

    def process_cfar_device(self, d_iq, F: int, in_dtype: int, outs: dict, q: CfarConfig | OsCfarConfig, d_rd,
                            cfar_outs: dict, out_dtype: int = FMCW_C64, d_mask=None, d_cube=None,
                            probe_column: int = 0,
                            stream=None) -> None:
        """IQ in, detections out, on one stream with no host round trip: process_device writing the
        RD map to d_rd (out_dtype), then cfar_device over it."""
        cfg = self._need()
        if d_rd is None:
            raise ValueError("process_cfar_device needs an RD buffer")
        self.process_device(d_iq, F, in_dtype, outs, d_cube=d_cube, d_rd=d_rd, out_dtype=out_dtype,
                            probe_column=probe_column, stream=stream)
        self.cfar_device(q, d_rd, out_dtype, F, cfg.nr, cfg.nd, cfar_outs, d_mask=d_mask, stream=stream)

    # ---- 2-D OS-CFAR over the RD map (include/fmcw.h, fmcw_oscfar_params) -------
    # cfar, cfar_device and process_cfar_device dispatch on the parameters' type, and with them
    # targets, angles, process_targets_device and process_tracks_device; these names say it aloud.
    def oscfar(self, rd: np.ndarray, q: OsCfarConfig, want_mask: bool = False) -> dict:
        """fmcw_oscfar: the dict of `cfar`, det_noise holding the order statistic X_(k)."""
        if not isinstance(q, OsCfarConfig):
            raise TypeError("oscfar needs an OsCfarConfig")
        return self.cfar(rd, q, want_mask=want_mask)

    def oscfar_device(self, q: OsCfarConfig, d_rd, rd_dtype: int, F: int, nr: int, nd: int, outs: dict, d_mask=None,
                      stream=None) -> None:
        """fmcw_oscfar_device, with the buffers of `cfar_device`.  Asynchronous on `stream`."""
        if not isinstance(q, OsCfarConfig):
            raise TypeError("oscfar_device needs an OsCfarConfig")
        self.cfar_device(q, d_rd, rd_dtype, F, nr, nd, outs, d_mask=d_mask, stream=stream)

    def process_oscfar_device(self, d_iq, F: int, in_dtype: int, outs: dict, q: OsCfarConfig, d_rd, cfar_outs: dict,
                              out_dtype: int = FMCW_C64, d_mask=None, d_cube=None, probe_column: int = 0,
                              stream=None) -> None:
        """IQ in, OS-CFAR detections out, on one stream with no host round trip."""
        if not isinstance(q, OsCfarConfig):
            raise TypeError("process_oscfar_device needs an OsCfarConfig")
        self.process_cfar_device(d_iq, F, in_dtype, outs, q, d_rd, cfar_outs, out_dtype=out_dtype, d_mask=d_mask,
                                 d_cube=d_cube, probe_column=probe_column, stream=stream)

    # ---- Doppler-time / range-time signatures of the RD map (include/fmcw.h, fmcw_sig_params) ----
    def signature(self, rd: np.ndarray, q: SigConfig, center: np.ndarray | None = None) -> dict:
        """Signatures of rd: complex64 [F][nr][nd], or float16 [F][nr][nd][2] holding D / (nr nd).
        Host arrays, sharded over the context's devices.  center: None (the rows are the gate), int32
        [F] or [F][stride] whose first column is the 1-based centre row of each frame (0: no target).
        Returns doppler_time [F][nd], range_time [F][nr] (in dB with q.db), the global maxima dt_max,
        rt_max of the linear maps and, once set_taps has given the geometry, the axes speed_mps [nd]
        and range_m [nr]."""
        rd, dt = _host_rd(rd, "F")
        F, nr, nd = rd.shape[:3]
        stride = 0
        if center is not None:
            center = np.ascontiguousarray(center, np.int32)
            if center.ndim not in (1, 2) or center.shape[0] != F:
                raise ValueError("center must be int32 [F] or [F][stride]")
            stride = 1 if center.ndim == 1 else center.shape[1]
        out = dict(doppler_time=np.zeros((F, nd), np.float32), range_time=np.zeros((F, nr), np.float32))
        dmx, rmx = ct.c_float(0.0), ct.c_float(0.0)
        qa = q.abi()
        check(self.lib.fmcw_sig(self.h, ct.byref(qa), _ptr(rd), dt, F, nr, nd, _ptr(center), stride,
                                _ptr(out["doppler_time"]), _ptr(out["range_time"]), ct.byref(dmx), ct.byref(rmx)))
        out["dt_max"], out["rt_max"] = np.float32(dmx.value), np.float32(rmx.value)
        if self.cfg is not None and (self.cfg.nr, self.cfg.nd) == (nr, nd):
            out["speed_mps"] = self.cfg.speed(np.arange(1, nd + 1))
            out["range_m"] = self.cfg.range_m(np.arange(1, nr + 1))
        return out

    def signature_device(self, q: SigConfig, d_rd, rd_dtype: int, F: int, nr: int, nd: int, d_doppler_time=None,
                         d_range_time=None, d_dt_max=None, d_rt_max=None, d_center=None, center_stride: int = 1,
                         stream=None) -> None:
        """fmcw_sig_device: d_rd [F][nr][nd] of rd_dtype on the device; d_doppler_time [F][nd] and
        d_range_time [F][nr] float32 (either may be None); d_dt_max / d_rt_max one float32 each,
        zeroed by the caller; d_center int32 with center_stride entries per frame, or None for the
        fixed gate.  Asynchronous on `stream`."""
        qa = q.abi()
        with _sided(stream) as hs:
            check(self.lib.fmcw_sig_device(self.h, ct.byref(qa), _ptr(d_rd), int(rd_dtype), int(F), int(nr), int(nd),
                                           _ptr(d_center), int(center_stride), _ptr(d_doppler_time),
                                           _ptr(d_range_time), _ptr(d_dt_max), _ptr(d_rt_max), hs))

    def signature_db_device(self, d_map, n: int, d_max, floor_db: float, d_out, stream=None) -> None:
        """fmcw_sig_db_device: d_out[i] = max(10 log10(d_map[i] / *d_max), floor_db); d_out may be d_map."""
        with _sided(stream) as hs:
            check(self.lib.fmcw_sig_db_device(self.h, _ptr(d_map), int(n), _ptr(d_max), float(floor_db), _ptr(d_out),
                                              hs))

    def process_signature_device(self, d_iq, F: int, in_dtype: int, outs: dict, q: SigConfig, d_rd, sig_outs: dict,
                                 out_dtype: int = FMCW_C64, track: bool = True, d_cube=None, probe_column: int = 0,
                                 stream=None) -> None:
        """IQ in, signatures out, on one stream with no host round trip: process_device writing the
        RD map to d_rd (out_dtype), then signature_device over it.  With `track` the centre of each
        frame is its strongest target, outs["tgt_range_idx"] at stride max_targets (q.track_half bins
        either side); without, the rows are q's gate.  sig_outs holds doppler_time, range_time,
        dt_max, rt_max (device buffers, any of them may be missing or None, not both maps)."""
        cfg = self._need()
        if d_rd is None:
            raise ValueError("process_signature_device needs an RD buffer")
        self.process_device(d_iq, F, in_dtype, outs, d_cube=d_cube, d_rd=d_rd, out_dtype=out_dtype,
                            probe_column=probe_column, stream=stream)
        self.signature_device(q, d_rd, out_dtype, F, cfg.nr, cfg.nd, sig_outs.get("doppler_time"),
                              sig_outs.get("range_time"), sig_outs.get("dt_max"), sig_outs.get("rt_max"),
                              d_center=outs["tgt_range_idx"] if track else None, center_stride=cfg.max_targets,
                              stream=stream)

    # ---- targets from the CFAR detection lists (include/fmcw.h, fmcw_cluster_params) ----------
    def cluster(self, det: dict, q: ClusterConfig, nr: int, nd: int) -> dict:
        """Targets of the detection lists `det` (the dict Engine.cfar returns, or any dict with
        det_count [F], det_range_idx, det_doppler_idx, det_power [F][max_det] and, optionally,
        det_noise).  Host arrays, sharded over the context's devices.  Returns tgt_count [F]; cells,
        peak_range_idx, peak_doppler_idx, extent_r, extent_d (int32) and peak_power, peak_noise,
        power, range, doppler (float32), each [F][max_tgt] with 1-based indices and 0 where unused;
        det_label [F][max_det]; and, once set_taps has given the geometry's scales, range_m /
        speed_mps of the centroids (NaN where unused)."""
        cnt = np.ascontiguousarray(det["det_count"], np.int32)
        ridx = np.ascontiguousarray(det["det_range_idx"], np.int32)
        didx = np.ascontiguousarray(det["det_doppler_idx"], np.int32)
        pw = np.ascontiguousarray(det["det_power"], np.float32)
        noise = det.get("det_noise")
        noise = None if noise is None else np.ascontiguousarray(noise, np.float32)
        F = cnt.shape[0]
        if ridx.ndim != 2 or ridx.shape[0] != F or didx.shape != ridx.shape or pw.shape != ridx.shape or \
                (noise is not None and noise.shape != ridx.shape):
            raise ValueError("the detection lists must be [F][max_det], det_count [F]")
        K, M = ridx.shape[1], int(q.max_tgt)
        out = dict(tgt_count=np.zeros(F, np.int32))
        for k in _lib.TARGET_INT_KEYS:
            out[k] = np.zeros((F, max(M, 0)), np.int32)
        for k in _lib.TARGET_FLOAT_KEYS:
            out[k] = np.zeros((F, max(M, 0)), np.float32)
        out["det_label"] = np.zeros((F, K), np.int32)
        qa = q.abi()
        t = _lib.Targets(*[_ptr(out[k]) for k, _ in _lib.Targets._fields_])
        check(self.lib.fmcw_cluster(self.h, ct.byref(qa), F, int(nr), int(nd), K, _ptr(cnt), _ptr(ridx), _ptr(didx),
                                    _ptr(pw), _ptr(noise), ct.byref(t), _ptr(out["det_label"])))
        if self.cfg is not None and (self.cfg.nr, self.cfg.nd) == (int(nr), int(nd)):
            used = out["cells"] > 0
            out["range_m"] = np.where(used, self.cfg.range_m(out["range"]), np.nan)
            out["speed_mps"] = np.where(used, self.cfg.speed(out["doppler"]), np.nan)
        return out

    def cluster_device(self, q: ClusterConfig, F: int, nr: int, nd: int, max_det: int, det: dict, outs: dict,
                       d_det_label=None, stream=None) -> None:
        """fmcw_cluster_device: det holds the device buffers fmcw_cfar_device wrote (det_count,
        det_range_idx, det_doppler_idx, det_power and, optionally, det_noise); outs the device
        buffers tgt_count [F] int32 and any of cells, peak_range_idx, peak_doppler_idx, extent_r,
        extent_d (int32), peak_power, peak_noise, power, range, doppler (float32), [F][max_tgt]
        each (missing or None: not written); d_det_label [F][max_det] int32 or None.  q: a
        ClusterConfig, or the C struct _lib.ClusterParams itself.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        t = _lib.Targets(*[_ptr(outs.get(k)) for k, _ in _lib.Targets._fields_])
        with _sided(stream) as hs:
            check(self.lib.fmcw_cluster_device(self.h, ct.byref(qa), int(F), int(nr), int(nd), int(max_det),
                                               _ptr(det["det_count"]), _ptr(det["det_range_idx"]),
                                               _ptr(det["det_doppler_idx"]), _ptr(det["det_power"]),
                                               _ptr(det.get("det_noise")), ct.byref(t), _ptr(d_det_label), hs))

    def targets(self, rd: np.ndarray, q_cfar: CfarConfig | OsCfarConfig, q_cluster: ClusterConfig) -> dict:
        """cfar then cluster over rd (host arrays): the dict of `cluster`, with the detection lists
        of `cfar` under their own names."""
        det = self.cfar(rd, q_cfar)
        nr, nd = rd.shape[1:3]
        out = self.cluster(det, q_cluster, nr, nd)
        for k in ("det_count", "det_range_idx", "det_doppler_idx", "det_power", "det_noise"):
            out[k] = det[k]
        return out

    def process_targets_device(self, d_iq, F: int, in_dtype: int, outs: dict,
                               q_cfar: CfarConfig | OsCfarConfig, d_rd, cfar_outs: dict,
                               q_cluster: ClusterConfig, tgt_outs: dict, d_det_label=None,
                               out_dtype: int = FMCW_C64, d_mask=None, d_cube=None, probe_column: int = 0,
                               stream=None) -> None:
        """IQ in, targets out, on one stream with no host round trip: process_cfar_device (RD map to
        d_rd, detection lists to cfar_outs), then cluster_device over those lists into tgt_outs."""
        cfg = self._need()
        self.process_cfar_device(d_iq, F, in_dtype, outs, q_cfar, d_rd, cfar_outs, out_dtype=out_dtype, d_mask=d_mask,
                                 d_cube=d_cube, probe_column=probe_column, stream=stream)
        self.cluster_device(q_cluster, F, cfg.nr, cfg.nd, q_cfar.max_det, cfar_outs, tgt_outs,
                            d_det_label=d_det_label, stream=stream)

    # ---- angle of arrival from several receive channels (include/fmcw.h, fmcw_aoa_params) -----
    def aoa(self, rds, det: dict, q: AoaConfig, labels: np.ndarray | None = None) -> dict:
        """Angles at the cells of the detection lists `det` (the dict Engine.cfar returns) from the
        q.n_chan RD maps `rds`, one per receive channel, each complex64 [F][nr][nd] or float16
        [F][nr][nd][2] holding D / (nr nd), all of one dtype and shape.  labels: det_label
        [F][max_det] of Engine.cluster, needed for the per-target outputs (without it, or with
        q.max_tgt 0, only the per-cell ones are returned).  Host arrays, sharded over the context's
        devices.  Returns det_zre, det_zim, det_phase, det_sin [F][max_det] and tgt_zre, tgt_zim,
        tgt_e0, tgt_e1, tgt_phase, tgt_sin, tgt_coh (float32), tgt_cells (int32) [F][max_tgt], 0
        where unused."""
        chans = [_host_rd(rd, "F") for rd in rds]
        if len(chans) != int(q.n_chan):
            raise ValueError("aoa: rds must hold q.n_chan maps")
        dt = chans[0][1]
        if any(c[1] != dt or c[0].shape != chans[0][0].shape for c in chans):
            raise ValueError("aoa: the channels must share one dtype and shape")
        F, nr, nd = chans[0][0].shape[:3]
        cnt = np.ascontiguousarray(det["det_count"], np.int32)
        ridx = np.ascontiguousarray(det["det_range_idx"], np.int32)
        didx = np.ascontiguousarray(det["det_doppler_idx"], np.int32)
        if cnt.shape != (F,) or ridx.ndim != 2 or ridx.shape[0] != F or didx.shape != ridx.shape:
            raise ValueError("the detection lists must be [F][max_det], det_count [F]")
        K, M = ridx.shape[1], int(q.max_tgt)
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.int32)
            if labels.shape != ridx.shape:
                raise ValueError("labels must be [F][max_det]")
        out = {k: np.zeros((F, K), np.float32) for k in _lib.ANGLE_DET_KEYS}
        if labels is not None and M > 0:
            for k in _lib.ANGLE_TGT_FLOAT_KEYS:
                out[k] = np.zeros((F, M), np.float32)
            out["tgt_cells"] = np.zeros((F, M), np.int32)
        qa = q.abi()
        ptrs = (ct.c_void_p * len(chans))(*[c[0].ctypes.data for c in chans])
        t = _lib.Angles(*[_ptr(out.get(k)) for k, _ in _lib.Angles._fields_])
        check(self.lib.fmcw_aoa(self.h, ct.byref(qa), ptrs, dt, F, nr, nd, K, _ptr(cnt), _ptr(ridx), _ptr(didx),
                                _ptr(labels), ct.byref(t)))
        return out

    def aoa_device(self, q: AoaConfig, d_rds, rd_dtype: int, F: int, nr: int, nd: int, max_det: int, det: dict,
                   outs: dict, d_det_label=None, stream=None) -> None:
        """fmcw_aoa_device: d_rds the q.n_chan device RD maps [F][nr][nd] of rd_dtype (separate
        allocations or slices of one, each 16-byte aligned); det the device buffers fmcw_cfar_device
        wrote (det_count, det_range_idx, det_doppler_idx); outs any of the device buffers det_zre,
        det_zim, det_phase, det_sin [F][max_det] and tgt_zre, tgt_zim, tgt_e0, tgt_e1, tgt_phase,
        tgt_sin, tgt_coh (float32), tgt_cells (int32) [F][max_tgt] (missing or None: not written);
        d_det_label [F][max_det] int32 of fmcw_cluster_device, needed by the tgt_* outputs.  q: an
        AoaConfig, or the C struct _lib.AoaParams itself.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        ptrs = (ct.c_void_p * len(d_rds))(*[_ptr(d).value or 0 for d in d_rds])
        t = _lib.Angles(*[_ptr(outs.get(k)) for k, _ in _lib.Angles._fields_])
        with _sided(stream) as hs:
            check(self.lib.fmcw_aoa_device(self.h, ct.byref(qa), ptrs, int(rd_dtype), int(F), int(nr), int(nd),
                                           int(max_det), _ptr(det["det_count"]), _ptr(det["det_range_idx"]),
                                           _ptr(det["det_doppler_idx"]), _ptr(d_det_label), ct.byref(t), hs))

    def angles(self, rds, q_cfar: CfarConfig | OsCfarConfig, q_cluster: ClusterConfig, q_aoa: AoaConfig,
               det_chan: int = 0) -> dict:
        """cfar on channel det_chan, cluster, then aoa over all channels (host arrays): the three
        dicts merged, plus angle_deg [F][max_det] and tgt_angle_deg [F][max_tgt], degrees(arcsin(sin))
        formed on the host."""
        out = self.targets(rds[det_chan], q_cfar, q_cluster)
        out.update(self.aoa(rds, out, q_aoa, labels=out["det_label"]))
        out["angle_deg"] = np.degrees(np.arcsin(out["det_sin"].astype(np.float64)))
        if "tgt_sin" in out:
            out["tgt_angle_deg"] = np.degrees(np.arcsin(out["tgt_sin"].astype(np.float64)))
        return out

    # ---- tracks from the per-frame targets (include/fmcw.h, fmcw_track_params) ----------------
    def track_state_bytes(self, max_trk: int) -> int:
        """fmcw_track_state_bytes: the bytes of one sequence's state block."""
        n = self.lib.fmcw_track_state_bytes(int(max_trk))
        if n < 0:
            check(n)
        return n

    def track(self, tgts: dict, q: TrackConfig, nr: int, nd: int, n_seq: int = 1, state: np.ndarray | None = None) -> dict:
        """Tracks over the targets `tgts` (the dict Engine.cluster returns, or any dict with tgt_count
        [S*F] and range, doppler, peak_power [S*F][max_tgt]): n_seq = S independent sequences of F
        consecutive frames each, sequence s in the rows s*F .. s*F + F - 1.  Host arrays; the sequences
        are sharded over the context's devices.  state: None for fresh sequences, or the uint8
        [S][track_state_bytes(max_trk)] array an earlier call returned, to carry the sequences on.
        Returns trk_count [S*F]; trk_id, trk_status, trk_age, trk_misses (int32) and trk_range,
        trk_range_rate, trk_doppler, trk_power (float32), each [S*F][max_trk] and 0 for a free slot;
        tgt_track [S*F][max_tgt]; `state` after the last frame; and, once set_taps has given the
        geometry's scales, range_m, speed_mps and range_rate_mps_per_frame (NaN for free slots)."""
        cnt = np.ascontiguousarray(tgts["tgt_count"], np.int32)
        zr = np.ascontiguousarray(tgts["range"], np.float32)
        zd = np.ascontiguousarray(tgts["doppler"], np.float32)
        zp = np.ascontiguousarray(tgts["peak_power"], np.float32)
        rows, S = cnt.shape[0], int(n_seq)
        if cnt.ndim != 1 or zr.ndim != 2 or zr.shape[0] != rows or zd.shape != zr.shape or zp.shape != zr.shape:
            raise ValueError("the targets must be [S*F][max_tgt], tgt_count [S*F]")
        if S < 1 or rows % S:
            raise ValueError("n_seq must divide the number of rows")
        F, M, T = rows // S, zr.shape[1], int(q.max_trk)
        sb = self.track_state_bytes(T)
        if state is None:
            st = np.zeros((S, sb), np.uint8)
        else:
            st = np.array(state, dtype=np.uint8, order="C", copy=True)
            if st.shape != (S, sb):
                raise ValueError(f"state must be uint8 [{S}][{sb}]")
        out = dict(trk_count=np.zeros(rows, np.int32))
        for k in _lib.TRACK_INT_KEYS:
            out[k] = np.zeros((rows, T), np.int32)
        for k in _lib.TRACK_FLOAT_KEYS:
            out[k] = np.zeros((rows, T), np.float32)
        out["tgt_track"] = np.zeros((rows, M), np.int32)
        qa = q.abi()
        t = _lib.Tracks(*[_ptr(out[k]) for k, _ in _lib.Tracks._fields_])
        check(self.lib.fmcw_track(self.h, ct.byref(qa), S, F, int(nr), int(nd), M, _ptr(cnt), _ptr(zr), _ptr(zd),
                                  _ptr(zp), _ptr(st), ct.byref(t), _ptr(out["tgt_track"])))
        out["state"] = st
        if self.cfg is not None and (self.cfg.nr, self.cfg.nd) == (int(nr), int(nd)):
            used = out["trk_status"] > 0
            out["range_m"] = np.where(used, self.cfg.range_m(out["trk_range"]), np.nan)
            out["speed_mps"] = np.where(used, self.cfg.speed(out["trk_doppler"]), np.nan)
            out["range_rate_mps_per_frame"] = np.where(
                used, out["trk_range_rate"].astype(np.float64) * self.cfg.dist_per_bin, np.nan)
        return out

    def track_device(self, q: TrackConfig, S: int, F: int, nr: int, nd: int, max_tgt: int, tgts: dict, d_state,
                     outs: dict, d_tgt_track=None, stream=None) -> None:
        """fmcw_track_device: tgts holds the device buffers fmcw_cluster_device wrote (tgt_count [S*F],
        range, doppler, peak_power [S*F][max_tgt]); d_state the uint8 [S][track_state_bytes(max_trk)]
        state, read and rewritten in place (zeros: fresh sequences); outs the device buffers trk_count
        [S*F] int32 and any of trk_id, trk_status, trk_age, trk_misses (int32), trk_range,
        trk_range_rate, trk_doppler, trk_power (float32), [S*F][max_trk] each (missing or None: not
        written); d_tgt_track [S*F][max_tgt] int32 or None.  q: a TrackConfig, or the C struct
        _lib.TrackParams itself.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        t = _lib.Tracks(*[_ptr(outs.get(k)) for k, _ in _lib.Tracks._fields_])
        with _sided(stream) as hs:
            check(self.lib.fmcw_track_device(self.h, ct.byref(qa), int(S), int(F), int(nr), int(nd), int(max_tgt),
                                             _ptr(tgts["tgt_count"]), _ptr(tgts["range"]), _ptr(tgts["doppler"]),
                                             _ptr(tgts["peak_power"]), _ptr(d_state), ct.byref(t), _ptr(d_tgt_track),
                                             hs))

    def process_tracks_device(self, d_iq, F: int, in_dtype: int, outs: dict,
                              q_cfar: CfarConfig | OsCfarConfig, d_rd, cfar_outs: dict, q_cluster: ClusterConfig,
                              tgt_outs: dict, q_track: TrackConfig, d_state, trk_outs: dict,
                              d_tgt_track=None, d_det_label=None, out_dtype: int = FMCW_C64, d_mask=None, d_cube=None,
                              probe_column: int = 0, stream=None) -> None:
        """IQ in, tracks out, on one stream with no host round trip: process_targets_device (targets
        to tgt_outs, which must hold range, doppler and peak_power), then track_device over the F
        frames as one sequence, carried on from d_state."""
        cfg = self._need()
        self.process_targets_device(d_iq, F, in_dtype, outs, q_cfar, d_rd, cfar_outs, q_cluster, tgt_outs,
                                    d_det_label=d_det_label, out_dtype=out_dtype, d_mask=d_mask, d_cube=d_cube,
                                    probe_column=probe_column, stream=stream)
        self.track_device(q_track, 1, F, cfg.nr, cfg.nd, q_cluster.max_tgt, tgt_outs, d_state, trk_outs,
                          d_tgt_track=d_tgt_track, stream=stream)

    # ---- frame-to-frame clutter filter of the RD map (include/fmcw.h, fmcw_mti_params) ---------
    def mti_ring(self, rd_dtype: int = FMCW_C64) -> int:
        """fmcw_mti_ring: the frames a lane of k_mti keeps in flight for that dtype."""
        n = self.lib.fmcw_mti_ring(int(rd_dtype))
        if n < 0:
            check(n)
        return n

    def mti(self, rd: np.ndarray, q: MtiConfig, n_seq: int = 1, bg: np.ndarray | None = None,
            seen: np.ndarray | None = None, want_out: bool = True) -> dict:
        """The filtered map of rd: complex64 [S*F][nr][nd], or float16 [S*F][nr][nd][2] holding
        D / (nr nd) -- n_seq = S independent sequences of F consecutive frames each, sequence s in the
        frames s*F .. s*F + F - 1.  Host arrays; the sequences are sharded over the context's devices.
        bg (complex64 [S][nr][nd]) and seen (int32 [S]): None for fresh sequences, or what an earlier
        call returned, to carry the sequences on (both or neither; the caller's arrays are not written
        through).  Returns `out` (the shape and dtype of rd; None without want_out, which only learns
        the background), `bg` and `seen` after the last frame."""
        rd, dt = _host_rd(rd, "S*F")
        rows, nr, nd = rd.shape[:3]
        S = int(n_seq)
        if S < 1 or rows % S:
            raise ValueError("n_seq must divide the number of frames")
        if (bg is None) != (seen is None):
            raise ValueError("bg and seen must both be given or both be None")
        if bg is None:
            b, n = np.zeros((S, nr, nd), np.complex64), np.zeros(S, np.int32)
        else:
            b = np.array(bg, dtype=np.complex64, order="C", copy=True)
            n = np.array(seen, dtype=np.int32, order="C", copy=True).reshape(-1)
            if b.shape != (S, nr, nd) or n.shape != (S,):
                raise ValueError(f"bg must be complex64 [{S}][{nr}][{nd}] and seen int32 [{S}]")
        out = np.empty_like(rd) if want_out else None
        qa = q.abi()
        check(self.lib.fmcw_mti(self.h, ct.byref(qa), _ptr(rd), dt, S, rows // S, nr, nd, _ptr(b), _ptr(n), _ptr(out)))
        return dict(out=out, bg=b, seen=n)

    def mti_device(self, q: MtiConfig, d_rd, rd_dtype: int, S: int, F: int, nr: int, nd: int, d_bg, d_seen, d_out=None,
                   stream=None) -> None:
        """fmcw_mti_device: d_rd [S*F][nr][nd] of rd_dtype on the device; d_bg [S][nr][nd] complex64
        and d_seen [S] int32, read and rewritten in place (zeros: fresh sequences); d_out of the shape
        and dtype of d_rd, d_rd itself (in place), or None: only the background is learned.  q: an
        MtiConfig, or the C struct _lib.MtiParams itself.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        with _sided(stream) as hs:
            check(self.lib.fmcw_mti_device(self.h, ct.byref(qa), _ptr(d_rd), int(rd_dtype), int(S), int(F), int(nr),
                                           int(nd), _ptr(d_bg), _ptr(d_seen), _ptr(d_out), hs))

    def process_mti_device(self, d_iq, F: int, in_dtype: int, outs: dict, q: MtiConfig, d_rd, d_bg, d_seen, d_out=None,
                           out_dtype: int = FMCW_C64, d_cube=None, probe_column: int = 0, stream=None) -> None:
        """IQ in, filtered RD map out, on one stream with no host round trip: process_device writing
        the RD map to d_rd (out_dtype), then mti_device over the F frames as one sequence, carried on
        from d_bg / d_seen.  d_out None: in place in d_rd.  cfar_device, signature_device and
        cluster_device / track_device then chain on the filtered buffer as they are."""
        cfg = self._need()
        if d_rd is None:
            raise ValueError("process_mti_device needs an RD buffer")
        self.process_device(d_iq, F, in_dtype, outs, d_cube=d_cube, d_rd=d_rd, out_dtype=out_dtype,
                            probe_column=probe_column, stream=stream)
        self.mti_device(q, d_rd, out_dtype, 1, F, cfg.nr, cfg.nd, d_bg, d_seen, d_out=d_rd if d_out is None else d_out,
                        stream=stream)

    # ---- the receive channels combined into beams (include/fmcw.h, fmcw_beam_params) -----------
    @staticmethod
    def beam_weights(n_chan: int, sin_theta, spacing: float = 0.5, cal=None, taper=None,
                     normalize: bool = True) -> np.ndarray:
        """fmcw_beam_steer: complex64 [n_beam][n_chan], the weights of one beam per entry of
        sin_theta for a uniform line of n_chan elements `spacing` wavelengths apart, in the sign
        convention of AoaConfig.spacing.  cal: the per-channel complex calibration weights a caller
        gives aoa; taper: a real weight per channel; normalize: divide by the taper's sum (n_chan
        without one).  Feed the result to BeamConfig."""
        st = np.ascontiguousarray(np.atleast_1d(sin_theta), np.float32)
        c = None if cal is None else np.ascontiguousarray(
            np.asarray(cal, np.complex64).reshape(-1)).view(np.float32)
        t = None if taper is None else np.ascontiguousarray(np.asarray(taper, np.float32).reshape(-1))
        if (c is not None and c.size != 2 * int(n_chan)) or (t is not None and t.size != int(n_chan)):
            raise ValueError("beam_weights: cal and taper need one value per channel")
        q = _lib.BeamParams()
        check(_lib.load().fmcw_beam_steer(int(n_chan), int(st.size), float(spacing), _ptr(st), _ptr(c), _ptr(t),
                                          1 if normalize else 0, ct.byref(q)))
        w = np.array(q.w[:], np.float32).reshape(8, 8, 2)[:st.size, :int(n_chan)]
        return np.ascontiguousarray(w).view(np.complex64).reshape(st.size, int(n_chan))

    def beam(self, rds, q: BeamConfig) -> list:
        """The q.n_beam maps combined from the q.n_chan RD maps `rds`, one per receive channel, each
        complex64 [F][nr][nd] or float16 [F][nr][nd][2] holding D / (nr nd), all of one dtype and
        shape.  Host arrays, frames sharded over the context's devices.  Returns a list of q.n_beam
        new arrays of the inputs' shape and dtype (with q.nci: one map, the amplitude sqrt(sum of the
        weighted channels' powers) in the real part)."""
        chans = [_host_rd(rd, "F") for rd in rds]
        if len(chans) != int(q.n_chan):
            raise ValueError("beam: rds must hold q.n_chan maps")
        dt = chans[0][1]
        if any(c[1] != dt or c[0].shape != chans[0][0].shape for c in chans):
            raise ValueError("beam: the channels must share one dtype and shape")
        F, nr, nd = chans[0][0].shape[:3]
        outs = [np.empty_like(chans[0][0]) for _ in range(int(q.n_beam))]
        qa = q.abi()
        ptrs = (ct.c_void_p * len(chans))(*[c[0].ctypes.data for c in chans])
        optrs = (ct.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        check(self.lib.fmcw_beam(self.h, ct.byref(qa), ptrs, dt, F, nr, nd, optrs))
        return outs

    def beam_device(self, q: BeamConfig, d_rds, rd_dtype: int, F: int, nr: int, nd: int, d_outs, stream=None) -> None:
        """fmcw_beam_device: d_rds the q.n_chan device RD maps [F][nr][nd] of rd_dtype and d_outs the
        q.n_beam device maps of the same shape and dtype to write (separate allocations or slices of
        one, each 16-byte aligned; an output may be one of the inputs itself: in place).  q: a
        BeamConfig, or the C struct _lib.BeamParams itself.  cfar_device, signature_device,
        mti_device and aoa_device chain on an output as on any RD buffer.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        ptrs = (ct.c_void_p * max(len(d_rds), 1))(*[_ptr(d).value or 0 for d in d_rds])
        optrs = (ct.c_void_p * max(len(d_outs), 1))(*[_ptr(d).value or 0 for d in d_outs])
        with _sided(stream) as hs:
            check(self.lib.fmcw_beam_device(self.h, ct.byref(qa), ptrs, int(rd_dtype), int(F), int(nr), int(nd), optrs,
                                            hs))

    # ---- range-angle maps: covariance, Bartlett and Capon spectra (include/fmcw.h, fmcw_ra_params) ----
    @staticmethod
    def ra_weights(n_chan: int, sin_theta=None, spacing: float = 0.5, cal=None, taper=None, normalize: bool = True,
                   n_ang: int = 65) -> np.ndarray:
        """fmcw_ra_steer: complex64 [n_ang][n_chan], the weights of one look direction per entry of
        sin_theta (default: n_ang points uniform in sin(theta) over [-1, 1]) for a uniform line of
        n_chan elements `spacing` wavelengths apart; the arguments are those of beam_weights, for up
        to 256 directions.  Feed the result to range_angle."""
        if sin_theta is None:
            sin_theta = np.linspace(-1.0, 1.0, int(n_ang)) if int(n_ang) > 1 else np.zeros(1)
        st = np.ascontiguousarray(np.atleast_1d(sin_theta), np.float32)
        c = None if cal is None else np.ascontiguousarray(
            np.asarray(cal, np.complex64).reshape(-1)).view(np.float32)
        t = None if taper is None else np.ascontiguousarray(np.asarray(taper, np.float32).reshape(-1))
        if (c is not None and c.size != 2 * int(n_chan)) or (t is not None and t.size != int(n_chan)):
            raise ValueError("ra_weights: cal and taper need one value per channel")
        w = np.zeros((max(st.size, 1), max(int(n_chan), 1), 2), np.float32)
        check(_lib.load().fmcw_ra_steer(int(n_chan), int(st.size), float(spacing), _ptr(st), _ptr(c), _ptr(t),
                                        1 if normalize else 0, _ptr(w)))
        return w.view(np.complex64).reshape(st.size, int(n_chan))

    def range_angle(self, rds, q: RaConfig, w=None, want_cov: bool = True, want_ra: bool = True) -> tuple:
        """(ra, cov, ra_max) from the q.n_chan RD maps `rds`, one per receive channel, each complex64
        [F][nr][nd] or float16 [F][nr][nd][2] holding D / (nr nd), all of one dtype and shape.  w:
        complex [q.n_ang][q.n_chan] of ra_weights (needed with want_ra).  Host arrays, frames sharded
        over the context's devices.  ra float32 [F][nr][q.n_ang] (None without want_ra), cov float32
        [F][nr][T][2], T = n_chan (n_chan + 1) / 2 (None without want_cov), ra_max the largest value
        of ra as float (0 without want_ra)."""
        chans = [_host_rd(rd, "F") for rd in rds]
        A, K = int(q.n_chan), int(q.n_ang)
        if len(chans) != A:
            raise ValueError("ra: rds must hold q.n_chan maps")
        dt = chans[0][1]
        if any(c[1] != dt or c[0].shape != chans[0][0].shape for c in chans):
            raise ValueError("ra: the channels must share one dtype and shape")
        F, nr, nd = chans[0][0].shape[:3]
        wf = None
        if want_ra:
            if w is None:
                raise ValueError("ra: the spectra need a weight table (Engine.ra_weights)")
            wf = np.ascontiguousarray(np.asarray(w).astype(np.complex64))
            if wf.shape != (K, A):
                raise ValueError("ra: w must be [q.n_ang][q.n_chan] complex")
        cov = np.empty((F, nr, A * (A + 1) // 2, 2), np.float32) if want_cov else None
        ra = np.empty((F, nr, K), np.float32) if want_ra else None
        mx = ct.c_float(0.0)
        qa = q.abi()
        ptrs = (ct.c_void_p * max(len(chans), 1))(*[c[0].ctypes.data for c in chans])
        check(self.lib.fmcw_ra(self.h, ct.byref(qa), ptrs, dt, F, nr, nd, _ptr(wf), _ptr(cov), _ptr(ra), ct.byref(mx)))
        return ra, cov, float(mx.value)

    def cov_device(self, q: RaConfig, d_rds, rd_dtype: int, F: int, nr: int, nd: int, d_cov, stream=None) -> None:
        """fmcw_cov_device: d_rds the q.n_chan device RD maps [F][nr][nd] of rd_dtype (separate
        allocations or slices of one, each 16-byte aligned); d_cov float32 [F][nr][T][2].  q: a
        RaConfig, or the C struct _lib.RaParams itself.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        ptrs = (ct.c_void_p * max(len(d_rds), 1))(*[_ptr(d).value or 0 for d in d_rds])
        with _sided(stream) as hs:
            check(self.lib.fmcw_cov_device(self.h, ct.byref(qa), ptrs, int(rd_dtype), int(F), int(nr), int(nd),
                                           _ptr(d_cov), hs))

    def range_angle_device(self, q: RaConfig, d_cov, F: int, nr: int, d_w, d_ra, d_ra_max=None, stream=None) -> None:
        """fmcw_ra_device: d_cov float32 [F][nr][T][2] (of cov_device, or the caller's own), d_w
        float32 [q.n_ang][q.n_chan][2], d_ra float32 [F][nr][q.n_ang]; d_ra_max one float32 zeroed by
        the caller, or None.  signature_db_device turns d_ra into dB.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        with _sided(stream) as hs:
            check(self.lib.fmcw_ra_device(self.h, ct.byref(qa), _ptr(d_cov), int(F), int(nr), _ptr(d_w), _ptr(d_ra),
                                          _ptr(d_ra_max), hs))

    # ---- MUSIC: eigen-decomposition of the rows' covariance, source count, pseudo-spectrum (fmcw_music_params) ----
    def music_device(self, q: MusicConfig, d_cov, F: int, nr: int, d_w=None, d_eval=None, d_evec=None, d_nsrc=None,
                     d_music=None, d_music_max=None, stream=None) -> None:
        """fmcw_music_device: d_cov float32 [F][nr][T][2] (of cov_device, or the caller's own); d_w
        float32 [q.n_ang][q.n_chan][2], needed with d_music; d_eval float32 [F][nr][A], d_evec float32
        [F][nr][A][A][2], d_nsrc int32 [F][nr], d_music float32 [F][nr][q.n_ang], any of them None but
        not all; d_music_max one float32 zeroed by the caller, or None.  q: a MusicConfig, or the C
        struct _lib.MusicParams itself.  Asynchronous on `stream`."""
        qa = q.abi() if hasattr(q, "abi") else q
        with _sided(stream) as hs:
            check(self.lib.fmcw_music_device(self.h, ct.byref(qa), _ptr(d_cov), int(F), int(nr), _ptr(d_w), _ptr(d_eval),
                                             _ptr(d_evec), _ptr(d_nsrc), _ptr(d_music), _ptr(d_music_max), hs))

    def music_host(self, cov, q: MusicConfig, w=None, want=("eval", "evec", "nsrc", "music")) -> dict:
        """fmcw_music on a host covariance float32 [F][nr][T][2]: dict(eval, evec, nsrc, music,
        music_max) with None for what `want` leaves out.  Frames sharded over the context's devices."""
        cov = np.ascontiguousarray(cov, np.float32)
        A, K = int(q.n_chan), int(q.n_ang)
        if cov.ndim != 4 or cov.shape[2:] != (A * (A + 1) // 2, 2):
            raise ValueError("music: cov must be [F][nr][n_chan (n_chan + 1) / 2][2]")
        F, nr = cov.shape[:2]
        wf = None
        if "music" in want:
            if w is None:
                raise ValueError("music: the spectrum needs a weight table (Engine.ra_weights)")
            wf = np.ascontiguousarray(np.asarray(w).astype(np.complex64))
            if wf.shape != (K, A):
                raise ValueError("music: w must be [q.n_ang][q.n_chan] complex")
        out = {"eval": np.empty((F, nr, A), np.float32) if "eval" in want else None,
               "evec": np.empty((F, nr, A, A, 2), np.float32) if "evec" in want else None,
               "nsrc": np.empty((F, nr), np.int32) if "nsrc" in want else None,
               "music": np.empty((F, nr, K), np.float32) if "music" in want else None}
        mx = ct.c_float(0.0)
        qa = q.abi()
        check(self.lib.fmcw_music(self.h, ct.byref(qa), _ptr(cov), F, nr, _ptr(wf), _ptr(out["eval"]), _ptr(out["evec"]),
                                  _ptr(out["nsrc"]), _ptr(out["music"]), ct.byref(mx)))
        out["music_max"] = float(mx.value)
        return out

    def music(self, rds, q: MusicConfig, ra_q: RaConfig, w) -> dict:
        """The q.n_chan RD maps `rds` (host arrays, as range_angle takes them) -> cov_device with ra_q
        (its dc_half and gate), then music_device with q, on the context's first device: dict(cov, eval,
        evec, nsrc, music, music_max) of numpy arrays.  w: complex [q.n_ang][q.n_chan] of ra_weights."""
        import torch
        chans = [_host_rd(rd, "F") for rd in rds]
        A, K = int(q.n_chan), int(q.n_ang)
        if len(chans) != A or int(ra_q.n_chan) != A:
            raise ValueError("music: rds must hold q.n_chan maps and ra_q.n_chan must equal q.n_chan")
        dt = chans[0][1]
        if any(c[1] != dt or c[0].shape != chans[0][0].shape for c in chans):
            raise ValueError("music: the channels must share one dtype and shape")
        F, nr, nd = chans[0][0].shape[:3]
        wf = np.ascontiguousarray(np.asarray(w).astype(np.complex64))
        if wf.shape != (K, A):
            raise ValueError("music: w must be [q.n_ang][q.n_chan] complex")
        dev = torch.device("cuda", self.device)
        d_rds = [torch.from_numpy(np.array(c[0])).to(dev) for c in chans]      # a copy: the caller's array may be read-only
        d_w = torch.from_numpy(wf.view(np.float32).reshape(K, A, 2)).to(dev)
        d_cov = torch.empty((F, nr, A * (A + 1) // 2, 2), dtype=torch.float32, device=dev)
        d_eval = torch.empty((F, nr, A), dtype=torch.float32, device=dev)
        d_evec = torch.empty((F, nr, A, A, 2), dtype=torch.float32, device=dev)
        d_nsrc = torch.empty((F, nr), dtype=torch.int32, device=dev)
        d_music = torch.empty((F, nr, K), dtype=torch.float32, device=dev)
        d_mx = torch.zeros(1, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        self.cov_device(ra_q, d_rds, dt, F, nr, nd, d_cov)
        self.music_device(q, d_cov, F, nr, d_w, d_eval, d_evec, d_nsrc, d_music, d_mx)
        self.synchronize()
        return {"cov": d_cov.cpu().numpy(), "eval": d_eval.cpu().numpy(), "evec": d_evec.cpu().numpy(),
                "nsrc": d_nsrc.cpu().numpy(), "music": d_music.cpu().numpy(), "music_max": float(d_mx.cpu()[0])}

    # ---- directions of arrival: the peaks of the angular spectra per range row (fmcw_doa_params) ----
    def doa_device(self, q: DoaConfig, d_spec, F: int, nr: int, d_sin, d_count=None, d_idx=None, d_pow=None, d_sin_out=None,
                   d_base=None, stream=None) -> None:
        """fmcw_doa_device: d_spec float32 [F][nr][q.n_ang] (of ra_device or music_device, or the
        caller's own); d_sin float32 [q.n_ang], the grid the weight table was formed on; d_count int32
        [F][nr], d_idx int32 [F][nr][q.max_pk], d_pow, d_sin_out, d_base float32 [F][nr][q.max_pk], any
        of them None but not all.  q: a DoaConfig, or the C struct _lib.DoaParams itself.
        Asynchronous on `stream`."""
        qa = q.to_c() if hasattr(q, "to_c") else q
        with _sided(stream) as hs:
            check(self.lib.fmcw_doa_device(self.h, ct.byref(qa), _ptr(d_spec), int(F), int(nr), _ptr(d_sin), _ptr(d_count),
                                           _ptr(d_idx), _ptr(d_pow), _ptr(d_sin_out), _ptr(d_base), hs))

    def doa(self, spec, q: DoaConfig, sin_theta, want=("count", "idx", "pow", "sin", "base")) -> dict:
        """fmcw_doa on a host spectrum float32 [F][nr][q.n_ang] and the grid sin_theta [q.n_ang]:
        dict(count, idx, pow, sin, base) with None for what `want` leaves out.  Frames sharded over
        the context's devices."""
        spec = np.ascontiguousarray(spec, np.float32)
        u = np.ascontiguousarray(sin_theta, np.float32)
        K, P = int(q.n_ang), int(q.max_pk)
        if spec.ndim != 3 or spec.shape[2] != K:
            raise ValueError("doa: spec must be [F][nr][n_ang]")
        if u.shape != (K,):
            raise ValueError("doa: sin_theta must be [n_ang]")
        F, nr = spec.shape[:2]
        out = {"count": np.empty((F, nr), np.int32) if "count" in want else None,
               "idx": np.empty((F, nr, P), np.int32) if "idx" in want else None}
        for k in ("pow", "sin", "base"):
            out[k] = np.empty((F, nr, P), np.float32) if k in want else None
        qa = q.to_c() if hasattr(q, "to_c") else q
        check(self.lib.fmcw_doa(self.h, ct.byref(qa), _ptr(spec), F, nr, _ptr(u), _ptr(out["count"]), _ptr(out["idx"]),
                                _ptr(out["pow"]), _ptr(out["sin"]), _ptr(out["base"])))
        return out

    @staticmethod
    def doa_positions(out: dict, range_m) -> tuple:
        """(x, y) float64 [F][nr][max_pk] of the written peaks of a doa result (its idx and sin) with
        the rows' ranges range_m [nr] in metres: x = R sin, y = R sqrt(1 - sin^2) (NaN where |sin| > 1);
        NaN in unused slots.  Host-side numpy, not held bit-exact."""
        sn = np.asarray(out["sin"], np.float64)
        R = np.asarray(range_m, np.float64).reshape(1, -1, 1)
        used = np.asarray(out["idx"]) >= 0
        with np.errstate(invalid="ignore"):
            x = np.where(used, R * sn, np.nan)
            y = np.where(used, R * np.sqrt(1.0 - sn * sn), np.nan)
        return x, y

    # ---- timing -----------------------------------------------------------------
    def timing(self, level: int) -> None:
        """0 off, 1 per range+Doppler chunk + STFT launches, 2 per kernel launch, 3 the dominant
        kernel's launches only (k_rdx / range-only K1)."""
        check(self.lib.fmcw_timing_enable(self.h, int(level)))

    def timing_reset(self) -> None:
        check(self.lib.fmcw_timing_reset(self.h))

    def timing_read(self) -> dict:
        out = {}
        for i, name in list(enumerate(STAGES)) + [(MUSIC_STAGE, "music"), (DOA_STAGE, "doa")]:
            ms, n = ct.c_double(), ct.c_int64()
            check(self.lib.fmcw_timing_read_ext(self.h, i, ct.byref(ms), ct.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def synchronize(self) -> None:
        check(self.lib.fmcw_synchronize(self.h))

    def rdx_clock(self) -> tuple:
        """(MHz, us) of the last k_rdx launch: its effective shader clock and stamped span."""
        mhz, us = ct.c_double(), ct.c_double()
        check(self.lib.fmcw_rdx_clock(self.h, ct.byref(mhz), ct.byref(us)))
        return mhz.value, us.value

    def copy_device(self, d_src, d_dst, nbytes: int, stream=None) -> None:
        """16-byte nontemporal device copy (the bench's HBM copy ceiling)."""
        with _sided(stream) as hs:
            check(self.lib.fmcw_copy_device(self.h, _ptr(d_src), _ptr(d_dst), int(nbytes), hs))

    def _need(self) -> FmcwConfig:
        if self.cfg is None:
            raise FmcwError(_lib.FMCW_E_STATE, "set_taps() first")
        return self.cfg


def _stream(stream) -> ct.c_void_p:
    """The hipStream_t of a call: None = the context's own stream (include/fmcw.h: NULL), an int
    = a raw handle, a torch.cuda.Stream = its handle (see _sided for torch's default stream)."""
    if stream is None:
        return ct.c_void_p(0)
    if isinstance(stream, int):
        return ct.c_void_p(stream)
    return ct.c_void_p(int(stream.cuda_stream))   # torch.cuda.Stream


_SIDE = {}


@contextlib.contextmanager
def _sided(stream):
    """The stream handle for a device call on `stream`.  torch's default stream has handle 0,
    which the C-ABI reads as the context's own (non-blocking) stream -- one that does not wait
    for the torch work queued before the call (a flip, a mul_, an RCCL collective) nor the torch
    work after it for the call.  So a call on torch's default stream runs on a side stream that
    waits for it first and that it waits for afterwards: ordered like any torch kernel."""
    if stream is None or isinstance(stream, int) or int(stream.cuda_stream) != 0:
        yield _stream(stream)
        return
    import torch
    side = _SIDE.get(stream.device)
    if side is None:
        side = _SIDE[stream.device] = torch.cuda.Stream(device=stream.device)
    side.wait_stream(stream)
    try:
        yield ct.c_void_p(int(side.cuda_stream))
    finally:
        stream.wait_stream(side)


def device_count() -> int:
    lib = _lib.load()
    n = ct.c_int32()
    st = lib.fmcw_device_count(ct.byref(n))
    return n.value if st == 0 else 0


def default_devices() -> list:
    """include/fmcw.h fmcw_default_devices: FMCW_DEVICES ("0,1,...") or every visible device."""
    lib = _lib.load()
    ids = (ct.c_int32 * 64)()
    n = ct.c_int32()
    check(lib.fmcw_default_devices(64, ids, ct.byref(n)))
    return list(ids[: n.value])
