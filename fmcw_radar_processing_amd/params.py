"""Host-side parameters of the FMCW path.

Mirrors what radar_processing.m computes on the MATLAB host before the loop:
device params from the sXML struct (:94-115), algorithm constants (:117-129),
derived quantities (:131-154), the calibration vector (:166-174) and the
window taps (:138-139, :276).  Nothing here touches the GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import windows
from ._lib import (FMCW_BEAM_NCI, FMCW_CFAR_LOCAL_MAX, FMCW_DOA_EDGES, FMCW_DOA_INV, FMCW_DOA_WRAP, FMCW_MTI_FREEZE, FMCW_MTI_RAMP,
                   FMCW_MUSIC_FB, FMCW_RA_CAPON, FMCW_SIG_DB, AoaParams, BeamParams, CfarParams, ClusterParams, DoaParams, MtiParams,
                   MusicParams, OsCfarParams, Params, RaParams, SigParams, TrackParams)

C0 = 3e8  # radar_processing.m:67

PARITY = "parity"          # literal constants and quirks of the reference
THROUGHPUT = "throughput"  # configs 2-5 of BASELINE.json


@dataclass
class FmcwConfig:
    prt: float
    bw: float
    fc: float
    nts: int
    pn: int
    nr: int
    nd: int
    n_rx: int = 1
    n_tx: int = 1
    fs_adc: float = 0.0
    mode: str = PARITY
    frame_time: float = 0.15                 # :91
    range_thr: float = 200.0                 # :123
    doppler_thr: float = 50.0                # :124
    min_d: float = 0.9                       # :126
    max_d: float = 25.0                      # :127
    max_targets: int = 1                     # :129
    window_length: int = 20                  # :178
    overlap: int = 19                        # :179
    batch_size: int = 100                    # :189 ('yes' branch)
    extra: dict = field(default_factory=dict)

    # ---- derived (:131-154) ----
    @property
    def if_scale(self) -> float:
        return 16 * 3.3 * self.nr / self.nts           # :121 / :136 (uses the literal Nr)

    @property
    def lam(self) -> float:
        return C0 / self.fc                            # :133

    @property
    def hz_to_mps(self) -> float:
        return self.lam / 2                            # :135

    @property
    def r_max(self) -> float:
        return self.nts * C0 / (2 * self.bw)           # :142

    @property
    def dist_per_bin(self) -> float:
        return self.r_max / self.nr                    # :147

    @property
    def array_bin_range(self) -> np.ndarray:
        return np.arange(self.nr) * self.dist_per_bin  # :149

    @property
    def fd_max(self) -> float:
        return 1 / (2 * self.prt)                      # :152

    @property
    def fd_per_bin(self) -> float:
        return self.fd_max / self.nd                   # :153

    @property
    def array_bin_fd(self) -> np.ndarray:             # :154
        return (np.arange(1, self.nd + 1) - self.nd / 2 - 1) * -self.fd_per_bin * self.hz_to_mps

    @property
    def doppler_fallback_idx(self) -> int:
        # :234 hard-codes 9 (the zero-Doppler bin only when Nd = 16)
        return 9 if self.mode == PARITY else self.nd // 2 + 1

    def speed(self, doppler_idx) -> np.ndarray:
        """:250 (idx - Nd/2 - 1) * -fD_per_bin * Hz_to_mps_constant."""
        return (np.asarray(doppler_idx, dtype=np.float64) - self.nd / 2 - 1) * -self.fd_per_bin * self.hz_to_mps

    def range_m(self, range_idx) -> np.ndarray:
        """:248 (idx - 1) * dist_per_bin."""
        return (np.asarray(range_idx, dtype=np.float64) - 1) * self.dist_per_bin

    def abi(self) -> Params:
        return Params(self.nts, self.pn, self.nr, self.nd, self.max_targets, self.doppler_fallback_idx,
                      self.if_scale, self.range_thr, self.doppler_thr, self.min_d, self.max_d,
                      self.dist_per_bin)

    # ---- window taps (:138-139, :276) ----
    def range_window(self) -> np.ndarray:
        return 2 * windows.blackman(self.nts)

    def doppler_window(self) -> np.ndarray:
        return 2 * windows.chebwin(self.pn, 100.0)

    def stft_window(self) -> np.ndarray:
        if self.mode == PARITY:
            return windows.kaiser(self.window_length, 3.0)   # :276 kaiser(window_length, 3)
        return windows.hann(self.window_length)              # config 4: Hann(20)


@dataclass
class CfarConfig:
    """fmcw_cfar_params (include/fmcw.h): 2-D cell-averaging CFAR over the RD map.  Half-widths in
    cells; the gate r_lo..r_hi is 1-based and inclusive, (0, 0) = every row; alpha is the linear
    power ratio of the test P > alpha * S / N."""
    guard_r: int = 1
    guard_d: int = 1
    train_r: int = 2
    train_d: int = 2
    alpha: float = 1.0
    r_lo: int = 0
    r_hi: int = 0
    max_det: int = 64
    local_max: bool = False

    @property
    def n_train_full(self) -> int:
        wr, wd = self.guard_r + self.train_r, self.guard_d + self.train_d
        return (2 * wr + 1) * (2 * wd + 1) - (2 * self.guard_r + 1) * (2 * self.guard_d + 1)

    def abi(self) -> CfarParams:
        return CfarParams(self.guard_r, self.guard_d, self.train_r, self.train_d, self.r_lo, self.r_hi, self.max_det,
                          FMCW_CFAR_LOCAL_MAX if self.local_max else 0, self.alpha)

    @staticmethod
    def alpha_for(n_train: int, pfa: float) -> float:
        """fmcw_cfar_alpha: N (pfa^(-1/N) - 1), as the float32 the C-ABI carries."""
        import ctypes as ct

        from . import _lib
        a = ct.c_float()
        _lib.check(_lib.load().fmcw_cfar_alpha(int(n_train), float(pfa), ct.byref(a)))
        return float(a.value)

    @classmethod
    def for_config(cls, cfg: "FmcwConfig", pfa: float = 1e-3, guard=(1, 1), train=(2, 2), max_det: int = 64,
                   local_max: bool = False) -> "CfarConfig":
        """The detector for cfg's RD map: the gate is the peak rule's (:211, f_search_peak), the
        1-based bins i in 2..nr-1 with (i - 1) * dist_per_bin in [min_d, max_d]; alpha is the
        cell-averaging value for pfa with the full window's training-cell count."""
        q = cls(guard_r=int(guard[0]), guard_d=int(guard[1]), train_r=int(train[0]), train_d=int(train[1]),
                max_det=int(max_det), local_max=bool(local_max))
        sel = gate_bins(cfg)
        if len(sel) == 0:
            raise ValueError("no range bin lies in [min_d, max_d]")
        q.r_lo, q.r_hi = int(sel[0]) + 1, int(sel[-1]) + 1
        q.alpha = cls.alpha_for(q.n_train_full, pfa)
        return q


@dataclass
class OsCfarConfig:
    """fmcw_oscfar_params (include/fmcw.h): 2-D ordered-statistic CFAR over the RD map.  CfarConfig's
    window, gate and list fields; `rank` in 1..n_train_full picks the order statistic X_(k) of the
    training powers (scaled to the clipped window near the range edges); alpha is the linear power
    ratio of the test P > alpha * X_(k)."""
    guard_r: int = 1
    guard_d: int = 1
    train_r: int = 2
    train_d: int = 2
    alpha: float = 1.0
    r_lo: int = 0
    r_hi: int = 0
    max_det: int = 64
    local_max: bool = False
    rank: int = 1

    @property
    def n_train_full(self) -> int:
        wr, wd = self.guard_r + self.train_r, self.guard_d + self.train_d
        return (2 * wr + 1) * (2 * wd + 1) - (2 * self.guard_r + 1) * (2 * self.guard_d + 1)

    def abi(self) -> OsCfarParams:
        win = CfarParams(self.guard_r, self.guard_d, self.train_r, self.train_d, self.r_lo, self.r_hi, self.max_det,
                         FMCW_CFAR_LOCAL_MAX if self.local_max else 0, self.alpha)
        return OsCfarParams(win, self.rank)

    @staticmethod
    def alpha_for(n_train: int, rank: int, pfa: float) -> float:
        """fmcw_oscfar_alpha: the alpha with prod_{i<rank} (N - i) / (N - i + alpha) = pfa, as the
        float32 the C-ABI carries."""
        import ctypes as ct

        from . import _lib
        a = ct.c_float()
        _lib.check(_lib.load().fmcw_oscfar_alpha(int(n_train), int(rank), float(pfa), ct.byref(a)))
        return float(a.value)

    @classmethod
    def for_config(cls, cfg: "FmcwConfig", pfa: float = 1e-3, guard=(1, 1), train=(2, 2), rank_share: float = 0.75,
                   max_det: int = 64, local_max: bool = False) -> "OsCfarConfig":
        """The detector for cfg's RD map: CfarConfig.for_config's gate (the peak rule's),
        rank = max(1, floor(rank_share * n_train_full)) and the alpha of that rank for pfa."""
        q = cls(guard_r=int(guard[0]), guard_d=int(guard[1]), train_r=int(train[0]), train_d=int(train[1]),
                max_det=int(max_det), local_max=bool(local_max))
        sel = gate_bins(cfg)
        if len(sel) == 0:
            raise ValueError("no range bin lies in [min_d, max_d]")
        q.r_lo, q.r_hi = int(sel[0]) + 1, int(sel[-1]) + 1
        q.rank = max(1, int(np.floor(rank_share * q.n_train_full)))
        q.alpha = cls.alpha_for(q.n_train_full, q.rank, pfa)
        return q


@dataclass
class SigConfig:
    """fmcw_sig_params (include/fmcw.h): Doppler-time and range-time signatures of the RD map.  The
    gate r_lo..r_hi is 1-based and inclusive, (0, 0) = every row; track_half is used only with a
    centre array (rows centre - h .. centre + h, clipped to the gate); dc_half leaves the Doppler bins
    |d - nd/2| <= dc_half out of the range-time map (-1: none); db (host call only) returns both maps
    in dB relative to their global maximum, clamped at floor_db."""
    r_lo: int = 0
    r_hi: int = 0
    track_half: int = 0
    dc_half: int = -1
    db: bool = False
    floor_db: float = -80.0

    def abi(self) -> SigParams:
        return SigParams(self.r_lo, self.r_hi, self.track_half, self.dc_half, FMCW_SIG_DB if self.db else 0,
                         self.floor_db)

    def validate(self, nr: int, nd: int) -> None:
        """The rules of fmcw_sig_check; ValueError naming the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("sig: nr must be a power of two in [16, 2048]")
        if nd < 4 or nd > 1024 or nd & (nd - 1):
            raise ValueError("sig: nd must be a power of two in [4, 1024]")
        if self.r_lo > self.r_hi:
            raise ValueError("sig: r_lo > r_hi")
        if (self.r_lo, self.r_hi) != (0, 0) and (self.r_lo < 1 or self.r_hi > nr):
            raise ValueError("sig: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)")
        if not 0 <= self.track_half <= 64:
            raise ValueError("sig: track_half must be in [0, 64]")
        if self.dc_half < -1:
            raise ValueError("sig: dc_half must be >= -1")
        if 2 * self.dc_half + 1 >= nd:
            raise ValueError("sig: 2 dc_half + 1 must be < nd")
        if not (self.floor_db < 0 and np.isfinite(self.floor_db)):
            raise ValueError("sig: floor_db must be finite and < 0")

    @classmethod
    def for_config(cls, cfg: "FmcwConfig", track_half: int = 2, dc_half: int = 0, db: bool = False,
                   floor_db: float = -80.0) -> "SigConfig":
        """The signatures over the peak rule's gate (CfarConfig.for_config), following the strongest
        target with track_half bins either side when a centre array is given."""
        g = CfarConfig.for_config(cfg)
        return cls(r_lo=g.r_lo, r_hi=g.r_hi, track_half=int(track_half), dc_half=int(dc_half), db=bool(db),
                   floor_db=float(floor_db))


@dataclass
class ClusterConfig:
    """fmcw_cluster_params (include/fmcw.h): groups the CFAR detection lists into targets.  Cells
    within link_r range bins and link_d (circular) Doppler bins of each other are linked, (1, 1) being
    8-connectivity; clusters of fewer than min_cells cells are dropped; the max_tgt targets of the
    largest peak power are written per frame."""
    link_r: int = 1
    link_d: int = 1
    min_cells: int = 1
    max_tgt: int = 16

    def abi(self) -> ClusterParams:
        return ClusterParams(self.link_r, self.link_d, self.min_cells, self.max_tgt, 0)

    def validate(self, nr: int, nd: int, max_det: int) -> None:
        """The rules of fmcw_cluster_check; ValueError naming the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("cluster: nr must be a power of two in [16, 2048]")
        if nd < 4 or nd > 1024 or nd & (nd - 1):
            raise ValueError("cluster: nd must be a power of two in [4, 1024]")
        if not (0 <= self.link_r <= 8 and 0 <= self.link_d <= 8):
            raise ValueError("cluster: link_r and link_d must be in [0, 8]")
        if 2 * self.link_d + 1 > nd:
            raise ValueError("cluster: the Doppler link 2 link_d + 1 exceeds nd")
        if not 1 <= self.min_cells <= 1024:
            raise ValueError("cluster: min_cells must be in [1, 1024]")
        if not 1 <= self.max_tgt <= 64:
            raise ValueError("cluster: max_tgt must be in [1, 64]")
        if not 1 <= max_det <= 1024:
            raise ValueError("cluster: max_det must be in [1, 1024]")

    @classmethod
    def for_config(cls, cfg: "FmcwConfig", link=(1, 1), min_cells: int = 2, max_tgt: int = 16,
                   max_det: int = 64) -> "ClusterConfig":
        """The clustering for cfg's RD map and lists of max_det entries (CfarConfig.for_config's
        default): 8-connectivity, single-cell clusters (isolated false alarms) dropped."""
        q = cls(link_r=int(link[0]), link_d=int(link[1]), min_cells=int(min_cells), max_tgt=int(max_tgt))
        q.validate(cfg.nr, cfg.nd, int(max_det))
        return q


@dataclass
class AoaConfig:
    """fmcw_aoa_params (include/fmcw.h): angle of arrival from n_chan receive channels' RD maps at the
    CFAR cells.  spacing is the element spacing in wavelengths (signed: the sign sets which side is
    positive); weights holds one complex weight per channel (None: 1 for every channel), which absorbs
    the receive paths' phase and gain mismatch; max_tgt 0 asks for no per-target outputs."""
    n_chan: int = 2
    spacing: float = 0.5
    max_tgt: int = 16
    weights: tuple | None = None

    def abi(self) -> AoaParams:
        w = [1.0, 0.0] * 8
        if self.weights is not None:
            ws = [complex(x) for x in self.weights]
            if len(ws) != self.n_chan or len(ws) > 8:
                raise ValueError("aoa: weights needs one complex value per channel")
            for i, x in enumerate(ws):
                w[2 * i], w[2 * i + 1] = x.real, x.imag
        q = AoaParams(self.n_chan, self.max_tgt, 0, self.spacing)
        with np.errstate(over="ignore"):
            q.w[:] = [float(np.float32(x)) for x in w]
        return q

    @property
    def kinv(self) -> np.float32:
        """1 / (2 pi spacing) from the float32 spacing the C struct carries, as the library forms it."""
        return np.float32(1.0 / (2.0 * np.pi * float(np.float32(self.spacing))))

    def weights_f32(self) -> np.ndarray:
        """float32 [n_chan][2]: the weights as the C struct carries them."""
        return np.array(self.abi().w[:2 * self.n_chan], np.float32).reshape(self.n_chan, 2)

    def validate(self, nr: int, nd: int, max_det: int) -> None:
        """The rules of fmcw_aoa_check, on the float32 values the C struct carries; ValueError naming
        the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("aoa: nr must be a power of two in [16, 2048]")
        if nd < 4 or nd > 1024 or nd & (nd - 1):
            raise ValueError("aoa: nd must be a power of two in [4, 1024]")
        if not 2 <= self.n_chan <= 8:
            raise ValueError("aoa: n_chan must be in [2, 8]")
        if not 0 <= self.max_tgt <= 64:
            raise ValueError("aoa: max_tgt must be 0 or in [1, 64]")
        if not 1 <= max_det <= 1024:
            raise ValueError("aoa: max_det must be in [1, 1024]")
        with np.errstate(over="ignore"):
            sp = np.float32(self.spacing)
        if not (np.isfinite(sp) and np.float32(0.01) <= abs(sp) <= np.float32(16)):
            raise ValueError("aoa: spacing must be finite with 0.01 <= |spacing| <= 16")
        if not np.isfinite(self.weights_f32()).all():
            raise ValueError("aoa: the weights must be finite")


@dataclass
class TrackConfig:
    """fmcw_track_params (include/fmcw.h): tracks the targets of fmcw_cluster across frames.  A
    measurement is associated with a track inside the gate (er / gate_r)^2 + (x / gate_d)^2 <= 1 (bins,
    Doppler circular); alpha_r / beta_r filter the range and the range rate, alpha_d the Doppler; a
    track is confirmed at confirm_hits hits and coasts through at most max_coast missed frames."""
    gate_r: float = 4.0
    gate_d: float = 4.0
    alpha_r: float = 0.5
    alpha_d: float = 0.5
    beta_r: float = 0.25
    confirm_hits: int = 3
    max_coast: int = 3
    max_trk: int = 16

    def abi(self) -> TrackParams:
        return TrackParams(self.gate_r, self.gate_d, self.alpha_r, self.alpha_d, self.beta_r, self.confirm_hits,
                           self.max_coast, self.max_trk, 0)

    def validate(self, nr: int, nd: int, max_tgt: int) -> None:
        """The rules of fmcw_track_check, on the float32 values the C struct carries; ValueError
        naming the first one violated."""
        f = np.float32
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("track: nr must be a power of two in [16, 2048]")
        if nd < 4 or nd > 1024 or nd & (nd - 1):
            raise ValueError("track: nd must be a power of two in [4, 1024]")
        if not 1 <= max_tgt <= 64:
            raise ValueError("track: max_tgt must be in [1, 64]")
        with np.errstate(over="ignore"):
            gr, gd, ar, ad, br = (f(x) for x in (self.gate_r, self.gate_d, self.alpha_r, self.alpha_d, self.beta_r))
        if not (np.isfinite(gr) and gr > 0):
            raise ValueError("track: gate_r must be finite and > 0")
        if not (np.isfinite(gd) and gd > 0):
            raise ValueError("track: gate_d must be finite and > 0")
        if not gd < f(nd // 2):
            raise ValueError("track: gate_d must be below nd/2")
        if not 0 < ar <= 1:
            raise ValueError("track: alpha_r must be in (0, 1]")
        if not 0 < ad <= 1:
            raise ValueError("track: alpha_d must be in (0, 1]")
        if not 0 <= br <= 1:
            raise ValueError("track: beta_r must be in [0, 1]")
        if not 1 <= self.confirm_hits <= 255:
            raise ValueError("track: confirm_hits must be in [1, 255]")
        if not 0 <= self.max_coast <= 255:
            raise ValueError("track: max_coast must be in [0, 255]")
        if not 1 <= self.max_trk <= 64:
            raise ValueError("track: max_trk must be in [1, 64]")

    @classmethod
    def for_config(cls, cfg: "FmcwConfig", gate=(4.0, 4.0), alpha=(0.5, 0.5), beta_r: float = 0.25,
                   confirm_hits: int = 3, max_coast: int = 3, max_trk: int = 16, max_tgt: int = 16) -> "TrackConfig":
        """The tracker for cfg's RD map and target lists of max_tgt entries (ClusterConfig.for_config's
        default); the Doppler gate is cut to stay below nd/2 on a short ring."""
        gd = min(float(gate[1]), cfg.nd / 2 - 0.5)
        q = cls(gate_r=float(gate[0]), gate_d=gd, alpha_r=float(alpha[0]), alpha_d=float(alpha[1]),
                beta_r=float(beta_r), confirm_hits=int(confirm_hits), max_coast=int(max_coast), max_trk=int(max_trk))
        q.validate(cfg.nr, cfg.nd, int(max_tgt))
        return q


def derive_params(device: dict, nr: int = 256, nd: int = 16, mode: str = PARITY, **over) -> FmcwConfig:
    """radar_processing.m:89-115 from the sXML fields.

    ``device`` keys (sXML.Device...Text): chirpDuration_ns, upperFrequency_kHz,
    lowerFrequency_kHz, numAntennasTx, numAntennasRx, numSamplesPerChirp,
    numChirpsPerFrame, samplerateHz.  ``nr``/``nd`` are the literal 256/16 of
    :118-119 in parity mode.
    """
    up = float(device["chirpDuration_ns"]) * 1e-9                                  # :94
    prt = up + 200e-6 + 300e-6                                                     # :95-97
    hi, lo = float(device["upperFrequency_kHz"]), float(device["lowerFrequency_kHz"])
    cfg = FmcwConfig(
        prt=prt, bw=(hi - lo) * 1e3, fc=(hi + lo) / 2 * 1e3,                     # :100, :106
        nts=int(device["numSamplesPerChirp"]), pn=int(device["numChirpsPerFrame"]),  # :109, :112
        nr=int(nr), nd=int(nd), n_rx=int(device.get("numAntennasRx", 1)),
        n_tx=int(device.get("numAntennasTx", 1)), fs_adc=float(device.get("samplerateHz", 0.0)),
        mode=mode)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def gate_bins(cfg: FmcwConfig) -> np.ndarray:
    """The 0-based range bins the peak rule (:211, f_search_peak) admits, as the kernels compute
    them (select_peaks in frame_ops.h, k_rdx's candidate keys): bins i in 1..nr-2 with
    i * dist_per_bin in [min_d, max_d], the product in double from the float32 parameters the
    C-ABI carries.  When a limit lies on a bin and dist_per_bin is not exact in binary, this
    gate and the one computed from the Python doubles differ by that bin; the CFAR and
    signature gates (CfarConfig.for_config) are this one, so all three are one set of rows."""
    f = np.float32
    with np.errstate(over="ignore"):
        dpb, lo, hi = float(f(cfg.dist_per_bin)), float(f(cfg.min_d)), float(f(cfg.max_d))
    i = np.arange(1, max(cfg.nr - 1, 1))
    d = i.astype(np.float64) * dpb
    return i[(d >= lo) & (d <= hi)]


def fp16_fp32_bins(cfg: FmcwConfig) -> np.ndarray:
    """Range bins whose hand-off stays fp32 under fp16 storage on the XCD-team schedule: the
    128-bin blocks that hold a bin able to become a detection or slow-time candidate (min_d /
    max_d of :126-127, two bins of margin); the other blocks travel as c32h X / Nr.  Mirror of
    fmcw_api.cpp host_s16mask (float32 parameters as the C-ABI carries them), for checks that
    hold the profile in those blocks, and the target magnitudes, to the fp32 bar."""
    nr = cfg.nr
    dpb = float(np.float32(cfg.dist_per_bin))
    keep = np.ones(nr, bool)
    if not (dpb > 0 and np.isfinite(dpb)) or nr % 128:
        return keep
    lo_d = np.floor(float(np.float32(cfg.min_d)) / dpb) - 2
    hi_d = np.ceil(float(np.float32(cfg.max_d)) / dpb) + 2
    lo = int(max(0.0, min(float(nr), lo_d)))
    hi = int(max(-1.0, min(float(nr - 1), hi_d)))
    for b in range(nr // 128):
        if hi < lo or 128 * b + 127 < lo or 128 * b > hi:
            keep[128 * b: 128 * b + 128] = False
    return keep


def calibration(calib_data: np.ndarray, n_rx: int, nts: int) -> np.ndarray:
    """:166-174 calib_rx1 = (I(1:dec:N_cal) + 1i*Q(1:dec:N_cal)).'"""
    calib_data = np.asarray(calib_data, dtype=np.float64).reshape(-1)
    n_cal = len(calib_data) // (2 * n_rx)
    if n_cal % nts:
        raise ValueError("calibration length is not a multiple of NTS (MATLAB would fail to index)")
    dec = n_cal // nts
    return calib_data[0:n_cal:dec] + 1j * calib_data[n_cal:2 * n_cal:dec]


def deployed_device(nts: int = 64, pn: int = 16) -> dict:
    """The deployed Infineon 24 GHz module: PRT 0.8 ms, BW 200 MHz,
    fc 24.125 GHz; NTS/PN as given (64 x 16 in the field, larger for configs 1-5)."""
    return dict(chirpDuration_ns=300000, upperFrequency_kHz=24225000, lowerFrequency_kHz=24025000,
                numAntennasTx=1, numAntennasRx=2, numSamplesPerChirp=nts, numChirpsPerFrame=pn,
                samplerateHz=nts / 300e-6)


def synth_calibration(nts: int) -> np.ndarray:
    """Calibration used with synthetic frames: 0.01 e^{j 2 pi 0.013 n}."""
    n = np.arange(nts)
    return 0.01 * np.exp(2j * np.pi * ((0.013 * n) % 1.0))


# BASELINE.json configs (geometry only; the device constants are the deployed ones)
CONFIGS = {
    1: dict(nts=256, pn=128, nr=256, nd=16, frames=1, mode=PARITY),
    2: dict(nts=512, pn=128, nr=512, nd=16, frames=4096, mode=THROUGHPUT),
    3: dict(nts=1024, pn=256, nr=1024, nd=256, frames=4096, mode=THROUGHPUT),
    4: dict(nts=1024, pn=256, nr=1024, nd=256, frames=4096, mode=THROUGHPUT, stft_nfft=64),
    5: dict(nts=1024, pn=256, nr=1024, nd=256, frames=65536, mode=THROUGHPUT, stft_nfft=64),
    "deployed": dict(nts=64, pn=16, nr=256, nd=16, frames=115, mode=PARITY),
}


def config(name, **over) -> FmcwConfig:
    c = dict(CONFIGS[name])
    c.update(over)
    cfg = derive_params(deployed_device(c["nts"], c["pn"]), nr=c["nr"], nd=c["nd"], mode=c["mode"])
    cfg.extra = {k: v for k, v in c.items() if k not in ("nts", "pn", "nr", "nd", "mode")}
    return cfg


@dataclass
class MtiConfig:
    """fmcw_mti_params (include/fmcw.h): the frame-to-frame clutter filter of the RD map.  A complex
    background per cell follows the frames with gain lambda_ (1: the two-frame canceller) and is
    subtracted coherently.  ramp: the gain starts at 1 / (frames seen + 1), the running mean, and
    settles at lambda_.  freeze: subtract the learned background without updating it."""
    lambda_: float = 0.05
    ramp: bool = True
    freeze: bool = False

    def abi(self) -> MtiParams:
        return MtiParams(self.lambda_, (FMCW_MTI_RAMP if self.ramp else 0) | (FMCW_MTI_FREEZE if self.freeze else 0))

    def validate(self, nr: int, nd: int) -> None:
        """The rules of fmcw_mti_check, on the float32 value the C struct carries; ValueError naming
        the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("mti: nr must be a power of two in [16, 2048]")
        if nd < 4 or nd > 1024 or nd & (nd - 1):
            raise ValueError("mti: nd must be a power of two in [4, 1024]")
        with np.errstate(over="ignore"):
            lam = np.float32(self.lambda_)
        if not (np.isfinite(lam) and 0 < lam <= 1):
            raise ValueError("mti: lambda must be finite and in (0, 1]")


@dataclass
class BeamConfig:
    """fmcw_beam_params (include/fmcw.h): the receive channels' RD maps combined into n_beam maps.
    weights holds one complex weight per (beam, channel), [n_beam][n_chan] (Engine.beam_weights forms
    those of a uniform line).  nci: non-coherent integration, one map of sqrt(sum |w_a x_a|^2) from
    weights[0]; it needs n_beam 1."""
    weights: np.ndarray
    nci: bool = False

    def __post_init__(self):
        w = np.asarray(self.weights)
        if w.ndim != 2:
            raise ValueError("beam: weights must be [n_beam][n_chan] complex")
        with np.errstate(over="ignore"):
            self.weights = w.astype(np.complex64)

    @property
    def n_beam(self) -> int:
        return self.weights.shape[0]

    @property
    def n_chan(self) -> int:
        return self.weights.shape[1]

    def abi(self) -> BeamParams:
        B, A = self.weights.shape
        if B > 8 or A > 8:
            raise ValueError("beam: at most 8 beams of 8 channels")
        w = np.zeros((8, 8, 2), np.float32)
        w[:B, :A, 0], w[:B, :A, 1] = self.weights.real, self.weights.imag
        q = BeamParams(A, B, FMCW_BEAM_NCI if self.nci else 0)
        q.w[:] = w.reshape(-1).tolist()
        return q

    def weights_f32(self) -> np.ndarray:
        """float32 [n_beam][n_chan][2]: the weights as the C struct carries them."""
        return np.ascontiguousarray(self.weights).view(np.float32).reshape(self.n_beam, self.n_chan, 2)

    def validate(self, nr: int, nd: int) -> None:
        """The rules of fmcw_beam_check; ValueError naming the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("beam: nr must be a power of two in [16, 2048]")
        if nd < 4 or nd > 1024 or nd & (nd - 1):
            raise ValueError("beam: nd must be a power of two in [4, 1024]")
        if not 2 <= self.n_chan <= 8:
            raise ValueError("beam: n_chan must be in [2, 8]")
        if not 1 <= self.n_beam <= 8:
            raise ValueError("beam: n_beam must be in [1, 8]")
        if self.nci and self.n_beam != 1:
            raise ValueError("beam: FMCW_BEAM_NCI needs n_beam == 1")
        if not np.isfinite(self.weights_f32()).all():
            raise ValueError("beam: the weights must be finite")


@dataclass
class RaConfig:
    """fmcw_ra_params (include/fmcw.h): range-angle maps from n_chan receive channels' RD maps.  Per
    range row the channels' spatial covariance over the Doppler bins kept (dc_half leaves the bins
    |d - nd/2| <= dc_half out, -1: none), then its angular power spectrum over n_ang look directions
    (a weight table of Engine.ra_weights): Bartlett, or with capon the Capon / MVDR spectrum under
    the diagonal loading `load` (relative to the mean diagonal).  The gate r_lo..r_hi is 1-based and
    inclusive, (0, 0) = every row; rows outside it are zero."""
    n_chan: int
    n_ang: int
    r_lo: int = 0
    r_hi: int = 0
    dc_half: int = 0
    capon: bool = False
    load: float = 1e-3

    def abi(self) -> RaParams:
        return RaParams(int(self.n_chan), int(self.n_ang), int(self.r_lo), int(self.r_hi), int(self.dc_half),
                        FMCW_RA_CAPON if self.capon else 0, self.load)

    def validate(self, nr: int, nd: int) -> None:
        """The rules of fmcw_ra_check, on the float32 value the C struct carries; ValueError naming
        the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("ra: nr must be a power of two in [16, 2048]")
        if nd < 4 or nd > 1024 or nd & (nd - 1):
            raise ValueError("ra: nd must be a power of two in [4, 1024]")
        if self.r_lo > self.r_hi:
            raise ValueError("ra: r_lo > r_hi")
        if (self.r_lo, self.r_hi) != (0, 0) and (self.r_lo < 1 or self.r_hi > nr):
            raise ValueError("ra: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)")
        if not 2 <= self.n_chan <= 8:
            raise ValueError("ra: n_chan must be in [2, 8]")
        if not 1 <= self.n_ang <= 256:
            raise ValueError("ra: n_ang must be in [1, 256]")
        if self.dc_half < -1:
            raise ValueError("ra: dc_half must be >= -1 (-1 leaves no Doppler bin out)")
        if 2 * self.dc_half + 1 >= nd:
            raise ValueError("ra: 2 dc_half + 1 must be < nd")
        with np.errstate(over="ignore"):
            load = np.float32(self.load)
        if not (np.isfinite(load) and load >= 0):
            raise ValueError("ra: load must be finite and >= 0")


@dataclass
class MusicConfig:
    """fmcw_music_params (include/fmcw.h): MUSIC angular spectra from the covariance of every range
    row (what RaConfig's covariance stage writes).  Per row the eigen-decomposition by `sweeps` cyclic
    Jacobi sweeps, a source count (n_src, or with n_src = 0 the number of eigenvalues above src_thr
    times the mean of the n_chan - max_src smallest, at most max_src) and the pseudo-spectrum over
    n_ang look directions (a weight table of Engine.ra_weights).  fb: forward-backward averaging,
    for a uniform line; it separates returns of one Doppler bin.  The gate r_lo..r_hi is 1-based and
    inclusive, (0, 0) = every row; rows outside it are zero."""
    n_chan: int
    n_ang: int
    r_lo: int = 0
    r_hi: int = 0
    n_src: int = 0
    max_src: int = 1
    sweeps: int = 8
    fb: bool = False
    src_thr: float = 8.0

    def abi(self) -> MusicParams:
        return MusicParams(int(self.n_chan), int(self.n_ang), int(self.r_lo), int(self.r_hi), int(self.n_src),
                           int(self.max_src), int(self.sweeps), FMCW_MUSIC_FB if self.fb else 0, self.src_thr)

    def validate(self, nr: int) -> None:
        """The rules of fmcw_music_check, on the float32 value the C struct carries; ValueError
        naming the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("music: nr must be a power of two in [16, 2048]")
        if self.r_lo > self.r_hi:
            raise ValueError("music: r_lo > r_hi")
        if (self.r_lo, self.r_hi) != (0, 0) and (self.r_lo < 1 or self.r_hi > nr):
            raise ValueError("music: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)")
        if not 2 <= self.n_chan <= 8:
            raise ValueError("music: n_chan must be in [2, 8]")
        if not 1 <= self.n_ang <= 256:
            raise ValueError("music: n_ang must be in [1, 256]")
        if not 0 <= self.n_src <= self.n_chan - 1:
            raise ValueError("music: n_src must be in [0, n_chan - 1] (0 estimates it)")
        if self.n_src == 0 and not 1 <= self.max_src <= self.n_chan - 1:
            raise ValueError("music: max_src must be in [1, n_chan - 1] when n_src is 0")
        if not 1 <= self.sweeps <= 16:
            raise ValueError("music: sweeps must be in [1, 16]")
        with np.errstate(over="ignore"):
            thr = np.float32(self.src_thr)
        if not (np.isfinite(thr) and thr > 0):
            raise ValueError("music: src_thr must be finite and > 0")


@dataclass
class DoaConfig:
    """fmcw_doa_params (include/fmcw.h): directions of arrival, the peaks of an angular spectrum
    [F][nr][n_ang] (Bartlett or Capon of RaConfig, MUSIC of MusicConfig, or a caller's own) per range
    row.  A peak is above both neighbours (of a flat top its first point); it is kept when positive,
    >= min_abs, >= min_rel times the row's maximum and >= min_prom times its base (the reference
    level of findpeaks' prominence; 0 switches the rule off); kept peaks are ordered by power and
    the first max_pk written, each with a sub-grid direction from a parabola through the peak and
    its neighbours (inv: through their reciprocals, for Capon and MUSIC).  edges: the first and
    the last grid point can be peaks; wrap: the grid is cyclic (not with edges; n_ang >= 3).  The
    gate r_lo..r_hi is 1-based and inclusive, (0, 0) = every row; rows outside it hold no peak."""
    n_ang: int
    max_pk: int = 4
    r_lo: int = 0
    r_hi: int = 0
    edges: bool = False
    wrap: bool = False
    inv: bool = False
    min_abs: float = 0.0
    min_rel: float = 0.0
    min_prom: float = 0.0

    @property
    def flags(self) -> int:
        return (FMCW_DOA_EDGES if self.edges else 0) | (FMCW_DOA_WRAP if self.wrap else 0) | (FMCW_DOA_INV if self.inv else 0)

    def to_c(self) -> DoaParams:
        return DoaParams(int(self.n_ang), int(self.r_lo), int(self.r_hi), int(self.max_pk), self.flags, self.min_abs,
                         self.min_rel, self.min_prom)

    abi = to_c                  # the name the other configurations use

    def check(self, nr: int) -> None:
        """The rules of fmcw_doa_check, on the float32 values the C struct carries; ValueError
        naming the first one violated."""
        if nr < 16 or nr > 2048 or nr & (nr - 1):
            raise ValueError("doa: nr must be a power of two in [16, 2048]")
        if self.r_lo > self.r_hi:
            raise ValueError("doa: r_lo > r_hi")
        if (self.r_lo, self.r_hi) != (0, 0) and (self.r_lo < 1 or self.r_hi > nr):
            raise ValueError("doa: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)")
        if not 1 <= self.n_ang <= 256:
            raise ValueError("doa: n_ang must be in [1, 256]")
        if not 1 <= self.max_pk <= 8:
            raise ValueError("doa: max_pk must be in [1, 8]")
        if self.edges and self.wrap:
            raise ValueError("doa: FMCW_DOA_EDGES and FMCW_DOA_WRAP exclude each other")
        if self.wrap and self.n_ang < 3:
            raise ValueError("doa: FMCW_DOA_WRAP needs n_ang >= 3")
        with np.errstate(over="ignore"):
            min_abs, min_rel, min_prom = np.float32(self.min_abs), np.float32(self.min_rel), np.float32(self.min_prom)
        if not (np.isfinite(min_abs) and min_abs >= 0):
            raise ValueError("doa: min_abs must be finite and >= 0")
        if not 0 <= min_rel <= 1:
            raise ValueError("doa: min_rel must be in [0, 1]")
        if not (np.isfinite(min_prom) and min_prom >= 0):
            raise ValueError("doa: min_prom must be finite and >= 0")

    validate = check            # the name the other configurations use
