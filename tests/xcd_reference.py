"""Cases, inputs and references of the single-pass schedule's grid (k_rdx of csrc/kernels_xcd.hip with
k_detect_1p of csrc/kernels_detect.hip; tests/test_gpu_xcd_grid.py); test-side numpy code, no GPU.
tests/test_xcd_reference_host.py proves on the oracle alone what the GPU module relies on.

The geometry is the single pass's own: 256 chirps, Nr 1024, Nd 256, and every even nts in 2..1024.  What
varies is nts (the masked 64-lane load pieces, S2 = nts / 2 sample pairs per chirp), where a frame's
energy lies (tone-dominated, white, in one chirp only), the frame's chirp 0 (k_rdx transforms every other
chirp as x_k - x_0 and hands over X_0 and X'_k = X_k - X_0), the hand-off storage under fp16 (one mask bit
per 128-bin block: c32h X / Nr) and the frame count against teams, slots and steps.

emulate_xcd() is streams_reference.emulate with the single pass's stores.  e_ref and bound() are those
of streams_reference: the kernels are held to 2 e_ref + the fp32 bar against the plain chain.
"""
from __future__ import annotations

import copy
import dataclasses

import numpy as np
import scipy.fft

from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import detect_reference as DR
from tests import streams_reference as SR
from tests import taps_cases as TC
from tests.helpers import TOL_FP32_REL_L2, rd_rel_err, rel_l2
from tests.streams_reference import C32H, C64

PN, NR, ND = 256, 1024, 256
NGROUPS = 32

# S2 = nts / 2 sample pairs per chirp, loaded as eight pieces of 64 lanes (lane + 64 i < S2)
NTS_CASES = [
    30,      # S2 = 15 < 64: seven pieces wholly masked
    62,      # S2 = 31 < 64
    64,      # S2 = 32 < 64
    66,      # S2 = 33 < 64
    126,     # S2 = 63, just below a multiple of 64
    128,     # S2 = 64, on a piece boundary: piece 0 whole, pieces 1..7 wholly masked
    130,     # S2 = 65, just above: one lane of piece 1
    254,     # S2 = 127, just below 128
    510,     # S2 = 255, just below 256; pieces 4..7 wholly masked
    512,     # S2 = 256, on a piece boundary
    514,     # S2 = 257, just above
    1000,    # S2 = 500: the mask inside the last piece (the case the suite had)
    1022,    # S2 = 511: one lane masked
    1024,    # FULL = true
]
DEGENERATE_NTS = [2, 4]                 # Blackman(2) is zero; at nts 4 every frame is a near tie
FP16_NTS = [30, 126, 128, 510, 1000, 1024]
FULL_HOT_NTS = (126, 1024)             # every chirp position 8 m + w of members m = 0, 1, 31 is hot once
HOT_SHORT = (0, 1, 7, 8, 9, 255)
HOT_FULL = tuple(8 * m + w for m in (0, 1, 31) for w in range(8))
HOT_TAPS, HOT_TAPS_MID = (0, 1, 254, 255), (7, 8, 9)   # the one-hot frames under the non-plain taps of tests/taps_cases.py
TAPS_TAG = 77                           # seeds the one-hot noise under non-plain taps
FRAME_COUNTS = [1, 2, 7, 8, 9, 15, 16, 17, 33]
FRAME_COUNTS_FP16 = (9, 17)
CHUNK_NTS = [126, 1024]
K_X0 = 3                                # item 4 of frames(): chirp 0 carries 2^K_X0 times its noise (choose_k)
K_MAX = 6
# Left out of the c32h RD comparison, by nts and name: the frames whose e_ref of the RD map is above
# streams_reference.E_REF_MAX there (test_xcd_reference_host asserts exactly these and no others, at every
# hand-off mask a test runs).  white_x0's slot holds X_k - X_0 at 2^K_X0 times the size of X_k, and the fp16
# rounding of that is what the RD map comes from wherever a block is c32h (every nts but 30, mask 0x00); a
# one-hot frame's map is wd[c] X_c in all but seven columns, which D / (Nr Nd) puts the deeper among the fp16
# subnormals the larger nts is (e_ref 2.6e-4 .. 5.0e-4 up to nts 128, 7.8e-4 .. 1.2e-3 from nts 510).
FP16_X0_LEFT_OUT = (126, 128, 510, 1000, 1024)
FP16_HOT_LEFT_OUT = (510, 1000, 1024)
HOT_SIGMA = SR.NOISE_SIGMA
# one-hot frames (nts, c) whose first noise draw is a near tie of the peak rule on the oracle: the next draw
RESEED = {(30, 7): [1]}

# min_d / max_d at nts 1024 (dist_per_bin 0.75) -> the hand-off mask of host_s16mask, bit b = block b is c32h
MASK_GATES = {
    0x00: dict(min_d=0.0, max_d=1.0e6),          # every block holds a gate bin
    0xFE: dict(),                                # the default gate: bins 2..33
    0x7F: dict(min_d=675.0, max_d=1.0e6),        # bins 900..1022: block 7 only
    0xE7: dict(min_d=300.0, max_d=450.0),        # bins 400..600: blocks 3 and 4
    0xFF: dict(min_d=100.0, max_d=1.0),          # an empty gate: no block stays fp32
}


def pieces(nts: int) -> dict:
    """How the eight 64-lane pieces of a chirp's loads are masked at nts."""
    s2 = nts // 2
    n = [max(0, min(64, s2 - 64 * i)) for i in range(8)]
    return dict(s2=s2, whole=sum(v == 64 for v in n), partial=sum(0 < v < 64 for v in n), masked=sum(v == 0 for v in n))


def geometry(nts: int):
    return (nts, PN, NR, ND, 2)


def build_case(nts: int, taps="plain", **over):
    """(cfg, p, wr, wd, cal) at nts with detection-parameter overrides; p carries the float32 ABI values.
    taps: the family of tests/taps_cases.py."""
    cfg, p, wr, wd, cal = SR.build_case(geometry(nts), taps=taps)
    if over:
        cfg = dataclasses.replace(cfg, **over)
        p = DR.oracle_params(p, cfg, cfg.max_targets)
    return cfg, p, wr, wd, cal


def mask_of(cfg) -> int:
    """The hand-off mask of cfg under fp16 storage (the mirror of host_s16mask)."""
    keep = P.fp16_fp32_bins(cfg)
    return sum(1 << b for b in range(cfg.nr // 128) if not keep[128 * b])


def group_rows(g: int) -> np.ndarray:
    """The 32 range bins of group g (team member g's Doppler stage)."""
    return np.array([r for r in range(NR) if DR.xcd_group(r) == g])


GROUP_ROWS = np.stack([group_rows(g) for g in range(NGROUPS)])
assert GROUP_ROWS.shape == (NGROUPS, 32) and len(np.unique(GROUP_ROWS)) == NR


# --------------------------------------------------------------------------
# the frames
# --------------------------------------------------------------------------
def _cn(rng, shape, sigma):
    return (sigma / np.sqrt(2.0)) * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def hot_chirps(nts: int, taps="plain") -> tuple:
    """The hot chirps of a batch.  Under non-plain taps: both ends of the frame, and 7, 8, 9 (a wave and a
    member boundary) where those chirps carry Doppler weight (not under `ends`)."""
    if taps != "plain":
        return HOT_TAPS if taps == "ends" else tuple(sorted(HOT_TAPS + HOT_TAPS_MID))
    return tuple(sorted(set(HOT_SHORT) | set(HOT_FULL))) if nts in FULL_HOT_NTS else HOT_SHORT


def white(nts: int, tag: int, taps="plain") -> np.ndarray:
    """Calibration tone + CN(0, 0.05^2), complex128 [C][S]; tag 7 is streams_reference.noise_frame."""
    rng = np.random.default_rng([nts, PN, NR, ND, tag])
    return TC.cal_of(taps, nts)[None, :] + _cn(rng, (PN, nts), SR.NOISE_SIGMA)


def white_x0(nts: int, k: int, taps="plain") -> np.ndarray:
    """A white frame whose chirp 0 carries 2^k times its own noise, the calibration tone unscaled."""
    x = white(nts, 9, taps)
    cal = TC.cal_of(taps, nts)
    x[0] = cal + (2.0 ** k) * (x[0] - cal)
    return x.astype(np.complex64)


def one_hot(nts: int, c: int, taps="plain") -> np.ndarray:
    """Every chirp the calibration tone, chirp c the calibration tone + CN(0, 0.05^2)."""
    cal = TC.cal_of(taps, nts)
    x = np.broadcast_to(cal[None, :], (PN, nts)).copy()
    seed = RESEED.get((nts, c), []) if taps == "plain" else [TAPS_TAG] + TC.RESEED_HOT.get((taps, nts, c), [])
    x[c] += _cn(np.random.default_rng([nts, 11, c] + seed), nts, HOT_SIGMA)
    return x.astype(np.complex64)


def frames(nts: int, taps="plain"):
    """(names, iq complex64 [F][C][S]): the batch of one nts, every frame distinct."""
    g = geometry(nts)
    _, p, *_ = build_case(nts, taps)
    ids = SR.frame_ids(g, p)
    names, out = [], []
    for f in ids:                                                   # 1: one synthetic frame with, one without a target
        A = O.synth_frame_params(f, NR, ND, p["dist_per_bin"])["A"]
        names.append("synth_target" if A > 0 else "synth_empty")
        out.append(TC.retone(O.synth_frames(1, PN, nts, NR, ND, p["dist_per_bin"], frame0=f)[0], taps))
    names.append("white")                                           # 2
    out.append(SR.noise_frame(g, taps)[0])
    x = white(nts, 8, taps)                                         # 3: chirp 0 the bare calibration tone
    x[0] = TC.cal_of(taps, nts)
    names.append("white_cal0")
    out.append(x.astype(np.complex64))
    names.append("white_x0")                                        # 4
    out.append(white_x0(nts, k_x0(taps), taps))
    for c in hot_chirps(nts, taps):                                 # 5
        names.append(f"hot{c}")
        out.append(one_hot(nts, c, taps))
    return names, np.stack(out)


def is_flat(name: str) -> bool:
    """The frames whose energy is in every range bin: held per group, per Doppler residue, element-wise."""
    return name.startswith("white") or name.startswith("hot")


# --------------------------------------------------------------------------
# item 4: how large chirp 0 may be.  The kernel's algebra in float32
# --------------------------------------------------------------------------
def restate_f32(x, cal, p, wr, wd):
    """k_rdx's algebra for one frame x complex64 [C][S], every step rounded to float32 (complex64):
    d_k = x_k - x_0 and its mean, X'_k = FFT((d_k - mean d_k) w') by scipy.fft on complex64, chirp 0 as
    (x_0 - mu) w' - cal w'; the profile from X'_k + X_0, the row mean from the X'_k (X'_0 = 0), in two passes.
    Returns (profile [nr], rd [nr][nd]) widened to double."""
    c64, f32 = np.complex64, np.float32
    C, S = x.shape
    nr, nd = p["nr"], p["nd"]
    x = x.astype(c64)
    w = (p["if_scale"] * np.asarray(wr)).astype(f32)
    calw = (np.asarray(cal) * p["if_scale"] * np.asarray(wr)).astype(c64)
    mu0 = ((x[0].sum(dtype=c64) - c64(np.sum(cal))) / f32(S)).astype(c64)
    X0 = scipy.fft.fft(((x[0] - mu0) * w - calw).astype(c64), n=nr)
    d = (x - x[0][None, :]).astype(c64)
    d = (d - (d.sum(axis=1, dtype=c64) / f32(S))[:, None]).astype(c64)
    Xp = scipy.fft.fft((d * w[None, :]).astype(c64), n=nr, axis=1)
    assert X0.dtype == c64 and Xp.dtype == c64
    Xp[0] = 0
    prof = np.abs((Xp + X0[None, :]).astype(c64)).max(axis=0)
    y = (Xp - (Xp.sum(axis=0, dtype=c64) / f32(C)).astype(c64)[None, :]).astype(c64)
    y = (y - (y.sum(axis=0, dtype=c64) / f32(C)).astype(c64)[None, :]).astype(c64)        # the mean in two passes
    y = (y * np.asarray(wd).astype(f32)[:, None]).astype(c64)
    rd = np.fft.fftshift(scipy.fft.fft(y, n=nd, axis=0), axes=0).T
    assert rd.dtype == c64
    return prof.astype(np.float64), rd.astype(np.complex128)


def restate_errors(nts: int, k: int, taps="plain", frame="white_x0"):
    """(rd, profile, rd_max): the float32 restatement of white_x0(nts, k), or of the white frame, against the
    oracle: the RD map with rd_rel_err's normalisation, the profile's plain L2, and the RD map element-wise,
    max |d| / rms."""
    _, p, wr, wd, cal = build_case(nts, taps)
    x = white_x0(nts, k, taps) if frame == "white_x0" else SR.noise_frame(geometry(nts), taps)[0]
    ref = O.process_frames(x[None], cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    prof, rd = restate_f32(x, cal, p, wr, wd)
    return (float(rd_rel_err(rd[None], ref["rd"], ref["cube"], wd, ND)[0]), float(rel_l2(prof, ref["profile"][0])),
            float(np.abs(rd - ref["rd"][0]).max()) / rms(ref["rd"][0]))


K_NTS = (1024, 1000, 126, 30)


def k_x0(taps="plain") -> int:
    """The chirp-0 scale of white_x0 under a family of taps: K_X0, or taps_cases.K_X0 (chosen by choose_k too)."""
    return K_X0 if taps == "plain" else TC.K_X0[taps]


def carries(figs) -> bool:
    """The condition on a chirp-0 scale: the restatement's L2 figures under half the fp32 bar, and its
    element-wise figure under half the bar the GPU test holds every white frame to as well (a frame that
    float32 arithmetic itself carries only just under that bar would test the number format, not the
    kernel: any reordering of the range FFT's sums could fail it)."""
    return max(figs) < 0.5 * TOL_FP32_REL_L2


def choose_k(taps="plain", k_from=0):
    """(k, figures): the largest k <= K_MAX up to which carries() holds at every nts of K_NTS (tried from
    k_from on); figures[k][nts] = restate_errors for every k tried."""
    figs, best = {}, k_from - 1
    for k in range(k_from, K_MAX + 1):
        figs[k] = {nts: restate_errors(nts, k, taps) for nts in K_NTS}
        if not all(carries(f) for f in figs[k].values()):
            break
        best = k
    return best, figs


# --------------------------------------------------------------------------
# the emulated chain
# --------------------------------------------------------------------------
def emulate_xcd(iq, cal, p, wr, wd, mask=0, rd_dtype=C64, probe_column=0) -> dict:
    """oracle.process_frames(rd_all_rows) with the single pass's stores.  Where bit b of mask is set, rows
    128 b .. 128 b + 127 of what the hand-off slot holds (X_0 for chirp 0, X_k - X_0 for the others) are
    fp16_round(., 1 / Nr) before X_k is formed again; the profile, the slow-time row, the target
    magnitudes and the probe column come from the re-formed X_k, the RD map from the rounded X'_k
    (X'_0 = 0), through fp16_round(., 1 / (Nr Nd)) where rd_dtype is C32H.  Rows of a block whose bit is
    clear are the oracle's own values, so mask 0 with a c64 RD map is oracle.process_frames bit for bit."""
    F, C, S = iq.shape
    nr, nd, M = p["nr"], p["nd"], p["max_targets"]
    out = dict(profile=np.zeros((F, nr)), tgt_range_idx=np.zeros((F, M), np.int32), tgt_range_mag=np.zeros((F, M)),
               tgt_doppler_idx=np.zeros((F, M), np.int32), tgt_count=np.zeros(F, np.int32), slow_mag=np.zeros((F, C)),
               cube=np.zeros((F, C, nr), np.complex128), rd=np.zeros((F, nr, nd), np.complex128), probe=None)
    rows = np.nonzero([(mask >> (r // 128)) & 1 for r in range(nr)])[0]
    for f in range(F):
        X = O.fast_time(iq[f].astype(np.complex128).T, cal, p["if_scale"], wr, nr)        # [nr][C]
        rd = O.doppler_all_rows(X, wd, nd)
        if len(rows):
            slot = X[rows] - X[rows, :1]
            slot[:, 0] = X[rows, 0]
            slot = SR.fp16_round(slot, 1.0 / nr)
            x0 = slot[:, :1].copy()
            slot[:, 0] = 0.0                                                              # X'_0 = 0
            X = X.copy()
            X[rows] = slot + x0
            rd[rows] = O.doppler_all_rows(slot, wd, nd)
        if rd_dtype == C32H:
            rd = SR.fp16_round(rd, 1.0 / (nr * nd))
        prof = O.range_profile(X)
        ridx, rmag = O.search_peak(prof, nr, p["range_thr"], M, p["min_d"], p["max_d"], p["dist_per_bin"])
        didx = O.doppler_index(rd, ridx, p["doppler_thr"], p["doppler_fallback_idx"])
        n = len(ridx)
        out["profile"][f] = prof
        out["tgt_count"][f] = n
        out["tgt_range_idx"][f, :n] = ridx
        out["tgt_range_mag"][f, :n] = rmag
        out["tgt_doppler_idx"][f, :n] = didx
        if n > 0:
            out["slow_mag"][f] = np.abs(X[ridx[0] - 1, :])
        out["cube"][f] = X.T
        out["rd"][f] = rd
    if probe_column:
        col = probe_column - 1
        out["probe"] = np.abs(out["cube"][col // C, col % C, :])
    return out


def plain_chain(iq, cal, p, wr, wd, probe_column=0) -> dict:
    pl = O.process_frames(iq, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    pl["wd"] = wd
    if probe_column:
        col = probe_column - 1
        pl["probe"] = np.abs(pl["cube"][col // iq.shape[1], col % iq.shape[1], :])
    return pl


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.abs(a) ** 2)))


def flat_measures(got_rd, got_prof, ref_rd, ref_prof) -> dict:
    """One frame's RD map [nr][nd] and profile [nr] against the reference: element-wise max |d| / rms of
    both, the relative L2 of each group's 32 rows and of each Doppler residue class d = d0 (mod 16)."""
    d = np.asarray(got_rd, np.complex128) - ref_rd
    grp = np.array([rel_l2(np.asarray(got_rd)[GROUP_ROWS[g]], ref_rd[GROUP_ROWS[g]]) for g in range(NGROUPS)])
    res = np.array([rel_l2(np.asarray(got_rd)[:, d0::16], ref_rd[:, d0::16]) for d0 in range(16)])
    return dict(rd_max=float(np.abs(d).max()) / rms(ref_rd), group=grp, residue=res,
                prof_max=float(np.abs(np.asarray(got_prof, np.float64) - ref_prof).max()) / rms(ref_prof))


def energy_shares(rd) -> tuple:
    """(lowest group rms, lowest Doppler column rms) of one RD map over the map's rms."""
    a = np.abs(rd) ** 2
    tot = np.sqrt(a.mean())
    return (float(min(np.sqrt(a[GROUP_ROWS[g]].mean()) for g in range(NGROUPS)) / tot),
            float(np.sqrt(a.mean(axis=0)).min() / tot))


def group_e_ref(emu_rd, plain_rd) -> np.ndarray:
    """[F][32]: e_ref of the RD map per group."""
    return np.array([[rel_l2(emu_rd[f][GROUP_ROWS[g]], plain_rd[f][GROUP_ROWS[g]]) for g in range(NGROUPS)]
                     for f in range(len(plain_rd))])


def block_e_ref(emu, plain, key) -> np.ndarray:
    """[F][8]: e_ref of the RD map's rows ('rd') or of the profile ('profile') per 128-bin block."""
    F = len(plain[key])
    return np.array([[rel_l2(emu[key][f][128 * b:128 * b + 128], plain[key][f][128 * b:128 * b + 128]) for b in range(NR // 128)]
                     for f in range(F)])


PER_FRAME = ("profile", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "tgt_count", "slow_mag", "cube", "rd")


def _head(chain: dict, F: int, probe_column: int) -> dict:
    """The first F frames of a chain's per-frame arrays, with the probe column of that batch."""
    out = {k: chain[k][:F] for k in PER_FRAME}
    out["probe"] = None
    if probe_column:
        col = probe_column - 1
        out["probe"] = np.abs(out["cube"][col // PN, col % PN, :])
    return out


class Ref:
    """One batch: the input as the device holds it, the plain chain, and the emulated chain per
    (mask, rd_dtype).  Shared among tests and never modified by one."""

    def __init__(self, nts, names, iq, in_dtype=C64, probe_column=0, taps="plain", **over):
        self.nts, self.names, self.taps = nts, list(names), taps
        self.cfg, self.p, self.wr, self.wd, self.cal = build_case(nts, taps, **over)
        self.F = iq.shape[0]
        self.probe_column = probe_column
        self.dev_iq, self.iq = SR.iq_as_stored(iq, in_dtype)
        self.plain = plain_chain(self.iq, self.cal, self.p, self.wr, self.wd, probe_column)
        self.mask = mask_of(self.cfg)
        self._emu, self._whole = {}, None

    def prefix(self, F, probe_column=0) -> "Ref":
        """The first F frames as a batch of their own.  Nothing of either chain crosses frames, so a
        frame's reference is the same in every batch that holds it: the whole batch's is sliced."""
        r = copy.copy(self)
        r.names, r.F, r.probe_column = self.names[:F], F, probe_column
        r.dev_iq, r.iq = self.dev_iq[:F], self.iq[:F]
        r.plain = _head(self.plain, F, probe_column)
        r.plain["wd"] = self.wd
        r._emu, r._whole = {}, self
        return r

    def index(self, name) -> int:
        return self.names.index(name)

    def flat(self) -> list:
        return [f for f, n in enumerate(self.names) if is_flat(n)]

    def emu(self, mask=0, rd_dtype=C64) -> dict:
        key = (mask, rd_dtype)
        if key not in self._emu:
            if self._whole is not None:
                e = _head(self._whole.emu(mask, rd_dtype), self.F, self.probe_column)
            else:
                e = emulate_xcd(self.iq, self.cal, self.p, self.wr, self.wd, mask, rd_dtype, self.probe_column)
            e["e_ref"] = SR.errors(e, self.plain)
            self._emu[key] = e
        return self._emu[key]

    def ambiguous(self, tol) -> np.ndarray:
        """[F]: frames whose peak decision the oracle itself leaves within tol (detect_reference)."""
        M = self.cfg.max_targets
        return np.array([DR.frame_ambiguous(self.plain["profile"][f], self.p, M, tol) for f in range(self.F)])

    def doppler_mask(self, mask, rd_dtype) -> np.ndarray:
        """[F][M]: where tgt_doppler_idx is held exactly (streams_reference.Ref.doppler_mask)."""
        e = self.emu(mask, rd_dtype)
        used = np.arange(self.plain["tgt_range_idx"].shape[1])[None, :] < self.plain["tgt_count"][:, None]
        return used & (e["tgt_doppler_idx"] == self.plain["tgt_doppler_idx"]) & SR.row_gap_ok(self.plain)


_refs = {}


def ref(nts, in_dtype=C64, taps="plain") -> Ref:
    """frames(nts) with its probe column on hot chirp 9 (a chirp of member 1, wave 1); on hot chirp 255
    where the batch has no hot9 (the `ends` taps)."""
    key = ("nts", nts, in_dtype, taps)
    if key not in _refs:
        names, iq = frames(nts, taps)
        c = 9 if "hot9" in names else 255
        _refs[key] = Ref(nts, names, iq, in_dtype, probe_column=names.index(f"hot{c}") * PN + c + 1, taps=taps)
    return _refs[key]


MASK_FRAMES = ("white", "synth_target", "hot0", "hot9")


def mask_ref(mask: int) -> Ref:
    """The four frames of the hand-off mask test at nts 1024 under the gate MASK_GATES[mask], c32h input."""
    key = ("mask", mask)
    if key not in _refs:
        names, iq = frames(1024)
        sel = [names.index(n) for n in MASK_FRAMES]
        _refs[key] = Ref(1024, MASK_FRAMES, iq[sel], C32H, **MASK_GATES[mask])
    return _refs[key]


def count_frames(F: int) -> tuple:
    """(names, iq): F distinct frames at nts 1024, white and synthetic alternating."""
    _, p, *_ = build_case(1024)
    names, out = [], []
    for f in range(F):
        if f % 2 == 0:
            names.append(f"white{f}")
            out.append(white(1024, 100 + f).astype(np.complex64))
        else:
            names.append(f"synth{f}")
            out.append(O.synth_frames(1, PN, 1024, NR, ND, p["dist_per_bin"], frame0=100 + f)[0])
    return names, np.stack(out)


def count_ref(F: int, in_dtype=C64) -> Ref:
    """The first F of count_frames(max F), the probe on the last chirp of the last frame; the frame counts
    of one storage share one reference."""
    key, whole = ("count", F, in_dtype), ("count", 0, in_dtype)
    if key not in _refs:
        if whole not in _refs:
            n = max(FRAME_COUNTS if in_dtype == C64 else FRAME_COUNTS_FP16)
            _refs[whole] = Ref(1024, *count_frames(n), in_dtype)
        _refs[key] = _refs[whole].prefix(F, probe_column=F * PN)
    return _refs[key]


def fp16_left_out(nts: int, name: str, taps="plain") -> bool:
    """Whether frame `name` of a batch at nts is left out of the c32h RD comparison (FP16_X0_LEFT_OUT,
    FP16_HOT_LEFT_OUT): its e_ref there is above E_REF_MAX.  Every other frame, the one-hot frames up to
    nts 128 among them, is held at bound(e_ref) per frame and per group; a frame left out still runs, and
    its profile, slow rows, magnitudes and detections are held like everyone's."""
    x0, hot = (FP16_X0_LEFT_OUT, FP16_HOT_LEFT_OUT) if taps == "plain" else TC.FP16_LEFT_OUT[taps]
    if name == "white_x0":
        return nts in x0
    return name.startswith("hot") and nts in hot

