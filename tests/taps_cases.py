"""Tap families for the range/Doppler chain (k_rdx, k_range, k_doppler, k_detect, k_detect_1p, k_probe);
test-side numpy code, no GPU.  tests/test_taps_cases_host.py proves on the oracle alone what
tests/test_gpu_taps.py relies on.

fmcw_set_taps takes any range window, any Doppler window and any calibration vector.  The taps every
other test runs (oracle.windows, oracle.synth_cal) are exactly symmetric, zero at both ends of the range
window, and one smooth calibration tone: a reversed tap index, a dropped end sample or a stale
calibration sum moves no output above a bar.  The families here have none of these properties.

  plain   oracle.windows and oracle.synth_cal, as the oracle returns them (the other tests' taps, unrounded)
  tilt    a usable window, asymmetric, non-zero at both ends
  rand    U[0.5, 2.0) per tap: no index permutation leaves it in place
  ends    only the first two and last two samples (chirps) that reach the FFT carry weight, and one tap
          just beyond the FFT's truncation, which must reach nothing

Every non-plain family shares one calibration vector of varying modulus, non-linear phase and non-zero
mean.  Non-plain taps are float32-exact (complex64-exact), held as float64 (complex128): the oracle and
the device then see the same numbers.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

KINDS = ("plain", "tilt", "rand", "ends")
NEW_KINDS = ("tilt", "rand", "ends")
ENDS_MIN = 5                           # the shortest length `ends` is defined for
ENDS_LO_R, ENDS_HI_R = (1.0, 1.5), (1.75, 2.0)
ENDS_LO_D, ENDS_HI_D = (2.0, 1.75), (1.5, 1.0)
ENDS_BEYOND = 1.25                     # the tap at index min(S, nfft) where the FFT truncates


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _c64(a):
    return np.asarray(a, np.complex128).astype(np.complex64).astype(np.complex128)


def _unit(n: int) -> np.ndarray:
    """k / (n - 1), 0 where n is 1."""
    return np.arange(n) / (n - 1) if n > 1 else np.zeros(n)


def reach(n: int, nfft) -> int:
    """How many of n samples reach an FFT of nfft points (fft(x, nfft) truncates)."""
    return n if nfft is None else min(n, nfft)


def _ends(n: int, nfft, lo, hi) -> np.ndarray:
    if n < ENDS_MIN:
        raise ValueError(f"the ends family needs a length of at least {ENDS_MIN}")
    m = reach(n, nfft)
    w = np.zeros(n)
    w[0], w[1] = lo
    w[m - 2], w[m - 1] = hi            # where m < 4 (Nd 2) the upper pair stands in place of the lower
    if m < n:
        w[m] = ENDS_BEYOND
    return w


def ends_support(n: int, nfft) -> list:
    """The indices inside the FFT where an `ends` window is non-zero."""
    m = reach(n, nfft)
    return sorted({0, 1, m - 2, m - 1})


def cal_vector(nts: int) -> np.ndarray:
    """(0.006 + 0.008 t) exp(2 pi i (0.013 n + 0.2 sin 6 pi t)) + (0.004 - 0.003 i), complex64-exact."""
    n = np.arange(nts)
    t = _unit(nts)
    return _c64((0.006 + 0.008 * t) * np.exp(2j * np.pi * (0.013 * n + 0.2 * np.sin(6 * np.pi * t))) + (0.004 - 0.003j))


def taps(kind: str, nts: int, pn: int, nr=None, nd=None):
    """(wr [nts], wd [pn], cal [nts]) of one family.  nr and nd matter to `ends` only, where they place
    the upper pair and the tap beyond a truncating FFT; None stands for an FFT that does not truncate."""
    if kind == "plain":
        wr, wd = O.windows(nts, pn)
        return wr, wd, O.synth_cal(nts)
    t, c = _unit(nts), _unit(pn)
    if kind == "tilt":
        wr = 2.0 * (0.54 - 0.46 * np.cos(2 * np.pi * t)) * (0.75 + 0.5 * t)
        wd = 2.0 * (0.54 - 0.46 * np.cos(2 * np.pi * c)) * (1.25 - 0.5 * c)
    elif kind == "rand":
        rng = np.random.default_rng([nts, pn, 77])
        wr = rng.uniform(0.5, 2.0, nts)
        wd = rng.uniform(0.5, 2.0, pn)
    elif kind == "ends":
        wr = _ends(nts, nr, ENDS_LO_R, ENDS_HI_R)
        wd = _ends(pn, nd, ENDS_LO_D, ENDS_HI_D)
    else:
        raise ValueError(kind)
    return _f32(wr), _f32(wd), cal_vector(nts)


def cal_of(kind: str, nts: int) -> np.ndarray:
    return O.synth_cal(nts) if kind == "plain" else cal_vector(nts)


def retone(iq: np.ndarray, kind: str) -> np.ndarray:
    """Frames complex64 [..][S] generated about oracle.synth_cal, moved to the family's calibration tone
    (cal - synth_cal added in double, rounded once more to complex64); `plain` frames are returned as
    they are."""
    if kind == "plain":
        return iq
    nts = iq.shape[-1]
    return (iq.astype(np.complex128) + (cal_vector(nts) - O.synth_cal(nts))).astype(np.complex64)


# one-hot frames (family, nts, chirp) of xcd_reference.frames whose first noise draw leaves the batch short of
# what tests/test_taps_cases_host.py asks of its decisions on the oracle: the next draw
RESEED_HOT = {}


# --------------------------------------------------------------------------
# where a float32 evaluation may decide otherwise than the float64 oracle
# --------------------------------------------------------------------------
TOL_DECISION = 1e-5                    # helpers.TOL_FP32_REL_L2: the band the single-pass grid holds its batches clear of


def flagged_frames(r, streams: bool) -> np.ndarray:
    """[F] bool: the frames of a reference batch (streams_reference.Ref or xcd_reference.Ref) left out of the
    exact comparison of count, range index, Doppler index, first magnitude and slow row.

    detect_reference.frame_ambiguous at 1e-5 decides: two of the strongest candidates of the peak rule, or one
    and range_thr, within the band a float32 profile may move.  A streams batch under tilt or rand taps also
    leaves out what streams_reference.near_ties flags (the profile's two largest values anywhere within 1e-3),
    as its plain counterpart asserts none is.  Under `ends` that second rule says nothing about the peak rule:
    four samples reach the range FFT, the profile of a chirp is a trigonometric polynomial of degree 2, and
    where S = Nr its two largest values are the neighbours of one smooth maximum (within (2 pi / Nr)^2 / 2 of
    each other), in every frame."""
    from tests import detect_reference as DR
    from tests.helpers import near_tie_frames
    prof = r.plain["profile"]
    M = r.cfg.max_targets
    out = np.array([DR.frame_ambiguous(prof[f], r.p, M, TOL_DECISION) for f in range(len(prof))])
    if streams and r.taps != "ends":
        out |= near_tie_frames(prof, rtol=1e-3)
    return out


def ambiguous_rows(r) -> np.ndarray:
    """[F][M] bool: the detected rows whose Doppler index the oracle leaves within 1e-5
    (detect_reference.row_ambiguous, with the row's energy before the mean removal): the index there is held
    by the self-consistent rule alone.  A one-hot frame's row is such a row under any real Doppler window:
    with chirp c alone hot, D[d] = X_c (wd[c] e^(-2 pi i c d / Nd) - W[d] / C), W the window's transform, and
    W[-d] = conj W[d] makes |D[d]| = |D[-d]| exactly; the plain window alone puts the maximum at d = 0.  Where
    the maximum lies on a column that is its own mirror (d = 0 or Nd / 2) the magnitude is stationary there, and
    under `ends`, whose transform is smooth, the columns beside it lie within the band."""
    from tests import detect_reference as DR
    pl = r.plain
    F, M = pl["tgt_range_idx"].shape
    nd = pl["rd"].shape[2]
    kf = min(pl["cube"].shape[1], nd)
    out = np.zeros((F, M), bool)
    for f in range(F):
        for j in range(int(pl["tgt_count"][f])):
            row = pl["tgt_range_idx"][f, j] - 1
            pre = float(np.sqrt(nd * np.sum(np.abs(pl["cube"][f, :kf, row] * np.asarray(r.wd)[:kf]) ** 2)))
            out[f, j] = DR.row_ambiguous(pl["rd"][f, row], r.p["doppler_thr"], TOL_DECISION, pre)
    return out


# --------------------------------------------------------------------------
# what tests/test_gpu_taps.py runs
# --------------------------------------------------------------------------
# white_x0's chirp 0 carries 2^k times its noise: the largest k at which the float32 restatement of k_rdx's algebra
# (xcd_reference.choose_k) stays under half the fp32 bar at every nts.  Under the plain taps that is 3; the element-wise
# figure of the RD map at k = 3 is 5.0e-6 under tilt (nts 1000) and 5.2e-6 under rand (nts 1024), 4.0e-6 under plain
# (`ends`, where four chirps reach the Doppler FFT, carries every k tried and keeps the plain 3)
K_X0 = {"tilt": 2, "rand": 2, "ends": 3}
TILT_NTS = (1024, 1000)                # k_rdx under tilt; the forced fix path under rand
K1_KINDS = ("rand", "ends")
# fmcw_range_fft_device with FMCW_K1_CPT set: (geometry of streams_reference.K1_CASES, value)
K1_CPT_CASES = [((16, 512, 16, 16, 3), "1"), ((100, 96, 64, 16, 7), "64")]
# k_rdx under fp16 storage, by family: (nts whose white_x0, nts whose one-hot frames) are left out of the c32h RD
# comparison (xcd_reference.fp16_left_out; test_taps_cases_host asserts exactly these).  white_x0 as under the
# plain taps from nts 510; a one-hot frame's map is wd[c] X_c, which a Doppler tap of 0.5 .. 2 keeps clear of the fp16
# subnormals where the plain window's end taps (1.2e-3) do not; white_x0 at 2^2 (K_X0) is held up to nts 128
FP16_LEFT_OUT = {"rand": ((510, 1000, 1024), ())}
# batches under `ends` in which the oracle leaves more than one frame open (flagged_frames), with their number:
# the four samples that reach the range FFT are not separated by it (test_taps_cases_host says when); at Nr 2048
# every frame with a target is open and only the empty frame is compared exactly
ENDS_OPEN_STREAMS = {(2048, 8, 2048, 2, 3): 3, (2100, 12, 2048, 1024, 3): 3}
ENDS_OPEN_XCD = {512: 3, 514: 5, 1024: 3}
