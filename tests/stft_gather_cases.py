"""The cases and inputs of tests/test_gpu_stft_gather.py, shared with tests/test_stft_gather_host.py (which
proves on the CPU the conditions the GPU module relies on), so the two cannot drift.  Test-side code.

The 20-tap STFT runs in five kernel forms (csrc/kernels_stft.hip), each with its own copy of the gather
"sample q < L is slow_mag[frame_list[q / pn]][q % pn], q >= L is d_halo[q - L]" and of the max_seg clip.
A case is a flat signal x of L samples scattered over the rows of a NaN-filled `slow` [nl + 3][pn]
through a frame list that is not sorted and repeats a row, so a wrong frame, a wrong offset or a read
outside the listed samples shows.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from tests import stft_reference as R

FS = 1250.0
WLEN = 20
FLOOR = -80.0
NSEG_MIN = 600          # two full 256-segment tiles and a partial third; nine full 64-segment units and a partial tenth

# form -> (FMCW_STFT_MFMA, FMCW_STFT64_FOLD, nfft values, hops)
FORMS = {"k_stft20": ("0", "0", (64, 100), (1, 3)),
         "k_stft_mfma": ("1", "0", (100,), (1, 3)),
         "k_stft64m": ("1", "0", (64,), (1, 3)),
         "k_stft64f_hop1": ("1", "1", (64,), (1,)),
         "k_stft64f": ("1", "1", (64,), (2, 3, 4))}
# 41 and 47 are the two smallest pn at which k_stft64f's float quotient needs its correction step
PNS = (1, 3, 7, 16, 19, 20, 21, 41, 47, 50, 277, 1000)
HALO_PNS = (16, 41, 256)
HALO_LENS = (0, 7, 19)
N_HALO = WLEN - 1
CLIP_PN = 41
CLIP_MAX_SEG = (1, 63, 64, 65, 255, 256, 257)
BOOST = 10.0

SPIKE = 300.0
SPIKE_MAX_SEG = (1, 65, 257)

Case = namedtuple("Case", "form nfft hop pn win halo_len max_seg spike", defaults=("asym", None, None, False))


def case_id(c: Case) -> str:
    s = f"{c.form}-nfft{c.nfft}-hop{c.hop}-pn{c.pn}"
    if c.win != "asym":
        s += f"-{c.win}"
    if c.halo_len is not None:
        s += f"-halo{c.halo_len}"
    if c.max_seg is not None:
        s += f"-max{c.max_seg}"
    if c.spike:
        s += "-spike"
    return s


def _combos(form):
    _, _, nffts, hops = FORMS[form]
    return [(form, nfft, hop) for nfft in nffts for hop in hops]


GRID = [Case(*fc, pn) for form in FORMS for fc in _combos(form) for pn in PNS]
HANN = [Case(form, FORMS[form][2][-1], FORMS[form][3][0], 41, "hann") for form in FORMS]
HALO = [Case(*fc, pn, "asym", h) for form in FORMS for fc in _combos(form) if fc[2] == 1 for pn in HALO_PNS for h in HALO_LENS]
CLIP = [Case(*fc, CLIP_PN, "asym", None, m) for form in FORMS for fc in _combos(form)
        if fc[2] == 1 or (form == "k_stft64f" and fc[2] == 3) for m in CLIP_MAX_SEG]
# The forms that take max(P) from raw matrix-core results, which hold the segments behind nseg of a partial
# unit or tile too (formed from the samples below the last kept one, zero behind them): the last kept
# sample carries a spike, which the last kept segment sees at tap 19 of the Hann window (0.02) and those
# segments at its middle taps
CLIP_SPIKE = [Case(form, 64, hop, CLIP_PN, "hann", None, m, True)
              for form, hop in (("k_stft64m", 1), ("k_stft64f_hop1", 1), ("k_stft64f", 3)) for m in SPIKE_MAX_SEG]
# the table forms whose bits must agree on the same gathered input: (k_stft_mfma, k_stft20) at nfft 100,
# (k_stft64m, k_stft20) at nfft 64
IDENTITY = [(Case(form, nfft, hop, pn), Case("k_stft20", nfft, hop, pn))
            for form, nfft in (("k_stft_mfma", 100), ("k_stft64m", 64)) for hop in (1, 3) for pn in PNS]


def window(c: Case) -> np.ndarray:
    if c.win == "hann":
        return np.hanning(WLEN + 2)[1:-1].astype(np.float32)
    return R.asym_window(WLEN, c.nfft)


def signal_length(c: Case) -> int:
    return NSEG_MIN * c.hop + WLEN - 1 + c.pn // 2


Inputs = namedtuple("Inputs", "x slow flist L nl halo xh w")


@functools.lru_cache(maxsize=None)
def inputs(pn: int, hop: int, win_key, halo_len, max_seg, spike=False) -> Inputs:
    """x [L] float32 (the flat signal), slow [nl + 3][pn] (NaN wherever no listed sample below L lies),
    flist [nl], halo [19] or None (NaN past halo_len), xh = x with the valid halo appended.  The form and
    nfft play no part: every form reads the same input."""
    L = NSEG_MIN * hop + WLEN - 1 + pn // 2
    nl = -(-L // pn)
    seed = 7919 * pn + 31 * hop
    xf = R.magnitude_signal(nl * pn, seed).reshape(nl, pn)
    xf = xf * (1 + np.arange(nl) % 5)[:, None].astype(np.float32)          # frame j at level 1 + j % 5
    xf = xf.reshape(-1)
    if max_seg is not None:
        # the largest values of the call lie only in clipped segments, some inside the clipped unit and tile
        xf[(max_seg - 1) * hop + WLEN:] *= np.float32(BOOST)
        if spike:
            xf[(max_seg - 1) * hop + WLEN - 1] = np.float32(SPIKE)
    rng = np.random.default_rng(seed + 1)
    while True:
        rows = rng.permutation(nl + 3)[:nl]
        mid = src = None
        if nl >= 3:                      # a row listed twice, never the last one (nl == 2 has no room for it)
            mid, src = nl // 2, nl // 4
            rows[mid] = rows[src]
        if np.any(np.diff(rows) < 0):
            break
    xf = xf.reshape(nl, pn)
    if mid is not None:
        xf[mid] = xf[src]                # the repeated row's samples stand at both places of the signal
    slow = np.full((nl + 3, pn), np.nan, np.float32)
    slow[rows] = xf
    slow[rows[-1], L - (nl - 1) * pn:] = np.nan                             # the last listed row past L
    x = xf.reshape(-1)[:L].copy()
    halo = None
    xh = x
    if halo_len is not None:
        halo = R.magnitude_signal(N_HALO, seed + 2) * np.float32(2)
        halo[halo_len:] = np.nan
        xh = np.concatenate([x, halo[:halo_len]])
    out = Inputs(x, slow, rows.astype(np.int32), L, nl, halo, xh, None)
    for a in (x, slow, out.flist, xh) + (() if halo is None else (halo,)):
        a.setflags(write=False)
    return out


def case_inputs(c: Case) -> Inputs:
    return inputs(c.pn, c.hop, c.win, c.halo_len, c.max_seg, c.spike)._replace(w=window(c))


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """(P float64 [nseg][nb] of the unclipped call, its dB map), computed once per case and shared."""
    i = case_inputs(c)
    P = R.stft_power(i.xh, i.w, WLEN - c.hop, c.nfft, FS)
    db = R.psd_db(P)
    P.setflags(write=False)
    db.setflags(write=False)
    return P, db


# ---------------------------------------------------------------------------------------------------
# k_stft64f's division-free gather (`locate`), replayed in numpy
# ---------------------------------------------------------------------------------------------------
def locate_f32(pn, r0, i):
    """(quotient, remainder, corrected) of (r0 + i) / pn the way k_stft64f takes it: truncate the float32
    product with the float32 reciprocal, then one correction step.  r0, i: integer arrays (broadcast)."""
    pn = int(pn)
    rr = (np.asarray(r0, np.int64) + np.asarray(i, np.int64)).astype(np.uint32)
    inv = np.float32(1.0) / np.float32(pn)
    df = (rr.astype(np.float32) * inv).astype(np.uint32)
    d = (rr - df * np.uint32(pn & 0xFFFFFFFF)).astype(np.int32).astype(np.int64)
    df = df.astype(np.int64)
    lo, hi = d < 0, d >= pn
    df = df - lo + hi
    d = d + lo * pn - hi * pn
    return df, d, lo | hi


def locate_f64(pn, q0):
    """(quotient, remainder, corrected) of q0 / pn from the double reciprocal, one correction step."""
    pn = int(pn)
    q0 = np.asarray(q0, np.int64)
    fq = (q0.astype(np.float64) * (1.0 / np.float64(pn))).astype(np.int64)
    r = q0 - fq * pn
    lo, hi = r < 0, r >= pn
    return fq - lo + hi, r + lo * pn - hi * pn, lo | hi


def units_of(c: Case):
    """(r0 [units], samples per unit) of k_stft64f's 64-segment units on case c's signal."""
    i = case_inputs(c)
    nseg = R.nseg_of(len(i.xh), WLEN, WLEN - c.hop)
    u = np.arange(-(-nseg // 64), dtype=np.int64)
    return (u * 64 * c.hop) % c.pn, 63 * c.hop + WLEN


def zero_filled_unit_power(c: Case) -> np.ndarray:
    """P float64 of the segments max_seg .. the end of their 64-segment unit as the matrix cores of the
    nfft-64 forms hold them under the clip: from the samples the kept segments read, zero behind them."""
    i = case_inputs(c)
    m = c.max_seg
    keep = (m - 1) * c.hop + WLEN
    end = -(-m // 64) * 64
    xz = np.zeros((end - 1) * c.hop + WLEN, np.float32)
    xz[:keep] = i.x[:keep]
    return R.stft_power(xz, i.w, WLEN - c.hop, c.nfft, FS)[m:end]
