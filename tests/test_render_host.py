"""CPU: the checker of the spectrogram picture (oracle/render.py) pinned before the kernel is pinned to it.

1. `pixel_index` is a second restatement of the rules in the header comment of csrc/kernels_render.hip:
   one pixel at a time, in plain Python floats, with the faces, the seam, the fold, the -1e30 floor and
   the clamp spelled out.  It has to agree with the vectorised render_indices index for index.
2. RENDER_CASES are the inputs tests/test_gpu_render.py gives the kernel.  The conditions asserted here,
   on the reference alone, say that those inputs reach the seam, the rows above Nyquist, the bins Q does
   not hold, both outcomes of the depth test and its ties, so the GPU test cannot pass by missing a branch.
3. Three wrong readings of the rules (a face across the seam, `>` for `>=`, a floor of -1e20) each change
   at least one index of those inputs: the same three changes made to the kernel would be seen.
"""
import functools
import math

import numpy as np
import pytest

from oracle import render as R

FMAX, CMIN, CMAX = 150.0, -40.0, 0.0

# (nfft, fs, nq, nseg, W, H, kind)
_ROWS = [
    (64, 200.0, 32, 24, 255, 97),      # seam rows; rows above Nyquist; nq = nb - 1
    (64, 1250.0, 32, 24, 257, 96),     # nq far above the window; W one past a 256-thread block
    (256, 520.0, 72, 40, 256, 120),    # seam at bin 64 = 130 Hz; Q ends at bin 71: bins 72, 73 of the top rows are not held
    (2048, 1250.0, 247, 30, 513, 64),  # the deployed nq rule
]
RENDER_CASES = ([r + (k,) for r in _ROWS for k in ("ridge", "holes")]
                + [_ROWS[1] + ("flat",),
                   (64, 1250.0, 1, 2, 1, 1, "ridge"),       # the smallest legal call
                   (64, 1250.0, 9, 2, 64, 7, "ridge")])     # nseg = 2: every pixel in the one segment pair
MAIN_CASES = [c for c in RENDER_CASES if c[:6] in _ROWS and c[6] != "flat"]


def case_id(case):
    nfft, fs, nq, nseg, W, H, kind = case
    return f"nfft{nfft}-fs{fs:g}-nq{nq}-nseg{nseg}-{W}x{H}-{kind}"


def case_times(case):
    """(t0, dt) of a 20-tap window at hop 1: the spectrogram's T(1) and T(2) - T(1)."""
    fs = case[1]
    return 10.0 / fs, 1.0 / fs


def _tie_segment(nseg, W):
    """The segment after the one whose pixel column lies closest behind a segment boundary (smallest
    fx > 0).  With that segment all zero, zn and zf of the column are both -1e30 * fx exactly (the finite
    vertices are absorbed), so `>=` decides; with a floor of -1e20 they are not absorbed."""
    u = (np.arange(W) + 0.5) * (nseg - 1) / W
    s = np.clip(np.floor(u).astype(int), 0, nseg - 2)
    fx = u - s
    fx[(fx <= 0) | (s < 1)] = 2.0
    return int(s[np.argmin(fx)]) + 1


def make_q(case, seed=0):
    """Q [nseg][nq + 1] float32 of a case (bins 0 .. nq-1, then the Nyquist bin), from a seeded generator."""
    nfft, fs, nq, nseg, W, H, kind = case
    rng = np.random.default_rng([seed, nfft, nq, nseg, W, H])
    nb = nfft // 2 + 1
    if kind == "flat":
        return np.full((nseg, nq + 1), 0.37, np.float32)
    bins = np.concatenate([np.arange(nq), [nb - 1]]).astype(np.float64)
    vb = min(nb - 1.0, FMAX / (fs / nfft))                       # the bins the picture shows
    seg = np.arange(nseg, dtype=np.float64)[:, None]
    centre = vb * (0.5 + 0.4 * np.sin(2 * np.pi * 1.5 * seg / max(nseg, 2) + 0.7))
    width = max(1.0, vb / 6.0)
    Q = 1e-3 * (1.0 + rng.random((nseg, nq + 1))) + np.exp(-0.5 * ((bins[None, :] - centre) / width) ** 2)
    up = (np.arange(nseg) // 2) % 2 == 0                           # DC and Nyquist raised on alternate segment pairs
    Q[up, 0] *= 30.0
    Q[up, nq] *= 30.0
    Q = Q.astype(np.float32)
    if kind == "holes":
        order = rng.permutation(Q.size)                           # 3 % zeros, 0.5 % each NaN, -1 and subnormal
        n0, n1 = math.ceil(0.03 * Q.size), max(2, math.ceil(0.005 * Q.size))
        flat = Q.reshape(-1)
        flat[order[:n0]] = 0.0
        flat[order[n0:n0 + n1]] = np.nan
        flat[order[n0 + n1:n0 + 2 * n1]] = -1.0
        flat[order[n0 + 2 * n1:n0 + 3 * n1]] = np.float32(1e-42)
        Q[_tie_segment(nseg, W)] = 0.0
    return Q


@functools.lru_cache(maxsize=None)
def reference(case, zero_pmax=False):
    """(Q, pmax, t0, dt, indices, details) of a case, computed once and shared read-only."""
    nfft, fs, nq, nseg, W, H, kind = case
    Q = make_q(case)
    pmax = np.float32(0.0) if zero_pmax else np.float32(np.nanmax(Q))
    t0, dt = case_times(case)
    idx, d = R.render_indices(Q, nq, float(pmax), nfft, fs, t0, dt, W, H, details=True)
    for a in (Q, idx, *d.values()):
        a.setflags(write=False)
    return Q, pmax, t0, dt, idx, d


# ---- the scalar restatement ---------------------------------------------------------------------------------
def pixel_index(Q, nq, pmax, nfft, fs, t0, dt, W, H, px, py, *, floor=-1.0e30, seam_face=False, strict=False):
    """Palette index of pixel (px, py).  floor / seam_face / strict are the three wrong readings of (3)."""
    nseg = len(Q)
    if nseg < 2:
        return 0
    nb = nfft // 2 + 1                       # the one-sided axis
    h = nb // 2                              # fftshift rotates it by h: rows run bins nb-h .. nb-1, 0 .. nb-h-1
    last_row_bin = nb - h - 1                # so the surface ends at this bin: no face joins it to the next one
    pm = float(np.float32(pmax))
    inv = 1.0 / pm if pm > 0.0 else 0.0

    def psd(s, b):                           # 20 log10(P / max P) of bin b at segment s, floored
        c = b if b < nq else nq              # Q holds bins 0 .. nq-1 and, in column nq, bin nb-1
        p = float(Q[s][c])
        if not p > 0.0:                      # 0, negative, NaN
            return floor
        r = p * inv
        v = 20.0 * math.log10(r) if r > 0.0 else -math.inf
        return max(v, floor)

    def held(b):
        return b < nq or b == nb - 1

    def face(s, b_lo, b_hi, fy, fx):         # bilinear z over the face between two bins and two segments
        lo = psd(s, b_lo) + (psd(s, b_hi) - psd(s, b_lo)) * fy
        hi = psd(s + 1, b_lo) + (psd(s + 1, b_hi) - psd(s + 1, b_lo)) * fy
        return lo + (hi - lo) * fx

    # the pixel's centre: x over [T(1), T(end)], y over [0, fmax] with the top row at fmax
    t_end = t0 + float(nseg - 1) * dt
    t = t0 + (float(px) + 0.5) * (t_end - t0) / float(W)
    y = FMAX * (1.0 - (float(py) + 0.5) / float(H))
    u = (t - t0) / dt
    s = min(max(int(math.floor(u)), 0), nseg - 2)
    fx = u - float(s)
    df = fs / float(nfft)
    # the fold face from bin nb-1 (y = fs/2) back to bin 0 (y = 0) lies over every y; first vertex: bin nb-1
    z_fold = face(s, 0, nb - 1, y / (fs * 0.5), fx)
    z_shown = psd(s, nb - 1)
    # the ordinary face between bins m and m+1, where the surface has one and Q holds both bins
    my = y / df
    m = int(math.floor(my))
    if m >= 0 and m + 1 <= nb - 1 and (seam_face or m != last_row_bin) and held(m) and held(m + 1):
        z_face = face(s, m, m + 1, my - float(m), fx)
        if (z_face > z_fold) if strict else (z_face >= z_fold):      # seen from +z: the higher one
            z_shown = psd(s, m)                                      # flat shading: first vertex = bin m
    q = (z_shown - CMIN) / (CMAX - CMIN) * 256.0
    if q < 0.0:
        return 0
    if q > 255.0:
        return 255
    return int(math.floor(q))


def restate(Q, nq, pmax, nfft, fs, t0, dt, W, H, **kw):
    Ql = np.asarray(Q, np.float32).tolist()
    return np.array([[pixel_index(Ql, nq, pmax, nfft, fs, t0, dt, W, H, px, py, **kw) for px in range(W)]
                     for py in range(H)], np.uint8).reshape(H, W)


def _crop(case):
    """The case itself when its image is small, else the same Q rendered at 48 x 48."""
    nfft, fs, nq, nseg, W, H, kind = case
    return (W, H) if W <= 64 and H <= 64 else (48, 48)


@pytest.mark.parametrize("zero_pmax", [False, True], ids=["pmax", "pmax0"])
@pytest.mark.parametrize("case", RENDER_CASES, ids=case_id)
def test_scalar_restatement_agrees(case, zero_pmax):
    nfft, fs, nq, nseg, _, _, kind = case
    W, H = _crop(case)
    Q, pmax, t0, dt, idx, _ = reference(case, zero_pmax)
    want = idx if (W, H) == case[4:6] else R.render_indices(Q, nq, float(pmax), nfft, fs, t0, dt, W, H)
    np.testing.assert_array_equal(restate(Q, nq, float(pmax), nfft, fs, t0, dt, W, H), want)
    if zero_pmax:
        assert not want.any()                # P / 0: every vertex on the floor


@pytest.mark.parametrize("nseg", [0, 1])
def test_fewer_than_two_segments_is_an_empty_picture(nseg):
    Q = make_q(RENDER_CASES[0])[:nseg]
    idx, d = R.render_indices(Q, 32, 1.0, 64, 200.0, 0.05, 0.005, 9, 5, details=True)
    assert idx.shape == (5, 9) and not idx.any() and not d["ok"].any() and not d["take"].any()
    assert not restate(Q, 32, 1.0, 64, 200.0, 0.05, 0.005, 9, 5).any()


def test_details_do_not_change_the_indices():
    nfft, fs, nq, nseg, W, H, _ = RENDER_CASES[0]
    Q, pmax, t0, dt, idx, d = reference(RENDER_CASES[0])
    np.testing.assert_array_equal(R.render_indices(Q, nq, float(pmax), nfft, fs, t0, dt, W, H), idx)
    assert sorted(d) == ["c0", "c1", "m", "ok", "take"] and all(v.shape == (H, W) for v in d.values())


# ---- what the cases reach -------------------------------------------------------------------------------------
def test_cases_hold_the_issue_rows():
    assert len(set(RENDER_CASES)) == len(RENDER_CASES)
    for nfft, fs, nq, nseg, W, H, kind in RENDER_CASES:
        assert nfft % 2 == 0 and 1 <= nq <= nfft // 2 and nseg >= 2 and W >= 1 and H >= 1
    assert RENDER_CASES[0][:6] == (64, 200.0, 32, 24, 255, 97) and RENDER_CASES[0][2] == 64 // 2
    n = int(math.floor(FMAX / (1250.0 / 2048))) + 2
    assert (2048, 1250.0, n, 30, 513, 64, "ridge") in RENDER_CASES        # the deployed nq rule


def test_cases_reach_every_branch():
    seam_rows = nyq_rows = absent = 0
    for case in MAIN_CASES:
        nfft, fs, nq = case[:3]
        nb = nfft // 2 + 1
        d = reference(case)[5]
        seam_rows += int(np.all(d["m"] == nb - nb // 2 - 1, axis=1).sum())
        nyq_rows += int(np.all(d["m"] + 1 > nb - 1, axis=1).sum())
        absent += int(((d["c0"] == -1) | (d["c1"] == -1)).sum())
    assert seam_rows >= 1 and nyq_rows >= 1 and absent >= 1, (seam_rows, nyq_rows, absent)


def test_third_row_reaches_bins_q_does_not_hold():
    """nq < nb - 1 there: the top rows read bins past nq, through m + 1 first and then through m."""
    case = next(c for c in MAIN_CASES if c[0] == 256)
    d = reference(case)[5]
    nb = case[0] // 2 + 1
    assert case[2] < nb - 1
    assert np.any((d["c1"] == -1) & (d["c0"] >= 0)) and np.any(d["c0"] == -1)
    assert np.any(np.all(d["m"] == nb - nb // 2 - 1, axis=1))             # and its seam is inside the window


@pytest.mark.parametrize("case", MAIN_CASES, ids=case_id)
def test_depth_test_goes_both_ways(case):
    d = reference(case)[5]
    share = d["take"][d["ok"]].mean()
    assert 0.10 <= share <= 0.90, share


@pytest.mark.parametrize("case", MAIN_CASES, ids=case_id)
def test_pictures_are_not_one_colour(case):
    idx = reference(case)[4]
    if case[6] == "ridge":
        assert len(np.unique(idx)) >= 20
    else:
        assert np.mean(idx == 0) <= 0.70
        Q = reference(case)[0]
        assert np.any(Q == 0) and np.any(np.isnan(Q)) and np.any(Q < 0) and np.any((Q > 0) & (Q < 1e-38))
        assert np.any(np.all(Q == 0, axis=1))


# ---- wrong readings of the rules change the pictures ----------------------------------------------------------
def _rows_of(idx_a, idx_b):
    return np.flatnonzero(np.any(idx_a != idx_b, axis=1))


@pytest.mark.parametrize("wrong", [dict(seam_face=True), dict(strict=True), dict(floor=-1.0e20)],
                         ids=["seam-face", "strict-depth-test", "floor-1e20"])
def test_a_wrong_reading_changes_an_index(wrong):
    """Full-size pictures (the GPU test compares these), restated only on the pixel rows and columns that can
    differ: the seam rows for the face across the seam, the tie column of `holes` for the other two."""
    changed = 0
    for case in MAIN_CASES:
        nfft, fs, nq, nseg, W, H, kind = case
        Q, pmax, t0, dt, idx, d = reference(case)
        Ql = Q.tolist()
        nb = nfft // 2 + 1
        if "seam_face" in wrong:
            pix = [(px, py) for py in np.flatnonzero(np.all(d["m"] == nb - nb // 2 - 1, axis=1)) for px in range(W)]
        elif kind == "holes":
            z = _tie_segment(nseg, W)
            u = (np.arange(W) + 0.5) * (nseg - 1) / W
            pix = [(px, py) for px in np.flatnonzero(np.floor(u).astype(int) == z - 1) for py in range(H)]
        else:
            pix = []
        for px, py in pix:
            right = pixel_index(Ql, nq, float(pmax), nfft, fs, t0, dt, W, H, int(px), int(py))
            assert right == idx[py, px]
            changed += pixel_index(Ql, nq, float(pmax), nfft, fs, t0, dt, W, H, int(px), int(py), **wrong) != right
    assert changed >= 1, changed
