"""float32 reference of the 2-D OS-CFAR detector (include/fmcw.h, fmcw_oscfar_params), written from its
definition; test-side code (the library's kernels are csrc/kernels_oscfar.hip).

All indices in here are 0-based; the library's outputs are 1-based.

  P = fl(fl(re re) + fl(im im)) in float32 of the stored value (float16 storage widened and times nr nd);
  training set of (r, d): CA-CFAR's (tests/cfar_reference.py); N(r) cells, N_full in the unclipped window;
  k(r) = 1 + ((rank - 1) (N(r) - 1)) // (N_full - 1)  (1 when N_full = 1);
  detection iff gated and #{x : fl(alpha x) < P} >= k(r), which is P > fl(alpha X_(k));  noise = X_(k).

numpy's float32 operations round every operation on its own, as the definition asks, so nothing is
rounded differently on the device: there are no exempt cells and every comparison is byte equality.
Both forms of the test are evaluated on every cell and asserted equal.
"""
from __future__ import annotations

import numpy as np

OUT_KEYS = ("det_count", "det_range_idx", "det_doppler_idx", "det_power", "det_noise")


def power(rd) -> np.ndarray:
    """P [F][nr][nd] float32 of the values the device is given: complex64 as is, float16
    [F][nr][nd][2] (D / (nr nd)) widened and multiplied by (float)nr (float)nd."""
    rd = np.asarray(rd)
    if rd.dtype == np.float16:
        nr, nd = rd.shape[1:3]
        v = rd.astype(np.float32) * (np.float32(nr) * np.float32(nd))
        re, im = v[..., 0], v[..., 1]
    else:
        assert rd.dtype == np.complex64
        re, im = np.ascontiguousarray(rd.real), np.ascontiguousarray(rd.imag)
    P = re * re + im * im                            # three float32 operations, each rounded
    assert P.dtype == np.float32
    return P


def window_cells(guard, train):
    """(dr, dd) of the full window's training cells."""
    (gr, gd), (tr, td) = guard, train
    Wr, Wd = gr + tr, gd + td
    return [(dr, dd) for dr in range(-Wr, Wr + 1) for dd in range(-Wd, Wd + 1) if not (abs(dr) <= gr and abs(dd) <= gd)]


def rank_of_row(rank, N, n_full):
    """k(r) for the clipped counts N."""
    N = np.asarray(N, np.int64)
    return np.ones_like(N) if n_full == 1 else 1 + ((rank - 1) * (N - 1)) // (n_full - 1)


class OsWindow:
    """The part of the reference that depends on the map and the window alone, made once and shared:
    P and, per frame, the training powers of every cell in ascending order ([N_full][nr][nd] float32,
    +inf where the window is clipped)."""

    def __init__(self, rd, guard, train):
        self.P = power(rd)
        self.guard, self.train = tuple(guard), tuple(train)
        F, nr, nd = self.P.shape
        cells = window_cells(guard, train)
        Wr, Wd = guard[0] + train[0], guard[1] + train[1]
        assert train[0] + train[1] >= 1 and 2 * Wr + 1 <= nr and 2 * Wd + 1 <= nd
        self.n_full = len(cells)
        rows = np.arange(nr)
        self.N = np.zeros(nr, np.int64)
        for dr, _ in cells:
            self.N += (rows + dr >= 0) & (rows + dr < nr)
        self.sorted = []
        for f in range(F):
            p = self.P[f]
            st = np.full((self.n_full, nr, nd), np.inf, np.float32)
            for i, (dr, dd) in enumerate(cells):
                s = np.roll(p, -dd, axis=1)          # s[r][d] = p[r][(d + dd) mod nd]
                if dr >= 0:
                    st[i, : nr - dr] = s[dr:]
                else:
                    st[i, -dr:] = s[: nr + dr]
            st.sort(axis=0)
            st.setflags(write=False)
            self.sorted.append(st)
        self.P.setflags(write=False)

    def decide(self, alpha, rank, r_lo=0, r_hi=0, local_max=False) -> dict:
        """alpha the float32 the device is given; rank in 1..N_full; r_lo..r_hi the 1-based inclusive
        gate (0, 0 = all rows).  Returns det [F][nr][nd] bool, P, noise [F][nr][nd] float32, N, k [nr],
        gated [nr]."""
        assert 1 <= rank <= self.n_full
        P = self.P
        F, nr, nd = P.shape
        a = np.float32(alpha)
        rows = np.arange(nr)
        gated = np.ones(nr, bool) if (r_lo, r_hi) == (0, 0) else (rows >= r_lo - 1) & (rows <= r_hi - 1)
        k = rank_of_row(rank, self.N, self.n_full)
        assert k.min() >= 1 and np.all(k <= self.N)
        det = np.zeros((F, nr, nd), bool)
        noise = np.zeros((F, nr, nd), np.float32)
        for f in range(F):
            p, st = P[f], self.sorted[f]
            # form 1: count the training cells below the cell (the order of the cells does not matter)
            cnt = np.zeros((nr, nd), np.int64)
            for i in range(self.n_full):
                cnt += (a * st[i]) < p
            by_count = cnt >= k[:, None]
            # form 2: the k-th smallest training power, then one compare
            xk = np.take_along_axis(st, (k - 1)[None, :, None].repeat(nd, axis=2), axis=0)[0]
            assert np.isfinite(xk).all() or not np.isfinite(p).all()
            by_sort = p > a * xk
            assert np.array_equal(by_count, by_sort), "the two forms of the OS test disagree"
            d = by_sort & gated[:, None]
            if local_max:
                top = np.ones_like(d)
                for dr in (-1, 0, 1):
                    for dd in (-1, 0, 1):
                        if (dr, dd) == (0, 0):
                            continue
                        s = np.roll(p, -dd, axis=1)
                        nb = np.zeros_like(p)
                        if dr >= 0:
                            nb[: nr - dr] = s[dr:]
                        else:
                            nb[-dr:] = s[: nr + dr]
                        exists = ((rows + dr >= 0) & (rows + dr < nr))[:, None]
                        top &= ~exists | ((p > nb) if (dr, dd) < (0, 0) else (p >= nb))
                d &= top
            det[f], noise[f] = d, xk
        return dict(det=det, P=P, noise=noise, N=self.N, k=k, gated=gated)


def oscfar_reference(rd, guard, train, alpha, rank, r_lo=0, r_hi=0, local_max=False) -> dict:
    return OsWindow(rd, guard, train).decide(alpha, rank, r_lo, r_hi, local_max)


def lists(ref, max_det) -> dict:
    """The library's per-frame outputs from the reference, in its dtypes: counts, the first max_det
    detections in (range, doppler) order with 1-based indices, power and noise; 0 where unused."""
    det = ref["det"]
    F, K = det.shape[0], max_det
    out = dict(det_count=np.zeros(F, np.int32), det_range_idx=np.zeros((F, K), np.int32),
               det_doppler_idx=np.zeros((F, K), np.int32), det_power=np.zeros((F, K), np.float32),
               det_noise=np.zeros((F, K), np.float32))
    for f in range(F):
        r, d = np.nonzero(det[f])                    # row-major: ascending (range, doppler)
        out["det_count"][f] = len(r)
        r, d = r[:K], d[:K]
        n = len(r)
        out["det_range_idx"][f, :n] = r + 1
        out["det_doppler_idx"][f, :n] = d + 1
        out["det_power"][f, :n] = ref["P"][f, r, d]
        out["det_noise"][f, :n] = ref["noise"][f, r, d]
    return out


def assert_bytes(got, ref, max_det, mask=None) -> None:
    """Every output byte of the library against the reference: count, both index lists, det_power,
    det_noise and, when given, the mask."""
    want = lists(ref, max_det)
    for k in OUT_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert got[k].tobytes() == want[k].tobytes(), k
    if mask is not None:
        assert mask.dtype == np.uint8
        np.testing.assert_array_equal(mask, ref["det"].astype(np.uint8))


# ---- the masking scenario: a weak target a few bins from a strong one --------------------------------
SCENE = dict(F=8, nr=64, nd=32, guard=(1, 1), train=(3, 3), rank=54, pfa=1e-4, r0=30, d0=12, strong_db=40.0)
SCENE_SEED = 2


def masking_scene(weak_db, seed=SCENE_SEED) -> np.ndarray:
    """complex64 [8][64][32]: unit-power complex noise, 40 dB targets at (r0, d0) and (r0 + 3, d0 + 2),
    and a target of weak_db at (r0 - 2, d0 + 3): the first strong one lies in its training window."""
    s = SCENE
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((s["F"], s["nr"], s["nd"])) + 1j * rng.standard_normal((s["F"], s["nr"], s["nd"]))) / np.sqrt(2)
    big = 10 ** (s["strong_db"] / 20)
    x[:, s["r0"], s["d0"]] += big
    x[:, s["r0"] + 3, s["d0"] + 2] += big
    x[:, s["r0"] - 2, s["d0"] + 3] += 10 ** (weak_db / 20)
    return x.astype(np.complex64)


def scene_cells():
    s = SCENE
    return dict(strong=[(s["r0"], s["d0"]), (s["r0"] + 3, s["d0"] + 2)], weak=(s["r0"] - 2, s["d0"] + 3))
