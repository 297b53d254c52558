"""The float32 reference of the frame-to-frame clutter filter, written from the definition in
include/fmcw.h (fmcw_mti_params): one frame step vectorised over the cells, the frames in a Python
loop.  numpy rounds every float32 operation on its own, which is what the definition asks for, and
astype(float16) rounds to nearest even with subnormals kept."""
import numpy as np

RAMP, FREEZE = 1, 2
SEEN_MAX = 1 << 30


def as_floats(rd):
    """rd complex64 [R][nr][nd] or float16 [R][nr][nd][2] -> (float32 [R][nr][nd][2], is_fp16)."""
    rd = np.ascontiguousarray(rd)
    if rd.dtype == np.complex64 and rd.ndim == 3:
        return rd.view(np.float32).reshape(rd.shape + (2,)), False
    if rd.dtype == np.float16 and rd.ndim == 4 and rd.shape[-1] == 2:
        return rd.astype(np.float32), True              # exact
    raise TypeError("rd must be complex64 [R][nr][nd] or float16 [R][nr][nd][2]")


def gain(lam, flags, n):
    """g of a frame that starts with n frames seen (n already clamped)."""
    lam = np.float32(lam)
    if flags & RAMP:
        return np.maximum(lam, np.float32(1) / np.float32(n + 1))
    return lam


def reference(rd, lam, flags, n_seq=1, bg=None, seen=None, want_out=True):
    """dict(out, bg, seen): out in the shape and dtype of rd (None without want_out), bg complex64
    [S][nr][nd], seen int32 [S].  bg / seen None: fresh sequences."""
    x_all, half = as_floats(rd)
    rows, nr, nd = x_all.shape[:3]
    S = int(n_seq)
    assert S >= 1 and rows % S == 0
    F = rows // S
    if bg is None:
        B = np.zeros((S, nr, nd, 2), np.float32)
        n_all = np.zeros(S, np.int32)
    else:
        B = np.array(np.ascontiguousarray(bg, np.complex64).view(np.float32).reshape(S, nr, nd, 2), copy=True)
        n_all = np.array(seen, np.int32, copy=True).reshape(S)
    y_all = np.empty_like(x_all) if want_out else None
    with np.errstate(all="ignore"):
        for s in range(S):
            n = int(min(max(int(n_all[s]), 0), SEEN_MAX))
            for f in range(F):
                x = x_all[s * F + f]
                y = x - B[s]
                if want_out:
                    y_all[s * F + f] = y
                if flags & FREEZE:
                    continue
                g = gain(lam, flags, n)
                if g == np.float32(1):
                    B[s] = x
                else:
                    t = g * y
                    B[s] = B[s] + t
                n = min(n + 1, SEEN_MAX)
            if not flags & FREEZE:
                n_all[s] = n
        out = None
        if want_out:
            out = y_all.astype(np.float16) if half else np.ascontiguousarray(y_all).view(np.complex64).reshape(rows, nr, nd)
    return dict(out=out, bg=np.ascontiguousarray(B).view(np.complex64).reshape(S, nr, nd), seen=n_all)


def assert_same(got, ref, keys=("out", "bg", "seen")):
    """Byte equality of every array named (None must meet None)."""
    for k in keys:
        if ref[k] is None or got[k] is None:
            assert ref[k] is None and got[k] is None, k
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            ua, ub = a.view(np.uint8).reshape(-1), b.view(np.uint8).reshape(-1)
            bad = np.flatnonzero(ua != ub)
            raise AssertionError(f"{k}: {bad.size} bytes differ, the first at byte {bad[0]} of {ua.size}")


def scene(seed, n_seq, F, nr, nd, half, static=4.0, moving=0.5):
    """Finite random frames: a fixed per-cell static part plus a part that changes every frame, so B
    and y have different magnitudes.  fp16 storage: scaled by 1 / (nr nd), as fmcw_process stores it."""
    rng = np.random.default_rng(seed)
    st = (rng.standard_normal((n_seq, 1, nr, nd, 2)) * static).astype(np.float32)
    mv = (rng.standard_normal((n_seq, F, nr, nd, 2)) * moving).astype(np.float32)
    x = (st + mv).reshape(n_seq * F, nr, nd, 2)
    if half:
        return (x * np.float32(1.0 / (nr * nd))).astype(np.float16)
    return np.ascontiguousarray(x).view(np.complex64).reshape(n_seq * F, nr, nd)
