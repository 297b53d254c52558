"""The reference of the channel-combining stage, written from the definition in include/fmcw.h
(fmcw_beam_params): every intermediate is a float32 numpy array operation, which numpy rounds on its
own, the sums run sequentially in ascending channel order, and astype(float16) rounds to nearest even
with subnormals kept and overflow to inf.  Also a float64 evaluation with the rounding bounds derived
below, steer() (the weights of fmcw_beam_steer, in float64 with the same quarter-turn reduction), and
the input pools of the GPU tests.

Rounding bounds, u = 2^-24, T_a = |x_a| |w_a|, S = sum T_a:
  coherent  each component of t_a is two rounded products and one rounded difference of terms whose
            magnitudes sum to at most T_a (Cauchy-Schwarz): error <= 2 u T_a to first order.  The
            sequential sum adds A - 1 roundings of partial sums of magnitude <= S: (A - 1) u S.  So a
            component of y is within (A + 1) u S to first order; COH_C = 2 covers the u^2 terms:
            |y32 - y64| <= (A + COH_C) u S (+ a few float32 subnormal steps where products underflow).
  NCI       |t^|^2 against |t|^2 = T_a^2: the component errors 2 u T_a give 4 sqrt(2) u T_a^2, the two
            squares and their sum 2 u T_a^2 more: below 8 u T_a^2.  The sum over a adds
            (A - 1) u sum T_a^2, the correctly rounded root gives re^2 = p (1 + d)^2, |d| <= u: 2 u p.
            So |re^2 - sum |t_a|^2| <= (A + NCI_C) u sum T_a^2 with NCI_C = 11 (one spare for u^2)."""
import functools
import math

import numpy as np

from tests.mti_reference import as_floats

U = 2.0 ** -24
COH_C = 2
NCI_C = 11
TINY = 2.0 ** -140          # float32 products that underflow lose absolute, not relative, accuracy


def weights_f32(w):
    """complex [B][A] -> float32 [B][A][2], the values the C struct carries."""
    w = np.asarray(w)
    if w.dtype != np.float32:
        w = np.ascontiguousarray(w.astype(np.complex64)).view(np.float32).reshape(w.shape + (2,))
    return w


def _terms(xs, wb, dt):
    """t_a of one beam for all channels: lists of (re, im) arrays in dtype dt."""
    out = []
    for x, w in zip(xs, wb):
        xr, xi = x[..., 0].astype(dt), x[..., 1].astype(dt)
        wr, wi = dt(w[0]), dt(w[1])
        out.append((xr * wr - xi * wi, xr * wi + xi * wr))
    return out


def combine(xs, w, nci=False, dt=np.float32, order="seq", fused=False):
    """The definition over float arrays xs[a] [...][2] with w float32 [B][A][2]: float array
    [B][...][2] in dtype dt, before any narrowing.  order "tree" sums pairwise, fused emulates a
    single-rounded multiply-add through float64 (both only to show that the pools can tell)."""
    A = len(xs)
    outs = []

    def total(ts):
        if order == "seq":
            acc = ts[0]
            for t in ts[1:]:
                acc = acc + t
            return acc
        if len(ts) == 1:
            return ts[0]
        m = len(ts) // 2
        return total(ts[:m]) + total(ts[m:])
    with np.errstate(all="ignore"):
        for wb in w[:1] if nci else w:
            if fused:
                d = np.float64
                ts = []
                for x, ww in zip(xs, wb[:A]):
                    xr, xi = x[..., 0].astype(np.float32), x[..., 1].astype(np.float32)
                    wr, wi = np.float32(ww[0]), np.float32(ww[1])
                    pr, pi = xi * wi, xi * wr                                   # rounded products
                    ts.append(((xr.astype(d) * d(wr) - pr.astype(d)).astype(np.float32),     # fma(xr, wr, -pr)
                               (xr.astype(d) * d(wi) + pi.astype(d)).astype(np.float32)))
            else:
                ts = _terms(xs, wb[:A], dt)
            if nci:
                ms = [tr * tr + ti * ti for tr, ti in ts]
                p = total(ms)
                y = np.stack([np.sqrt(p), np.zeros_like(p)], axis=-1)
            else:
                y = np.stack([total([t[0] for t in ts]), total([t[1] for t in ts])], axis=-1)
            outs.append(y)
    return np.stack(outs)


def narrow(y, half):
    """float32 [...][2] -> the stored form: float16 [...][2], or complex64 [...]."""
    with np.errstate(all="ignore"):
        if half:
            return y.astype(np.float16)
    return np.ascontiguousarray(y).view(np.complex64).reshape(y.shape[:-1])


def reference(rds, w, nci=False, **kw):
    """The B output maps (a list, in the shape and dtype of the inputs) from the A input maps."""
    xs, halves = zip(*(as_floats(rd) for rd in rds))
    assert len(set(halves)) == 1
    y = combine(list(xs), weights_f32(w), nci=nci, **kw)
    return [narrow(yb, halves[0]) for yb in y]


def magnitudes(xs, w, nci=False):
    """float64 [B][...]: S = sum |x_a| |w_a| (coherent), or sum (|x_a| |w_a|)^2 (NCI)."""
    out = []
    for wb in w[:1] if nci else w:
        T = [np.hypot(x[..., 0].astype(np.float64), x[..., 1].astype(np.float64)) * math.hypot(float(ww[0]), float(ww[1]))
             for x, ww in zip(xs, wb)]
        out.append(sum(t * t for t in T) if nci else sum(T))
    return np.stack(out)


def bound(xs, w, nci=False):
    """The bound of the module docstring: float64 [B][...], per component (coherent) or on re^2 (NCI)."""
    A = len(xs)
    return (A + (NCI_C if nci else COH_C)) * U * magnitudes(xs, w, nci) + 8 * A * TINY


def steer(n_chan, sin_theta, spacing=0.5, cal=None, taper=None, normalize=True):
    """fmcw_beam_steer in float64: complex64 [B][A], w[b][a] = cal_a (taper_a / norm)
    exp(-j 2 pi spacing a sin_theta_b), the phase reduced in turns so that whole quarter turns are
    exact, rounded once to float32.  The inputs are taken at their float32 values, as the C call
    receives them."""
    sp = float(np.float32(spacing))
    st = [float(v) for v in np.atleast_1d(np.asarray(sin_theta, np.float32))]
    tp = None if taper is None else [float(v) for v in np.asarray(taper, np.float32)]
    cl = None if cal is None else [complex(v) for v in np.asarray(cal, np.complex64)]
    norm = float(n_chan) if normalize else 1.0
    if tp is not None and normalize:
        norm = 0.0
        for v in tp:
            norm = norm + v
    w = np.zeros((len(st), n_chan, 2), np.float32)
    for b, s in enumerate(st):
        for a in range(n_chan):
            t = -(sp * float(a) * s)
            t = t - float(np.rint(t))
            q4 = 4.0 * t
            k = float(np.rint(q4))
            ang = (q4 - k) * 1.5707963267948966
            c, sn = math.cos(ang), math.sin(ang)
            er, ei = ((c, sn), (0.0 - sn, c), (0.0 - c, 0.0 - sn), (sn, 0.0 - c))[(int(k) + 4) & 3]
            g = (1.0 if tp is None else tp[a]) / norm
            gr = (1.0 if cl is None else cl[a].real) * g
            gi = (0.0 if cl is None else cl[a].imag) * g
            with np.errstate(over="ignore"):
                w[b, a] = np.float32(gr * er - gi * ei), np.float32(gr * ei + gi * er)
    return np.ascontiguousarray(w).view(np.complex64).reshape(len(st), n_chan)


# ---- the variants a wrong kernel could compute -------------------------------------------------------
def variants(A):
    """name -> what to change in reference(): each must change bytes of the output of every pool."""
    v = {"reversed": dict(rev=True), "transposed": dict(tr=True), "conjugated": dict(conj=True), "fused": dict(fused=True)}
    if A >= 3:
        v["tree"] = dict(order="tree")
    return v


def variant_output(xs, w, nci, half, rev=False, tr=False, conj=False, **kw):
    A = len(xs)
    w8 = np.zeros((8, 8, 2), np.float32)
    w8[:w.shape[0], :A] = w
    if tr:
        w8 = np.ascontiguousarray(w8.transpose(1, 0, 2))
    if conj:
        w8 = w8 * np.array([1, -1], np.float32)
    ww = w8[:w.shape[0], :A]
    y = combine(xs[::-1] if rev else xs, ww, nci=nci, **kw)
    with np.errstate(over="ignore"):
        return y.astype(np.float16) if half else y


# ---- the pools of the GPU tests ---------------------------------------------------------------------
def weights(seed, B, A):
    """float32 [B][A][2]: a distinct weight per (beam, channel), magnitudes in [0.8, 1.5], no
    symmetry; w[0][0] = (0.75, -0.625), which the fp16 pool's tie cells rest on."""
    rng = np.random.default_rng(1000 + seed)
    mag = rng.uniform(0.8, 1.5, (B, A))
    ph = rng.uniform(-np.pi, np.pi, (B, A))
    w = np.stack([mag * np.cos(ph), mag * np.sin(ph)], axis=-1).astype(np.float32)
    w[0, 0] = (0.75, -0.625)
    return w


def _random_cells(rng, A, n, scale, half):
    """float [A][n][2] of the storage dtype: normal values over a few binades."""
    v = rng.standard_normal((A, n, 2)) * 4.0 * np.exp2(rng.integers(-3, 4, (A, n, 1))) * scale
    return v.astype(np.float16) if half else v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def pool(seed, A, B, F, nr, nd, half, nci=False):
    """(channels, w): A maps [F][nr][nd] (complex64, or float16 [..][2] scaled by 1 / (nr nd) as
    fmcw_process stores it) and the weights float32 [B][A][2].  Frame 0 starts with planted cells:
    one cell per variant of variants(A) at which that variant changes the stored output (found by a
    seeded search over random cells, which matters in fp16 storage, where a last-bit float32
    difference rarely survives the narrowing), and in fp16 storage cells whose beam-0 result
    overflows to inf, is a subnormal half, or is an exact tie between two halves.
    The arrays are shared between tests: read only."""
    rng = np.random.default_rng(seed)
    w = weights(seed, B, A)
    scale = 1.0 / (nr * nd) if half else 1.0
    n = F * nr * nd
    cells = _random_cells(rng, A, n, scale, half)
    plant = []
    for name, kw in variants(A).items():
        for _ in range(64):
            cand = _random_cells(rng, A, 1 << 14, scale, half)
            xs = [c.astype(np.float32) for c in cand]
            ref = variant_output(xs, w, nci, half)
            alt = variant_output(xs, w, nci, half, **kw)
            hit = np.flatnonzero((ref.view(np.uint16 if half else np.uint32) != alt.view(np.uint16 if half else np.uint32))
                                 .reshape(ref.shape[0], -1, 2).any(axis=(0, 2)))
            if hit.size:
                plant.append(cand[:, hit[0]])
                break
        else:
            raise AssertionError(f"no cell found at which '{name}' changes the output")
    if half:
        w0 = w[0].astype(np.float64)
        unit = np.stack([w0[:, 0], -w0[:, 1]], axis=-1) / np.hypot(w0[:, 0], w0[:, 1])[:, None]    # conj(w) / |w|
        plant.append((60000.0 * unit).astype(np.float16))                                         # t_a = 60000 |w_a| > 0
        for k in range(4):                                                                         # subnormal halves in
            bits = rng.integers(1, 0x20, (A, 2)).astype(np.uint16) | (rng.integers(0, 2, (A, 2)).astype(np.uint16) << 15)
            plant.append(bits.view(np.float16))
        for k in range(4):                               # m odd in [1025, 1365]: 3 m has 12 bits and is odd, a tie
            m = 1025 + 2 * int(rng.integers(0, 170))
            c = np.zeros((A, 2), np.float16)
            c[0, 0] = np.float16(m * 2.0 ** (-14 - k))
            plant.append(c)
    assert len(plant) <= nr * nd
    for i, c in enumerate(plant):
        cells[:, i] = c
    if half:
        chans = [np.ascontiguousarray(cells[a]).reshape(F, nr, nd, 2) for a in range(A)]
    else:
        chans = [np.ascontiguousarray(cells[a]).view(np.complex64).reshape(F, nr, nd) for a in range(A)]
    for c in chans:
        c.setflags(write=False)
    w.setflags(write=False)
    return chans, w


def is_tie(y32):
    """True where a float32 value lies exactly halfway between two neighbouring halves."""
    with np.errstate(all="ignore"):
        h = y32.astype(np.float16)
        hf = h.astype(np.float32)
        other = np.nextafter(h, np.where(y32 > hf, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)).astype(np.float32)
        return (y32 != hf) & np.isfinite(hf) & np.isfinite(other) & ((y32 - hf) == (other - y32))


def subnormal_halves(out):
    u = np.ascontiguousarray(out).view(np.uint16)
    return int((((u & 0x7C00) == 0) & ((u & 0x03FF) != 0)).sum())


def assert_same_maps(got, ref):
    """Byte equality of every map of two lists."""
    assert len(got) == len(ref)
    for b, (g, r) in enumerate(zip(got, ref)):
        g, r = np.ascontiguousarray(g), np.ascontiguousarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, (b, g.dtype, r.dtype, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            ug, ur = g.view(np.uint8).reshape(-1), r.view(np.uint8).reshape(-1)
            bad = np.flatnonzero(ug != ur)
            raise AssertionError(f"beam {b}: {bad.size} bytes differ, the first at byte {bad[0]} of {ug.size}")


# ---- the cases of the GPU parity test: (nr, nd, F, A, B, half, nci) ------------------------------------
AS, BS, FS = (2, 3, 5, 8), (1, 2, 3, 8), (1, 2, 3, 5)


def parity_cases():
    cases = []
    i = 0
    for nr, nd in ((16, 4), (16, 8), (32, 16)):
        for half in (False, True):
            for A in AS:
                for B in BS:
                    cases.append((nr, nd, FS[i % 4], A, B, half, False))
                    i += 1
                cases.append((nr, nd, FS[i % 4], A, 1, half, True))
                i += 1
    for half in (False, True):
        for A, B in ((2, 1), (3, 2), (5, 3), (8, 8)):
            cases.append((256, 32, 2 + (A & 1), A, B, half, False))
        cases.append((256, 32, 2, 8, 1, half, True))
    # the total piece count one step either side of a whole 256-piece block: fp16 frames of 16 x 4 are
    # 16 pieces, complex64 ones 32 (the smallest step there is)
    for F in (15, 16, 17):
        cases.append((16, 4, F, 3, 2, True, False))
    for F in (7, 8, 9):
        cases.append((16, 4, F, 3, 2, False, False))
    # several blocks per frame
    cases += [(1024, 256, 2, 2, 1, False, False), (1024, 256, 2, 3, 2, True, False), (1024, 256, 2, 5, 1, True, True)]
    return cases


def case_id(c):
    nr, nd, F, A, B, half, nci = c
    return f"{nr}x{nd}-F{F}-A{A}-B{B}-{'c32h' if half else 'c64'}{'-nci' if nci else ''}"


def case_seed(c):
    nr, nd, F, A, B, half, nci = c
    return nr * 7 + nd * 3 + F * 101 + A * 11 + B * 13 + (500 if half else 0) + (900 if nci else 0)
