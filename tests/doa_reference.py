"""The reference of the direction-of-arrival stage, written from the definition in include/fmcw.h
(fmcw_doa_params); test-side code (the library's kernel is csrc/kernels_doa.hip).

  doa_reference  the definition as plain loops, one row after the other.  Every arithmetic operation
                 is one operation on np.float32 scalars (rounded on its own); compares and the
                 minima of step 2 run on the same values as Python floats, which holds every
                 float32 exactly and compares it exactly.  Its bytes are what the device must write.
  row_pool       rows that force the hard cases of the definition.
  HITS           how often each branch of the definition was taken since reset_hits().
Indices are 0-based except the gate, which is 1-based as in the library."""
import collections
import functools

import numpy as np

F32 = np.float32
EDGES, WRAP, INV = 1, 2, 4
OUTS = ("count", "idx", "pow", "sin", "base")

# every branch of the definition (include/fmcw.h)
BRANCHES = (
    "row_flat", "row_not_positive", "row_searched",
    "left_missing_default", "left_missing_edges", "left_wraps", "left_not_lower",
    "right_next", "right_after_flat", "right_missing_default", "right_missing_edges", "right_wraps",
    "right_higher", "flat_then_rises", "flat_top_peak", "peak",
    "base_left_stopped", "base_left_end", "base_left_all_round", "base_right_stopped", "base_right_end",
    "base_right_all_round", "base_left_empty", "base_right_empty", "base_two_sides",
    "drop_not_positive", "drop_min_abs", "drop_min_rel", "drop_min_prom", "kept",
    "on_min_rel", "on_min_prom", "more_than_max_pk", "equal_powers", "unused_slot",
    "neighbour_missing", "inv_reciprocals", "inv_neighbour_not_positive", "den_zero", "not_finite",
    "clamp_hi", "clamp_lo", "delta_right", "delta_left", "seam_right", "seam_left",
)
HITS = collections.Counter()


def reset_hits():
    HITS.clear()


def _hit(name):
    HITS[name] += 1


def gate_rows(nr, r_lo=0, r_hi=0):
    """0-based [g0, g1] inclusive."""
    return (0, nr - 1) if (r_lo, r_hi) == (0, 0) else (r_lo - 1, r_hi - 1)


def is_peak(v, k, flags):
    """Step 1 on the Python floats v."""
    K = len(v)
    if k > 0:
        left = v[k - 1]
    elif flags & WRAP:
        _hit("left_wraps")
        left = v[K - 1]
    elif flags & EDGES:
        _hit("left_missing_edges")
        left = None
    else:
        _hit("left_missing_default")
        return False
    if left is not None and not left < v[k]:
        _hit("left_not_lower")
        return False
    j, steps = k, 0
    while True:                                   # R: the first index right of k whose value differs
        j, steps = j + 1, steps + 1
        if j == K:
            if flags & WRAP:
                _hit("right_wraps")
                j = 0                             # hi > lo: a different value exists
            elif flags & EDGES:
                _hit("right_missing_edges")
                right = None
                break
            else:
                _hit("right_missing_default")
                return False
        if v[j] != v[k]:
            right = v[j]
            break
    _hit("right_next" if steps == 1 else "right_after_flat")
    if right is not None and not right < v[k]:
        _hit("right_higher" if steps == 1 else "flat_then_rises")
        return False
    _hit("peak" if steps == 1 else "flat_top_peak")
    return True


def base_of(v, k, flags):
    """Step 2 on the Python floats v: the larger of the two sides' minima, a zero as +0."""
    K = len(v)
    sides = []
    for step, name in ((-1, "left"), (1, "right")):
        j, seen, m = k, 0, None
        while True:
            j += step
            if j < 0 or j >= K:
                if not flags & WRAP:
                    _hit(f"base_{name}_end")
                    break
                j %= K
            if seen == K - 1:
                _hit(f"base_{name}_all_round")
                break
            if v[j] > v[k]:
                _hit(f"base_{name}_stopped")
                break
            seen += 1
            m = v[j] if m is None or v[j] < m else m
        if m is None:
            _hit(f"base_{name}_empty")
        else:
            sides.append(m)
    if len(sides) == 2:
        _hit("base_two_sides")
    return F32(max(sides)) + F32(0)


def refine(s, u, k, flags):
    """Step 5 on the np.float32 arrays s, u: sin of the written peak k."""
    K = len(s)
    kl, kr = k - 1, k + 1
    if flags & WRAP:
        kl, kr = kl % K, kr % K
    elif kl < 0 or kr >= K:
        _hit("neighbour_missing")
        return u[k]
    lft, c, r = s[kl], s[k], s[kr]
    delta = F32(0)
    ok = True
    if flags & INV:
        if lft > 0 and r > 0:
            _hit("inv_reciprocals")
            lft, c, r = F32(1) / lft, F32(1) / c, F32(1) / r
        else:
            _hit("inv_neighbour_not_positive")
            ok = False
    if ok:
        den = (lft - c) + (r - c)
        num = F32(0.5) * (lft - r)
        if den == 0:
            _hit("den_zero")
        elif not (np.isfinite(den) and np.isfinite(num)):
            _hit("not_finite")
        else:
            # in exact arithmetic |delta| <= 0.5 at a peak; the halving of num rounds when l - r is an odd
            # number of denormal units (0.5f * 3u = 2u over den = 3u gives 2/3), which the clamp bounds
            delta = num / den
    if delta < F32(-0.5):
        _hit("clamp_lo")
        delta = F32(-0.5)
    elif delta > F32(0.5):
        _hit("clamp_hi")
        delta = F32(0.5)
    if delta >= 0:
        _hit("delta_right")
        if kr < k:
            _hit("seam_right")
            return u[k] + delta * (u[k] - u[kl])
        return u[k] + delta * (u[kr] - u[k])
    _hit("delta_left")
    if kl > k:
        _hit("seam_left")
        return u[k] + delta * (u[kr] - u[k])
    return u[k] + delta * (u[k] - u[kl])


def row_reference(s, u, max_pk, flags, min_abs, min_rel, min_prom):
    """One row: (count, idx [max_pk], pow, sin, base)."""
    s = np.asarray(s, F32)
    u = np.asarray(u, F32)
    v = s.tolist()
    K = len(v)
    idx = np.full(max_pk, -1, np.int32)
    out = [np.zeros(max_pk, F32) for _ in range(3)]
    hi, lo = max(v), min(v)
    if not hi > lo:
        _hit("row_flat")
        return 0, idx, *out
    if not hi > 0:
        _hit("row_not_positive")
        return 0, idx, *out
    _hit("row_searched")
    t_rel = F32(min_rel) * F32(hi)
    kept = []
    for k in range(K):
        if not is_peak(v, k, flags):
            continue
        base = base_of(v, k, flags)
        t_prom = F32(min_prom) * base
        if not v[k] > 0:
            _hit("drop_not_positive")
        elif not s[k] >= F32(min_abs):
            _hit("drop_min_abs")
        elif not s[k] >= t_rel:
            _hit("drop_min_rel")
        elif not s[k] >= t_prom:
            _hit("drop_min_prom")
        else:
            _hit("kept")
            if min_rel > 0 and s[k] == t_rel:
                _hit("on_min_rel")
            if min_prom > 0 and s[k] == t_prom:
                _hit("on_min_prom")
            kept.append((-v[k], k, base))
    kept.sort()
    if len(kept) > max_pk:
        _hit("more_than_max_pk")
    if any(a[0] == b[0] for a, b in zip(kept, kept[1:])):
        _hit("equal_powers")
    if len(kept) < max_pk:
        _hit("unused_slot")
    for i, (_, k, base) in enumerate(kept[:max_pk]):
        idx[i] = k
        out[0][i] = s[k]
        out[1][i] = refine(s, u, k, flags)
        out[2][i] = base
    return len(kept), idx, *out


def doa_reference(spec, sin_theta, max_pk, flags=0, min_abs=0.0, min_rel=0.0, min_prom=0.0, r_lo=0, r_hi=0):
    """spec float32 [F][nr][K], sin_theta float32 [K] -> dict(count int32 [F][nr], idx int32
    [F][nr][max_pk], pow, sin, base float32 [F][nr][max_pk]).  Unused slots and rows outside the gate:
    idx -1, floats +0, count 0."""
    spec = np.ascontiguousarray(spec, F32)
    u = np.ascontiguousarray(sin_theta, F32)
    F, nr, K = spec.shape
    assert u.shape == (K,)
    g0, g1 = gate_rows(nr, r_lo, r_hi)
    res = {"count": np.zeros((F, nr), np.int32), "idx": np.full((F, nr, max_pk), -1, np.int32),
           "pow": np.zeros((F, nr, max_pk), F32), "sin": np.zeros((F, nr, max_pk), F32),
           "base": np.zeros((F, nr, max_pk), F32)}
    with np.errstate(all="ignore"):
        for f in range(F):
            for r in range(g0, g1 + 1):
                n, idx, pw, sn, bs = row_reference(spec[f, r], u, max_pk, flags, F32(min_abs), F32(min_rel), F32(min_prom))
                res["count"][f, r] = n
                res["idx"][f, r], res["pow"][f, r], res["sin"][f, r], res["base"][f, r] = idx, pw, sn, bs
    return res


def idx_set(out, f, r):
    """The grid points of row (f, r)'s written peaks."""
    return {int(k) for k in out["idx"][f, r] if k >= 0}


def assert_same_bytes(got, ref, name=""):
    for k in OUTS:
        if got.get(k) is None:
            continue
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint32).reshape(-1) != w.view(np.uint32).reshape(-1))
            i = bad[0]
            raise AssertionError(f"{name} {k}: {bad.size} of {g.size} values differ, the first at {i}: "
                                 f"{g.reshape(-1)[i]!r} for {w.reshape(-1)[i]!r}")


# ---- the grid and the rows that force the hard cases --------------------------------------------------
def grid(K, seed=0):
    """A strictly ascending float32 grid in [-1, 1] with uneven steps (the two steps beside a point
    differ, so a wrong side in step 5 shows)."""
    if K == 1:
        return np.zeros(1, F32)
    rng = np.random.default_rng(1000 + K + seed)
    w = rng.uniform(0.5, 1.5, K - 1)
    x = np.concatenate([[0.0], np.cumsum(w)])
    return (2.0 * x / x[-1] - 1.0).astype(F32)


DEN = float(np.finfo(F32).smallest_subnormal)


def _below(x):
    return np.nextafter(F32(x), F32(-np.inf))


def _recip_tie():
    """A float32 c in (1, 2) whose reciprocal rounds to the reciprocal of the float just below it."""
    c = F32(1.9)
    while F32(1) / c != F32(1) / _below(c):
        c = np.nextafter(c, F32(2))
    return c


RECIP_TIE = _recip_tie()
TINY = float(np.finfo(F32).tiny)                   # 2^-126, the smallest normal number
HUGE = F32(2.0 ** 127)                             # its reciprocal is the denormal 2^-127 = 2^22 u, exactly


def _huge_with_reciprocal(units):
    """A float32 below HUGE whose reciprocal rounds to 1 / HUGE + units u."""
    with np.errstate(all="ignore"):
        want = F32(1) / HUGE + F32(units * DEN)
        x = F32(1.0 / float(want))
        assert F32(1) / x == want and x < HUGE
    return x


with np.errstate(all="ignore"):
    assert F32(1) / _below(HUGE) == F32(1) / HUGE
HUGE_3U = _huge_with_reciprocal(3)
HUGE_LOW = _huge_with_reciprocal(64)               # the level of the rest of such a row


@functools.lru_cache(maxsize=None)
def row_pool(K, seed=0):
    """float32 [n][K], read only: the rows the issue lists, as far as K allows them, then seeded
    rows of a few levels (ties, flat tops, flat stretches that rise) and of continuous values."""
    rng = np.random.default_rng(77 * K + seed)
    rows = []

    def add(x):
        x = np.asarray(x, np.float64)
        assert x.shape == (K,)
        rows.append(x.astype(F32))

    for levels in (3, 4, 5):
        for _ in range(3):
            add(rng.integers(0, levels, K) * 0.5 + 0.5)
    add(rng.integers(-2, 2, K) * 1.0)                                   # levels around zero: peaks that are not positive
    add(np.arange(K) + 1.0)                                             # strictly monotone, both ways
    add(K - np.arange(K) + 0.0)
    add(np.full(K, 2.5))                                                # constant, zero, negative
    add(np.zeros(K))
    add(-1.0 - rng.uniform(0, 1, K))
    for at in ((0,), (K - 1,), (0, K - 1)):                             # single spikes at the ends
        x = np.ones(K)
        x[list(at)] = 9.0
        add(x)
    if K >= 4:
        x = 1.0 + rng.uniform(0, 1, K)                                  # the maximum on the seam, flat across it
        x[[K - 1, 0]] = 7.0
        add(x)
        x = 1.0 + rng.uniform(0, 1, K)                                  # ... a flat top of three across the seam
        x[[K - 2, K - 1, 0]] = 7.0
        add(x)
        x = np.ones(K)                                                  # flat top in the middle; flat stretch that rises
        x[1:3] = 4.0
        add(x)
        x = np.ones(K)
        x[1:3] = 4.0
        x[3:] = 6.0
        x[K - 1] = 5.0
        add(x)
        x = np.ones(K)                                                  # a flat top that runs into the end
        x[K - 2:] = 3.0
        add(x)
    x = np.ones(K)                                                      # more peaks than max_pk, equal powers
    x[1::2] = 5.0
    add(x)
    x = 1.0 + rng.uniform(0, 0.25, K)
    x[1::2] = 5.0 + rng.integers(0, 2, len(x[1::2]))
    add(x)
    if K >= 3:
        x = np.ones(K)                                                  # l == r: num = 0
        x[K // 2] = 4.0
        add(x)
        x = np.full(K, float(_below(RECIP_TIE)))                        # l == r one step below c, all three with
        x[K // 2] = float(RECIP_TIE)                                    # one reciprocal: den = 0 under INV
        add(x)
        x = np.ones(K) * 2.0                                            # denormal neighbours: the reciprocal is infinite
        x[K // 2] = 8.0
        x[K // 2 - 1] = DEN
        if K // 2 + 1 < K:
            x[K // 2 + 1] = DEN * 3
        add(x)
        x = np.ones(K) * 2.0                                            # one denormal neighbour only
        x[K // 2] = 8.0
        x[K // 2 - 1] = DEN
        add(x)
        x = np.ones(K) * 2.0                                            # a zero and a negative neighbour
        x[K // 2] = 8.0
        x[K // 2 - 1] = 0.0
        add(x)
        x = np.ones(K) * 2.0
        x[K // 2] = 8.0
        if K // 2 + 1 < K:
            x[K // 2 + 1] = -3.0
        add(x)
        x = np.full(K, 3e38)                                            # differences that overflow: den is not finite
        x[K // 2] = 3.2e38
        x[K // 2 - 1] = -3e38
        add(x)
    if K >= 3:
        # the clamp of step 5: a flat top three denormal units above its left neighbour: den = -3u,
        # num = fl(0.5 * -3u) = -2u, delta = 2/3 (over zero and over the smallest normal number)
        for m in (0.0, TINY):
            x = np.full(K, m)
            x[K // 2] = m + 3 * DEN
            if K // 2 + 1 < K:
                x[K // 2 + 1] = m + 3 * DEN
            add(x)
        # ... and under INV, where the reciprocals of huge values are denormal: 1/l == 1/c and
        # 1/r == 1/c + 3u (delta = -2/3), and the mirror image (delta = +2/3)
        for mirror in (False, True):
            x = np.full(K, float(HUGE_LOW))
            x[K // 2] = float(HUGE)
            near, far = K // 2 - 1, K // 2 + 1
            if mirror:
                near, far = far, near
            if 0 <= near < K:
                x[near] = float(_below(HUGE))
            if 0 <= far < K:
                x[far] = float(HUGE_3U)
            add(x)
    # thresholds landing exactly on a peak: with min_rel = 0.25 and min_prom = 4 (exact in float32), a
    # peak of 2 under a maximum of 8 over a base of 0.5
    x = np.full(K, 0.5)
    if K >= 7:
        x[1], x[3], x[5] = 8.0, 2.0, 1.75
    add(x)
    for _ in range(4):
        add(rng.uniform(0.01, 1.0, K) ** 4)
    add(rng.standard_normal(K))
    out = np.stack(rows)
    out.setflags(write=False)
    return out


def pool_spec(K, nr=16, F=1, seed=0):
    """float32 [F][nr][K]: the pool's rows, in a seeded order, then seeded random rows to fill F nr."""
    P = row_pool(K, seed)
    rng = np.random.default_rng(5 * K + nr + F + seed)
    n = F * nr
    pick = rng.permutation(len(P))[:n]
    rows = [P[i] for i in pick]
    while len(rows) < n:
        rows.append((rng.uniform(0.01, 1.0, K) ** 3).astype(F32))
    return np.ascontiguousarray(np.stack(rows).reshape(F, nr, K))


# ---- the off-grid scenario: ra_reference.scene's construction with sources between grid points ------------
OFFGRID_POINTS = (32.25, 37.5)          # a quarter and a half step off a grid point: sin(theta) = 0.0078125, 0.171875


@functools.lru_cache(maxsize=None)
def offgrid_scene(seed=1):
    """ra_reference.scene with the two sources at OFFGRID_POINTS of the 65-point grid."""
    from tests import ra_reference as R
    S = R.SCENE
    rng = np.random.default_rng(seed)
    chans = []
    ph = rng.uniform(-np.pi, np.pi, (S["frames"], 2))
    for a in range(S["A"]):
        z = (rng.standard_normal((S["frames"], S["nr"], S["nd"])) + 1j * rng.standard_normal((S["frames"], S["nr"], S["nd"]))) \
            * np.sqrt(0.5)
        for s, (d, k) in enumerate(zip(S["bins"], OFFGRID_POINTS)):
            z[:, S["row"], d] += S["amp"] * np.exp(1j * (2 * np.pi * S["spacing"] * a * ((k - 32) / 32.0) + ph[:, s]))
        chans.append(R.store(z, False))
    for c in chans:
        c.setflags(write=False)
    return chans


def direction_errors(out, u, f, r, truths):
    """Per true direction: (|sin - truth|, |u[idx] - truth|) of the written peak whose grid point is
    nearest to it."""
    res = []
    n = min(int(out["count"][f, r]), out["idx"].shape[2])
    for t in truths:
        i = min(range(n), key=lambda j: abs(float(u[out["idx"][f, r, j]]) - t))
        res.append((abs(float(out["sin"][f, r, i]) - t), abs(float(u[out["idx"][f, r, i]]) - t)))
    return res
