"""The reference of the MUSIC stage, written from the definition in include/fmcw.h
(fmcw_music_params); test-side code (the library's kernel is csrc/kernels_music.hip).

  music_reference   float32, the steps of the header literally: vectorised over rows and directions
                    (numpy rounds every float32 array operation on its own), Python loops over
                    sweeps, p, q, k, j and a only.  Its bytes are what the device must write.
Also the pools of the float64 comparison, the close-pair and the coherent-pair scenarios (built as
ra_reference.scene builds its own) and the cases of the GPU parity tests.
Indices are 0-based except the gate, which is 1-based as in the library."""
import functools

import numpy as np

from tests.ra_reference import F32, SCENE, gate_rows, max_bits, n_tri, scene_sines, store, tri, weights_f32

FB = 1
FLT_MAX = np.finfo(np.float32).max
SWEEPS = 8                 # the default of MusicConfig


def dense(cov, fb=False):
    """cov float32 [rows][T][2] -> the state of step 1: {(a, b): (re, im)} for a <= b, arrays [rows].
    A diagonal entry's im is not read (taken as +0); with fb every entry is first replaced from the
    original by 0.5 (R_ab + R_a'b'), a' = A - 1 - b, b' = A - 1 - a."""
    rows, T = cov.shape[:2]
    A = next(a for a in range(2, 9) if n_tri(a) == T)
    R = {}
    for a in range(A):
        for b in range(a, A):
            t = tri(A, a, b)
            R[a, b] = (cov[:, t, 0].copy(), cov[:, t, 1].copy() if b > a else np.zeros(rows, F32))
    if fb:
        half = F32(0.5)
        R = {(a, b): (half * (R[a, b][0] + R[A - 1 - b, A - 1 - a][0]), half * (R[a, b][1] + R[A - 1 - b, A - 1 - a][1]))
             for (a, b) in R}
        for a in range(A):
            R[a, a] = (R[a, a][0], np.zeros(rows, F32))
    return A, R


def _get(M, k, p):
    """M_kp: the stored upper entry, or the conjugate of its mirror."""
    if k <= p:
        return M[k, p]
    re, im = M[p, k]
    return re, -im


def _put(M, k, p, re, im):
    if k <= p:
        M[k, p] = (re, im)
    else:
        M[p, k] = (re, -im)


def _rot(x, y, c, sr, si):
    """(c x - conj(sp) y, sp x + c y): four real products per complex product, the pair's sum or
    difference rounded, then combined with the c term."""
    xr, xi = x
    yr, yi = y
    nxr = c * xr - (sr * yr + si * yi)
    nxi = c * xi - (sr * yi - si * yr)
    nyr = (sr * xr - si * xi) + c * yr
    nyi = (sr * xi + si * xr) + c * yi
    return (nxr, nxi), (nyr, nyi)


def jacobi(A, M, sweeps, want_off=False):
    """Step 2 on the state M (changed in place).  Returns V {(k, j): (re, im)}."""
    rows = M[0, 0][0].shape[0]
    one, zero = np.ones(rows, F32), np.zeros(rows, F32)
    V = {(k, j): ((one if k == j else zero).copy(), zero.copy()) for k in range(A) for j in range(A)}
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(A - 1):
                for q in range(p + 1, A):
                    hr, hi = M[p, q]
                    g = np.sqrt(hr * hr + hi * hi)
                    on = g != 0                                        # a pair with g == 0 is skipped
                    phr, phi = hr / g, hi / g
                    a, b = M[p, p][0], M[q, q][0]
                    tau = (b - a) / (F32(2) * g)
                    at = np.abs(tau)
                    t = F32(1) / (at + np.sqrt(F32(1) + at * at))
                    t = np.where(tau < 0, -t, t)
                    c = F32(1) / np.sqrt(F32(1) + t * t)
                    s = t * c
                    sr, si = s * phr, s * phi

                    def keep(new, old):
                        return (np.where(on, new[0], old[0]), np.where(on, new[1], old[1]))
                    for k in range(A):
                        if k == p or k == q:
                            continue
                        x, y = _get(M, k, p), _get(M, k, q)
                        nx, ny = _rot(x, y, c, sr, si)
                        nx, ny = keep(nx, x), keep(ny, y)
                        _put(M, k, p, *nx)
                        _put(M, k, q, *ny)
                    tg = t * g
                    M[p, p] = (np.where(on, a - tg, a), M[p, p][1])
                    M[q, q] = (np.where(on, b + tg, b), M[q, q][1])
                    M[p, q] = (np.where(on, F32(0), hr), np.where(on, F32(0), hi))
                    for k in range(A):
                        x, y = V[k, p], V[k, q]
                        nx, ny = _rot(x, y, c, sr, si)
                        V[k, p], V[k, q] = keep(nx, x), keep(ny, y)
    return V


def music_reference(cov, w=None, n_src=0, max_src=1, sweeps=SWEEPS, fb=False, src_thr=4.0, r_lo=0, r_hi=0):
    """cov float32 [F][nr][T][2] (the device's bytes), w float32 [K][A][2] or complex [K][A] or None.
    Returns dict(eval [F][nr][A], evec [F][nr][A][A][2] (evec[j][a]), nsrc int32 [F][nr], music
    [F][nr][K] or None, music_max float32): the header's steps, every operation rounded on its own."""
    cov = np.ascontiguousarray(cov, np.float32)
    F, nr, T = cov.shape[:3]
    rows = F * nr
    A, M = dense(cov.reshape(rows, T, 2), fb)
    V = jacobi(A, M, sweeps)
    lam = np.stack([M[a, a][0] for a in range(A)], axis=1)                 # [rows][A]
    order = np.argsort(lam, axis=1, kind="stable")                          # ties by original index
    ev = np.take_along_axis(lam, order, axis=1)
    Vr = np.stack([np.stack([V[a, j][0] for a in range(A)], axis=1) for j in range(A)], axis=1)   # [rows][j][a]
    Vi = np.stack([np.stack([V[a, j][1] for a in range(A)], axis=1) for j in range(A)], axis=1)
    Er = np.take_along_axis(Vr, order[:, :, None], axis=1)
    Ei = np.take_along_axis(Vi, order[:, :, None], axis=1)
    with np.errstate(all="ignore"):
        if n_src:
            n = np.full(rows, n_src, np.int32)
        else:
            nu = np.zeros(rows, F32)
            for j in range(A - max_src):
                nu = nu + ev[:, j]
            nu = nu / F32(A - max_src)
            thr = F32(src_thr) * nu
            n = np.minimum(max_src, (ev > thr[:, None]).sum(axis=1)).astype(np.int32)
        music = None
        if w is not None:
            w = weights_f32(w)
            K = w.shape[0]
            wr = [w[:, a, 0][None, :] for a in range(A)]
            wi = [w[:, a, 1][None, :] for a in range(A)]
            e = np.zeros((1, K), F32)
            for a in range(A):
                e = e + (wr[a] * wr[a] + wi[a] * wi[a])
            den = np.zeros((rows, K), F32)
            for j in range(A):                                          # j < A - n, n in 0..A-1
                pr, pi = np.zeros((rows, K), F32), np.zeros((rows, K), F32)
                for a in range(A):
                    vr, vi = Er[:, j, a][:, None], Ei[:, j, a][:, None]
                    pr = pr + (wr[a] * vr - wi[a] * vi)
                    pi = pi + (wr[a] * vi + wi[a] * vr)
                den = np.where((j < A - n)[:, None], den + (pr * pr + pi * pi), den)
            music = np.where(den == 0, FLT_MAX, e / den).astype(F32)
            assert music.dtype == np.float32
    g0, g1 = gate_rows(nr, r_lo, r_hi)
    out = dict(eval=ev.reshape(F, nr, A), evec=np.stack([Er, Ei], axis=-1).reshape(F, nr, A, A, 2),
               nsrc=n.reshape(F, nr), music=None if music is None else music.reshape(F, nr, -1))
    for v in out.values():
        if v is not None:
            v[:, :g0] = 0
            v[:, g1 + 1:] = 0
    for k, v in out.items():
        if v is not None:
            out[k] = np.ascontiguousarray(v)
    out["music_max"] = F32(0) if music is None else max_bits(out["music"])
    return out


def full_matrix(cov, fb=False):
    """The complex128 A x A matrices of step 1 from float32 cov [rows][T][2]."""
    A, R = dense(np.ascontiguousarray(cov, np.float32), fb)
    rows = cov.shape[0]
    out = np.zeros((rows, A, A), np.complex128)
    for (a, b), (re, im) in R.items():
        out[:, a, b] = re.astype(np.float64) + 1j * im.astype(np.float64)
        if b > a:
            out[:, b, a] = np.conj(out[:, a, b])
    return out


def pack(Rm):
    """complex [rows][A][A] Hermitian -> float32 cov [rows][T][2]."""
    rows, A = Rm.shape[:2]
    cov = np.zeros((rows, n_tri(A), 2), F32)
    for a in range(A):
        for b in range(a, A):
            cov[:, tri(A, a, b), 0] = Rm[:, a, b].real
            cov[:, tri(A, a, b), 1] = Rm[:, a, b].imag if b > a else 0
    return cov


def outer_sum(x):
    """sum over d of x[:, a, d] conj(x[:, b, d]), snapshot by snapshot (elementwise: the same bits
    on every host, whatever its BLAS)."""
    out = np.zeros(x.shape[:2] + x.shape[1:2], np.complex128)
    for d in range(x.shape[2]):
        out += x[:, :, None, d] * np.conj(x[:, None, :, d])
    return out


# ---- the pools of the float64 comparison -------------------------------------------------------------
POOLS = ("source", "rank2", "near_identity")


@functools.lru_cache(maxsize=None)
def eig_pool(kind, A, rows=1024, seed=7):
    """float32 cov [rows][T][2].  source: nd = 64 snapshots of unit noise plus one source of amplitude
    10^U(-1, 3) from a random direction; rank2: nd = 2 < A snapshots; near_identity: I + 1e-7 R."""
    rng = np.random.default_rng(seed * 100 + A * 10 + POOLS.index(kind))
    nd = 2 if kind == "rank2" else 64
    x = (rng.standard_normal((rows, A, nd)) + 1j * rng.standard_normal((rows, A, nd))) * np.sqrt(0.5)
    if kind == "source":
        amp = 10.0 ** rng.uniform(-1, 3, (rows, 1, 1))
        st = rng.uniform(-1, 1, (rows, 1, 1))
        ph = rng.uniform(-np.pi, np.pi, (rows, 1, nd))
        x = x + amp * np.exp(1j * (np.pi * np.arange(A)[None, :, None] * st + ph))
    Rm = outer_sum(x)
    if kind == "near_identity":
        Rm = np.eye(A)[None] + 1e-7 * Rm
    cov = pack(Rm)
    cov.setflags(write=False)
    return cov


def eig_errors(cov, sweeps=SWEEPS):
    """The reference against numpy.linalg.eigh in float64 on the same float32 matrix: the largest
    |lambda - lambda_ref| / tr, ||R V - V L||_F / tr, ||V^H V - I||_F and off-diagonal norm / tr."""
    cov = np.asarray(cov)
    rows = cov.shape[0]
    A, M = dense(cov)
    V = jacobi(A, M, sweeps)
    off = np.zeros(rows)
    for a in range(A):
        for b in range(a + 1, A):
            off += 2 * (M[a, b][0].astype(np.float64) ** 2 + M[a, b][1].astype(np.float64) ** 2)
    lam = np.stack([M[a, a][0] for a in range(A)], axis=1).astype(np.float64)
    Vc = np.zeros((rows, A, A), np.complex128)
    for (k, j), (re, im) in V.items():
        Vc[:, k, j] = re.astype(np.float64) + 1j * im.astype(np.float64)
    Rm = full_matrix(cov)
    tr = np.einsum("raa->r", Rm).real
    ref = np.linalg.eigvalsh(Rm)
    e_lam = np.abs(np.sort(lam, axis=1) - ref).max(axis=1) / tr
    res = np.linalg.norm(Rm @ Vc - Vc * lam[:, None, :], axis=(1, 2)) / tr
    orth = np.linalg.norm(np.conj(np.swapaxes(Vc, 1, 2)) @ Vc - np.eye(A)[None], axis=(1, 2))
    return float(e_lam.max()), float(res.max()), float(orth.max()), float((np.sqrt(off) / tr).max())


# ---- the scenarios: ra_reference.scene's construction with other points ----------------------------------
CLOSE = dict(SCENE, points=(32, 35))                  # 0.094 apart in sin(theta); two Doppler bins
COHERENT = dict(SCENE, bins=(20, 20), points=(32, 37))   # one Doppler bin; phase pi/2 apart at the array's centre
CLOSE_SEED = 2                 # seeds 1..4 were tried on the CPU: 1 gives MUSIC {32, 35} in 7 of 8 frames; 2, 3, 4 meet all three conditions
COHERENT_SEED = 2              # seeds 1..4 tried: 2 gives {32, 37} with FB in 8 of 8 frames, the others in 7 of 8


@functools.lru_cache(maxsize=None)
def close_scene(seed=CLOSE_SEED, half=False):
    """ra_reference.scene with the sources at grid points 32 and 35."""
    S = CLOSE
    rng = np.random.default_rng(seed)
    sines = scene_sines().astype(np.float64)
    chans = []
    ph = rng.uniform(-np.pi, np.pi, (S["frames"], 2))
    for a in range(S["A"]):
        z = (rng.standard_normal((S["frames"], S["nr"], S["nd"])) + 1j * rng.standard_normal((S["frames"], S["nr"], S["nd"]))) \
            * np.sqrt(0.5)
        for s, (d, k) in enumerate(zip(S["bins"], S["points"])):
            z[:, S["row"], d] += S["amp"] * np.exp(1j * (2 * np.pi * S["spacing"] * a * sines[k] + ph[:, s]))
        chans.append(store(z, half))
    for c in chans:
        c.setflags(write=False)
    return chans


@functools.lru_cache(maxsize=None)
def coherent_scene(seed=COHERENT_SEED, half=False):
    """Both sources in Doppler bin 20, from grid points 32 and 37: the first has a random phase per
    frame, the second is pi/2 ahead of it at the array's centre (element (A - 1) / 2)."""
    S = COHERENT
    rng = np.random.default_rng(seed)
    sines = scene_sines().astype(np.float64)
    chans = []
    ph0 = rng.uniform(-np.pi, np.pi, S["frames"])
    mid = (S["A"] - 1) / 2.0
    for a in range(S["A"]):
        z = (rng.standard_normal((S["frames"], S["nr"], S["nd"])) + 1j * rng.standard_normal((S["frames"], S["nr"], S["nd"]))) \
            * np.sqrt(0.5)
        for s, k in enumerate(S["points"]):
            z[:, S["row"], S["bins"][s]] += S["amp"] * np.exp(
                1j * (2 * np.pi * S["spacing"] * (a - mid) * sines[k] + ph0 + s * np.pi / 2))
        chans.append(store(z, half))
    for c in chans:
        c.setflags(write=False)
    return chans


# ---- the cases of the GPU parity test ----------------------------------------------------------------------
def random_cov(seed, A, F, nr, garbage=False, zero_rows=()):
    """A caller's own cov: Hermitian from nd = 2 A snapshots over a few binades; garbage: the
    diagonal's imaginary parts hold values that must not be read; zero_rows: (f, r) all zero."""
    rng = np.random.default_rng(seed)
    rows = F * nr
    x = (rng.standard_normal((rows, A, 2 * A)) + 1j * rng.standard_normal((rows, A, 2 * A))) * np.exp2(
        rng.integers(-3, 4, (rows, 1, 1)))
    cov = pack(outer_sum(x)).reshape(F, nr, n_tri(A), 2)
    for f, r in zero_rows:
        cov[f, r] = 0
    if garbage:
        for a in range(A):
            cov[:, :, tri(A, a, a), 1] = rng.standard_normal((F, nr)).astype(F32) * 1e6
            cov[0, 0, tri(A, a, a), 1] = np.nan
    return np.ascontiguousarray(cov)
