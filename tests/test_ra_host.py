"""CPU: the host-side half of the range-angle stage (include/fmcw.h, fmcw_ra_params) -- the rules of
fmcw_ra_check and fmcw_ra_steer -- and the conditions the GPU tests rest on (tests/ra_reference.py):
the covariance reference against a plain loop, the float32 spectra against float64 within derived
bounds, the two-source scenario that is the reason for the stage, and the degenerate rows."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import RaConfig, _lib
from fmcw_radar_processing_amd import params as P
from fmcw_radar_processing_amd.engine import Engine
from tests import ra_reference as R
from tests.mti_reference import as_floats
from tests.test_beam_host import STEER_REJECTED

F32 = np.float32
U = R.U


def _q(n_chan=2, n_ang=8, r_lo=0, r_hi=0, dc_half=0, flags=0, load=1e-3):
    return _lib.RaParams(n_chan, n_ang, r_lo, r_hi, dc_half, flags, load)


def hermitian(cov_row, A):
    """float64 complex [A][A] from one packed row [T][2]."""
    M = np.zeros((A, A), complex)
    for a in range(A):
        for b in range(a, A):
            v = complex(float(cov_row[R.tri(A, a, b), 0]), float(cov_row[R.tri(A, a, b), 1]) if b > a else 0.0)
            M[a, b] = v
            M[b, a] = v.conjugate()
    return M


def table(A, K, seed):
    """float32 [K][A][2] of ra_weights over a random grid with a taper and a calibration."""
    rng = np.random.default_rng(seed)
    sines = np.sort(rng.uniform(-1, 1, K))
    cal = (0.8 + 0.4 * rng.random(A)) * np.exp(2j * np.pi * rng.random(A))
    return R.weights_f32(Engine.ra_weights(A, sines, 0.5, cal=cal, taper=0.5 + rng.random(A)))


# ---- 1. cov_reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 3, 5, 8])
@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_cov_reference_equals_a_plain_loop(A, half):
    """The vectorised float64 reference against a loop over every frame, row, bin and pair, over
    gates and dc_half; the packed index is the header's; N is the number of bins kept."""
    chans = R.pool(40 + A, A, 2, 16, 8, half)
    assert [R.tri(A, a, b) for a in range(A) for b in range(a, A)] == list(range(R.n_tri(A)))
    assert R.tri(A, A - 1, A - 1) == A * (A + 1) // 2 - 1
    for dc, gate, n in ((-1, (0, 0), 8), (0, (3, 9), 7), (2, (16, 16), 3), (3, (1, 1), 1)):
        cov, N, bound = R.cov_reference(chans, dc, *gate)
        want = R.cov_loop(chans, dc, *gate)
        assert N == n
        assert np.abs(cov - want).max() <= 1e-12 * np.abs(want).max()
        g0, g1 = R.gate_rows(16, *gate)
        assert not cov[:, :g0].any() and not cov[:, g1 + 1:].any()
        assert (cov[:, g0:g1 + 1, [R.tri(A, a, a) for a in range(A)], 0] > 0).all()
        assert not cov[..., [R.tri(A, a, a) for a in range(A)], 1].any()
        assert (bound[:, g0:g1 + 1] > 0).all()
    if half:       # the stored values are D / (nr nd): the sums come back in the units of |D|^2
        x = [as_floats(c)[0].astype(np.float64) * (16 * 8) for c in chans]
        p00 = (x[0][..., 0] ** 2 + x[0][..., 1] ** 2).sum(axis=-1)
        assert np.allclose(R.cov_reference(chans)[0][..., 0, 0], p00, rtol=1e-12)


# ---- 2. Bartlett ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 3, 5, 8])
def test_bartlett_reference_against_float64(A):
    """ra of the float32 reference against float64 w^T R conj(w) on the same cov bytes, and against
    sum_d |w . x|^2 formed from the maps, both within (N + 8 + 4 A^2) 2^-24 (sum_a |w_a| sqrt(R_aa))^2:
    absolute, because a direction in a null has no relative bound.  cov carries (N + 8) 2^-24
    sqrt(R_aa R_bb) per entry, each of the A^2 terms of the form three roundings and the running sum
    one more."""
    nr, nd, F, K = 16, 32, 2, 33
    chans = R.pool(60 + A, A, F, nr, nd, False)
    cov64, N, _ = R.cov_reference(chans, 0)
    cov = cov64.astype(F32)
    w = table(A, K, A)
    ra, mx = R.spectra_reference(cov, w)
    assert ra.dtype == np.float32 and mx == ra.max()
    wc = w[..., 0].astype(np.float64) + 1j * w[..., 1].astype(np.float64)            # [K][A]
    z = [c.astype(np.complex128) for c in chans]
    keep = R.kept_bins(nd, 0)
    worst = 0.0
    for f in range(F):
        for r in range(nr):
            M = hermitian(cov[f, r], A)
            quad = np.einsum("ka,ab,kb->k", wc, M, wc.conj()).real
            beam = sum(wc[:, a, None] * z[a][f, r][None, keep] for a in range(A))
            direct = (np.abs(beam) ** 2).sum(axis=1)
            bound = (N + 8 + 4 * A * A) * U * (np.abs(wc) * np.sqrt(np.diag(M).real)[None, :]).sum(axis=1) ** 2
            for other in (quad, direct):
                err = np.abs(ra[f, r].astype(np.float64) - other)
                assert (err <= bound).all(), (f, r, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
    print(f"A = {A}: largest error / bound {worst:.3f}")
    assert 0 < worst <= 1


# ---- 3. Capon -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 3, 5, 8])
def test_capon_reference_against_numpy_linalg(A):
    """Well-conditioned rows (load 1e-2): the float32 steps against |u|^4 / (u^H M^-1 u) by
    numpy.linalg in float64, u = conj(w).  The tolerance comes from the condition number the test
    computes: a Cholesky solve is backward stable, its computed y solves (L + dL) y = u with
    |dL| <= gamma_A |L| per triangular solve and L L^H = M + dM with |dM| <= gamma_(A+1) |L| |L^H|, so
    q = u^H M^-1 u is off by at most about (3 A + 1) u kappa_2(M) relative, times 4 for the complex
    products (each is four real multiplies and two adds); e^2 / q adds 2 A + 4 roundings."""
    nr, nd, F, K, load = 16, 64, 2, 17, 1e-2
    chans = R.pool(80 + A, A, F, nr, nd, False)
    cov = R.cov_reference(chans, 0)[0].astype(F32)
    w = table(A, K, 10 + A)
    ra, _ = R.spectra_reference(cov, w, True, load)
    u = w[..., 0].astype(np.float64) - 1j * w[..., 1].astype(np.float64)
    worst = 0.0
    for f in range(F):
        for r in range(nr):
            M = hermitian(cov[f, r], A)
            M = M + float(F32(load)) * np.trace(M).real / A * np.eye(A)
            kappa = np.linalg.cond(M)
            assert kappa < 1e4
            q = np.einsum("ka,ka->k", u.conj(), np.linalg.solve(M, u.T).T).real
            want = (np.abs(u) ** 2).sum(axis=1) ** 2 / q
            tol = (4 * (3 * A + 1) * kappa + 2 * A + 4) * U
            rel = np.abs(ra[f, r].astype(np.float64) - want) / want
            assert (rel <= tol).all(), (f, r, float((rel / tol).max()), kappa)
            worst = max(worst, float((rel / tol).max()))
    print(f"A = {A}: largest relative error / tolerance {worst:.3f}")
    assert 0 < worst <= 1
    # with w = conj(a) / A this is the usual MVDR power 1 / (a^H M^-1 a)
    sines = np.linspace(-0.9, 0.9, 7)
    wa = R.weights_f32(Engine.ra_weights(A, sines, 0.5))
    ra, _ = R.spectra_reference(cov[:1, :1], wa, True, load)
    a = np.exp(2j * np.pi * 0.5 * np.arange(A)[None, :] * sines.astype(F32).astype(np.float64)[:, None])
    M = hermitian(cov[0, 0], A)
    M = M + float(F32(load)) * np.trace(M).real / A * np.eye(A)
    mvdr = 1.0 / np.einsum("ka,ka->k", a.conj(), np.linalg.solve(M, a.T).T).real
    assert np.allclose(ra[0, 0], mvdr, rtol=1e-4)


# ---- 4. what the stage is for ------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_two_sources_in_one_range_row(half):
    """A = 8, nd = 64, two sources of amplitude 30 over unit noise in one range row, 5 grid points
    (0.15625 in sin(theta)) apart: in every one of 8 frames the Bartlett spectrum shows ONE peak above
    a quarter of its maximum, between the two, and the Capon spectrum exactly two, at the true grid
    points."""
    S = R.SCENE
    chans = R.scene(1, half)
    cov = R.cov_reference(chans, S["dc_half"])[0].astype(F32)
    w = R.weights_f32(Engine.ra_weights(S["A"], R.scene_sines(), S["spacing"]))
    bart, _ = R.spectra_reference(cov, w)
    capon, _ = R.spectra_reference(cov, w, True, S["load"])
    for f in range(S["frames"]):
        pb, pc = R.peaks(bart[f, S["row"]]), R.peaks(capon[f, S["row"]])
        print(f"frame {f}: Bartlett peaks {pb}, Capon peaks {pc}")
        assert len(pb) == 1 and pb[0] in (34, 35), (f, pb)
        assert pc == list(S["points"]), (f, pc)
        # both estimate a lone source's summed power: the Capon peaks sit near amp^2 (scaled units in fp16 too)
        assert np.all(np.abs(capon[f, S["row"], list(S["points"])] / S["amp"] ** 2 - 1) < 0.5)


# ---- 5. degenerate rows -------------------------------------------------------------------------------------
def test_degenerate_rows():
    A, K = 8, 9
    w = table(A, K, 3)
    zero = np.zeros((1, 16, R.n_tri(A), 2), F32)
    for load in (0.0, 1e-3, 1.0):
        ra, mx = R.spectra_reference(zero, w, True, load)            # delta = load * 0 = 0: not factorable
        assert not ra.view(np.uint32).any() and mx == 0
    ra, mx = R.spectra_reference(zero, w)
    assert not ra.any() and mx == 0
    # N < A with load 0: nd = 4 with dc_half 0 keeps 3 bins, R has rank 3 of 8
    chans = R.pool(7, A, 2, 16, 4, False)
    cov = R.cov_reference(chans, 0)[0].astype(F32)
    ra, mx = R.spectra_reference(cov, w, True, 0.0)
    assert np.isfinite(ra).all() and np.isfinite(mx)
    bart, _ = R.spectra_reference(cov, w)
    assert np.isfinite(bart).all() and (bart > 0).any()
    # a row made degenerate among good ones zeroes only itself
    good = R.cov_reference(R.pool(8, A, 1, 16, 64, False), 0)[0].astype(F32)
    mixed = good.copy()
    mixed[0, 4] = 0
    mixed[0, 9, R.tri(A, 2, 2), 0] = -1.0
    ra, _ = R.spectra_reference(mixed, w, True, 1e-3)
    ref, _ = R.spectra_reference(good, w, True, 1e-3)
    assert not ra[0, 4].any() and not ra[0, 9].any()
    keep = [r for r in range(16) if r not in (4, 9)]
    assert ra[0, keep].tobytes() == ref[0, keep].tobytes() and (ra[0, keep] > 0).all()
    # the imaginary part of a diagonal entry is not read
    odd = good.copy()
    odd[..., [R.tri(A, a, a) for a in range(A)], 1] = 7.5
    for capon in (False, True):
        assert R.spectra_reference(odd, w, capon, 1e-3)[0].tobytes() == R.spectra_reference(good, w, capon, 1e-3)[0].tobytes()
    # the maximum ignores what is below +0
    assert R.max_bits(np.array([-3.0, -0.0], F32)) == 0 and R.max_bits(np.array([-3.0, 2.5, 1.0], F32)) == 2.5


# ---- 6. fmcw_ra_check and RaConfig ------------------------------------------------------------------------
# every violation fmcw_ra_check must name (shared with tests/test_gpu_ra.py): (params, nr, nd, the message)
REJECTED = {
    "one_channel": (dict(n_chan=1), 256, 16, "ra: n_chan must be in [2, 8]"),
    "nine_channels": (dict(n_chan=9), 256, 16, "ra: n_chan must be in [2, 8]"),
    "no_direction": (dict(n_ang=0), 256, 16, "ra: n_ang must be in [1, 256]"),
    "too_many_directions": (dict(n_ang=257), 256, 16, "ra: n_ang must be in [1, 256]"),
    "dc_half_below_minus_1": (dict(dc_half=-2), 256, 16, "ra: dc_half must be >= -1 (-1 leaves no Doppler bin out)"),
    "dc_band_is_the_whole_axis": (dict(dc_half=8), 256, 16, "ra: 2 dc_half + 1 must be < nd"),
    "stray_flag_bit": (dict(flags=2), 256, 16, "ra: unknown flag bits"),
    "stray_flag_bit_with_capon": (dict(flags=5), 256, 16, "ra: unknown flag bits"),
    "load_negative": (dict(load=-1e-3), 256, 16, "ra: load must be finite and >= 0"),
    "load_nan": (dict(load=float("nan")), 256, 16, "ra: load must be finite and >= 0"),
    "load_inf": (dict(load=float("inf")), 256, 16, "ra: load must be finite and >= 0"),
    "gate_reversed": (dict(r_lo=9, r_hi=8), 256, 16, "ra: r_lo > r_hi"),
    "gate_from_0": (dict(r_lo=0, r_hi=8), 256, 16, "ra: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
    "gate_past_nr": (dict(r_lo=1, r_hi=257), 256, 16, "ra: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
    "nd_not_a_power_of_two": (dict(), 256, 24, "ra: nd must be a power of two in [4, 1024]"),
    "nd_below_4": (dict(), 64, 2, "ra: nd must be a power of two in [4, 1024]"),
    "nd_above_1024": (dict(), 64, 2048, "ra: nd must be a power of two in [4, 1024]"),
    "nr_above_2048": (dict(), 4096, 16, "ra: nr must be a power of two in [16, 2048]"),
    "nr_below_16": (dict(), 8, 16, "ra: nr must be a power of two in [16, 2048]"),
}


def test_check_accepts_what_the_gpu_tests_use():
    lib = _lib.load()
    for over, nr, nd in ((dict(), 16, 4), (dict(n_chan=8, n_ang=256, flags=1, load=0.0), 2048, 1024),
                         (dict(n_chan=5, n_ang=1, dc_half=-1, r_lo=16, r_hi=16), 16, 1024), (dict(dc_half=1), 64, 4),
                         (dict(n_chan=3, n_ang=65, dc_half=127, flags=1, load=1.0, r_lo=1, r_hi=1), 32, 256)):
        assert lib.fmcw_ra_check(ct.byref(_q(**over)), nr, nd) == _lib.FMCW_OK, over
    assert lib.fmcw_ra_check(None, 256, 16) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ra params is NULL"
    q = RaConfig(n_chan=5, n_ang=65, r_lo=2, r_hi=9, dc_half=1, capon=True, load=0.25)
    q.validate(256, 16)
    a = q.abi()
    assert (a.n_chan, a.n_ang, a.r_lo, a.r_hi, a.dc_half, a.flags, a.load) == (5, 65, 2, 9, 1, _lib.FMCW_RA_CAPON, 0.25)
    assert RaConfig(2, 1).abi().flags == 0 and P.RaConfig is RaConfig


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_check_rejects(name):
    lib = _lib.load()
    over, nr, nd, msg = REJECTED[name]
    assert lib.fmcw_ra_check(ct.byref(_q(**dict(over))), nr, nd) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error().decode() == msg
    kw = dict(over)
    flags = kw.pop("flags", 0)
    if not flags & ~_lib.FMCW_RA_CAPON:                     # the Python mirror names the same rule
        cfg = RaConfig(**{**dict(n_chan=2, n_ang=8, dc_half=0), **kw}, capon=bool(flags))
        with pytest.raises(ValueError) as e:
            cfg.validate(nr, nd)
        assert str(e.value) == msg


def test_shape_comes_first_then_the_gate():
    lib = _lib.load()
    assert lib.fmcw_ra_check(ct.byref(_q(n_chan=1, r_lo=5, r_hi=2)), 24, 2) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ra: nr must be a power of two in [16, 2048]"
    assert lib.fmcw_ra_check(ct.byref(_q(n_chan=1, r_lo=5, r_hi=2)), 32, 2) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ra: nd must be a power of two in [4, 1024]"
    assert lib.fmcw_ra_check(ct.byref(_q(n_chan=1, r_lo=5, r_hi=2)), 32, 16) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ra: r_lo > r_hi"


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    q = _q()
    assert lib.fmcw_ra(None, ct.byref(q), None, 0, 1, 256, 16, None, None, None, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_cov_device(None, ct.byref(q), None, 0, 1, 256, 16, None, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_ra_device(None, ct.byref(q), None, 1, 256, None, None, None, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ctx is NULL"
    assert "ra" == _lib.STAGES[17] and len(_lib.STAGES) == 18


# ---- 7. fmcw_ra_steer ---------------------------------------------------------------------------------
def _ra_steer(n_chan, sin_theta, spacing=0.5, cal=None, taper=None, normalize=1, w=None):
    lib = _lib.load()
    st = None if sin_theta is None else np.ascontiguousarray(sin_theta, F32)
    c = None if cal is None else np.ascontiguousarray(np.asarray(cal, np.complex64)).view(F32)
    t = None if taper is None else np.ascontiguousarray(taper, F32)
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    n = 0 if st is None else st.size
    w = np.full((max(n, 1), max(min(n_chan, 8), 1), 2), np.nan, F32) if w is None else w
    return lib.fmcw_ra_steer(n_chan, n, spacing, ptr(st), ptr(c), ptr(t), normalize, w.ctypes.data), w


def _beam_steer(n_chan, sins, spacing, cal, taper, normalize):
    st = np.ascontiguousarray(sins, F32)
    c = None if cal is None else np.ascontiguousarray(np.asarray(cal, np.complex64)).view(F32)
    t = None if taper is None else np.ascontiguousarray(taper, F32)
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    q = _lib.BeamParams()
    assert _lib.load().fmcw_beam_steer(n_chan, st.size, spacing, ptr(st), ptr(c), ptr(t), normalize, ct.byref(q)) == _lib.FMCW_OK
    return np.array(q.w[:], F32).reshape(8, 8, 2)[:st.size, :n_chan]


def test_steer_equals_beam_steer_in_every_block_of_8():
    rng = np.random.default_rng(11)
    for A in (2, 3, 5, 8):
        for K in (1, 8, 63, 65, 256):
            for spacing, use_cal, use_taper, normalize in ((0.5, 0, 0, 1), (-0.37, 1, 1, 1), (16.0, 1, 0, 0), (0.01, 0, 1, 0)):
                sins = np.concatenate([[1.0, -1.0, 0.0, 0.5], rng.uniform(-1, 1, K)])[:K].astype(F32)
                cal = ((0.5 + rng.random(A)) * np.exp(2j * np.pi * rng.random(A))).astype(np.complex64) if use_cal else None
                taper = (0.5 + rng.random(A)).astype(F32) if use_taper else None
                st, w = _ra_steer(A, sins, spacing, cal, taper, normalize)
                assert st == _lib.FMCW_OK and w.shape == (K, A, 2)
                for k0 in range(0, K, 8):
                    want = _beam_steer(A, sins[k0:k0 + 8], spacing, cal, taper, normalize)
                    assert w[k0:k0 + 8].tobytes() == np.ascontiguousarray(want).tobytes(), (A, K, k0)
                got = Engine.ra_weights(A, sins, spacing, cal, taper, bool(normalize))
                assert got.dtype == np.complex64 and got.tobytes() == w.tobytes()
    # the default grid: n_ang points uniform in sin(theta), the ends included
    w = Engine.ra_weights(4)
    assert w.shape == (65, 4) and w.tobytes() == Engine.ra_weights(4, np.linspace(-1, 1, 65)).tobytes()
    assert Engine.ra_weights(4, n_ang=1).tobytes() == Engine.ra_weights(4, [0.0]).tobytes()


@pytest.mark.parametrize("name", sorted(STEER_REJECTED))
def test_steer_rejects_what_beam_steer_rejects(name):
    """Every argument fmcw_beam_steer refuses is refused here with the same words after the stage's
    prefix (the count of directions has its own name and limit), and w is not written."""
    kw, word = STEER_REJECTED[name]
    if name == "nine_beams":                                  # nine directions are fine here: the limit is 256
        assert _ra_steer(**kw)[0] == _lib.FMCW_OK
        kw = dict(kw, sin_theta=[0] * 257)
    st, w = _ra_steer(**kw)
    assert st == _lib.FMCW_E_ARG
    msg = _lib.load().fmcw_last_error().decode()
    assert msg.startswith("ra: ") and word.replace("n_beam", "n_ang") in msg
    assert np.isnan(w).all()                                  # a rejected call writes nothing
    lib = _lib.load()
    if name not in ("no_beam", "nine_beams"):                 # word for word beam_steer's message
        from tests.test_beam_host import _steer
        assert _steer(**kw)[0] == _lib.FMCW_E_ARG
        assert lib.fmcw_last_error().decode() == "beam: " + msg[len("ra: "):]


def test_steer_null_pointers():
    lib = _lib.load()
    st = np.zeros(1, F32)
    assert lib.fmcw_ra_steer(2, 1, 0.5, st.ctypes.data, None, None, 1, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ra: w is NULL"
    w = np.zeros((1, 2, 2), F32)
    assert lib.fmcw_ra_steer(2, 1, 0.5, None, None, None, 1, w.ctypes.data) == _lib.FMCW_E_ARG
    assert b"sin_theta" in lib.fmcw_last_error()
    with pytest.raises(ValueError):
        Engine.ra_weights(3, [0.0], cal=[1, 1])


# ---- 8. the MEX gateway dispatches what it documents ------------------------------------------------------
def test_mex_gateway_dispatches_every_documented_command():
    """The compile check of the gateway (tests/test_host.py) cannot see a command block nested inside
    another one: the braces balance and the command can never run.  So, on the source: every command
    the gateway's header comment documents is compared against `cmd` at the top level of mexFunction
    (two spaces of indent), no dispatching `if` sits inside another, and the commands documented as needing no context
    ('json', 'beam_steer', 'ra_steer') are dispatched before the top-level context check."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = open(os.path.join(root, "mex", "fmcw_mex.c")).read().split("\n")
    documented = set(re.findall(r"fmcw_mex\('([a-z_]+)'", "\n".join(lines)))
    assert {"ra", "ra_steer", "beam", "beam_steer", "init", "json", "process", "oscfar"} <= documented
    top = {}
    for n, line in enumerate(lines):
        if re.match(r"  \S", line):
            for name in re.findall(r'strcmp\(cmd, "([a-z_]+)"\)', line):
                top.setdefault(name, n)
    assert documented <= set(top), sorted(documented - set(top))
    assert set(top) <= documented, sorted(set(top) - documented)
    need_ctx = [n for n, line in enumerate(lines) if line.startswith("  if (!g_ctx)")]
    assert len(need_ctx) == 1
    for name in ("init", "close", "json", "beam_steer", "ra_steer"):
        assert top[name] < need_ctx[0], name
    for name in ("ra", "beam", "process", "cfar"):
        assert top[name] > need_ctx[0], name
    nested = [line for line in lines if re.match(r"\s{3,}if \(.*strcmp\(cmd, ", line)]      # a dispatch inside a dispatch
    assert not nested, nested
