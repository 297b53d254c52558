"""CPU: the MUSIC stage's reference (tests/music_reference.py, the steps of include/fmcw.h in float32)
proved against a float64 eigh, on the close-pair and coherent-pair scenarios and on the properties
of the definition; and every rule and message of fmcw_music_check and MusicConfig.  The device is
compared with this reference byte for byte in tests/test_gpu_music.py."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import MusicConfig, _lib
from fmcw_radar_processing_amd.engine import Engine
from tests import music_reference as M
from tests import ra_reference as R

F32 = np.float32

# ---- 1. against float64 eigh ------------------------------------------------------------------------------
# The largest values the reference showed on these pools (1024 rows each, sweeps = 8), as measured:
# (|lambda - lambda_ref| / tr, ||R V - V L||_F / tr, ||V^H V - I||_F).  The test asserts TWICE each; the
# margin covers pool-to-pool variation and is not a derived bound.
# near_identity at A = 5 and 8: one row of 1024, and a few, lose orthogonality.  An off-diagonal entry
# of about 5e-23 is met on its way to zero; h.re^2 + h.im^2 is then a denormal of a few units, and |ph|^2
# came out as 1.053 in the A = 5 row.  The eigenvalues of such rows are still right to 1e-7 (every
# vector is an eigenvector to that accuracy); the definition is kept as stated.
MEASURED = {
    (2, "source"): (1.49e-07, 1.99e-07, 4.16e-07), (2, "rank2"): (1.14e-07, 1.63e-07, 3.68e-07),
    (2, "near_identity"): (2.98e-08, 4.21e-08, 3.71e-07),
    (3, "source"): (1.45e-07, 2.37e-07, 8.29e-07), (3, "rank2"): (1.59e-07, 2.22e-07, 9.98e-07),
    (3, "near_identity"): (5.51e-08, 7.51e-08, 9.41e-07),
    (5, "source"): (1.96e-07, 2.69e-07, 2.01e-06), (5, "rank2"): (2.00e-07, 3.00e-07, 1.75e-06),
    (5, "near_identity"): (5.75e-08, 8.65e-08, 6.01e-02),
    (8, "source"): (2.28e-07, 3.68e-07, 3.10e-06), (8, "rank2"): (2.36e-07, 3.99e-07, 3.91e-06),
    (8, "near_identity"): (4.83e-08, 7.91e-08, 5.38e-04),
}


@pytest.mark.parametrize("kind", M.POOLS)
@pytest.mark.parametrize("A", [2, 3, 5, 8])
def test_reference_against_float64_eigh(A, kind):
    cov = M.eig_pool(kind, A)
    assert cov.shape[0] >= 1000
    lam, res, orth, off = M.eig_errors(cov, M.SWEEPS)
    off6 = M.eig_errors(cov, 6)[3]
    print(f"A={A} {kind}: |dlambda|/tr {lam:.3g}, residual/tr {res:.3g}, orthogonality {orth:.3g}, "
          f"off-diagonal/tr after 8 sweeps {off:.3g}, after 6 {off6:.3g}")
    m = MEASURED[A, kind]
    assert lam <= 2 * m[0] and res <= 2 * m[1] and orth <= 2 * m[2], (lam, res, orth, m)


def test_eigenpairs_are_sorted_and_matched():
    """eval ascending, and evec[j] the eigenvector OF eval[j]: R e_j = lambda_j e_j row by row."""
    A = 5
    cov = M.eig_pool("source", A)[:64].reshape(1, 64, -1, 2)
    out = M.music_reference(cov, n_src=1)
    ev = out["eval"][0].astype(np.float64)
    assert (np.diff(ev, axis=1) >= 0).all()
    E = out["evec"][0][..., 0].astype(np.float64) + 1j * out["evec"][0][..., 1]       # [rows][j][a]
    Rm = M.full_matrix(cov[0])
    tr = np.einsum("raa->r", Rm).real
    for j in range(A):
        r = np.einsum("rab,rb->ra", Rm, E[:, j]) - ev[:, j, None] * E[:, j]
        assert (np.linalg.norm(r, axis=1) / tr < 1e-6).all(), j


# ---- 2. the scenarios -----------------------------------------------------------------------------------
def _scene_cov(chans):
    return R.cov_reference(chans, R.SCENE["dc_half"])[0].astype(F32)


def _weights():
    S = R.SCENE
    return R.weights_f32(Engine.ra_weights(S["A"], R.scene_sines(), S["spacing"]))


@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_close_pair_is_resolved_by_music_alone(half):
    """ra_reference.scene's construction with the sources at grid points 32 and 35, 0.094 apart in
    sin(theta): MUSIC with n_src = 2 shows exactly {32, 35} in 8 of 8 frames, Bartlett one peak in 8 of
    8, Capon one peak in at least 6 of 8 (seed: music_reference.CLOSE_SEED)."""
    S = M.CLOSE
    cov = _scene_cov(M.close_scene(M.CLOSE_SEED, half))
    w = _weights()
    bart, _ = R.spectra_reference(cov, w)
    capon, _ = R.spectra_reference(cov, w, True, S["load"])
    music = M.music_reference(cov, w, n_src=2)["music"]
    pb = [R.peaks(bart[f, S["row"]]) for f in range(S["frames"])]
    pc = [R.peaks(capon[f, S["row"]]) for f in range(S["frames"])]
    pm = [R.peaks(music[f, S["row"]]) for f in range(S["frames"])]
    print("Bartlett", pb, "Capon", pc, "MUSIC", pm)
    assert all(p == list(S["points"]) for p in pm), pm
    assert all(len(p) == 1 for p in pb), pb
    assert sum(len(p) == 1 for p in pc) >= 6, pc


SRC_THR, MAX_SRC = 8.0, 4          # thresholds 4, 8 and 16 were searched on the CPU: all three give the counts below


@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_estimated_count(half):
    """max_src 4, src_thr 8: the source row's count is 2 in 8 of 8 frames and every one of the 120
    noise rows counts 0 (share 120 / 120)."""
    S = M.CLOSE
    cov = _scene_cov(M.close_scene(M.CLOSE_SEED, half))
    n = M.music_reference(cov, None, n_src=0, max_src=MAX_SRC, src_thr=SRC_THR)["nsrc"]
    assert n.dtype == np.int32 and (n[:, S["row"]] == 2).all(), n[:, S["row"]]
    noise = np.delete(n, S["row"], axis=1)
    print("noise rows counting 0:", int((noise == 0).sum()), "of", noise.size)
    assert noise.size == 120 and (noise == 0).all()


@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_coherent_pair_needs_forward_backward_averaging(half):
    """Both sources in Doppler bin 20 at points (32, 37), pi/2 apart in phase at the array's centre
    in every frame: without FMCW_MUSIC_FB no frame shows {32, 37}, with it 8 of 8 do (seed:
    music_reference.COHERENT_SEED)."""
    S = M.COHERENT
    cov = _scene_cov(M.coherent_scene(M.COHERENT_SEED, half))
    w = _weights()
    plain = M.music_reference(cov, w, n_src=2)["music"]
    fb = M.music_reference(cov, w, n_src=2, fb=True)["music"]
    pp = [R.peaks(plain[f, S["row"]]) for f in range(S["frames"])]
    pf = [R.peaks(fb[f, S["row"]]) for f in range(S["frames"])]
    print("without FB", pp, "with FB", pf)
    assert not any(p == list(S["points"]) for p in pp), pp
    assert all(p == list(S["points"]) for p in pf), pf


# ---- 3. properties of the definition -------------------------------------------------------------------------
def _toeplitz_cov(rows, A, seed):
    """Hermitian Toeplitz rows: R_ab = t[b - a], which is persymmetric (R_ab == R_a'b' exactly)."""
    rng = np.random.default_rng(seed)
    t = (rng.standard_normal((rows, A)) + 1j * rng.standard_normal((rows, A))).astype(np.complex64)
    t[:, 0] = A + rng.uniform(0, 1, rows)
    Rm = np.zeros((rows, A, A), np.complex128)
    for a in range(A):
        for b in range(a, A):
            Rm[:, a, b] = t[:, b - a]
            Rm[:, b, a] = np.conj(t[:, b - a])
    return M.pack(Rm)


@pytest.mark.parametrize("A", [2, 5, 8])
def test_fb_on_a_persymmetric_matrix_changes_no_byte(A):
    cov = _toeplitz_cov(32, A, A).reshape(2, 16, -1, 2)
    w = R.weights_f32(Engine.ra_weights(A, n_ang=17))
    a = M.music_reference(cov, w, n_src=1)
    b = M.music_reference(cov, w, n_src=1, fb=True)
    for k in ("eval", "evec", "nsrc", "music"):
        R.assert_same_bytes(a[k], b[k], k)
    # and on a general matrix it does change the result
    cov = M.random_cov(3, A, 2, 16)
    assert M.music_reference(cov, w, n_src=1)["music"].tobytes() != M.music_reference(cov, w, n_src=1, fb=True)["music"].tobytes()


@pytest.mark.parametrize("A", [2, 3, 8])
def test_zero_rows(A):
    """A zero row skips every rotation: lambda = 0, V = I, an estimated count of 0 and music exactly 1,
    with or without FB, whatever the diagonal's imaginary parts hold."""
    cov = M.random_cov(5, A, 1, 16, garbage=True, zero_rows=((0, 3), (0, 15)))
    w = R.weights_f32(Engine.ra_weights(A, n_ang=9))
    for fb in (False, True):
        out = M.music_reference(cov, w, n_src=0, max_src=A - 1, fb=fb)
        for r in (3, 15):
            assert not out["eval"][0, r].view(np.uint32).any()
            eye = np.zeros((A, A, 2), F32)
            eye[np.arange(A), np.arange(A), 0] = 1
            R.assert_same_bytes(out["evec"][0, r], eye)
            assert out["nsrc"][0, r] == 0
            assert (out["music"][0, r] == 1).all()
        assert np.isfinite(out["music"]).all() and np.isfinite(out["evec"]).all()      # the garbage is not read


def test_every_source_count_and_the_empty_signal_subspace():
    """n_src = A - 1 leaves one noise vector; an estimated n = 0 sums over all A eigenvectors, and V
    unitary then makes music 1 to rounding."""
    A = 4
    cov = M.random_cov(8, A, 1, 16)
    w = R.weights_f32(Engine.ra_weights(A, n_ang=33))
    full = M.music_reference(cov, w, n_src=A - 1)
    E = full["evec"][..., 0].astype(np.float64) + 1j * full["evec"][..., 1]
    wc = w[..., 0].astype(np.float64) + 1j * w[..., 1]
    want = np.abs(np.einsum("ka,fra->frk", wc, E[:, :, 0])) ** 2 / (np.abs(wc) ** 2).sum(axis=1)[None, None]   # den / e
    assert np.abs(1.0 / full["music"].astype(np.float64) - want).max() < 1e-5
    none = M.music_reference(cov, w, n_src=0, max_src=2, src_thr=1e30)
    assert (none["nsrc"] == 0).all()
    np.testing.assert_allclose(none["music"], 1.0, rtol=1e-5)
    R.assert_same_bytes(none["eval"], full["eval"])                       # the count touches neither eval nor evec
    R.assert_same_bytes(none["evec"], full["evec"])


def test_zero_denominator_gives_flt_max():
    """A diagonal R has V = I; with n_src = A - 1 the noise vector is the unit vector of the smallest
    entry, and a direction whose weight there is zero has den == 0."""
    A = 3
    Rm = np.zeros((16, A, A), np.complex128)
    Rm[:, 0, 0], Rm[:, 1, 1], Rm[:, 2, 2] = 3, 1, 2
    cov = M.pack(Rm).reshape(1, 16, -1, 2)
    w = np.zeros((2, A, 2), F32)
    w[0, 0, 0] = w[0, 2, 1] = 0.5                   # nothing in channel 1
    w[1, :, 0] = 0.25
    out = M.music_reference(cov, w, n_src=A - 1)
    assert (out["music"][..., 0] == M.FLT_MAX).all() and (out["music"][..., 1] == F32(0.1875) / F32(0.0625)).all()
    assert out["music_max"] == M.FLT_MAX
    zero_w = M.music_reference(cov, np.zeros((1, A, 2), F32), n_src=1)
    assert (zero_w["music"] == M.FLT_MAX).all()


def test_ties_keep_their_original_order():
    A = 4
    Rm = np.zeros((16, A, A), np.complex128)
    for a in range(A):
        Rm[:, a, a] = 7
    Rm[8:, 0, 0] = Rm[8:, 2, 2] = 9                  # rows 8..: (9, 7, 9, 7) -> order 1, 3, 0, 2
    out = M.music_reference(M.pack(Rm).reshape(1, 16, -1, 2), n_src=1)
    for r, order in ((0, (0, 1, 2, 3)), (12, (1, 3, 0, 2))):
        want = np.zeros((A, A, 2), F32)
        for j, a in enumerate(order):
            want[j, a, 0] = 1
        R.assert_same_bytes(out["evec"][0, r], want)
    assert (out["eval"][0, 0] == 7).all() and out["eval"][0, 12].tolist() == [7, 7, 9, 9]


def test_gate_and_running_maximum():
    A = 3
    cov = M.random_cov(11, A, 2, 16)
    w = R.weights_f32(Engine.ra_weights(A, n_ang=5))
    out = M.music_reference(cov, w, n_src=1, r_lo=4, r_hi=6)
    for k in ("eval", "evec", "nsrc", "music"):
        assert not out[k][:, :3].any() and not out[k][:, 6:].any() and out[k][:, 3:6].any(), k
    assert out["music_max"] == out["music"].max()
    whole = M.music_reference(cov, w, n_src=1)
    R.assert_same_bytes(out["music"][:, 3:6], whole["music"][:, 3:6])


# ---- 4. the argument rules: fmcw_music_check and MusicConfig agree, rule by rule ------------------------------
def _q(**over):
    kw = dict(n_chan=4, n_ang=16, r_lo=0, r_hi=0, n_src=0, max_src=2, sweeps=8, flags=0, src_thr=8.0)
    kw.update(over)
    return _lib.MusicParams(*[kw[k] for k in ("n_chan", "n_ang", "r_lo", "r_hi", "n_src", "max_src", "sweeps", "flags")],
                            kw["src_thr"])


# name -> (overrides, nr, message)
REJECTED = {
    "nr_small": ({}, 8, "music: nr must be a power of two in [16, 2048]"),
    "nr_not_pow2": ({}, 24, "music: nr must be a power of two in [16, 2048]"),
    "nr_large": ({}, 4096, "music: nr must be a power of two in [16, 2048]"),
    "gate_reversed": (dict(r_lo=5, r_hi=3), 64, "music: r_lo > r_hi"),
    "gate_half_zero": (dict(r_lo=0, r_hi=5), 64, "music: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
    "gate_past_nr": (dict(r_lo=1, r_hi=65), 64, "music: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
    "n_chan_1": (dict(n_chan=1, max_src=1), 64, "music: n_chan must be in [2, 8]"),
    "n_chan_9": (dict(n_chan=9), 64, "music: n_chan must be in [2, 8]"),
    "n_ang_0": (dict(n_ang=0), 64, "music: n_ang must be in [1, 256]"),
    "n_ang_257": (dict(n_ang=257), 64, "music: n_ang must be in [1, 256]"),
    "n_src_negative": (dict(n_src=-1), 64, "music: n_src must be in [0, n_chan - 1] (0 estimates it)"),
    "n_src_is_n_chan": (dict(n_src=4), 64, "music: n_src must be in [0, n_chan - 1] (0 estimates it)"),
    "max_src_0": (dict(max_src=0), 64, "music: max_src must be in [1, n_chan - 1] when n_src is 0"),
    "max_src_is_n_chan": (dict(max_src=4), 64, "music: max_src must be in [1, n_chan - 1] when n_src is 0"),
    "sweeps_0": (dict(sweeps=0), 64, "music: sweeps must be in [1, 16]"),
    "sweeps_17": (dict(sweeps=17), 64, "music: sweeps must be in [1, 16]"),
    "flag_unknown": (dict(flags=2), 64, "music: unknown flag bits"),
    "thr_zero": (dict(src_thr=0.0), 64, "music: src_thr must be finite and > 0"),
    "thr_negative": (dict(src_thr=-1.0), 64, "music: src_thr must be finite and > 0"),
    "thr_nan": (dict(src_thr=float("nan")), 64, "music: src_thr must be finite and > 0"),
    "thr_inf": (dict(src_thr=float("inf")), 64, "music: src_thr must be finite and > 0"),
}


def _config(over):
    kw = dict(n_chan=4, n_ang=16, r_lo=0, r_hi=0, n_src=0, max_src=2, sweeps=8, src_thr=8.0)
    kw.update({k: v for k, v in over.items() if k != "flags"})
    return MusicConfig(**kw)


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_rejected(name):
    over, nr, msg = REJECTED[name]
    lib = _lib.load()
    assert lib.fmcw_music_check(ct.byref(_q(**over)), nr) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error().decode() == msg
    if "flags" not in over:                       # MusicConfig has no way to set an unknown bit
        with pytest.raises(ValueError) as e:
            _config(over).validate(nr)
        assert str(e.value) == msg


def test_accepted():
    lib = _lib.load()
    for over, nr in ((dict(), 64), (dict(n_chan=2, max_src=1), 16), (dict(n_chan=8, n_src=7, max_src=0), 2048),
                     (dict(n_chan=8, n_src=7, max_src=99), 64),          # max_src is read only when n_src = 0
                     (dict(r_lo=7, r_hi=7), 64), (dict(r_lo=1, r_hi=64), 64), (dict(sweeps=1), 64), (dict(sweeps=16), 64),
                     (dict(n_ang=1), 64), (dict(n_ang=256), 64), (dict(src_thr=1e-30), 64)):
        assert lib.fmcw_music_check(ct.byref(_q(**over)), nr) == _lib.FMCW_OK, over
        _config(over).validate(nr)
    assert lib.fmcw_music_check(ct.byref(_q(flags=_lib.FMCW_MUSIC_FB)), 64) == _lib.FMCW_OK
    assert MusicConfig(4, 16, fb=True).abi().flags == _lib.FMCW_MUSIC_FB and MusicConfig(4, 16).abi().flags == 0
    assert MusicConfig(4, 16).sweeps == M.SWEEPS
    assert lib.fmcw_music_check(None, 64) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"music params is NULL"


def test_the_first_violated_rule_is_reported():
    lib = _lib.load()
    assert lib.fmcw_music_check(ct.byref(_q(n_chan=1, sweeps=0)), 24) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"music: nr must be a power of two in [16, 2048]"
    assert lib.fmcw_music_check(ct.byref(_q(n_chan=1, sweeps=0, r_lo=5, r_hi=2)), 32) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"music: r_lo > r_hi"


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    q = _q()
    assert lib.fmcw_music(None, ct.byref(q), None, 1, 64, None, None, None, None, None, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ctx is NULL"
    assert lib.fmcw_music_device(None, ct.byref(q), None, 1, 64, None, None, None, None, None, None, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ctx is NULL"
    assert _lib.MUSIC_STAGE == 18


def test_mex_gateway_documents_and_dispatches_music():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "mex", "fmcw_mex.c")).read()
    assert "fmcw_mex('music'" in src and re.search(r'^  if \(!strcmp\(cmd, "music"\)\)', src, re.M)
    assert "fmcw_mex('music'" in open(os.path.join(root, "INTEGRATION.md")).read()
