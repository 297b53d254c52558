"""CPU: the host-side half of the angle-of-arrival stage (include/fmcw.h, fmcw_aoa_params) -- the
argument rules -- and checks that pin the reference the GPU tests compare against
(tests/aoa_reference.py): exact quarter-turn rotations, a weight that undoes one, the float32 sums
against the float64 ones, the coherence clamp, the order sensitivity of the constructed values, and
the physics on the oracle's RD maps."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import _lib
from fmcw_radar_processing_amd import params as P
from tests import aoa_reference as R
from tests import cfar_reference as CR
from tests import cluster_reference as CL
from tests.test_cluster_host import lists_of_mask

F32 = np.float32


def _q(**over):
    d = dict(n_chan=2, max_tgt=16, flags=0, spacing=0.5)
    w = over.pop("w", None)
    d.update(over)
    q = _lib.AoaParams(d["n_chan"], d["max_tgt"], d["flags"], d["spacing"])
    q.w[:] = [1.0, 0.0] * 8
    for i, x in (w or {}).items():
        q.w[i] = x
    return q


# every violation fmcw_aoa_check must name (shared with tests/test_gpu_aoa.py):
# (params, nr, nd, max_det, a word of the message)
REJECTED = {
    "one_channel": (dict(n_chan=1), 256, 16, 64, "n_chan"),
    "nine_channels": (dict(n_chan=9), 256, 16, 64, "n_chan"),
    "max_tgt_negative": (dict(max_tgt=-1), 256, 16, 64, "max_tgt"),
    "max_tgt_65": (dict(max_tgt=65), 256, 16, 64, "max_tgt"),
    "max_det_0": (dict(), 256, 16, 0, "max_det"),
    "max_det_1025": (dict(), 256, 16, 1025, "max_det"),
    "spacing_0": (dict(spacing=0.0), 256, 16, 64, "spacing"),
    "spacing_nan": (dict(spacing=float("nan")), 256, 16, 64, "spacing"),
    "spacing_small": (dict(spacing=0.005), 256, 16, 64, "spacing"),
    "spacing_negative_small": (dict(spacing=-0.005), 256, 16, 64, "spacing"),
    "spacing_17": (dict(spacing=17.0), 256, 16, 64, "spacing"),
    "spacing_inf": (dict(spacing=float("-inf")), 256, 16, 64, "spacing"),
    "weight_inf": (dict(w={2: float("inf")}), 256, 16, 64, "weights"),
    "weight_nan": (dict(w={1: float("nan")}), 256, 16, 64, "weights"),
    "stray_flag_bit": (dict(flags=1), 256, 16, 64, "flag"),
    "nd_not_a_power_of_two": (dict(), 256, 24, 64, "nd"),
    "nr_above_2048": (dict(), 4096, 16, 64, "nr"),
    "nr_below_16": (dict(), 8, 16, 64, "nr"),
    "nd_below_4": (dict(), 64, 2, 64, "nd"),
}


# ---- 1. fmcw_aoa_check -----------------------------------------------------------------------------
def test_check_accepts_what_the_gpu_tests_use():
    lib = _lib.load()
    for over, nr, nd, max_det in ((dict(), 256, 16, 1024), (dict(n_chan=3, max_tgt=64), 1024, 256, 1024),
                                  (dict(n_chan=8, max_tgt=64), 64, 16, 65), (dict(max_tgt=0), 16, 4, 1),
                                  (dict(spacing=-0.5), 64, 16, 63), (dict(spacing=0.01), 2048, 1024, 256),
                                  (dict(spacing=-16.0), 128, 32, 64),
                                  (dict(n_chan=3, w={0: 0.8, 1: -0.3, 2: 0.1, 3: 1.2, 4: -0.9, 5: 0.4}), 256, 32, 1024)):
        assert lib.fmcw_aoa_check(ct.byref(_q(**over)), nr, nd, max_det) == _lib.FMCW_OK, over
    assert lib.fmcw_aoa_check(None, 256, 16, 64) == _lib.FMCW_E_ARG
    # a non-finite weight of a channel the call does not use is ignored
    assert lib.fmcw_aoa_check(ct.byref(_q(w={4: float("nan")})), 256, 16, 64) == _lib.FMCW_OK
    q = P.AoaConfig(n_chan=3, spacing=-0.25, max_tgt=8, weights=(1, 0.5 - 0.25j, -2j))
    q.validate(256, 16, 64)
    a = q.abi()
    assert (a.n_chan, a.max_tgt, a.flags, a.spacing) == (3, 8, 0, -0.25)
    assert list(a.w[:8]) == [1.0, 0.0, 0.5, -0.25, 0.0, -2.0, 1.0, 0.0]
    assert q.kinv == F32(1.0 / (2 * np.pi * -0.25))
    with pytest.raises(ValueError, match="weights"):
        P.AoaConfig(n_chan=3, weights=(1, 1)).abi()


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_check_rejects(name):
    lib = _lib.load()
    over, nr, nd, max_det, word = REJECTED[name]
    assert lib.fmcw_aoa_check(ct.byref(_q(**dict(over))), nr, nd, max_det) == _lib.FMCW_E_ARG
    msg = lib.fmcw_last_error().decode()
    assert msg.startswith("aoa: ") and word in msg
    if "flags" not in over:                    # the Python mirror names the same rule
        kw = {k: v for k, v in over.items() if k != "w"}
        if "w" in over:
            ws = [1 + 0j, 1 + 0j]
            for i, x in over["w"].items():
                ws[i // 2] = complex(x, 0) if i % 2 == 0 else complex(1, x)
            kw["weights"] = tuple(ws)
        with pytest.raises(ValueError, match=word):
            P.AoaConfig(**kw).validate(nr, nd, max_det)


def test_shape_messages_and_nr_before_nd():
    lib = _lib.load()
    assert lib.fmcw_aoa_check(ct.byref(_q()), 24, 16, 64) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"aoa: nr must be a power of two in [16, 2048]"
    assert lib.fmcw_aoa_check(ct.byref(_q()), 64, 2048, 64) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"aoa: nd must be a power of two in [4, 1024]"
    assert lib.fmcw_aoa_check(ct.byref(_q()), 24, 2, 64) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"aoa: nr must be a power of two in [16, 2048]"


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    q, t = _q(), _lib.Angles()
    assert lib.fmcw_aoa(None, ct.byref(q), None, 0, 1, 256, 16, 64, *([None] * 4), ct.byref(t)) == _lib.FMCW_E_ARG
    assert lib.fmcw_aoa_device(None, ct.byref(q), None, 0, 1, 256, 16, 64, *([None] * 4), ct.byref(t), None) \
        == _lib.FMCW_E_ARG


# ---- constructed inputs (shared with tests/test_gpu_aoa.py) ------------------------------------------
def quarter_turn(x, k):
    """x * j^k, exactly: components swapped and negated, no multiplication."""
    x = np.asarray(x, np.complex64)
    k %= 4
    re, im = (x.real, x.imag) if k == 0 else (-x.imag, x.real) if k == 1 else (-x.real, -x.imag) if k == 2 \
        else (x.imag, -x.real)
    out = np.empty(x.shape, np.complex64)
    out.real, out.imag = re, im
    return out


def sensitive_channels(nr, nd, A, seed, F=1):
    """A complex64 [F][nr][nd] maps whose magnitudes are spread over 2^-12 .. 2^12, so that a float32
    sum over the cells depends on the order of its terms; channel a is channel 0 turned by 0.7 a rad
    with 10 % of independent disturbance."""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.uniform(-12, 12, (F, nr, nd)))
    ch0 = mag * np.exp(2j * np.pi * rng.random((F, nr, nd)))
    out = [ch0.astype(np.complex64)]
    for a in range(1, A):
        dist = 0.1 * mag * (rng.standard_normal((F, nr, nd)) + 1j * rng.standard_normal((F, nr, nd)))
        out.append((ch0 * np.exp(0.7j * a) + dist).astype(np.complex64))
    return out


def full_lists(nr, nd, K, F=1):
    """F frames of lists holding the first K cells of the map in raster order (ascending (r, d))."""
    assert K <= nr * nd
    i = np.arange(K)
    return dict(det_count=np.full(F, K, np.int32), det_range_idx=np.tile((i // nd + 1).astype(np.int32), (F, 1)),
                det_doppler_idx=np.tile((i % nd + 1).astype(np.int32), (F, 1)))


def dealt_labels(K, M, F=1):
    """Labels 1..M dealt over the list positions in turn."""
    return np.tile((np.arange(K) % M + 1).astype(np.int32), (F, 1))


def noisy_channels(rd0, psis, seed, level=0.05):
    """ch_0 = rd0, ch_a = rd0 e^{j psis[a]} plus complex noise at `level` of the map's RMS; complex64."""
    rng = np.random.default_rng(seed)
    rd0 = np.asarray(rd0, np.complex128)
    rms = np.sqrt(np.mean(np.abs(rd0) ** 2))
    out = [rd0.astype(np.complex64)]
    for psi in psis[1:]:
        noise = level * rms * np.sqrt(0.5) * (rng.standard_normal(rd0.shape) + 1j * rng.standard_normal(rd0.shape))
        out.append((rd0 * np.exp(1j * psi) + noise).astype(np.complex64))
    return out


# ---- 2. the reference's own conditions -----------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
def test_quarter_turns_are_exact(k):
    """ch1 = ch0 j^k with unit weights: z is exactly (S, 0), (0, S), (-S, +0), (0, -S), S = the energy
    sum, and the phase is float32 0, pi/2, pi, -pi/2 -- per cell and per target."""
    nr, nd, K = 64, 16, 300
    ch0 = sensitive_channels(nr, nd, 1, 11)[0]
    q = P.AoaConfig(n_chan=2, spacing=0.5, max_tgt=4)
    det = full_lists(nr, nd, K)
    ref = R.reference_of([ch0, quarter_turn(ch0, k)], det, q, labels=dealt_labels(K, 4))
    for pre, e in (("det", None), ("tgt", ref["tgt_e0"])):
        zr, zi = ref[pre + "_zre"], ref[pre + "_zim"]
        if e is None:                                        # one cell: its own |x|^2, as the reference rounds it
            re, im = R.stored(ch0)
            e = (re * re + im * im)[:, :K // nd + 1].reshape(1, -1)[:, :K]
        assert (e > 0).all()
        want = [(e, 0 * e), (0 * e, e), (-e, 0 * e), (0 * e, -e)][k]
        assert zr.tobytes() == want[0].astype(F32).tobytes() and zi.tobytes() == want[1].astype(F32).tobytes()
        assert not np.signbit(zr[zr == 0]).any() and not np.signbit(zi[zi == 0]).any()
        phase = F32([0, np.pi / 2, np.pi, -np.pi / 2][k])
        assert (ref[pre + "_phase"] == phase).all()
    np.testing.assert_array_equal(ref["tgt_e0"], ref["tgt_e1"])
    np.testing.assert_array_equal(ref["tgt_cells"], [[75, 75, 75, 75]])


def test_a_weight_undoes_a_rotation():
    nr, nd, K = 64, 16, 128
    ch0 = sensitive_channels(nr, nd, 1, 12)[0]
    det, lab = full_lists(nr, nd, K), dealt_labels(K, 3)
    turned = R.reference_of([ch0, quarter_turn(ch0, 1)], det, P.AoaConfig(max_tgt=3, weights=(1, -1j)), labels=lab)
    plain = R.reference_of([ch0, ch0], det, P.AoaConfig(max_tgt=3), labels=lab)
    for k in ("det_zre", "det_zim", "det_phase", "tgt_zre", "tgt_zim", "tgt_e0", "tgt_e1", "tgt_phase", "tgt_coh"):
        assert turned[k].tobytes() == plain[k].tobytes(), k
    assert (plain["tgt_phase"] == 0).all() and (plain["det_zim"] == 0).all()


@pytest.mark.parametrize("A", [2, 3, 8])
def test_float32_sums_stay_within_the_bound_of_the_float64_ones(A):
    """|Z32 - Z64| <= (N + 8) 2^-23 sum |terms| (tests/aoa_reference.py derives (N + 9) 2^-24)."""
    nr, nd, K, M = 64, 16, 1024, 5
    chans = sensitive_channels(nr, nd, A, 20 + A)
    q = P.AoaConfig(n_chan=A, max_tgt=M, weights=tuple(np.exp(0.3j * a) * (1 + 0.1 * a) for a in range(A)))
    det, lab = full_lists(nr, nd, K), dealt_labels(K, M)
    r32 = R.reference_of(chans, det, q, labels=lab)
    r64 = R.reference_of(chans, det, q, labels=lab, ftype=np.float64)
    n = r32["tgt_terms_n"].astype(np.float64)
    assert n.min() >= (A - 1) * (K // M)
    for k, row in (("tgt_zre", 0), ("tgt_zim", 0), ("tgt_e0", 1), ("tgt_e1", 2)):
        err = np.abs(r32[k].astype(np.float64) - r64[k])
        assert np.all(err <= (n + 8) * 2.0 ** -23 * r32["terms_tgt"][row]), k
        assert err.max() > 0                                  # the comparison is not vacuous
    for k, row in (("det_zre", 0), ("det_zim", 0)):
        err = np.abs(r32[k].astype(np.float64) - r64[k])
        assert np.all(err <= (A - 1 + 8) * 2.0 ** -23 * r32["terms_det"][row]), k


def test_coherence_clamp():
    """Raw coherence exceeds 1 by rounding only; where it does, the clamp gives exactly 1."""
    nr, nd, K, M = 64, 16, 1024, 64
    ch0 = sensitive_channels(nr, nd, 1, 31)[0]
    det, lab = full_lists(nr, nd, K), dealt_labels(K, M)
    over = 0
    for k in range(4):
        for seed in range(4):
            x = sensitive_channels(nr, nd, 1, 40 + seed)[0]
            ref = R.reference_of([x, quarter_turn(x, k)], det, P.AoaConfig(max_tgt=M), labels=lab)
            raw, coh = ref["tgt_coh_raw"], ref["tgt_coh"]
            assert raw.max() <= 1 + 4 * 2.0 ** -23 and raw.min() >= 1 - 4 * 2.0 ** -23
            assert coh.max() == 1 and coh.dtype == F32
            assert (coh[raw > 1] == 1).all()
            over += int((raw > 1).sum())
    assert over > 0
    # incoherent channels: well below 1; an empty target: 0
    ref = R.reference_of([ch0, sensitive_channels(nr, nd, 1, 32)[0]], det, P.AoaConfig(max_tgt=M), labels=lab % 63)
    assert 0 < ref["tgt_coh"][0, :62].max() < 1 and ref["tgt_coh"][0, 62:].tolist() == [0, 0]


def test_the_constructed_values_are_order_sensitive():
    """Summing a target's cells in reverse list order changes bits of Z: the GPU tests that use these
    values can see a wrong order."""
    nr, nd, M = 64, 16, 64
    for K in (63, 64, 65, 256, 1024):
        for A in (2, 8):
            chans = sensitive_channels(nr, nd, A, 5)
            det = full_lists(nr, nd, K)
            q = P.AoaConfig(n_chan=A, max_tgt=M)
            for lab in (np.ones((1, K), np.int32), dealt_labels(K, M)):
                fwd = R.reference_of(chans, det, q, labels=lab)
                # the same cells listed backwards (the reference sums in list order, whatever it is)
                rev = {k: (v if k == "det_count" else np.ascontiguousarray(v[:, ::-1])) for k, v in det.items()}
                bwd = R.reference_of(chans, rev, q, labels=np.ascontiguousarray(lab[:, ::-1]))
                np.testing.assert_array_equal(fwd["tgt_cells"], bwd["tgt_cells"])
                many = fwd["tgt_cells"] > 2
                if not many.any():
                    continue
                differ = sum(int((fwd[k][many] != bwd[k][many]).sum()) for k in ("tgt_zre", "tgt_zim", "tgt_e0", "tgt_e1"))
                assert differ > 0, (K, A)


# ---- 3. physics ----------------------------------------------------------------------------------------
_CPU = {}


def cpu_lists(geo):
    """The CFAR reference's detections (pfa 1e-3, gate 3..nr-2) of the oracle's RD map of the geometry,
    as lists, and the clustering reference's labels (link (1, 1), min_cells 1, max_tgt 64); made once."""
    from tests.test_gpu_cfar import cfg_for, rd_map
    if geo not in _CPU:
        rd = rd_map(geo)
        nr, nd = geo[2:]
        q = cfg_for(nr, 1e-3)
        ref = CR.cfar_reference(rd, (q.guard_r, q.guard_d), (q.train_r, q.train_d), q.alpha, q.r_lo, q.r_hi, False)
        frames = [lists_of_mask(ref["det"][f], ref["P"][f].astype(F32)) for f in range(len(rd))]
        det = {k: np.concatenate([fr[k] for fr in frames]) for k in frames[0]}
        lab = CL.reference_of(det, P.ClusterConfig(link_r=1, link_d=1, min_cells=1, max_tgt=64), nd)["det_label"]
        _CPU[geo] = (rd, det, lab.astype(np.int32))
    return _CPU[geo]


@pytest.mark.parametrize("geo", [(64, 16, 256, 16), (100, 20, 128, 32)], ids=lambda g: "x".join(map(str, g)))
def test_the_phase_between_the_channels_is_recovered(geo):
    """ch_a = ch0 e^{j psi a} plus noise at 5 % of the RMS: the median target phase is within 0.01 rad
    of psi, for two channels and for a line of three (psi 0.9, seed 7: 0.900 / 0.899 at 256 x 16,
    0.898 / 0.900 at 128 x 32).  The third small geometry, 256 x 32, is left to the test below: of its
    74 targets at pfa 1e-3 most are false alarms far below this noise, their phases spread over the
    whole circle (quartiles -0.2 and 1.5 rad), and the median over all of them is 0.883, 0.899 and
    0.554 for seeds 7, 8 and 9 -- it measures the draw, not the estimator."""
    rd, det, lab = cpu_lists(geo)
    psi = 0.9
    for A in (2, 3):
        chans = noisy_channels(rd, [psi * a for a in range(A)], seed=7)
        ref = R.reference_of(chans, det, P.AoaConfig(n_chan=A, spacing=0.5, max_tgt=64), labels=lab)
        used = ref["tgt_cells"] > 0
        assert used.sum() >= len(rd)
        med = float(np.median(ref["tgt_phase"][used]))
        print(f"median target phase at {geo[2]} x {geo[3]}, A = {A}: {med:.4f}")
        assert abs(med - psi) <= 0.01
        # sin(theta) = phase / (2 pi spacing)
        np.testing.assert_array_equal(ref["tgt_sin"], R.sin_of(ref["tgt_phase"], F32(1 / np.pi)))


@pytest.mark.parametrize("geo", [(64, 16, 256, 16), (100, 20, 128, 32), (256, 32, 256, 32)],
                         ids=lambda g: "x".join(map(str, g)))
def test_the_strongest_target_gives_the_phase(geo):
    """The strongest target of a frame (place 1 of the clustering order) against the same noise.  With
    noise of standard deviation s on channel 1 alone, z = sum x1 conj(x0) has the phase error
    Im(sum n conj(x0) e^{-j psi}) / sum |x0|^2, of standard deviation s / sqrt(2 sum |x0|^2): the
    target is held to five of them, and is coherent."""
    rd, det, lab = cpu_lists(geo)
    psi, level = 0.9, 0.05
    chans = noisy_channels(rd, [0, psi], seed=7, level=level)
    ref = R.reference_of(chans, det, P.AoaConfig(n_chan=2, spacing=0.5, max_tgt=64), labels=lab)
    s = level * np.sqrt(np.mean(np.abs(rd.astype(np.complex128)) ** 2))
    have = ref["tgt_cells"][:, 0] > 0
    assert have.sum() >= len(rd) - 1
    tol = 5 * s / np.sqrt(2 * ref["tgt_e0"][have, 0].astype(np.float64))
    err = np.abs(ref["tgt_phase"][have, 0] - psi)
    print(f"strongest target at {geo[2]} x {geo[3]}: phase error at most {err.max():.2e} rad, bound at least {tol.min():.2e}")
    assert np.all(err <= tol) and np.median(tol) < 0.01
    assert ref["tgt_coh"][have, 0].min() > 0.99
