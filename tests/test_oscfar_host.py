"""CPU: the host-side half of the 2-D OS-CFAR stage (include/fmcw.h, fmcw_oscfar_params) -- the
argument rules and the alpha rule -- and a self-check that pins the float32 reference the GPU tests
compare against (tests/oscfar_reference.py): its two forms of the test, the clipped ranks, ties, the
masking scenario that cell averaging loses, and the false-alarm rate the alpha rule promises."""
import ctypes as ct
import math

import numpy as np
import pytest

from fmcw_radar_processing_amd import _lib
from fmcw_radar_processing_amd import params as P
from tests import cfar_reference as CA
from tests import oscfar_reference as R
from tests.test_cfar_host import REJECTED


def _q(rank=30, **over):
    d = dict(guard_r=1, guard_d=1, train_r=2, train_d=2, r_lo=0, r_hi=0, max_det=64, flags=0, alpha=7.54)
    d.update(over)
    return _lib.OsCfarParams(_lib.CfarParams(*[d[k] for k, _ in _lib.CfarParams._fields_]), rank)


def _pfa(n, k, alpha):
    """The product formula in double precision."""
    return math.exp(sum(math.log(n - i) - math.log(n - i + alpha) for i in range(k)))


def test_check_accepts_and_counts_the_full_window():
    lib = _lib.load()
    n = ct.c_int32(-1)
    for rank in (1, 20, 40):
        q = _q(rank)
        assert lib.fmcw_oscfar_check(ct.byref(q), 256, 16, ct.byref(n)) == _lib.FMCW_OK
        assert n.value == 40 == P.OsCfarConfig().n_train_full
    q = _q(800, guard_r=8, guard_d=8, train_r=8, train_d=8)
    assert lib.fmcw_oscfar_check(ct.byref(q), 1024, 256, ct.byref(n)) == _lib.FMCW_OK
    assert n.value == 33 * 33 - 17 * 17
    assert lib.fmcw_oscfar_check(ct.byref(q), 1024, 256, None) == _lib.FMCW_OK
    assert lib.fmcw_oscfar_check(None, 1024, 256, None) == _lib.FMCW_E_ARG


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_check_rejects_what_ca_rejects(name):
    lib = _lib.load()
    over, nr, nd = REJECTED[name]
    q = _q(1, **over)
    n = ct.c_int32(-1)
    assert lib.fmcw_oscfar_check(ct.byref(q), nr, nd, ct.byref(n)) == _lib.FMCW_E_ARG
    assert len(lib.fmcw_last_error()) > 8 and n.value == -1


@pytest.mark.parametrize("rank", [0, 41, -1])
def test_check_rejects_a_rank_outside_the_window(rank):
    lib = _lib.load()
    n = ct.c_int32(-1)
    q = _q(rank)
    assert lib.fmcw_oscfar_check(ct.byref(q), 256, 16, ct.byref(n)) == _lib.FMCW_E_ARG
    assert b"rank" in lib.fmcw_last_error() and n.value == -1


def test_null_context_or_parameters_are_argument_errors():
    lib = _lib.load()
    q = _q()
    assert lib.fmcw_oscfar(None, ct.byref(q), None, 0, 1, 256, 16, *([None] * 6)) == _lib.FMCW_E_ARG
    assert lib.fmcw_oscfar_device(None, ct.byref(q), None, 0, 1, 256, 16, *([None] * 7)) == _lib.FMCW_E_ARG
    assert lib.fmcw_oscfar_check(None, 256, 16, None) == _lib.FMCW_E_ARG


def test_alpha_rule():
    lib = _lib.load()
    a = ct.c_float()
    # closed forms: N = 1, and k = 1 (the smallest of N exponentials is an exponential of mean 1 / N)
    for pfa in (1e-2, 1e-4, 1e-6):
        assert lib.fmcw_oscfar_alpha(1, 1, pfa, ct.byref(a)) == _lib.FMCW_OK
        assert a.value == pytest.approx(1 / pfa - 1, rel=1e-6)
        for n in (2, 40, 1088):
            assert lib.fmcw_oscfar_alpha(n, 1, pfa, ct.byref(a)) == _lib.FMCW_OK
            assert a.value == pytest.approx(n * (1 / pfa - 1), rel=1e-6)
    # the product formula at the returned float: rounding alpha to float moves ln pfa by about k 2^-24
    for n, k, pfa in ((72, 54, 1e-4), (40, 30, 1e-3), (40, 40, 1e-5), (1088, 816, 1e-6), (1088, 1088, 1e-2),
                      (144, 108, 1e-6), (8, 4, 0.5)):
        assert lib.fmcw_oscfar_alpha(n, k, pfa, ct.byref(a)) == _lib.FMCW_OK
        assert a.value > 0 and _pfa(n, k, a.value) == pytest.approx(pfa, rel=1e-4)
        assert P.OsCfarConfig.alpha_for(n, k, pfa) == a.value
    for n, k, pfa in ((0, 1, 1e-3), (-1, 1, 1e-3), (40, 0, 1e-3), (40, 41, 1e-3), (40, 20, 0.0), (40, 20, 1.0),
                      (40, 20, -0.1), (40, 20, 1.5), (40, 20, float("nan"))):
        assert lib.fmcw_oscfar_alpha(n, k, pfa, ct.byref(a)) == _lib.FMCW_E_ARG
    assert lib.fmcw_oscfar_alpha(40, 20, 1e-3, None) == _lib.FMCW_E_ARG


def test_config_carries_the_rank():
    from tests.helpers import case
    cfg, *_ = case(64, 16, 256, 16)
    q = P.OsCfarConfig.for_config(cfg, pfa=1e-5, guard=(1, 2), train=(3, 4), max_det=9, local_max=True)
    c = P.CfarConfig.for_config(cfg, pfa=1e-5, guard=(1, 2), train=(3, 4), max_det=9, local_max=True)
    assert (q.r_lo, q.r_hi, q.n_train_full) == (c.r_lo, c.r_hi, c.n_train_full)
    assert q.rank == (3 * q.n_train_full) // 4 and q.alpha == P.OsCfarConfig.alpha_for(q.n_train_full, q.rank, 1e-5)
    assert P.OsCfarConfig.for_config(cfg, rank_share=0.0).rank == 1
    a = q.abi()
    assert (a.win.r_lo, a.win.r_hi, a.win.flags, a.win.max_det, a.rank) == (q.r_lo, q.r_hi, 1, 9, q.rank)
    assert a.win.alpha == np.float32(q.alpha)
    assert _lib.load().fmcw_oscfar_check(ct.byref(a), cfg.nr, cfg.nd, None) == _lib.FMCW_OK
    assert "oscfar" in _lib.STAGES and _lib.STAGES.index("oscfar") == 16


def _noise(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def test_reference_self_check():
    """The two forms agree on every cell (asserted inside decide), the clipped ranks are the ones
    worked out by hand, and a brute-force visit of every training cell gives the same X_(k) and the
    same decision."""
    nr, nd, (gr, gd), (tr, td) = 64, 32, (1, 1), (3, 3)
    x = _noise((2, nr, nd), 3)
    x[0, 20, 5] += 30
    x[1, 0, 0] += 30
    x[1, nr - 1, nd - 1] += 30
    w = R.OsWindow(x, (gr, gd), (tr, td))
    assert w.n_full == 72
    alpha = P.OsCfarConfig.alpha_for(72, 54, 1e-2)
    ref = w.decide(alpha, 54)
    # rows 0..4: a missing outer row takes 9 cells away, a missing guard row 6
    assert ref["N"][:5].tolist() == [39, 45, 54, 63, 72] and ref["N"][-5:].tolist() == [72, 63, 54, 45, 39]
    assert ref["k"][:5].tolist() == [29, 33, 40, 47, 54] and ref["k"][nr - 1] == 29
    assert w.decide(alpha, 1)["k"].tolist() == [1] * nr and np.array_equal(w.decide(alpha, 72)["k"], ref["N"])
    assert ref["det"][0, 20, 5] and ref["det"][1, 0, 0] and ref["det"][1, nr - 1, nd - 1]
    Wr, Wd = gr + tr, gd + td
    a32 = np.float32(alpha)
    for f, r, d in [(0, 0, 0), (0, 0, nd - 1), (0, nr - 1, 0), (0, nr - 1, nd - 1), (0, 20, 5), (1, 0, 0), (1, 2, 31),
                    (1, 33, 16), (1, nr - 1, nd - 1)]:
        cells = [(r + dr, (d + dd) % nd) for dr in range(-Wr, Wr + 1) for dd in range(-Wd, Wd + 1)
                 if not (abs(dr) <= gr and abs(dd) <= gd) and 0 <= r + dr < nr]
        assert len(cells) == ref["N"][r] and len(set(cells)) == len(cells)
        xs = sorted(w.P[f, a, b] for a, b in cells)
        k = ref["k"][r]
        assert ref["noise"][f, r, d] == xs[k - 1]
        below = sum(1 for v in xs if a32 * v < w.P[f, r, d])
        assert ref["det"][f, r, d] == (below >= k) == bool(w.P[f, r, d] > a32 * xs[k - 1])
    # the gate and LOCAL_MAX only take detections away
    g = w.decide(alpha, 54, 3, nr - 2)
    assert not g["det"][:, :2].any() and not g["det"][:, nr - 2:].any()
    np.testing.assert_array_equal(g["det"][:, 2:nr - 2], ref["det"][:, 2:nr - 2])
    lm = w.decide(alpha, 54, local_max=True)
    assert not (lm["det"] & ~ref["det"]).any() and lm["det"][0, 20, 5]
    out = R.lists(ref, 4)
    assert out["det_count"][1] == ref["det"][1].sum() >= 2
    assert (out["det_range_idx"][1, 0], out["det_doppler_idx"][1, 0]) == (1, 1)
    assert out["det_power"].dtype == np.float32 and out["det_noise"][1, 0] == ref["noise"][1, 0, 0]


def test_reference_with_ties_and_zeros():
    """A map of 7 distinct powers: the count form and the sorted form still agree on every cell
    (ties included), and the noise is one of the 7.  An all-zero map detects nothing."""
    rng = np.random.default_rng(11)
    amp = rng.integers(0, 7, (2, 32, 16)).astype(np.float32)
    x = (amp + 0j).astype(np.complex64)
    w = R.OsWindow(x, (0, 1), (2, 1))
    assert len(np.unique(w.P)) == 7
    for rank in (1, w.n_full // 2, w.n_full):
        for alpha in (0.5, 1.0, 3.0):
            ref = w.decide(alpha, rank)                      # asserts the two forms equal
            assert set(np.unique(ref["noise"])) <= set(np.unique(w.P))
    assert w.decide(0.5, 1)["det"].any() and not w.decide(0.5, 1)["det"][w.P == 0].any()
    z = R.oscfar_reference(np.zeros((1, 16, 8), np.complex64), (1, 1), (1, 1), 2.0, 3)
    assert not z["det"].any() and not z["noise"].any()


@pytest.mark.parametrize("weak_db", [14, 16, 18, 20])
def test_masking_ca_misses_what_os_finds(weak_db):
    """8 frames of 64 x 32 unit noise, two 40 dB targets and a weak one with the first strong target
    in its training window; guard (1, 1), train (3, 3), N = 72, pfa 1e-4 for both detectors.  The
    cell-averaging threshold of the weak cell carries 10^4 / 72 from the strong one: it misses in
    every frame, with no exempt cell.  OS with rank 54 finds it in every frame."""
    s = R.SCENE
    x = R.masking_scene(weak_db)
    r, d = R.scene_cells()["weak"]
    ca = CA.cfar_reference(x, s["guard"], s["train"], P.CfarConfig.alpha_for(72, s["pfa"]))
    assert CA.check_exempt(ca) == 0
    assert ca["det"][:, r, d].sum() == 0
    os_ = R.oscfar_reference(x, s["guard"], s["train"], P.OsCfarConfig.alpha_for(72, s["rank"], s["pfa"]), s["rank"])
    assert os_["det"][:, r, d].sum() == s["F"]
    for rr, dd in R.scene_cells()["strong"]:
        assert ca["det"][:, rr, dd].all() and os_["det"][:, rr, dd].all()


def test_masking_scene_holds_nothing_but_its_targets():
    """What the device test of Engine.targets relies on: in the 14 dB scene CA-CFAR detects exactly the
    two strong cells of every frame and OS-CFAR exactly the three targets."""
    s = R.SCENE
    x = R.masking_scene(14)
    ca = CA.cfar_reference(x, s["guard"], s["train"], P.CfarConfig.alpha_for(72, s["pfa"]))
    os_ = R.oscfar_reference(x, s["guard"], s["train"], P.OsCfarConfig.alpha_for(72, s["rank"], s["pfa"]), s["rank"])
    assert ca["det"].sum(axis=(1, 2)).tolist() == [2] * s["F"]
    assert os_["det"].sum(axis=(1, 2)).tolist() == [3] * s["F"]


def test_false_alarm_rate_is_the_design_value():
    """Noise only, full windows only (rows Wr .. nr - 1 - Wr), design pfa 1e-2: the reference's rate
    over more than 100 000 cells is within 10 % of it.  This guards the alpha formula."""
    x = _noise((4, 128, 256), 5)
    alpha = P.OsCfarConfig.alpha_for(72, 54, 1e-2)
    ref = R.oscfar_reference(x, (1, 1), (3, 3), alpha, 54, 5, 124)
    cells = 4 * 120 * 256
    rate = ref["det"].sum() / cells
    assert cells >= 100_000 and ref["N"][4:124].min() == 72
    assert abs(rate - 1e-2) <= 1e-3, rate
