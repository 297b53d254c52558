"""CPU: the direction-of-arrival stage's reference (tests/doa_reference.py, the steps of
include/fmcw.h as plain loops) on the rows that force every branch of the definition, against the
project's own peak helper on the Bartlett, Capon and MUSIC scenarios, the prominence rule on noise
rows, the sub-grid directions of sources between grid points; and every rule and message of
fmcw_doa_check and DoaConfig.  The device is compared with this reference byte for byte in
tests/test_gpu_doa.py."""
import ctypes as ct
import functools

import numpy as np
import pytest

from fmcw_radar_processing_amd import DoaConfig, _lib
from fmcw_radar_processing_amd.engine import Engine
from tests import doa_reference as D
from tests import music_reference as M
from tests import ra_reference as R

F32 = np.float32
S = R.SCENE


# ---- 1. the pool hits every branch -------------------------------------------------------------------------
def test_the_pool_hits_every_branch_of_the_definition():
    """Every branch the reference can take is taken on the pool, under the flags and thresholds the GPU
    grid uses; the clamp of step 5 among them, both ways (the halving of num rounds when l - r is an
    odd number of denormal units)."""
    D.reset_hits()
    for K in (3, 4, 7, 64, 65):
        spec = D.row_pool(K)[None]
        u = D.grid(K)
        for flags in (0, D.EDGES, D.WRAP, D.INV, D.EDGES | D.INV, D.WRAP | D.INV):
            for max_pk, (ma, mr, mp) in ((3, (0.0, 0.0, 0.0)), (1, (1.0, 0.25, 4.0)), (8, (0.0, 0.25, 4.0))):
                D.doa_reference(spec, u, max_pk, flags, ma, mr, mp)
    hits = {b: D.HITS[b] for b in D.BRANCHES}
    print(hits)
    assert set(D.HITS) <= set(D.BRANCHES)
    assert all(n > 0 for n in hits.values()), [b for b, n in hits.items() if n == 0]


def test_pool_rows_answer_as_written():
    """A few rows by hand: the first point of a flat top, a flat stretch that rises, the seam."""
    u = np.linspace(-1, 1, 6).astype(F32)
    row = np.array([[[1, 4, 4, 1, 2, 2]]], F32)                               # flat top at 1..2; 4..5 runs into the end
    assert D.idx_set(D.doa_reference(np.repeat(row, 16, 1), u, 4), 0, 0) == {1}
    assert D.idx_set(D.doa_reference(np.repeat(row, 16, 1), u, 4, D.EDGES), 0, 0) == {1, 4}
    assert D.idx_set(D.doa_reference(np.repeat(row, 16, 1), u, 4, D.WRAP), 0, 0) == {1, 4}
    row = np.array([[[1, 3, 3, 5, 2, 2]]], F32)                               # 1..2 rises afterwards: no peak
    out = D.doa_reference(np.repeat(row, 16, 1), u, 4)
    assert D.idx_set(out, 0, 0) == {3} and out["base"][0, 0, 0] == 2 and out["count"][0, 0] == 1
    d = D.DEN                                                                 # the clamp: den = -3u, num = fl(-1.5u) = -2u
    for m in (0.0, D.TINY):
        row = np.array([[[m, m, m, m + 3 * d, m + 3 * d, m]]], F32)
        out = D.doa_reference(np.repeat(row, 16, 1), u, 4)
        assert out["idx"][0, 0, 0] == 3 and out["sin"][0, 0, 0] == u[3] + F32(0.5) * (u[4] - u[3])
    row = np.array([[[7, 1, 2, 1, 1, 7]]], F32)                               # the flat top K-1, 0 across the seam
    out = D.doa_reference(np.repeat(row, 16, 1), u, 4, D.WRAP)
    assert out["idx"][0, 0].tolist() == [5, 2, -1, -1] and out["base"][0, 0].tolist() == [1, 1, 0, 0]
    assert out["sin"][0, 0, 0] == u[5] + F32(0.5) * (u[5] - u[4])             # delta = +0.5 across the seam: the step before k
    gated = D.doa_reference(np.repeat(row, 16, 1), u, 4, D.WRAP, r_lo=3, r_hi=9)
    assert (gated["count"][0, 2:9] == 2).all() and not gated["count"][0, :2].any() and not gated["count"][0, 9:].any()
    assert (gated["idx"][0, :2] == -1).all() and not gated["pow"][0, 9:].view(np.uint32).any()


# ---- 2. agreement with the project's helper ----------------------------------------------------------------
def _weights():
    return R.weights_f32(Engine.ra_weights(S["A"], R.scene_sines(), S["spacing"]))


def _cov(chans):
    return R.cov_reference(chans, S["dc_half"])[0].astype(F32)


@functools.lru_cache(maxsize=None)
def spectra(which):
    w = _weights()
    if which == "bartlett":
        return R.spectra_reference(_cov(R.scene()), w)[0]
    if which == "capon":
        return R.spectra_reference(_cov(R.scene()), w, True, S["load"])[0]
    if which == "music_close":
        return M.music_reference(_cov(M.close_scene(M.CLOSE_SEED)), w, n_src=2)["music"]
    return M.music_reference(_cov(M.coherent_scene(M.COHERENT_SEED)), w, n_src=2, fb=True)["music"]


FIGURES = {"capon": {32, 37}, "music_close": {32, 35}, "music_coherent": {32, 37}}       # the README's, in 8 of 8 frames


@pytest.mark.parametrize("which", ["bartlett", "capon", "music_close", "music_coherent"])
def test_agrees_with_the_projects_peak_helper(which):
    """EDGES, min_rel = 0.25, min_prom = 0: in every row free of equal neighbours and of a value
    exactly on the threshold, count is the number of ra_reference.peaks(row, 0.25) and the written
    grid points are those peaks (the strongest max_pk of them where there are more)."""
    spec = spectra(which)
    u = R.scene_sines()
    max_pk = 8
    out = D.doa_reference(spec, u, max_pk, D.EDGES, 0.0, 0.25, 0.0)
    compared = 0
    for f in range(spec.shape[0]):
        for r in range(spec.shape[1]):
            row = spec[f, r]
            if (row[1:] == row[:-1]).any() or (row == F32(0.25) * row.max()).any():
                continue
            compared += 1
            pk = R.peaks(row, 0.25)
            assert out["count"][f, r] == len(pk), (f, r)
            strongest = sorted(pk, key=lambda k: (-float(row[k]), k))[:max_pk]
            assert out["idx"][f, r, :len(strongest)].tolist() == strongest, (f, r)
    assert compared >= spec.shape[0] * spec.shape[1] - 2, compared
    if which in FIGURES:
        sets = [D.idx_set(out, f, S["row"]) for f in range(S["frames"])]
        assert all(s == FIGURES[which] for s in sets), sets


# ---- 3. the prominence rule --------------------------------------------------------------------------------------
# Measured with the reference on the Bartlett spectra of ra_reference.scene(seed), EDGES, no thresholds
# (pow / base of every peak; 15 noise rows x 8 frames, the source row x 8 frames):
#   seed   noise rows, largest   source row, strongest peak per frame   source row, smallest (a sidelobe)
#    1          1.89                    63.5 .. 84.9                          1.11
#    2          1.78                    61.4 .. 81.4                          1.17
#    3          1.89                    68.8 .. 89.4                          1.13
#    4          1.75                    69.5 .. 82.9                          1.11
# Seeds 1..4 were tried.  Read as "the smallest pow / base of ANY peak of the source row" the two ranges
# overlap for every seed: the merged return's sidelobes are ripples like the noise rows' (1.1 .. 1.9).  The
# rule is there to drop exactly those, so the threshold sits between the noise rows' largest ratio and the
# source row's strongest peak, for seed 1: 1.89 < 8 < 63.5 (8 is exact in float32).
PROM_SEED, MIN_PROM = 1, 8.0


def test_prominence_rule_silences_the_noise_rows():
    """Without the rule every ripple of a noise row's Bartlett spectrum counts; with min_prom = 8 every
    one of the 15 noise rows counts 0 and the source row at least one peak, in 8 of 8 frames."""
    bart = R.spectra_reference(_cov(R.scene(PROM_SEED)), _weights())[0]
    u = R.scene_sines()
    free = D.doa_reference(bart, u, 8, D.EDGES)
    n = np.minimum(free["count"], 8)
    ratio = [[free["pow"][f, r, :n[f, r]].astype(np.float64) / free["base"][f, r, :n[f, r]] for r in range(S["nr"])]
             for f in range(S["frames"])]
    noise = max(ratio[f][r].max() for f in range(S["frames"]) for r in range(S["nr"]) if r != S["row"])
    strongest = [ratio[f][S["row"]].max() for f in range(S["frames"])]
    smallest = min(ratio[f][S["row"]].min() for f in range(S["frames"]))
    print(f"noise rows: largest pow/base {noise:.3f}; source row: strongest {min(strongest):.1f} .. {max(strongest):.1f}, "
          f"smallest {smallest:.3f}; counts without the rule {free['count'].min()} .. {free['count'].max()}")
    assert (free["count"] <= 8).all() and (np.delete(free["count"], S["row"], axis=1) >= 2).all()
    assert noise < MIN_PROM < min(strongest)
    out = D.doa_reference(bart, u, 8, D.EDGES, 0.0, 0.0, MIN_PROM)
    assert not np.delete(out["count"], S["row"], axis=1).any()
    assert (out["count"][:, S["row"]] >= 1).all(), out["count"][:, S["row"]]


# ---- 4. sub-grid directions ---------------------------------------------------------------------------------------
# Measured with the references on doa_reference.offgrid_scene(1) (sources at grid points 32.25 and 37.5,
# sin(theta) = 0.0078125 and 0.171875; the grid step is 0.03125), EDGES, min_rel = 0.25, over the 8
# frames: |sin - truth| mean / max, against |u[idx] - truth| of the bare grid point (0.00781 and 0.01562):
#                      source at 32.25            source at 37.5
#   Capon  plain     0.00276 / 0.00564          0.00694 / 0.01234
#   Capon  INV       0.00310 / 0.00721          0.00478 / 0.00957
#   MUSIC  plain     0.00589 / 0.00741          0.00882 / 0.01374
#   MUSIC  INV       0.00241 / 0.00583          0.00349 / 0.00845
# The refined direction is nearer the truth than the grid point in 8 of 8 frames in all eight cells: that
# count is the floor below.  INV more than halves MUSIC's mean error; for Capon it helps the half-step
# source and not the quarter-step one, so nothing is asserted about INV against plain.
NEARER_FLOOR = 8


@pytest.mark.parametrize("inv", [False, True], ids=["plain", "inv"])
@pytest.mark.parametrize("method", ["capon", "music"])
def test_sub_grid_direction_is_nearer_than_the_grid_point(method, inv):
    cov = _cov(D.offgrid_scene(1))
    w = _weights()
    u = R.scene_sines()
    spec = R.spectra_reference(cov, w, True, S["load"])[0] if method == "capon" else M.music_reference(cov, w, n_src=2)["music"]
    out = D.doa_reference(spec, u, 4, D.EDGES | (D.INV if inv else 0), 0.0, 0.25, 0.0)
    truths = [(k - 32) / 32.0 for k in D.OFFGRID_POINTS]
    err = np.array([D.direction_errors(out, u, f, S["row"], truths) for f in range(S["frames"])])     # [frame][source][refined, grid]
    for s in range(2):
        nearer = int((err[:, s, 0] < err[:, s, 1]).sum())
        print(f"{method} {'INV' if inv else 'plain'} source {s}: refined mean {err[:, s, 0].mean():.5f} max {err[:, s, 0].max():.5f}, "
              f"grid mean {err[:, s, 1].mean():.5f} max {err[:, s, 1].max():.5f}, nearer in {nearer} of 8")
        assert nearer >= NEARER_FLOOR


def test_positions():
    out = {"idx": np.array([[[3, -1]]], np.int32), "sin": np.array([[[0.6, 0.0]]], F32)}
    x, y = Engine.doa_positions(out, [10.0])
    assert x.dtype == np.float64 and np.isnan(x[0, 0, 1]) and np.isnan(y[0, 0, 1])
    np.testing.assert_allclose([x[0, 0, 0], y[0, 0, 0]], [6.0, 8.0], rtol=1e-6)


# ---- 5. the argument rules: fmcw_doa_check and DoaConfig agree, rule by rule -------------------------------------
def _q(**over):
    kw = dict(n_ang=16, r_lo=0, r_hi=0, max_pk=4, flags=0, min_abs=0.0, min_rel=0.0, min_prom=0.0)
    kw.update(over)
    return _lib.DoaParams(*[kw[k] for k in ("n_ang", "r_lo", "r_hi", "max_pk", "flags", "min_abs", "min_rel", "min_prom")])


# name -> (overrides, nr, message)
REJECTED = {
    "nr_small": ({}, 8, "doa: nr must be a power of two in [16, 2048]"),
    "nr_not_pow2": ({}, 24, "doa: nr must be a power of two in [16, 2048]"),
    "nr_large": ({}, 4096, "doa: nr must be a power of two in [16, 2048]"),
    "gate_reversed": (dict(r_lo=5, r_hi=3), 64, "doa: r_lo > r_hi"),
    "gate_half_zero": (dict(r_lo=0, r_hi=5), 64, "doa: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
    "gate_past_nr": (dict(r_lo=1, r_hi=65), 64, "doa: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
    "n_ang_0": (dict(n_ang=0), 64, "doa: n_ang must be in [1, 256]"),
    "n_ang_257": (dict(n_ang=257), 64, "doa: n_ang must be in [1, 256]"),
    "max_pk_0": (dict(max_pk=0), 64, "doa: max_pk must be in [1, 8]"),
    "max_pk_9": (dict(max_pk=9), 64, "doa: max_pk must be in [1, 8]"),
    "flag_unknown": (dict(flags=8), 64, "doa: unknown flag bits"),
    "edges_and_wrap": (dict(flags=3), 64, "doa: FMCW_DOA_EDGES and FMCW_DOA_WRAP exclude each other"),
    "wrap_n_ang_2": (dict(flags=2, n_ang=2), 64, "doa: FMCW_DOA_WRAP needs n_ang >= 3"),
    "min_abs_negative": (dict(min_abs=-1.0), 64, "doa: min_abs must be finite and >= 0"),
    "min_abs_nan": (dict(min_abs=float("nan")), 64, "doa: min_abs must be finite and >= 0"),
    "min_abs_inf": (dict(min_abs=float("inf")), 64, "doa: min_abs must be finite and >= 0"),
    "min_rel_negative": (dict(min_rel=-0.5), 64, "doa: min_rel must be in [0, 1]"),
    "min_rel_above_1": (dict(min_rel=1.5), 64, "doa: min_rel must be in [0, 1]"),
    "min_rel_nan": (dict(min_rel=float("nan")), 64, "doa: min_rel must be in [0, 1]"),
    "min_prom_negative": (dict(min_prom=-1.0), 64, "doa: min_prom must be finite and >= 0"),
    "min_prom_nan": (dict(min_prom=float("nan")), 64, "doa: min_prom must be finite and >= 0"),
    "min_prom_inf": (dict(min_prom=float("inf")), 64, "doa: min_prom must be finite and >= 0"),
}


def _config(over):
    kw = dict(n_ang=16, r_lo=0, r_hi=0, max_pk=4, min_abs=0.0, min_rel=0.0, min_prom=0.0)
    kw.update({k: v for k, v in over.items() if k != "flags"})
    fl = over.get("flags", 0)
    return DoaConfig(edges=bool(fl & 1), wrap=bool(fl & 2), inv=bool(fl & 4), **kw)


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_rejected(name):
    over, nr, msg = REJECTED[name]
    lib = _lib.load()
    assert lib.fmcw_doa_check(ct.byref(_q(**over)), nr) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error().decode() == msg
    if name != "flag_unknown":                    # DoaConfig has no way to set an unknown bit
        with pytest.raises(ValueError) as e:
            _config(over).check(nr)
        assert str(e.value) == msg


def test_accepted():
    lib = _lib.load()
    for over, nr in ((dict(), 64), (dict(n_ang=1), 16), (dict(n_ang=256, max_pk=8), 2048), (dict(max_pk=1), 64),
                     (dict(r_lo=7, r_hi=7), 64), (dict(r_lo=1, r_hi=64), 64), (dict(flags=1, n_ang=2), 64),
                     (dict(flags=2, n_ang=3), 64), (dict(flags=4), 64), (dict(flags=5), 64), (dict(flags=6), 64),
                     (dict(min_abs=1e30, min_rel=1.0, min_prom=1e30), 64)):
        assert lib.fmcw_doa_check(ct.byref(_q(**over)), nr) == _lib.FMCW_OK, over
        cfg = _config(over)
        cfg.check(nr)
        assert cfg.to_c().flags == over.get("flags", 0)
    assert lib.fmcw_doa_check(None, 64) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"doa params is NULL"
    c = DoaConfig(65, max_pk=3, r_lo=2, r_hi=9, wrap=True, inv=True, min_abs=0.5, min_rel=0.25, min_prom=2.0).to_c()
    assert (c.n_ang, c.r_lo, c.r_hi, c.max_pk, c.flags, c.min_abs, c.min_rel, c.min_prom) == (65, 2, 9, 3, 6, 0.5, 0.25, 2.0)


def test_the_first_violated_rule_is_reported():
    lib = _lib.load()
    assert lib.fmcw_doa_check(ct.byref(_q(n_ang=0, max_pk=0)), 24) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"doa: nr must be a power of two in [16, 2048]"
    assert lib.fmcw_doa_check(ct.byref(_q(n_ang=0, max_pk=0)), 32) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"doa: n_ang must be in [1, 256]"


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    q = _q()
    assert lib.fmcw_doa(None, ct.byref(q), None, 1, 64, None, None, None, None, None, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ctx is NULL"
    assert lib.fmcw_doa_device(None, ct.byref(q), None, 1, 64, None, None, None, None, None, None, None) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == b"ctx is NULL"
    assert lib.fmcw_timing_read_ext(None, _lib.DOA_STAGE, None, None) == _lib.FMCW_E_ARG


# ---- 6, 7. the stage list and the MEX gateway -----------------------------------------------------------------------
def test_stage_list_keeps_its_18_names():
    assert len(_lib.STAGES) == 18 and _lib.STAGES[-1] == "ra" and "doa" not in _lib.STAGES
    assert _lib.MUSIC_STAGE == 18 and _lib.DOA_STAGE == 19


def test_mex_gateway_documents_and_dispatches_doa():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "mex", "fmcw_mex.c")).read()
    assert "fmcw_mex('doa'" in src and re.search(r'^  if \(!strcmp\(cmd, "doa"\)\)', src, re.M)
    assert "fmcw_mex('doa'" in open(os.path.join(root, "INTEGRATION.md")).read()
