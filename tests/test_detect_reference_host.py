"""CPU: the detection reference (tests/detect_reference.py) against the float64 oracle, the
conditions the scenes of tests/test_gpu_detect_rules.py rely on, and the 10 % caps on what those
tests may leave out of their exact comparisons -- all on the oracle alone.  Also the float32-ABI
gate (params.gate_bins) that CfarConfig.for_config and SigConfig.for_config use."""
import numpy as np
import pytest

from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import detect_reference as R

DEPLOYED = (64, 16, 256, 16)
RAGGED = (100, 20, 128, 32)


# ---- the gate -------------------------------------------------------------------------------
GRID_BW = (150e6, 180e6, 200e6, 250e6, 300e6)
GRID_K = (2, 3, 5, 7, 11, 41, 60, 100, 333)


def _cfg(bw, **over):
    cfg = P.derive_params(P.deployed_device(1024, 256), nr=1024, nd=256, mode=P.THROUGHPUT)
    cfg.bw = bw
    for k, v in over.items():
        setattr(cfg, k, v(cfg) if callable(v) else v)
    return cfg


def test_gate_is_the_float32_abi_gate_over_the_grid():
    """for_config's gate is gate_bins (library and reference agree) for limits that lie on a bin;
    where dist_per_bin is inexact in binary the double-precision gate differs from it in some."""
    differ = 0
    for bw in GRID_BW:
        for k in GRID_K:
            for cfg in (_cfg(bw, max_d=lambda c: k * c.dist_per_bin, min_d=0.0),
                        _cfg(bw, min_d=lambda c: k * c.dist_per_bin, max_d=700.0)):
                g = R.gate_bins(cfg)
                np.testing.assert_array_equal(P.gate_bins(cfg), g)
                np.testing.assert_array_equal(g, np.arange(g[0], g[-1] + 1))
                q = P.CfarConfig.for_config(cfg)
                s = P.SigConfig.for_config(cfg)
                assert (q.r_lo, q.r_hi) == (g[0] + 1, g[-1] + 1) == (s.r_lo, s.r_hi)
                d = R.double_gate(cfg)
                same = len(d) == len(g) and np.array_equal(d, g)
                if float(np.float32(cfg.dist_per_bin)) == cfg.dist_per_bin:
                    assert same, (bw, k)
                differ += not same
    assert differ >= 5, differ


def test_gate_named_cases():
    cfg = P.derive_params(P.deployed_device(1024, 256), nr=1024, nd=256, mode=P.THROUGHPUT)
    q = P.CfarConfig.for_config(cfg)
    assert (q.r_lo, q.r_hi) == (3, 34)                       # dist_per_bin 0.75: unchanged
    np.testing.assert_array_equal(R.gate_bins(cfg), np.arange(2, 34))
    b = R.batch_gate("max")
    assert R.double_gate(b.cfg)[-1] + 1 == 42 and P.CfarConfig.for_config(b.cfg).r_hi == 41
    b = R.batch_gate("min")
    assert R.double_gate(b.cfg)[0] + 1 == 4 and P.CfarConfig.for_config(b.cfg).r_lo == 5
    for geom, mode in ((DEPLOYED, P.PARITY), (RAGGED, P.THROUGHPUT)):
        c = R.batch_main(geom, mode).cfg
        np.testing.assert_array_equal(R.gate_bins(c), R.double_gate(c))


def test_empty_gate_raises():
    cfg = _cfg(200e6, min_d=10.1, max_d=10.2)
    assert len(P.gate_bins(cfg)) == 0
    with pytest.raises(ValueError, match="no range bin"):
        P.CfarConfig.for_config(cfg)
    with pytest.raises(ValueError, match="no range bin"):
        P.SigConfig.for_config(cfg)


# ---- the parametrisations of the GPU tests, on the oracle --------------------------------------
def _sets(name):
    """(batch, fp16_input, cfg with the set's parameters) for every run the GPU tests make."""
    out = []
    if name == "main":
        b = R.batch_main()
        thr10 = R.s10_threshold(b, b.oracle())
        for h in (False, True):
            for M, over in ((1, {}), (8, {}), (3, {}), (3, dict(doppler_thr=thr10))):
                out.append((b, h, R.with_params(b.cfg, M, **over)))
    elif name == "noise":
        b = R.batch_noise()
        for h in (False, True):
            q0 = R.oracle_params(b.p, b.cfg, 8)
            thr = R.median_row_peak(b.oracle(h), R.decide(b.oracle(h), q0))
            out.append((b, h, R.with_params(b.cfg, 8, doppler_thr=thr)))
    elif name == "gate":
        for w in ("max", "min", "exact"):
            b = R.batch_gate(w)
            out += [(b, False, R.with_params(b.cfg, M)) for M in (1, 3)]
    elif name == "zero":
        b = R.batch_zero()
        out.append((b, False, R.with_params(b.cfg, 1)))
    elif name == "wide":
        b = R.batch_wide()
        out += [(b, True, R.with_params(b.cfg, M, **R.WIDE_GATES[g])) for g in R.WIDE_GATES for M in (1, 3)]
    else:
        for geom, mode in ((DEPLOYED, P.PARITY), (RAGGED, P.THROUGHPUT)):
            b = R.batch_main(geom, mode)
            out.append((b, False, R.with_params(b.cfg, 3)))
    return out


ALL = ("main", "noise", "gate", "wide", "zero", "small")


@pytest.mark.parametrize("name", ALL)
def test_reference_agrees_with_oracle(name):
    """peaks() and doppler_choice() against oracle.search_peak and oracle.doppler_index on the same
    double-precision inputs: the oracle's profile rounded to float32 (peaks() takes float32), its RD
    rows as they are."""
    for b, h, cfg in _sets(name):
        ob = b.oracle(h)
        prm = R.abi_params(cfg)
        M = cfg.max_targets
        for f in range(len(b.names)):
            p32 = ob["profile"][f].astype(np.float32)
            n, idx, mag = R.peaks(p32, prm, M)
            ridx, rmag = O.search_peak(p32.astype(np.float64), cfg.nr, prm["range_thr"], M, prm["min_d"], prm["max_d"],
                                       prm["dist_per_bin"])
            assert n == len(ridx) and list(idx[:n]) == ridx and list(mag[:n].astype(np.float64)) == rmag
            assert np.all(idx[n:] == 0) and np.all(mag[n:] == 0)
            want = O.doppler_index(ob["rd"][f], ridx, prm["doppler_thr"], cfg.doppler_fallback_idx)
            for j, r in enumerate(ridx):
                c = R.doppler_choice(ob["rd"][f, r - 1], prm["doppler_thr"], cfg.doppler_fallback_idx)
                assert c["idx"] == want[j] and c["idx"] in c["allowed"]
                assert c["ambiguous"] or c["allowed"] == {c["idx"]}


@pytest.mark.parametrize("name", ALL)
def test_caps_hold(name):
    """At most 10 % of a batch's frames and of its Doppler rows are left out of the exact
    comparison with the oracle (1e-5; 3e-3 under fp16 storage)."""
    for b, h, cfg in _sets(name):
        q = R.oracle_params(b.p, cfg, cfg.max_targets)
        dec = R.decide(b.oracle(h), q)
        fa, ra = R.ambiguity(b.oracle(h), dec, q, 3e-3 if h else 1e-5)
        R.check_caps(fa, ra, dec)


def test_doppler_choice_band():
    row = np.zeros(16, np.complex128)
    row[3], row[11] = 100.0, 100.0 * (1 - 2.0 ** -23)
    c = R.doppler_choice(row, 50.0, 9)
    assert c["idx"] == 4 and c["allowed"] == {4, 12} and c["ambiguous"]
    row[11] = 100.0 * (1 - 2.0 ** -19)
    c = R.doppler_choice(row, 50.0, 9)
    assert c["allowed"] == {4} and not c["ambiguous"]
    c = R.doppler_choice(row, 100.0 * (1 + 2.0 ** -23), 9)          # the threshold is the ambiguous part
    assert c["idx"] == 9 and c["allowed"] == {4, 9} and c["ambiguous"]
    row[8] = 500.0                                                  # the maximum on the fallback bin
    assert R.doppler_choice(row, 50.0, 9)["allowed"] == {9}


def test_xcd_group_is_a_partition_into_32_groups_of_32():
    g = np.array([R.xcd_group(r) for r in range(1024)])
    assert sorted(set(g)) == list(range(32)) and np.all(np.bincount(g) == 32)
    assert R.xcd_group(17) == R.xcd_group(32) == R.xcd_group(33) == 0


# ---- the scene conditions ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main():
    b = R.batch_main()
    ob = b.oracle()
    return b, ob, {M: R.decide(ob, R.oracle_params(b.p, b.cfg, M)) for M in (1, 3, 8)}


def test_multi_target_scenes(main):
    b, ob, dec = main
    g = R.gate_bins(b.cfg)
    for f in b.frames("S1"):            # 10 tones 3 bins apart: more candidates than M, all on tone bins
        assert dec[8]["tgt_count"][f] == 8 and dec[3]["tgt_count"][f] == 3
        assert set(dec[8]["tgt_range_idx"][f] - 1) <= set(range(g[0] + 1, g[0] + 29, 3))
        assert np.all(np.diff(dec[8]["tgt_range_mag"][f]) < 0)
    for f in b.frames("S2"):            # two tones: slots 2.. stay zero
        assert dec[8]["tgt_count"][f] == 2 and np.all(dec[8]["tgt_range_idx"][f, 2:] == 0)
    for f in b.frames("S3"):            # equal amplitudes at r, r + 8: a near tie
        m = dec[8]["tgt_range_mag"][f]
        assert dec[8]["tgt_count"][f] == 2 and abs(m[0] - m[1]) <= 1e-6 * m[0]
        assert abs(int(dec[8]["tgt_range_idx"][f, 0]) - int(dec[8]["tgt_range_idx"][f, 1])) == 8
    for f in b.frames("S5"):            # adjacent tones: one peak
        assert dec[8]["tgt_count"][f] >= 1


def test_plateau_scene(main):
    b, ob, dec = main
    mid = (R.gate_bins(b.cfg)[0] + R.gate_bins(b.cfg)[-1]) // 2
    for f, r in zip(b.frames("S4")[:2], (mid, mid + 7)):     # noise-free half-bin tone: bins r, r + 1 within rounding
        p = ob["profile"][f]
        assert abs(p[r] - p[r + 1]) <= 1e-6 * p[r] and p[r] > 2 * p[r - 1] and dec[1]["tgt_range_idx"][f, 0] - 1 in (r, r + 1)
        assert R.frame_ambiguous(p, R.oracle_params(b.p, b.cfg, 1), 1, 1e-5)
    for f in b.frames("S4")[2:]:        # with noise: split by more than the fp16-storage band
        assert not R.frame_ambiguous(b.oracle(True)["profile"][f], R.oracle_params(b.p, b.cfg, 1), 1, 3e-3)


def test_edge_and_threshold_scenes(main):
    b, ob, dec = main
    g = R.gate_bins(b.cfg)
    thr = R.abi_params(b.cfg)["range_thr"]
    got = sorted(int(dec[8]["tgt_range_idx"][f, 0]) - 1 for f in b.frames("S6in"))
    assert got == sorted([int(g[0]), int(g[-1])] * 2)
    for f in b.frames("S6in"):
        assert dec[8]["tgt_count"][f] == 1
    for f in b.frames("S6out"):         # the strongest bin lies outside, its in-gate neighbour is no peak
        assert dec[8]["tgt_count"][f] == 0 and int(np.argmax(ob["profile"][f])) in (g[0] - 1, g[-1] + 1)
        assert ob["profile"][f][[g[0], g[-1]]].max() > thr
    for f in b.frames("S7hi"):
        assert dec[8]["tgt_count"][f] == 1 and abs(dec[8]["tgt_range_mag"][f, 0] / thr - 1.02) < 1e-3
    for f in b.frames("S7lo"):
        assert dec[8]["tgt_count"][f] == 0 and abs(ob["profile"][f][R.gate_bins(b.cfg)].max() / thr - 0.98) < 1e-3


def test_candidate_miss_scene(main):
    """S8: the detected row is absent from its group's two strongest keys, in the c64 and in the
    fp16-rounded frame."""
    b, ob, dec = main
    for h in (False, True):
        o = b.oracle(h)
        d = R.decide(o, R.oracle_params(b.p, b.cfg, 8))
        for f in b.frames("S8"):
            assert d["tgt_count"][f] == 1 and d["tgt_range_idx"][f, 0] == 18
            keys = R.group_keys(o["profile"][f], R.abi_params(b.cfg), R.xcd_group(17))
            assert keys == [33, 32], keys
        f = b.frames("C1")[0]          # the stronger target: candidate 1 of its group
        assert d["tgt_range_idx"][f, 0] == 18 and R.group_keys(o["profile"][f], R.abi_params(b.cfg), 0) == [33, 17]


def test_doppler_scenes(main):
    b, ob, dec = main
    fb = b.cfg.doppler_fallback_idx
    for f in b.frames("S9"):            # AM static target: lines at +-9 of about equal height
        r = dec[1]["tgt_range_idx"][f, 0] - 1
        m = np.abs(ob["rd"][f, r])
        top = np.argsort(m)[::-1][:2]
        assert sorted(top) == [128 - 9, 128 + 9] and abs(m[top[0]] - m[top[1]]) <= 3e-3 * m[top[0]]
    f = b.frames("S9")[0]               # noise-free: within the float32 band
    assert R.doppler_choice(ob["rd"][f, dec[1]["tgt_range_idx"][f, 0] - 1], 50.0, fb)["allowed"] == {120, 138}
    thr = R.s10_threshold(b, ob)
    d = R.decide(ob, dict(R.oracle_params(b.p, b.cfg, 3), doppler_thr=float(np.float32(thr))))
    for f in b.frames("S10"):           # the weakest of three moving targets falls back
        assert d["tgt_count"][f] == 3 and d["tgt_doppler_idx"][f, 2] == fb and np.all(d["tgt_doppler_idx"][f, :2] != fb)
        assert np.all(dec[3]["tgt_doppler_idx"][f] != fb)


def test_zero_row_scene():
    """doppler_thr 0: the static noise-free target's row is rounding residue in the oracle (left out of the
    exact comparison), every other row is kept; an exactly zero row leaves doppler_choice nothing open."""
    b = R.batch_zero()
    ob = b.oracle()
    q = R.oracle_params(b.p, b.cfg, 1)
    dec = R.decide(ob, q)
    fa, ra = R.ambiguity(ob, dec, q, 1e-5)
    assert np.all(dec["tgt_count"] == 1) and not fa.any() and list(np.nonzero(ra[:, 0])[0]) == b.frames("static")
    assert np.abs(ob["rd"][0, 12]).max() < 1e-9 * ob["row_pre"][0, 12]
    c = R.doppler_choice(np.zeros(256, np.complex64), 0.0, 129)
    assert c["idx"] == 1 and c["allowed"] == {1} and not c["ambiguous"]
    c = R.doppler_choice(np.zeros(256, np.complex64), 50.0, 129)
    assert c["idx"] == 129 and c["allowed"] == {129} and not c["ambiguous"]


def test_noise_scenes():
    b = R.batch_noise()
    ob = b.oracle()
    q = R.oracle_params(b.p, b.cfg, 8)
    dec = R.decide(ob, q)
    assert np.all(dec["tgt_count"] == 8)
    thr = R.median_row_peak(ob, dec)
    d = R.decide(ob, dict(q, doppler_thr=float(np.float32(thr))))
    share = np.mean(d["tgt_doppler_idx"] == b.cfg.doppler_fallback_idx)
    assert 0.4 <= share <= 0.6, share


def test_inexact_gate_scenes():
    """Set 4: the double-precision gate admits the planted tone's bin, the float32 gate does not."""
    for w in ("max", "min"):
        b = R.batch_gate(w)
        ob = b.oracle()
        g, d = R.gate_bins(b.cfg), R.double_gate(b.cfg)
        extra = sorted(set(d) - set(g))
        assert len(extra) == 1 and extra[0] in (g[0] - 1, g[-1] + 1)
        abi = R.decide(ob, R.oracle_params(b.p, b.cfg, 1))
        dbl = R.decide(ob, dict(b.p, max_targets=1, min_d=b.cfg.min_d, max_d=b.cfg.max_d,
                                doppler_fallback_idx=b.cfg.doppler_fallback_idx))
        differ = np.nonzero(abi["tgt_count"] != dbl["tgt_count"])[0]
        assert len(differ) == 2 and all(b.names[f] == "out" for f in differ)
        assert np.all(dbl["tgt_range_idx"][differ, 0] - 1 == extra[0]) and np.all(abi["tgt_count"][differ] == 0)
        assert np.all(abi["tgt_count"][b.frames("in")] == 1)


def test_exact_gate_scene():
    """Both limits on a bin, exactly: the edge bins are admitted (rng == min_d, rng == max_d)."""
    b = R.batch_gate("exact")
    a = R.abi_params(b.cfg)
    g = R.gate_bins(b.cfg)
    np.testing.assert_array_equal(g, R.double_gate(b.cfg))
    assert (g[0], g[-1]) == (3, 30) and g[0] * a["dist_per_bin"] == a["min_d"] and g[-1] * a["dist_per_bin"] == a["max_d"]
    dec = R.decide(b.oracle(), R.oracle_params(b.p, b.cfg, 1))
    assert sorted(dec["tgt_range_idx"][b.frames("in"), 0] - 1) == [3, 3, 30, 30]
    assert np.all(dec["tgt_count"][b.frames("out")] == 0)


def test_wide_gate_scenes():
    b = R.batch_wide()
    ob = b.oracle(True)
    for gname, over in R.WIDE_GATES.items():
        cfg = R.with_params(b.cfg, 1, **over)
        keep = P.fp16_fp32_bins(cfg)
        blocks = sorted(set(np.nonzero(keep)[0] // 128))
        assert blocks == {"200": [0, 1, 2], "all": list(range(8)), "95": [0, 1], "97": [0, 1, 2]}[gname]
        dec = R.decide(ob, R.oracle_params(b.p, cfg, 1))
        g = R.gate_bins(cfg)
        for f, n in enumerate(b.names):
            r = int(round(float(n[3:])))
            assert int(np.argmax(ob["profile"][f])) == r
            assert dec["tgt_count"][f] == int(r in g), (gname, n)
            if r in g:
                assert dec["tgt_range_idx"][f, 0] - 1 == r
