"""Host tests of tests/taps_cases.py: what tests/test_gpu_taps.py relies on, proved on the float64 oracle
alone.  No GPU.

  sensitivity  a reversed window, a dropped end sample or end chirp and a stale calibration vector move an
               output the GPU module compares by 100 bars or more under every non-plain family, at every
               geometry that module runs; under the plain taps the reversals and the end samples stay under
               one bar, which is why the module exists
  carrying     the float32 restatement of k_rdx's algebra stays under half the fp32 bar under every family
  fp16         e_ref <= E_REF_MAX for every fp16 case run, or the frame is in the left-out table, exactly
  decisions    which frames and rows the oracle leaves open, that every batch keeps a frame with and one
               without a target, and where the `ends` taps make that impossible
  K1           the profile paths fmcw_range_fft_device takes over the cases run
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import streams_reference as SR
from tests import taps_cases as TC
from tests import xcd_reference as XR
from tests.helpers import TOL_FP32_REL_L2, rd_rel_err, rel_l2
from tests.streams_reference import C32H, C64, STORAGE

BAR = TOL_FP32_REL_L2
MOVES = 100.0                           # a mutation must move an output by this many bars

# every geometry test_gpu_taps runs, with the outputs it compares there
STREAMS_G = list(dict.fromkeys(SR.SIZE_CASES + SR.STORAGE_CASES + SR.PAIR_CASES))
K1_G = [g for g in SR.K1_CASES if g not in STREAMS_G]
XCD_G = [XR.geometry(n) for n in XR.NTS_CASES]


def _kinds_of(g):
    if g in XCD_G and g not in STREAMS_G:           # 1024 x 256 is a size case too: every family
        return ("rand", "ends") + (("tilt",) if g[0] in TC.TILT_NTS else ())
    if g in K1_G:
        return TC.K1_KINDS
    return TC.NEW_KINDS if g in SR.SIZE_CASES else ("rand",)


def _outputs_of(g):
    if g in K1_G:
        return ("cube", "profile")
    if g in XCD_G:                                  # the single pass keeps no range cube
        return ("rd", "profile")
    return ("cube", "rd", "profile")


def test_families_are_what_the_module_says():
    for nts, pn, nr, nd in ((1024, 256, 1024, 256), (100, 70, 64, 64), (27, 5, 32, 8), (16, 6, 16, 2)):
        for kind in TC.NEW_KINDS:
            wr, wd, cal = TC.taps(kind, nts, pn, nr, nd)
            assert wr.shape == (nts,) and wd.shape == (pn,) and cal.shape == (nts,)
            assert np.array_equal(wr, wr.astype(np.float32)) and np.array_equal(wd, wd.astype(np.float32))
            assert np.array_equal(cal, cal.astype(np.complex64))
            assert not np.allclose(wr, wr[::-1]) and not np.allclose(wd, wd[::-1])
            assert wr[0] != 0 and wd[0] != 0 and wr[min(nts, nr) - 1] != 0 and wd[min(pn, nd) - 1] != 0
            mod = np.abs(cal - (0.004 - 0.003j))
            assert mod.max() > 2 * mod.min() and abs(cal.mean()) > 1e-3          # varying modulus, non-zero mean
        wr, wd, _ = TC.taps("ends", nts, pn, nr, nd)
        for w, n, nfft in ((wr, nts, nr), (wd, pn, nd)):
            inside = np.nonzero(w[:min(n, nfft)])[0].tolist()
            assert inside == TC.ends_support(n, nfft)
            assert (np.nonzero(w[nfft:])[0].tolist() == [0]) == (n > nfft)      # the one tap beyond a truncating FFT
    a = TC.taps("plain", 64, 16)
    b = O.windows(64, 16) + (O.synth_cal(64),)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        TC.taps("ends", 4, 16)
    wr, wd, _ = TC.taps("ends", 1024, 256, 1024, 256)
    assert wr[[0, 1, 1022, 1023]].tolist() == [1.0, 1.5, 1.75, 2.0] and wd[[0, 1, 254, 255]].tolist() == [2.0, 1.75, 1.5, 1.0]
    assert TC.retone(np.zeros((2, 8), np.complex64), "plain").sum() == 0
    np.testing.assert_allclose(TC.retone(O.synth_cal(8).astype(np.complex64)[None], "rand")[0], TC.cal_vector(8), atol=1e-8)


# ---------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------
def _zeroed(w, i):
    w = w.copy()
    w[i] = 0.0
    return w


def mutations(g, wr, wd, cal) -> dict:
    """name -> (wr, wd, cal).  The oracle removes the mean before it applies a window, so a zeroed tap drops
    that sample's (chirp's) windowed contribution and keeps the mean."""
    nts, pn, nr, nd, _ = g
    return {
        "wr reversed": (wr[::-1].copy(), wd, cal),
        "wd reversed": (wr, wd[::-1].copy(), cal),
        "sample 0": (_zeroed(wr, 0), wd, cal),
        "sample last": (_zeroed(wr, min(nts, nr) - 1), wd, cal),
        "chirp 0": (wr, _zeroed(wd, 0), cal),
        "chirp last": (wr, _zeroed(wd, min(pn, nd) - 1), cal),
        "stale cal": (wr, wd, O.synth_cal(nts)),
    }


def moved(g, kind, outputs) -> dict:
    """name -> the largest of the outputs' errors, in bars, of the white frame processed with the mutated
    taps against the same frame with the family's own."""
    _, p, wr, wd, cal = SR.build_case(g, taps=kind)
    iq = SR.noise_frame(g, kind)
    ref = O.process_frames(iq, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    out = {}
    for name, (mr, md, mc) in mutations(g, wr, wd, cal).items():
        got = O.process_frames(iq, mc, p, mr, md, want_cube=True, want_rd=True, rd_all_rows=True)
        e = dict(cube=rel_l2(got["cube"], ref["cube"]), profile=rel_l2(got["profile"], ref["profile"]),
                 rd=rd_rel_err(got["rd"], ref["rd"], ref["cube"], wd, g[3])[0])
        out[name] = max(float(e[k]) for k in outputs) / BAR
    return out


ALL_G = list(dict.fromkeys(STREAMS_G + K1_G + XCD_G))


@pytest.mark.parametrize("g", ALL_G, ids=SR.case_id)
def test_every_mutation_moves_an_output_by_100_bars(g):
    outputs = _outputs_of(g)
    for kind in _kinds_of(g):
        m = moved(g, kind, outputs)
        print(f"\nTAPS moved {SR.case_id(g)} {kind} (bars) " + " ".join(f"{k}: {v:.1e}" for k, v in m.items()))
        for name, v in m.items():
            if "rd" not in outputs and (name.startswith("wd") or name.startswith("chirp")):
                continue                                    # fmcw_range_fft_device: the Doppler window plays no part
            assert v >= MOVES, (kind, name, v)


@pytest.mark.parametrize("g", ALL_G, ids=SR.case_id)
def test_the_plain_taps_hide_the_same_mutations(g):
    """Both plain windows are symmetric and Blackman ends in zeros: the reversals, and from nts 1000 the end
    samples, stay under one bar (the reason for tests/test_gpu_taps.py)."""
    m = moved(g, "plain", ("cube", "rd", "profile"))
    print(f"\nTAPS moved {SR.case_id(g)} plain (bars) " + " ".join(f"{k}: {v:.1e}" for k, v in m.items()))
    assert m["wr reversed"] < 1.0 and m["wd reversed"] < 1.0 and m["stale cal"] == 0.0
    if 1000 <= g[0] <= g[2]:                                # where the FFT truncates, its last sample is no end of the window
        assert m["sample 0"] < 1.0 and m["sample last"] < 1.0


# ---------------------------------------------------------------------------
# carrying: k_rdx's algebra in float32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", TC.KINDS)
def test_the_fp32_algebra_carries_every_family(kind):
    k = XR.k_x0(kind)
    for nts in XR.K_NTS:
        for frame in ("white", "white_x0"):
            figs = XR.restate_errors(nts, k, kind, frame)
            print(f"\nTAPS restated {kind} nts {nts} {frame} k {k}: rd {figs[0]:.2e} profile {figs[1]:.2e} rd_max {figs[2]:.2e}")
            assert XR.carries(figs), (kind, nts, frame, figs)


@pytest.mark.parametrize("kind", TC.NEW_KINDS)
def test_chirp0_scale_is_the_largest_each_family_carries(kind):
    """taps_cases.K_X0, by the rule that chose xcd_reference.K_X0 (test_xcd_reference_host): carried at k, not at
    k + 1."""
    k, figs = XR.choose_k(kind, k_from=TC.K_X0[kind])
    for kk, by_nts in figs.items():
        print(f"\nTAPS {kind} k {kk} " + " ".join(f"nts {n}: rd {a:.2e} profile {b:.2e} rd_max {c:.2e}" for n, (a, b, c) in by_nts.items()))
    assert min(k, XR.K_X0) == TC.K_X0[kind] > 0


# ---------------------------------------------------------------------------
# fp16
# ---------------------------------------------------------------------------
OUTPUTS_1P = ("rd", "profile", "slow_mag", "tgt_range_mag", "probe")        # what the single pass returns


@pytest.mark.parametrize("nts", XR.FP16_NTS)
def test_rdx_fp16_cases_meet_their_conditions(nts):
    r = XR.ref(nts, C32H, "rand")
    e = r.emu(r.mask, C32H)
    assert XR.mask_of(r.cfg) == r.mask
    # the fp16 hand-off changes no decision of the peak rule, and the oracle leaves none open
    np.testing.assert_array_equal(e["tgt_count"], r.plain["tgt_count"])
    np.testing.assert_array_equal(e["tgt_range_idx"], r.plain["tgt_range_idx"])
    np.testing.assert_array_equal(e["slow_mag"], r.plain["slow_mag"])
    assert not TC.flagged_frames(r, False).any()
    for k in OUTPUTS_1P:
        v = e["e_ref"][k]
        if k == "probe":
            assert v[0] <= SR.E_REF_MAX
            continue
        for f in range(r.F):
            out = k == "rd" and XR.fp16_left_out(nts, r.names[f], "rand")
            assert (v[f] > SR.E_REF_MAX) == out, (k, nts, r.names[f], v[f])
    # never more left out than under the plain taps at the same nts
    for name in r.names:
        if XR.fp16_left_out(nts, name, "rand"):
            assert XR.fp16_left_out(nts, name), (nts, name)
    x0, hot = TC.FP16_LEFT_OUT["rand"]
    assert len(x0) <= len(XR.FP16_X0_LEFT_OUT) and len(hot) <= len(XR.FP16_HOT_LEFT_OUT)


@pytest.mark.parametrize("g", SR.STORAGE_CASES, ids=SR.case_id)
def test_storage_cases_meet_their_conditions(g):
    r = SR.ref(g, C64, "storage", "rand")
    pl = r.plain
    has = pl["tgt_count"] > 0
    assert has.any() and (~has).any()
    assert not TC.flagged_frames(r, True).any()              # every frame compared exactly, as under the plain taps
    assert r.emu()["cube_peak"] < 100.0
    for st in STORAGE:
        e = r.emu(*st)
        for k, v in e["e_ref"].items():
            assert np.max(v) <= SR.E_REF_MAX, (st, k, v)     # no frame left out
        np.testing.assert_array_equal(e["tgt_count"], pl["tgt_count"])
        np.testing.assert_array_equal(e["tgt_range_idx"], pl["tgt_range_idx"])


def test_k1_cases_meet_their_conditions():
    for kind in TC.K1_KINDS:
        seen = set()
        for g in SR.K1_CASES:
            e = SR.ref(g, C64, "synth", kind).emu(C32H, C64)
            assert np.max(e["e_ref"]["cube"]) <= SR.E_REF_MAX and e["cube_peak"] < 100.0
            seen |= SR.k1_profile_paths(g, None)
        for g, cpt in TC.K1_CPT_CASES:
            assert g in SR.K1_CASES and cpt in ("1", "64")
            seen |= SR.k1_profile_paths(g, cpt)
        assert seen == {"store", "parts", "atomic", "tail"}, (kind, seen)
    assert {cpt for _, cpt in TC.K1_CPT_CASES} == {"1", "64"}


# ---------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------
def _check_decisions(r, streams, label, open_frames):
    """At most one frame of the batch left open (open_frames where the `ends` taps leave more, exactly), a
    frame with and one without a target among the others, and at most one frame outside the one-hot frames
    with an open Doppler row."""
    pl = r.plain
    flagged = TC.flagged_frames(r, streams)
    rows = TC.ambiguous_rows(r)
    names = getattr(r, "names", [str(f) for f in range(r.F)])
    has = pl["tgt_count"] > 0
    print(f"\nTAPS decisions {label} targets {int(has.sum())} of {r.F} open frames {[names[f] for f in np.nonzero(flagged)[0]]} "
          f"open rows {[names[f] for f in np.nonzero(rows.any(axis=1))[0]]}")
    if open_frames is None:
        assert flagged.sum() <= 1, label
        assert (has & ~flagged).any() and (~has & ~flagged).any(), label
    else:
        assert flagged.sum() == open_frames > 1, label
        assert (~has & ~flagged).any(), label
    other = [names[f] for f in np.nonzero(rows.any(axis=1))[0] if not names[f].startswith("hot")]
    assert len(other) <= 1, (label, other)
    # a one-hot frame's open row is the exact tie of D[d] and D[-d], or lies about a stationary column
    # (taps_cases.ambiguous_rows)
    nd = pl["rd"].shape[2]
    for f, j in zip(*np.nonzero(rows)):
        if names[f].startswith("hot"):
            mag = np.abs(pl["rd"][f, pl["tgt_range_idx"][f, j] - 1])
            top = np.argsort(mag)[-2:]                      # columns after fftshift: d + nd / 2
            own = {0, nd // 2}                              # the columns that are their own mirror
            assert (int(top[0]) + int(top[1])) % nd == 0 or own & {int(top[0]), int(top[1])}, (label, names[f], top)
    return flagged


SIZE_GRID = [(g, k) for k in TC.NEW_KINDS for g in SR.SIZE_CASES]


@pytest.mark.parametrize("g,kind", SIZE_GRID, ids=[f"{SR.case_id(g)}-{k}" for g, k in SIZE_GRID])
def test_size_batches_keep_their_decisions(g, kind):
    r = SR.ref(g, C64, "noise", kind)
    assert r.noise == r.F - 1 and r.F == g[4] + 1
    _check_decisions(r, True, f"{SR.case_id(g)} {kind}", TC.ENDS_OPEN_STREAMS.get(tuple(g)) if kind == "ends" else None)


NTS_GRID = [(n, k) for k in ("rand", "ends") for n in XR.NTS_CASES] + [(n, "tilt") for n in TC.TILT_NTS]


@pytest.mark.parametrize("nts,kind", NTS_GRID, ids=[f"{n}-{k}" for n, k in NTS_GRID])
def test_rdx_batches_keep_their_decisions(nts, kind):
    r = XR.ref(nts, C64, kind)
    pl = r.plain
    hot = [f"hot{c}" for c in ((0, 1, 254, 255) if kind == "ends" else (0, 1, 7, 8, 9, 254, 255))]
    assert r.names == ["synth_target", "synth_empty", "white", "white_cal0", "white_x0"] + hot
    assert len({r.iq[f].tobytes() for f in range(r.F)}) == r.F
    _check_decisions(r, False, f"nts {nts} {kind}", TC.ENDS_OPEN_XCD.get(nts) if kind == "ends" else None)
    # noise yields peaks: every white frame has a target
    assert all(pl["tgt_count"][r.index(n)] == 1 for n in ("white", "white_cal0", "white_x0"))
    assert pl["tgt_count"][r.index("synth_empty")] == 0
    # under `ends` a one-hot frame is listed only where its chirp carries Doppler weight
    for n in hot:
        assert r.wd[int(n[3:])] != 0
    # every group's rows and, for the white frames, every Doppler column hold energy (as test_xcd_reference_host)
    for f in r.flat():
        grp, col = XR.energy_shares(pl["rd"][f])
        assert grp >= 0.1, (r.names[f], grp)
        if r.names[f].startswith("white"):
            assert col >= 0.1, (r.names[f], col)
    f, c = divmod(r.probe_column - 1, XR.PN)
    assert r.names[f] == f"hot{c}" and c in (9, 255)


def test_the_ends_tables_name_smooth_profiles_only():
    """Where more than one frame is left open under `ends`, the range FFT does not separate the four samples
    that reach it: S = Nr (the last two samples alias to bins -2 and -1, and a maximum's neighbours lie within
    (2 pi / Nr)^2 / 2 <= 1.9e-5 of it), or S within 2 of Nr / 2 (the last two samples alternate in sign from
    bin to bin, so every other bin is a local maximum of nearly one height)."""
    for g in TC.ENDS_OPEN_STREAMS:
        assert g in SR.SIZE_CASES and min(g[0], g[2]) == g[2] == 2048
    for nts in TC.ENDS_OPEN_XCD:
        assert nts == XR.NR or abs(nts - XR.NR // 2) <= 2
