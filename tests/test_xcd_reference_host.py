"""Host tests of tests/xcd_reference.py: what tests/test_gpu_xcd_grid.py relies on, proved on the float64
oracle alone.  No GPU."""
import numpy as np
import pytest

from fmcw_radar_processing_amd import params as P
from tests import detect_reference as DR
from tests import streams_reference as SR
from tests import xcd_reference as XR
from tests.helpers import TOL_FP32_REL_L2, near_tie_frames
from tests.streams_reference import C32H, C64

OUTPUTS = ("rd", "profile", "slow_mag", "tgt_range_mag", "probe")        # what the single pass returns


def _rows_ambiguous(r, tol):
    pl = r.plain
    return [r.names[f] for f in range(r.F) for j in range(int(pl["tgt_count"][f]))
            if DR.row_ambiguous(pl["rd"][f, pl["tgt_range_idx"][f, j] - 1], r.p["doppler_thr"], tol)]


def test_nts_list_has_the_coverage_its_comments_claim():
    s2 = [n // 2 for n in XR.NTS_CASES]
    assert all(n % 2 == 0 and 2 < n <= 1024 for n in XR.NTS_CASES)
    assert sum(v < 64 for v in s2) >= 3                                          # S2 < 64
    for m in (64, 256):                                                          # just below, on, just above a multiple of 64
        assert {m - 1, m, m + 1} <= set(s2)
    assert any(XR.pieces(n)["masked"] > 0 and XR.pieces(n)["whole"] > 0 for n in XR.NTS_CASES)   # a wholly masked piece
    assert any(XR.pieces(n)["partial"] == 0 and XR.pieces(n)["masked"] > 0 for n in XR.NTS_CASES)  # the mask on a boundary
    assert {1000, 1022, 1024} <= set(XR.NTS_CASES)
    # the number of whole pieces 0, 1, 3, 4, 7 and 8 each occurs
    assert {XR.pieces(n)["whole"] for n in XR.NTS_CASES} >= {0, 1, 3, 4, 7, 8}
    assert set(XR.FP16_NTS) <= set(XR.NTS_CASES) and set(XR.CHUNK_NTS) <= set(XR.NTS_CASES)
    assert set(XR.FULL_HOT_NTS) == {126, 1024} and XR.pieces(126)["masked"] == 7
    assert set(XR.HOT_FULL) == set(range(16)) | set(range(248, 256)) and set(XR.HOT_SHORT) == {0, 1, 7, 8, 9, 255}
    assert XR.DEGENERATE_NTS == [2, 4]


def test_group_rows_are_the_team_members_bins():
    seen = np.concatenate([XR.group_rows(g) for g in range(32)])
    assert sorted(seen.tolist()) == list(range(1024))
    assert all(DR.xcd_group(int(r)) == g for g in range(32) for r in XR.group_rows(g))
    # bins 4..31, where every synthetic tone of the older tests lies, are groups 0..3
    assert {DR.xcd_group(r) for r in range(4, 32)} == {0, 1, 2, 3}


# the masks of the nts cases under the default gate (dist_per_bin follows nts): recorded in DESIGN 5.4
MASKS = {30: 0x00, 62: 0xE0, 64: 0xE0, 66: 0xE0, 126: 0xF8, 128: 0xF8, 130: 0xF8, 254: 0xFC, 510: 0xFE, 512: 0xFE,
         514: 0xFE, 1000: 0xFE, 1022: 0xFE, 1024: 0xFE}


@pytest.mark.parametrize("nts", XR.NTS_CASES)
def test_nts_case_meets_its_conditions(nts):
    r = XR.ref(nts)
    pl = r.plain
    assert r.mask == MASKS[nts]
    assert len(set(r.names)) == r.F <= 40
    assert len({r.iq[f].tobytes() for f in range(r.F)}) == r.F                   # every frame distinct
    assert pl["tgt_count"][r.index("synth_target")] == 1 and pl["tgt_count"][r.index("synth_empty")] == 0
    # no near tie of the two synthetic frames at 1e-5, and no frame of the batch whose peak decision or Doppler
    # row the oracle leaves within 1e-5: the detections are compared exactly, no frame left out
    assert not near_tie_frames(pl["profile"][:2]).any()
    assert not r.ambiguous(TOL_FP32_REL_L2).any()
    assert _rows_ambiguous(r, TOL_FP32_REL_L2) == []
    # the white and one-hot frames: every group's rows at or above 1 / 10 of the map's rms (0.33 at the least);
    # every Doppler column of a white frame too.  A one-hot frame's map is wd[c] X_c in every column plus
    # sum(wd) X_c / 256 in the seven columns around Doppler 0 (the mean removal): the other columns lie at
    # 0.011 (c = 1, 254) to 0.094 (c = 12) of the map's rms, far above any rounding floor, and the
    # per-residue figures of the GPU test are relative to each residue class's own norm
    for f in r.flat():
        grp, col = XR.energy_shares(pl["rd"][f])
        assert grp >= 0.1, (r.names[f], grp)
        assert col >= (0.1 if r.names[f].startswith("white") else 0.01), (r.names[f], col)
    # the probe column is a one-hot frame's hot chirp
    f, c = divmod(r.probe_column - 1, XR.PN)
    assert r.names[f] == f"hot{c}" == "hot9"


@pytest.mark.parametrize("nts", XR.DEGENERATE_NTS)
def test_degenerate_nts(nts):
    r = XR.ref(nts)
    if nts == 2:                                  # Blackman(2) is zero: every output is rounding residue
        assert np.abs(r.wr).max() < 1e-15 and r.plain["profile"].max() < 1e-9 and not r.plain["tgt_count"].any()
    else:                                         # every frame with a target is a near tie: self-consistent rule only
        assert r.ambiguous(TOL_FP32_REL_L2).sum() >= 5


def test_chirp0_scale_is_the_largest_the_fp32_algebra_carries():
    """K_X0: the float32 restatement of k_rdx's algebra meets xcd_reference.carries up to 2^K_X0 at every nts
    of K_NTS and not beyond; its own L2 figure at k = 0 is below 2e-6, so the growth is the algebra's, not
    the FFT's."""
    k, figs = XR.choose_k()
    for kk, by_nts in figs.items():
        print(f"\nXCD k {kk} " + " ".join(f"nts {n}: rd {a:.2e} profile {b:.2e} rd_max {c:.2e}" for n, (a, b, c) in by_nts.items()))
    assert all(max(f[:2]) < 2e-6 for f in figs[0].values())
    assert k == XR.K_X0 and 0 < k <= XR.K_MAX
    assert all(XR.carries(f) for f in figs[k].values())
    if k < XR.K_MAX:
        assert not all(XR.carries(f) for f in figs[k + 1].values())


@pytest.mark.parametrize("nts", [30, 128, 1024])
def test_mask_0_c64_is_the_oracle_bit_for_bit(nts):
    r = XR.ref(nts)
    e = r.emu(0, C64)
    for k in ("profile", "cube", "rd", "slow_mag", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "probe"):
        np.testing.assert_array_equal(e[k], r.plain[k], err_msg=k)
    assert all(np.all(v == 0) for v in e["e_ref"].values())


def _check_fp16_conditions(r, mask):
    e = r.emu(mask, C32H)
    keep = P.fp16_fp32_bins(r.cfg) if mask else np.ones(XR.NR, bool)
    assert XR.mask_of(r.cfg) == r.mask
    # the blocks the mask leaves fp32 hold the oracle's own values: the peak rule sees those only (the gate lies
    # inside them), so its decisions are the plain chain's, and ambiguity is a matter of 1e-5, not of 1e-3
    np.testing.assert_array_equal(e["profile"][:, keep], r.plain["profile"][:, keep])
    np.testing.assert_array_equal(e["tgt_count"], r.plain["tgt_count"])
    np.testing.assert_array_equal(e["tgt_range_idx"], r.plain["tgt_range_idx"])
    np.testing.assert_array_equal(e["slow_mag"], r.plain["slow_mag"])
    assert not r.ambiguous(TOL_FP32_REL_L2).any() and _rows_ambiguous(r, TOL_FP32_REL_L2) == []
    for k in OUTPUTS:
        v = e["e_ref"].get(k)
        if v is None:
            continue
        if k == "probe":                          # one column of one frame
            assert v[0] <= SR.E_REF_MAX
            continue
        # a frame is left out of the RD comparison at this nts if and only if it breaks the condition here,
        # at its own nts and under this mask; no frame breaks it for any other output
        for f in range(r.F):
            out = k == "rd" and XR.fp16_left_out(r.nts, r.names[f])
            assert (v[f] > SR.E_REF_MAX) == out, (k, r.nts, hex(mask), r.names[f], v[f])
    # per group and per block: the white frames meet E_REF_MAX there too; a one-hot frame's 32 rows scatter about
    # its per-frame figure (7.6e-4 at the most), which leaves 2 e_ref + 1e-5 the bound: the 3e-3 cap does not bind
    ge = XR.group_e_ref(e["rd"], r.plain["rd"])
    be = XR.block_e_ref(e, r.plain, "rd")
    uncapped = (SR.bound(1.0) - TOL_FP32_REL_L2) / 2.0
    for f in range(r.F):
        if not XR.fp16_left_out(r.nts, r.names[f]) and XR.is_flat(r.names[f]):
            lim = SR.E_REF_MAX if r.names[f].startswith("white") else uncapped
            assert ge[f].max() <= lim and be[f].max() <= lim, (r.names[f], ge[f].max(), be[f].max())
    return e


@pytest.mark.parametrize("nts", XR.FP16_NTS)
def test_fp16_nts_case_meets_its_conditions(nts):
    r = XR.ref(nts, C32H)
    e = _check_fp16_conditions(r, r.mask)
    # the one-hot frames are in the RD comparison at every nts where a piece of the loads is wholly masked and
    # S2 <= 64, all 24 chirp positions of nts 126 among them; the 2^K_X0 frame where no block is c32h
    held = [n for n in r.names if not XR.fp16_left_out(nts, n)]
    print(f"\nXCD fp16 nts {nts} mask {r.mask:#04x} held {len(held)} of {r.F}, e_ref rd "
          + " ".join(f"{n} {v:.2e}" for n, v in zip(r.names, e["e_ref"]["rd"])))
    assert any(n.startswith("hot") for n in held) == (nts <= 128) and ("white_x0" in held) == (r.mask == 0)
    assert {"synth_target", "synth_empty", "white", "white_cal0"} <= set(held)


@pytest.mark.parametrize("mask", list(XR.MASK_GATES), ids=lambda m: f"{m:02x}")
def test_mask_gates_give_their_masks(mask):
    r = XR.mask_ref(mask)
    keep = P.fp16_fp32_bins(r.cfg)
    assert [not keep[128 * b] for b in range(8)] == [bool((mask >> b) & 1) for b in range(8)]
    assert all(len(set(keep[128 * b:128 * b + 128])) == 1 for b in range(8))
    assert r.mask == mask and r.names == list(XR.MASK_FRAMES)
    _check_fp16_conditions(r, mask)
    if mask == 0xFF:
        assert len(DR.gate_bins(r.cfg)) == 0 and not r.plain["tgt_count"].any()
    # FMCW_S16=0 under the default gate: every block fp32, the RD map still c32h
    if mask == 0xFE:
        _check_fp16_conditions(r, 0)


@pytest.mark.parametrize("F", XR.FRAME_COUNTS)
def test_frame_count_case_meets_its_conditions(F):
    r = XR.count_ref(F)
    assert r.F == F and len({r.iq[f].tobytes() for f in range(F)}) == F
    assert not r.ambiguous(TOL_FP32_REL_L2).any() and _rows_ambiguous(r, TOL_FP32_REL_L2) == []
    assert r.probe_column == F * XR.PN
    if F in XR.FRAME_COUNTS_FP16:
        r16 = XR.count_ref(F, C32H)
        _check_fp16_conditions(r16, r16.mask)
