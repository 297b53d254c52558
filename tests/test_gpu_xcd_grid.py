"""The single-pass schedule (k_rdx of csrc/kernels_xcd.hip, k_detect_1p of csrc/kernels_detect.hip) over
nts, frame contents, hand-off storage and frame counts, FMCW_PIPE_XCD forced, against the float64 oracle
and the storage-emulating chain of tests/xcd_reference.py.

  nts c64    every nts case through Engine.process: the bars of test_gpu_onepass per frame, and for the
             white and one-hot frames element-wise, per range-bin group and per Doppler residue
  nts fp16   c32h in and out through process_device at each case's own hand-off mask, every output held
             to 2 e_ref + the fp32 bar, guard frames behind the RD map and the IQ tensor
  masks      five gates at nts 1024 (hand-off masks 0x00, 0xFE, 0x7F, 0xE7, 0xFF) and FMCW_S16=0, per block
  counts     F = 1 .. 33: every frame bit-identical to the same frame processed alone
  chunks     chunks of 3 and 8 frames bit-identical to one chunk

Each measured figure is printed before it is asserted (pytest -s shows them; DESIGN.md 5.4 records them).
"""
import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
from fmcw_radar_processing_amd import params as P
from fmcw_radar_processing_amd._lib import FMCW_PIPE_AUTO, FMCW_PIPE_XCD
from tests import streams_reference as SR
from tests import xcd_reference as XR
from tests.helpers import TOL_FP32_REL_L2, rd_rel_err, rel_l2
from tests.test_gpu_detect_rules import check_self
from tests.test_gpu_streams_grid import Guarded

pytestmark = pytest.mark.gpu

assert (XR.C64, XR.C32H) == (FMCW_C64, FMCW_C32H)
BAR = TOL_FP32_REL_L2
DECISIONS = ("profile", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "slow_mag")


@pytest.fixture
def xcd(engine):
    engine.set_pipeline(FMCW_PIPE_XCD)
    try:
        yield engine
    finally:
        engine.set_chunk_frames(0)
        engine.set_pipeline(FMCW_PIPE_AUTO)


def _run(engine, r, iq=None, want_rd=True, probe_column=0):
    engine.set_taps(r.cfg, r.cal, r.wr, r.wd)
    got = engine.process(r.dev_iq if iq is None else iq, want_rd=want_rd, probe_column=probe_column)
    engine.synchronize()                           # no hand-off wait timed out, no ticket error
    return got


def _same(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


# ---------------------------------------------------------------------------
# the c64 bars
# ---------------------------------------------------------------------------
def _check_c64(r, got, label, probe_ref=None, flagged=None, rows=None):
    """Every frame at the fp32 bars, the flat frames element-wise, per group and per Doppler residue, the
    detections exactly (no frame of these batches is ambiguous: test_xcd_reference_host) and by the
    self-consistent rule.  flagged [F]: frames the oracle itself leaves open (tests/taps_cases.py), whose
    decisions, first magnitude and slow row are held by the self-consistent rule only; rows [F][M]: the
    detected rows whose Doppler index is."""
    pl = r.plain
    ok = np.ones(r.F, bool) if flagged is None else ~np.asarray(flagged)
    e_rd = rd_rel_err(got["rd"], pl["rd"], pl["cube"], r.wd, XR.ND)
    e_prof = rel_l2(got["profile"], pl["profile"], axis=1)
    has = (pl["tgt_count"] > 0) & ok
    none = (pl["tgt_count"] == 0) & ok
    e_slow = rel_l2(got["slow_mag"][has], pl["slow_mag"][has], axis=1) if has.any() else np.zeros(1)
    e_mag = np.abs(got["tgt_range_mag"][has, 0] / pl["tgt_range_mag"][has, 0] - 1.0) if has.any() else np.zeros(1)
    e_probe = rel_l2(got["probe_mag"], probe_ref) if probe_ref is not None else 0.0
    worst = dict(rd_max=(0.0, ""), group=(0.0, ""), residue=(0.0, ""), prof_max=(0.0, ""))
    for f in r.flat():
        m = XR.flat_measures(got["rd"][f], got["profile"][f], pl["rd"][f], pl["profile"][f])
        for k, where in (("rd_max", ""), ("group", f" g{int(np.argmax(m['group']))}"),
                         ("residue", f" d{int(np.argmax(m['residue']))}"), ("prof_max", "")):
            v = float(np.max(m[k]))
            if v > worst[k][0]:
                worst[k] = (v, r.names[f] + where)
    print(f"\nXCD {label} F {r.F} rd {e_rd.max():.2e} profile {e_prof.max():.2e} slow {e_slow.max():.2e} "
          f"mag {e_mag.max():.2e} probe {e_probe:.2e} flat: " + " ".join(f"{k} {v:.2e} ({w})" for k, (v, w) in worst.items()))
    assert e_rd.max() <= BAR, (label, r.names[int(np.argmax(e_rd))], e_rd.max())
    assert e_prof.max() <= BAR, (label, r.names[int(np.argmax(e_prof))], e_prof.max())
    assert e_slow.max() <= BAR and e_mag.max() <= BAR and e_probe <= BAR, (label, e_slow.max(), e_mag.max(), e_probe)
    assert np.all(got["slow_mag"][none] == 0)
    for k, (v, w) in worst.items():
        assert v <= BAR, (label, k, v, w)
    for k in ("tgt_count", "tgt_range_idx"):
        np.testing.assert_array_equal(got[k][ok], pl[k][ok], err_msg=f"{label}: {k}")
    dop = ok[:, None] & (True if rows is None else ~np.asarray(rows))
    np.testing.assert_array_equal(got["tgt_doppler_idx"][dop], pl["tgt_doppler_idx"][dop], err_msg=f"{label}: tgt_doppler_idx")
    check_self(got, r.cfg)
    return worst


@pytest.mark.parametrize("nts", XR.NTS_CASES)
def test_nts_c64(xcd, nts):
    r = XR.ref(nts)
    pl = r.plain
    a = _run(xcd, r, probe_column=r.probe_column)                               # the probe on hot chirp 9 of 'hot9'
    _check_c64(r, a, f"nts {nts}", pl["probe"])
    # chirp 0 of the frame whose chirp 0 is 2^K_X0 times larger; without the RD map (the row peaks only)
    f0 = r.index("white_x0")
    b = _run(xcd, r, want_rd=False, probe_column=f0 * XR.PN + 1)
    e = rel_l2(b["probe_mag"], np.abs(pl["cube"][f0, 0]))
    print(f"XCD nts {nts} probe of chirp 0 {e:.2e}")
    assert e <= BAR
    _same(a, b, DECISIONS, f"nts {nts} with and without the RD map")
    check_self(b, r.cfg)


@pytest.mark.parametrize("nts", XR.DEGENERATE_NTS)
def test_nts_degenerate(xcd, nts):
    r = XR.ref(nts)
    pl = r.plain
    got = _run(xcd, r)
    check_self(got, r.cfg)
    if nts == 2:
        # Blackman(2) is zero: what is left is rounding, below 1e-4 of what the calibration tone (|cal| = 0.01)
        # would give through a window of unit gain (test_gpu_edges.test_calibration_only_frames_are_empty)
        tone = 0.01 * nts
        figs = (np.abs(got["profile"]).max(), np.abs(got["rd"]).max(), np.abs(got["slow_mag"]).max())
        print(f"\nXCD nts 2 profile {figs[0]:.2e} rd {figs[1]:.2e} slow {figs[2]:.2e} (bars {1e-4 * tone:.1e}, "
              f"{1e-4 * tone * np.sum(r.wd):.1e})")
        assert figs[0] <= 1e-4 * tone and figs[2] <= 1e-4 * tone and figs[1] <= 1e-4 * tone * float(np.sum(r.wd))
        assert np.all(got["tgt_count"] == 0)
    else:
        e_rd = rd_rel_err(got["rd"], pl["rd"], pl["cube"], r.wd, XR.ND).max()
        e_prof = rel_l2(got["profile"], pl["profile"], axis=1).max()
        print(f"\nXCD nts 4 rd {e_rd:.2e} profile {e_prof:.2e}")
        assert e_rd <= BAR and e_prof <= BAR


# ---------------------------------------------------------------------------
# fp16 storage through process_device
# ---------------------------------------------------------------------------
def _run_fp16(engine, r, frames=None, want_rd=True, probe_column=0):
    """c32h in, c32h RD out.  Every buffer is pre-filled (NaN, -1), the IQ tensor and the RD map have as many
    guard frames behind them, NaN before the call and NaN after it."""
    import torch
    h = r.dev_iq if frames is None else r.dev_iq[frames]
    F, M = h.shape[0], r.cfg.max_targets
    dev = dict(device="cuda")
    nan = float("nan")
    g_iq = Guarded(F, (XR.PN, r.nts, 2), True)
    g_iq.buf.copy_(torch.from_numpy(np.ascontiguousarray(h)))
    g_rd = Guarded(F, (XR.NR, XR.ND, 2), True) if want_rd else None
    outs = dict(profile=torch.full((F, XR.NR), nan, **dev), tgt_count=torch.full((F,), -1, dtype=torch.int32, **dev),
                tgt_range_idx=torch.full((F, M), -1, dtype=torch.int32, **dev), tgt_range_mag=torch.full((F, M), nan, **dev),
                tgt_doppler_idx=torch.full((F, M), -1, dtype=torch.int32, **dev), slow_mag=torch.full((F, XR.PN), nan, **dev))
    if probe_column:
        outs["probe_mag"] = torch.full((XR.NR,), nan, **dev)
    engine.set_taps(r.cfg, r.cal, r.wr, r.wd)
    torch.cuda.synchronize()
    engine.process_device(g_iq.buf, F, FMCW_C32H, outs, d_rd=g_rd.buf if want_rd else None, out_dtype=FMCW_C32H,
                          probe_column=probe_column, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    engine.synchronize()
    g_iq.check()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    got["probe"] = got.pop("probe_mag", None)
    if want_rd:
        g_rd.check()
        got["rd"] = g_rd.buf.cpu().numpy()                                     # float16 pairs holding D / (Nr Nd)
        assert not np.isnan(got["rd"]).any()
    assert not any(np.isnan(got[k]).any() for k in ("profile", "tgt_range_mag", "slow_mag"))
    return got


def _rd128(got):
    v = got["rd"].astype(np.float64) * (XR.NR * XR.ND)
    return v[..., 0] + 1j * v[..., 1]


def _near_choices(r, chain, f) -> set:
    """What :227-239 may return for target 0 of frame f of `chain` when the maximum is any of the bins within
    streams_reference.ROW_GAP of the row's largest: that bin, or the fallback index where the maximum is
    below doppler_thr or the bin is the fallback's own (both outcomes where the maximum is within ROW_GAP of
    the threshold)."""
    thr, fb = r.p["doppler_thr"], r.cfg.doppler_fallback_idx
    mx = np.abs(chain["rd"][f, chain["tgt_range_idx"][f, 0] - 1]).max()
    passes = {mx >= thr} if abs(mx - thr) > SR.ROW_GAP * max(mx, thr) else {True, False}
    return {d if (ok and d != fb) else fb for d in SR.near_max_bins(chain, f, 0) for ok in passes}


def _check_fp16(r, got, mask, label, blocks=False):
    """Against the plain chain on the fp16-exact input at bound(e_ref) of emulate_xcd under `mask`."""
    pl, emu = r.plain, r.emu(mask, FMCW_C32H)
    rd = _rd128(got)
    keep_rd = np.array([not XR.fp16_left_out(r.nts, n, r.taps) for n in r.names])   # e_ref above E_REF_MAX (asserted on the host)
    err = SR.errors(dict(got, rd=rd), pl)
    line = []
    for k, e in err.items():
        sel = keep_rd if k == "rd" else np.ones(len(e), bool)
        lim = SR.bound(emu["e_ref"][k])
        line.append(f"{k} {np.max(e[sel]):.2e}/{np.max(emu['e_ref'][k][sel]):.2e}")
        err[k] = (e, lim, sel)
    # the profile of the blocks the mask leaves fp32, the slow rows and the target magnitudes come from fp32 values
    keep = P.fp16_fp32_bins(r.cfg) if mask else np.ones(XR.NR, bool)
    e_keep = rel_l2(got["profile"][:, keep], pl["profile"][:, keep], axis=1)
    has = pl["tgt_count"] > 0
    e_slow = rel_l2(got["slow_mag"][has], pl["slow_mag"][has], axis=1) if has.any() else np.zeros(1)
    e_mag = np.abs(got["tgt_range_mag"][has, 0] / pl["tgt_range_mag"][has, 0] - 1.0) if has.any() else np.zeros(1)
    # the white and one-hot frames per group (all that the RD comparison holds: xcd_reference.fp16_left_out)
    ge_ref = XR.group_e_ref(emu["rd"], pl["rd"])
    g_worst, g_fail = (0.0, 0.0, ""), []
    for f in r.flat():
        if not keep_rd[f]:
            continue
        for g in range(XR.NGROUPS):
            e = float(rel_l2(rd[f][XR.GROUP_ROWS[g]], pl["rd"][f][XR.GROUP_ROWS[g]]))
            if e > g_worst[0]:
                g_worst = (e, ge_ref[f, g], f"{r.names[f]} g{g}")
            if e > SR.bound(ge_ref[f, g]):
                g_fail.append((r.names[f], g, e, ge_ref[f, g]))
    b_fail, b_worst = [], {"rd": (0.0, 0.0, ""), "profile": (0.0, 0.0, "")}
    if blocks:
        for key, val in (("rd", rd), ("profile", got["profile"])):
            be_ref = XR.block_e_ref(emu, pl, key)
            for f in range(r.F):
                if key == "rd" and not keep_rd[f]:
                    continue
                for b in range(8):
                    e = float(rel_l2(val[f][128 * b:128 * b + 128], pl[key][f][128 * b:128 * b + 128]))
                    lim = BAR if (key == "profile" and not (mask >> b) & 1) else SR.bound(be_ref[f, b])
                    if e > b_worst[key][0]:
                        b_worst[key] = (e, be_ref[f, b], f"{r.names[f]} b{b}")
                    if e > lim:
                        b_fail.append((key, r.names[f], b, e, be_ref[f, b]))
    print(f"\nXCD {label} mask {mask:#04x} F {r.F} " + " ".join(line) + f" fp32 blocks {e_keep.max():.2e} slow {e_slow.max():.2e} "
          f"mag {e_mag.max():.2e} group {g_worst[0]:.2e}/{g_worst[1]:.2e} ({g_worst[2]})"
          + (" block " + " ".join(f"{k} {v[0]:.2e}/{v[1]:.2e} ({v[2]})" for k, v in b_worst.items()) if blocks else ""))
    for k, (e, lim, sel) in err.items():
        assert np.all(np.isfinite(e)) and np.all(e[sel] <= lim[sel]), (label, k, e, lim)
    assert e_keep.max() <= BAR and e_slow.max() <= BAR and e_mag.max() <= BAR, (label, e_keep.max(), e_slow.max(), e_mag.max())
    assert not g_fail, (label, g_fail[:5])
    assert not b_fail, (label, b_fail[:5])
    # detections: the peak rule reads fp32 blocks only, so exactly the plain chain's; the Doppler index exact where
    # the emulated and the plain chain agree on a row whose two largest magnitudes are 1e-3 apart, else within
    # that band of the maximum; always by the self-consistent rule on the returned values
    np.testing.assert_array_equal(got["tgt_count"], pl["tgt_count"])
    np.testing.assert_array_equal(got["tgt_range_idx"], pl["tgt_range_idx"])
    assert np.all(got["slow_mag"][~has] == 0)
    exact = r.doppler_mask(mask, FMCW_C32H)
    np.testing.assert_array_equal(got["tgt_doppler_idx"][exact], pl["tgt_doppler_idx"][exact])
    for f in np.nonzero(has)[0]:
        if not exact[f, 0]:
            near = _near_choices(r, pl, f) | _near_choices(r, emu, f)
            assert int(got["tgt_doppler_idx"][f, 0]) in near, (label, r.names[f], got["tgt_doppler_idx"][f, 0], near)
    check_self(got, r.cfg)


@pytest.mark.parametrize("nts", XR.FP16_NTS)
def test_nts_fp16(xcd, nts):
    r = XR.ref(nts, FMCW_C32H)
    got = _run_fp16(xcd, r, probe_column=r.probe_column)
    _check_fp16(r, got, r.mask, f"fp16 nts {nts}")


MASK_RUNS = [(m, True) for m in XR.MASK_GATES] + [(0xFE, False)]


@pytest.mark.parametrize("gate,s16", MASK_RUNS, ids=[f"{m:02x}{'' if s else '-s16off'}" for m, s in MASK_RUNS])
def test_handoff_masks(xcd, monkeypatch, gate, s16):
    r = XR.mask_ref(gate)
    assert r.mask == gate
    if not s16:
        monkeypatch.setenv("FMCW_S16", "0")
    got = _run_fp16(xcd, r)
    monkeypatch.delenv("FMCW_S16", raising=False)
    _check_fp16(r, got, gate if s16 else 0, f"gate {gate:#04x}{'' if s16 else ' FMCW_S16=0'}", blocks=True)
    if gate == 0xFF:
        assert np.all(got["tgt_count"] == 0) and np.all(got["slow_mag"] == 0)
    # without the RD map (the c32h hand-off with the row peaks only): the same decisions
    b = _run_fp16(xcd, r, want_rd=False) if s16 else None
    if b is not None:
        _same(got, b, DECISIONS, f"gate {gate:#04x} with and without the RD map")


# ---------------------------------------------------------------------------
# frame count against teams, slots and steps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("F", XR.FRAME_COUNTS)
def test_frame_count(xcd, F):
    r = XR.count_ref(F)
    a = _run(xcd, r, probe_column=r.probe_column)
    _check_c64(r, a, f"count {F}", r.plain["probe"])
    b = _run(xcd, r, want_rd=False)
    _same(a, b, DECISIONS, f"F {F} with and without the RD map")
    # team index, slot parity and step position against the frame's content: each frame alone gives the same bits
    for f in range(F):
        one = _run(xcd, r, iq=r.dev_iq[f:f + 1])
        for k in DECISIONS + ("rd",):
            np.testing.assert_array_equal(one[k][0], a[k][f], err_msg=f"F {F} frame {f} alone: {k}")
        one = _run(xcd, r, iq=r.dev_iq[f:f + 1], want_rd=False)
        for k in DECISIONS:
            np.testing.assert_array_equal(one[k][0], a[k][f], err_msg=f"F {F} frame {f} alone, no RD map: {k}")


@pytest.mark.parametrize("F", XR.FRAME_COUNTS_FP16)
def test_frame_count_fp16(xcd, F):
    r = XR.count_ref(F, FMCW_C32H)
    a = _run_fp16(xcd, r, probe_column=r.probe_column)
    _check_fp16(r, a, r.mask, f"fp16 count {F}")
    b = _run_fp16(xcd, r, want_rd=False)
    _same(a, b, DECISIONS, f"fp16 F {F} with and without the RD map")
    for f in range(F):
        one = _run_fp16(xcd, r, frames=slice(f, f + 1))
        for k in DECISIONS + ("rd",):
            np.testing.assert_array_equal(one[k][0], a[k][f], err_msg=f"fp16 F {F} frame {f} alone: {k}")
        one = _run_fp16(xcd, r, frames=slice(f, f + 1), want_rd=False)
        for k in DECISIONS:
            np.testing.assert_array_equal(one[k][0], a[k][f], err_msg=f"fp16 F {F} frame {f} alone, no RD map: {k}")


@pytest.mark.parametrize("nts", XR.CHUNK_NTS)
def test_chunks(xcd, nts):
    r = XR.ref(nts)
    a = _run(xcd, r, probe_column=r.probe_column)
    for n in (3, 8):
        xcd.set_chunk_frames(n)
        b = _run(xcd, r, probe_column=r.probe_column)
        assert set(a) == set(b)
        _same(a, b, sorted(a), f"nts {nts} in chunks of {n}")
    xcd.set_chunk_frames(0)
