"""GPU: the single-pass XCD-team schedule (FMCW_PIPE_XCD, kernels_xcd.hip k_rdx +
kernels_detect.hip) against the float64 oracle and against the streams schedule.

k_rdx computes the range FFT as DFT8 x DFT16 x DFT8 with the frame's reference chirp
subtracted (static-target cancellation) instead of the Stockham FFT of k_range, so it
agrees with the streams schedule to fp32 rounding, not bit for bit; both are held to
the SURVEY.md 8d tolerances against the oracle.  FMCW_PIPE_ONEPASS names the same
schedule (ABI 2's 8-tile single pass is retired).
"""
import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_PIPE_AUTO, FMCW_PIPE_ONEPASS, FMCW_PIPE_STREAMS, FMCW_PIPE_XCD, FmcwError
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests.helpers import TOL_FP32_REL_L2, case, near_tie_frames, rd_rel_err, rel_l2

pytestmark = pytest.mark.gpu


def _frames(F, nts=1024, frame0=0):
    cfg, p, wr, wd, cal = case(nts, 256, 1024, 256, P.THROUGHPUT)
    iq = O.synth_frames(F, 256, nts, 1024, 256, p["dist_per_bin"], frame0=frame0)
    return cfg, p, wr, wd, cal, iq


# the single-pass schedule, by both of its names (FMCW_PIPE_ONEPASS is FMCW_PIPE_XCD since ABI 3)
@pytest.fixture(params=[FMCW_PIPE_XCD], ids=["xcd"])
def onepass(engine, request):
    engine.set_pipeline(request.param)
    yield engine
    engine.set_pipeline(FMCW_PIPE_AUTO)
    engine.set_chunk_frames(0)


def _check_vs_oracle(cfg, got, ref, wd, probe=None):
    # fp32: per-frame relative L2 <= 1e-5 (RD normalisation: helpers.rd_rel_err)
    assert rd_rel_err(got["rd"], ref["rd"], ref["cube"], wd, cfg.nd).max() <= TOL_FP32_REL_L2
    assert rel_l2(got["profile"], ref["profile"], axis=1).max() <= TOL_FP32_REL_L2
    ok = ~near_tie_frames(ref["profile"])
    for k in ("tgt_count", "tgt_range_idx", "tgt_doppler_idx"):
        np.testing.assert_array_equal(got[k][ok], ref[k][ok], err_msg=k)
    np.testing.assert_allclose(got["tgt_range_mag"], ref["tgt_range_mag"], rtol=1e-5, atol=0)
    has = ref["tgt_count"] > 0
    if has.any():
        assert rel_l2(got["slow_mag"][has], ref["slow_mag"][has], axis=1).max() <= TOL_FP32_REL_L2
    assert np.all(got["slow_mag"][~has] == 0)
    if probe is not None:
        col = probe - 1
        want = np.abs(ref["cube"][col // cfg.pn, col % cfg.pn, :])
        assert rel_l2(got["probe_mag"], want) <= TOL_FP32_REL_L2


# F = 3: fewer frames than XCDs; 21: a partial group of 8; nts 1000: zero-padding
# to Nr 1024 (masked loads, taps 0 beyond NTS)
@pytest.mark.parametrize("F,nts", [(3, 1024), (21, 1024), (9, 1000)])
def test_onepass_matches_oracle(onepass, F, nts):
    cfg, p, wr, wd, cal, iq = _frames(F, nts, frame0=100)
    onepass.set_taps(cfg, cal, wr, wd)
    probe = min(100 + 256 * (F // 2), F * 256)
    got = onepass.process(iq, want_rd=True, probe_column=probe)
    ref = O.process_frames(iq, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    _check_vs_oracle(cfg, got, ref, wd, probe)


def test_onepass_slow_row_fix_path(onepass, monkeypatch):
    """With no candidates kept, every slow-time row comes from k_slow_fix."""
    monkeypatch.setenv("FMCW_ONEPASS_FORCE_FIX", "1")
    cfg, p, wr, wd, cal, iq = _frames(10, frame0=300)
    onepass.set_taps(cfg, cal, wr, wd)
    got = onepass.process(iq, want_rd=True)
    ref = O.process_frames(iq, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    assert (ref["tgt_count"] > 0).sum() >= 5
    _check_vs_oracle(cfg, got, ref, wd)


def test_onepass_without_rd_output(onepass):
    """RD not requested: only the row peaks are kept; detections unchanged."""
    cfg, p, wr, wd, cal, iq = _frames(12, frame0=55)
    onepass.set_taps(cfg, cal, wr, wd)
    a = onepass.process(iq, want_rd=True)
    b = onepass.process(iq, want_rd=False)
    for k in ("profile", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "slow_mag"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_onepass_chunking_invariant(onepass):
    cfg, p, wr, wd, cal, iq = _frames(20, frame0=9)
    onepass.set_taps(cfg, cal, wr, wd)
    a = onepass.process(iq, want_rd=True, probe_column=2000)
    onepass.set_chunk_frames(7)
    b = onepass.process(iq, want_rd=True, probe_column=2000)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_onepass_agrees_with_streams(onepass):
    cfg, p, wr, wd, cal, iq = _frames(16, frame0=7)
    onepass.set_taps(cfg, cal, wr, wd)
    a = onepass.process(iq, want_rd=True, probe_column=300)
    onepass.set_pipeline(FMCW_PIPE_STREAMS)
    b = onepass.process(iq, want_rd=True, probe_column=300)
    for k in ("tgt_count", "tgt_range_idx", "tgt_doppler_idx"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert rel_l2(a["rd"], b["rd"], axis=(1, 2)).max() <= 2 * TOL_FP32_REL_L2
    assert rel_l2(a["profile"], b["profile"], axis=1).max() <= 2 * TOL_FP32_REL_L2


def test_onepass_known_answer(onepass):
    """Integer-bin range tone r -> idx r+1; Doppler tone d -> d+Nd/2+1 (0 -> fallback)."""
    cfg, p, wr, wd, cal, iq = _frames(8, frame0=40)
    onepass.set_taps(cfg, cal, wr, wd)
    got = onepass.process(iq)
    for i in range(iq.shape[0]):
        fp = O.synth_frame_params(40 + i, 1024, 256, p["dist_per_bin"])
        if fp["A"] == 0:
            assert got["tgt_count"][i] == 0
            continue
        assert got["tgt_range_idx"][i, 0] == fp["r"] + 1
        want = cfg.doppler_fallback_idx if fp["d"] == 0 else fp["d"] + 128 + 1
        assert got["tgt_doppler_idx"][i, 0] == want


def test_xcd_static_target_raw_rd(engine):
    """k_rdx subtracts the frame's chirp 0 before the range FFT (kernels_xcd.hip, reference
    chirp), so a static target (Doppler 0: removed by the :218 mean) cancels before any fp32
    rounding of its large FFT values.  Frames 1904, 1914 and 1923 of the SURVEY 8d stream
    are static; every frame meets the 1e-5 bar on the RAW per-frame relative L2 of the RD
    map (no relaxed normalisation), as the full-size check in bench.py requires."""
    F, f0 = 24, 1904
    cfg, p, wr, wd, cal, iq = _frames(F, frame0=f0)
    static = [i for i in range(F) if O.synth_frame_params(f0 + i, 1024, 256, p["dist_per_bin"])["d"] == 0
              and O.synth_frame_params(f0 + i, 1024, 256, p["dist_per_bin"])["A"] > 0]
    assert len(static) >= 3
    engine.set_pipeline(FMCW_PIPE_XCD)
    try:
        engine.set_taps(cfg, cal, wr, wd)
        got = engine.process(iq, want_rd=True)
        engine.synchronize()
    finally:
        engine.set_pipeline(FMCW_PIPE_AUTO)
    ref = O.process_frames(iq, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    raw = rel_l2(got["rd"], ref["rd"], axis=(1, 2))
    assert raw.max() <= TOL_FP32_REL_L2, (raw.max(), np.argmax(raw))
    _check_vs_oracle(cfg, got, ref, wd)


def test_onepass_rejects_unsupported(onepass):
    cfg, p, wr, wd, cal, iq = _frames(2)
    onepass.set_taps(cfg, cal, wr, wd)
    with pytest.raises(FmcwError, match="E_ARG"):
        onepass.process(iq, want_cube=True)
    cfg, p, wr, wd, cal = case(512, 128, 512, 16, P.THROUGHPUT)
    iq = O.synth_frames(2, 128, 512, 512, 16, p["dist_per_bin"])
    onepass.set_taps(cfg, cal, wr, wd)
    with pytest.raises(FmcwError, match="E_ARG"):
        onepass.process(iq)


def _run_fp16(eng, iq16, F, C, want_rd=True):
    import torch
    from fmcw_radar_processing_amd import FMCW_C32H
    d_iq = torch.from_numpy(iq16).cuda()
    outs = dict(profile=torch.empty((F, 1024), device="cuda"),
                tgt_count=torch.empty(F, dtype=torch.int32, device="cuda"),
                tgt_range_idx=torch.empty((F, 1), dtype=torch.int32, device="cuda"),
                tgt_range_mag=torch.empty((F, 1), device="cuda"),
                tgt_doppler_idx=torch.empty((F, 1), dtype=torch.int32, device="cuda"),
                slow_mag=torch.empty((F, C), device="cuda"))
    d_rd = torch.empty((F, 1024, 256, 2), dtype=torch.float16, device="cuda") if want_rd else None
    eng.process_device(d_iq, F, FMCW_C32H, outs, d_rd=d_rd, out_dtype=FMCW_C32H,
                       stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    if want_rd:   # fp16 outputs hold D / (Nr*Nd) (include/fmcw.h, FMCW_C32H)
        got["rd"] = d_rd.float().cpu().numpy().view(np.complex64)[..., 0].astype(np.complex128) * (1024 * 256)
    return got


def _check_fp16_vs_oracle(cfg, got, ref, wd, s16=True):
    """The fp16-storage bars: ref is the oracle on the fp16-rounded input."""
    from tests.helpers import TOL_FP16_REL_L2, TOL_FP32_REL_L2
    assert rd_rel_err(got["rd"], ref["rd"], ref["cube"], wd, 256).max() <= TOL_FP16_REL_L2
    # the profile in the c32h hand-off blocks (away from the detection window) at the fp16-storage
    # bar, in the blocks around the window (fp32 hand-off) at the fp32 bar; slow rows and target
    # magnitudes from fp32 values at the fp32 bar; detections exact except frames whose two
    # strongest bins are within fp16 rounding of each other
    keep = P.fp16_fp32_bins(cfg) if s16 else np.ones(cfg.nr, bool)
    assert keep.any()
    assert rel_l2(got["profile"][:, keep], ref["profile"][:, keep], axis=1).max() <= TOL_FP32_REL_L2
    if (~keep).any():
        assert rel_l2(got["profile"][:, ~keep], ref["profile"][:, ~keep], axis=1).max() <= TOL_FP16_REL_L2
    ok = ~near_tie_frames(ref["profile"], rtol=1e-3)
    for k in ("tgt_count", "tgt_range_idx", "tgt_doppler_idx"):
        np.testing.assert_array_equal(got[k][ok], ref[k][ok], err_msg=k)
    has = ref["tgt_count"] > 0
    assert has.sum() >= 1
    assert rel_l2(got["slow_mag"][has], ref["slow_mag"][has], axis=1).max() <= TOL_FP32_REL_L2
    m = has & ok
    assert np.max(np.abs(got["tgt_range_mag"][m, 0] - ref["tgt_range_mag"][m, 0]) / ref["tgt_range_mag"][m, 0]) \
        <= TOL_FP32_REL_L2
    assert np.all(got["slow_mag"][~has] == 0)


# fp16 storage (BASELINE config 4 tolerance sweep): c32h IQ in, c32h RD out,
# fp32 arithmetic, through the single pass.  SURVEY 8d: relative L2 <= 3e-3.
# The hand-off under fp16 storage is c32h for the 128-bin blocks that hold no candidate-capable
# bin (FMCW_S16=0: c64 everywhere); the slow rows come from fp32 values either way.
@pytest.mark.parametrize("F,nts,fix,s16", [(3, 1024, False, True), (21, 1024, False, True), (9, 1000, False, True),
                                           (10, 1024, True, True), (21, 1024, False, False)])
def test_onepass_fp16_storage(onepass, monkeypatch, F, nts, fix, s16):
    if fix:
        monkeypatch.setenv("FMCW_ONEPASS_FORCE_FIX", "1")
    if not s16:
        monkeypatch.setenv("FMCW_S16", "0")
    cfg, p, wr, wd, cal, iq = _frames(F, nts, frame0=700)
    onepass.set_taps(cfg, cal, wr, wd)
    iq16 = np.stack([iq.real, iq.imag], -1).astype(np.float16)
    got = _run_fp16(onepass, iq16, F, 256)
    x = iq16.astype(np.float32).view(np.complex64)[..., 0]
    ref = O.process_frames(x, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    _check_fp16_vs_oracle(cfg, got, ref, wd, s16)


def test_onepass_fp16_matches_streams_fp16(engine):
    """AUTO picks the single pass for fp16 storage; it agrees with the streams
    schedule's fp16 path within the fp16 bar, detections exactly."""
    from tests.helpers import TOL_FP16_REL_L2
    F = 16
    cfg, p, wr, wd, cal, iq = _frames(F, frame0=1234)
    engine.set_taps(cfg, cal, wr, wd)
    iq16 = np.stack([iq.real, iq.imag], -1).astype(np.float16)
    try:
        engine.set_pipeline(FMCW_PIPE_AUTO)
        a = _run_fp16(engine, iq16, F, 256)
        engine.set_pipeline(FMCW_PIPE_STREAMS)
        b = _run_fp16(engine, iq16, F, 256)
    finally:
        engine.set_pipeline(FMCW_PIPE_AUTO)
    assert (rel_l2(a["rd"].reshape(F, -1), b["rd"].reshape(F, -1), axis=1) <= TOL_FP16_REL_L2).all()
    for k in ("tgt_count", "tgt_range_idx", "tgt_doppler_idx"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- the XCD-team schedule (kernels_xcd.hip) on its own ----------------------
def test_xcd_slot_ring(engine):
    """One frame per XCD and step: 75 frames = 9-10 steps per team, so every slot of
    the hand-off ring is reused several times; the oracle's fp32 bars hold, and
    FMCW_PIPE_ONEPASS (the same schedule) gives bit-identical outputs."""
    F = 75
    cfg, p, wr, wd, cal, iq = _frames(F, frame0=5000)
    engine.set_taps(cfg, cal, wr, wd)
    try:
        engine.set_pipeline(FMCW_PIPE_XCD)
        a = engine.process(iq, want_rd=True, probe_column=F * 256)
        engine.synchronize()                       # no hand-off error reported
        engine.set_pipeline(FMCW_PIPE_ONEPASS)
        b = engine.process(iq, want_rd=True, probe_column=F * 256)
    finally:
        engine.set_pipeline(FMCW_PIPE_AUTO)
    ref = O.process_frames(iq, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
    _check_vs_oracle(cfg, a, ref, wd, F * 256)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_xcd_deterministic_and_chunked(engine):
    """Two runs are bit-identical, and so are chunks of 13 frames (partial teams)."""
    F = 40
    cfg, p, wr, wd, cal, iq = _frames(F, frame0=777)
    engine.set_taps(cfg, cal, wr, wd)
    try:
        engine.set_pipeline(FMCW_PIPE_XCD)
        a = engine.process(iq, want_rd=True)
        b = engine.process(iq, want_rd=True)
        engine.set_chunk_frames(13)
        c = engine.process(iq, want_rd=True)
    finally:
        engine.set_chunk_frames(0)
        engine.set_pipeline(FMCW_PIPE_AUTO)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)


def test_auto_picks_xcd(engine):
    """AUTO selects the XCD schedule for config-3/4 geometry: bit-identical to FMCW_PIPE_XCD."""
    F = 16
    cfg, p, wr, wd, cal, iq = _frames(F, frame0=31)
    engine.set_taps(cfg, cal, wr, wd)
    try:
        engine.set_pipeline(FMCW_PIPE_AUTO)
        a = engine.process(iq, want_rd=True)
        engine.set_pipeline(FMCW_PIPE_XCD)
        b = engine.process(iq, want_rd=True)
    finally:
        engine.set_pipeline(FMCW_PIPE_AUTO)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
