"""GPU: the 2-D CA-CFAR stage (csrc/kernels_cfar.hip through fmcw_cfar / fmcw_cfar_device) against
the float64 reference of tests/cfar_reference.py, which always runs on exactly the bytes the device
is given -- the only difference is float32 arithmetic, and the reference marks the cells whose
outcome that may flip (at most 1 in 10^4 of the gated cells, else the test fails; none on the inputs
here, so the comparisons are exact: counts, index lists and mask equal, det_power at rtol 8 2^-24,
det_noise at rtol (N + 8) 2^-24, unused entries 0)."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64, FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS, FmcwError, _lib
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import cfar_reference as R
from tests.helpers import case
from tests.test_cfar_host import REJECTED

pytestmark = pytest.mark.gpu

# (nts, pn, nr, nd) -> frames (from frame 0 of the synthetic stream)
GEOS = {(64, 16, 256, 16): 12, (100, 20, 128, 32): 5, (256, 32, 256, 32): 6, (1024, 256, 1024, 256): 2}
OUT_KEYS = ("det_count", "det_range_idx", "det_doppler_idx", "det_power", "det_noise")
_RD = {}


def rd_map(geo):
    """complex64 [F][nr][nd]: the oracle's RD map (every range row) of the geometry's frames, made once."""
    if geo not in _RD:
        nts, pn, nr, nd = geo
        _, p, wr, wd, cal = case(nts, pn, nr, nd)
        iq = O.synth_frames(GEOS[geo], pn, nts, nr, nd, p["dist_per_bin"])
        rd = O.process_frames(iq, cal, p, wr, wd, want_rd=True, rd_all_rows=True)["rd"].astype(np.complex64)
        rd.setflags(write=False)
        _RD[geo] = rd
    return _RD[geo]


def halves(rd):
    """fp16 storage of an RD map: float16 [F][nr][nd][2] holding D / (nr nd)."""
    nr, nd = rd.shape[1:]
    return (np.stack([rd.real, rd.imag], -1) / np.float32(nr * nd)).astype(np.float16)


def cfg_for(nr, pfa, guard=(1, 1), train=(2, 2), max_det=1024, local_max=False, gate=None):
    q = P.CfarConfig(guard_r=guard[0], guard_d=guard[1], train_r=train[0], train_d=train[1], max_det=max_det,
                     local_max=local_max)
    q.r_lo, q.r_hi = gate if gate is not None else (3, nr - 2)
    q.alpha = P.CfarConfig.alpha_for(q.n_train_full, pfa)
    return q


def reference(rd, q):
    return R.cfar_reference(rd, (q.guard_r, q.guard_d), (q.train_r, q.train_d), q.alpha, q.r_lo, q.r_hi, q.local_max)


def run_and_check(engine, rd, q):
    got = engine.cfar(rd, q, want_mask=True)
    ref = reference(rd, q)
    R.assert_matches(got, ref, q.max_det, got["mask"])
    return got, ref


# ---- 1. parity, complex64 ------------------------------------------------------------------------
@pytest.mark.parametrize("local_max", [False, True], ids=["all", "local_max"])
@pytest.mark.parametrize("pfa", [1e-3, 1e-5])
@pytest.mark.parametrize("geo", sorted(GEOS), ids=lambda g: "x".join(map(str, g)))
def test_parity_c64(engine, geo, pfa, local_max):
    """nd = 16 and 32 make the circular wrap a large share of the map; the gate 3..nr-2 reaches rows
    whose window is clipped."""
    rd = rd_map(geo)
    got, ref = run_and_check(engine, rd, cfg_for(geo[2], pfa, local_max=local_max))
    assert got["det_count"].sum() > 0 and ref["N"][2] < ref["N"][8]


# ---- 2. largest window -----------------------------------------------------------------------------
@pytest.mark.parametrize("geo,guard,train", [((64, 16, 256, 16), (8, 2), (6, 2)),
                                             ((1024, 256, 1024, 256), (8, 8), (8, 8))], ids=["256x16", "1024x256"])
@pytest.mark.parametrize("local_max", [False, True], ids=["all", "local_max"])
def test_largest_window(engine, geo, guard, train, local_max):
    """Wr = 14 at 256 x 16 (2 Wd + 1 = 9 of the 16 Doppler bins) and Wr = Wd = 16 at 1024 x 256: the halo."""
    run_and_check(engine, rd_map(geo), cfg_for(geo[2], 1e-3, guard, train, local_max=local_max))


@pytest.mark.parametrize("guard,train", [((0, 0), (1, 0)), ((0, 0), (0, 1)), ((2, 0), (0, 3)), ((0, 3), (2, 0)),
                                         ((1, 1), (2, 2))])
def test_degenerate_windows_and_the_whole_map(engine, guard, train):
    """Windows with no training rows or no training columns, no guard, and the gate 0, 0 (every
    row, the clipped first and last ones included) at nd 32."""
    geo = (100, 20, 128, 32)
    q = cfg_for(geo[2], 1e-2, guard, train, local_max=True, gate=(0, 0))
    run_and_check(engine, rd_map(geo), q)


# ---- 3. overflow -------------------------------------------------------------------------------------
def test_overflow_keeps_the_first_in_raster_order(engine):
    geo = (1024, 256, 1024, 256)
    rd = rd_map(geo)
    got, ref = run_and_check(engine, rd, cfg_for(1024, 1e-3, max_det=64))
    assert got["det_count"].tolist() == [464, 449]                       # the full number, not 64
    assert got["mask"].sum(axis=(1, 2)).tolist() == [464, 449]           # the mask is complete
    for f in range(2):
        r, d = np.nonzero(ref["det"][f])
        np.testing.assert_array_equal(got["det_range_idx"][f], r[:64] + 1)
        np.testing.assert_array_equal(got["det_doppler_idx"][f], d[:64] + 1)
    # max_det 1: the first detection alone
    one = engine.cfar(rd, cfg_for(1024, 1e-3, max_det=1))
    np.testing.assert_array_equal(one["det_range_idx"], got["det_range_idx"][:, :1])
    np.testing.assert_array_equal(one["det_power"], got["det_power"][:, :1])
    assert one["det_count"].tolist() == [464, 449]


# ---- 4. fp16 storage ---------------------------------------------------------------------------------
@pytest.mark.parametrize("local_max", [False, True], ids=["all", "local_max"])
@pytest.mark.parametrize("pfa", [1e-3, 1e-5])
@pytest.mark.parametrize("geo", [(256, 32, 256, 32), (1024, 256, 1024, 256)], ids=["256x32", "1024x256"])
def test_fp16_storage(engine, geo, pfa, local_max):
    """The reference runs on the halves the device is given, times nr nd; the outputs are in the
    units of |D|^2 (the (nr nd)^2 is exact)."""
    h = halves(rd_map(geo))
    got, _ = run_and_check(engine, h, cfg_for(geo[2], pfa, local_max=local_max))
    assert got["det_count"].sum() > 0


# ---- 5. known answer, end to end ------------------------------------------------------------------------
@pytest.mark.parametrize("geo,guard,train,pipe", [((1024, 256, 1024, 256), (4, 4), (4, 4), FMCW_PIPE_AUTO),
                                                  ((256, 32, 256, 32), (4, 3), (4, 4), FMCW_PIPE_STREAMS)],
                         ids=["1024x256_auto", "256x32_streams"])
def test_known_answer_end_to_end(geo, guard, train, pipe):
    """IQ in, detections out on one stream (process_cfar_device): frames 40-46 of the synthetic
    stream hold one target each, whose cell is the detection with the largest power / noise; frame
    47 has none.  The whole output equals the reference applied to the RD map the device wrote."""
    import torch
    from fmcw_radar_processing_amd.engine import Engine
    nts, pn, nr, nd = geo
    cfg, p, wr, wd, cal = case(nts, pn, nr, nd, P.THROUGHPUT)
    F, dev = 8, "cuda"
    iq = O.synth_frames(F, pn, nts, nr, nd, p["dist_per_bin"], frame0=40)
    q = P.CfarConfig.for_config(cfg, pfa=1e-6, guard=guard, train=train, max_det=64, local_max=True)
    K, M = q.max_det, cfg.max_targets
    eng = Engine(0)
    try:
        eng.set_taps(cfg, cal, wr, wd)
        eng.set_pipeline(pipe)
        d_iq = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32).reshape(F, pn, nts, 2)).to(dev)
        outs = dict(profile=torch.empty((F, nr), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                    tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                    tgt_range_mag=torch.empty((F, M), device=dev),
                    tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                    slow_mag=torch.empty((F, pn), device=dev))
        d_rd = torch.full((F, nr, nd, 2), np.nan, dtype=torch.float32, device=dev)
        co = dict(det_count=torch.full((F,), -3, dtype=torch.int32, device=dev),
                  det_range_idx=torch.full((F, K), -3, dtype=torch.int32, device=dev),
                  det_doppler_idx=torch.full((F, K), -3, dtype=torch.int32, device=dev),
                  det_power=torch.full((F, K), np.nan, device=dev), det_noise=torch.full((F, K), np.nan, device=dev))
        d_mask = torch.full((F, nr, nd), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        eng.process_cfar_device(d_iq, F, FMCW_C64, outs, q, d_rd, co, d_mask=d_mask, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        eng.synchronize()
        got = {k: v.cpu().numpy() for k, v in co.items()}
        rd = d_rd.cpu().numpy().view(np.complex64)[..., 0]
        mask = d_mask.cpu().numpy()
    finally:
        eng.close()
    R.assert_matches(got, reference(rd, q), K, mask)
    for i in range(F):
        fp = O.synth_frame_params(40 + i, nr, nd, p["dist_per_bin"])
        n = min(int(got["det_count"][i]), K)
        if fp["A"] == 0:
            assert i == 7 and n == 0
            continue
        assert n >= 1
        best = np.argmax(got["det_power"][i, :n] / got["det_noise"][i, :n])
        assert (got["det_range_idx"][i, best], got["det_doppler_idx"][i, best]) == (fp["r"] + 1, fp["d"] + nd // 2 + 1)


# ---- 6. determinism ------------------------------------------------------------------------------------
def _same(a, b, keys=OUT_KEYS + ("mask",)):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_frames_are_independent(engine):
    """The 12-frame call equals twelve one-frame calls, byte for byte (the strip height follows the
    frame count; the results do not)."""
    rd = rd_map((64, 16, 256, 16))
    q = cfg_for(256, 1e-3, local_max=True)
    whole = engine.cfar(rd, q, want_mask=True)
    for f in range(len(rd)):
        one = engine.cfar(rd[f:f + 1], q, want_mask=True)
        _same(one, {k: whole[k][f:f + 1] for k in one})
    big = rd_map((1024, 256, 1024, 256))
    q = cfg_for(1024, 1e-3, (4, 2), (3, 5), max_det=700)
    whole = engine.cfar(big, q, want_mask=True)
    assert whole["det_count"].min() > 0
    for f in range(len(big)):
        one = engine.cfar(big[f:f + 1], q, want_mask=True)
        _same(one, {k: whole[k][f:f + 1] for k in one})


def test_call_sequence_on_one_context():
    """Geometry A with config 1, then B with config 2 (fp16 storage, another window, cut list), then A
    with config 1 again, on one context: the first and the third result are identical, and equal a
    new context's."""
    from fmcw_radar_processing_amd.engine import Engine
    a, b = rd_map((1024, 256, 1024, 256)), halves(rd_map((256, 32, 256, 32)))
    q1 = cfg_for(1024, 1e-3, (2, 2), (4, 4), max_det=512, local_max=True)
    q2 = cfg_for(256, 1e-3, (1, 3), (6, 2), max_det=5)
    seq, fresh = Engine(0), Engine(0)
    try:
        first = seq.cfar(a, q1, want_mask=True)
        other = seq.cfar(b, q2, want_mask=True)
        third = seq.cfar(a, q1, want_mask=True)
        want = fresh.cfar(a, q1, want_mask=True)
    finally:
        seq.close()
        fresh.close()
    _same(first, third)
    _same(first, want)
    R.assert_matches(first, reference(a, q1), q1.max_det, first["mask"])
    R.assert_matches(other, reference(b, q2), q2.max_det, other["mask"])


def test_shards_are_bit_identical():
    from fmcw_radar_processing_amd.engine import Engine
    rd = rd_map((64, 16, 256, 16))
    q = cfg_for(256, 1e-3, max_det=4)
    multi, single = Engine([0, 0, 0]), Engine(0)
    try:
        _same(multi.cfar(rd, q, want_mask=True), single.cfar(rd, q, want_mask=True))
    finally:
        multi.close()
        single.close()


def test_chunk_seams_of_both_calls(engine, monkeypatch):
    """The host call cut into one-frame chunks (FMCW_HOST_CHUNK=1) and the device call cut into
    launch pairs of 5, 5 and 2 frames (FMCW_CFAR_SCRATCH: room for five frames' lists) give the
    bytes of the uncut calls; timing stage cfar counts the three launch pairs."""
    import torch
    rd = rd_map((64, 16, 256, 16))
    F, nr, nd = rd.shape
    q = cfg_for(nr, 1e-3, max_det=16, local_max=True)
    want = engine.cfar(rd, q, want_mask=True)
    want_h = engine.cfar(halves(rd), q, want_mask=True)
    assert want["det_count"].min() > 0 and want_h["det_count"].sum() > 0
    monkeypatch.setenv("FMCW_HOST_CHUNK", "1")
    _same(engine.cfar(rd, q, want_mask=True), want)
    _same(engine.cfar(halves(rd), q, want_mask=True), want_h)
    monkeypatch.delenv("FMCW_HOST_CHUNK")
    # 12 frames at 256 x 16 run as strips of 16 rows, one wave each: 16 lists of 16 entries of 16 bytes + 16 counts
    per_frame = 16 * (16 * 16 + 4)
    monkeypatch.setenv("FMCW_CFAR_SCRATCH", str(5 * per_frame + per_frame // 2))
    d_rd = torch.from_numpy(np.array(rd).view(np.float32).reshape(F, nr, nd, 2)).to("cuda")
    outs = _device_buffers(F, nr, nd, 16)
    d_mask = torch.full((F, nr, nd), 9, dtype=torch.uint8, device="cuda")
    engine.timing_reset()
    engine.timing(1)
    try:
        engine.cfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, d_mask=d_mask, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert engine.timing_read()["cfar"][1] == 3
    finally:
        engine.timing(0)
        engine.timing_reset()
    got = {k: v.cpu().numpy() for k, v in outs.items()} | {"mask": d_mask.cpu().numpy()}
    _same(got, want)


# ---- 7. arguments ----------------------------------------------------------------------------------------
def _device_buffers(F, nr, nd, K, fill=-3):
    import torch
    dev = "cuda"
    return dict(det_count=torch.full((F,), fill, dtype=torch.int32, device=dev),
                det_range_idx=torch.full((F, K), fill, dtype=torch.int32, device=dev),
                det_doppler_idx=torch.full((F, K), fill, dtype=torch.int32, device=dev),
                det_power=torch.full((F, K), float(fill), device=dev),
                det_noise=torch.full((F, K), float(fill), device=dev))


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_device_call_rejects_what_the_check_rejects(engine, name):
    """E_ARG before any launch: the outputs keep what they held, timing stage cfar counts nothing."""
    import torch
    over, nr, nd = REJECTED[name]
    q = P.CfarConfig(max_det=8, alpha=7.54)
    for k, v in over.items():
        setattr(q, k, v)
    K = 8
    d_rd = torch.zeros((1, nr, nd, 2), dtype=torch.float32, device="cuda")
    outs = _device_buffers(1, nr, nd, K)
    engine.timing_reset()
    engine.timing(1)
    try:
        with pytest.raises(FmcwError, match="E_ARG"):
            engine.cfar_device(q, d_rd, FMCW_C64, 1, nr, nd, outs, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert engine.timing_read()["cfar"][1] == 0
    finally:
        engine.timing(0)
    for v in outs.values():
        assert bool((v == -3).all())


def test_device_call_arguments_and_timing(engine):
    import torch
    geo = (64, 16, 256, 16)
    rd = rd_map(geo)
    F, nr, nd = rd.shape
    q = cfg_for(nr, 1e-3, max_det=16)
    d_rd = torch.from_numpy(np.array(rd).view(np.float32).reshape(F, nr, nd, 2)).to("cuda")
    outs = _device_buffers(F, nr, nd, 16)
    s = torch.cuda.current_stream()
    # F = 0 is a no-op; a bad dtype, a missing output and an unaligned map are argument errors
    engine.cfar_device(q, d_rd, FMCW_C64, 0, nr, nd, outs, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.cfar_device(q, d_rd, 2, F, nr, nd, outs, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.cfar_device(q, d_rd, FMCW_C64, -1, nr, nd, outs, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.cfar_device(q, d_rd, FMCW_C64, F, nr, nd, dict(outs, det_noise=None), stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.cfar_device(q, d_rd.view(-1)[2:], FMCW_C64, F - 1, nr, nd, outs, stream=s)
    torch.cuda.synchronize()
    for v in outs.values():
        assert bool((v == -3).all())
    # timing stage `cfar`: one event pair per launch pair, nothing when timing is off
    engine.timing_reset()
    engine.cfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, stream=s)
    torch.cuda.synchronize()
    assert engine.timing_read()["cfar"] == (0.0, 0)
    engine.timing(1)
    try:
        engine.cfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, stream=s)
        engine.cfar_device(q, d_rd, FMCW_C64, 1, nr, nd, outs, stream=s)
        torch.cuda.synchronize()
        ms, n = engine.timing_read()["cfar"]
        assert n == 2 and ms > 0
    finally:
        engine.timing(0)
        engine.timing_reset()
    # without a mask the lists are the same as with one (the host call, checked against the reference above)
    engine.cfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, stream=s)
    torch.cuda.synchronize()
    want = engine.cfar(rd, q, want_mask=True)
    _same({k: v.cpu().numpy() for k, v in outs.items()}, want, OUT_KEYS)
    assert "range_m" not in want or want["range_m"].shape == want["det_range_idx"].shape


def test_cfar_result_carries_metres_and_speed():
    """With the geometry's taps set, Engine.cfar adds range_m / speed_mps of the listed detections
    (cfg.range_m, cfg.speed); NaN where unused."""
    from fmcw_radar_processing_amd.engine import Engine
    geo = (64, 16, 256, 16)
    cfg, p, wr, wd, cal = case(*geo)
    eng = Engine(0)
    try:
        eng.set_taps(cfg, cal, wr, wd)
        got = eng.cfar(rd_map(geo), cfg_for(256, 1e-3, max_det=16))
    finally:
        eng.close()
    used = got["det_range_idx"] > 0
    assert used.any() and np.isnan(got["range_m"][~used]).all() and np.isnan(got["speed_mps"][~used]).all()
    np.testing.assert_array_equal(got["range_m"][used], cfg.range_m(got["det_range_idx"][used]))
    np.testing.assert_array_equal(got["speed_mps"][used], cfg.speed(got["det_doppler_idx"][used]))
