"""GPU: the 2-D OS-CFAR stage (csrc/kernels_oscfar.hip through fmcw_oscfar / fmcw_oscfar_device) against
the float32 reference of tests/oscfar_reference.py, which always runs on exactly the bytes the device
is given.  The decision is made of compares alone and every float operation of the definition is
rounded on its own, so there is no tolerance and no exempt cell: every comparison is byte equality of
det_count, both index lists, det_power, det_noise and the mask."""
import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C64, FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS, FmcwError
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import oscfar_reference as R
from tests.helpers import case
from tests.test_cfar_host import REJECTED
from tests.test_gpu_cfar import halves, rd_map

pytestmark = pytest.mark.gpu

OUT_KEYS = R.OUT_KEYS
_WIN = {}


def window(key, rd, guard, train):
    """The map-and-window part of the reference (the sorted training powers), made once per map."""
    k = (key, tuple(guard), tuple(train))
    if k not in _WIN:
        _WIN[k] = R.OsWindow(rd, guard, train)
    return _WIN[k]


def parity_map(geo, fp16=False):
    """The oracle's RD map of the geometry (tests/test_gpu_cfar.py); one frame of the 1024 x 256 one."""
    rd = rd_map(geo)
    rd = rd[:1] if geo[2] == 1024 else rd
    return halves(rd) if fp16 else rd


def cfg_for(nr, pfa, rank, guard=(1, 1), train=(2, 2), max_det=1024, local_max=False, gate=None):
    q = P.OsCfarConfig(guard_r=guard[0], guard_d=guard[1], train_r=train[0], train_d=train[1], max_det=max_det,
                       local_max=local_max)
    q.r_lo, q.r_hi = gate if gate is not None else (3, nr - 2)
    n = q.n_train_full
    q.rank = {"1": 1, "half": max(1, n // 2), "3/4": max(1, (3 * n) // 4), "full": n}.get(rank, rank)
    q.alpha = P.OsCfarConfig.alpha_for(n, q.rank, pfa)
    return q


def decide(win, q):
    return win.decide(q.alpha, q.rank, q.r_lo, q.r_hi, q.local_max)


def run_and_check(engine, key, rd, q):
    got = engine.oscfar(rd, q, want_mask=True)
    ref = decide(window(key, rd, (q.guard_r, q.guard_d), (q.train_r, q.train_d)), q)
    R.assert_bytes(got, ref, q.max_det, got["mask"])
    return got, ref


def noise_map(shape, seed, targets=24):
    """complex64 noise of unit power with a few strong cells, some next to each other and some on the
    first and last rows and columns."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)
    F, nr, nd = shape
    for f in range(F):
        r = rng.integers(0, nr, targets)
        d = rng.integers(0, nd, targets)
        x[f, r, d] += rng.uniform(5, 100, targets)
        x[f, 0, 0] += 30
        x[f, nr - 1, nd - 1] += 30
        x[f, nr // 2, nd - 1] += 40
        x[f, nr // 2, 0] += 35
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


# ---- 1. parity, complex64 ------------------------------------------------------------------------
PARITY_GEOS = [(64, 16, 256, 16), (100, 20, 128, 32), (256, 32, 256, 32), (1024, 256, 1024, 256)]


@pytest.mark.parametrize("local_max", [False, True], ids=["all", "local_max"])
@pytest.mark.parametrize("pfa", [1e-3, 1e-5])
@pytest.mark.parametrize("geo", PARITY_GEOS, ids=lambda g: "x".join(map(str, g)))
def test_parity_c64(engine, geo, pfa, local_max):
    """nd = 16 and 32 make the circular wrap a large share of the map; the gate 3..nr-2 reaches rows
    whose window is clipped, where the rank is scaled down."""
    rd = parity_map(geo)
    total = 0
    for rank in ("1", "half", "3/4", "full"):
        got, ref = run_and_check(engine, geo, rd, cfg_for(geo[2], pfa, rank, local_max=local_max))
        total += int(got["det_count"].sum())
        if rank != "1":
            assert ref["k"][2] < ref["k"][8] and ref["N"][2] < ref["N"][8]
        if rank == "3/4":
            assert got["det_count"].sum() > 0
    assert total > 0


# ---- 2. tiles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [512, 1024])
def test_doppler_tiles_and_their_seams(engine, nd):
    """2 and 4 tiles of 256 columns: the halo across the tile seams and the circular wrap; strong
    cells sit on columns 0 and nd - 1 and on rows 0 and nr - 1."""
    rd = noise_map((2, 32, nd), 100 + nd, targets=64)
    for guard, train, lm in (((1, 2), (2, 5), False), ((0, 0), (3, 16), True)):
        got, _ = run_and_check(engine, ("tiles", nd), rd, cfg_for(32, 1e-3, "3/4", guard, train, local_max=lm,
                                                                  gate=(0, 0)))
        assert got["det_count"].min() > 0


def test_smallest_map(engine):
    """3 x 16 x 4 with guard (0, 0), train (1, 1): the window is 3 of the 4 Doppler bins."""
    rd = noise_map((3, 16, 4), 5, targets=3)
    for rank in ("1", "half", "full"):
        for lm in (False, True):
            run_and_check(engine, "smallest", rd, cfg_for(16, 1e-1, rank, (0, 0), (1, 1), local_max=lm, gate=(0, 0)))


# ---- 3. largest window ------------------------------------------------------------------------------
@pytest.mark.parametrize("guard,train", [((0, 0), (16, 16)), ((8, 8), (8, 8))], ids=["train16", "guard8_train8"])
@pytest.mark.parametrize("nd", [256, 64])
def test_largest_window(engine, nd, guard, train):
    """Wr = Wd = 16 (N = 1088 without a guard): the deepest ring, the widest halo and, in the selection,
    18 window positions per lane.  Gate (0, 0) over 64 rows: every row is clipped on one side or the
    other.  The reference's stack is 1088 x 64 x 256 x 4 B = 71 MB at most."""
    rd = noise_map((1, 64, nd), 200 + nd, targets=16)
    win = R.OsWindow(rd, guard, train)
    for rank, lm in (("3/4", False), ("full", True), ("1", False)):
        q = cfg_for(64, 1e-3, rank, guard, train, local_max=lm, gate=(0, 0))
        got = engine.oscfar(rd, q, want_mask=True)
        ref = decide(win, q)
        R.assert_bytes(got, ref, q.max_det, got["mask"])
    assert ref["N"][0] < ref["N"][15] < ref["N"][16] == win.n_full and ref["k"][0] <= ref["k"][16]


# ---- 4. degenerate windows ----------------------------------------------------------------------------
@pytest.mark.parametrize("guard,train", [((0, 0), (1, 0)), ((0, 0), (0, 1)), ((2, 0), (0, 3)), ((0, 3), (2, 0)),
                                         ((1, 1), (2, 2))])
def test_degenerate_windows_and_the_whole_map(engine, guard, train):
    """Windows with no training rows or no training columns, no guard, and the gate 0, 0 (every
    row, the clipped first and last ones included) at nd 32."""
    geo = (100, 20, 128, 32)
    rd = parity_map(geo)
    for rank in ("1", "3/4", "full"):
        run_and_check(engine, geo, rd, cfg_for(geo[2], 1e-2, rank, guard, train, local_max=True, gate=(0, 0)))


# ---- 5. ties ----------------------------------------------------------------------------------------------
def test_ties_and_an_all_zero_frame(engine):
    """A map quantised to 7 distinct powers (most training cells tie with each other and with the
    cell under test), and an all-zero frame between two noise frames: it detects nothing."""
    rng = np.random.default_rng(21)
    x = (rng.integers(0, 7, (2, 64, 32)).astype(np.float32) + 0j).astype(np.complex64)
    total = 0
    for alpha in (0.5, 1.0, 2.0):
        for rank in (1, 20, 40):
            q = cfg_for(64, 1e-3, rank, gate=(0, 0))
            q.alpha = alpha
            got, _ = run_and_check(engine, "ties", x, q)
            total += int(got["det_count"].sum())
    assert total > 0
    z = np.array(noise_map((3, 64, 32), 22))
    z[1] = 0
    got, _ = run_and_check(engine, "zero", z, cfg_for(64, 1e-2, "3/4", gate=(0, 0)))
    assert got["det_count"][1] == 0 and got["det_count"][0] > 0 and got["det_count"][2] > 0
    assert not got["mask"][1].any()


# ---- 6. fp16 storage -------------------------------------------------------------------------------------
@pytest.mark.parametrize("local_max", [False, True], ids=["all", "local_max"])
@pytest.mark.parametrize("geo", [(256, 32, 256, 32), (1024, 256, 1024, 256)], ids=["256x32", "1024x256"])
def test_fp16_storage(engine, geo, local_max):
    """The reference runs on the halves the device is given, widened and times nr nd; the outputs are
    in the units of |D|^2."""
    h = parity_map(geo, fp16=True)
    for pfa, rank in ((1e-3, "3/4"), (1e-5, "half"), (1e-3, "full")):
        got, _ = run_and_check(engine, (geo, "h"), h, cfg_for(geo[2], pfa, rank, local_max=local_max))
    assert got["det_count"].sum() > 0


# ---- 7. cut list -----------------------------------------------------------------------------------------
def test_cut_list_keeps_the_first_in_raster_order(engine):
    rd = noise_map((2, 256, 256), 31, targets=600)
    q = cfg_for(256, 1e-3, "3/4", max_det=64, gate=(0, 0))
    got, ref = run_and_check(engine, "cut", rd, q)
    n = ref["det"].sum(axis=(1, 2))
    assert n.min() >= 200                                                 # hundreds of detections
    assert got["det_count"].tolist() == n.tolist()                        # the full number, not 64
    assert got["mask"].sum(axis=(1, 2)).tolist() == n.tolist()            # the mask is complete
    for f in range(2):
        r, d = np.nonzero(ref["det"][f])
        np.testing.assert_array_equal(got["det_range_idx"][f], r[:64] + 1)
        np.testing.assert_array_equal(got["det_doppler_idx"][f], d[:64] + 1)
        np.testing.assert_array_equal(got["det_noise"][f], ref["noise"][f, r[:64], d[:64]])
        assert (got["det_noise"][f] > 0).all()
    q1 = cfg_for(256, 1e-3, "3/4", max_det=1, gate=(0, 0))
    one, _ = run_and_check(engine, "cut", rd, q1)
    assert one["det_count"].tolist() == n.tolist()
    for k in ("det_range_idx", "det_doppler_idx", "det_power", "det_noise"):
        np.testing.assert_array_equal(one[k], got[k][:, :1])
    # a frame with fewer detections than the list: det_noise is filled for exactly the listed entries
    few = noise_map((1, 64, 32), 32, targets=3)
    got, ref = run_and_check(engine, "few", few, cfg_for(64, 1e-4, "3/4", max_det=64, gate=(0, 0)))
    n = int(got["det_count"][0])
    assert 0 < n < 64 and (got["det_noise"][0, :n] > 0).all() and not got["det_noise"][0, n:].any()


# ---- 8. masking on the device ---------------------------------------------------------------------------
def _scene_configs(max_det=64):
    s = R.SCENE
    kw = dict(guard_r=s["guard"][0], guard_d=s["guard"][1], train_r=s["train"][0], train_d=s["train"][1], max_det=max_det)
    ca = P.CfarConfig(alpha=P.CfarConfig.alpha_for(72, s["pfa"]), **kw)
    os_ = P.OsCfarConfig(alpha=P.OsCfarConfig.alpha_for(72, s["rank"], s["pfa"]), rank=s["rank"], **kw)
    return ca, os_


@pytest.mark.parametrize("weak_db", [14, 20])
def test_masking_ca_misses_what_os_finds(engine, weak_db):
    """tests/test_oscfar_host.py's scenario on the device: the weak target next to a 40 dB one is missed
    by Engine.cfar in every frame and found by Engine.oscfar in every frame."""
    x = R.masking_scene(weak_db)
    ca, os_ = _scene_configs()
    r, d = R.scene_cells()["weak"]
    m_ca = engine.cfar(x, ca, want_mask=True)["mask"]
    got = engine.oscfar(x, os_, want_mask=True)
    assert m_ca[:, r, d].sum() == 0 and got["mask"][:, r, d].sum() == R.SCENE["F"]
    R.assert_bytes(got, R.oscfar_reference(x, R.SCENE["guard"], R.SCENE["train"], os_.alpha, os_.rank), 64, got["mask"])


def test_targets_dispatch_on_the_detector(engine):
    """Engine.targets with an OsCfarConfig forms three targets per frame where the CfarConfig gives
    two: the lists feed the clustering unchanged."""
    x = R.masking_scene(14)
    ca, os_ = _scene_configs()
    qc = P.ClusterConfig(link_r=1, link_d=1, min_cells=1, max_tgt=8)
    two = engine.targets(x, ca, qc)
    three = engine.targets(x, os_, qc)
    assert two["tgt_count"].tolist() == [2] * R.SCENE["F"] and three["tgt_count"].tolist() == [3] * R.SCENE["F"]
    cells = R.scene_cells()
    want = sorted((r + 1, d + 1) for r, d in cells["strong"] + [cells["weak"]])
    for f in range(R.SCENE["F"]):
        have = sorted(zip(three["peak_range_idx"][f, :3].tolist(), three["peak_doppler_idx"][f, :3].tolist()))
        assert have == want
    _same(three, engine.oscfar(x, os_), OUT_KEYS)


# ---- 9. determinism -----------------------------------------------------------------------------------
def _same(a, b, keys=OUT_KEYS + ("mask",)):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_frames_are_independent(engine):
    """The 12-frame call equals twelve one-frame calls, byte for byte (the strip height follows the
    frame count; the results do not)."""
    rd = rd_map((64, 16, 256, 16))
    q = cfg_for(256, 1e-3, "3/4", local_max=True)
    whole = engine.oscfar(rd, q, want_mask=True)
    assert whole["det_count"].sum() > 0
    for f in range(len(rd)):
        one = engine.oscfar(rd[f:f + 1], q, want_mask=True)
        _same(one, {k: whole[k][f:f + 1] for k in one})


def test_call_sequence_on_one_context():
    """Map A with config 1, then B with config 2 (fp16 storage, another window, cut list), then A with
    config 1 again, on one context: the first and the third result are identical, and equal a new
    context's."""
    from fmcw_radar_processing_amd.engine import Engine
    a, b = parity_map((1024, 256, 1024, 256)), halves(rd_map((256, 32, 256, 32)))
    q1 = cfg_for(1024, 1e-3, "3/4", max_det=512, local_max=True)
    q2 = cfg_for(256, 1e-3, "half", (1, 3), (6, 2), max_det=5)
    seq, fresh = Engine(0), Engine(0)
    try:
        first = seq.oscfar(a, q1, want_mask=True)
        other = seq.oscfar(b, q2, want_mask=True)
        third = seq.oscfar(a, q1, want_mask=True)
        want = fresh.oscfar(a, q1, want_mask=True)
    finally:
        seq.close()
        fresh.close()
    _same(first, third)
    _same(first, want)
    R.assert_bytes(first, decide(window((1024, 256, 1024, 256), a, (1, 1), (2, 2)), q1), q1.max_det, first["mask"])
    R.assert_bytes(other, decide(window("seq_b", b, (1, 3), (6, 2)), q2), q2.max_det, other["mask"])


def test_shards_are_bit_identical():
    from fmcw_radar_processing_amd.engine import Engine
    rd = rd_map((64, 16, 256, 16))
    q = cfg_for(256, 1e-3, "3/4", max_det=4)
    multi, single = Engine([0, 0, 0]), Engine(0)
    try:
        _same(multi.oscfar(rd, q, want_mask=True), single.oscfar(rd, q, want_mask=True))
    finally:
        multi.close()
        single.close()


def _device_buffers(F, nr, nd, K, fill=-3):
    import torch
    dev = "cuda"
    return dict(det_count=torch.full((F,), fill, dtype=torch.int32, device=dev),
                det_range_idx=torch.full((F, K), fill, dtype=torch.int32, device=dev),
                det_doppler_idx=torch.full((F, K), fill, dtype=torch.int32, device=dev),
                det_power=torch.full((F, K), float(fill), device=dev),
                det_noise=torch.full((F, K), float(fill), device=dev))


def test_chunk_seams_of_both_calls(engine, monkeypatch):
    """The host call cut into one-frame chunks (FMCW_HOST_CHUNK=1) and the device call cut into
    launch groups of 5, 5 and 2 frames (FMCW_CFAR_SCRATCH: room for five frames' lists) give the
    bytes of the uncut calls; timing stage oscfar counts the three launch groups."""
    import torch
    rd = rd_map((64, 16, 256, 16))
    F, nr, nd = rd.shape
    q = cfg_for(nr, 1e-3, "3/4", max_det=16, local_max=True)
    want = engine.oscfar(rd, q, want_mask=True)
    want_h = engine.oscfar(halves(rd), q, want_mask=True)
    assert want["det_count"].sum() > 0 and want_h["det_count"].sum() > 0
    monkeypatch.setenv("FMCW_HOST_CHUNK", "1")
    _same(engine.oscfar(rd, q, want_mask=True), want)
    _same(engine.oscfar(halves(rd), q, want_mask=True), want_h)
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
        engine.oscfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, d_mask=d_mask, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        t = engine.timing_read()
        assert t["oscfar"][1] == 3 and t["cfar"][1] == 0
    finally:
        engine.timing(0)
        engine.timing_reset()
    got = {k: v.cpu().numpy() for k, v in outs.items()} | {"mask": d_mask.cpu().numpy()}
    _same(got, want)


# ---- 10. arguments ----------------------------------------------------------------------------------------
_REJECTED = dict({k: (v[0], v[1], v[2], 1) for k, v in REJECTED.items()},
                 rank_0=(dict(), 256, 16, 0), rank_above_the_window=(dict(), 256, 16, 41))


@pytest.mark.parametrize("name", sorted(_REJECTED))
def test_device_call_rejects_what_the_check_rejects(engine, name):
    """E_ARG before any launch: the outputs keep what they held, timing stage oscfar counts nothing."""
    import torch
    over, nr, nd, rank = _REJECTED[name]
    q = P.OsCfarConfig(max_det=8, alpha=7.54, rank=rank)
    for k, v in over.items():
        setattr(q, k, v)
    K = 8
    d_rd = torch.zeros((1, nr, nd, 2), dtype=torch.float32, device="cuda")
    outs = _device_buffers(1, nr, nd, K)
    engine.timing_reset()
    engine.timing(1)
    try:
        with pytest.raises(FmcwError, match="E_ARG"):
            engine.oscfar_device(q, d_rd, FMCW_C64, 1, nr, nd, outs, stream=torch.cuda.current_stream())
        with pytest.raises(FmcwError, match="E_ARG"):
            engine.oscfar(np.zeros((1, nr, nd), np.complex64), q)
        torch.cuda.synchronize()
        assert engine.timing_read()["oscfar"][1] == 0
    finally:
        engine.timing(0)
    for v in outs.values():
        assert bool((v == -3).all())


def test_device_call_arguments_and_timing(engine):
    import torch
    geo = (64, 16, 256, 16)
    rd = rd_map(geo)
    F, nr, nd = rd.shape
    q = cfg_for(nr, 1e-3, "3/4", max_det=16)
    d_rd = torch.from_numpy(np.array(rd).view(np.float32).reshape(F, nr, nd, 2)).to("cuda")
    outs = _device_buffers(F, nr, nd, 16)
    s = torch.cuda.current_stream()
    # F = 0 is a no-op; a bad dtype, F < 0, a missing output and an unaligned map are argument errors
    engine.oscfar_device(q, d_rd, FMCW_C64, 0, nr, nd, outs, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.oscfar_device(q, d_rd, 2, F, nr, nd, outs, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.oscfar_device(q, d_rd, FMCW_C64, -1, nr, nd, outs, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.oscfar_device(q, d_rd, FMCW_C64, F, nr, nd, dict(outs, det_noise=None), stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.oscfar_device(q, d_rd.view(-1)[2:], FMCW_C64, F - 1, nr, nd, outs, stream=s)
    with pytest.raises(TypeError):
        engine.oscfar_device(P.CfarConfig(), d_rd, FMCW_C64, F, nr, nd, outs, stream=s)
    torch.cuda.synchronize()
    for v in outs.values():
        assert bool((v == -3).all())
    # timing stage `oscfar`: one event pair per launch group, nothing when timing is off
    engine.timing_reset()
    engine.oscfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, stream=s)
    torch.cuda.synchronize()
    assert engine.timing_read()["oscfar"] == (0.0, 0)
    engine.timing(1)
    try:
        engine.oscfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, stream=s)
        engine.oscfar_device(q, d_rd, FMCW_C64, 1, nr, nd, outs, stream=s)
        torch.cuda.synchronize()
        ms, n = engine.timing_read()["oscfar"]
        assert n == 2 and ms > 0
    finally:
        engine.timing(0)
        engine.timing_reset()
    # without a mask the lists are the same as with one (the host call, checked against the reference)
    engine.oscfar_device(q, d_rd, FMCW_C64, F, nr, nd, outs, stream=s)
    torch.cuda.synchronize()
    want, _ = run_and_check(engine, geo, rd, q)
    _same({k: v.cpu().numpy() for k, v in outs.items()}, want, OUT_KEYS)


def test_oscfar_result_carries_metres_and_speed():
    """With the geometry's taps set, Engine.oscfar adds range_m / speed_mps of the listed detections."""
    from fmcw_radar_processing_amd.engine import Engine
    geo = (64, 16, 256, 16)
    cfg, p, wr, wd, cal = case(*geo)
    eng = Engine(0)
    try:
        eng.set_taps(cfg, cal, wr, wd)
        got = eng.oscfar(rd_map(geo), cfg_for(256, 1e-3, "3/4", max_det=16))
    finally:
        eng.close()
    used = got["det_range_idx"] > 0
    assert used.any() and np.isnan(got["range_m"][~used]).all() and np.isnan(got["speed_mps"][~used]).all()
    np.testing.assert_array_equal(got["range_m"][used], cfg.range_m(got["det_range_idx"][used]))
    np.testing.assert_array_equal(got["speed_mps"][used], cfg.speed(got["det_doppler_idx"][used]))


# ---- 11. known answer, end to end -----------------------------------------------------------------------
@pytest.mark.parametrize("geo,guard,train,pipe", [((1024, 256, 1024, 256), (2, 2), (1, 1), FMCW_PIPE_AUTO),
                                                  ((256, 32, 256, 32), (4, 3), (4, 4), FMCW_PIPE_STREAMS)],
                         ids=["1024x256_auto", "256x32_streams"])
def test_known_answer_end_to_end(geo, guard, train, pipe):
    """IQ in, detections out on one stream (process_oscfar_device): frames 40-46 of the synthetic
    stream hold one target each, whose cell is the detection with the largest power / noise.  The
    whole output equals the reference applied, frame by frame, to the RD map the device wrote."""
    import torch
    from fmcw_radar_processing_amd.engine import Engine
    nts, pn, nr, nd = geo
    cfg, p, wr, wd, cal = case(nts, pn, nr, nd, P.THROUGHPUT)
    F, dev = 8, "cuda"
    iq = O.synth_frames(F, pn, nts, nr, nd, p["dist_per_bin"], frame0=40)
    q = P.OsCfarConfig.for_config(cfg, pfa=1e-6, guard=guard, train=train, max_det=64, local_max=True)
    assert q.rank == (3 * q.n_train_full) // 4
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
        eng.process_oscfar_device(d_iq, F, FMCW_C64, outs, q, d_rd, co, d_mask=d_mask,
                                  stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        eng.synchronize()
        got = {k: v.cpu().numpy() for k, v in co.items()}
        rd = d_rd.cpu().numpy().view(np.complex64)[..., 0]
        mask = d_mask.cpu().numpy()
    finally:
        eng.close()
    for i in range(F):                                   # one frame's stack of sorted training powers at a time
        ref = R.oscfar_reference(rd[i:i + 1], guard, train, q.alpha, q.rank, q.r_lo, q.r_hi, True)
        R.assert_bytes({k: got[k][i:i + 1] for k in got}, ref, K, mask[i:i + 1])
        fp = O.synth_frame_params(40 + i, nr, nd, p["dist_per_bin"])
        if fp["A"] == 0:
            assert i == 7
            continue
        n = min(int(got["det_count"][i]), K)
        assert n >= 1
        best = np.argmax(got["det_power"][i, :n] / got["det_noise"][i, :n])
        assert (got["det_range_idx"][i, best], got["det_doppler_idx"][i, best]) == (fp["r"] + 1, fp["d"] + nd // 2 + 1)
