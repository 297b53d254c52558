"""GPU: the Doppler-time / range-time signature stage (csrc/kernels_sig.hip through fmcw_sig /
fmcw_sig_device / fmcw_sig_db_device) against the float64 reference of tests/sig_reference.py, which
always runs on exactly the bytes the device is given: every output within (N + 8) 2^-24 relative of
the reference (N cells summed), exact zeros where the reference is 0, the maxima equal to the
maximum of the returned map; bit-identical across calls, frame counts, shards and chunks."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64, FmcwError, _lib
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import sig_reference as R
from tests.helpers import case
from tests.test_gpu_cfar import GEOS, halves, rd_map
from tests.test_sig_host import REJECTED

pytestmark = pytest.mark.gpu

# (nr, nd): the smallest shapes on either side of "a row fills one wave-load" for both dtypes
# (128 complex64 or 256 fp16-storage cells), the shortest rows (one lane's 16 bytes hold a whole fp16
# row at nd = 4), the most rows, and the longest row (two loads per thread in complex64)
CORNERS = [(16, 4), (2048, 4), (16, 1024), (64, 64), (32, 128), (32, 256)]
_MAPS = {}


def random_map(nr, nd, F=3, seed=0):
    key = (nr, nd, F, seed)
    if key not in _MAPS:
        rng = np.random.default_rng(1000 * nr + nd + seed)
        x = (rng.standard_normal((F, nr, nd)) + 1j * rng.standard_normal((F, nr, nd))).astype(np.complex64)
        x *= np.float32(3.0) ** rng.integers(-3, 4, (F, nr, 1)).astype(np.float32)    # rows of unlike power
        x.setflags(write=False)
        _MAPS[key] = x
    return _MAPS[key]


def dominant_map():
    """(256, 32), unit-variance noise, one cell of power 1e12 in frame 1: a row or column sum formed as
    (full sum) - (left-out band) would be off by 2^-24 * 1e12 around it."""
    if "dominant" not in _MAPS:
        rng = np.random.default_rng(77)
        x = ((rng.standard_normal((2, 256, 32)) + 1j * rng.standard_normal((2, 256, 32))) / np.sqrt(2)).astype(np.complex64)
        x[1, 100, 16] = 1e6                          # zero Doppler (bin nd/2): inside every dc band
        x.setflags(write=False)
        _MAPS["dominant"] = x
    return _MAPS["dominant"]


INPUTS = {"geo_" + "x".join(map(str, g)): (lambda g=g: rd_map(g)) for g in sorted(GEOS)}
INPUTS.update({f"corner_{nr}x{nd}": (lambda nr=nr, nd=nd: random_map(nr, nd)) for nr, nd in CORNERS})
INPUTS["dominant_256x32"] = dominant_map


def stored(x, storage):
    return x if storage == "c64" else halves(x)


def to_device(rd):
    import torch
    rd = np.array(rd)                                # a writable copy: the cached maps are read-only
    if rd.dtype == np.complex64:
        return torch.from_numpy(rd.view(np.float32).reshape(*rd.shape, 2)).to("cuda"), FMCW_C64
    return torch.from_numpy(rd).to("cuda"), FMCW_C32H


def device_call(eng, rd, q, center=None, stride=1, maps=("doppler_time", "range_time"), fill=np.nan):
    """fmcw_sig_device on a host map: uploads it, runs on the current torch stream, returns numpy."""
    import torch
    d_rd, dt = to_device(rd)
    F, nr, nd = rd.shape[:3]
    bufs = dict(doppler_time=torch.full((F, nd), fill, device="cuda") if "doppler_time" in maps else None,
                range_time=torch.full((F, nr), fill, device="cuda") if "range_time" in maps else None)
    mx = torch.zeros(2, device="cuda")
    d_c = None if center is None else torch.from_numpy(np.ascontiguousarray(center, np.int32)).to("cuda")
    eng.signature_device(q, d_rd, dt, F, nr, nd, bufs["doppler_time"], bufs["range_time"], mx[0:1], mx[1:2],
                         d_center=d_c, center_stride=stride, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}
    out["dt_max"], out["rt_max"] = mx.cpu().numpy()
    return out


def reference(rd, q, center=None, stride=1):
    return R.sig_reference(rd, q.r_lo, q.r_hi, q.dc_half, center, stride, q.track_half)


def _same(a, b, keys=("doppler_time", "range_time", "dt_max", "rt_max")):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


# ---- 1. parity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["c64", "fp16"])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_parity(engine, name, storage):
    """Every geometry and corner shape and the dominant-cell map, both maps: the gates 0/0, 3..nr-2,
    one row and the last row only, each with dc_half -1, 0 and 2 (1 at nd = 4, where 2 dc_half + 1 < nd
    rules 2 out); then each map alone with the other pointer NULL."""
    rd = stored(INPUTS[name](), storage)
    F, nr, nd = rd.shape[:3]
    for gate in ((0, 0), (3, nr - 2), (7, 7), (nr, nr)):
        for dc in (-1, 0, 2 if nd > 4 else 1):
            q = P.SigConfig(r_lo=gate[0], r_hi=gate[1], dc_half=dc)
            got = engine.signature(rd, q)
            R.assert_matches(got, reference(rd, q))
            assert got["dt_max"] > 0 and got["rt_max"] > 0
    q = P.SigConfig(r_lo=3, r_hi=nr - 2, dc_half=0)
    both = engine.signature(rd, q)
    for only in ("doppler_time", "range_time"):
        got = device_call(engine, rd, q, maps=(only,))
        R.assert_matches(got, reference(rd, q), maps=(only,))
        assert got[only].tobytes() == both[only].tobytes()
        other = "rt_max" if only == "doppler_time" else "dt_max"
        assert got[other] == 0                         # nothing was written to the missing map


# ---- 2. tracked gate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["c64", "fp16"])
@pytest.mark.parametrize("track_half", [0, 2, 64])
@pytest.mark.parametrize("stride", [1, 3])
def test_tracked_gate_at_nr_16(engine, storage, track_half, stride):
    """Centres 0 (no target), 1, nr, one whose window the gate clips, and nr + 5 / -1 (behave as 0), from
    an array with stride 1 or 3 whose unused slots hold garbage; track_half 64 is wider than the map."""
    nr, nd = 16, 64
    rd = stored(random_map(nr, nd, F=7), storage)
    centres = [0, 1, nr, 4, nr + 5, -1, 9]
    ctr = np.full((7, stride), 1 << 30, np.int32)
    ctr[:, 0] = centres
    for gate in ((0, 0), (3, 12)):
        q = P.SigConfig(r_lo=gate[0], r_hi=gate[1], track_half=track_half, dc_half=1)
        ref = reference(rd, q, ctr, stride)
        got = device_call(engine, rd, q, ctr, stride)
        R.assert_matches(got, ref)
        _same(got, engine.signature(rd, q, ctr))
        for f in (0, 4, 5):                            # no target, and the two invalid centres
            assert not got["doppler_time"][f].any() and not got["range_time"][f].any()
        # a tracked frame equals the fixed-gate call over the same rows within the bound
        for f, c in enumerate(centres):
            ra, rb = R.frame_rows(nr, gate[0], gate[1], c, track_half)
            assert ref["n_dt"][f] == rb - ra
            if ra == rb:
                continue
            fixed = engine.signature(rd[f:f + 1], P.SigConfig(r_lo=ra + 1, r_hi=rb, dc_half=1))
            for k, n in (("doppler_time", rb - ra), ("range_time", ref["n_rt"])):
                err = np.abs(fixed[k][0].astype(np.float64) - got[k][f])
                assert np.all(err <= 2 * (n + 8) * R.U * ref[k][f]), k


@pytest.mark.parametrize("storage", ["c64", "fp16"])
def test_tracked_gate_over_several_slabs(engine, storage):
    """nd = 1024 with track_half 64: the 129 rows of a window are split over several workgroups, fewer
    where the map's edge or the gate clips it."""
    nr, nd = 256, 1024
    rd = stored(random_map(nr, nd, F=4), storage)
    ctr = np.array([[128, -7], [3, -7], [0, -7], [250, -7]], np.int32)
    for gate in ((0, 0), (100, 200)):
        q = P.SigConfig(r_lo=gate[0], r_hi=gate[1], track_half=64, dc_half=2)
        got = device_call(engine, rd, q, ctr, 2)
        R.assert_matches(got, reference(rd, q, ctr, 2))
        assert not got["doppler_time"][2].any() and got["doppler_time"][0].all()


# ---- 3. end to end on one stream -----------------------------------------------------------------------
@pytest.mark.parametrize("geo,F,out_dtype", [((64, 16, 256, 16), 12, FMCW_C64), ((1024, 256, 1024, 256), 2, FMCW_C64),
                                             ((64, 16, 256, 16), 12, FMCW_C32H)],
                         ids=["256x16", "1024x256", "256x16_fp16"])
def test_end_to_end_on_one_stream(geo, F, out_dtype):
    """IQ in, signatures out (process_signature_device): the outputs are within the bound of the
    reference applied to the RD map the call wrote, with the centres the call wrote.  With
    track_half 0 the Doppler-time row of a frame is |D|^2 of its target's range row, so its arg-max is
    the frame's tgt_doppler_idx wherever the peak rule did not fall back."""
    import torch
    from fmcw_radar_processing_amd.engine import Engine
    nts, pn, nr, nd = geo
    mode = P.THROUGHPUT if nr == 1024 else P.PARITY
    cfg, p, wr, wd, cal = case(nts, pn, nr, nd, mode)
    dev, M = "cuda", cfg.max_targets
    iq = O.synth_frames(F, pn, nts, nr, nd, p["dist_per_bin"])
    eng = Engine(0)
    try:
        eng.set_taps(cfg, cal, wr, wd)
        d_iq = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32).reshape(F, pn, nts, 2)).to(dev)
        outs = dict(profile=torch.empty((F, nr), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                    tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                    tgt_range_mag=torch.empty((F, M), device=dev),
                    tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                    slow_mag=torch.empty((F, pn), device=dev))
        rd_t = torch.float32 if out_dtype == FMCW_C64 else torch.float16
        seen = 0
        for th in (2, 0):
            q = P.SigConfig.for_config(cfg, track_half=th, dc_half=0)
            d_rd = torch.full((F, nr, nd, 2), np.nan, dtype=rd_t, device=dev)
            so = dict(doppler_time=torch.full((F, nd), np.nan, device=dev),
                      range_time=torch.full((F, nr), np.nan, device=dev),
                      dt_max=torch.zeros(1, device=dev), rt_max=torch.zeros(1, device=dev))
            torch.cuda.synchronize()
            eng.process_signature_device(d_iq, F, FMCW_C64, outs, q, d_rd, so, out_dtype=out_dtype,
                                         stream=torch.cuda.current_stream())
            torch.cuda.synchronize()
            eng.synchronize()
            got = {k: v.cpu().numpy() for k, v in so.items()}
            got["dt_max"], got["rt_max"] = got["dt_max"][0], got["rt_max"][0]
            rd = d_rd.cpu().numpy()
            rd = rd.view(np.complex64)[..., 0] if out_dtype == FMCW_C64 else rd
            ridx, didx, cnt = (outs[k].cpu().numpy() for k in ("tgt_range_idx", "tgt_doppler_idx", "tgt_count"))
            R.assert_matches(got, reference(rd, q, ridx, M))
            if th == 0:
                for f in range(F):
                    if cnt[f] > 0 and didx[f, 0] != cfg.doppler_fallback_idx:
                        assert int(np.argmax(got["doppler_time"][f])) + 1 == didx[f, 0], f
                        seen += 1
                    elif cnt[f] == 0:
                        assert ridx[f, 0] == 0 and not got["doppler_time"][f].any() and not got["range_time"][f].any()
        assert seen > 0
    finally:
        eng.close()


# ---- 4. determinism --------------------------------------------------------------------------------------
def test_frames_are_independent_and_calls_repeat(engine):
    """12 frames in one call equal twelve one-frame calls bit for bit, fixed and tracked; so do the two
    frames of the 1024 x 256 map, whose rows are split over several workgroups; two calls in a row are
    bit-identical; the maxima are the maxima of the one-frame calls."""
    for rd, q, ctr in ((rd_map((64, 16, 256, 16)), P.SigConfig(3, 254, 0, 0), None),
                       (halves(rd_map((64, 16, 256, 16))), P.SigConfig(0, 0, 64, 1), np.arange(12, dtype=np.int32) * 23),
                       (rd_map((1024, 256, 1024, 256)), P.SigConfig(0, 0, 0, 2), None),
                       (halves(rd_map((1024, 256, 1024, 256))), P.SigConfig(2, 1000, 0, -1), None)):
        whole = engine.signature(rd, q, ctr)
        _same(whole, engine.signature(rd, q, ctr))
        mx = np.zeros(2, np.float32)
        for f in range(len(rd)):
            one = engine.signature(rd[f:f + 1], q, None if ctr is None else ctr[f:f + 1])
            _same(one, {k: whole[k][f:f + 1] for k in ("doppler_time", "range_time")}, ("doppler_time", "range_time"))
            mx = np.maximum(mx, [one["dt_max"], one["rt_max"]])
        assert (whole["dt_max"], whole["rt_max"]) == (mx[0], mx[1])


def test_shards_and_chunks_are_bit_identical(engine, monkeypatch):
    """Three shards of one device and one-frame chunks (FMCW_HOST_CHUNK=1) equal the unsharded host
    call bit for bit, linear and in dB, maxima included."""
    from fmcw_radar_processing_amd.engine import Engine
    rd = rd_map((64, 16, 256, 16))
    ctr = (np.arange(12, dtype=np.int32) * 29) % 257
    multi = Engine([0, 0, 0])
    try:
        for q, c in ((P.SigConfig(3, 254, 0, 0), None), (P.SigConfig(0, 0, 2, 1), ctr),
                     (P.SigConfig(3, 254, 0, 0, db=True, floor_db=-70.0), None)):
            want = engine.signature(rd, q, c)
            _same(multi.signature(rd, q, c), want)
            monkeypatch.setenv("FMCW_HOST_CHUNK", "1")
            _same(engine.signature(rd, q, c), want)
            _same(multi.signature(rd, q, c), want)
            monkeypatch.delenv("FMCW_HOST_CHUNK")
    finally:
        multi.close()


# ---- 5. dB -------------------------------------------------------------------------------------------------
def test_db_device_and_host(engine):
    import torch
    rd = rd_map((256, 32, 256, 32))
    F, nr, nd = rd.shape
    q = P.SigConfig(3, nr - 2, 0, 1)
    lin = engine.signature(rd, q)
    assert (lin["range_time"] == 0).any()                 # the rows outside the gate
    for floor in (-80.0, -20.0):
        tol = R.db_tolerance(floor)
        for k, m in (("doppler_time", "dt_max"), ("range_time", "rt_max")):
            d_map = torch.from_numpy(lin[k]).to("cuda")
            d_mx = torch.tensor([float(lin[m])], device="cuda")
            d_out = torch.full_like(d_map, np.nan)
            s = torch.cuda.current_stream()
            engine.signature_db_device(d_map, d_map.numel(), d_mx, floor, d_out, stream=s)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            want = R.db_reference(lin[k], lin[m], floor)
            assert np.abs(out - want).max() <= tol
            assert np.all(out[lin[k] == 0] == np.float32(floor)) and out.max() == 0 and out.min() >= np.float32(floor)
            engine.signature_db_device(d_map, d_map.numel(), d_mx, floor, d_map, stream=s)      # in place
            torch.cuda.synchronize()
            assert d_map.cpu().numpy().tobytes() == out.tobytes()
            # an all-zero map, and a zero maximum
            z = torch.zeros(100, device="cuda")
            engine.signature_db_device(z, 100, d_mx, floor, z, stream=s)
            d_map2 = torch.from_numpy(lin[k]).to("cuda")
            engine.signature_db_device(d_map2, d_map2.numel(), torch.zeros(1, device="cuda"), floor, d_map2, stream=s)
            torch.cuda.synchronize()
            assert bool((z == floor).all()) and bool((d_map2 == floor).all())
        # the host call with FMCW_SIG_DB: the linear call followed by the reference dB on the global maximum
        db = engine.signature(rd, P.SigConfig(3, nr - 2, 0, 1, db=True, floor_db=floor))
        assert (db["dt_max"], db["rt_max"]) == (lin["dt_max"], lin["rt_max"])
        ref = reference(rd, q)
        for k, m, n in (("doppler_time", "dt_max", ref["n_dt"].max()), ("range_time", "rt_max", ref["n_rt"])):
            want = R.db_reference(lin[k], lin[m], floor)
            assert np.abs(db[k] - want).max() <= tol + (10 / np.log(10)) * (n + 8) * R.U
            assert np.all(db[k][lin[k] == 0] == np.float32(floor))


# ---- 6. arguments through the context -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REJECTED))
def test_device_call_rejects_what_the_check_rejects(engine, name):
    import torch
    over, nr, nd = REJECTED[name]
    q = P.SigConfig()
    flags = over.get("flags", 0)
    for k, v in over.items():
        if k != "flags":
            setattr(q, k, v)
    qa = q.abi()
    qa.flags = flags
    d_rd = torch.zeros((1, nr, nd, 2), dtype=torch.float32, device="cuda")
    dt, rt = torch.full((1, nd), -3.0, device="cuda"), torch.full((1, nr), -3.0, device="cuda")

    class _Q:                                            # hands the raw struct (an unknown flag bit) through
        def abi(self):
            return qa
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.signature_device(_Q(), d_rd, FMCW_C64, 1, nr, nd, dt, rt, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert bool((dt == -3).all()) and bool((rt == -3).all())


def test_device_call_arguments(engine):
    import torch
    rd = random_map(64, 64)
    F, nr, nd = rd.shape
    d_rd, _ = to_device(rd)
    q = P.SigConfig()
    dt, rt = torch.full((F, nd), -3.0, device="cuda"), torch.full((F, nr), -3.0, device="cuda")
    mx = torch.full((2,), -3.0, device="cuda")
    ctr = torch.ones(F, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    with pytest.raises(FmcwError, match="E_ARG"):         # both maps NULL
        engine.signature_device(q, d_rd, FMCW_C64, F, nr, nd, None, None, mx[0:1], mx[1:2], stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):         # misaligned map
        engine.signature_device(q, d_rd.view(-1)[2:], FMCW_C64, F - 1, nr, nd, dt, rt, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):         # bad dtype
        engine.signature_device(q, d_rd, 2, F, nr, nd, dt, rt, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):         # center_stride 0 with a centre array
        engine.signature_device(q, d_rd, FMCW_C64, F, nr, nd, dt, rt, d_center=ctr, center_stride=0, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.signature_device(q, d_rd, FMCW_C64, -1, nr, nd, dt, rt, stream=s)
    with pytest.raises(FmcwError, match="E_ARG"):
        engine.signature_db_device(dt, dt.numel(), mx[0:1], 0.0, dt, stream=s)
    engine.signature_device(q, d_rd, FMCW_C64, 0, nr, nd, dt, rt, mx[0:1], mx[1:2], stream=s)    # F = 0: a no-op
    torch.cuda.synchronize()
    assert bool((dt == -3).all()) and bool((rt == -3).all()) and bool((mx == -3).all())
    # the host call rejects the same: both maps NULL, a bad dtype
    qa = q.abi()
    h_dt = np.zeros((F, nd), np.float32)
    for dtype, maps in ((FMCW_C64, (None, None)), (2, (h_dt.ctypes.data, None))):
        with pytest.raises(FmcwError, match="E_ARG"):
            _lib.check(engine.lib.fmcw_sig(engine.h, ct.byref(qa), rd.ctypes.data, dtype, F, nr, nd, None, 1, *maps,
                                           None, None))


def test_signature_carries_the_axes():
    """With the geometry's taps set, Engine.signature adds speed_mps [nd] and range_m [nr]."""
    from fmcw_radar_processing_amd.engine import Engine
    geo = (64, 16, 256, 16)
    cfg, p, wr, wd, cal = case(*geo)
    eng = Engine(0)
    try:
        assert "speed_mps" not in eng.signature(rd_map(geo), P.SigConfig())
        eng.set_taps(cfg, cal, wr, wd)
        got = eng.signature(rd_map(geo), P.SigConfig())
    finally:
        eng.close()
    np.testing.assert_array_equal(got["speed_mps"], cfg.array_bin_fd)
    np.testing.assert_array_equal(got["range_m"], cfg.array_bin_range)
    assert got["speed_mps"][16 // 2] == 0                  # zero Doppler sits at bin nd/2


# ---- 7. a call sequence on one context --------------------------------------------------------------------
def test_call_sequence_on_one_context():
    """Geometry, dtype, gate and tracked / fixed interleaved on one context, with a CFAR call in between:
    every result has the bits a fresh context gives for that call alone."""
    from fmcw_radar_processing_amd.engine import Engine
    a, b, c = rd_map((1024, 256, 1024, 256)), halves(rd_map((256, 32, 256, 32))), random_map(16, 1024)
    ctr_a, ctr_b = np.array([[700, 5], [0, 5]], np.int32), np.arange(6, dtype=np.int32) * 50
    calls = [(a, P.SigConfig(0, 0, 0, 2), None), (b, P.SigConfig(3, 200, 2, 0), ctr_b), (c, P.SigConfig(16, 16, 0, -1), None),
             (a, P.SigConfig(10, 900, 64, 1), ctr_a), (b, P.SigConfig(0, 0, 0, -1, db=True, floor_db=-50.0), None),
             (a, P.SigConfig(0, 0, 0, 2), None)]
    cq = P.CfarConfig(max_det=16, alpha=P.CfarConfig.alpha_for(40, 1e-3), r_lo=3, r_hi=254)
    seq = Engine(0)
    try:
        got = []
        for i, (rd, q, ctr) in enumerate(calls):
            got.append(seq.signature(rd, q, ctr))
            if i == 2:
                seq.cfar(rd_map((256, 32, 256, 32)), cq)
    finally:
        seq.close()
    for (rd, q, ctr), g in zip(calls, got):
        fresh = Engine(0)
        try:
            _same(g, fresh.signature(rd, q, ctr))
        finally:
            fresh.close()
        if not q.db:
            R.assert_matches(g, reference(rd, q, ctr, 1 if ctr is None or ctr.ndim == 1 else ctr.shape[1]))
    _same(got[0], got[5])
