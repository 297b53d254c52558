"""GPU: the MUSIC stage (csrc/kernels_music.hip through fmcw_music_device and fmcw_music) against
tests/music_reference.py, byte for byte, on cov made by fmcw_cov_device and on a caller's own cov with
garbage in the diagonal's imaginary parts.  Device buffers sit between guards of NaN that must come
back untouched; inputs must come back unchanged."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import FmcwError, MusicConfig, RaConfig, _lib
from fmcw_radar_processing_amd.engine import Engine
from tests import music_reference as M
from tests import ra_reference as R
from tests.test_gpu_ra import GUARD, NAN32, At, cfg_of, cov_run, guarded, inner
from tests.test_music_host import MAX_SRC, REJECTED, SRC_THR, _q

pytestmark = pytest.mark.gpu

F32 = np.float32
OUTS = ("eval", "evec", "nsrc", "music")


def params(A, K, n_src=1, max_src=1, sweeps=8, fb=False, gate=(0, 0), thr=8.0):
    return _lib.MusicParams(A, K, gate[0], gate[1], n_src, max_src, sweeps, _lib.FMCW_MUSIC_FB if fb else 0, thr)


def ref_of(cov, w, q):
    return M.music_reference(cov, w, n_src=q.n_src, max_src=q.max_src, sweeps=q.sweeps, fb=bool(q.flags & 1),
                             src_thr=q.src_thr, r_lo=q.r_lo, r_hi=q.r_hi)


def music_run(engine, cov, w, q, want=OUTS, want_max=True, F=None, nr=None, shift=None, drop=None, rejects=False, stream=None,
              mx0=0.0):
    """fmcw_music_device over cov float32 [F][nr][T][2] and w float32 [K][A][2], all buffers between
    guards of NaN; cov and w must come back unchanged.  want: the outputs asked for (the others are
    passed as NULL and come back None).  shift: {name: bytes} moves a pointer off its alignment; drop:
    the pointer given as NULL; rejects: the call must fail with FMCW_E_ARG and every output must then
    hold what it held.  Returns dict(eval, evec, nsrc, music, music_max)."""
    import torch
    cov = np.ascontiguousarray(cov, F32)
    w = R.weights_f32(w)
    rows, mr = cov.shape[:2]
    A = w.shape[1]
    K = w.shape[0]
    cw = cov[0].size
    words = {"eval": mr * A, "evec": mr * A * A * 2, "nsrc": mr, "music": mr * K}
    d_cov = guarded(cov.view(np.uint32).reshape(rows, cw))
    d_w = guarded(w.view(np.uint32).reshape(1, -1))
    d_out = {k: guarded(np.full((rows, words[k]), NAN32, np.uint32)) for k in OUTS}
    d_mx = torch.full((4,), float(mx0), device="cuda")
    sh = dict(shift or {})
    ptr = {"cov": d_cov.data_ptr() + GUARD * cw * 4, "w": d_w.data_ptr() + GUARD * w.size * 4, "max": d_mx.data_ptr()}
    for k in OUTS:
        ptr[k] = d_out[k].data_ptr() + GUARD * words[k] * 4 if k in want else 0
    p = {k: (None if (drop == k or v == 0) else At(v + sh.get(k, 0))) for k, v in ptr.items()}
    if not want_max:
        p["max"] = None
    torch.cuda.synchronize()

    def call():
        engine.music_device(q, p["cov"], rows if F is None else F, mr if nr is None else nr, p["w"], p["eval"], p["evec"],
                            p["nsrc"], p["music"], p["max"], stream=torch.cuda.current_stream() if stream is None else stream)
    try:
        if rejects:
            with pytest.raises(FmcwError, match="E_ARG"):
                call()
        else:
            call()
    finally:
        torch.cuda.synchronize()
    assert inner(d_cov, cw).tobytes() == cov.tobytes() and inner(d_w, w.size).tobytes() == w.tobytes()
    mx = d_mx.cpu().numpy()
    assert (mx[1:] == F32(mx0)).all()
    res = {}
    untouched = rejects or (F is not None and F <= 0)
    for k in OUTS:
        o = inner(d_out[k], words[k])
        if untouched or k not in want or drop == k:
            assert (o == NAN32).all(), k                                      # never written
            res[k] = None
        else:
            res[k] = o
    if untouched or "music" not in want:
        assert mx[0] == F32(mx0)
    if res["eval"] is not None:
        res["eval"] = res["eval"].view(F32).reshape(rows, mr, A)
    if res["evec"] is not None:
        res["evec"] = res["evec"].view(F32).reshape(rows, mr, A, A, 2)
    if res["nsrc"] is not None:
        res["nsrc"] = res["nsrc"].view(np.int32).reshape(rows, mr)
    if res["music"] is not None:
        res["music"] = res["music"].view(F32).reshape(rows, mr, K)
    res["music_max"] = mx[0]
    return res


def table(A, K, seed):
    """A weight table float32 [K][A][2]: steering weights of random directions with a random taper."""
    rng = np.random.default_rng(seed)
    w = Engine.ra_weights(A, rng.uniform(-1, 1, K), 0.5, taper=rng.uniform(0.5, 1.5, A))
    return R.weights_f32(w)


def same(got, want, name=""):
    for k in OUTS:
        if got.get(k) is not None:
            R.assert_same_bytes(got[k], want[k], f"{name} {k}")


# ---- 1. parity ----------------------------------------------------------------------------------------------
# (A, n_ang, nr, F, sweeps, n_src, max_src, fb, gate index, caller's own cov)
CASES = [
    (2, 1, 16, 1, 8, 1, 1, False, 0, False),
    (2, 64, 64, 3, 1, 0, 1, True, 1, True),
    (2, 256, 16, 2, 16, 1, 1, True, 2, False),
    (3, 63, 64, 2, 8, 0, 2, False, 3, True),
    (3, 65, 16, 3, 16, 2, 1, True, 0, False),
    (3, 256, 64, 1, 1, 1, 1, False, 2, True),
    (5, 64, 16, 9, 8, 0, 4, True, 0, True),         # 144 rows: two whole workgroups and a partial one
    (5, 1, 64, 1, 16, 4, 1, False, 1, False),
    (5, 65, 16, 3, 1, 2, 1, True, 3, True),         # 48 rows: a partial workgroup
    (8, 65, 16, 1, 8, 2, 1, False, 0, False),       # 16 rows: a partial workgroup and a partial LDS batch
    (8, 63, 64, 3, 16, 0, 4, True, 2, True),
    (8, 256, 16, 3, 8, 7, 1, True, 1, False),       # 48 rows: a whole LDS batch of 32 and a partial one
    (8, 64, 16, 9, 1, 0, 7, False, 3, True),
    (4, 65, 64, 2, 8, 0, 3, True, 0, True),
    (6, 63, 16, 3, 8, 3, 1, False, 0, False),
    (7, 64, 16, 9, 8, 0, 3, True, 2, True),
]


def case_id(c):
    A, K, nr, F, sw, n, mx, fb, g, own = c
    return f"A{A}-K{K}-{nr}x{F}-sw{sw}-n{n}_{mx}-{'fb' if fb else 'plain'}-g{g}-{'own' if own else 'dev'}"


def case_inputs(engine, c):
    A, K, nr, F, sw, n, mx, fb, g, own = c
    gate = ((0, 0), (nr // 2, nr // 2), (1, 3), (nr - 4, nr))[g]
    seed = A * 1000 + K * 7 + nr + F
    if own:
        cov = M.random_cov(seed, A, F, nr, garbage=True, zero_rows=((0, 1), (F - 1, nr - 1), (F // 2, nr // 2)))
    else:
        cov = cov_run(engine, R.pool(seed, A, F, nr, 16, False), cfg_of(A, 8, (0, 0), 0))
    return cov, table(A, K, seed), params(A, K, n, mx, sw, fb, gate, 3.0)


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_bytes_equal_the_reference(engine, c):
    """Every output byte for byte, all outputs asked for together and each one alone (the bytes of an
    output do not depend on which others were asked for), with and without the running maximum."""
    cov, w, q = case_inputs(engine, c)
    want = ref_of(cov, w, q)
    got = music_run(engine, cov, w, q)
    same(got, want, "together")
    assert got["music_max"].tobytes() == want["music_max"].tobytes()
    if q.n_src == 0:
        assert len(np.unique(want["nsrc"])) > 1                              # the estimate is exercised
    for k in OUTS:
        alone = music_run(engine, cov, w, q, want=(k,), want_max=(k == "music"))
        assert all(alone[o] is None for o in OUTS if o != k)
        same(alone, want, "alone")
    same(music_run(engine, cov, w, q, want=("eval", "nsrc"), drop="w"), want, "without w")
    same(music_run(engine, cov, w, q, want=("music",), want_max=False), want, "without the maximum")


def test_running_maximum_is_only_raised(engine):
    A, K = 3, 9
    cov = M.random_cov(1, A, 1, 16)
    w, q = table(A, K, 1), params(A, K)
    want = ref_of(cov, w, q)
    assert music_run(engine, cov, w, q, mx0=3e38)["music_max"] == F32(3e38)
    assert music_run(engine, cov, w, q, mx0=0.0)["music_max"] == want["music_max"] == want["music"].max()


# ---- 2. frames, calls, chunks, shards, contexts ---------------------------------------------------------------
def test_frames_calls_chunks_and_shards(engine, monkeypatch):
    """12 frames in one device call equal twelve one-frame calls and a repeated call; the host call at
    the default chunk, in one-frame chunks and over three shards equals them too."""
    import torch
    A, K, nr, F = 5, 33, 16, 12
    cov = M.random_cov(77, A, F, nr, zero_rows=((3, 3),))
    w = table(A, K, 5)
    cfg = MusicConfig(A, K, n_src=0, max_src=3, sweeps=8, fb=True, src_thr=3.0)
    q = cfg.abi()
    want = ref_of(cov, w, q)
    got = music_run(engine, cov, w, q)
    same(got, want, "one call")
    for f in range(F):
        one = music_run(engine, cov[f:f + 1], w, q)
        for k in OUTS:
            R.assert_same_bytes(one[k], want[k][f:f + 1], f"frame {f} alone {k}")
    same(music_run(engine, cov, w, q), want, "the call repeated")
    multi = Engine([0, 0, 0])
    engines = [engine, multi]
    if torch.cuda.device_count() >= 2:
        engines.append(Engine([0, 1]))
    wc = w.view(np.complex64)[..., 0]
    try:
        for chunk in (None, "1"):
            if chunk:
                monkeypatch.setenv("FMCW_HOST_CHUNK", chunk)
            for e in engines:
                h = e.music_host(cov, cfg, wc)
                same(h, want, f"host chunk {chunk}")
                assert F32(h["music_max"]) == want["music_max"]
        monkeypatch.delenv("FMCW_HOST_CHUNK")
        part = multi.music_host(cov, cfg, want=("nsrc", "eval"))
        assert part["music"] is None and part["evec"] is None and part["music_max"] == 0.0
        same(part, want, "host, two outputs")
    finally:
        for e in engines[1:]:
            e.close()
    empty = engine.music_host(cov[:0], cfg, wc)
    assert empty["music"].shape == (0, nr, K) and empty["music_max"] == 0.0


def test_one_long_lived_context_equals_fresh_contexts(engine):
    seq = [(3, 16, 2, 17, False), (8, 64, 3, 65, True), (2, 16, 1, 256, True), (8, 16, 2, 33, False), (3, 16, 2, 17, True)]
    for A, nr, F, K, fb in seq:
        cov = M.random_cov(A * 31 + nr, A, F, nr)
        w = table(A, K, A).view(np.complex64)[..., 0]
        cfg = MusicConfig(A, K, n_src=0, max_src=A - 1, fb=fb, src_thr=3.0)
        a = engine.music_host(cov, cfg, w)
        fresh = Engine(0)
        try:
            b = fresh.music_host(cov, cfg, w)
        finally:
            fresh.close()
        same(a, b)
        assert a["music_max"] == b["music_max"]


# ---- 3. the scenarios on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_close_pair_on_the_device(engine, half):
    """Engine.music (cov_device, then music_device) on the close pair: the bytes of the reference on
    the device's own cov, MUSIC peaks exactly {32, 35} in 8 of 8 frames, the estimated count 2 in the
    source row and 0 in every noise row."""
    S = M.CLOSE
    chans = M.close_scene(M.CLOSE_SEED, half)
    w = Engine.ra_weights(S["A"], R.scene_sines(), S["spacing"])
    ra_q = RaConfig(S["A"], S["n_ang"], dc_half=S["dc_half"])
    cfg = MusicConfig(S["A"], S["n_ang"], n_src=2)
    out = engine.music(chans, cfg, ra_q, w)
    R.assert_same_bytes(out["cov"], engine.range_angle(chans, ra_q, want_ra=False)[1])
    want = ref_of(out["cov"], R.weights_f32(w), cfg.abi())
    same(out, want, "Engine.music")
    assert F32(out["music_max"]) == want["music_max"]
    pm = [R.peaks(out["music"][f, S["row"]]) for f in range(S["frames"])]
    assert all(p == list(S["points"]) for p in pm), pm
    est = engine.music(chans, MusicConfig(S["A"], S["n_ang"], n_src=0, max_src=MAX_SRC, src_thr=SRC_THR), ra_q, w)
    assert (est["nsrc"][:, S["row"]] == 2).all() and (np.delete(est["nsrc"], S["row"], axis=1) == 0).all()
    pm = [R.peaks(est["music"][f, S["row"]]) for f in range(S["frames"])]
    assert all(p == list(S["points"]) for p in pm), pm


@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_coherent_pair_on_the_device(engine, half):
    S = M.COHERENT
    chans = M.coherent_scene(M.COHERENT_SEED, half)
    w = Engine.ra_weights(S["A"], R.scene_sines(), S["spacing"])
    ra_q = RaConfig(S["A"], S["n_ang"], dc_half=S["dc_half"])
    peaks = {}
    for fb in (False, True):
        cfg = MusicConfig(S["A"], S["n_ang"], n_src=2, fb=fb)
        out = engine.music(chans, cfg, ra_q, w)
        same(out, ref_of(out["cov"], R.weights_f32(w), cfg.abi()), f"fb {fb}")
        peaks[fb] = [R.peaks(out["music"][f, S["row"]]) for f in range(S["frames"])]
    assert not any(p == list(S["points"]) for p in peaks[False]), peaks[False]
    assert all(p == list(S["points"]) for p in peaks[True]), peaks[True]


# ---- 4. arguments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REJECTED))
def test_device_calls_reject_what_the_check_rejects(engine, name):
    """E_ARG before any launch: every buffer keeps what it held (music_run checks it), stage music
    counts nothing."""
    over, nr, _ = REJECTED[name]
    q = _q(**dict(over))
    A = max(min(q.n_chan, 8), 2)
    K = max(min(q.n_ang, 256), 1)
    cov = np.ones((2, 64, R.n_tri(A), 2), F32)
    w = np.ones((K, A, 2), F32)
    engine.timing_reset()
    engine.timing(1)
    try:
        music_run(engine, cov, w, q, nr=nr, rejects=True)
        out = np.full((2, 64, 256), np.nan, F32)
        assert engine.lib.fmcw_music(engine.h, ct.byref(q), cov.ctypes.data, 2, nr, w.ctypes.data, None, None, None,
                                     out.ctypes.data, None) == _lib.FMCW_E_ARG
        assert np.isnan(out).all()
        assert engine.timing_read()["music"][1] == 0
    finally:
        engine.timing(0)


def test_call_arguments(engine):
    A, K, nr, F = 3, 9, 64, 3
    cov = M.random_cov(4, A, F, nr)
    w, q = table(A, K, 2), params(A, K)
    # F = 0 is a no-op, whatever the other pointers
    music_run(engine, cov, w, q, F=0)
    music_run(engine, cov, w, q, F=0, drop="cov")
    for kw in (dict(F=-1), dict(drop="cov"), dict(drop="w"), dict(want=()), dict(shift={"cov": 8}), dict(shift={"w": 8}),
               dict(shift={"eval": 4}), dict(shift={"evec": 8}), dict(shift={"nsrc": 4}), dict(shift={"music": 4}),
               dict(shift={"max": 2})):
        music_run(engine, cov, w, q, rejects=True, **kw)
    # w is not needed without music
    same(music_run(engine, cov, w, q, want=("evec",), drop="w"), ref_of(cov, w, q))
    lib, h = engine.lib, engine.h
    o = np.full((F, nr, K), np.nan, F32)
    mx = ct.c_float(-1.0)
    cp, wp, op = cov.ctypes.data, w.ctypes.data, o.ctypes.data
    assert lib.fmcw_music(h, ct.byref(q), cp, F, nr, wp, None, None, None, None, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert b"every output is NULL" in lib.fmcw_last_error()
    assert lib.fmcw_music(h, ct.byref(q), None, F, nr, wp, None, None, None, op, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert lib.fmcw_music(h, ct.byref(q), cp, F, nr, None, None, None, None, op, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert lib.fmcw_music(h, ct.byref(q), cp, -1, nr, wp, None, None, None, op, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert np.isnan(o).all() and mx.value == -1.0
    assert lib.fmcw_music(h, ct.byref(q), None, 0, nr, None, None, None, None, op, ct.byref(mx)) == _lib.FMCW_OK      # F = 0
    assert mx.value == 0.0 and np.isnan(o).all()
    with pytest.raises(ValueError):
        engine.music_host(cov, MusicConfig(A, K))                             # the spectrum needs w
    with pytest.raises(ValueError):
        engine.music_host(cov, MusicConfig(A + 1, K), w.view(np.complex64)[..., 0])


def test_stream_and_timing(engine, monkeypatch):
    """A non-default torch stream; timing stage 18 (`music`): one event pair per k_music launch, none
    with timing off, none for a rejected call."""
    import torch
    A, K, nr, F = 4, 65, 16, 3
    cov = M.random_cov(9, A, F, nr)
    w, q = table(A, K, 4), params(A, K, 0, 2)
    engine.timing_reset()
    got = music_run(engine, cov, w, q)
    assert engine.timing_read()["music"] == (0.0, 0)
    s = torch.cuda.Stream()
    engine.timing(1)
    try:
        with torch.cuda.stream(s):
            side = music_run(engine, cov, w, q, stream=s)
        s.synchronize()
        ms, n = engine.timing_read()["music"]
        assert n == 1 and ms > 0
        cfg = MusicConfig(A, K, n_src=0, max_src=2)
        engine.music_host(cov, cfg, w.view(np.complex64)[..., 0])             # one chunk: one launch
        assert engine.timing_read()["music"][1] == 2
        monkeypatch.setenv("FMCW_HOST_CHUNK", "1")
        engine.music_host(cov, cfg, w.view(np.complex64)[..., 0])             # three one-frame chunks
        monkeypatch.delenv("FMCW_HOST_CHUNK")
        assert engine.timing_read()["music"][1] == 5
        music_run(engine, cov, w, q, F=-1, rejects=True)
        music_run(engine, cov, w, q, F=0)
        assert engine.timing_read()["music"][1] == 5
        assert engine.timing_read()["ra"][1] == 0
        lib = engine.lib
        msd, nn = ct.c_double(), ct.c_int64()
        assert lib.fmcw_timing_read(engine.h, 18, ct.byref(msd), ct.byref(nn)) == _lib.FMCW_OK and nn.value == 5
        assert lib.fmcw_timing_read(engine.h, 19, ct.byref(msd), ct.byref(nn)) == _lib.FMCW_E_ARG
    finally:
        engine.timing(0)
        engine.timing_reset()
    same(side, got)
    assert side["music_max"] == got["music_max"]
