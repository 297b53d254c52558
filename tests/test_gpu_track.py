"""GPU: the tracking stage (csrc/kernels_track.hip through fmcw_track / fmcw_track_device) against the
float32 reference of tests/track_reference.py, which runs on exactly the target bytes the device is
given.  Every output and the final state block are compared exactly, bit for bit, with no exempt
cases.  Except for the end-to-end test the targets are built in numpy."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C64, FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS, FmcwError, _lib
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import cluster_reference as CR
from tests import track_reference as R
from tests.helpers import case
from tests.test_track_host import DEFAULTS, REJECTED, frames_to_tgts, random_scene, slice_rows

pytestmark = pytest.mark.gpu

GUARD = 3                       # guard rows before and after every device output
ALL = R.OUT_KEYS + ("state",)


def run_and_check(engine, tgts, q, nr, nd, n_seq=1, state=None):
    got = engine.track(tgts, q, nr, nd, n_seq=n_seq, state=state)
    ref = R.reference_of(tgts, q, nr, nd, n_seq=n_seq, state=state)
    R.assert_same(got, ref)
    return got


def _same(a, b, keys=ALL):
    for k in keys:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def device_run(engine, tgts, q, nr, nd, n_seq=1, state=None, leave_out=(), tgt_track=True, S=None, F=None,
               max_tgt=None):
    """fmcw_track_device over buffers pre-filled with -3 / NaN, each between GUARD guard rows that
    must come back untouched, the state block between guard bytes as well; returns what the buffers
    hold afterwards (None for the outputs left out)."""
    import torch
    dev = "cuda"
    rows, M = tgts["range"].shape
    T = q.max_trk if hasattr(q, "abi") else min(max(q.max_trk, 1), 64)
    nS = n_seq if S is None else S
    nF = rows // n_seq if F is None else F
    sb = R.state_bytes(T)
    d_in = {k: torch.from_numpy(np.ascontiguousarray(tgts[k])).to(dev) for k in R.IN_KEYS}
    st = np.full((n_seq + 2, sb), 0xA5, np.uint8)
    st[1:-1] = 0 if state is None else np.asarray(state, np.uint8).reshape(n_seq, sb)
    d_state = torch.from_numpy(st).to(dev)

    def buf(cols, dtype, fill):
        shape = (rows + 2 * GUARD,) if cols is None else (rows + 2 * GUARD, cols)
        return torch.full(shape, fill, dtype=dtype, device=dev)
    full = dict(trk_count=buf(None, torch.int32, -3))
    for k in R.INT_KEYS:
        full[k] = buf(T, torch.int32, -3)
    for k in R.FLOAT_KEYS:
        full[k] = buf(T, torch.float32, np.nan)
    full["tgt_track"] = buf(M, torch.int32, -3)
    outs = {k: (None if k in leave_out else v[GUARD:GUARD + rows]) for k, v in full.items() if k != "tgt_track"}
    d_tt = full["tgt_track"][GUARD:GUARD + rows] if tgt_track else None
    torch.cuda.synchronize()
    try:
        engine.track_device(q, nS, nF, nr, nd, M if max_tgt is None else max_tgt, d_in, d_state[1:-1], outs,
                            d_tgt_track=d_tt, stream=torch.cuda.current_stream())
    finally:
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in full.items()}
        host["state"] = d_state.cpu().numpy()
        device_run.last = host
    for k, v in host.items():
        g = np.concatenate([v[:GUARD], v[-GUARD:]]) if k != "state" else np.concatenate([v[:1], v[-1:]])
        assert (g == 0xA5).all() if k == "state" else (np.isnan(g).all() if g.dtype == np.float32 else (g == -3).all()), k
    got = {k: (None if k in leave_out or (k == "tgt_track" and not tgt_track) else v[GUARD:GUARD + rows])
           for k, v in host.items() if k != "state"}
    got["state"] = host["state"][1:-1]
    return got


def untouched(raw, state_fill):
    """Every output row still holds the fill device_run gave it, and the state block its bytes."""
    for k, v in raw.items():
        if k == "state":
            assert (v[1:-1] == state_fill).all()
        else:
            assert np.isnan(v).all() if v.dtype == np.float32 else (v == -3).all(), k


# ---- 1. shapes -----------------------------------------------------------------------------------------
def dense_scene(seed, rows, nr, nd, M):
    """Rows whose count runs over -2 .. M + 2, with measurements drawn around a few anchors so that
    gates overlap and slots compete; some values are not finite or lie outside the map."""
    rng = np.random.default_rng(seed)
    anchors_r = rng.uniform(1, nr, 6)
    anchors_d = rng.uniform(0.5, nd + 0.5, 6)
    cnt = rng.integers(-2, M + 3, rows).astype(np.int32)
    cnt[rng.random(rows) < 0.3] = min(M, 2)
    pick = rng.integers(0, 6, (rows, M))
    zr = (anchors_r[pick] + rng.normal(0, 0.6, (rows, M))).astype(np.float32)
    zd = ((anchors_d[pick] + rng.normal(0, 0.4, (rows, M)) - 0.5) % nd + 0.5).astype(np.float32)
    zp = rng.uniform(1, 100, (rows, M)).astype(np.float32)
    odd = rng.random((rows, M))
    zr[odd < 0.02] = np.nan
    zd[(odd >= 0.02) & (odd < 0.03)] = np.inf
    zr[(odd >= 0.03) & (odd < 0.04)] = nr + 0.5
    zd[(odd >= 0.04) & (odd < 0.05)] = 0.25
    return dict(tgt_count=cnt, range=zr, doppler=zd, peak_power=zp)


@pytest.mark.parametrize("nr,nd", [(16, 4), (1024, 256)], ids=["16x4", "1024x256"])
@pytest.mark.parametrize("T,M", [(1, 1), (3, 5), (16, 16), (64, 64)], ids=lambda v: str(v))
def test_shapes(engine, T, M, nr, nd):
    q = P.TrackConfig(gate_r=1.5, gate_d=1.25, alpha_r=0.625, alpha_d=0.375, beta_r=0.3, confirm_hits=2, max_coast=1,
                      max_trk=T)
    for S, F in ((1, 1), (70, 2), (3, 37), (1, 37)):
        got = run_and_check(engine, dense_scene(1000 * T + M + S, S * F, nr, nd, M), q, nr, nd, n_seq=S)
        if F == 37:
            assert got["trk_count"].max() >= 1 and got["trk_id"].max() > T        # tracks confirm, slots are reused


# ---- 2. a scene ------------------------------------------------------------------------------------------
def test_random_scene(engine):
    """Two drifting targets with 10 % dropouts in Poisson clutter over 200 frames: exact parity, and
    the tracker does what it is for -- two long-lived confirmed tracks, clutter tracks short-lived."""
    nr, nd, M = 256, 32, 8
    tgts = random_scene(2026, 200, nr, nd, M, clutter=0.7, dropout=0.1)
    q = P.TrackConfig(gate_r=3.0, gate_d=3.0, alpha_r=0.5, alpha_d=0.5, beta_r=0.25, confirm_hits=3, max_coast=3, max_trk=8)
    got = run_and_check(engine, tgts, q, nr, nd)
    conf = got["trk_status"] == 2
    ids, n = np.unique(got["trk_id"][conf], return_counts=True)
    assert (n >= 150).sum() == 2                            # the two targets, each one id nearly throughout
    assert np.median(got["trk_count"][20:]) == 2


# ---- 3. hand-built cases ---------------------------------------------------------------------------------
def _cfg(**over):
    d = {k: v for k, v in DEFAULTS.items() if k != "flags"}
    d.update(gate_r=2.0, gate_d=2.0, confirm_hits=2, max_coast=2, max_trk=4)
    d.update(over)
    return P.TrackConfig(**d)


def test_equal_costs(engine):
    nr, nd = 64, 16
    # one slot, two measurements at the same cost: the lower j; the other one starts a track
    got = run_and_check(engine, frames_to_tgts([[(20.0, 8.0)], [(21.0, 8.0), (19.0, 8.0)]], 4), _cfg(), nr, nd)
    assert got["tgt_track"][1, :2].tolist() == [1, 2] and got["trk_range"][1, 0] == 21.0
    got = run_and_check(engine, frames_to_tgts([[(20.0, 8.0)], [(20.0, 9.0), (20.0, 7.0)]], 4), _cfg(), nr, nd)
    assert got["tgt_track"][1, :2].tolist() == [1, 2] and got["trk_doppler"][1, 0] == 9.0
    # two slots, one measurement at the same cost: the lower slot; the other slot misses
    got = run_and_check(engine, frames_to_tgts([[(20.0, 8.0), (23.0, 8.0)], [(21.5, 8.0)]], 4), _cfg(), nr, nd)
    assert got["tgt_track"][1, 0] == 1 and got["trk_id"][1].tolist() == [1, 0, 0, 0]
    # four slots in a chain, every measurement between two of them
    frames = [[(20.0, 8.0), (23.0, 8.0), (26.0, 8.0), (29.0, 8.0)], [(27.5, 8.0), (24.5, 8.0), (21.5, 8.0)]]
    got = run_and_check(engine, frames_to_tgts(frames, 4), _cfg(), nr, nd)
    assert got["tgt_track"][1, :3].tolist() == [3, 2, 1] and got["trk_id"][1].tolist() == [1, 2, 3, 0]


def test_cost_of_exactly_one_and_the_next_float(engine):
    """gate 2 x 2, so wr = wd = 0.25 exactly.  er = 2, x = 0: c = 1.0, admitted.  er = 2, x = 2^-11:
    1 + 2^-24, a tie that rounds to even, c = 1.0, admitted.  er = 2, x = 3 * 2^-12: 1 + 1.125 * 2^-23
    rounds to the float above 1.0, not admitted: the tentative track dies, its slot is reused by the
    measurement in the same frame."""
    f = np.float32
    nr, nd = 64, 16
    xs = [f(0), f(2.0 ** -11), f(3 * 2.0 ** -12)]
    cs = [f(f(f(2) * f(2)) * f(0.25)) + f(f(x * x) * f(0.25)) for x in xs]
    assert cs[0] == cs[1] == f(1) and cs[2] == np.nextafter(f(1), f(2))
    rows = []
    for x in xs:
        assert f(f(8) + x) - f(8) == x
        rows += [[(20.0, 8.0)], [(22.0, f(8) + x)]]
    got = run_and_check(engine, frames_to_tgts(rows, 2), _cfg(), nr, nd, n_seq=3)
    assert got["tgt_track"][1::2, 0].tolist() == [1, 1, 2]
    assert got["trk_id"][1::2, 0].tolist() == [1, 1, 2] and got["trk_age"][1::2, 0].tolist() == [2, 2, 1]


def test_confirmed_before_tentative(engine):
    nr, nd = 64, 16
    frames = [[(20.0, 8.0)], [(20.0, 8.0)], [(20.0, 8.0), (23.0, 8.0)], [(21.75, 8.0)]]
    got = run_and_check(engine, frames_to_tgts(frames, 2), _cfg(), nr, nd)
    assert got["trk_status"][2].tolist() == [2, 1, 0, 0]
    # the measurement is nearer the tentative track, the confirmed one takes it; the tentative one dies
    assert got["tgt_track"][3, 0] == 1 and got["trk_status"][3].tolist() == [2, 0, 0, 0]
    # both tentative: the nearer one
    got = run_and_check(engine, frames_to_tgts(frames[2:], 2), _cfg(), nr, nd)
    assert got["tgt_track"][1, 0] == 2


def test_doppler_across_the_seam(engine):
    nr, nd = 64, 16
    up = [15.25, 15.75, 16.25, 0.75, 1.25, 1.75]
    ds = up + up[::-1]
    got = run_and_check(engine, frames_to_tgts([[(30.0, d)] for d in ds], 2),
                        _cfg(alpha_d=0.75, confirm_hits=3), nr, nd)
    assert (got["trk_id"][:, 0] == 1).all() and (got["tgt_track"][:, 0] == 1).all()
    d = got["trk_doppler"][:, 0]
    assert ((d >= 0.5) & (d < nd + 0.5)).all() and d.min() < 2 and d.max() > 15
    # alpha_d 1 lands on the measurement; the far side of the ring is outside the gate
    got = run_and_check(engine, frames_to_tgts([[(30.0, 16.25)], [(30.0, 0.75)], [(30.0, 1.0)], [(30.0, 16.0)], [(30.0, 8.0)]], 2),
                        _cfg(alpha_d=1.0), nr, nd)
    assert got["trk_doppler"][:4, 0].tolist() == [16.25, 0.75, 1.0, 16.0] and got["tgt_track"][4, 0] == 2


def test_coasting_out_of_the_map(engine):
    nr, nd = 16, 4
    q = _cfg(gate_d=1.5, max_coast=9)
    out_top = frames_to_tgts([[(12.0, 2.0)], [(13.5, 2.0)], [(15.0, 2.0)], [], [], []], 1)
    got = run_and_check(engine, out_top, q, nr, nd)
    assert got["trk_range"][:, 0].tolist() == [12.0, 13.5, 15.0, 0.0, 0.0, 0.0]      # 16.5 is outside [0.5, 16.5)
    out_bottom = frames_to_tgts([[(2.5, 2.0)], [(1.75, 2.0)], [], [], []], 1)
    got = run_and_check(engine, out_bottom, q, nr, nd)
    assert got["trk_range"][:, 0].tolist() == [2.5, 1.75, 1.0, 0.0, 0.0] and got["trk_misses"][2, 0] == 1


def test_invalid_measurements_and_counts(engine):
    nr, nd, M = 64, 16, 6
    bad = [(np.nan, 8.0), (20.0, np.nan), (np.inf, 8.0), (20.0, -np.inf), (0.25, 8.0), (64.5, 8.0), (20.0, 0.25),
           (20.0, 16.5), (-3.0, 8.0), (20.0, 1e30)]
    frames = [[(20.0, 8.0)] + bad[:5], [bad[5], (20.5, 8.0)] + bad[6:], [bad[0], bad[1], (21.0, 8.0)]]
    got = run_and_check(engine, frames_to_tgts(frames, M), _cfg(), nr, nd)
    assert got["tgt_track"].tolist() == [[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0]]
    assert got["trk_id"].max() == 1
    # the edges of the map are valid
    got = run_and_check(engine, frames_to_tgts([[(0.5, 0.5), (np.nextafter(np.float32(64.5), 0), np.nextafter(np.float32(16.5), 0))]], M),
                        _cfg(), nr, nd)
    assert got["tgt_track"][0, :2].tolist() == [1, 2]
    # counts: negative and 0 are empty frames, above max_tgt is cut to max_tgt
    full = [(10.0 * (j + 1) - 5, 8.0) for j in range(M)]
    tg = frames_to_tgts([full] * 5, M, counts=[-7, 0, M + 9, 2, 2 ** 31 - 1])
    got = run_and_check(engine, tg, _cfg(max_trk=8), nr, nd)
    assert (got["tgt_track"] > 0).sum(axis=1).tolist() == [0, 0, M, 2, M]


def test_slot_exhaustion_and_reuse(engine):
    nr, nd = 256, 32
    six = [(20.0 * (j + 1), 4.0 * (j + 1)) for j in range(6)]
    got = run_and_check(engine, frames_to_tgts([six, six + [(200.0, 30.0)]], 8), _cfg(), nr, nd)
    assert got["tgt_track"].tolist() == [[1, 2, 3, 4, 0, 0, 0, 0]] * 2
    # slots 1 and 3 (0-based) miss while tentative: freed and taken again in the same frame, in slot order
    frames = [six[:4], [six[0], six[2], six[4], six[5], (200.0, 30.0)]]
    got = run_and_check(engine, frames_to_tgts(frames, 8), _cfg(), nr, nd)
    assert got["trk_id"][1].tolist() == [1, 5, 3, 6] and got["tgt_track"][1, :5].tolist() == [1, 3, 5, 6, 0]
    assert got["trk_age"][1].tolist() == [2, 1, 2, 1]


def test_confirm_hits_1_and_max_coast_0(engine):
    nr, nd = 64, 16
    frames = [[(20.0, 8.0)], [(20.5, 8.0)], [], [(21.5, 8.0)], []]
    got = run_and_check(engine, frames_to_tgts(frames, 1), _cfg(confirm_hits=1, max_coast=0), nr, nd)
    assert got["trk_status"][:, 0].tolist() == [2, 2, 0, 2, 0] and got["trk_id"][:, 0].tolist() == [1, 1, 0, 2, 0]
    got = run_and_check(engine, frames_to_tgts(frames, 1), _cfg(confirm_hits=1, max_coast=1), nr, nd)
    assert got["trk_id"][:, 0].tolist() == [1, 1, 1, 1, 1] and got["trk_misses"][:, 0].tolist() == [0, 0, 1, 0, 1]
    got = run_and_check(engine, frames_to_tgts(frames, 1), _cfg(confirm_hits=255, max_coast=0), nr, nd)
    assert got["trk_count"].tolist() == [0] * 5


# ---- 4. splits, sequences, shards --------------------------------------------------------------------------
SPLIT_Q = P.TrackConfig(gate_r=3.0, gate_d=3.0, max_trk=4, confirm_hits=2, max_coast=2)


def test_37_frames_equal_1_5_31_with_the_state_carried(engine):
    nr, nd, M = 64, 16, 5
    tgts = random_scene(11, 37, nr, nd, M, clutter=1.5)
    whole = run_and_check(engine, tgts, SPLIT_Q, nr, nd)
    state, f0, parts = None, 0, []
    for n in (1, 5, 31):
        part = engine.track(slice_rows(tgts, f0, f0 + n), SPLIT_Q, nr, nd, state=state)
        state, f0 = part["state"], f0 + n
        parts.append(part)
    joined = {k: np.concatenate([p[k] for p in parts]) for k in R.OUT_KEYS}
    joined["state"] = state
    _same(joined, whole)
    # the device call, the state carried in device memory
    dev = [device_run(engine, slice_rows(tgts, 0, 6), SPLIT_Q, nr, nd)]
    dev.append(device_run(engine, slice_rows(tgts, 6, 37), SPLIT_Q, nr, nd, state=dev[0]["state"]))
    _same({k: np.concatenate([p[k] for p in dev]) for k in R.OUT_KEYS}, whole, R.OUT_KEYS)
    assert dev[1]["state"].tobytes() == whole["state"].tobytes()


def _three_sequences(nr, nd, M, F):
    seqs = [random_scene(s, F, nr, nd, M, clutter=1.0) for s in (5, 6, 7)]
    return seqs, {k: np.concatenate([s[k] for s in seqs]) for k in R.IN_KEYS}


def test_a_sequence_does_not_depend_on_its_neighbours(engine):
    nr, nd, M, F = 64, 16, 5, 20
    seqs, tgts = _three_sequences(nr, nd, M, F)
    three = run_and_check(engine, tgts, SPLIT_Q, nr, nd, n_seq=3)
    alone = run_and_check(engine, seqs[1], SPLIT_Q, nr, nd)
    _same({k: three[k][F:2 * F] for k in R.OUT_KEYS}, alone, R.OUT_KEYS)
    assert three["state"][1].tobytes() == alone["state"][0].tobytes()
    again = engine.track(tgts, SPLIT_Q, nr, nd, n_seq=3)
    _same(again, three)                                     # bit-identical from call to call


def test_host_call_equals_device_call_and_null_members(engine):
    nr, nd, M, F = 64, 16, 5, 20
    _, tgts = _three_sequences(nr, nd, M, F)
    want = engine.track(tgts, SPLIT_Q, nr, nd, n_seq=3)
    _same(device_run(engine, tgts, SPLIT_Q, nr, nd, n_seq=3), want)
    # each optional output and tgt_track may be missing
    for k in R.INT_KEYS + R.FLOAT_KEYS:
        part = device_run(engine, tgts, SPLIT_Q, nr, nd, n_seq=3, leave_out=(k,))
        assert part[k] is None
        _same(part, want, [x for x in ALL if x != k])
    part = device_run(engine, tgts, SPLIT_Q, nr, nd, n_seq=3, leave_out=R.INT_KEYS + R.FLOAT_KEYS, tgt_track=False)
    _same(part, want, ["trk_count", "state"])


def test_fresh_state_equals_a_zeroed_one(engine):
    """state NULL on the host call: fresh sequences, the state is discarded; the outputs are those of
    an explicitly zeroed block.  NULL output members on the host call."""
    nr, nd, M, F = 64, 16, 5, 20
    _, tgts = _three_sequences(nr, nd, M, F)
    zero = np.zeros((3, R.state_bytes(SPLIT_Q.max_trk)), np.uint8)
    want = engine.track(tgts, SPLIT_Q, nr, nd, n_seq=3, state=zero)
    assert not zero.any()                                    # the caller's array is not written through
    _same(engine.track(tgts, SPLIT_Q, nr, nd, n_seq=3), want)
    cnt, ids = np.full(3 * F, -3, np.int32), np.full((3 * F, SPLIT_Q.max_trk), -3, np.int32)
    t = _lib.Tracks(trk_count=cnt.ctypes.data, trk_id=ids.ctypes.data)
    qa = SPLIT_Q.abi()
    args = [np.ascontiguousarray(tgts[k]) for k in R.IN_KEYS]
    st = engine.lib.fmcw_track(engine.h, ct.byref(qa), 3, F, nr, nd, M, *[a.ctypes.data for a in args], None, ct.byref(t), None)
    assert st == _lib.FMCW_OK
    _same(dict(trk_count=cnt, trk_id=ids), want, ["trk_count", "trk_id"])


def test_shards_and_chunks(engine, monkeypatch):
    """S = 5 over a 3-device context (sequences, never frames, are sharded), and the frames staged in
    chunks of 1, 7 and 36 with the state kept on the device."""
    from fmcw_radar_processing_amd.engine import Engine
    nr, nd, M, F = 64, 16, 5, 37
    tgts = {k: np.concatenate([random_scene(s, F, nr, nd, M, clutter=1.0)[k] for s in range(20, 25)]) for k in R.IN_KEYS}
    want = run_and_check(engine, tgts, SPLIT_Q, nr, nd, n_seq=5)
    multi = Engine([0, 0, 0])
    try:
        _same(multi.track(tgts, SPLIT_Q, nr, nd, n_seq=5), want)
        for chunk in ("1", "7", "36"):
            monkeypatch.setenv("FMCW_HOST_CHUNK", chunk)
            _same(engine.track(tgts, SPLIT_Q, nr, nd, n_seq=5), want)
        _same(multi.track(tgts, SPLIT_Q, nr, nd, n_seq=5), want)
        monkeypatch.delenv("FMCW_HOST_CHUNK")
    finally:
        multi.close()


# ---- 5. any state bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", [(3, 5), (64, 64)], ids=lambda v: str(v))
def test_arbitrary_state_ends_within_bounds(engine, T, M):
    """A seeded non-zero state block (any status, NaN and huge values, a counter near the wrap) and
    targets full of odd values: the call ends, the guard rows and guard bytes are intact (device_run),
    every output row is written, a free slot is all zero, and the result is the same on a second call."""
    nr, nd, S, F = 64, 16, 4, 9
    rng = np.random.default_rng(99)
    state = rng.integers(0, 256, (S, R.state_bytes(T)), dtype=np.uint8)
    state[1] = 0xff
    q = P.TrackConfig(gate_r=3.0, gate_d=3.0, max_trk=T, confirm_hits=2, max_coast=2)
    tgts = dense_scene(5, S * F, nr, nd, M)
    a = device_run(engine, tgts, q, nr, nd, n_seq=S, state=state)
    b = device_run(engine, tgts, q, nr, nd, n_seq=S, state=state)
    _same(a, b)
    free = a["trk_status"] == 0
    assert set(np.unique(a["trk_status"]).tolist()) <= {0, 1, 2}
    for k in R.INT_KEYS + R.FLOAT_KEYS:
        assert not a[k][free].any(), k                      # a NaN counts as non-zero
    assert ((a["trk_count"] >= 0) & (a["trk_count"] <= T)).all() and (a["tgt_track"] != -3).all()


# ---- 6. end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,guard,train,pipe", [((1024, 256, 1024, 256), (4, 4), (4, 4), FMCW_PIPE_AUTO),
                                                  ((256, 32, 256, 32), (4, 3), (4, 4), FMCW_PIPE_STREAMS)],
                         ids=["1024x256_auto", "256x32_streams"])
def test_iq_to_tracks_end_to_end(geo, guard, train, pipe):
    """IQ in, tracks out on one stream (process_tracks_device), frames 40-47 of the synthetic stream:
    the tracks equal the reference run on the cluster outputs the device itself wrote."""
    import torch
    from fmcw_radar_processing_amd.engine import Engine
    nts, pn, nr, nd = geo
    cfg, p, wr, wd, cal = case(nts, pn, nr, nd, P.THROUGHPUT)
    F, dev = 8, "cuda"
    iq = O.synth_frames(F, pn, nts, nr, nd, p["dist_per_bin"], frame0=40)
    qc = P.CfarConfig.for_config(cfg, pfa=1e-6, guard=guard, train=train, max_det=256)
    qt = P.ClusterConfig.for_config(cfg, link=(1, 1), min_cells=2, max_tgt=4, max_det=qc.max_det)
    qk = P.TrackConfig.for_config(cfg, gate=(float(nr), nd / 2 - 1.0), confirm_hits=2, max_coast=1, max_trk=3, max_tgt=qt.max_tgt)
    K, M, T, N = qc.max_det, cfg.max_targets, qt.max_tgt, qk.max_trk
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
        to = dict(tgt_count=torch.full((F,), -3, dtype=torch.int32, device=dev))
        for k in CR.INT_KEYS:
            to[k] = torch.full((F, T), -3, dtype=torch.int32, device=dev)
        for k in CR.FLOAT_KEYS:
            to[k] = torch.full((F, T), np.nan, dtype=torch.float32, device=dev)
        ko = dict(trk_count=torch.full((F,), -3, dtype=torch.int32, device=dev))
        for k in R.INT_KEYS:
            ko[k] = torch.full((F, N), -3, dtype=torch.int32, device=dev)
        for k in R.FLOAT_KEYS:
            ko[k] = torch.full((F, N), np.nan, dtype=torch.float32, device=dev)
        d_tt = torch.full((F, T), -3, dtype=torch.int32, device=dev)
        d_state = torch.zeros(eng.track_state_bytes(N), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        eng.process_tracks_device(d_iq, F, FMCW_C64, outs, qc, d_rd, co, qt, to, qk, d_state, ko, d_tgt_track=d_tt,
                                  stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        eng.synchronize()
        tg = {k: v.cpu().numpy() for k, v in to.items()}
        got = {k: v.cpu().numpy() for k, v in ko.items()}
        got["tgt_track"] = d_tt.cpu().numpy()
        got["state"] = d_state.cpu().numpy().reshape(1, -1)
    finally:
        eng.close()
    assert tg["tgt_count"][:7].min() >= 1 and tg["tgt_count"][7] == 0       # frame 47 has no target
    R.assert_same(got, R.reference_of(tg, qk, nr, nd))
    assert got["trk_id"].max() >= 1 and got["tgt_track"].max() >= 1


# ---- 7. arguments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REJECTED))
def test_device_call_rejects_what_the_check_rejects(engine, name):
    """E_ARG before any launch: the outputs and the state keep their fill, timing stage track counts nothing."""
    over, nr, nd, max_tgt, _ = REJECTED[name]
    d = dict(DEFAULTS, gate_r=2.0, gate_d=1.5, max_trk=4)
    d.update(over)
    q = _lib.TrackParams(*[d[k] for k, _ in _lib.TrackParams._fields_])      # the C struct: it can carry a flag bit
    tgts = frames_to_tgts([[(5.0, 2.0), (9.0, 3.0)]], 4)
    state = np.full((1, R.state_bytes(min(max(q.max_trk, 1), 64))), 0x5A, np.uint8)
    engine.timing_reset()
    engine.timing(1)
    try:
        with pytest.raises(FmcwError, match="E_ARG"):
            device_run(engine, tgts, q, nr, nd, state=state, max_tgt=max_tgt)
        untouched(device_run.last, 0x5A)
        assert engine.timing_read()["track"][1] == 0
    finally:
        engine.timing(0)


def test_device_call_arguments_and_timing(engine):
    import torch
    nr, nd = 64, 16
    tgts = frames_to_tgts([[(20.0 + f, 8.0), (40.0, 3.0)] for f in range(3)], 4)
    q = _cfg()
    want = engine.track(tgts, q, nr, nd)
    state = np.full((1, R.state_bytes(4)), 0x5A, np.uint8)
    # F = 0 and S = 0 are no-ops; negative sizes and a missing required pointer are argument errors
    for kw in (dict(F=0), dict(S=0)):
        device_run(engine, tgts, q, nr, nd, state=state, **kw)
        untouched(device_run.last, 0x5A)
    for kw in (dict(F=-1), dict(S=-1), dict(leave_out=("trk_count",))):
        with pytest.raises(FmcwError, match="E_ARG"):
            device_run(engine, tgts, q, nr, nd, state=state, **kw)
        untouched(device_run.last, 0x5A)
    # timing stage `track`: one event pair per launch, nothing when timing is off
    engine.timing_reset()
    _same(device_run(engine, tgts, q, nr, nd), want)
    assert engine.timing_read()["track"] == (0.0, 0)
    engine.timing(1)
    try:
        _same(device_run(engine, tgts, q, nr, nd), want)
        device_run(engine, tgts, q, nr, nd, F=1)
        engine.track(tgts, q, nr, nd)
        torch.cuda.synchronize()
        ms, n = engine.timing_read()["track"]
        assert n == 3 and ms > 0
    finally:
        engine.timing(0)
        engine.timing_reset()


def test_track_result_carries_metres_and_speed():
    """With the geometry's taps set, Engine.track adds range_m / speed_mps / range_rate_mps_per_frame
    of the slots (cfg.range_m, cfg.speed, dist_per_bin); NaN for free slots."""
    from fmcw_radar_processing_amd.engine import Engine
    geo = (64, 16, 256, 16)
    cfg, p, wr, wd, cal = case(*geo)
    tgts = frames_to_tgts([[(20.0 + 0.5 * f, 8.0)] for f in range(4)], 2)
    q = P.TrackConfig.for_config(cfg, max_trk=3, max_tgt=2)
    eng = Engine(0)
    try:
        plain = eng.track(tgts, q, 256, 16)
        assert "range_m" not in plain
        eng.set_taps(cfg, cal, wr, wd)
        got = eng.track(tgts, q, 256, 16)
    finally:
        eng.close()
    _same(got, plain)
    used = got["trk_status"] > 0
    assert used.any() and not used.all()
    for k in ("range_m", "speed_mps", "range_rate_mps_per_frame"):
        assert np.isnan(got[k][~used]).all() and not np.isnan(got[k][used]).any()
    np.testing.assert_array_equal(got["range_m"][used], cfg.range_m(got["trk_range"][used]))
    np.testing.assert_array_equal(got["speed_mps"][used], cfg.speed(got["trk_doppler"][used]))
    np.testing.assert_array_equal(got["range_rate_mps_per_frame"][used],
                                  got["trk_range_rate"][used].astype(np.float64) * cfg.dist_per_bin)
    assert got["range_rate_mps_per_frame"][3, 0] == 0.5 * cfg.dist_per_bin
