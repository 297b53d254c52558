"""GPU: one long-lived context gives what a brand-new context gives, over call sequences.

The other GPU tests make one call (or the same call twice) per geometry and compare it with the
float64 oracle.  A context also keeps state from one call to the next: k_rdx's two counter sets
and which of them comes next, the per-stream STFT table cache keyed on (window pointer, nfft), the
XT_* table's "built for these taps" flag, the hand-off slot ring (whose lines differ in format
between c64 and c32h launches), the detection's arrival counters per stream, the sticky error
word.  Here every op of a sequence runs on `seq`, one Engine kept for the whole module, and is
compared with the same op in a new Engine:

  (a) seq.synchronize() reports no error;
  (b) every output is bit-identical to the new context's (k_rdx, the detection and the STFT
      kernels are deterministic: test_xcd_deterministic_and_chunked, test_deterministic);
  (c) the new context's result meets the existing bars against the float64 oracle
      (test_gpu_onepass._check_vs_oracle / _check_fp16_vs_oracle, helpers.TOL_FP32_DB).

Every op of a sequence has its own first frame, so a slot, table or counter left by the op before
it changes the bits.  The host-side half of the counter-set rule is tests/test_xcd_ctr_plan.py.
"""
from dataclasses import dataclass, replace

import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64, FMCW_PIPE_STREAMS, FMCW_PIPE_XCD
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests.helpers import TOL_FP32_DB, case
from tests.test_gpu_onepass import _check_fp16_vs_oracle, _check_vs_oracle

pytestmark = pytest.mark.gpu

FRAME_BASE = 5000          # first frame of the synthetic stream (SURVEY 8d generator) the ops draw from
OUT_KEYS = ("profile", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "slow_mag")


def _geometries():
    """name -> (cfg, oracle params, range window, Doppler window, calibration).  A: config-3/4
    geometry with the SURVEY 8d taps; B: the same geometry as P.config(3) with other taps; C: 1000
    samples per chirp (zero-padded to Nr 1024: the masked k_rdx instantiations) with a third set."""
    cfg, p, wr, wd, cal = case(1024, 256, 1024, 256, P.THROUGHPUT)
    geo = {"A": (cfg, p, wr, wd, cal)}
    geo["B"] = (P.config(3), p, wr * 0.98, wd * 1.03, cal * (1.02 * np.exp(0.01j)))
    cfg, p, wr, wd, cal = case(1000, 256, 1024, 256, P.THROUGHPUT)
    geo["C"] = (cfg, p, wr * 1.01, wd * 0.97, cal * (0.99 * np.exp(-0.02j)))
    geo["C0"] = (cfg, p, wr, wd, cal)
    return geo


@dataclass(frozen=True)
class Op:
    F: int
    off: int                   # first frame = FRAME_BASE + off
    geo: str = "A"
    pipe: int = FMCW_PIPE_XCD
    chunk: int = 0
    api: str = "host"          # host: Engine.process; device: process_device; slow: process_slow_device
    h: bool = False            # fp16 storage: c32h IQ in, c32h RD out
    rd: bool = True
    stream: int = 0            # device / slow: index into the module's torch streams

    def launches(self, cfg):
        """k_rdx launches of the call on the single-pass schedule: one per chunk of the device call;
        the host call makes one device call per 64 MiB of input (api_internal.h host_chunk)."""
        if self.pipe == FMCW_PIPE_STREAMS:
            return 0
        per = lambda n: 1 if self.chunk <= 0 else -(-n // self.chunk)
        if self.api != "host":
            return per(self.F)
        fc = max(1, min((64 << 20) // (cfg.pn * cfg.nts * 8), self.F))
        return sum(per(min(fc, self.F - f0)) for f0 in range(0, self.F, fc))


SOURCE = {"A": "A", "B": "A", "C": "C", "C0": "C0"}     # the geometry whose frame window an op's input is cut from


class Frames:
    """Windows of consecutive synthetic frames (the library's own generator) per geometry
    and storage, each passed through the oracle once and sliced per op: the frames are independent
    of each other in every stage the ops run."""

    def __init__(self):
        self.geo = _geometries()
        self.win = {}          # (geo, h) -> (first offset, complex64 [n][C][S], oracle dict over the window)

    def reserve(self, geo, h, lo, hi):
        """Frames FRAME_BASE + lo .. FRAME_BASE + hi - 1 of a geometry, and the oracle on them."""
        import torch
        from fmcw_radar_processing_amd.engine import Engine
        if (geo, h) in self.win:
            assert self.win[(geo, h)][0] == lo and len(self.win[(geo, h)][1]) == hi - lo
            return
        cfg, p, wr, wd, cal = self.geo[geo]
        if (geo, False) in self.win and self.win[(geo, False)][0] <= lo and \
                hi <= self.win[(geo, False)][0] + len(self.win[(geo, False)][1]):
            l0, x0, _ = self.win[(geo, False)]
            x = x0[lo - l0: hi - l0]
        else:
            d = torch.empty((hi - lo, cfg.pn, cfg.nts, 2), dtype=torch.float32, device="cuda")
            e = Engine(0)
            try:
                e.set_taps(cfg, cal, wr, wd)
                e.synth_device(d, FRAME_BASE + lo, hi - lo, FMCW_C64, stream=torch.cuda.current_stream())
                torch.cuda.synchronize()
            finally:
                e.close()
            x = d.cpu().numpy().view(np.complex64)[..., 0]
        if h:                  # the oracle sees the fp16-rounded samples the device is given
            x = np.stack([x.real, x.imag], -1).astype(np.float16).astype(np.float32).view(np.complex64)[..., 0]
        x = np.ascontiguousarray(x)
        self.win[(geo, h)] = (lo, x, O.process_frames(x, cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True))

    def input(self, op):
        lo, x, _ = self.win[(SOURCE[op.geo], op.h)]
        assert lo <= op.off and op.off + op.F <= lo + len(x), "reserve() the op's frames first"
        return x[op.off - lo: op.off - lo + op.F]

    def oracle(self, op):
        if SOURCE[op.geo] != op.geo:       # the window's frames under another geometry's taps: this op's only
            cfg, p, wr, wd, cal = self.geo[op.geo]
            return O.process_frames(self.input(op), cal, p, wr, wd, want_cube=True, want_rd=True, rd_all_rows=True)
        lo, _, r = self.win[(op.geo, op.h)]
        return {k: v[op.off - lo: op.off - lo + op.F] for k, v in r.items()}

    def release(self, *keys):
        for k in keys:
            self.win.pop(k, None)


def _run(eng, op, frames, streams, fused=True):
    """Apply the op's taps, pipeline and chunk setting to eng, run it, synchronise: host arrays."""
    import torch
    cfg, p, wr, wd, cal = frames.geo[op.geo]
    eng.set_taps(cfg, cal, wr, wd)
    eng.set_pipeline(op.pipe)
    eng.set_chunk_frames(op.chunk)
    iq = frames.input(op)
    F, C, M = op.F, cfg.pn, cfg.max_targets
    if op.api == "host":
        assert not op.h
        got = eng.process(iq, want_rd=op.rd)
        eng.synchronize()
        return got
    dev, s = "cuda", streams[op.stream]
    dt = FMCW_C32H if op.h else FMCW_C64
    host = np.ascontiguousarray(iq).view(np.float32).reshape(F, C, cfg.nts, 2)
    d_iq = torch.from_numpy(host.astype(np.float16) if op.h else host).to(dev)
    outs = dict(profile=torch.full((F, cfg.nr), np.nan, device=dev),
                tgt_count=torch.full((F,), -3, dtype=torch.int32, device=dev),
                tgt_range_idx=torch.full((F, M), -3, dtype=torch.int32, device=dev),
                tgt_range_mag=torch.full((F, M), np.nan, device=dev),
                tgt_doppler_idx=torch.full((F, M), -3, dtype=torch.int32, device=dev),
                slow_mag=torch.full((F, C), np.nan, device=dev))
    d_rd = torch.full((F, cfg.nr, cfg.nd, 2), np.nan, dtype=torch.float16 if op.h else torch.float32,
                      device=dev) if op.rd else None
    torch.cuda.synchronize()                   # the inputs are in place before the op's stream starts
    extra = {}
    if op.api == "slow":
        flist = torch.full((F,), -7, dtype=torch.int32, device=dev)
        d_len = torch.full((1,), -1, dtype=torch.int64, device=dev)
        pmax = torch.full((1,), 123.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if fused:
            eng.process_slow_device(d_iq, F, dt, outs, flist, d_len, d_pmax=pmax, d_rd=d_rd, out_dtype=dt, stream=s)
        else:                                  # what the fused call must equal (test_gpu_slow_leg._both)
            eng.process_device(d_iq, F, dt, outs, d_rd=d_rd, out_dtype=dt, stream=s)
            eng.compact_device(outs["tgt_count"], F, flist, d_len, stream=s)
        torch.cuda.synchronize()
        n = int((outs["tgt_count"] > 0).sum().item())
        extra = dict(frame_list=flist.cpu().numpy()[:n], L=np.int64(d_len.item()), pmax=np.float32(pmax.item()))
    else:
        eng.process_device(d_iq, F, dt, outs, d_rd=d_rd, out_dtype=dt, stream=s)
        torch.cuda.synchronize()
    eng.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    if op.rd:
        got["rd_raw"] = d_rd.cpu().numpy()     # the stored bits (c64 pairs, or c32h holding D / (Nr Nd))
    got.update(extra)
    return got


def _rd_complex(got, cfg, h):
    if "rd" in got:
        return got["rd"]
    if h:                                      # include/fmcw.h, FMCW_C32H: the output holds D / (Nr * Nd)
        return got["rd_raw"].astype(np.float32).view(np.complex64)[..., 0].astype(np.complex128) * (cfg.nr * cfg.nd)
    return got["rd_raw"].view(np.complex64)[..., 0]


class Ctx:
    def __init__(self, frames):
        import torch
        from fmcw_radar_processing_amd.engine import Engine
        self.Engine = Engine
        self.frames = frames
        self.streams = [torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()]
        self.seq = Engine(0)
        self.launches = 0          # k_rdx launches on seq so far: every one moves to the other counter set
        self.kept = {}             # op -> its new-context result, for the ops a test asks to keep

    def fresh(self, op, fused=True):
        e = self.Engine(0)
        try:
            return _run(e, op, self.frames, self.streams, fused)
        finally:
            e.close()

    def reference(self, op, keep=False):
        """The op in a new context (the slow leg: process + compact there), checked against the oracle."""
        if op in self.kept:
            return self.kept[op]
        cfg, p, wr, wd, cal = self.frames.geo[op.geo]
        want = self.fresh(op, fused=False)
        full = want if op.rd else self.fresh(replace(op, rd=True), fused=False)
        if not op.rd:              # without the RD map only the row peaks are kept: nothing else may change
            for k in OUT_KEYS:
                np.testing.assert_array_equal(want[k], full[k], err_msg=k)
        ref = self.frames.oracle(op)
        got = {k: full[k] for k in OUT_KEYS} | {"rd": _rd_complex(full, cfg, op.h)}
        if op.h:
            _check_fp16_vs_oracle(cfg, got, ref, wd)
        else:
            _check_vs_oracle(cfg, got, ref, wd)
        if op.api == "slow":
            assert int(want["L"]) == cfg.pn * len(want["frame_list"])
            np.testing.assert_array_equal(want["frame_list"], np.nonzero(want["tgt_count"] > 0)[0])
        if keep:
            self.kept[op] = want
        return want

    def step(self, op):
        """One op on the long-lived context against its new-context reference, bit for bit."""
        want = self.reference(op)
        got = _run(self.seq, op, self.frames, self.streams)      # (a): synchronize() inside raises on an error
        self.launches += op.launches(self.frames.geo[op.geo][0])
        assert set(got) == set(want)
        for k in want:
            if k == "pmax":            # the fused call zeroes the running max(P); process + compact leave it
                assert got[k] == 0.0 and want[k] == 123.0
            else:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{op}: {k}")
        return got


@pytest.fixture(scope="module")
def ctx():
    c = Ctx(Frames())
    yield c
    c.seq.close()


# ---- FMCW_XCD_MEMSET switched inside one context ------------------------------------------------
KNOBS = [0, 0, 1, 0, 1, 1, 0, 0, 1, 0]
SHAPES = [(75, 0), (39, 13), (3, 0), (40, 13), (21, 0)]      # (F, chunk): 1, 3, 1, 4, 1 launches


def test_xcd_memset_knob_switched_between_launches(ctx, monkeypatch):
    """FMCW_XCD_MEMSET is read per launch.  A memset launch counts in the set the context would
    count in anyway and moves on to the other one like any launch (xcd_ctr_plan.h), so the knob may
    change between calls.  Ten device calls with the knob 0 0 1 0 1 1 0 0 1 0 over F 75 (every slot of
    the ring reused), 39 and 40 in chunks of 13 (three and four launches: the next set ends on either
    parity), 3 (fewer frames than XCDs) and 21 (a partial group).

    Both counter sets must see the knob go 0 -> 1 and 1 -> 0 at a launch that counts in them.  The
    set of a launch is the parity of the context's k_rdx launches before it, counted here.  The ten
    calls above meet three of the four combinations whichever parity they start on (1 3 1 4 1
    launches per call), so up to three single-launch calls per missing combination follow them: the
    knob brought to the value the switch starts from, the parity to the set, then the switch."""
    ctx.frames.reserve("A", False, 0, 92)
    cfg = ctx.frames.geo["A"][0]
    every = {(0, 0, 1), (0, 1, 0), (1, 0, 1), (1, 1, 0)}       # (set, knob before, knob of the launch)
    met = set()
    prev = None
    calls = [(k, SHAPES[i % len(SHAPES)]) for i, k in enumerate(KNOBS)]
    i = 0
    while i < len(calls):
        knob, (F, chunk) = calls[i]
        if prev is not None and prev != knob:
            met.add((ctx.launches % 2, prev, knob))
        monkeypatch.setenv("FMCW_XCD_MEMSET", str(knob))
        op = Op(F=F, off=i, chunk=chunk, api="device")
        before = ctx.launches
        ctx.step(op)
        assert ctx.launches - before == (1 if chunk == 0 else -(-F // chunk)) == op.launches(cfg)
        prev = knob
        i += 1
        if i == len(KNOBS):                    # plan the calls for what the ten left unmet
            parity, last = ctx.launches % 2, prev
            for q, a, b in sorted(every - met):
                for knob_, need in ((a, last != a), (a, (parity + (last != a)) % 2 != q), (b, True)):
                    if need:
                        calls.append((knob_, (21, 0) if len(calls) % 2 else (3, 0)))
                        parity ^= 1
                last = b
    assert len(calls) <= len(KNOBS) + 6
    assert met == every, (met, calls)


# ---- c64 / c32h launches and launches with / without the RD map, alternating ---------------------
def test_xcd_storage_and_output_alternation(ctx):
    """All eight k_rdx instantiations (1024 / 1000 samples per chirp x c64 / c32h x RD map written or
    not) on one context through the device API.  F falls from op to op and the storage alternates,
    so every launch finds, in every slot line it uses, what a launch of the other format left there:
    every c32h launch follows a c64 launch of larger F and every c64 launch a c32h one."""
    fr = ctx.frames
    fr.reserve("A", False, 0, 92)
    fr.reserve("A", True, 40, 72)
    fr.reserve("C0", False, 50, 80)
    fr.reserve("C0", True, 50, 80)
    ops = []
    F = 27
    for geo, lo in (("A", 40), ("C0", 50), ("A", 47)):
        for rd in (True, False):
            for h in (False, True):
                ops.append(Op(F=F, off=lo + len(ops) % 5, geo=geo, api="device", h=h, rd=rd))
                F -= 1
    assert len({(o.geo, o.h, o.rd) for o in ops}) == 8
    for a, b in zip(ops, ops[1:]):
        assert a.h != b.h and a.F > b.F
    for op in ops:
        assert op.F >= 16                      # both of the ring's slots in use on every XCD
        ctx.step(op)
    fr.release(("A", True), ("C0", False), ("C0", True))


# ---- set_taps: A -> other taps on the streams schedule -> 1000 samples per chirp -> A again --------
def test_set_taps_round_trip(ctx):
    """calw, the twiddles, cal_sum and the XT_* table follow every set_taps: geometry A, the same
    geometry as P.config(3) with another calibration and other windows on the streams schedule, 1000
    samples per chirp with a third set, and A again.  Every call equals its new-context result; the
    second A is the first A's op, so it equals the first A's new-context result bit for bit."""
    fr = ctx.frames
    fr.reserve("A", False, 0, 92)
    fr.reserve("C", False, 60, 70)
    a = Op(F=9, off=3)
    first = ctx.reference(a, keep=True)
    ctx.step(a)
    ctx.step(Op(F=7, off=14, geo="B", pipe=FMCW_PIPE_STREAMS))
    ctx.step(Op(F=9, off=61, geo="C"))
    again = ctx.step(a)
    assert ctx.reference(a) is first
    for k in first:
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)
    fr.release(("C", False))
    ctx.kept.clear()


# ---- the fused slow-time leg between other calls, on two streams -------------------------------
def test_slow_leg_between_other_calls(ctx):
    """process_slow_device (61 frames in chunks of 9) on one stream, process_device (24) on another,
    process_slow_device (8 in chunks of 3) on the first again, and once more on the second: the
    detection's arrival counters are per stream and are reset by each call's last workgroup.  Each
    fused result is process_device + compact_device in a new context (test_gpu_slow_leg._both)."""
    ctx.frames.reserve("A", False, 0, 92)
    got = ctx.step(Op(F=61, off=20, chunk=9, api="slow", stream=1))
    assert 0 < len(got["frame_list"]) < 61     # frames with and without a target
    ctx.step(Op(F=24, off=5, api="device", stream=2))
    ctx.step(Op(F=8, off=33, chunk=3, api="slow", stream=1))
    ctx.step(Op(F=13, off=51, chunk=0, api="slow", stream=2))


# ---- the nfft-64 STFT's cached table against every kernel form ----------------------------------
PN, NFR, WLEN, NOV, FS = 256, 9, 20, 19, 1250.0
MAX_SEG = NFR * PN - NOV


@pytest.fixture(scope="module")
def stft_case():
    """The slow-time samples and the float64 references (dB, [seg][bin]) per (window, nfft)."""
    rng = np.random.default_rng(4)
    slow = (np.abs(rng.standard_normal((NFR, PN))) * 30).astype(np.float32)
    x = slow.reshape(-1).astype(np.float64)
    ref = {(w, n): O.spectrogram_pipeline(x, 1.0 / FS, O.stft_window(w), NOV, nfft=n, nbins=0)["intensity"].T
           for w in ("hann", "kaiser") for n in (64, 128)}
    return slow, ref


def _stft(eng, slow_d, flist, d_len, win, nfft, off, direct, stream):
    """One spectrogram in dB into a slice that starts `off` floats into a -7-filled buffer:
    (the slice [seg][bin], the rest of the buffer, max(P))."""
    import torch
    dev, nb = "cuda", nfft // 2 + 1
    pmax = torch.zeros(1, dtype=torch.float32, device=dev)
    nseg = torch.zeros(1, dtype=torch.int64, device=dev)
    buf = torch.full((MAX_SEG * nb + 8,), -7.0, dtype=torch.float32, device=dev)
    out = buf[off:off + MAX_SEG * nb].view(MAX_SEG, nb)
    assert (out.data_ptr() % 16 == 0) == (off % 4 == 0)
    torch.cuda.synchronize()
    if direct:
        eng.stft_power_device(slow_d, flist, d_len, PN, win, WLEN, NOV, nfft, FS, MAX_SEG, None, pmax, nseg, stream=stream)
        eng.stft_db_direct_device(slow_d, flist, d_len, PN, win, WLEN, NOV, nfft, FS, MAX_SEG, pmax, out, stream=stream)
    else:
        eng.stft_power_device(slow_d, flist, d_len, PN, win, WLEN, NOV, nfft, FS, MAX_SEG, out, pmax, nseg, stream=stream)
        eng.stft_db_device(out, nseg, MAX_SEG, nfft, FS, pmax, 0, out, stream=stream)
    torch.cuda.synchronize()
    eng.synchronize()
    b = buf.cpu().numpy()
    return b[off:off + MAX_SEG * nb].reshape(MAX_SEG, nb), np.concatenate([b[:off], b[off + MAX_SEG * nb:]]), \
        float(pmax.item())


@pytest.mark.parametrize("mfma", [None, "0"], ids=["mfma", "valu"])
@pytest.mark.parametrize("fold", ["1", "0"], ids=["fold", "nofold"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("direct", [False, True], ids=["stored_P", "direct_dB"])
def test_stft64_window_change_reaches_every_form(ctx, stft_case, monkeypatch, direct, off, fold, mfma):
    """A window rewritten in place (same pointer, same nfft) must reach whichever kernel runs: the
    aligned nfft-64 forms (k_stft64f applies the taps itself, k_stft64m verifies the cached table),
    and the table forms an output that is not 16-byte aligned or FMCW_STFT_MFMA=0 select
    (k_stft_mfma / k_stft20), which trust the table they are given -- so the API builds it for them
    on every call instead of consulting the cache (stft_form).  Two window slots of one device
    buffer; Hann at slot 0, Kaiser written over it, Hann at slot 1, an nfft-128 call, Kaiser at
    slot 0 again, the same on a second stream whose first call comes after the rewrite, then Hann
    written over slot 0 for both streams.  A stale table gives the other window's spectrogram,
    which is more than 1 dB away where the 1e-3 dB bar applies (asserted from the oracle alone)."""
    import torch
    slow, ref = stft_case
    # before anything runs on the device: a stale table cannot pass the bar
    for w, other in (("hann", "kaiser"), ("kaiser", "hann")):
        sel = ref[(w, 64)] > -80
        assert np.abs(ref[(w, 64)][sel] - ref[(other, 64)][sel]).max() > 1.0
    monkeypatch.setenv("FMCW_STFT64_FOLD", fold)
    if mfma is None:
        monkeypatch.delenv("FMCW_STFT_MFMA", raising=False)
    else:
        monkeypatch.setenv("FMCW_STFT_MFMA", mfma)
    dev = "cuda"
    slow_d = torch.from_numpy(slow).to(dev)
    flist = torch.arange(NFR, dtype=torch.int32, device=dev)
    d_len = torch.tensor([NFR * PN], dtype=torch.int64, device=dev)
    wbuf = torch.zeros(64, dtype=torch.float32, device=dev)
    slot = [wbuf[0:20], wbuf[32:52]]
    taps = {w: torch.tensor(O.stft_window(w), dtype=torch.float32, device=dev) for w in ("hann", "kaiser")}
    s1, s2 = ctx.streams[1], ctx.streams[2]
    # (window written first or None, slot, nfft, stream, the window the slot then holds)
    steps = [("hann", 0, 64, s1, "hann"), ("kaiser", 0, 64, s1, "kaiser"), ("hann", 1, 64, s1, "hann"),
             (None, 1, 128, s1, "hann"), (None, 0, 64, s1, "kaiser"), (None, 0, 64, s2, "kaiser"),
             ("hann", 0, 64, s2, "hann"), (None, 0, 64, s1, "hann")]
    fresh = {}
    for n, (write, k, nfft, stream, holds) in enumerate(steps):
        if write is not None:
            slot[k].copy_(taps[write])                     # in place: the pointer does not change
            torch.cuda.synchronize()
        got, rest, pmax = _stft(ctx.seq, slow_d, flist, d_len, slot[k], nfft, off, direct, stream)
        assert np.all(rest == -7.0), f"step {n}: a write outside the output slice"
        if (holds, nfft) not in fresh:                     # the same call in a new context, held to the oracle's bar
            e = ctx.Engine(0)
            try:
                fresh[(holds, nfft)] = _stft(e, slow_d, flist, d_len, taps[holds].clone(), nfft, off, direct, stream)
            finally:
                e.close()
            want, wrest, _ = fresh[(holds, nfft)]
            assert np.all(wrest == -7.0)
            r = ref[(holds, nfft)]
            sel = r > -80
            assert np.isfinite(want).all() and np.abs(want[sel] - r[sel]).max() <= TOL_FP32_DB
        want, _, wmax = fresh[(holds, nfft)]
        r = ref[(holds, nfft)]
        sel = r > -80
        assert np.abs(got[sel] - r[sel]).max() <= TOL_FP32_DB, f"step {n} ({holds}, nfft {nfft})"
        np.testing.assert_array_equal(got, want, err_msg=f"step {n} ({holds}, nfft {nfft})")
        assert pmax == wmax, f"step {n}"
