"""GPU: the range-angle stage (csrc/kernels_ra.hip through fmcw_cov_device, fmcw_ra_device and
fmcw_ra) against the references of tests/ra_reference.py, which run on exactly the bytes the device is
given.  Stage 1 is held to the error bound of include/fmcw.h on every entry; stage 2 is compared byte
for byte on the device's own cov bytes, no cell exempt.  Device buffers sit between guards of NaN
that must come back untouched; inputs must come back unchanged."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64, FmcwError, RaConfig, _lib
from fmcw_radar_processing_amd import params as P
from fmcw_radar_processing_amd.engine import Engine
from tests import ra_reference as R
from tests.test_ra_host import REJECTED, _q, table

pytestmark = pytest.mark.gpu

F32 = np.float32
U = R.U
GUARD = 2                       # guard frames before and after every buffer
NAN32 = 0x7FC00000
CASES = R.parity_cases()


class At:
    """A device address, as engine._ptr reads one."""
    def __init__(self, a):
        self.a = a

    def data_ptr(self):
        return self.a


def cfg_of(A, K=8, gate=(0, 0), dc=0, capon=False, load=1e-3):
    return _lib.RaParams(A, K, gate[0], gate[1], dc, _lib.FMCW_RA_CAPON if capon else 0, load)


def guarded(frames):
    """uint32 words [F][words] -> a device tensor with GUARD frames of NaN words either side."""
    import torch
    frames = np.ascontiguousarray(frames)
    h = np.full((frames.shape[0] + 2 * GUARD, frames.shape[1]), NAN32, np.uint32)
    h[GUARD:GUARD + frames.shape[0]] = frames
    return torch.from_numpy(h.view(np.int32)).to("cuda")


def inner(t, words):
    """The frames between the guards, as uint32 [F][words]; the guards must be untouched."""
    m = t.cpu().numpy().view(np.uint32).reshape(-1, words)
    assert (m[:GUARD] == NAN32).all() and (m[-GUARD:] == NAN32).all(), "a guard frame was written"
    return np.ascontiguousarray(m[GUARD:-GUARD])


def cov_run(engine, chans, q, arena=False, F=None, nr=None, nd=None, dtype=None, shift=None, drop=None, rejects=False,
            stream=None):
    """fmcw_cov_device over map buffers between guard frames of NaN, the channels as separate
    allocations or (arena) as slices of one.  shift: {("rd", a) or "cov": bytes} moves a pointer off
    its place, drop: a ("rd", a) / "cov" whose pointer is NULL, F / nr / nd / dtype override what the
    call is told; rejects: the call must fail with FMCW_E_ARG and cov must then hold what it held.
    The inputs must come back unchanged.  Returns cov float32 [F][nr][T][2] as the buffer holds it."""
    import torch
    A = len(chans)
    half = np.asarray(chans[0]).dtype == np.float16
    rows, mr, md = np.asarray(chans[0]).shape[:3]
    raws = [np.ascontiguousarray(c).view(np.uint32).reshape(rows, -1) for c in chans]
    fbytes = raws[0].shape[1] * 4
    T2 = q.n_chan * (q.n_chan + 1) if 1 <= q.n_chan <= 8 else A * (A + 1)
    cw = mr * T2
    if arena:
        d_all = guarded(np.concatenate([np.concatenate([r, np.full((2 * GUARD, r.shape[1]), NAN32, np.uint32)]) for r in raws]))
        per = (rows + 2 * GUARD) * fbytes
        addr_in = [d_all.data_ptr() + GUARD * fbytes + a * per for a in range(A)]
    else:
        d_in = [guarded(r) for r in raws]
        addr_in = [t.data_ptr() + GUARD * fbytes for t in d_in]
    d_cov = guarded(np.full((rows, cw), NAN32, np.uint32))
    sh = dict(shift or {})
    p_in = [At(0 if drop == ("rd", a) else addr_in[a] + sh.get(("rd", a), 0)) for a in range(A)]
    p_cov = At(0 if drop == "cov" else d_cov.data_ptr() + GUARD * cw * 4 + sh.get("cov", 0))
    torch.cuda.synchronize()

    def call():
        engine.cov_device(q, p_in, (FMCW_C32H if half else FMCW_C64) if dtype is None else dtype, rows if F is None else F,
                          mr if nr is None else nr, md if nd is None else nd, p_cov,
                          stream=torch.cuda.current_stream() if stream is None else stream)
    try:
        if rejects:
            with pytest.raises(FmcwError, match="E_ARG"):
                call()
        else:
            call()
    finally:
        torch.cuda.synchronize()
    if arena:
        m = d_all.cpu().numpy().view(np.uint32).reshape(-1, raws[0].shape[1])
        per_f = rows + 2 * GUARD
        for a, r in enumerate(raws):
            blk = m[GUARD + a * per_f: GUARD + (a + 1) * per_f]
            assert blk[:rows].tobytes() == r.tobytes() and (blk[rows:] == NAN32).all(), a
        assert (m[:GUARD] == NAN32).all() and (m[-GUARD:] == NAN32).all()
    else:
        for a, (t, r) in enumerate(zip(d_in, raws)):
            assert inner(t, r.shape[1]).tobytes() == r.tobytes(), a           # the input is only read
    out = inner(d_cov, cw)
    if rejects or (F is not None and F <= 0):
        assert (out == NAN32).all()                                           # never written
    return out.view(F32).reshape(rows, mr, T2 // 2, 2)


def ra_run(engine, cov, w, q, want_max=True, F=None, nr=None, shift=None, drop=None, rejects=False, stream=None, mx0=0.0):
    """fmcw_ra_device over cov float32 [F][nr][T][2] and w float32 [K][A][2], all buffers between
    guards of NaN; cov and w must come back unchanged.  Returns (ra float32 [F][nr][K], ra_max)."""
    import torch
    cov = np.ascontiguousarray(cov, F32)
    w = R.weights_f32(w)
    rows, mr = cov.shape[:2]
    K = q.n_ang if 1 <= q.n_ang <= 256 else w.shape[0]
    cw = cov[0].size
    d_cov = guarded(cov.view(np.uint32).reshape(rows, cw))
    d_w = guarded(w.view(np.uint32).reshape(1, -1))
    d_ra = guarded(np.full((rows, mr * K), NAN32, np.uint32))
    d_mx = torch.full((4,), float(mx0), device="cuda")
    sh = dict(shift or {})
    ptr = {"cov": d_cov.data_ptr() + GUARD * cw * 4, "w": d_w.data_ptr() + GUARD * w.size * 4,
           "ra": d_ra.data_ptr() + GUARD * mr * K * 4, "max": d_mx.data_ptr() if want_max else 0}
    p = {k: At(0 if drop == k else v + sh.get(k, 0)) for k, v in ptr.items()}
    torch.cuda.synchronize()

    def call():
        engine.range_angle_device(q, p["cov"], rows if F is None else F, mr if nr is None else nr, p["w"], p["ra"],
                                  p["max"] if want_max and drop != "max" else None,
                                  stream=torch.cuda.current_stream() if stream is None else stream)
    try:
        if rejects:
            with pytest.raises(FmcwError, match="E_ARG"):
                call()
        else:
            call()
    finally:
        torch.cuda.synchronize()
    assert inner(d_cov, cw).tobytes() == cov.tobytes() and inner(d_w, w.size).tobytes() == w.tobytes()
    out = inner(d_ra, mr * K)
    mx = d_mx.cpu().numpy()
    assert (mx[1:] == F32(mx0)).all()
    if rejects or (F is not None and F <= 0):
        assert (out == NAN32).all() and mx[0] == F32(mx0)
    return out.view(F32).reshape(rows, mr, K), mx[0]


def _pool_of(c, dominant=False):
    nr, nd, F, A, half, dc, gate = c
    return R.pool(R.case_seed(c), A, F, nr, nd, half, dominant)


# ---- 1. covariance -------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=[R.case_id(c) for c in CASES])
def test_cov_within_its_bound(engine, i):
    """Every shape, A, dtype, frame count, dc_half and gate of ra_reference.parity_cases(): every
    entry within (N + 8) 2^-24 sqrt(R_aa R_bb) of the float64 sums, rows outside the gate and every
    diagonal im exactly zero; separate allocations and arena slices in turn."""
    c = CASES[i]
    nr, nd, F, A, half, dc, gate = c
    chans = _pool_of(c)
    got = cov_run(engine, chans, cfg_of(A, 8, gate, dc), arena=bool(i & 1))
    share = R.assert_cov_within_bound(got, chans, dc, *gate, name=R.case_id(c))
    print(f"{R.case_id(c)}: largest error / bound {share:.3f}")


@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_cov_of_a_dominant_cell(engine, half):
    """One cell 120 dB above unit noise in channels 0 and A - 1: the bound, which scales with
    sqrt(R_aa R_bb) of each pair, still holds for every entry, the pairs without the cell included."""
    for nr, nd, A in ((64, 64, 5), (32, 256, 8)):
        chans = R.pool(900 + nd, A, 2, nr, nd, half, True)
        got = cov_run(engine, chans, cfg_of(A, 8, (0, 0), 0))
        share = R.assert_cov_within_bound(got, chans, 0, name=f"dominant {nr}x{nd}")
        big = got[1, nr // 3, R.tri(A, 0, A - 1)]
        small = got[1, nr // 3, R.tri(A, 1, 2)]
        assert np.hypot(*big) > 1e9 * np.hypot(*small)
        print(f"dominant cell {nr}x{nd} A{A}: largest error / bound {share:.3f}")


# ---- 2. spectra ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_covs(engine):
    """A -> the device's cov [3][16][T][2] of a 16 x 64 pool with rows 0, 1 and 15 gated out (zero rows)."""
    out = {}
    for A in R.AS:
        chans = R.pool(300 + A, A, 3, 16, 64, bool(A & 1))
        out[A] = cov_run(engine, chans, cfg_of(A, 8, (3, 15), 0))
        R.assert_cov_within_bound(out[A], chans, 0, 3, 15)
    return out


@pytest.mark.parametrize("K", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("A", R.AS)
def test_spectra_equal_the_reference_bytes(engine, device_covs, A, K):
    """ra and ra_max, Bartlett and Capon at load 0, 1e-3 and 1, byte for byte the float32 reference on
    the device's own cov bytes; the zero rows of cov are degenerate rows under Capon; the gate of
    stage 2 zeroes further rows."""
    cov = device_covs[A]
    w = table(A, K, 100 * A + K)
    for capon, load, gate in ((False, 0.0, (0, 0)), (True, 0.0, (0, 0)), (True, 1e-3, (2, 9)), (True, 1.0, (0, 0)),
                              (False, 0.0, (16, 16))):
        got, mx = ra_run(engine, cov, w, cfg_of(A, K, gate, 0, capon, load))
        want, wmx = R.spectra_reference(cov, w, capon, load, *gate)
        R.assert_same_bytes(got, want, f"A{A} K{K} capon{capon} load{load} gate{gate}")
        assert mx.tobytes() == wmx.tobytes() and mx == got.max()
        assert not got[:, :2].any()
        if gate == (0, 0):
            assert (got[:, 3:15] > 0).all()
    # without a maximum; and a maximum that is already larger stays
    got, _ = ra_run(engine, cov, w, cfg_of(A, K), want_max=False)
    R.assert_same_bytes(got, R.spectra_reference(cov, w)[0])
    assert ra_run(engine, cov, w, cfg_of(A, K), mx0=3e38)[1] == F32(3e38)


def test_rank_deficient_rows_without_loading(engine):
    """nd = 4 with dc_half 0 keeps 3 bins: R has rank 3 of A = 8.  With load 0 the factorisation
    meets a pivot that is not positive, or only rounding keeps it positive: the bytes equal the
    reference either way, every value finite or zero."""
    A, K = 8, 65
    chans = R.pool(7, A, 2, 16, 4, False)
    cov = cov_run(engine, chans, cfg_of(A, K, (0, 0), 0))
    R.assert_cov_within_bound(cov, chans, 0)
    w = table(A, K, 5)
    for load in (0.0, 1e-3):
        got, mx = ra_run(engine, cov, w, cfg_of(A, K, (0, 0), 0, True, load))
        want, wmx = R.spectra_reference(cov, w, True, load)
        R.assert_same_bytes(got, want, f"load {load}")
        assert np.isfinite(got).all() and mx.tobytes() == wmx.tobytes()


def test_a_callers_own_covariance(engine):
    """Covariances that did not come from stage 1: random Hermitian positive definite rows, an
    all-zero row, a row with a negative diagonal, and garbage in the imaginary part of the diagonal
    entries, which is not read."""
    rng = np.random.default_rng(21)
    for A in (3, 8):
        K = 65
        G = rng.standard_normal((2, 16, A, 2 * A)) + 1j * rng.standard_normal((2, 16, A, 2 * A))
        M = G @ np.conj(np.swapaxes(G, -1, -2))
        cov = np.zeros((2, 16, R.n_tri(A), 2), F32)
        for a in range(A):
            for b in range(a, A):
                cov[..., R.tri(A, a, b), 0], cov[..., R.tri(A, a, b), 1] = M[..., a, b].real, M[..., a, b].imag
        cov[0, 3] = 0
        cov[1, 7, R.tri(A, 1, 1), 0] = -2.0
        clean = cov.copy()
        cov[..., [R.tri(A, a, a) for a in range(A)], 1] = rng.standard_normal((2, 16, A)).astype(F32) * 100
        w = table(A, K, 31 + A)
        for capon in (False, True):
            got, mx = ra_run(engine, cov, w, cfg_of(A, K, (0, 0), 0, capon, 1e-3))
            want, wmx = R.spectra_reference(clean, w, capon, 1e-3)
            R.assert_same_bytes(got, want, f"A{A} capon{capon}")
            assert mx.tobytes() == wmx.tobytes()
            if capon:
                assert not got[0, 3].any() and not got[1, 7].any()


# ---- 3. chain and determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_frames_calls_chunks_and_shards(engine, monkeypatch, half):
    """12 frames in one device call equal twelve one-frame calls and a repeated call; the host call
    at the default chunk, in one-frame chunks and over three shards equals them too, in cov and in
    ra, byte for byte; Engine.range_angle is the two device calls."""
    import torch
    A, K, nr, nd, F = 5, 65, 32, 128, 12
    chans = R.pool(55, A, F, nr, nd, half)
    w = table(A, K, 9)
    for capon in (False, True):
        q = RaConfig(A, K, r_lo=2, r_hi=30, dc_half=1, capon=capon, load=1e-3)
        cov = cov_run(engine, chans, q.abi())
        R.assert_cov_within_bound(cov, chans, 1, 2, 30)
        ra, mx = ra_run(engine, cov, w, q.abi())
        R.assert_same_bytes(ra, R.spectra_reference(cov, w, capon, 1e-3, 2, 30)[0])
        if not capon:
            for f in range(F):
                one = cov_run(engine, [c[f:f + 1] for c in chans], q.abi(), arena=bool(f & 1))
                R.assert_same_bytes(one, cov[f:f + 1], f"frame {f} alone")
                R.assert_same_bytes(ra_run(engine, one, w, q.abi())[0], ra[f:f + 1])
            R.assert_same_bytes(cov_run(engine, chans, q.abi()), cov, "the call repeated")
        multi = Engine([0, 0, 0])
        engines = [engine, multi]
        if torch.cuda.device_count() >= 2:
            engines.append(Engine([0, 1]))
        try:
            for chunk in (None, "1"):
                if chunk:
                    monkeypatch.setenv("FMCW_HOST_CHUNK", chunk)
                for e in engines:
                    h_ra, h_cov, h_mx = e.range_angle(chans, q, w.view(np.complex64)[..., 0])
                    R.assert_same_bytes(h_cov, cov, f"host cov chunk {chunk}")
                    R.assert_same_bytes(h_ra, ra, f"host ra chunk {chunk}")
                    assert F32(h_mx) == mx
            monkeypatch.delenv("FMCW_HOST_CHUNK")
            only_cov = multi.range_angle(chans, q, want_ra=False)
            assert only_cov[0] is None and only_cov[2] == 0.0
            R.assert_same_bytes(only_cov[1], cov)
            only_ra = multi.range_angle(chans, q, w.view(np.complex64)[..., 0], want_cov=False)
            assert only_ra[1] is None
            R.assert_same_bytes(only_ra[0], ra)
        finally:
            for e in engines[1:]:
                e.close()
    e_ra, e_cov, e_mx = engine.range_angle([c[:0] for c in chans], RaConfig(A, K), w.view(np.complex64)[..., 0])      # F = 0
    assert e_ra.shape == (0, nr, K) and e_cov.shape == (0, nr, R.n_tri(A), 2) and e_mx == 0.0


def test_one_long_lived_context_equals_fresh_contexts(engine):
    """A sequence of calls of different A, dtype, shape and flags on the session's context gives the
    bytes that a fresh context gives for each call."""
    seq = [(3, False, 16, 64, True), (8, True, 32, 256, False), (2, False, 16, 4, True), (8, False, 16, 1024, True),
           (3, False, 16, 64, False)]
    for A, half, nr, nd, capon in seq:
        chans = R.pool(70 + A + nd, A, 2, nr, nd, half)
        w = table(A, 33, A)
        q = RaConfig(A, 33, dc_half=0, capon=capon, load=1e-2)
        a = engine.range_angle(chans, q, w.view(np.complex64)[..., 0])
        fresh = Engine(0)
        try:
            b = fresh.range_angle(chans, q, w.view(np.complex64)[..., 0])
        finally:
            fresh.close()
        R.assert_same_bytes(a[1], b[1])
        R.assert_same_bytes(a[0], b[0])
        assert a[2] == b[2]
        R.assert_cov_within_bound(a[1], chans, 0)
        R.assert_same_bytes(a[0], R.spectra_reference(a[1], w, capon, 1e-2)[0])


# ---- 4. against the stages that exist ---------------------------------------------------------------------
def test_bartlett_equals_beam_then_range_time(engine):
    """complex64: the Bartlett ra[f][r][k] against fmcw_beam_device (the same w, 8 directions at a
    time) followed by fmcw_sig_device's range_time with the same dc_half, within the absolute bound
    of tests/test_ra_host.py's Bartlett test plus (N + 8) 2^-24 relative for k_sig."""
    import torch
    A, K, nr, nd, F, dc = 8, 16, 32, 128, 2, 1
    chans = R.pool(123, A, F, nr, nd, False)
    w = table(A, K, 77)
    cov = cov_run(engine, chans, cfg_of(A, K, (0, 0), dc))
    ra, _ = ra_run(engine, cov, w, cfg_of(A, K, (0, 0), dc))
    N = int(R.kept_bins(nd, dc).sum())
    d_in = [torch.from_numpy(np.array(c).view(F32).reshape(F, nr, nd, 2)).to("cuda") for c in chans]
    st = torch.cuda.current_stream()
    worst = 0.0
    for k0 in range(0, K, 8):
        wk = w[k0:k0 + 8].view(np.complex64)[..., 0]
        d_out = [torch.full_like(d_in[0], np.nan) for _ in range(wk.shape[0])]
        engine.beam_device(P.BeamConfig(wk), d_in, FMCW_C64, F, nr, nd, d_out, stream=st)
        for b in range(wk.shape[0]):
            rt = torch.full((F, nr), np.nan, device="cuda")
            mx = torch.zeros(1, device="cuda")
            engine.signature_device(P.SigConfig(dc_half=dc), d_out[b], FMCW_C64, F, nr, nd, None, rt, None, mx, stream=st)
            torch.cuda.synchronize()
            rt = rt.cpu().numpy().astype(np.float64)
            wabs = np.hypot(w[k0 + b, :, 0].astype(np.float64), w[k0 + b, :, 1].astype(np.float64))
            diag = np.stack([cov[..., R.tri(A, a, a), 0].astype(np.float64) for a in range(A)], axis=-1)
            bound = (N + 8 + 4 * A * A) * U * (np.sqrt(diag) * wabs).sum(axis=-1) ** 2 + (N + 8) * U * rt
            err = np.abs(ra[..., k0 + b].astype(np.float64) - rt)
            assert (err <= bound).all(), (k0 + b, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    print(f"Bartlett against beam + range_time: largest error / bound {worst:.3f}")
    assert worst > 0


@pytest.mark.parametrize("half", [False, True], ids=["c64", "c32h"])
def test_two_sources_on_the_device(engine, half):
    """The scenario of tests/test_ra_host.py through the library: the device's Bartlett map shows one
    peak between the two sources and its Capon map the two, in all 8 frames; the peak sets equal the
    reference's (as the bytes do)."""
    S = R.SCENE
    chans = R.scene(1, half)
    w = Engine.ra_weights(S["A"], R.scene_sines(), S["spacing"])
    peaks = {}
    for capon in (False, True):
        q = RaConfig(S["A"], S["n_ang"], dc_half=S["dc_half"], capon=capon, load=S["load"])
        ra, cov, mx = engine.range_angle(chans, q, w)
        want, _ = R.spectra_reference(cov, R.weights_f32(w), capon, S["load"])
        R.assert_same_bytes(ra, want)
        peaks[capon] = [R.peaks(ra[f, S["row"]]) for f in range(S["frames"])]
        assert peaks[capon] == [R.peaks(want[f, S["row"]]) for f in range(S["frames"])]
        assert mx == ra.max() and np.unravel_index(ra.argmax(), ra.shape)[1] == S["row"]
    assert all(len(p) == 1 and p[0] in (34, 35) for p in peaks[False]), peaks[False]
    assert all(p == list(S["points"]) for p in peaks[True]), peaks[True]


# ---- 5. arguments ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REJECTED))
def test_device_calls_reject_what_the_check_rejects(engine, name):
    """E_ARG before any launch: every buffer keeps what it held (cov_run and ra_run check it), stage
    ra counts nothing.  Stage 2 has no nd: the rules that need one are stage 1's and the host call's."""
    over, nr, nd, _ = REJECTED[name]
    q = _q(**dict(over))
    A = max(min(q.n_chan, 8), 2)
    chans = R.pool(3, A, 2, 64, 16, False)
    engine.timing_reset()
    engine.timing(1)
    try:
        cov_run(engine, chans, q, nr=nr, nd=nd, rejects=True)
        if "nd" not in name and name != "dc_band_is_the_whole_axis":
            cov = np.ones((2, 64, R.n_tri(A), 2), F32)
            ra_run(engine, cov, np.ones((max(min(q.n_ang, 256), 1), A, 2), F32), q, nr=nr, rejects=True)
        out = np.full((2, 64, 8), np.nan, F32)
        ptrs = (ct.c_void_p * A)(*[np.asarray(c).ctypes.data for c in chans])
        assert engine.lib.fmcw_ra(engine.h, ct.byref(q), ptrs, FMCW_C64, 2, nr, nd, out.ctypes.data, None, out.ctypes.data,
                                  None) == _lib.FMCW_E_ARG
        assert np.isnan(out).all()
        assert engine.timing_read()["ra"][1] == 0
    finally:
        engine.timing(0)


def test_call_arguments(engine):
    nr, nd, F, A, K = 64, 16, 3, 3, 9
    chans = R.pool(4, A, F, nr, nd, False)
    q = cfg_of(A, K)
    w = table(A, K, 2)
    # F = 0 is a no-op, whatever the pointers
    cov_run(engine, chans, q, F=0)
    cov_run(engine, chans, q, F=0, drop=("rd", 1))
    for kw in (dict(F=-1), dict(dtype=2), dict(dtype=-1), dict(drop=("rd", 0)), dict(drop=("rd", 2)), dict(drop="cov"),
               dict(shift={("rd", 1): 8}), dict(shift={("rd", 2): 4}), dict(shift={"cov": 8}), dict(shift={"cov": 4})):
        cov_run(engine, chans, q, rejects=True, **kw)
        cov_run(engine, chans, q, rejects=True, arena=True, **kw)
    cov = cov_run(engine, chans, q)
    ra_run(engine, cov, w, q, F=0)
    ra_run(engine, cov, w, q, F=0, drop="w")
    for kw in (dict(F=-1), dict(drop="cov"), dict(drop="w"), dict(drop="ra"), dict(shift={"cov": 8}), dict(shift={"w": 8}),
               dict(shift={"ra": 4}), dict(shift={"max": 2})):
        ra_run(engine, cov, w, q, rejects=True, **kw)
    # an unused pointer may be anything: the array holds n_chan entries that count
    R.assert_same_bytes(cov_run(engine, list(chans) + [chans[0]], q, shift={("rd", 3): 4}), cov)
    # the host call: the same rules before any device work, and not both outputs NULL
    lib, h = engine.lib, engine.h
    ptrs = (ct.c_void_p * A)(*[np.asarray(c).ctypes.data for c in chans])
    o_cov = np.full(cov.shape, np.nan, F32)
    o_ra = np.full((F, nr, K), np.nan, F32)
    mx = ct.c_float(-1.0)
    wp, cp, rp = w.ctypes.data, o_cov.ctypes.data, o_ra.ctypes.data
    assert lib.fmcw_ra(h, ct.byref(q), ptrs, FMCW_C64, F, nr, nd, wp, None, None, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert b"both NULL" in lib.fmcw_last_error()
    assert lib.fmcw_ra(h, ct.byref(q), ptrs, FMCW_C64, F, nr, nd, None, cp, rp, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert lib.fmcw_ra(h, ct.byref(q), None, FMCW_C64, F, nr, nd, wp, cp, rp, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert lib.fmcw_ra(h, ct.byref(q), (ct.c_void_p * A)(ptrs[0], 0, ptrs[2]), FMCW_C64, F, nr, nd, wp, cp, rp,
                       ct.byref(mx)) == _lib.FMCW_E_ARG
    assert lib.fmcw_ra(h, ct.byref(q), ptrs, 2, F, nr, nd, wp, cp, rp, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert lib.fmcw_ra(h, ct.byref(q), ptrs, FMCW_C64, -1, nr, nd, wp, cp, rp, ct.byref(mx)) == _lib.FMCW_E_ARG
    assert np.isnan(o_cov).all() and np.isnan(o_ra).all() and mx.value == -1.0
    assert lib.fmcw_ra(h, ct.byref(q), None, FMCW_C64, 0, nr, nd, None, cp, None, ct.byref(mx)) == _lib.FMCW_OK      # F = 0
    assert mx.value == 0.0 and np.isnan(o_cov).all()
    with pytest.raises(ValueError):
        engine.range_angle(chans[:2], RaConfig(A, K), w.view(np.complex64)[..., 0])
    with pytest.raises(ValueError):
        engine.range_angle(chans, RaConfig(A, K))


def test_stream_and_timing(engine):
    """A non-default torch stream; timing stage `ra`: one event pair per k_cov launch and one per k_ra
    launch, none with timing off, none for a rejected call."""
    import torch
    A, K = 3, 65
    chans = R.pool(9, A, 2, 32, 256, False)
    w = table(A, K, 4)
    q = cfg_of(A, K, (0, 0), 0, True, 1e-3)
    engine.timing_reset()
    cov = cov_run(engine, chans, q)
    ra, mx = ra_run(engine, cov, w, q)
    assert engine.timing_read()["ra"] == (0.0, 0)
    s = torch.cuda.Stream()
    engine.timing(1)
    try:
        with torch.cuda.stream(s):
            side = cov_run(engine, chans, q, stream=s)
        s.synchronize()
        ms, n = engine.timing_read()["ra"]
        assert n == 1 and ms > 0
        with torch.cuda.stream(s):
            side_ra, side_mx = ra_run(engine, side, w, q, stream=s)
        s.synchronize()
        assert engine.timing_read()["ra"][1] == 2
        engine.range_angle(chans, RaConfig(A, K, capon=True), w.view(np.complex64)[..., 0])      # one chunk: a k_cov and a k_ra
        assert engine.timing_read()["ra"][1] == 4
        engine.range_angle(chans, RaConfig(A, K), want_ra=False)
        assert engine.timing_read()["ra"][1] == 5
        cov_run(engine, chans, q, F=-1, rejects=True)
        ra_run(engine, cov, w, q, F=-1, rejects=True)
        assert engine.timing_read()["ra"][1] == 5
    finally:
        engine.timing(0)
        engine.timing_reset()
    R.assert_same_bytes(side, cov)
    R.assert_same_bytes(side_ra, ra)
    assert side_mx == mx


# ---- 6. the channel counts between the named ones, over several workgroups ---------------------------------
@pytest.mark.parametrize("A", [4, 6, 7])
def test_every_other_channel_count(engine, A):
    """A = 4, 6, 7 (the kernels are instantiated on A, and the cases above run 2, 3, 5, 8): stage 1 in
    both storages with rows that fill a wave-load and rows that do not, then both spectra over 192
    rows, three workgroups of k_ra, on the device's cov bytes."""
    F, nr, K = 3, 64, 65
    w = table(A, K, 40 + A)
    for nd in (256, 16):
        for half in (False, True):
            chans = R.pool(600 + 10 * A + nd, A, F, nr, nd, half)
            cov = cov_run(engine, chans, cfg_of(A, K, (2, 63), 0), arena=half)
            share = R.assert_cov_within_bound(cov, chans, 0, 2, 63, name=f"A{A} nd{nd} half{half}")
            print(f"A{A} {nr}x{nd} {'c32h' if half else 'c64'}: largest error / bound {share:.3f}")
            if nd == 16 and not half:
                continue
            for capon in (False, True):
                got, mx = ra_run(engine, cov, w, cfg_of(A, K, (0, 0), 0, capon, 1e-3))
                want, wmx = R.spectra_reference(cov, w, capon, 1e-3)
                R.assert_same_bytes(got, want, f"A{A} nd{nd} half{half} capon{capon}")
                assert mx.tobytes() == wmx.tobytes()
                assert not got[:, 0].any() and not got[:, 63].any() and (got[:, 1:63] > 0).all()


@pytest.mark.parametrize("A", [2, 8])
def test_spectra_over_several_workgroups(engine, A):
    """n_ang 1, 64 and 256 over 160 rows: two whole workgroups of k_ra and a partial one."""
    F, nr, nd = 10, 16, 64
    chans = R.pool(700 + A, A, F, nr, nd, False)
    cov = cov_run(engine, chans, cfg_of(A, 8, (0, 0), 0))
    for K in (1, 64, 256):
        w = table(A, K, 50 + A + K)
        for capon in (False, True):
            got, mx = ra_run(engine, cov, w, cfg_of(A, K, (3, 14), 0, capon, 1e-3))
            want, wmx = R.spectra_reference(cov, w, capon, 1e-3, 3, 14)
            R.assert_same_bytes(got, want, f"A{A} K{K} capon{capon}")
            assert mx.tobytes() == wmx.tobytes()
