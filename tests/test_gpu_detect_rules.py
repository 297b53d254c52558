"""GPU: the peak rule (:211, select_peaks in frame_ops.h, k_rdx's candidate keys) and the Doppler
index (:227-239) at their decision edges, on both schedules and under fp16 storage.

Every run is held to two references (tests/detect_reference.py):

  self-consistent  tgt_count, tgt_range_idx and tgt_range_mag equal peaks() of the profile the same
                   call returned, bit for bit; tgt_doppler_idx is what doppler_choice() allows on the
                   returned RD row; slots j >= count are zero.  No frame is left out, ties included.
  oracle           the float64 oracle with the float32 parameters of the C-ABI, at the bars of
                   tests/helpers.py; exact on the decisions except the frames and rows the oracle
                   itself marks ambiguous (at most 10 % of a batch: test_detect_reference_host.py).

The scenes S1-S11 and the parameter sets are described with the batches in detect_reference.py.
The slow-time row is compared with the oracle's row at the bin the GPU chose, normalised by the
norm of the strongest row of that frame's cube (the row's own norm whenever the detected row is the
strongest): the rounding is that of the uncancelled data (helpers.rd_rel_err)."""
import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS, FMCW_PIPE_XCD
from fmcw_radar_processing_amd import params as P
from tests import detect_reference as R
from tests.helpers import TOL_FP16_REL_L2, TOL_FP32_REL_L2

pytestmark = pytest.mark.gpu

DEPLOYED = (64, 16, 256, 16)
RAGGED = (100, 20, 128, 32)


@pytest.fixture
def eng(engine):
    try:
        yield engine
    finally:
        engine.set_pipeline(FMCW_PIPE_AUTO)
        engine.set_chunk_frames(0)


# ---- runs ------------------------------------------------------------------------------------
def _run(eng, b, cfg, pipe, want_rd=True):
    eng.set_pipeline(pipe)
    eng.set_taps(cfg, b.cal, b.wr, b.wd)
    got = eng.process(b.iq, want_rd=want_rd)
    eng.synchronize()
    return got


def _run_fp16(eng, b, cfg):
    """c32h in, c32h RD out, device path, output buffers shaped (F, M) and pre-filled so that a slot
    the kernel leaves unwritten shows."""
    import torch

    from fmcw_radar_processing_amd import FMCW_C32H
    F, M = b.iq.shape[0], cfg.max_targets
    eng.set_pipeline(FMCW_PIPE_XCD)
    eng.set_taps(cfg, b.cal, b.wr, b.wd)
    d_iq = torch.from_numpy(b.iq16()[0]).cuda()

    def buf(shape, dtype):
        return torch.full(shape, -7, dtype=dtype, device="cuda")

    outs = dict(profile=buf((F, cfg.nr), torch.float32), tgt_count=buf((F,), torch.int32),
                tgt_range_idx=buf((F, M), torch.int32), tgt_range_mag=buf((F, M), torch.float32),
                tgt_doppler_idx=buf((F, M), torch.int32), slow_mag=buf((F, cfg.pn), torch.float32))
    d_rd = torch.empty((F, cfg.nr, cfg.nd, 2), dtype=torch.float16, device="cuda")
    eng.process_device(d_iq, F, FMCW_C32H, outs, d_rd=d_rd, out_dtype=FMCW_C32H, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    eng.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    got["rd"] = d_rd.cpu().numpy()              # float16 pairs holding D / (Nr Nd)
    return got


def _rd(got, cfg, f, r=slice(None)):
    """RD row r (or every row) of frame f as the device holds it, complex128."""
    v = got["rd"][f, r]
    if v.dtype == np.float16:
        v = v.astype(np.float64) * (cfg.nr * cfg.nd)
        return v[..., 0] + 1j * v[..., 1]
    return v.astype(np.complex128)


# ---- the two references ------------------------------------------------------------------------
def check_self(got, cfg):
    """The self-consistent assertion; returns flagged [F][M]: the rows doppler_choice calls ambiguous."""
    prm = R.abi_params(cfg)
    F, M = got["tgt_range_idx"].shape
    assert M == cfg.max_targets and got["profile"].dtype == np.float32 and got["tgt_range_mag"].dtype == np.float32
    flagged = np.zeros((F, M), bool)
    for f in range(F):
        n, idx, mag = R.peaks(got["profile"][f], prm, M)
        assert got["tgt_count"][f] == n, (f, got["tgt_count"][f], n)
        np.testing.assert_array_equal(got["tgt_range_idx"][f], idx, err_msg=f"frame {f}")
        np.testing.assert_array_equal(got["tgt_range_mag"][f].view(np.int32), mag.view(np.int32), err_msg=f"frame {f}")
        assert np.all(got["tgt_doppler_idx"][f, n:] == 0), f
        if "rd" not in got:
            continue
        for j in range(n):
            c = R.doppler_choice(_rd(got, cfg, f, idx[j] - 1), prm["doppler_thr"], cfg.doppler_fallback_idx)
            flagged[f, j] = c["ambiguous"]
            d = int(got["tgt_doppler_idx"][f, j])
            assert d in c["allowed"] if c["ambiguous"] else d == c["idx"], (f, j, d, c["idx"], sorted(c["allowed"]))
    return flagged


def check_oracle(got, b, cfg, fp16=False):
    """The oracle comparison.  Returns (frames, rows) left out as ambiguous and the per-frame slow-row
    errors relative to the row's own norm."""
    ob = b.oracle(fp16)
    q = R.oracle_params(b.p, cfg, cfg.max_targets)
    dec = R.decide(ob, q)
    tol = TOL_FP16_REL_L2 if fp16 else TOL_FP32_REL_L2
    fa, ra = R.ambiguity(ob, dec, q, tol)
    R.check_caps(fa, ra, dec)
    ok = ~fa
    np.testing.assert_array_equal(got["tgt_count"][ok], dec["tgt_count"][ok])
    np.testing.assert_array_equal(got["tgt_range_idx"][ok], dec["tgt_range_idx"][ok])
    np.testing.assert_allclose(got["tgt_range_mag"][ok], dec["tgt_range_mag"][ok], rtol=TOL_FP32_REL_L2, atol=0)
    if "rd" in got:                                # without the RD map: compared with the with-RD run instead
        rows = ok[:, None] & ~ra
        np.testing.assert_array_equal(got["tgt_doppler_idx"][rows], dec["tgt_doppler_idx"][rows])
    F = len(fa)
    # profile: fp32 bar; under fp16 storage the blocks fp16_fp32_bins names at the fp32 bar, block by block
    # (relative to the norm of all of them), the others at the fp16-storage bar
    keep = P.fp16_fp32_bins(cfg) if fp16 else np.ones(cfg.nr, bool)
    perr = np.abs(got["profile"].astype(np.float64) - ob["profile"])
    den = np.sqrt(np.sum(ob["profile"][:, keep] ** 2, axis=1))
    if fp16:
        for blk in sorted(set(np.nonzero(keep)[0] // 128)):
            e = np.sqrt(np.sum(perr[:, 128 * blk: 128 * blk + 128] ** 2, axis=1)) / den
            assert e.max() <= TOL_FP32_REL_L2, (blk, e.max(), int(np.argmax(e)))
        if (~keep).any():
            e = np.sqrt(np.sum(perr[:, ~keep] ** 2, axis=1)) / np.sqrt(np.sum(ob["profile"][:, ~keep] ** 2, axis=1))
            assert e.max() <= TOL_FP16_REL_L2, e.max()
    else:
        e = np.sqrt(np.sum(perr ** 2, axis=1)) / den
        assert e.max() <= TOL_FP32_REL_L2, (e.max(), int(np.argmax(e)))
    if "rd" in got:
        for f in range(F):
            e = np.sqrt(np.sum(np.abs(_rd(got, cfg, f) - ob["rd"][f]) ** 2)) / ob["rd_den"][f]
            assert e <= tol, (f, b.names[f], e)
    # slow-time row at the bin the GPU chose
    own = np.zeros(F)
    for f in range(F):
        if got["tgt_count"][f] == 0:
            assert np.all(got["slow_mag"][f] == 0), f
            continue
        norms = np.sqrt(np.sum(ob["absx"][f] ** 2, axis=0))
        ref = ob["absx"][f][:, got["tgt_range_idx"][f, 0] - 1]
        num = np.sqrt(np.sum((got["slow_mag"][f].astype(np.float64) - ref) ** 2))
        own[f] = num / np.sqrt(np.sum(ref ** 2))
        assert num / norms.max() <= TOL_FP32_REL_L2, (f, b.names[f], num / norms.max(), own[f])
    return fa, ra, own


def check_same_decisions(a, c, frames, rows, what):
    """Two runs' decisions: equal on `frames` [F] bool, the Doppler index on `rows` [F][M] bool."""
    for k in ("tgt_count", "tgt_range_idx"):
        np.testing.assert_array_equal(a[k][frames], c[k][frames], err_msg=f"{what}: {k}")
    m = frames[:, None] & rows
    np.testing.assert_array_equal(a["tgt_doppler_idx"][m], c["tgt_doppler_idx"][m], err_msg=f"{what}: tgt_doppler_idx")


# ---- the parameter sets ------------------------------------------------------------------------
def _main_cfg(which):
    b = R.batch_main()
    if which == "s10":
        return b, R.with_params(b.cfg, 3, doppler_thr=R.s10_threshold(b, b.oracle()))
    return b, R.with_params(b.cfg, int(which))


def _noise_cfg(fp16=False):
    b = R.batch_noise()
    ob = b.oracle(fp16)
    thr = R.median_row_peak(ob, R.decide(ob, R.oracle_params(b.p, b.cfg, 8)))
    return b, R.with_params(b.cfg, 8, doppler_thr=thr)


def _case(name, fp16=False):
    kind, _, which = name.partition("-")
    if kind == "main":
        return _main_cfg(which)
    if kind == "noise":
        return _noise_cfg(fp16)
    if kind == "zero":
        b = R.batch_zero()
        return b, R.with_params(b.cfg, 1)
    b = R.batch_gate(which)
    return b, R.with_params(b.cfg, 3)


_xcd = {}


def _xcd_run(eng, name):
    """The XCD-schedule c64 run of a case with the RD map (made once; the streams tests compare with it)."""
    if name not in _xcd:
        b, cfg = _case(name)
        got = _run(eng, b, cfg, FMCW_PIPE_XCD)
        _xcd[name] = (got, check_self(got, cfg))
    return _xcd[name]


def _check_gate_disagreement(got, b, cfg):
    """Set 4: the detections reach both edge bins of CfarConfig.for_config's gate, and on the planted tone's
    bin the kernels follow the float32 gate, where the oracle with the double-precision parameters detects
    the tone."""
    ob = b.oracle()
    gate = P.CfarConfig.for_config(cfg)
    used = got["tgt_range_idx"][got["tgt_range_idx"] > 0]
    assert used.min() == gate.r_lo and used.max() == gate.r_hi   # tones sit on both edge bins of the kernels' gate
    if np.array_equal(R.gate_bins(cfg), R.double_gate(cfg)):      # 'exact': both limits on a bin, the gates agree
        return
    dbl = R.decide(ob, dict(b.p, max_targets=cfg.max_targets, min_d=cfg.min_d, max_d=cfg.max_d,
                            doppler_fallback_idx=cfg.doppler_fallback_idx))
    abi = R.decide(ob, R.oracle_params(b.p, cfg, cfg.max_targets))
    differ = dbl["tgt_count"] != abi["tgt_count"]
    assert differ.sum() == 2
    assert np.all(got["tgt_count"][differ] == 0) and np.all(dbl["tgt_count"][differ] == 1)
    np.testing.assert_array_equal(got["tgt_count"], abi["tgt_count"])


MAIN = ["main-1", "main-8", "main-3", "main-s10"]


# ---- FMCW_PIPE_XCD, c64 ------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAIN + ["noise", "zero", "gate-max", "gate-min", "gate-exact"])
def test_xcd_c64(eng, name, capsys):
    b, cfg = _case(name)
    got, flagged = _xcd_run(eng, name)
    fa, ra, own = check_oracle(got, b, cfg)
    if name.startswith("gate"):
        _check_gate_disagreement(got, b, cfg)
        return
    if name == "zero":                        # the static frame's RD row is exactly zero: first maximum, 0 >= 0
        assert np.all(got["rd"][0, 12] == 0) and got["tgt_doppler_idx"][0, 0] == 1 and not flagged.any()
    if name == "main-1":                      # S8, the natural candidate miss: the figure DESIGN.md quotes
        with capsys.disabled():
            print("\nS8 slow row, relative to its own norm:", ["%.3g" % own[f] for f in b.frames("S8")])
    # without the RD map (the row peaks come from k_rdx): the same outputs, except the Doppler index on
    # the rows flagged ambiguous
    lean = _run(eng, b, cfg, FMCW_PIPE_XCD, want_rd=False)
    check_self(lean, cfg)
    for k in ("profile", "tgt_count", "tgt_range_idx", "tgt_range_mag", "slow_mag"):
        np.testing.assert_array_equal(got[k], lean[k], err_msg=k)
    np.testing.assert_array_equal(got["tgt_doppler_idx"][~flagged], lean["tgt_doppler_idx"][~flagged])


def test_xcd_chunking(eng):
    """Parameter set 2 (M = 8) in chunks of 5 frames: bit-identical to the unchunked call."""
    b, cfg = _case("main-8")
    got, _ = _xcd_run(eng, "main-8")
    eng.set_chunk_frames(5)
    c = _run(eng, b, cfg, FMCW_PIPE_XCD)
    for k in got:
        np.testing.assert_array_equal(got[k], c[k], err_msg=k)


# ---- FMCW_PIPE_XCD, fp16 storage, device path --------------------------------------------------------
@pytest.mark.parametrize("name", ["main-1", "main-8", "main-3", "noise"])
def test_xcd_fp16(eng, name):
    b, cfg = _case(name, fp16=True)
    got = _run_fp16(eng, b, cfg)
    check_self(got, cfg)
    check_oracle(got, b, cfg, fp16=True)


@pytest.mark.parametrize("gate", list(R.WIDE_GATES))
def test_xcd_fp16_wide_gate(eng, gate):
    """Set 5: the blocks around the gate stay fp32 (fp16_fp32_bins), so the profile there, the target
    magnitudes and the slow-time rows meet the fp32 bar; 'all' admits every bin (empty mask)."""
    b = R.batch_wide()
    cfg = R.with_params(b.cfg, 3, **R.WIDE_GATES[gate])
    got = _run_fp16(eng, b, cfg)
    check_self(got, cfg)
    check_oracle(got, b, cfg, fp16=True)


# ---- FMCW_PIPE_STREAMS, c64 ---------------------------------------------------------------------
@pytest.mark.parametrize("name", MAIN + ["noise", "zero", "gate-max", "gate-min", "gate-exact"])
def test_streams_c64(eng, name):
    b, cfg = _case(name)
    got = _run(eng, b, cfg, FMCW_PIPE_STREAMS)
    check_self(got, cfg)
    fa, ra, _ = check_oracle(got, b, cfg)
    if name.startswith("gate"):
        _check_gate_disagreement(got, b, cfg)
    x, _ = _xcd_run(eng, name)
    check_same_decisions(got, x, ~fa, ~ra, "streams vs xcd")


@pytest.mark.parametrize("geom,mode", [(DEPLOYED, P.PARITY), (RAGGED, P.THROUGHPUT)], ids=["deployed", "ragged"])
def test_streams_small_geometries(eng, geom, mode):
    """S1-S7 rebuilt for the deployed module's geometry (literal fallback 9) and a ragged one, M = 3."""
    b = R.batch_main(geom, mode)
    cfg = R.with_params(b.cfg, 3)
    got = _run(eng, b, cfg, FMCW_PIPE_STREAMS)
    check_self(got, cfg)
    check_oracle(got, b, cfg)
