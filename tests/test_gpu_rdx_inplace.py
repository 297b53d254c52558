"""k_rdx's one in-place hand-off slot (csrc/kernels_xcd.hip, xcd_place of csrc/fmcw_internal.h) over frame
counts and orders, FMCW_PIPE_XCD forced.

The XCD's slot is rewritten every team step, transposed over (reader, writer) from one step to the next, and
a wave overwrites only the rows it has itself just read.  C, Nr and the team geometry are fixed by the
kernel, so what can go wrong depends on the step a frame runs in and on its neighbours in the slot, not on
a size.  With 8 teams, frame f is step f // 8 of team f % 8:

  alone      F = 61 (8 or 7 steps per team: the steady loop at both parities more than once), c64 and c32h,
             with and without the RD map: every frame bit-identical to the same frame processed alone
  shifted    frames 8..60 as a batch of their own: every frame's step parity flips, its team stays; all
             outputs bit-identical to the F = 61 run
  scales     consecutive frames of a team 4x or 16x apart (the noise scaled by 4^(f mod 3)) against the
             float64 chain at TOL_FP32_REL_L2: a stale 2 KiB chunk of the neighbouring frame in the slot is
             1/32 of a group's rows at 4x to 16x (or 1/4 to 1/16) their size, far above the bar
  nts 1000   F = 29 through the copy with run-time flags (nts < 1024), every frame against itself alone
  chunks     set_chunk_frames(24) over F = 61 (launches of 3, 3 and 2-or-1 steps per team) against one chunk
  context    F = 9 then F = 61 on one context against a fresh context's F = 61

Everything runs on device tensors uploaded once (process_device on slices), so a case takes a few seconds.
"""
import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
from fmcw_radar_processing_amd._lib import FMCW_PIPE_AUTO, FMCW_PIPE_XCD
from oracle import oracle as O
from tests import streams_reference as SR
from tests import xcd_reference as XR
from tests.helpers import TOL_FP32_REL_L2, rd_rel_err, rel_l2

pytestmark = pytest.mark.gpu

F_ALL = 61
DECISIONS = ("profile", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "slow_mag")
STORAGE = {"c64": FMCW_C64, "c32h": FMCW_C32H}


@pytest.fixture
def xcd(engine):
    engine.set_pipeline(FMCW_PIPE_XCD)
    try:
        yield engine
    finally:
        engine.set_chunk_frames(0)
        engine.set_pipeline(FMCW_PIPE_AUTO)


class Batch:
    """Frames of one nts and storage on the device, uploaded once and never modified."""

    def __init__(self, nts, iq, dtype):
        import torch
        self.nts, self.dtype, self.F = nts, dtype, iq.shape[0]
        self.cfg, self.p, self.wr, self.wd, self.cal = XR.build_case(nts)
        dev_iq, self.iq = SR.iq_as_stored(iq, dtype)
        if dtype == FMCW_C64:
            dev_iq = np.ascontiguousarray(dev_iq).view(np.float32).reshape(self.F, XR.PN, nts, 2)
        self.dev = torch.from_numpy(np.ascontiguousarray(dev_iq)).to("cuda")


_batches, _runs = {}, {}


def batch(nts, dtype, F=F_ALL) -> Batch:
    key = (nts, dtype, F)
    if key not in _batches:
        if nts == 1024:
            iq = XR.count_frames(F)[1]
        else:       # white and synthetic frames alternating, as count_frames at nts 1024
            p = XR.build_case(nts)[1]
            iq = np.stack([XR.white(nts, 100 + f).astype(np.complex64) if f % 2 == 0 else
                           O.synth_frames(1, XR.PN, nts, XR.NR, XR.ND, p["dist_per_bin"], frame0=100 + f)[0] for f in range(F)])
        _batches[key] = Batch(nts, iq, dtype)
    return _batches[key]


def run(engine, b: Batch, f0=0, f1=None, want_rd=True) -> dict:
    """Frames f0..f1-1 of the batch through process_device; every buffer pre-filled (NaN, -1)."""
    import torch
    f1 = b.F if f1 is None else f1
    F, M = f1 - f0, b.cfg.max_targets
    half = b.dtype == FMCW_C32H
    dev, nan = dict(device="cuda"), float("nan")
    outs = dict(profile=torch.full((F, XR.NR), nan, **dev), tgt_count=torch.full((F,), -1, dtype=torch.int32, **dev),
                tgt_range_idx=torch.full((F, M), -1, dtype=torch.int32, **dev), tgt_range_mag=torch.full((F, M), nan, **dev),
                tgt_doppler_idx=torch.full((F, M), -1, dtype=torch.int32, **dev), slow_mag=torch.full((F, XR.PN), nan, **dev))
    rd = torch.full((F, XR.NR, XR.ND, 2), nan, dtype=torch.float16 if half else torch.float32, **dev) if want_rd else None
    engine.set_taps(b.cfg, b.cal, b.wr, b.wd)
    torch.cuda.synchronize()
    engine.process_device(b.dev[f0:f1], F, b.dtype, outs, d_rd=rd, out_dtype=b.dtype, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    engine.synchronize()                           # no hand-off wait timed out, no ticket error
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    if want_rd:
        got["rd"] = rd.cpu().numpy()
        assert not np.isnan(got["rd"]).any()
    assert not np.isnan(got["profile"]).any() and (got["tgt_count"] >= 0).all()
    return got


def whole(engine, storage, want_rd) -> dict:
    """The F = 61 run of one storage, shared among the tests and never modified."""
    key = (storage, want_rd)
    if key not in _runs:
        _runs[key] = run(engine, batch(1024, STORAGE[storage]), want_rd=want_rd)
    return _runs[key]


def same(a, b, what, fa=slice(None), fb=slice(None)):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k][fa], b[k][fb], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("want_rd", [True, False], ids=["rd", "nord"])
@pytest.mark.parametrize("storage", list(STORAGE))
def test_every_frame_as_alone(xcd, storage, want_rd):
    b = batch(1024, STORAGE[storage])
    a = whole(xcd, storage, want_rd)
    assert (a["tgt_count"] > 0).any() and (a["tgt_count"] == 0).any()      # both kinds of frame in the batch
    for f in range(F_ALL):
        same(run(xcd, b, f, f + 1, want_rd), a, f"{storage} frame {f} alone", fb=slice(f, f + 1))


@pytest.mark.parametrize("storage", list(STORAGE))
def test_frames_8_to_60_flip_every_parity(xcd, storage):
    b = batch(1024, STORAGE[storage])
    for want_rd in (True, False):
        same(run(xcd, b, 8, F_ALL, want_rd), whole(xcd, storage, want_rd), f"{storage} frames 8..60", fb=slice(8, F_ALL))


def test_neighbouring_frames_of_very_different_scale(xcd):
    # 40 frames: 5 steps on every team, the steady loop at both parities; frames f and f + 8 share a team
    # and 4^(f mod 3) differs between them by 4x or 16x
    F = 40
    cal = O.synth_cal(1024)
    iq = np.stack([(cal[None, :] + 4.0 ** (f % 3) * (XR.white(1024, 300 + f) - cal[None, :])).astype(np.complex64) for f in range(F)])
    b = Batch(1024, iq, FMCW_C64)
    ref = O.process_frames(b.iq, b.cal, b.p, b.wr, b.wd, want_cube=True, want_rd=True, rd_all_rows=True)
    got = run(xcd, b)
    rd = got["rd"].astype(np.float64)
    e_rd = rd_rel_err(rd[..., 0] + 1j * rd[..., 1], ref["rd"], ref["cube"], b.wd, XR.ND)
    e_prof = rel_l2(got["profile"], ref["profile"], axis=1)
    print(f"\nin-place scales F {F}: rd {e_rd.max():.2e} (frame {int(np.argmax(e_rd))}) profile {e_prof.max():.2e} "
          f"(frame {int(np.argmax(e_prof))})")
    assert e_rd.max() <= TOL_FP32_REL_L2, (int(np.argmax(e_rd)), e_rd)
    assert e_prof.max() <= TOL_FP32_REL_L2, (int(np.argmax(e_prof)), e_prof)


def test_nts_1000_run_time_copy(xcd):
    b = batch(1000, FMCW_C64, 29)
    a = run(xcd, b)
    for f in range(b.F):
        same(run(xcd, b, f, f + 1), a, f"nts 1000 frame {f} alone", fb=slice(f, f + 1))


@pytest.mark.parametrize("storage", list(STORAGE))
def test_chunks_of_24(xcd, storage):
    b = batch(1024, STORAGE[storage])
    a = whole(xcd, storage, True)
    xcd.set_chunk_frames(24)
    try:
        same(run(xcd, b), a, f"{storage} in chunks of 24")
    finally:
        xcd.set_chunk_frames(0)


@pytest.mark.parametrize("storage", list(STORAGE))
def test_short_then_long_on_one_context(xcd, storage):
    from fmcw_radar_processing_amd.engine import Engine
    b = batch(1024, STORAGE[storage])
    a = whole(xcd, storage, True)
    same(run(xcd, b, 0, 9), a, f"{storage} F 9", fb=slice(0, 9))
    same(run(xcd, b), a, f"{storage} F 61 after F 9 on one context")
    fresh = Engine(0)
    try:
        fresh.set_pipeline(FMCW_PIPE_XCD)
        same(run(fresh, b), a, f"{storage} F 61 on a fresh context")
    finally:
        fresh.close()
