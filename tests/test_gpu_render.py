"""GPU: spectrogram.png (radar_processing.m:331-348) rendered by
libfmcw (kernels_render.hip) and written as a palette PNG.

1. The rules: given the same float32 P, the GPU indices equal the numpy
   restatement (oracle/render.py) pixel for pixel (float64 arithmetic, same
   operation order, FMA contraction off in the kernel).
2. End to end: fmcw_stft_png on a slow-time signal against the restatement on
   the float64 oracle's P; fp32 rounding of P may move a colour-index boundary
   or a depth tie, so >= 99.5 % of the pixels agree and no pixel is off by more
   than one colour step except at depth ties (counted separately).
3. The rules at their seams and holes: RENDER_CASES of tests/test_render_host.py (which proves on the CPU that they
   reach the seam, the rows above Nyquist, bins Q does not hold, depth-test ties and the -1e30 floor), exact,
   every byte of the image written; nseg read from the device; the argument checks, the stream and timing stage.
The pixels are parity-unpinned against MATLAB graphics (not runnable here)."""
import numpy as np
import pytest

from fmcw_radar_processing_amd._lib import FmcwError
from oracle import oracle as O
from oracle import render as R
from tests import test_render_host as RH

pytestmark = pytest.mark.gpu


def _slow_signal(L, seed=0):
    rng = np.random.default_rng(seed)
    k = np.arange(L)
    x = np.abs(1.0 + 0.6 * np.sin(2 * np.pi * 37.0 * k / 1250.0) + 0.3 * np.sin(2 * np.pi * 90.0 * k / 1250.0)
               + 0.05 * rng.standard_normal(L))
    return x.astype(np.float32).astype(np.float64)


def _Q(P_nb_nseg, nq):
    """[nseg][nq + 1]: bins 0..nq-1 then the Nyquist bin."""
    P = np.asarray(P_nb_nseg).T
    return np.concatenate([P[:, :nq], P[:, -1:]], axis=1)


@pytest.mark.parametrize("L,nfft,W,H", [(1840, 2048, 640, 400), (900, 64, 300, 120), (3000, 0, 2906, 2038)])
def test_render_rules_exact(engine, L, nfft, W, H):
    import torch
    x = _slow_signal(L)
    prt = 8e-4
    fs = 1 / prt
    nfft = nfft or 2 ** O.nextpow2(L)
    win = O.stft_window("kaiser")
    _, Fv, T, P = O.spectrogram(x, win, 19, nfft, fs)
    P32 = P.astype(np.float32)
    nb = nfft // 2 + 1
    nq = nb - 1 if nfft == 64 else min(nb - 1, int(np.floor(150.0 / (fs / nfft))) + 2)
    Q = np.ascontiguousarray(_Q(P32, nq), np.float32)
    pmax = np.float32(P32.max())
    d_Q = torch.from_numpy(Q).cuda()
    d_nseg = torch.tensor([Q.shape[0]], dtype=torch.int64, device="cuda")
    d_pmax = torch.tensor([pmax], dtype=torch.float32, device="cuda")
    d_img = torch.empty((H, W + 1), dtype=torch.uint8, device="cuda")
    engine.render_spectrogram_device(d_Q, nq, d_nseg, d_pmax, nfft, fs, float(T[0]), float(T[1] - T[0]), W, H, d_img,
                                     stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    img = d_img.cpu().numpy()
    assert np.all(img[:, 0] == 0)
    want = R.render_indices(Q, nq, float(pmax), nfft, fs, float(T[0]), float(T[1] - T[0]), W, H)
    np.testing.assert_array_equal(img[:, 1:], want)
    assert len(np.unique(want)) > 20                  # a real picture, not one colour


def test_stft_png_end_to_end(engine, tmp_path):
    L, prt = 1840, 8e-4                               # 115 deployed frames x 16 chirps
    x = _slow_signal(L, seed=3)
    fs = 1 / prt
    path = tmp_path / "spectrogram.png"
    got = engine.stft_png(x, O.stft_window("kaiser"), 19, fs, str(path))
    idx, pal = R.read_png_indexed(str(path))
    assert idx.shape == (2038, 2906)                  # default: exportgraphics at 600 dpi of the default axes box
    assert got["png_bytes"] == path.stat().st_size
    np.testing.assert_array_equal(pal, R.jet_palette_u8())
    # the JSON-side outputs are those of fmcw_stft
    ref = O.spectrogram_pipeline(x, prt, O.stft_window("kaiser"), 19)
    sel = ref["intensity"].T > -80
    assert np.abs(got["intensity"][sel] - ref["intensity"].T[sel]).max() <= 1e-3
    # the picture against the restatement on the float64 oracle's P
    nfft = got["nfft"]
    _, Fv, T, P = O.spectrogram(x, O.stft_window("kaiser"), 19, nfft, fs)
    nq = min(nfft // 2, int(np.floor(150.0 / (fs / nfft))) + 2)
    want = R.render_indices(_Q(P, nq), nq, float(P.max()), nfft, fs, float(T[0]), float(T[1] - T[0]), 2906, 2038)
    same = np.mean(idx == want)
    assert same >= 0.995, same
    far = np.abs(idx.astype(int) - want.astype(int)) > 1
    assert np.mean(far) <= 0.002, np.mean(far)


# ---- the kernel against the restatement at its seams, holes and ties ------------------------------------------
FILL = 0xA5


def _render(engine, Q, nq, pmax, nfft, fs, t0, dt, W, H, *, nseg=None, stream=None, img=None, **ptrs):
    """One fmcw_render_spectrogram_device call into an image pre-filled with 0xA5: [H][1 + W] bytes back.
    ptrs: d_Q / d_nseg / d_pmax / d_img overridden (None = a NULL pointer)."""
    import torch
    t = dict(d_Q=torch.from_numpy(np.array(Q, np.float32)).cuda(),            # a copy: the shared inputs are read-only
             d_nseg=torch.tensor([len(Q) if nseg is None else nseg], dtype=torch.int64, device="cuda"),
             d_pmax=torch.tensor([pmax], dtype=torch.float32, device="cuda"),
             d_img=torch.full((max(H, 1), max(W, 0) + 1), FILL, dtype=torch.uint8, device="cuda") if img is None else img)
    kept = t["d_img"]
    t.update(ptrs)
    try:
        engine.render_spectrogram_device(t["d_Q"], nq, t["d_nseg"], t["d_pmax"], nfft, fs, t0, dt, W, H, t["d_img"],
                                         stream=torch.cuda.current_stream() if stream is None else stream)
    finally:
        torch.cuda.synchronize()
    return kept.cpu().numpy()


def _assert_picture(img, want):
    assert np.all(img[:, 0] == 0)                       # the PNG filter byte of every row
    np.testing.assert_array_equal(img[:, 1:], want)     # and every other byte is an index: nothing keeps the fill


@pytest.mark.parametrize("zero_pmax", [False, True], ids=["pmax", "pmax0"])
@pytest.mark.parametrize("case", RH.RENDER_CASES, ids=RH.case_id)
def test_render_cases_exact(engine, case, zero_pmax):
    nfft, fs, nq, nseg, W, H, kind = case
    Q, pmax, t0, dt, want, _ = RH.reference(case, zero_pmax)
    img = _render(engine, Q, nq, pmax, nfft, fs, t0, dt, W, H)
    assert img.shape == (H, W + 1)
    _assert_picture(img, want)


@pytest.mark.parametrize("nseg", [24, 13, 2, 1, 0])
def test_nseg_is_read_from_the_device(engine, nseg):
    case = RH.RENDER_CASES[0]
    nfft, fs, nq, rows, W, H, kind = case
    Q0, pmax, t0, dt, _, _ = RH.reference(case)
    assert rows == 24
    Q = Q0.copy()
    Q[nseg:] = np.nan                                   # rows past nseg are not read
    img = _render(engine, Q, nq, pmax, nfft, fs, t0, dt, W, H, nseg=nseg)
    want = R.render_indices(Q0[:nseg], nq, float(pmax), nfft, fs, t0, dt, W, H)
    assert want.any() == (nseg >= 2)
    _assert_picture(img, want)


_OK = dict(nfft=64, nq=32, fs=200.0, dt=0.005, W=255, H=97)
REJECTED = {
    "nfft-odd": dict(nfft=63), "nfft-0": dict(nfft=0), "nq-0": dict(nq=0), "nq-nfft/2+1": dict(nq=33),
    "fs-0": dict(fs=0.0), "fs-nan": dict(fs=float("nan")), "dt-0": dict(dt=0.0), "dt-negative": dict(dt=-0.005),
    "width-0": dict(W=0), "width-65537": dict(W=65537), "height-0": dict(H=0), "height-65536": dict(H=65536),
    "Q-null": dict(d_Q=None), "nseg-null": dict(d_nseg=None), "pmax-null": dict(d_pmax=None), "img-null": dict(d_img=None),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_render_rejects(engine, name):
    """E_ARG before any launch: the image keeps its fill, timing stage `render` counts nothing."""
    import torch
    kw = dict(_OK, **REJECTED[name])
    ptrs = {k: kw.pop(k) for k in list(kw) if k.startswith("d_")}
    Q, pmax, t0, _, _, _ = RH.reference(RH.RENDER_CASES[0])
    img = torch.full((_OK["H"], _OK["W"] + 1), FILL, dtype=torch.uint8, device="cuda")   # the buffer a legal call fills
    engine.timing_reset()
    engine.timing(1)
    try:
        with pytest.raises(FmcwError, match="E_ARG"):
            _render(engine, Q, kw["nq"], pmax, kw["nfft"], kw["fs"], t0, kw["dt"], kw["W"], kw["H"], img=img, **ptrs)
        assert engine.timing_read()["render"][1] == 0
    finally:
        engine.timing(0)
        engine.timing_reset()
    torch.cuda.synchronize()
    assert np.all(img.cpu().numpy() == FILL)


def test_render_stream_and_timing(engine):
    """A non-default torch stream, with timing stage `render`: one event pair for the one launch."""
    import torch
    case = RH.RENDER_CASES[0]
    nfft, fs, nq, nseg, W, H, kind = case
    Q, pmax, t0, dt, want, _ = RH.reference(case)
    s = torch.cuda.Stream()
    engine.timing_reset()
    engine.timing(1)
    try:
        with torch.cuda.stream(s):
            img = _render(engine, Q, nq, pmax, nfft, fs, t0, dt, W, H, stream=s)
        s.synchronize()
        ms, n = engine.timing_read()["render"]
        assert n == 1 and ms > 0
    finally:
        engine.timing(0)
        engine.timing_reset()
    _assert_picture(img, want)
