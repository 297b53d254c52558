"""GPU: the picture through fmcw_stft_png, exact, over every P layout stft_impl gathers its columns from.

The picture is given the library's own P, so no fp32 tolerance is needed: fmcw_stft_power_device (the
function stft_impl itself calls for the all-bins layouts; for the 20-tap window its kernel forms give the
same P and max(P) bits, tests/test_gpu_stft_mfma.py, tests/test_gpu_stft_gather.py, stft_coarse_max) runs on
the same float32 signal; bins 0 .. nq-1 and bin nb-1 of its P and its max(P) go through the restatement
(oracle/render.py), and the PNG's indices have to equal the result pixel for pixel.

Layouts: listed bins after the table-form max pass (nfft 1024 and 64), all bins from the 20-tap kernel,
all bins from the general kernel (a 24-tap window), listed bins after the coarse-to-fine max pass
(nfft 2^16).  Each also over three contexts on one device (segments sharded, the gather offset
s0 * (nq + 1), max(P) through the host): the same file, index for index.  The signal holds a stretch of exact
zeros, so whole segments have P = 0 and reach the picture's -1e30 floor from real input.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from oracle import render as R

pytestmark = pytest.mark.gpu

FMAX = 150.0
KAISER = ("kaiser", 20, 19)
HANN24 = ("hann", 24, 20)                 # not 20 taps: the general kernel, hop 4

# (L, nfft, n_log_bins, window, fs, W, H)
CONFIGS = [
    (900, 0, 1024, KAISER, 1250.0, 300, 120),       # listed bins, table max pass (nfft -> 1024)
    (900, 64, 1024, KAISER, 1250.0, 300, 17),       # listed bins at nfft 64; H not divisible by the strip count
    (900, 64, 0, KAISER, 200.0, 255, 97),           # all bins; seam and above-Nyquist rows end to end; nq = nb - 1
    (900, 256, 0, HANN24, 1250.0, 128, 1),          # general kernel, hop 4; H = 1 (one strip)
    (2000, 65536, 1024, KAISER, 1250.0, 400, 100),  # coarse-to-fine max pass; nq = 7866
]


def _id(cfg):
    L, nfft, nlog, (kind, wlen, nov), fs, W, H = cfg
    return f"L{L}-nfft{nfft}-log{nlog}-{kind}{wlen}-fs{fs:g}-{W}x{H}"


@functools.lru_cache(maxsize=None)
def _signal(L):
    """The slow-time signal of tests/test_gpu_render.py plus one stretch of 40 exact zeros, float32."""
    rng = np.random.default_rng(11)
    k = np.arange(L)
    x = np.abs(1.0 + 0.6 * np.sin(2 * np.pi * 37.0 * k / 1250.0) + 0.3 * np.sin(2 * np.pi * 90.0 * k / 1250.0)
               + 0.05 * rng.standard_normal(L)).astype(np.float32)
    if L >= 200:
        x[L // 3:L // 3 + 40] = 0.0
    x.setflags(write=False)
    return x


def _window(spec):
    kind, wlen, _ = spec
    return O.stft_window(kind, wlen).astype(np.float32)


@pytest.fixture(scope="module")
def multi():
    from fmcw_radar_processing_amd.engine import Engine
    e = Engine([0, 0, 0])
    yield e
    e.close()


def _library_q(engine, x, w, noverlap, nfft, fs, nseg, nq):
    """(Q [nseg][nq + 1], max(P)) of fmcw_stft_power_device on x: frame list [0], pn = L, max_seg = nseg."""
    import torch
    dev = "cuda"
    nb = nfft // 2 + 1
    d_x = torch.from_numpy(np.array(x, np.float32)).to(dev)
    d_list = torch.zeros(1, dtype=torch.int32, device=dev)
    d_len = torch.tensor([len(x)], dtype=torch.int64, device=dev)
    d_win = torch.from_numpy(np.array(w, np.float32)).to(dev)
    d_P = torch.full((nseg, nb), np.nan, dtype=torch.float32, device=dev)
    d_pmax = torch.zeros(1, dtype=torch.float32, device=dev)
    d_nseg = torch.full((1,), -1, dtype=torch.int64, device=dev)
    engine.stft_power_device(d_x, d_list, d_len, len(x), d_win, len(w), noverlap, nfft, fs, nseg, d_P, d_pmax, d_nseg,
                             stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert int(d_nseg.item()) == nseg
    Q = torch.cat([d_P[:, :nq], d_P[:, nb - 1:]], dim=1).cpu().numpy()     # sliced on the device: Q, not P, comes back
    return Q, np.float32(d_pmax.item())


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), what                                 # NaN and -Inf compare equal


def _check_outputs(got, ref, path):
    for k in ("time", "frequency", "intensity"):
        _same_bits(got[k], ref[k], k)
    assert got["nfft"] == ref["nfft"]
    assert got["png_bytes"] == path.stat().st_size


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_stft_png_is_the_restatement_of_the_library_p(engine, multi, tmp_path, cfg):
    L, nfft_arg, nlog, spec, fs, W, H = cfg
    _, wlen, noverlap = spec
    x, w = _signal(L), _window(spec)
    hop = wlen - noverlap
    one, three = tmp_path / "one.png", tmp_path / "three.png"
    got = engine.stft_png(x, w, noverlap, fs, str(one), nfft=nfft_arg, n_log_bins=nlog, width=W, height=H)
    nfft = got["nfft"]
    nseg = len(got["time"])
    nb = nfft // 2 + 1
    df = fs / nfft
    nq = min(nb - 1, int(np.floor(FMAX / df)) + 2)
    # the other outputs are those of fmcw_stft (whose listed-bins column remap differs: no picture columns)
    _check_outputs(got, engine.stft(x, w, noverlap, fs, nfft=nfft_arg, n_log_bins=nlog), one)
    idx, pal = R.read_png_indexed(str(one))
    assert idx.shape == (H, W)
    np.testing.assert_array_equal(pal, R.jet_palette_u8())
    # the picture: the restatement on the library's own P and max(P)
    Q, pmax = _library_q(engine, x, w, noverlap, nfft, fs, nseg, nq)
    assert np.any(np.all(Q == 0, axis=1)) and pmax > 0                      # whole segments on the floor
    want = R.render_indices(Q, nq, float(pmax), nfft, fs, (wlen / 2.0) / fs, hop / fs, W, H)
    assert len(np.unique(want)) > (3 if H == 1 else 20)
    bad = idx != want
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad.any(axis=1))[:8], np.flatnonzero(bad.any(axis=0))[:8])
    # three contexts on one device: shards gathered at s0 * (nq + 1), max(P) through the host
    got3 = multi.stft_png(x, w, noverlap, fs, str(three), nfft=nfft_arg, n_log_bins=nlog, width=W, height=H)
    _check_outputs(got3, got, three)
    idx3, pal3 = R.read_png_indexed(str(three))
    np.testing.assert_array_equal(idx3, idx)
    np.testing.assert_array_equal(pal3, pal)


def test_one_segment_is_an_empty_picture(engine, multi, tmp_path):
    """L = wlen: nseg 1, nothing to join: an all-zero picture in a valid PNG, and no error."""
    x, w = _signal(20), _window(KAISER)
    ref = engine.stft(x, w, 19, 1250.0)
    for k, e in enumerate((engine, multi)):                                 # three contexts: two sit the call out
        path = tmp_path / f"{k}.png"
        got = e.stft_png(x, w, 19, 1250.0, str(path), width=64, height=33)
        assert len(got["time"]) == 1
        _check_outputs(got, ref, path)
        idx, pal = R.read_png_indexed(str(path))
        assert idx.shape == (33, 64) and not idx.any()
        np.testing.assert_array_equal(pal, R.jet_palette_u8())


def test_zero_signal_is_an_empty_picture(engine, multi, tmp_path):
    """max(P) = 0: every vertex on the floor; intensity is that of fmcw_stft (0/0), bit for bit."""
    x, w = np.zeros(200, np.float32), _window(KAISER)
    ref = engine.stft(x, w, 19, 1250.0)
    for k, e in enumerate((engine, multi)):
        path = tmp_path / f"{k}.png"
        got = e.stft_png(x, w, 19, 1250.0, str(path), width=97, height=40)
        assert len(got["time"]) == 181
        _check_outputs(got, ref, path)
        idx, _ = R.read_png_indexed(str(path))
        assert idx.shape == (40, 97) and not idx.any()
