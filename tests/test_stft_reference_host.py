"""tests/stft_reference.py (the direct-DFT float64 reference the GPU STFT tests compare with) pinned
against the oracle's FFT-based spectrogram on the CPU: asymmetric windows, no overlap, a one-tap window,
nfft = wlen, non-power-of-two nfft, few log bins, and the impulse known answer."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import stft_reference as R

FS = 1250.0

# (wlen, noverlap, nfft, L)
SHAPES = [(1, 0, 2, 50), (2, 1, 2, 40), (5, 3, 6, 60), (20, 19, 22, 90), (20, 15, 64, 200), (32, 0, 32, 700),
          (64, 0, 100, 1000), (128, 121, 300, 600), (256, 128, 1000, 900), (24, 12, 2048, 150)]


def _close_power(got, want):
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * want.max())


@pytest.mark.parametrize("wlen,noverlap,nfft,L", SHAPES)
def test_power_matches_the_oracle_fft(wlen, noverlap, nfft, L):
    x = R.magnitude_signal(L, wlen).astype(np.float64)
    w = R.asym_window(wlen, wlen)
    assert wlen < 3 or not np.array_equal(w, w[::-1])
    P = R.stft_power(x, w, noverlap, nfft, FS)
    _, Fv, T, Po = O.spectrogram(x, w.astype(np.float64), noverlap, nfft, FS)
    assert P.shape[0] == R.nseg_of(L, wlen, noverlap) == Po.shape[1]
    _close_power(P, Po.T)
    np.testing.assert_allclose(R.seg_times(P.shape[0], wlen, noverlap, FS), T, rtol=1e-14)
    np.testing.assert_allclose(R.lin_freqs(nfft, FS), Fv, rtol=1e-14)
    db, dbo = R.psd_db(P), O.psd_db(Po).T
    sel = dbo > -200
    assert sel.mean() > 0.9
    np.testing.assert_allclose(db[sel], dbo[sel], rtol=0, atol=1e-8)


def test_float32_taps_are_what_the_reference_uses():
    """The device receives float32 taps: a float64 window is rounded first, so the reference of kaiser(20, 3)
    is the spectrogram of its float32 rounding, not of the float64 taps."""
    x = R.magnitude_signal(300, 1).astype(np.float64)
    w = O.stft_window("kaiser")
    w32 = w.astype(np.float32).astype(np.float64)
    assert not np.array_equal(w, w32)
    _close_power(R.stft_power(x, w, 19, 64, FS), O.spectrogram(x, w32, 19, 64, FS)[3].T)


@pytest.mark.parametrize("L,wlen,noverlap,want", [(0, 20, 19, 0), (19, 20, 19, 0), (20, 20, 19, 1), (31, 32, 0, 0),
                                                  (95, 32, 0, 2), (96, 32, 0, 3), (10, 20, 15, 0), (700, 256, 192, 7),
                                                  (1, 1, 0, 1)])
def test_segment_count(L, wlen, noverlap, want):
    assert R.nseg_of(L, wlen, noverlap) == want
    assert R.stft_power(np.ones(L), np.ones(wlen), noverlap, 256, FS).shape == (want, 129)


@pytest.mark.parametrize("wlen,noverlap,nfft,L,pos", [(256, 192, 300, 900, 400), (7, 2, 8, 60, 21)])
def test_impulse_known_answer(wlen, noverlap, nfft, L, pos):
    """x = delta at pos: |S| = w[pos - seg hop] at every bin, so P is flat over the bins of a segment that
    holds the sample and exactly 0 elsewhere; a reversed tap index gives w[wlen-1-m] instead."""
    w = R.asym_window(wlen, 3)
    x = np.zeros(L)
    x[pos] = 1.0
    P = R.stft_power(x, w, noverlap, nfft, FS)
    K = R.impulse_power(L, pos, w, noverlap, nfft, FS)
    hit = K[:, 0] > 0
    hop = wlen - noverlap
    assert hit.sum() == len([s for s in range(K.shape[0]) if 0 <= pos - s * hop < wlen]) >= 2 and not hit.all()
    assert np.all(P[~hit] == 0)
    np.testing.assert_allclose(P[hit], K[hit], rtol=1e-12)
    _close_power(K, O.spectrogram(x, R.taps(w), noverlap, nfft, FS)[3].T)
    # the reversed window is a different answer at this bar
    Krev = R.impulse_power(L, pos, w[::-1].copy(), noverlap, nfft, FS)
    assert np.abs(10 * np.log10(Krev[hit] / K[hit])).max() > 1.0
    assert np.all(np.isneginf(R.psd_db(P)[~hit]))


@pytest.mark.parametrize("nlog", [1, 2, 7])
@pytest.mark.parametrize("wlen,noverlap,nfft,L", [(1, 0, 2, 50), (5, 3, 6, 60), (64, 0, 100, 1000), (128, 121, 300, 600)])
def test_pipeline_matches_the_oracle(wlen, noverlap, nfft, L, nlog):
    x = R.magnitude_signal(L, nfft).astype(np.float64)
    w = R.asym_window(wlen, nfft)
    got = R.pipeline(x, w, noverlap, nfft, FS, nlog)
    ref = O.spectrogram_pipeline(x, 1 / FS, R.taps(w), noverlap, nfft=nfft, nbins=nlog)
    np.testing.assert_allclose(got["time"], ref["time"], rtol=1e-14)
    np.testing.assert_allclose(got["frequency"], ref["frequency"], rtol=1e-12)
    assert got["intensity"].shape == ref["intensity"].T.shape == (R.nseg_of(L, wlen, noverlap), nlog)
    np.testing.assert_allclose(got["intensity"], ref["intensity"].T, rtol=0, atol=1e-7)
    assert got["frequency"][-1] == pytest.approx(FS / 2, rel=1e-14)       # one log bin: the end point (MATLAB)
    # the same resampling through the oracle's interp1 from this reference's own dB map
    np.testing.assert_allclose(O.log_resample(R.lin_freqs(nfft, FS), got["psd"].T, got["frequency"]).T, got["intensity"],
                               rtol=0, atol=1e-7)


def test_pipeline_linear_bins_and_1024_log_bins():
    x = R.magnitude_signal(400, 9).astype(np.float64)
    w = R.asym_window(33, 9)
    for nlog in (0, 1024):
        got = R.pipeline(x, w, 20, 300, FS, nlog)
        ref = O.spectrogram_pipeline(x, 1 / FS, R.taps(w), 20, nfft=300, nbins=nlog)
        np.testing.assert_allclose(got["frequency"], ref["frequency"], rtol=1e-12)
        np.testing.assert_allclose(got["intensity"], ref["intensity"].T, rtol=0, atol=1e-7)
