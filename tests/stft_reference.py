"""float64 reference of the STFT stages (include/fmcw.h: fmcw_stft_power_device, fmcw_stft_db_device,
fmcw_stft), written from their definition; test-side code (the library's kernels are
csrc/kernels_stft.hip).  No FFT call in here: every bin is the direct DFT sum.

  hop = wlen - noverlap,  nseg = fix((L - noverlap) / hop)  (0 when L < wlen),  nb = nfft / 2 + 1
  S[seg][bin] = sum_m x[seg hop + m] w[m] e^{-2 pi i ((bin m) mod nfft) / nfft}
  P[seg][bin] = k |S|^2 / (fs sum(w^2)),  k = 1 at DC and Nyquist (2 bin == nfft), else 2   ('psd')
  psd = 20 log10(P / max(P))                       (of the power, as radar_processing.m:283; P = 0: -Inf)
  log bins: MATLAB's logspace(log10(fs / nfft), log10(fs / 2), n) (n = 1: its end point, fs / 2), each
  located on F = bin fs / nfft at i0 = clip(floor(fq / df), 0, nb - 2) and interpolated (extrapolated
  past the ends) linearly between the dB values of bins i0 and i0 + 1.

The window is what the device receives: float32 taps, widened to float64.  Arrays are [seg][bin], the
device layout (the oracle's are bins x segments).
"""
from __future__ import annotations

import numpy as np


def magnitude_signal(L: int, seed: int = 0) -> np.ndarray:
    """|N(0,1) + 3 sin(0.3 n)| as float32: the slow-time magnitude signal of test_stft_matches_oracle."""
    rng = np.random.default_rng(seed)
    return np.abs(rng.standard_normal(L) + 3 * np.sin(np.arange(L) * 0.3)).astype(np.float32)


def asym_window(wlen: int, seed: int = 0) -> np.ndarray:
    """Random taps in [0.1, 1): no symmetry, so a reversed tap index cannot pass."""
    return np.random.default_rng(1000 + seed).uniform(0.1, 1.0, wlen).astype(np.float32)


def taps(win) -> np.ndarray:
    """The window as the device sees it: rounded to float32, then exact in float64."""
    return np.asarray(win, np.float64).astype(np.float32).astype(np.float64)


def nseg_of(L: int, wlen: int, noverlap: int) -> int:
    return (L - noverlap) // (wlen - noverlap) if L >= wlen else 0


def one_sided_k(nfft: int) -> np.ndarray:
    k = np.full(nfft // 2 + 1, 2.0)
    k[0] = 1.0
    if nfft % 2 == 0:
        k[-1] = 1.0
    return k


def stft_power(x, win, noverlap: int, nfft: int, fs: float) -> np.ndarray:
    """P [nseg][nfft/2+1] in float64."""
    x = np.asarray(x, np.float64).reshape(-1)
    w = taps(win)
    wlen = len(w)
    hop = wlen - noverlap
    ns = nseg_of(len(x), wlen, noverlap)
    nb = nfft // 2 + 1
    if ns == 0:
        return np.zeros((0, nb))
    seg = x[np.arange(ns)[:, None] * hop + np.arange(wlen)[None, :]] * w[None, :]        # [seg][m]
    ph = ((np.arange(nb, dtype=np.int64)[:, None] * np.arange(wlen, dtype=np.int64)[None, :]) % nfft) / float(nfft)
    re = seg @ np.cos(2 * np.pi * ph).T                                                   # [seg][bin]
    im = -(seg @ np.sin(2 * np.pi * ph).T)
    return (re * re + im * im) * one_sided_k(nfft)[None, :] / (fs * np.sum(w * w))


def impulse_power(L: int, pos: int, win, noverlap: int, nfft: int, fs: float) -> np.ndarray:
    """The known answer for x = 0 but x[pos] = 1: every bin of segment seg is k w[pos - seg hop]^2 /
    (fs sum(w^2)), and exactly 0 in the segments that do not hold the sample."""
    w = taps(win)
    wlen = len(w)
    hop = wlen - noverlap
    ns = nseg_of(L, wlen, noverlap)
    P = np.zeros((ns, nfft // 2 + 1))
    for s in range(ns):
        m = pos - s * hop
        if 0 <= m < wlen:
            P[s] = one_sided_k(nfft) * (w[m] * w[m] / (fs * np.sum(w * w)))
    return P


def psd_db(P, pmax=None) -> np.ndarray:
    """20 log10(P / max(P)) in float64; -Inf where P is 0 (and everywhere when the maximum is 0)."""
    P = np.asarray(P, np.float64)
    pm = float(P.max(initial=0.0) if pmax is None else pmax)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20 * np.log10(P / pm) if pm > 0 else np.full(P.shape, -np.inf)


def seg_times(ns: int, wlen: int, noverlap: int, fs: float) -> np.ndarray:
    return (np.arange(ns) * (wlen - noverlap) + wlen / 2) / fs


def lin_freqs(nfft: int, fs: float) -> np.ndarray:
    return np.arange(nfft // 2 + 1) * fs / nfft


def log_freqs(nfft: int, fs: float, n: int) -> np.ndarray:
    """MATLAB logspace(log10(fs/nfft), log10(fs/2), n): the last point is the end point itself."""
    a, b = np.log10(fs / nfft), np.log10((nfft // 2) * fs / nfft)
    e = np.array([b if j == n - 1 else a + j * (b - a) / (n - 1) for j in range(n)])
    return 10.0 ** e


def log_resample(db, nfft: int, fs: float, n: int):
    """db [seg][nb] onto the n log bins.  Returns (out [seg][n], i0 [n]): i0 and i0 + 1 are the two
    source bins of every output."""
    db = np.asarray(db, np.float64)
    nb = nfft // 2 + 1
    df = fs / nfft
    fq = log_freqs(nfft, fs, n)
    i0 = np.clip(np.floor(fq / df).astype(np.int64), 0, nb - 2)
    wt = (fq - i0 * df) / df
    with np.errstate(invalid="ignore"):
        out = db[:, i0] + wt[None, :] * (db[:, i0 + 1] - db[:, i0])
    return out, i0


def pipeline(x, win, noverlap: int, nfft: int, fs: float, n_log_bins: int = 0) -> dict:
    """What fmcw_stft returns: time [nseg], frequency, intensity [nseg][nbins], plus the linear-bin dB
    map `psd` and, with log bins, `i0`."""
    w = taps(win)
    P = stft_power(x, w, noverlap, nfft, fs)
    psd = psd_db(P)
    out = dict(time=seg_times(P.shape[0], len(w), noverlap, fs), frequency=lin_freqs(nfft, fs), intensity=psd,
               psd=psd, P=P, nfft=nfft)
    if n_log_bins:
        out["intensity"], out["i0"] = log_resample(psd, nfft, fs, n_log_bins)
        out["frequency"] = log_freqs(nfft, fs, n_log_bins)
    return out
