"""The five kernel forms of the 20-tap STFT (k_stft20, k_stft_mfma, k_stft64m, k_stft64f at hop 1 and at
hop 2..4) over what each of them writes for itself: the gather through the frame list and the max_seg
clip; and k_compact, which makes that list, against its definition.

Every other 20-tap test passes frame_list = arange(n) at pn 256 (the gather is the identity and every
tile and unit starts on a frame boundary) or an ascending list through the default form only, and none
clips a 20-tap call.  Here the list is not sorted and repeats a row, pn runs from 1 (a segment spans 20
frames) over 41 and 47 (where k_stft64f's float quotient takes its correction step) to 1000, every
unlisted sample is NaN, and the reference is the float64 direct DFT of tests/stft_reference.py on the
flat signal.  The cases and inputs are tests/stft_gather_cases.py; tests/test_stft_gather_host.py proves
their conditions on the CPU.

The bar is TOL_FP32_DB: |dB error| <= 1e-3 where the float64 map is >= -80 dB; below the
floor an output only has to stay below it.
"""
import numpy as np
import pytest

from fmcw_radar_processing_amd import params as P
from tests import stft_gather_cases as C
from tests.helpers import TOL_FP32_DB, case
from tests.test_gpu_stft_general import _assert_db_bar, _db, _power

pytestmark = pytest.mark.gpu

FOLD_MAX_REL = 2e-6       # k_stft64f's max(P): the bar of test_folded_stft64_meets_the_db_bar


def _run(engine, monkeypatch, c, max_seg=None, db_pmax=None):
    """Both passes of case c: the stored pass (P, max(P), nseg), then the max-only pass (`pmax1`, `n1`)
    followed by the direct dB pass into a NaN-filled map of the same padded shape (`db`).  db_pmax: the
    maximum the direct dB pass is given instead of its own max-only pass's."""
    import torch
    mfma, fold = C.FORMS[c.form][:2]
    monkeypatch.setenv("FMCW_STFT_MFMA", mfma)
    monkeypatch.setenv("FMCW_STFT64_FOLD", fold)
    i = C.case_inputs(c)
    kw = dict(L=i.L, slow=i.slow, flist=i.flist, pn=c.pn, halo=None if i.halo is None else i.halo.copy(),   # read-only
              halo_len=c.halo_len, max_seg=max_seg)
    nov = C.WLEN - c.hop
    st = _power(engine, i.x, i.w, nov, c.nfft, store=True, **kw)
    mo = _power(engine, i.x, i.w, nov, c.nfft, store=False, **kw)
    assert np.isnan(mo["P"]).all()
    t = mo["t"]
    if db_pmax is not None:
        t["pmax"].copy_(torch.tensor([db_pmax], dtype=torch.float32))
    out = torch.full_like(t["P"], np.nan)
    engine.stft_db_direct_device(t["slow"], t["flist"], t["len"], c.pn, t["win"], C.WLEN, nov, c.nfft, C.FS, mo["max_seg"],
                                 t["pmax"], out, d_halo=t["halo"], n_halo=0 if i.halo is None else len(i.halo),
                                 d_halo_len=t["halo_len"])
    torch.cuda.synchronize()
    return dict(n=st["n"], P=st["P"], pmax=st["pmax"], n1=mo["n"], pmax1=mo["pmax"], db=out.cpu().numpy())


_GPU = {}


def _case(engine, monkeypatch, c):
    """An unclipped case, run once and shared with the bit-identity tests (which only read it)."""
    if c not in _GPU:
        _GPU[c] = _run(engine, monkeypatch, c)
    return _GPU[c]


def _check_parity(c, r):
    Pr, ref_db = C.reference(c)
    n = Pr.shape[0]
    what = C.case_id(c)
    assert r["n"] == n and r["n1"] == n, what
    assert n >= C.NSEG_MIN
    # the stored pass
    got = r["P"][:n]
    assert not np.isnan(got).any(), what                                # no unlisted sample, no sample past L
    assert np.isnan(r["P"][n:]).all(), what                             # rows from nseg on untouched
    _assert_db_bar(_db(got, r["pmax"]), ref_db, f"{what} P")
    # the max-only pass and the direct dB pass
    d = r["db"][:n]
    assert np.isnan(r["db"][n:]).all(), what
    _assert_db_bar(d.astype(np.float64), ref_db, f"{what} dB")
    for pm in (r["pmax"], r["pmax1"]):
        e = abs(float(_db(pm, Pr.max())))
        print(f"STFT_ERR {what}: |dB err| of max(P) {e:.3e}")
        assert e <= TOL_FP32_DB, what


@pytest.mark.parametrize("c", C.GRID, ids=C.case_id)
def test_gather_through_an_unsorted_list(engine, monkeypatch, c):
    """pn from 1 to 1000, a partial last frame, a list that is a permutation with one row listed twice."""
    _check_parity(c, _case(engine, monkeypatch, c))


@pytest.mark.parametrize("c", C.HANN, ids=C.case_id)
def test_gather_with_the_hann_window(engine, monkeypatch, c):
    _check_parity(c, _case(engine, monkeypatch, c))


@pytest.mark.parametrize("c", C.HALO, ids=C.case_id)
def test_gather_into_the_halo(engine, monkeypatch, c):
    """A 19-sample halo buffer of which the device-held length says 0, 7 or 19 are valid (the rest NaN)."""
    _check_parity(c, _case(engine, monkeypatch, c))


@pytest.mark.parametrize("a,b", C.IDENTITY, ids=lambda c: C.case_id(c))
def test_table_forms_are_bit_identical_on_a_gathered_input(engine, monkeypatch, a, b):
    """k_stft_mfma (nfft 100) and k_stft64m (nfft 64) against k_stft20: the same k-ordered chain of fmas,
    so the same bits whatever the list; NaN rows compare equal."""
    ra, rb = _case(engine, monkeypatch, a), _case(engine, monkeypatch, b)
    assert ra["n"] == rb["n"] and ra["n1"] == rb["n1"]
    np.testing.assert_array_equal(ra["P"], rb["P"])
    np.testing.assert_array_equal(ra["db"], rb["db"])
    assert ra["pmax"].tobytes() == rb["pmax"].tobytes() and ra["pmax1"].tobytes() == rb["pmax1"].tobytes()


@pytest.mark.parametrize("c", C.CLIP + C.CLIP_SPIKE, ids=C.case_id)
def test_clip_at_max_seg(engine, monkeypatch, c):
    """max_seg below the segment count, the input ten times larger from the first clipped segment's last
    sample on: nseg, the kept rows, nothing behind them, and a maximum that saw no clipped segment (one
    that did is off by up to 20 dB).  The nfft-64 forms zero-fill behind the last kept segment's samples, so the
    segments of the clipped unit behind max_seg never see those larger samples: in the spike cases the last
    kept sample is 300 under the Hann window, which the last kept segment sees at tap 19 (0.02) and the
    zero-filled segments at the window's middle, so a maximum taken before the `sl < ns` test is caught."""
    m = c.max_seg
    r = _run(engine, monkeypatch, c, max_seg=m)
    full = _run(engine, monkeypatch, c, db_pmax=r["pmax1"])
    what = C.case_id(c)
    assert m < full["n"] == C.reference(c)[0].shape[0]
    assert r["n"] == m and r["n1"] == m, what
    for k in ("P", "db"):
        assert not np.isnan(r[k][:m]).any(), (what, k)
        np.testing.assert_array_equal(r[k][:m], full[k][:m], err_msg=f"{what} {k}")    # bit for bit the unclipped rows
        assert np.isnan(r[k][m:]).all(), (what, k)                                       # nothing past them
    kept = r["P"][:m].max()
    assert full["pmax"] >= 10 * kept                                     # the clipped segments hold the call's maximum
    for pm in (r["pmax"], r["pmax1"]):
        print(f"STFT_ERR {what}: max(P) / max of the kept rows - 1 = {float(pm) / float(kept) - 1:.3e}")
        if c.form.startswith("k_stft64f"):
            assert abs(float(pm) / float(kept) - 1) <= FOLD_MAX_REL, what
        else:
            assert pm == kept, what


# ---------------------------------------------------------------------------------------------------
# k_compact against its definition
# ---------------------------------------------------------------------------------------------------
COMPACT_F = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 5000)
COMPACT_PATTERNS = ("zero", "positive", "alternating", "first", "last", "sparse", "dense")
POSITIVE = np.array([1, 3, 2 ** 31 - 1], np.int32)
NOT_POSITIVE = np.array([-1, 0], np.int32)
SENTINEL = -7
_TAPS = {}


def _counts(pattern, F, rng):
    pos = rng.choice(POSITIVE, F)
    neg = rng.choice(NOT_POSITIVE, F)
    if pattern == "zero":
        return np.zeros(F, np.int32)
    if pattern == "positive":
        return pos
    on = {"alternating": np.arange(F) % 2 == 1,
          "first": np.arange(F) == 0,
          "last": np.arange(F) == F - 1,
          "sparse": rng.random(F) < 0.1,
          "dense": rng.random(F) < 0.9}[pattern]
    return np.where(on, pos, neg).astype(np.int32)


@pytest.mark.parametrize("F", COMPACT_F)
@pytest.mark.parametrize("pn", [16, 256])
def test_compact_is_nonzero_of_the_counts(engine, pn, F):
    """Engine.compact_device on counts the test writes (no frame is processed): the list is
    np.nonzero(count > 0), the entries behind it keep their sentinel, *d_len = n pn.  1024 frames per pass:
    one pass, a full pass and one frame, two passes, a partial fifth.  The two counts behind F are
    positive, so a read past F shows as a listed frame."""
    import torch
    if _TAPS.get("pn") != pn:                              # the taps of each geometry once (pn outermost)
        cfg, _, wr, wd, cal = case(64, 16, 256, 16) if pn == 16 else case(1024, 256, 1024, 256, P.THROUGHPUT)
        assert cfg.pn == pn
        engine.set_taps(cfg, cal, wr, wd)
        _TAPS["pn"] = pn
    rng = np.random.default_rng(1000 * pn + F)
    for pattern in COMPACT_PATTERNS:
        count = np.concatenate([_counts(pattern, F, rng), POSITIVE[:2]])
        want = np.nonzero(count[:F] > 0)[0]
        d_count = torch.from_numpy(count).to("cuda")
        d_list = torch.full((F + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        engine.compact_device(d_count, F, d_list, d_len)
        torch.cuda.synchronize()
        got = d_list.cpu().numpy()
        n = len(want)
        np.testing.assert_array_equal(got[:n], want, err_msg=pattern)
        assert (got[n:] == SENTINEL).all(), pattern
        assert int(d_len.item()) == n * pn, pattern
