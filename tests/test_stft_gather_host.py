"""Host tests of tests/stft_gather_cases.py: the cases of tests/test_gpu_stft_gather.py meet the conditions
its assertions rest on, and the division-free gather of k_stft64f (`locate`: a double reciprocal per unit,
a float reciprocal per sample, one correction step each) is exact where its comment says so.  No GPU."""
import numpy as np
import pytest

from tests import stft_gather_cases as C
from tests import stft_reference as R

ALL = C.GRID + C.HANN + C.HALO + C.CLIP + C.CLIP_SPIKE


def test_coverage_of_the_grid():
    forms = {(c.form, c.nfft, c.hop) for c in C.GRID}
    assert forms == {("k_stft20", 64, 1), ("k_stft20", 64, 3), ("k_stft20", 100, 1), ("k_stft20", 100, 3),
                     ("k_stft_mfma", 100, 1), ("k_stft_mfma", 100, 3), ("k_stft64m", 64, 1), ("k_stft64m", 64, 3),
                     ("k_stft64f_hop1", 64, 1), ("k_stft64f", 64, 2), ("k_stft64f", 64, 3), ("k_stft64f", 64, 4)}
    assert len(C.GRID) == len(forms) * len(C.PNS) and set(C.PNS) == {1, 3, 7, 16, 19, 20, 21, 41, 47, 50, 277, 1000}
    assert {c.form for c in C.HANN} == set(C.FORMS) and all(c.win == "hann" for c in C.HANN)
    # the halo at hop 1 only (the API's rule), every form that runs hop 1
    assert all(c.hop == 1 for c in C.HALO)
    assert {(c.form, c.nfft) for c in C.HALO} == {(f, n) for f, n, h in forms if h == 1}
    assert {(c.pn, c.halo_len) for c in C.HALO} == {(p, h) for p in (16, 41, 256) for h in (0, 7, 19)}
    # the clip: every form at pn 41 and hop 1, and the general k_stft64f at hop 3
    assert {(c.form, c.nfft, c.hop) for c in C.CLIP} == {(f, n, h) for f, n, h in forms if h == 1} | {("k_stft64f", 64, 3)}
    assert all(c.pn == 41 for c in C.CLIP) and {c.max_seg for c in C.CLIP} == {1, 63, 64, 65, 255, 256, 257}
    assert {(c.form, c.hop) for c in C.CLIP_SPIKE} == {("k_stft64m", 1), ("k_stft64f_hop1", 1), ("k_stft64f", 3)}
    assert all(c.spike and c.max_seg % 64 == 1 and c._replace(spike=False, win="asym") in C.CLIP for c in C.CLIP_SPIKE)
    # each identity pair is two cases of the grid on the same input
    for a, b in C.IDENTITY:
        assert a in C.GRID and b in C.GRID and a[1:] == b[1:] and b.form == "k_stft20"
    assert len(C.IDENTITY) == 2 * 2 * len(C.PNS)
    # the environment switches select the forms as kernels_stft.hip's stft_form does
    assert C.FORMS["k_stft20"][0] == "0" and all(C.FORMS[f][0] == "1" for f in C.FORMS if f != "k_stft20")
    assert C.FORMS["k_stft64m"][1] == "0" and C.FORMS["k_stft64f"][1] == C.FORMS["k_stft64f_hop1"][1] == "1"


@pytest.mark.parametrize("c", ALL, ids=C.case_id)
def test_cases_meet_their_conditions(c):
    i = C.case_inputs(c)
    pn, hop = c.pn, c.hop
    assert i.L == C.signal_length(c) == 600 * hop + 19 + pn // 2 and i.nl == -(-i.L // pn)
    assert i.slow.shape == (i.nl + 3, pn) and len(i.flist) == i.nl and len(i.x) == i.L
    # a partial last frame; vacuous at pn 1, and at hop 4 the length 2422 happens to be 346 frames of 7
    assert (i.L % pn != 0) == (pn != 1 and (hop, pn) != (4, 7))
    # the list: not sorted, a row listed twice (where it has three entries), the last row once, rows left out
    fl = i.flist
    assert np.any(np.diff(fl) < 0) and 0 <= fl.min() and fl.max() < i.nl + 3
    assert len(set(fl)) == (i.nl - 1 if i.nl >= 3 else i.nl)
    assert np.count_nonzero(fl == fl[-1]) == 1
    assert i.nl + 3 - len(set(fl)) >= 3
    # the signal is what the list reads, and NaN lies exactly where no listed sample below L does
    q = np.arange(i.L)
    np.testing.assert_array_equal(i.slow[fl[q // pn], q % pn], i.x)
    touched = np.zeros(i.slow.shape, bool)
    touched[fl[q // pn], q % pn] = True
    np.testing.assert_array_equal(np.isnan(i.slow), ~touched)
    assert not np.isnan(i.x).any()
    # levels: the frames differ by up to 5x, so a wrong frame moves the map by far more than the bar
    lev = [float(np.mean(i.x[j * pn:(j + 1) * pn])) for j in range(min(i.nl, 5))] if pn >= 16 else None
    assert lev is None or i.nl < 2 or max(lev) > 1.5 * min(lev)
    if c.halo_len is not None:
        assert len(i.halo) == C.N_HALO == 19
        np.testing.assert_array_equal(np.isnan(i.halo), np.arange(19) >= c.halo_len)
        assert len(i.xh) == i.L + c.halo_len
    else:
        assert i.halo is None and i.xh is i.x
    # the reference map: enough segments, and at least half of it carries the bar
    Pr, db = C.reference(c)
    n = Pr.shape[0]
    assert n == R.nseg_of(len(i.xh), 20, 20 - hop) >= 600
    assert (db >= C.FLOOR).mean() >= 0.5
    if c.max_seg is not None:
        m = c.max_seg
        assert m < n
        assert Pr[:m].max() < 0.1 * Pr.max()                            # the maximum lies in clipped segments only
        assert Pr[m].max() > 10 * Pr[:m].max() or Pr[m:m + 20].max() > 10 * Pr[:m].max()
        # some of them inside the clipped 64-segment unit and 256-segment tile (where more than one segment
        # of the unit is clipped: the first clipped segment holds few of the larger samples)
        assert m % 64 in (0, 63) or Pr[m:-(-m // 64) * 64].max() > 10 * Pr[:m].max()
        assert (R.psd_db(Pr[:m]) >= C.FLOOR).mean() >= 0.5
        # the unboosted samples are the unclipped case's: the kept rows read nothing that changed
        base = C.case_inputs(c._replace(max_seg=None))
        keep = (m - 1) * hop + 20
        np.testing.assert_array_equal(i.x[:keep - c.spike], base.x[:keep - c.spike])
        if c.spike:
            # a maximum that takes in the segments behind max_seg of the clipped unit is at least twice too large
            assert C.zero_filled_unit_power(c).max() > 2 * Pr[:m].max()


# ---------------------------------------------------------------------------------------------------
# k_stft64f's `locate`
# ---------------------------------------------------------------------------------------------------
LOCATE_PN = list(range(1, 2049)) + [65535, 65536, 2 ** 24 - 277, 2 ** 24 + 5]


def test_float_quotient_is_exact_after_one_correction():
    """(r0 + i) / pn from the float32 reciprocal: quotient and remainder equal divmod after one correction
    step, for r0 at both ends and in the middle of a frame and every i a unit can hold (0..275)."""
    needs = []
    i = np.arange(276)[None, :]
    for pn in LOCATE_PN:
        r0 = np.array([0, min(1, pn - 1), pn // 2, pn - 1])[:, None]
        df, d, fixed = C.locate_f32(pn, r0, i)
        Q, Rm = np.divmod(r0 + i, pn)
        np.testing.assert_array_equal(df, Q, err_msg=str(pn))
        np.testing.assert_array_equal(d, Rm, err_msg=str(pn))
        if fixed.any():
            needs.append(pn)
    # the step is taken: 41 and 47 are the two smallest pn that need it (none of 1, 3, 7, 16, 19, 20, 21, 50,
    # 128, 256, 277, 1000 does), 137 values up to 1024
    assert needs[:5] == [41, 47, 55, 61, 82]
    assert sum(p <= 1024 for p in needs) == 137
    assert not set(needs) & {1, 3, 7, 16, 19, 20, 21, 50, 128, 256, 277, 1000}


@pytest.mark.parametrize("c", [c for c in ALL if c.form.startswith("k_stft64f")], ids=C.case_id)
def test_float_quotient_on_the_units_of_the_grid(c):
    """On the units k_stft64f forms on the case's own signal (r0 = 64 u hop mod pn): exact, and at pn 41
    and 47 the correction step is what makes it so."""
    r0, ns = C.units_of(c)
    assert ns <= 276 and len(r0) >= 10
    i = np.arange(ns)[None, :]
    df, d, fixed = C.locate_f32(c.pn, r0[:, None], i)
    Q, Rm = np.divmod(r0[:, None] + i, c.pn)
    np.testing.assert_array_equal(df, Q)
    np.testing.assert_array_equal(d, Rm)
    assert fixed.any() == (c.pn in (41, 47))


def test_double_quotient_is_exact_after_one_correction():
    """q0 / pn from the double reciprocal for q0 up to 2^40: multiples of pn, their neighbours, and random."""
    rng = np.random.default_rng(5)
    top = 2 ** 40
    for pn in LOCATE_PN:
        k = rng.integers(0, top // pn, 400)
        q0 = np.concatenate([k * pn, k * pn + pn - 1, np.maximum(k * pn - 1, 0), rng.integers(0, top, 400),
                             [0, 1, pn - 1, pn, top - 1, top, (top // pn) * pn]])
        fq, r, _ = C.locate_f64(pn, q0)
        Q, Rm = np.divmod(q0, pn)
        np.testing.assert_array_equal(fq, Q, err_msg=str(pn))
        np.testing.assert_array_equal(r, Rm, err_msg=str(pn))
