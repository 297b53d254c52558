"""The streams schedule (K1 k_range, K2 k_doppler, K3 k_detect of csrc/kernels_frame.hip) over its size
and storage grid, against the float64 oracle and the storage-emulating chain of tests/streams_reference.py.

  sizes      every Nr of 16..2048 and every Nd of 2..1024 through Engine.process with FMCW_PIPE_STREAMS
             forced, c64, at the assertions of test_gpu_parity.test_process_matches_oracle, plus one white
             frame per case held element-wise
  storage    process_device with every (in, out, requested buffers) combination: every (cube, rd) storage
             pair of K1, K2 and K3, each output held to 2 e_ref + the fp32 bar
  pair       FMCW_PAIR=1 bit-identical to the default path
  K1         range_fft_device over its profile paths and storage pairs

Each measured figure is printed before it is asserted (pytest -s shows them; DESIGN.md 5.7 records them).
"""
import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
from fmcw_radar_processing_amd._lib import FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS
from tests import streams_reference as SR
from tests.helpers import TOL_FP16_REL_L2, TOL_FP32_REL_L2, rd_rel_err, rel_l2
from tests.streams_reference import STORAGE

pytestmark = pytest.mark.gpu

assert (SR.C64, SR.C32H) == (FMCW_C64, FMCW_C32H)
# the grid's coverage, asserted where the cases are used (tests/test_streams_reference_host.py restates it)
assert {g[2] for g in SR.SIZE_CASES} == set(SR.ALL_NR) and {g[3] for g in SR.SIZE_CASES} == set(SR.ALL_ND)
_RUNS = SR.SIZE_CASES + SR.STORAGE_CASES + SR.PAIR_CASES
assert all([g[2] for g in _RUNS].count(n) >= 2 for n in SR.NEW_NR)
assert all([g[3] for g in _RUNS].count(n) >= 2 for n in SR.NEW_ND)

DT = {FMCW_C64: "c64", FMCW_C32H: "c32h"}
WANTS = [(False, False), (False, True), (True, False), (True, True)]          # (d_cube, d_rd)
# (cube, rd) storage of K1/K2/K3 for a combination: the scratch buffers are c64
assert {(o if c else FMCW_C64, o if r else FMCW_C64) for o in DT for c, r in WANTS} == set(STORAGE)


@pytest.fixture
def streams(engine):
    engine.set_pipeline(FMCW_PIPE_STREAMS)
    try:
        yield engine
    finally:
        engine.set_chunk_frames(0)
        engine.set_pipeline(FMCW_PIPE_AUTO)


def _taps(engine, r):
    engine.set_taps(r.cfg, r.cal, r.wr, r.wd)


# ---------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------
def _process(engine, r):
    return engine.process(r.dev_iq, want_cube=True, want_rd=True, probe_column=r.probe_column)


@pytest.mark.parametrize("g", SR.SIZE_CASES, ids=SR.case_id)
def test_sizes_match_oracle(streams, g):
    r = SR.ref(g, FMCW_C64, "noise")
    ref, cfg = r.plain, r.cfg
    _taps(streams, r)
    got = _process(streams, r)
    e_cube = rel_l2(got["cube"], ref["cube"], axis=(1, 2)).max()
    e_rd = rd_rel_err(got["rd"], ref["rd"], ref["cube"], r.wd, cfg.nd).max()
    e_prof = rel_l2(got["profile"], ref["profile"], axis=1).max()
    # the white frame, element-wise: max |got - ref| / rms(ref)
    n = r.noise
    m_cube = np.abs(got["cube"][n] - ref["cube"][n]).max() / np.sqrt(np.mean(np.abs(ref["cube"][n]) ** 2))
    m_rd = np.abs(got["rd"][n] - ref["rd"][n]).max() / np.sqrt(np.mean(np.abs(ref["rd"][n]) ** 2))
    print(f"\nGRID sizes {SR.case_id(g)} cube {e_cube:.2e} rd {e_rd:.2e} profile {e_prof:.2e} "
          f"white: cube {m_cube:.2e} rd {m_rd:.2e}")
    assert e_cube <= TOL_FP32_REL_L2
    assert e_rd <= TOL_FP32_REL_L2
    assert e_prof <= TOL_FP32_REL_L2
    assert m_cube <= TOL_FP32_REL_L2
    assert m_rd <= TOL_FP32_REL_L2
    # detections: exact, no frame left out (the near-tie mask is empty)
    assert not SR.near_ties(r).any()
    np.testing.assert_array_equal(got["tgt_count"], ref["tgt_count"])
    np.testing.assert_array_equal(got["tgt_range_idx"], ref["tgt_range_idx"])
    np.testing.assert_array_equal(got["tgt_doppler_idx"], ref["tgt_doppler_idx"])
    np.testing.assert_allclose(got["tgt_range_mag"], ref["tgt_range_mag"], rtol=1e-5, atol=0)
    has = ref["tgt_count"] > 0
    assert has.any() and (~has).any()
    assert rel_l2(got["slow_mag"][has], ref["slow_mag"][has], axis=1).max() <= TOL_FP32_REL_L2
    assert np.all(got["slow_mag"][~has] == 0)
    assert rel_l2(got["probe_mag"], ref["probe"]) <= TOL_FP32_REL_L2


@pytest.mark.parametrize("g", [SR.SIZE_CASES[2], SR.SIZE_CASES[6]], ids=SR.case_id)
def test_chunks_of_two_frames_change_no_bit(streams, g):
    """The three-slot chunk pipeline at small sizes (odd pn, and an odd number of chunks)."""
    r = SR.ref(g, FMCW_C64, "noise")
    _taps(streams, r)
    a = _process(streams, r)
    streams.set_chunk_frames(2)
    b = _process(streams, r)
    assert r.F > 4 and set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---------------------------------------------------------------------------
# storage grid through process_device
# ---------------------------------------------------------------------------
def _to_device(r, in_dtype):
    import torch
    a = r.dev_iq if in_dtype == FMCW_C32H else np.ascontiguousarray(r.dev_iq).view(np.float32).reshape(r.dev_iq.shape + (2,))
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _complex(t, scale):
    """A device buffer [..][2] of float32 or float16 as complex128, stored halves multiplied back."""
    return t.float().cpu().numpy().view(np.complex64)[..., 0].astype(np.complex128) * scale


class Guarded:
    """A device buffer of F frames with as many guard frames behind it, all NaN before the call: the
    guard must still be NaN afterwards (a kernel instantiated for the wider element type would write, or
    read, up to twice the buffer)."""

    def __init__(self, F, shape, half):
        import torch
        self.full = torch.full((2 * F,) + tuple(shape), float("nan"), dtype=torch.float16 if half else torch.float32,
                               device="cuda")
        self.F = F
        self.buf = self.full[:F]

    def check(self):
        import torch
        assert bool(torch.isnan(self.full[self.F:]).all()), "the call wrote behind its output buffer"


def _process_device(engine, r, in_dtype, out_dtype, want_cube, want_rd):
    import torch
    nts, pn, nr, nd, _ = r.g
    F, M = r.F, r.cfg.max_targets
    dev = dict(device="cuda")
    nan = float("nan")
    outs = dict(profile=torch.full((F, nr), nan, **dev), tgt_count=torch.full((F,), -1, dtype=torch.int32, **dev),
                tgt_range_idx=torch.full((F, M), -1, dtype=torch.int32, **dev), tgt_range_mag=torch.full((F, M), nan, **dev),
                tgt_doppler_idx=torch.full((F, M), -1, dtype=torch.int32, **dev), slow_mag=torch.full((F, pn), nan, **dev))
    if want_cube:
        outs["probe_mag"] = torch.full((nr,), nan, **dev)
    half = out_dtype == FMCW_C32H
    g_cube = Guarded(F, (pn, nr, 2), half) if want_cube else None
    g_rd = Guarded(F, (nr, nd, 2), half) if want_rd else None
    d_cube = g_cube.buf if want_cube else None
    d_rd = g_rd.buf if want_rd else None
    d_iq = _to_device(r, in_dtype)
    torch.cuda.synchronize()
    engine.process_device(d_iq, F, in_dtype, outs, d_cube=d_cube, d_rd=d_rd, out_dtype=out_dtype,
                          probe_column=r.probe_column if want_cube else 0, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    for gb in (g_cube, g_rd):
        if gb is not None:
            gb.check()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    got["probe"] = got.pop("probe_mag", None)
    got["cube"] = _complex(d_cube, nr if half else 1) if want_cube else None
    got["rd"] = _complex(d_rd, nr * nd if half else 1) if want_rd else None
    got["raw"] = (None if d_cube is None else d_cube.cpu().numpy(), None if d_rd is None else d_rd.cpu().numpy())
    return got


def _check_against_chain(r, got, cube_dt, rd_dt, label):
    """Every output `got` holds against the plain chain at 2 e_ref + the fp32 bar; the detections."""
    pl, emu = r.plain, r.emu(cube_dt, rd_dt)
    err = SR.errors(got, pl)
    worst = {}
    for k, e in err.items():
        lim = SR.bound(emu["e_ref"][k])
        worst[k] = (float(np.max(e)), float(np.max(emu["e_ref"][k])))
        assert np.all(np.isfinite(e)), (label, k)
        assert np.all(e <= lim), (label, k, e, lim)
        assert np.all(e <= TOL_FP16_REL_L2), (label, k, e)
        if np.all(emu["e_ref"][k] == 0):
            assert np.all(e <= TOL_FP32_REL_L2), (label, k, e)
    print(f"\nGRID {label} " + " ".join(f"{k} {a:.2e}/{b:.2e}" for k, (a, b) in worst.items()))
    np.testing.assert_array_equal(got["tgt_count"], pl["tgt_count"])
    np.testing.assert_array_equal(got["tgt_range_idx"], pl["tgt_range_idx"])
    has = pl["tgt_count"] > 0
    assert np.all(got["slow_mag"][~has] == 0)
    assert np.all(got["tgt_doppler_idx"][~has] == 0) and np.all(got["tgt_range_mag"][~has] == 0)
    exact = r.doppler_mask(cube_dt, rd_dt)
    np.testing.assert_array_equal(got["tgt_doppler_idx"][exact], pl["tgt_doppler_idx"][exact])
    left_out = 0
    for f in np.nonzero(has)[0]:
        if not exact[f, 0]:
            # no exact index: one of the bins within ROW_GAP of the row's maximum (streams_reference.near_max_bins)
            near = SR.near_max_bins(pl, f, 0) | SR.near_max_bins(emu, f, 0)
            assert int(got["tgt_doppler_idx"][f, 0]) in near, (label, f, got["tgt_doppler_idx"][f, 0], near)
            left_out += r.g[1] >= r.g[3]
    assert left_out <= 0.10 * has.sum(), (label, left_out)


GRID = [(g, i, o, w) for g in SR.STORAGE_CASES for i in DT for o in DT for w in WANTS]


def _grid_id(c):
    g, i, o, (wc, wr) = c
    return f"{SR.case_id(g)}-in_{DT[i]}-out_{DT[o]}-{'cube' if wc else ''}{'+' if wc and wr else ''}{'rd' if wr else ''}{'' if wc or wr else 'neither'}"


@pytest.mark.parametrize("c", GRID, ids=_grid_id)
def test_storage_grid(streams, c):
    g, in_dtype, out_dtype, (want_cube, want_rd) = c
    r = SR.ref(g, in_dtype, "storage")
    _taps(streams, r)
    got = _process_device(streams, r, in_dtype, out_dtype, want_cube, want_rd)
    cube_dt = out_dtype if want_cube else FMCW_C64
    rd_dt = out_dtype if want_rd else FMCW_C64
    _check_against_chain(r, got, cube_dt, rd_dt, "storage " + _grid_id(c))


# ---------------------------------------------------------------------------
# FMCW_PAIR=1: the 16-byte lane-pair access of K2 (ld_c2 / st_c2 / pair_xchg, staging rows of ND + 2)
# ---------------------------------------------------------------------------
PAIR_GRID = [(g, st) for g in SR.PAIR_CASES for st in STORAGE]


@pytest.mark.parametrize("g,st", PAIR_GRID, ids=[f"{SR.case_id(g)}-cube_{DT[s[0]]}-rd_{DT[s[1]]}" for g, s in PAIR_GRID])
def test_pair_access_changes_no_bit(streams, monkeypatch, g, st):
    """The pair path changes the load and store forms only, the arithmetic and its order not: the RD
    map, the profile and the detections are those of the default path, bit for bit.  (cube, rd) storage
    st is reached through the requested buffers: a c32h cube needs d_cube with out_dtype C32H, and so on;
    the mixed pairs request one buffer only."""
    cube_dt, rd_dt = st
    out_dtype = FMCW_C32H if FMCW_C32H in st else FMCW_C64
    want_cube = cube_dt == out_dtype
    want_rd = rd_dt == out_dtype
    r = SR.ref(g, FMCW_C64, "synth")
    _taps(streams, r)
    _pair_identity(streams, monkeypatch, r, cube_dt, rd_dt, out_dtype, want_cube, want_rd)


def _pair_identity(streams, monkeypatch, r, cube_dt, rd_dt, out_dtype, want_cube, want_rd):
    monkeypatch.delenv("FMCW_PAIR", raising=False)
    a = _process_device(streams, r, FMCW_C64, out_dtype, want_cube, want_rd)
    monkeypatch.setenv("FMCW_PAIR", "1")
    b = _process_device(streams, r, FMCW_C64, out_dtype, want_cube, want_rd)
    monkeypatch.delenv("FMCW_PAIR")
    for k in ("profile", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "slow_mag"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for x, y in zip(a["raw"], b["raw"]):
        if x is not None:
            assert not np.isnan(x).any()
            np.testing.assert_array_equal(x, y)
    # the default path itself is right, so the identity is not one between two wrong results
    assert rel_l2(a["profile"], r.emu(cube_dt, rd_dt)["profile"], axis=1).max() <= TOL_FP16_REL_L2


@pytest.mark.parametrize("g", [SR.PAIR_CASES[0], SR.PAIR_CASES[3]], ids=SR.case_id)
def test_pair_access_meets_the_oracle_bars(streams, monkeypatch, g):
    """FMCW_PAIR=1 on its own, c64 throughout, against the oracle at the fp32 bars (Nr 16 x Nd 2 with its
    partial tile, and Nd 128)."""
    r = SR.ref(g, FMCW_C64, "synth")
    _taps(streams, r)
    monkeypatch.setenv("FMCW_PAIR", "1")
    got = _process_device(streams, r, FMCW_C64, FMCW_C64, True, True)
    monkeypatch.delenv("FMCW_PAIR")
    pl = r.plain
    err = SR.errors(got, pl)
    print(f"\nGRID pair {SR.case_id(g)} " + " ".join(f"{k} {float(np.max(e)):.2e}" for k, e in err.items()))
    for k, e in err.items():
        assert np.all(e <= TOL_FP32_REL_L2), (k, e)
    for k in ("tgt_count", "tgt_range_idx", "tgt_doppler_idx"):
        np.testing.assert_array_equal(got[k], pl[k], err_msg=k)


# ---------------------------------------------------------------------------
# fmcw_range_fft_device: K1 with the profile
# ---------------------------------------------------------------------------
K1_GRID = [(g, st, cpt) for g in SR.K1_CASES for st in STORAGE for cpt in SR.K1_CPT]


@pytest.mark.parametrize("g,st,cpt", K1_GRID,
                         ids=[f"{SR.case_id(g)}-in_{DT[s[0]]}-cube_{DT[s[1]]}-cpt_{c or 'unset'}" for g, s, c in K1_GRID])
def test_range_fft_device_grid(engine, monkeypatch, g, st, cpt):
    in_dtype, cube_dtype = st
    if cpt is None:
        monkeypatch.delenv("FMCW_K1_CPT", raising=False)
    else:
        monkeypatch.setenv("FMCW_K1_CPT", cpt)
    _range_fft_device(engine, SR.ref(g, in_dtype, "synth"), in_dtype, cube_dtype, cpt)


def _range_fft_device(engine, r, in_dtype, cube_dtype, cpt, label="k1"):
    import torch
    g = r.g
    _taps(engine, r)
    nts, pn, nr, nd, F = g
    half = cube_dtype == FMCW_C32H
    d_iq = _to_device(r, in_dtype)
    g_cube = Guarded(F, (pn, nr, 2), half)
    d_cube = g_cube.buf
    d_prof = torch.full((F, nr), float("nan"), device="cuda")
    runs = []
    for _ in range(2):                   # the second call into the same buffers: the call zeroes the profile itself
        torch.cuda.synchronize()
        engine.range_fft_device(d_iq, F, in_dtype, d_cube, d_prof, out_dtype=cube_dtype, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        runs.append((d_cube.cpu().numpy(), d_prof.cpu().numpy()))
    g_cube.check()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    emu = r.emu(cube_dtype, FMCW_C64)
    e_cube = rel_l2(_complex(d_cube, nr if half else 1), r.plain["cube"], axis=(1, 2))
    # the profile comes from the fp32 registers before the store: the fp32 bar also for a c32h cube
    e_prof = rel_l2(runs[0][1], r.plain["profile"], axis=1)
    print(f"\nGRID {label} {SR.case_id(g)} in {DT[in_dtype]} cube {DT[cube_dtype]} cpt {cpt or 'unset'} "
          f"paths {'/'.join(sorted(SR.k1_profile_paths(g, cpt)))} cube {e_cube.max():.2e}/{np.max(emu['e_ref']['cube']):.2e} "
          f"profile {e_prof.max():.2e}")
    assert np.all(e_cube <= SR.bound(emu["e_ref"]["cube"])) and np.all(e_cube <= TOL_FP16_REL_L2)
    if not half:
        assert np.all(e_cube <= TOL_FP32_REL_L2)
    assert np.all(e_prof <= TOL_FP32_REL_L2)
