"""The range/Doppler chain (k_rdx, k_range, k_doppler, k_detect, k_detect_1p, k_probe) under the tap families
of tests/taps_cases.py: windows with no symmetry and non-zero ends, windows that weigh the edge samples and
edge chirps alone, and a calibration vector of varying modulus, non-linear phase and non-zero mean.  The
references are the float64 oracle and the storage-emulating chains of tests/streams_reference.py and
tests/xcd_reference.py under the same taps; the bars are those of the two grids (the fp32 bar for c64,
2 e_ref + the fp32 bar behind an fp16 store), unchanged.  tests/test_taps_cases_host.py proves on the oracle
that each family moves an output by 100 bars or more under a reversed tap index, a dropped end sample or
chirp, or a stale calibration vector, where the plain taps stay under one.

  streams sizes   every size case x {tilt, rand, ends}, c64
  streams storage the storage cases x the four (cube, RD) pairs, rand
  K1              fmcw_range_fft_device x {rand, ends}, and FMCW_K1_CPT 1 and 64
  pair            FMCW_PAIR=1 bit-identical to the default path, rand
  k_rdx c64       every nts case x {rand, ends}, tilt at nts 1024 and 1000; with and without the RD map
  k_rdx fp16      c32h in and out at each nts's own hand-off mask, rand
  fix path        FMCW_ONEPASS_FORCE_FIX with a probe column, rand
  re-tapping      one context through a sequence of taps, each call bit-identical to a new context's

Each measured figure is printed before it is asserted (pytest -s shows them; DESIGN.md 5.5 records them).
"""
import dataclasses

import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
from fmcw_radar_processing_amd import params as P
from fmcw_radar_processing_amd._lib import FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS, FMCW_PIPE_XCD
from tests import streams_reference as SR
from tests import taps_cases as TC
from tests import xcd_reference as XR
from tests.helpers import TOL_FP32_REL_L2, rd_rel_err, rel_l2
from tests.streams_reference import STORAGE
from tests.test_gpu_detect_rules import check_self
from tests.test_gpu_streams_grid import (DT, _check_against_chain, _pair_identity, _process, _process_device,
                                         _range_fft_device, _taps)
from tests.test_gpu_xcd_grid import DECISIONS, _check_c64, _check_fp16, _run, _run_fp16, _same

pytestmark = pytest.mark.gpu

BAR = TOL_FP32_REL_L2


@pytest.fixture
def streams(engine):
    engine.set_pipeline(FMCW_PIPE_STREAMS)
    try:
        yield engine
    finally:
        engine.set_pipeline(FMCW_PIPE_AUTO)


@pytest.fixture
def xcd(engine):
    engine.set_pipeline(FMCW_PIPE_XCD)
    try:
        yield engine
    finally:
        engine.set_pipeline(FMCW_PIPE_AUTO)


# ---------------------------------------------------------------------------
# the streams schedule, c64
# ---------------------------------------------------------------------------
SIZE_GRID = [(g, k) for k in TC.NEW_KINDS for g in SR.SIZE_CASES]


@pytest.mark.parametrize("g,kind", SIZE_GRID, ids=[f"{SR.case_id(g)}-{k}" for g, k in SIZE_GRID])
def test_streams_sizes(streams, g, kind):
    """test_gpu_streams_grid.test_sizes_match_oracle under the family's taps, the white frame element-wise;
    the frames and rows the oracle leaves open (taps_cases.flagged_frames, ambiguous_rows) by check_self only."""
    r = SR.ref(g, FMCW_C64, "noise", kind)
    ref, cfg = r.plain, r.cfg
    _taps(streams, r)
    got = _process(streams, r)
    ok = ~TC.flagged_frames(r, True)
    rows = TC.ambiguous_rows(r)
    e_cube = rel_l2(got["cube"], ref["cube"], axis=(1, 2)).max()
    e_rd = rd_rel_err(got["rd"], ref["rd"], ref["cube"], r.wd, cfg.nd).max()
    e_prof = rel_l2(got["profile"], ref["profile"], axis=1).max()
    n = r.noise
    m_cube = np.abs(got["cube"][n] - ref["cube"][n]).max() / XR.rms(ref["cube"][n])
    m_rd = np.abs(got["rd"][n] - ref["rd"][n]).max() / XR.rms(ref["rd"][n])
    has = (ref["tgt_count"] > 0) & ok
    none = (ref["tgt_count"] == 0) & ok
    e_slow = rel_l2(got["slow_mag"][has], ref["slow_mag"][has], axis=1).max() if has.any() else 0.0
    e_mag = np.abs(got["tgt_range_mag"][has, 0] / ref["tgt_range_mag"][has, 0] - 1.0).max() if has.any() else 0.0
    e_probe = rel_l2(got["probe_mag"], ref["probe"])
    print(f"\nTAPS sizes {SR.case_id(g)} {kind} cube {e_cube:.2e} rd {e_rd:.2e} profile {e_prof:.2e} white: cube {m_cube:.2e} "
          f"rd {m_rd:.2e} slow {e_slow:.2e} mag {e_mag:.2e} probe {e_probe:.2e} open frames {int((~ok).sum())} rows {int(rows.sum())}")
    assert e_cube <= BAR and e_rd <= BAR and e_prof <= BAR
    assert m_cube <= BAR and m_rd <= BAR
    assert e_slow <= BAR and e_mag <= BAR and e_probe <= BAR
    assert np.all(got["slow_mag"][none] == 0)
    np.testing.assert_array_equal(got["tgt_count"][ok], ref["tgt_count"][ok])
    np.testing.assert_array_equal(got["tgt_range_idx"][ok], ref["tgt_range_idx"][ok])
    dop = ok[:, None] & ~rows
    np.testing.assert_array_equal(got["tgt_doppler_idx"][dop], ref["tgt_doppler_idx"][dop])
    check_self(got, cfg)


# ---------------------------------------------------------------------------
# the streams schedule, storage
# ---------------------------------------------------------------------------
def _requests(st):
    """(out_dtype, want_cube, want_rd) that reach (cube, rd) storage st: the scratch buffers are c64."""
    out_dtype = FMCW_C32H if FMCW_C32H in st else FMCW_C64
    return out_dtype, st[0] == out_dtype, st[1] == out_dtype


STORAGE_GRID = [(g, st) for g in SR.STORAGE_CASES for st in STORAGE]
ST_IDS = [f"{SR.case_id(g)}-cube_{DT[s[0]]}-rd_{DT[s[1]]}" for g, s in STORAGE_GRID]


@pytest.mark.parametrize("g,st", STORAGE_GRID, ids=ST_IDS)
def test_streams_storage(streams, g, st):
    r = SR.ref(g, FMCW_C64, "storage", "rand")
    _taps(streams, r)
    out_dtype, want_cube, want_rd = _requests(st)
    got = _process_device(streams, r, FMCW_C64, out_dtype, want_cube, want_rd)
    _check_against_chain(r, got, st[0], st[1], f"taps storage {SR.case_id(g)} rand cube {DT[st[0]]} rd {DT[st[1]]}")
    check_self({k: v for k, v in got.items() if k != "rd"}, r.cfg)


# ---------------------------------------------------------------------------
# fmcw_range_fft_device
# ---------------------------------------------------------------------------
K1_GRID = ([(g, k, cd, None) for k in TC.K1_KINDS for g in SR.K1_CASES for cd in (FMCW_C64, FMCW_C32H)]
           + [(g, k, FMCW_C64, cpt) for k in TC.K1_KINDS for g, cpt in TC.K1_CPT_CASES])


@pytest.mark.parametrize("g,kind,cube_dtype,cpt", K1_GRID,
                         ids=[f"{SR.case_id(g)}-{k}-cube_{DT[c]}-cpt_{p or 'unset'}" for g, k, c, p in K1_GRID])
def test_range_fft_device(engine, monkeypatch, g, kind, cube_dtype, cpt):
    if cpt is None:
        monkeypatch.delenv("FMCW_K1_CPT", raising=False)
    else:
        monkeypatch.setenv("FMCW_K1_CPT", cpt)
    _range_fft_device(engine, SR.ref(g, FMCW_C64, "synth", kind), FMCW_C64, cube_dtype, cpt, f"taps k1 {kind}")


# ---------------------------------------------------------------------------
# FMCW_PAIR=1
# ---------------------------------------------------------------------------
PAIR_GRID = [(g, st) for g in SR.PAIR_CASES for st in STORAGE]


@pytest.mark.parametrize("g,st", PAIR_GRID, ids=[f"{SR.case_id(g)}-cube_{DT[s[0]]}-rd_{DT[s[1]]}" for g, s in PAIR_GRID])
def test_pair_access_changes_no_bit(streams, monkeypatch, g, st):
    r = SR.ref(g, FMCW_C64, "synth", "rand")
    _taps(streams, r)
    _pair_identity(streams, monkeypatch, r, st[0], st[1], *_requests(st))


# ---------------------------------------------------------------------------
# k_rdx
# ---------------------------------------------------------------------------
NTS_GRID = [(n, k) for k in ("rand", "ends") for n in XR.NTS_CASES] + [(n, "tilt") for n in TC.TILT_NTS]


def _rdx_c64(xcd, r, label):
    pl = r.plain
    flagged, rows = TC.flagged_frames(r, False), TC.ambiguous_rows(r)
    a = _run(xcd, r, probe_column=r.probe_column)
    _check_c64(r, a, label, pl["probe"], flagged, rows)
    f0 = r.index("white_x0")
    b = _run(xcd, r, want_rd=False, probe_column=f0 * XR.PN + 1)
    e = rel_l2(b["probe_mag"], np.abs(pl["cube"][f0, 0]))
    print(f"TAPS {label} probe of chirp 0 {e:.2e} open frames {int(flagged.sum())} rows {int(rows.sum())}")
    assert e <= BAR
    _same(a, b, DECISIONS, f"{label} with and without the RD map")
    check_self(b, r.cfg)


@pytest.mark.parametrize("nts,kind", NTS_GRID, ids=[f"{n}-{k}" for n, k in NTS_GRID])
def test_rdx_c64(xcd, nts, kind):
    _rdx_c64(xcd, XR.ref(nts, FMCW_C64, kind), f"nts {nts} {kind}")


@pytest.mark.parametrize("nts", XR.FP16_NTS)
def test_rdx_fp16(xcd, nts):
    r = XR.ref(nts, FMCW_C32H, "rand")
    got = _run_fp16(xcd, r, probe_column=r.probe_column)
    _check_fp16(r, got, r.mask, f"taps fp16 nts {nts} rand")


@pytest.mark.parametrize("nts", TC.TILT_NTS)
def test_rdx_slow_row_fix_path_and_probe(xcd, monkeypatch, nts):
    """With no candidates kept every slow-time row comes from k_slow_fix (test_gpu_onepass); the probe column
    is hot chirp 9."""
    monkeypatch.setenv("FMCW_ONEPASS_FORCE_FIX", "1")
    _rdx_c64(xcd, XR.ref(nts, FMCW_C64, "rand"), f"fix path nts {nts} rand")


# ---------------------------------------------------------------------------
# re-tapping a live context
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class ScaledConfig(P.FmcwConfig):
    """A configuration whose if_scale alone differs (if_scale is derived from nr / nts)."""
    scale: float = 1.0

    @property
    def if_scale(self) -> float:
        return self.scale * P.FmcwConfig.if_scale.fget(self)


def _scaled(cfg, scale):
    return ScaledConfig(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg)}, scale=scale)


G_XCD = (1024, 256, 1024, 256, 9)
G_SMALL = (64, 16, 256, 16, 5)
RETAP = [(FMCW_PIPE_XCD, G_XCD), (FMCW_PIPE_STREAMS, G_XCD), (FMCW_PIPE_STREAMS, G_SMALL)]


def _retap_frames(g, kind):
    """F frames about the family's calibration tone: the first F of the single-pass batch, or the size case's."""
    if g == G_XCD:
        return XR.frames(1024, kind)[1][:g[4]]
    return SR.synth(g, SR.build_case(g, taps=kind)[1], kind)


def _retap_steps(g):
    """[(label, cfg, cal, wr, wd, iq, rebuild)]: rebuild False leaves the taps of the step before and
    hands the call the new parameters alone."""
    c = {k: SR.build_case(g, taps=k) for k in ("plain", "rand", "ends")}
    steps = [(k, c[k][0], c[k][4], c[k][2], c[k][3], _retap_frames(g, k), True) for k in ("plain", "rand", "ends", "plain")]
    cfg, _, wr, wd, _ = c["rand"]
    cal = c["plain"][4]
    iq = _retap_frames(g, "plain")
    steps.append(("rand windows, plain cal", cfg, cal, wr, wd, iq, True))
    steps.append(("if_scale / 2", _scaled(cfg, 0.5), cal, wr, wd, iq, False))
    return steps


def _call(eng, pipe, g, iq):
    """Every output the pipeline returns (the single pass keeps no range cube), the probe on chirp 1 of frame 1."""
    got = eng.process(iq, want_cube=pipe == FMCW_PIPE_STREAMS, want_rd=True, probe_column=g[1] + 2)
    eng.synchronize()
    return got


def _fresh(devices, pipe):
    from fmcw_radar_processing_amd.engine import Engine
    e = Engine(devices)
    e.set_pipeline(pipe)
    return e


@pytest.mark.parametrize("pipe,g", RETAP, ids=[f"{'xcd' if p == FMCW_PIPE_XCD else 'streams'}-{SR.case_id(g)}" for p, g in RETAP])
def test_retapping_a_live_context(pipe, g):
    """One context through plain, rand, ends, plain, rand's windows with plain's calibration, and the same taps
    with if_scale alone changed (the calibration-and-window table is rebuilt by the call, not by
    fmcw_set_taps): every call bit-identical to a new context given only those taps.  Then two contexts of
    one device under rand taps against one: the peers' calibration sum and tables."""
    live = _fresh(0, pipe)
    try:
        prev = None
        for label, cfg, cal, wr, wd, iq, rebuild in _retap_steps(g):
            if rebuild:
                live.set_taps(cfg, cal, wr, wd)
            else:
                live.cfg, live.p = cfg, cfg.abi()                  # new parameters, no fmcw_set_taps
            got = _call(live, pipe, g, iq)
            new = _fresh(0, pipe)
            try:
                new.set_taps(cfg, cal, wr, wd)
                want = _call(new, pipe, g, iq)
            finally:
                new.close()
            assert set(got) == set(want)
            _same(got, want, sorted(want), f"retap {label}")
            assert np.abs(want["profile"]).max() > 0 and np.isfinite(want["rd"]).all()
            if prev is not None and not rebuild:
                # the step is not a no-op: half the scale gives another profile
                assert not np.array_equal(prev["profile"], got["profile"])
            prev = got
        # two contexts of one device
        multi = _fresh([0, 0], pipe)
        try:
            cfg, _, wr, wd, cal = SR.build_case(g, taps="rand")
            iq = _retap_frames(g, "rand")
            live.set_taps(cfg, cal, wr, wd)
            multi.set_taps(cfg, cal, wr, wd)
            _same(_call(multi, pipe, g, iq), _call(live, pipe, g, iq), DECISIONS + ("rd", "probe_mag"), "two contexts, rand")
            half = _scaled(cfg, 0.5)
            for e in (live, multi):
                e.cfg, e.p = half, half.abi()
            _same(_call(multi, pipe, g, iq), _call(live, pipe, g, iq), DECISIONS + ("rd", "probe_mag"), "two contexts, rand, if_scale / 2")
        finally:
            multi.close()
    finally:
        live.close()
