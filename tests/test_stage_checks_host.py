"""CPU: the messages of the rules the five RD-map stages share (api_stages.cpp check_rd_shape,
check_gate), through each stage's host-only fmcw_*_check.  The map-shape and gate rules are one
function each with the stage's prefix passed in; the strings here are written out, stage by
stage, as the callers have always seen them."""
import ctypes as ct

import pytest

from fmcw_radar_processing_amd import _lib

# stage -> (message for a bad nr, message for a bad nd)
SHAPE_MESSAGES = {
    "cfar": (b"cfar: nr must be a power of two in [16, 2048]", b"cfar: nd must be a power of two in [4, 1024]"),
    "sig": (b"sig: nr must be a power of two in [16, 2048]", b"sig: nd must be a power of two in [4, 1024]"),
    "cluster": (b"cluster: nr must be a power of two in [16, 2048]", b"cluster: nd must be a power of two in [4, 1024]"),
    "track": (b"track: nr must be a power of two in [16, 2048]", b"track: nd must be a power of two in [4, 1024]"),
    "mti": (b"mti: nr must be a power of two in [16, 2048]", b"mti: nd must be a power of two in [4, 1024]"),
}
# stage -> (message for r_lo > r_hi, message for a gate outside 1..nr)
GATE_MESSAGES = {
    "cfar": (b"cfar: r_lo > r_hi", b"cfar: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
    "sig": (b"sig: r_lo > r_hi", b"sig: the gate r_lo..r_hi must lie in 1..nr (or be 0, 0 for all rows)"),
}
# (nr, nd, which of the two shape messages): nd = 2 is a size the frame pipeline itself takes
# (its rule is [2, 1024]); the RD-map stages start at 4
BAD_SHAPES = [(8, 16, 0), (24, 16, 0), (4096, 16, 0), (64, 2, 1), (64, 2048, 1)]


def _check(stage, nr, nd, r_lo=0, r_hi=0):
    """The stage's fmcw_*_check on parameters that are valid for a 64 x 16 map but for nr, nd and
    the gate."""
    lib = _lib.load()
    if stage == "cfar":
        q = _lib.CfarParams(1, 1, 2, 2, r_lo, r_hi, 16, 0, 5.0)
        return lib.fmcw_cfar_check(ct.byref(q), nr, nd, None)
    if stage == "sig":
        q = _lib.SigParams(r_lo, r_hi, 2, 0, 0, -60.0)
        return lib.fmcw_sig_check(ct.byref(q), nr, nd)
    if stage == "cluster":
        q = _lib.ClusterParams(1, 1, 1, 8, 0)
        return lib.fmcw_cluster_check(ct.byref(q), nr, nd, 16)
    if stage == "track":
        q = _lib.TrackParams(2.0, 2.0, 0.5, 0.5, 0.1, 2, 2, 8, 0)
        return lib.fmcw_track_check(ct.byref(q), nr, nd, 8)
    q = _lib.MtiParams(0.25, 1)
    return lib.fmcw_mti_check(ct.byref(q), nr, nd)


@pytest.mark.parametrize("stage", sorted(SHAPE_MESSAGES))
def test_the_parameters_used_here_are_valid(stage):
    for nr, nd in ((64, 16), (16, 8), (2048, 1024)):
        assert _check(stage, nr, nd) == _lib.FMCW_OK


@pytest.mark.parametrize("nr,nd,which", BAD_SHAPES, ids=[f"nr{a}_nd{b}" for a, b, _ in BAD_SHAPES])
@pytest.mark.parametrize("stage", sorted(SHAPE_MESSAGES))
def test_shape_message(stage, nr, nd, which):
    assert _check(stage, nr, nd) == _lib.FMCW_E_ARG
    assert _lib.load().fmcw_last_error() == SHAPE_MESSAGES[stage][which]


@pytest.mark.parametrize("stage", sorted(SHAPE_MESSAGES))
def test_nr_is_reported_before_nd(stage):
    assert _check(stage, 24, 2) == _lib.FMCW_E_ARG
    assert _lib.load().fmcw_last_error() == SHAPE_MESSAGES[stage][0]


@pytest.mark.parametrize("stage", sorted(GATE_MESSAGES))
def test_gate_messages(stage):
    lib = _lib.load()
    assert _check(stage, 64, 16, 1, 64) == _lib.FMCW_OK
    assert _check(stage, 64, 16, 7, 7) == _lib.FMCW_OK
    assert _check(stage, 64, 16, 5, 3) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error() == GATE_MESSAGES[stage][0]
    for r_lo, r_hi in ((0, 5), (1, 65), (-2, 5)):
        assert _check(stage, 64, 16, r_lo, r_hi) == _lib.FMCW_E_ARG
        assert lib.fmcw_last_error() == GATE_MESSAGES[stage][1]
