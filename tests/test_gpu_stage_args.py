"""GPU: what the ten entry points of the five RD-map stages (api_stages.cpp: fmcw_cfar, fmcw_sig,
fmcw_cluster, fmcw_track, fmcw_mti and their *_device forms) answer to arguments they refuse, and
to F = 0 -- the status, the message, and which of two wrong arguments is the one reported.  The
map is the smallest (nr 16, nd 4, one frame) and no call here launches anything: each is refused,
or has nothing to do."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C64, _lib

pytestmark = pytest.mark.gpu

NR, ND, K, M, T = 16, 4, 4, 4, 4
OK, E_ARG = _lib.FMCW_OK, _lib.FMCW_E_ARG
NULL_MSG = b"required pointer is NULL"

# entry -> its arguments after the context, in order
ORDER = {
    "fmcw_cfar_device": "q rd dtype F nr nd count ridx didx power noise mask stream",
    "fmcw_cfar": "q rd dtype F nr nd count ridx didx power noise mask",
    "fmcw_sig_device": "q rd dtype F nr nd center stride dt rt dt_max rt_max stream",
    "fmcw_sig": "q rd dtype F nr nd center stride dt rt dt_max rt_max",
    "fmcw_cluster_device": "q F nr nd max_det count ridx didx power noise out label stream",
    "fmcw_cluster": "q F nr nd max_det count ridx didx power noise out label",
    "fmcw_track_device": "q S F nr nd max_tgt count range doppler power state out tgt_track stream",
    "fmcw_track": "q S F nr nd max_tgt count range doppler power state out tgt_track",
    "fmcw_mti_device": "q rd dtype S F nr nd bg seen out stream",
    "fmcw_mti": "q rd dtype S F nr nd bg seen out",
}
WITH_DTYPE = [e for e, o in ORDER.items() if " dtype " in o]
WITH_S = [e for e, o in ORDER.items() if " S " in o]
STAGE = {e: e.split("_")[1] for e in ORDER}
# a mandatory pointer of each entry
MANDATORY = {e: "rd" if " rd " in o else "count" for e, o in ORDER.items()}


class Entries:
    """Every entry with a set of good arguments for a 1-frame 16 x 4 map; call(entry, **changed)
    returns (status, message)."""

    def __init__(self, engine):
        import torch
        self.lib, self.h = engine.lib, engine.h
        self.dev = torch.zeros(32 * 1024, dtype=torch.uint8, device="cuda")
        self.host = np.zeros(32 * 1024 + 64, np.uint8)
        hbase = (self.host.ctypes.data + 63) & ~63
        self.slot = {True: lambda i: self.dev.data_ptr() + 1024 * i, False: lambda i: hbase + 1024 * i}
        self.q = dict(cfar=_lib.CfarParams(0, 0, 1, 1, 0, 0, K, 0, 5.0), sig=_lib.SigParams(0, 0, 2, 0, 0, -60.0),
                      cluster=_lib.ClusterParams(1, 1, 1, M, 0), track=_lib.TrackParams(2.0, 1.0, 0.5, 0.5, 0.1, 2, 2, T, 0),
                      mti=_lib.MtiParams(0.25, 1))

    def good(self, entry):
        at = self.slot[entry.endswith("_device")]
        names = ORDER[entry].split()
        a = {n: at(i) for i, n in enumerate(names)}                       # every pointer its own 1 KiB slot
        a.update(q=ct.byref(self.q[STAGE[entry]]), dtype=FMCW_C64, F=1, S=1, nr=NR, nd=ND, max_det=K, max_tgt=M, stride=1,
                 stream=None)
        if "out" in a and STAGE[entry] == "cluster":
            a["out"] = ct.byref(_lib.Targets(*[at(16 + i) for i in range(11)]))
        if "out" in a and STAGE[entry] == "track":
            a["out"] = ct.byref(_lib.Tracks(*[at(16 + i) for i in range(9)]))
        return {n: a[n] for n in names}

    def call(self, entry, **changed):
        a = self.good(entry)
        assert set(changed) <= set(a), (entry, changed)
        a.update(changed)
        st = getattr(self.lib, entry)(self.h, *a.values())
        return st, self.lib.fmcw_last_error()


@pytest.fixture(scope="module")
def entries(engine):
    return Entries(engine)


@pytest.mark.parametrize("entry", WITH_DTYPE)
def test_bad_dtype(entries, entry):
    assert entries.call(entry, dtype=2) == (E_ARG, b"bad rd_dtype")
    assert entries.call(entry, dtype=-1) == (E_ARG, b"bad rd_dtype")
    # two wrong arguments: the dtype is looked at before F
    assert entries.call(entry, dtype=2, F=-1) == (E_ARG, b"bad rd_dtype")


@pytest.mark.parametrize("entry", sorted(ORDER))
def test_negative_frame_count(entries, entry):
    want = b"S < 0 or F < 0" if entry in WITH_S else b"F < 0"
    assert entries.call(entry, F=-1) == (E_ARG, want)
    assert entries.call(entry, F=-1, **{MANDATORY[entry]: None}) == (E_ARG, want)
    if entry in WITH_S:
        assert entries.call(entry, S=-1) == (E_ARG, want)


@pytest.mark.parametrize("entry", sorted(ORDER))
def test_null_mandatory_pointer(entries, entry):
    assert entries.call(entry, **{MANDATORY[entry]: None}) == (E_ARG, NULL_MSG)
    if STAGE[entry] in ("cluster", "track"):                               # the struct, and the count inside it
        assert entries.call(entry, out=None) == (E_ARG, NULL_MSG)
        empty = _lib.Targets() if STAGE[entry] == "cluster" else _lib.Tracks()
        assert entries.call(entry, out=ct.byref(empty)) == (E_ARG, NULL_MSG)


@pytest.mark.parametrize("entry", sorted(ORDER))
def test_no_frames_is_ok_before_the_pointers_are_looked_at(entries, entry):
    assert entries.call(entry, F=0)[0] == OK
    assert entries.call(entry, F=0, **{MANDATORY[entry]: None})[0] == OK
    if entry in WITH_S:
        assert entries.call(entry, S=0, **{MANDATORY[entry]: None})[0] == OK


def test_what_is_checked_before_no_frames(entries):
    """The rules that come before the F == 0 return hold at F = 0 too."""
    for entry in ("fmcw_sig_device", "fmcw_sig"):
        assert entries.call(entry, F=0, dt=None, rt=None) == (E_ARG, b"sig: both maps are NULL")
        assert entries.call(entry, F=0, stride=0) == (E_ARG, b"sig: center_stride must be >= 1")
        assert entries.call(entry, F=0, stride=0, center=None)[0] == OK
    assert entries.call("fmcw_mti", F=0, seen=None) == (E_ARG, b"mti: bg and seen must both be given or both be NULL")
    assert entries.call("fmcw_mti", F=0, bg=None, seen=None)[0] == OK
    for entry in sorted(ORDER):
        assert entries.call(entry, F=0, nd=2) == (E_ARG, STAGE[entry].encode() + b": nd must be a power of two in [4, 1024]")
        assert entries.call(entry, F=0, q=None) == (E_ARG, STAGE[entry].encode() + b" params is NULL")


def test_sig_without_frames_writes_both_maxima(entries):
    mx = np.full(2, -3.0, np.float32)
    assert entries.call("fmcw_sig", F=0, rd=None, dt_max=mx[0:].ctypes.data, rt_max=mx[1:].ctypes.data)[0] == OK
    assert mx.tolist() == [0.0, 0.0]
    assert entries.call("fmcw_sig", F=0, dt_max=None, rt_max=None)[0] == OK


@pytest.mark.parametrize("entry", WITH_S)
def test_too_many_sequences(entries, entry):
    msg = STAGE[entry].encode() + b": S must be below 2^31 and S * F at most 2^40"
    assert entries.call(entry, S=2 ** 31) == (E_ARG, msg)
    assert entries.call(entry, S=2 ** 31, F=0) == (E_ARG, msg)
    assert entries.call(entry, S=2 ** 20, F=2 ** 20 + 1) == (E_ARG, msg)
    assert entries.call(entry, S=2 ** 31 - 1, F=0)[0] == OK


def test_misaligned_map(entries):
    rd = entries.good("fmcw_cfar_device")["rd"] + 8
    assert entries.call("fmcw_cfar_device", rd=rd) == (E_ARG, b"cfar: d_rd must be 16-byte aligned")
    assert entries.call("fmcw_sig_device", rd=rd) == (E_ARG, b"sig: d_rd must be 16-byte aligned")
    assert entries.call("fmcw_mti_device", rd=rd) == (E_ARG, b"mti: d_rd, d_out, d_bg and d_seen must be 16-byte aligned")
    for entry in ("fmcw_cfar_device", "fmcw_sig_device", "fmcw_mti_device"):
        assert entries.call(entry, rd=rd, F=0)[0] == OK                    # not looked at without frames
        assert entries.call(entry, rd=rd, dtype=2) == (E_ARG, b"bad rd_dtype")


def test_mti_freeze_needs_an_output(entries):
    q = ct.byref(_lib.MtiParams(0.25, _lib.FMCW_MTI_FREEZE))
    for entry in ("fmcw_mti_device", "fmcw_mti"):
        assert entries.call(entry, q=q, out=None, F=0) == (E_ARG, b"mti: FREEZE without an output leaves nothing to do")
        assert entries.call(entry, q=q, out=None, S=2 ** 31)[1] == b"mti: S must be below 2^31 and S * F at most 2^40"
