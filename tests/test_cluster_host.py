"""CPU: the host-side half of the clustering stage (include/fmcw.h, fmcw_cluster_params) -- the
argument rules -- and checks that pin the float64 reference the GPU tests compare against
(tests/cluster_reference.py): its partition against scipy's labelling, and its targets on the CFAR
reference's detections of the synthetic stream."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import _lib
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import cfar_reference as CR
from tests import cluster_reference as R
from tests.helpers import case


def _q(**over):
    d = dict(link_r=1, link_d=1, min_cells=1, max_tgt=16, flags=0)
    d.update(over)
    return _lib.ClusterParams(*[d[k] for k, _ in _lib.ClusterParams._fields_])


# every violation fmcw_cluster_check must name (shared with tests/test_gpu_cluster.py):
# (params, nr, nd, max_det, a word of the message)
REJECTED = {
    "link_r_9": (dict(link_r=9), 256, 32, 64, "link"),
    "link_d_9": (dict(link_d=9), 256, 32, 64, "link"),
    "link_r_negative": (dict(link_r=-1), 256, 32, 64, "link"),
    "doppler_link_exceeds_nd": (dict(link_d=8), 256, 16, 64, "exceeds nd"),      # 2 link_d + 1 = 17 > 16
    "min_cells_0": (dict(min_cells=0), 256, 16, 64, "min_cells"),
    "min_cells_1025": (dict(min_cells=1025), 256, 16, 64, "min_cells"),
    "max_tgt_0": (dict(max_tgt=0), 256, 16, 64, "max_tgt"),
    "max_tgt_65": (dict(max_tgt=65), 256, 16, 64, "max_tgt"),
    "max_det_0": (dict(), 256, 16, 0, "max_det"),
    "max_det_1025": (dict(), 256, 16, 1025, "max_det"),
    "stray_flag_bit": (dict(flags=4), 256, 16, 64, "flag"),
    "nd_not_a_power_of_two": (dict(), 256, 24, 64, "nd"),
    "nr_above_2048": (dict(), 4096, 16, 64, "nr"),
}


def test_check_accepts_the_defaults_and_the_limits():
    lib = _lib.load()
    q = P.ClusterConfig().abi()
    assert lib.fmcw_cluster_check(ct.byref(q), 256, 16, 64) == _lib.FMCW_OK
    assert lib.fmcw_cluster_check(ct.byref(_q(link_r=8, link_d=7, min_cells=1024, max_tgt=64)), 16, 16, 1024) == _lib.FMCW_OK
    assert lib.fmcw_cluster_check(ct.byref(_q(link_r=0, link_d=0, max_tgt=1)), 2048, 4, 1) == _lib.FMCW_OK
    assert lib.fmcw_cluster_check(None, 256, 16, 64) == _lib.FMCW_E_ARG
    P.ClusterConfig().validate(256, 16, 64)
    cfg, *_ = case(64, 16, 256, 16)
    q = P.ClusterConfig.for_config(cfg, link=(2, 1), min_cells=3, max_tgt=8)
    assert (q.link_r, q.link_d, q.min_cells, q.max_tgt) == (2, 1, 3, 8)
    a = q.abi()
    assert (a.link_r, a.link_d, a.min_cells, a.max_tgt, a.flags) == (2, 1, 3, 8, 0)


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_check_rejects(name):
    lib = _lib.load()
    over, nr, nd, max_det, word = REJECTED[name]
    assert lib.fmcw_cluster_check(ct.byref(_q(**over)), nr, nd, max_det) == _lib.FMCW_E_ARG
    assert word in lib.fmcw_last_error().decode()
    if "flags" not in over:                    # the Python mirror names the same rule
        q = P.ClusterConfig(**{k: v for k, v in over.items()})
        with pytest.raises(ValueError, match=word):
            q.validate(nr, nd, max_det)


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    q = _q()
    t = _lib.Targets()
    assert lib.fmcw_cluster(None, ct.byref(q), 1, 256, 16, 64, *([None] * 5), ct.byref(t), None) == _lib.FMCW_E_ARG
    assert lib.fmcw_cluster_device(None, ct.byref(q), 1, 256, 16, 64, *([None] * 5), ct.byref(t), None, None) \
        == _lib.FMCW_E_ARG


def lists_of_mask(mask, power=None, max_det=1024):
    """One frame's detection lists, as fmcw_cfar writes them, from a [nr][nd] mask (row-major =
    ascending (range, Doppler)); power [nr][nd] float32, or 1 + a ramp."""
    r, d = np.nonzero(mask)
    n = min(len(r), max_det)
    out = dict(det_count=np.array([len(r)], np.int32), det_range_idx=np.zeros((1, max_det), np.int32),
               det_doppler_idx=np.zeros((1, max_det), np.int32), det_power=np.zeros((1, max_det), np.float32))
    out["det_range_idx"][0, :n] = r[:n] + 1
    out["det_doppler_idx"][0, :n] = d[:n] + 1
    out["det_power"][0, :n] = (1 + np.arange(n)) if power is None else power[r[:n], d[:n]]
    return out


@pytest.mark.parametrize("seed", range(6))
def test_reference_partition_equals_scipy_label(seed):
    """Link (1, 1) is 8-connectivity: the reference's components are scipy.ndimage.label's with the
    3 x 3 structure, on masks rolled so that an empty Doppler column sits at the seam (scipy does
    not wrap)."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    nr, nd = 64, 16
    mask = rng.random((nr, nd)) < (0.08, 0.15, 0.25, 0.35, 0.5, 0.7)[seed]
    mask[:, rng.integers(nd)] = False
    empty = int(np.nonzero(~mask.any(axis=0))[0][0])
    mask = np.roll(mask, nd - 1 - empty, axis=1)           # the empty column becomes the last one
    assert not mask[:, -1].any() and mask.sum() > 20
    det = lists_of_mask(mask)
    n = int(det["det_count"][0])
    label = R.components(det["det_range_idx"][0, :n], det["det_doppler_idx"][0, :n], nd, (1, 1))
    want, nblob = ndi.label(mask, structure=np.ones((3, 3)))
    w = want[det["det_range_idx"][0, :n] - 1, det["det_doppler_idx"][0, :n] - 1]
    assert len(np.unique(label)) == nblob
    # the same partition: one reference label per scipy label and the other way round
    assert len(set(zip(label.tolist(), w.tolist()))) == nblob
    for root in np.unique(label):
        assert root == np.nonzero(label == root)[0].min()
    # and the per-target outputs add up
    ref = R.reference_of(det, P.ClusterConfig(max_tgt=64), nd)
    assert ref["tgt_count"][0] == nblob
    if nblob <= 64:
        assert ref["cells"][0].sum() == n
    # the wrap: the circular relation does not care where the seam lies, so any roll keeps the count
    wrapped = lists_of_mask(np.roll(mask, 5, axis=1))
    ref2 = R.reference_of(wrapped, P.ClusterConfig(max_tgt=64), nd)
    assert ref2["tgt_count"][0] == nblob


def test_reference_on_the_cfar_detections_of_the_synthetic_stream():
    """Frames 40..47 at (256, 32, 256, 32), guard (4, 3), train (4, 4), pfa 1e-6, gate 3..nr-2: in
    every frame that has a target the strongest target contains the synthetic cell; frame 47 has
    none.  One point target is one blob of many cells, which is why the stage exists."""
    nts, pn, nr, nd = 256, 32, 256, 32
    cfg, p, wr, wd, cal = case(nts, pn, nr, nd, P.THROUGHPUT)
    iq = O.synth_frames(8, pn, nts, nr, nd, p["dist_per_bin"], frame0=40)
    rd = O.process_frames(iq, cal, p, wr, wd, want_rd=True, rd_all_rows=True)["rd"].astype(np.complex64)
    alpha = P.CfarConfig.alpha_for(17 * 15 - 9 * 7, 1e-6)
    cf = CR.cfar_reference(rd, (4, 3), (4, 4), alpha, 3, nr - 2)
    assert CR.check_exempt(cf) == 0
    det = CR.lists(cf, 1024)
    det["det_power"] = det["det_power"].astype(np.float32)
    q = P.ClusterConfig(link_r=1, link_d=1, min_cells=1, max_tgt=16)
    ref = R.reference_of(det, q, nd)
    many = 0
    for i in range(8):
        fp = O.synth_frame_params(40 + i, nr, nd, p["dist_per_bin"])
        if fp["A"] == 0:
            assert i == 7 and ref["tgt_count"][i] == 0 and not ref["det_label"][i].any()
            continue
        assert ref["tgt_count"][i] >= 1
        n = int(det["det_count"][i])
        cell = np.nonzero((det["det_range_idx"][i, :n] == fp["r"] + 1) &
                          (det["det_doppler_idx"][i, :n] == fp["d"] + nd // 2 + 1))[0]
        assert len(cell) == 1 and ref["det_label"][i, cell[0]] == 1
        assert ref["extent_r"][i, 0] >= 1 and ref["cells"][i, 0] <= n
        assert abs(ref["range"][i, 0] - (fp["r"] + 1)) < ref["extent_r"][i, 0]
        many += ref["cells"][i, 0] > 1
    assert many >= 1
