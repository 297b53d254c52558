"""GPU: the clustering stage (csrc/kernels_cluster.hip through fmcw_cluster / fmcw_cluster_device)
against the float64 reference of tests/cluster_reference.py, which runs on exactly the list bytes
the device is given.  The partition, cells, the extents, the peak, peak_power, peak_noise, tgt_count,
the order and det_label are compared exactly, with no exempt cases; power and the centroids within
the n-term float32 bounds stated there.  Except for the end-to-end test the lists are built in numpy."""
import numpy as np
import pytest

from fmcw_radar_processing_amd import FMCW_C64, FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS, FmcwError, _lib
from fmcw_radar_processing_amd import params as P
from oracle import oracle as O
from tests import cluster_reference as R
from tests.helpers import case
from tests.test_cluster_host import REJECTED, lists_of_mask
from tests.test_gpu_cfar import GEOS, cfg_for, rd_map

pytestmark = pytest.mark.gpu

IN_KEYS = ("det_count", "det_range_idx", "det_doppler_idx", "det_power", "det_noise")
TGT_KEYS = ("tgt_count",) + R.INT_KEYS + R.FLOAT_KEYS
OUT_KEYS = TGT_KEYS + ("det_label",)


def cells_to_lists(cells, max_det, count=None):
    """One frame's lists from (r, d, power[, noise]) tuples, 1-based, sorted as fmcw_cfar writes them."""
    cells = sorted(cells)
    assert len({c[:2] for c in cells}) == len(cells) <= max_det
    out = dict(det_count=np.array([len(cells) if count is None else count], np.int32),
               det_range_idx=np.zeros((1, max_det), np.int32), det_doppler_idx=np.zeros((1, max_det), np.int32),
               det_power=np.zeros((1, max_det), np.float32), det_noise=np.zeros((1, max_det), np.float32))
    for i, c in enumerate(cells):
        out["det_range_idx"][0, i], out["det_doppler_idx"][0, i], out["det_power"][0, i] = c[:3]
        out["det_noise"][0, i] = c[3] if len(c) > 3 else 0.25 + i
    return out


def stack(*dets):
    keys = [k for k in IN_KEYS if all(k in d for d in dets)]
    return {k: np.concatenate([d[k] for d in dets]) for k in keys}


def with_noise(det):
    if "det_noise" not in det:
        det = dict(det, det_noise=(det["det_power"] * np.float32(0.125)).astype(np.float32))
    return det


def run_and_check(engine, det, q, nr, nd):
    got = engine.cluster(det, q, nr, nd)
    ref = R.reference_of(det, q, nd)
    R.assert_matches(got, ref, nr, nd)
    return got, ref


def _same(a, b, keys=OUT_KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def device_run(engine, det, q, nr, nd, leave_out=(), label=True, noise=True, F=None):
    """fmcw_cluster_device over buffers pre-filled with -3 / NaN; returns what they hold afterwards
    (None for the outputs left out)."""
    import torch
    dev = "cuda"
    K, M = det["det_range_idx"].shape[1], q.max_tgt
    nf = len(det["det_count"])
    d_in = {k: torch.from_numpy(np.ascontiguousarray(det[k])).to(dev) for k in IN_KEYS if k in det}
    if not noise:
        d_in.pop("det_noise", None)
    outs = dict(tgt_count=torch.full((nf,), -3, dtype=torch.int32, device=dev))
    for k in R.INT_KEYS:
        outs[k] = torch.full((nf, M), -3, dtype=torch.int32, device=dev)
    for k in R.FLOAT_KEYS:
        outs[k] = torch.full((nf, M), np.nan, dtype=torch.float32, device=dev)
    for k in leave_out:
        outs[k] = None
    d_label = torch.full((nf, K), -3, dtype=torch.int32, device=dev) if label else None
    torch.cuda.synchronize()
    engine.cluster_device(q, nf if F is None else F, nr, nd, K, d_in, outs, d_det_label=d_label,
                          stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = {k: (None if v is None else v.cpu().numpy()) for k, v in outs.items()}
    got["det_label"] = None if d_label is None else d_label.cpu().numpy()
    return got


# ---- 1. parity on CFAR lists ---------------------------------------------------------------------
_DET = {}


def cfar_lists(engine, geo):
    """The device's own detection lists of the geometry's frames at pfa 1e-3 (max_det 1024), made once."""
    if geo not in _DET:
        det = engine.cfar(rd_map(geo), cfg_for(geo[2], 1e-3))
        for v in det.values():
            v.setflags(write=False)
        _DET[geo] = det
    return _DET[geo]


@pytest.mark.parametrize("min_cells", [1, 3])
@pytest.mark.parametrize("link", [(1, 1), (2, 1)], ids=["link11", "link21"])
@pytest.mark.parametrize("geo", sorted(GEOS), ids=lambda g: "x".join(map(str, g)))
def test_parity_on_cfar_lists(engine, geo, link, min_cells):
    det = cfar_lists(engine, geo)
    nr, nd = geo[2:]
    q = P.ClusterConfig(link_r=link[0], link_d=link[1], min_cells=min_cells, max_tgt=64)
    got, ref = run_and_check(engine, det, q, nr, nd)
    assert (ref["cells"] > 1).any()                         # some frame has a multi-cell target
    every = R.reference_of(det, P.ClusterConfig(link_r=link[0], link_d=link[1], min_cells=1, max_tgt=64), nd)
    if min_cells > 1:                                       # and min_cells drops some target
        assert got["tgt_count"].sum() < every["tgt_count"].sum()
        n = np.clip(det["det_count"], 0, det["det_range_idx"].shape[1])
        assert any((got["det_label"][f, :n[f]] == 0).any() for f in range(len(n)))
    else:
        np.testing.assert_array_equal(got["tgt_count"], every["tgt_count"])


# ---- 2. slowest convergence ----------------------------------------------------------------------
def serpentine(nr, nd, rows, mirrored):
    """Odd rows carry Doppler bins 1..7, even rows one connector cell, at bin 7 and at bin 1
    alternately; bins 8..nd stay empty, so the ring stays cut: one component whose path runs through
    every cell.  mirrored: the row order reversed, the path's other end first in the list."""
    mask = np.zeros((nr, nd), bool)
    for k in range(rows):
        if k % 2 == 0:
            mask[k, 0:7] = True
        else:
            mask[k, 6 if (k // 2) % 2 == 0 else 0] = True
    if mirrored:
        mask[:rows] = mask[:rows][::-1].copy()
    return mask


def test_serpentine_converges_within_the_bound(engine):
    nr, nd = 256, 16
    a, b = serpentine(nr, nd, 201, False), serpentine(nr, nd, 200, True)
    det = stack(lists_of_mask(a), lists_of_mask(b))
    n = det["det_count"]
    assert n.tolist() == [101 * 7 + 100, 100 * 7 + 100] and n.max() <= 1024
    got, ref = run_and_check(engine, with_noise(det), P.ClusterConfig(max_tgt=4), nr, nd)
    assert got["tgt_count"].tolist() == [1, 1]
    np.testing.assert_array_equal(got["cells"][:, 0], n)
    for f in range(2):
        assert (got["det_label"][f, :n[f]] == 1).all() and not got["det_label"][f, n[f]:].any()
    assert got["extent_r"][:, 0].tolist() == [201, 200] and got["extent_d"][:, 0].tolist() == [7, 7]
    # without the connector rows the path is cut into its rows
    cut = a.copy()
    cut[1::2] = False
    got, _ = run_and_check(engine, with_noise(lists_of_mask(cut)), P.ClusterConfig(max_tgt=64), nr, nd)
    assert got["tgt_count"].tolist() == [101]


# ---- 3. the seam -----------------------------------------------------------------------------------
def test_the_doppler_seam(engine):
    nr, nd = 64, 16
    blob = [(r, d, 1.0 + 0.25 * d + r) for r in (10, 11) for d in (15, 16, 1, 2)]
    det = cells_to_lists(blob, 32)
    got, ref = run_and_check(engine, det, P.ClusterConfig(link_r=1, link_d=1, max_tgt=8), nr, nd)
    assert got["tgt_count"].tolist() == [1] and got["cells"][0, 0] == 8
    assert got["extent_d"][0, 0] == 4 and got["extent_r"][0, 0] == 2
    assert (got["peak_range_idx"][0, 0], got["peak_doppler_idx"][0, 0]) == (11, 16)
    c = float(got["doppler"][0, 0])
    assert min(abs(c - 16.5), abs(c - 0.5)) < 1.0          # the centroid lies at the fold, not mid-ring
    # equal powers: the peak is the first cell, (10, 1), and the centroid is exactly the fold
    flat = cells_to_lists([(r, d, 2.0) for r in (10, 11) for d in (15, 16, 1, 2)], 32)
    got, _ = run_and_check(engine, flat, P.ClusterConfig(max_tgt=8), nr, nd)
    assert (got["peak_range_idx"][0, 0], got["peak_doppler_idx"][0, 0]) == (10, 1)
    assert got["doppler"][0, 0] == 0.5 and got["range"][0, 0] == 10.5
    # no Doppler link: one target per Doppler bin
    got, _ = run_and_check(engine, det, P.ClusterConfig(link_r=1, link_d=0, max_tgt=8), nr, nd)
    assert got["tgt_count"].tolist() == [4] and got["cells"][0, :4].tolist() == [2, 2, 2, 2]
    # the widest Doppler link nd allows: a ring row of every other bin is one target, at link 1 it is eight
    ring = cells_to_lists([(20, d, float(d)) for d in range(1, nd + 1, 2)], 32)
    got, _ = run_and_check(engine, ring, P.ClusterConfig(link_r=0, link_d=(nd - 1) // 2, max_tgt=8), nr, nd)
    assert got["tgt_count"].tolist() == [1] and got["cells"][0, 0] == 8 and got["extent_d"][0, 0] == 15
    got, _ = run_and_check(engine, ring, P.ClusterConfig(link_r=0, link_d=1, max_tgt=8), nr, nd)
    assert got["tgt_count"].tolist() == [8]
    full = cells_to_lists([(20, d, 1.0 + (d % 5)) for d in range(1, nd + 1)], 32)
    got, _ = run_and_check(engine, full, P.ClusterConfig(link_r=0, link_d=(nd - 1) // 2, max_tgt=8), nr, nd)
    assert got["tgt_count"].tolist() == [1] and got["cells"][0, 0] == nd and got["extent_d"][0, 0] == nd


# ---- 4. adjacency limits ---------------------------------------------------------------------------
def test_adjacency_limits(engine):
    nr, nd = 64, 16
    diag = cells_to_lists([(10, 5, 3.0), (10, 4, 1.0), (11, 6, 2.0), (12, 7, 1.5)], 16)
    for link, want in (((1, 1), 1), ((1, 0), 4), ((0, 1), 3)):
        got, _ = run_and_check(engine, diag, P.ClusterConfig(link_r=link[0], link_d=link[1], max_tgt=8), nr, nd)
        assert got["tgt_count"].tolist() == [want], link
    # link (2, 3): exactly link + 1 apart stays apart, exactly link apart merges
    apart = cells_to_lists([(10, 5, 9.0), (13, 5, 8.0), (20, 5, 7.0), (20, 9, 6.0), (30, 5, 5.0), (32, 8, 4.0),
                            (40, 15, 3.0), (40, 2, 2.0), (50, 14, 1.0), (50, 2, 0.5)], 16)
    got, _ = run_and_check(engine, apart, P.ClusterConfig(link_r=2, link_d=3, max_tgt=16), nr, nd)
    assert got["tgt_count"].tolist() == [8]
    assert got["cells"][0, :8].tolist() == [1, 1, 1, 1, 2, 2, 1, 1]       # (30,5)+(32,8); (40,15)+(40,2) across the seam


def test_every_cell_its_own_cluster_at_1024(engine):
    nr, nd, n = 256, 16, 1024
    rng = np.random.default_rng(7)
    mask = np.zeros(nr * nd, bool)
    mask[rng.choice(nr * nd, n, replace=False)] = True
    power = rng.permutation(nr * nd).astype(np.float32).reshape(nr, nd) + 1
    det = with_noise(lists_of_mask(mask.reshape(nr, nd), power))
    got, ref = run_and_check(engine, det, P.ClusterConfig(link_r=0, link_d=0, max_tgt=64), nr, nd)
    assert got["tgt_count"].tolist() == [n]
    order = np.argsort(-det["det_power"][0], kind="stable")
    np.testing.assert_array_equal(got["peak_power"][0], det["det_power"][0][order[:64]])
    np.testing.assert_array_equal(got["peak_range_idx"][0], det["det_range_idx"][0][order[:64]])
    assert sorted(got["det_label"][0].tolist()) == list(range(1, n + 1))
    assert (got["cells"][0] == 1).all() and (got["extent_r"][0] == 1).all() and (got["extent_d"][0] == 1).all()
    np.testing.assert_array_equal(got["power"][0], got["peak_power"][0])
    # dense: the same cells at link (8, 7) are a handful of targets
    run_and_check(engine, det, P.ClusterConfig(link_r=8, link_d=7, max_tgt=64), nr, nd)
    run_and_check(engine, det, P.ClusterConfig(link_r=1, link_d=1, min_cells=2, max_tgt=64), nr, nd)


# ---- 5. ties and cuts ------------------------------------------------------------------------------
def test_ties_and_cuts(engine):
    nr, nd = 64, 16
    cells = [(5, 3, 4.0), (9, 9, 4.0), (20, 2, 4.0),                       # three clusters of equal peak power
             (30, 5, 7.0), (30, 6, 7.0), (31, 5, 7.0),                     # an equal maximum inside a cluster
             (40, 12, 9.0), (41, 12, 1.0), (50, 1, 0.0), (60, 8, 2.0), (60, 9, 4.0)]
    det = cells_to_lists(cells, 16)
    got, ref = run_and_check(engine, det, P.ClusterConfig(max_tgt=16), nr, nd)
    assert got["tgt_count"].tolist() == [7]
    np.testing.assert_array_equal(got["peak_power"][0, :7], np.float32([9, 7, 4, 4, 4, 4, 0]))
    # equal peak powers: by label, the smallest list index (the lists are sorted by range)
    assert got["peak_range_idx"][0, 2:6].tolist() == [5, 9, 20, 60]
    # the first of the equal maxima is the peak
    assert (got["peak_range_idx"][0, 1], got["peak_doppler_idx"][0, 1]) == (30, 5)
    # all powers 0: the centroid is the peak
    assert (got["range"][0, 6], got["doppler"][0, 6], got["power"][0, 6]) == (50.0, 1.0, 0.0)
    # cut at max_tgt: the count is complete, the arrays hold the first ones, the labels run past
    cut, _ = run_and_check(engine, det, P.ClusterConfig(max_tgt=3), nr, nd)
    assert cut["tgt_count"].tolist() == [7] and cut["det_label"].max() == 7
    _same(cut, {k: (got[k] if got[k].ndim == 1 or k == "det_label" else got[k][:, :3]) for k in OUT_KEYS})
    one, _ = run_and_check(engine, det, P.ClusterConfig(max_tgt=1), nr, nd)
    _same(one, {k: (got[k] if got[k].ndim == 1 or k == "det_label" else np.ascontiguousarray(got[k][:, :1]))
                for k in OUT_KEYS})


# ---- 6. counts ---------------------------------------------------------------------------------------
def test_counts_and_unused_entries(engine):
    nr, nd, K = 64, 16, 8
    cells = [(5, 3, 4.0), (5, 4, 5.0), (9, 9, 3.0), (20, 2, 1.0), (21, 2, 2.0), (30, 7, 6.0), (31, 8, 6.5), (40, 1, 2.5)]
    full = cells_to_lists(cells, K)
    q = P.ClusterConfig(max_tgt=6)
    frames = [dict(full, det_count=np.array([c], np.int32)) for c in (0, K + 5, -4, 3, K)]
    det = stack(*frames)
    got, ref = run_and_check(engine, det, q, nr, nd)
    assert got["tgt_count"].tolist() == [0, 5, 0, 2, 5]
    _same({k: got[k][1:2] for k in OUT_KEYS}, {k: got[k][4:5] for k in OUT_KEYS})     # a cut list: its first max_det cells
    for f in (0, 2):
        assert all(not got[k][f].any() for k in OUT_KEYS)
    assert not got["det_label"][3, 3:].any() and got["det_label"][3, :3].tolist() == [1, 1, 2]
    # the device call over buffers filled with -3 / NaN: every entry is written, unused ones are 0
    dev = device_run(engine, det, q, nr, nd)
    _same(dev, got)
    # each optional output, the noise list and the labels may be missing
    for k in R.INT_KEYS + R.FLOAT_KEYS:
        part = device_run(engine, det, q, nr, nd, leave_out=(k,))
        assert part[k] is None
        _same(part, got, [x for x in OUT_KEYS if x != k])
    part = device_run(engine, det, q, nr, nd, label=False, noise=False)
    _same(part, got, [x for x in TGT_KEYS if x != "peak_noise"])
    assert not part["peak_noise"].any()
    no_noise = engine.cluster({k: v for k, v in det.items() if k != "det_noise"}, q, nr, nd)
    _same(no_noise, got, [x for x in OUT_KEYS if x != "peak_noise"])
    assert not no_noise["peak_noise"].any()


# ---- 7. reproducibility, byte for byte --------------------------------------------------------------
def test_frames_are_independent(engine):
    geo = (64, 16, 256, 16)
    det = cfar_lists(engine, geo)
    assert len(det["det_count"]) == 12
    q = P.ClusterConfig(link_r=2, link_d=1, min_cells=1, max_tgt=8)
    whole = engine.cluster(det, q, 256, 16)
    assert whole["tgt_count"].min() > 0
    for f in range(12):
        one = engine.cluster({k: det[k][f:f + 1] for k in IN_KEYS}, q, 256, 16)
        _same(one, {k: whole[k][f:f + 1] for k in OUT_KEYS})


def test_call_sequence_shards_and_chunks(engine, monkeypatch):
    from fmcw_radar_processing_amd.engine import Engine
    a = cfar_lists(engine, (1024, 256, 1024, 256))
    b = cfar_lists(engine, (64, 16, 256, 16))
    qa = P.ClusterConfig(link_r=1, link_d=1, min_cells=2, max_tgt=16)
    qb = P.ClusterConfig(link_r=3, link_d=2, min_cells=1, max_tgt=5)
    seq, fresh, multi = Engine(0), Engine(0), Engine([0, 0, 0])
    try:
        first = seq.cluster(a, qa, 1024, 256)
        other = seq.cluster(b, qb, 256, 16)
        third = seq.cluster(a, qa, 1024, 256)
        want = fresh.cluster(a, qa, 1024, 256)
        want_b = fresh.cluster(b, qb, 256, 16)
        _same(multi.cluster(b, qb, 256, 16), want_b)
        _same(multi.cluster(a, qa, 1024, 256), want)
        monkeypatch.setenv("FMCW_HOST_CHUNK", "1")
        _same(seq.cluster(b, qb, 256, 16), want_b)
        _same(multi.cluster(b, qb, 256, 16), want_b)
        monkeypatch.delenv("FMCW_HOST_CHUNK")
    finally:
        seq.close()
        fresh.close()
        multi.close()
    _same(first, third)
    _same(first, want)
    _same(other, want_b)
    R.assert_matches(first, R.reference_of(a, qa, 256), 1024, 256)
    R.assert_matches(other, R.reference_of(b, qb, 16), 256, 16)


# ---- 8. end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,guard,train,pipe", [((1024, 256, 1024, 256), (4, 4), (4, 4), FMCW_PIPE_AUTO),
                                                  ((256, 32, 256, 32), (4, 3), (4, 4), FMCW_PIPE_STREAMS)],
                         ids=["1024x256_auto", "256x32_streams"])
def test_iq_to_targets_end_to_end(geo, guard, train, pipe):
    """IQ in, targets out on one stream (process_targets_device), frames 40-47 of the synthetic
    stream: the whole output equals the reference applied to the lists the device wrote; target 1's
    peak is the synthetic cell and its centroid lies within its extents; frame 47 has no target."""
    import torch
    from fmcw_radar_processing_amd.engine import Engine
    nts, pn, nr, nd = geo
    cfg, p, wr, wd, cal = case(nts, pn, nr, nd, P.THROUGHPUT)
    F, dev = 8, "cuda"
    iq = O.synth_frames(F, pn, nts, nr, nd, p["dist_per_bin"], frame0=40)
    qc = P.CfarConfig.for_config(cfg, pfa=1e-6, guard=guard, train=train, max_det=256)
    qt = P.ClusterConfig.for_config(cfg, link=(1, 1), min_cells=2, max_tgt=4, max_det=qc.max_det)
    K, M, T = qc.max_det, cfg.max_targets, qt.max_tgt
    eng = Engine(0)
    try:
        eng.set_taps(cfg, cal, wr, wd)
        eng.set_pipeline(pipe)
        d_iq = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32).reshape(F, pn, nts, 2)).to(dev)
        outs = dict(profile=torch.empty((F, nr), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                    tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                    tgt_range_mag=torch.empty((F, M), device=dev),
                    tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                    slow_mag=torch.empty((F, pn), device=dev))
        d_rd = torch.full((F, nr, nd, 2), np.nan, dtype=torch.float32, device=dev)
        co = dict(det_count=torch.full((F,), -3, dtype=torch.int32, device=dev),
                  det_range_idx=torch.full((F, K), -3, dtype=torch.int32, device=dev),
                  det_doppler_idx=torch.full((F, K), -3, dtype=torch.int32, device=dev),
                  det_power=torch.full((F, K), np.nan, device=dev), det_noise=torch.full((F, K), np.nan, device=dev))
        to = dict(tgt_count=torch.full((F,), -3, dtype=torch.int32, device=dev))
        for k in R.INT_KEYS:
            to[k] = torch.full((F, T), -3, dtype=torch.int32, device=dev)
        for k in R.FLOAT_KEYS:
            to[k] = torch.full((F, T), np.nan, dtype=torch.float32, device=dev)
        d_label = torch.full((F, K), -3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        eng.process_targets_device(d_iq, F, FMCW_C64, outs, qc, d_rd, co, qt, to, d_det_label=d_label,
                                   stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        eng.synchronize()
        det = {k: v.cpu().numpy() for k, v in co.items()}
        got = {k: v.cpu().numpy() for k, v in to.items()}
        got["det_label"] = d_label.cpu().numpy()
    finally:
        eng.close()
    R.assert_matches(got, R.reference_of(det, qt, nd), nr, nd)
    for i in range(F):
        fp = O.synth_frame_params(40 + i, nr, nd, p["dist_per_bin"])
        if fp["A"] == 0:
            assert i == 7 and got["tgt_count"][i] == 0
            continue
        assert got["tgt_count"][i] >= 1 and got["cells"][i, 0] >= 2
        r0, d0 = int(got["peak_range_idx"][i, 0]), int(got["peak_doppler_idx"][i, 0])
        assert (r0, d0) == (fp["r"] + 1, fp["d"] + nd // 2 + 1)
        assert abs(float(got["range"][i, 0]) - r0) < got["extent_r"][i, 0]
        dd = (float(got["doppler"][i, 0]) - d0 + nd / 2) % nd - nd / 2
        assert abs(dd) < got["extent_d"][i, 0]


# ---- 9. arguments --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REJECTED))
def test_device_call_rejects_what_the_check_rejects(engine, name):
    """E_ARG before any launch: the outputs keep their fill, timing stage cluster counts nothing."""
    over, nr, nd, max_det, _ = REJECTED[name]
    q = _lib.ClusterParams(link_r=1, link_d=1, min_cells=1, max_tgt=4, flags=0)      # the C struct: it can carry a flag bit
    for k, v in over.items():
        setattr(q, k, v)
    K = min(max(max_det, 2), 1024)              # the buffers exist; the call is given the rejected max_det
    det = cells_to_lists([(5, 3, 4.0), (5, 4, 5.0)], K)
    engine.timing_reset()
    engine.timing(1)
    try:
        with pytest.raises(FmcwError, match="E_ARG"):
            _rejected_run(engine, det, q, nr, nd, max_det)
        assert engine.timing_read()["cluster"][1] == 0
    finally:
        engine.timing(0)


def _rejected_run(engine, det, q, nr, nd, max_det):
    import torch
    dev = "cuda"
    M = min(max(q.max_tgt, 1), 64)
    d_in = {k: torch.from_numpy(det[k]).to(dev) for k in IN_KEYS}
    outs = dict(tgt_count=torch.full((1,), -3, dtype=torch.int32, device=dev))
    for k in R.INT_KEYS:
        outs[k] = torch.full((1, M), -3, dtype=torch.int32, device=dev)
    for k in R.FLOAT_KEYS:
        outs[k] = torch.full((1, M), -3.0, dtype=torch.float32, device=dev)
    d_label = torch.full((1, det["det_range_idx"].shape[1]), -3, dtype=torch.int32, device=dev)
    try:
        engine.cluster_device(q, 1, nr, nd, max_det, d_in, outs, d_det_label=d_label, stream=torch.cuda.current_stream())
    finally:
        torch.cuda.synchronize()
        for v in list(outs.values()) + [d_label]:
            assert bool((v == -3).all())


def test_device_call_arguments_and_timing(engine):
    import torch
    nr, nd = 64, 16
    det = stack(*[cells_to_lists([(5, 3, 4.0), (5, 4, 5.0), (9, 9, 3.0 + f)], 8) for f in range(3)])
    q = P.ClusterConfig(max_tgt=4)
    want = engine.cluster(det, q, nr, nd)
    # F = 0 is a no-op, F < 0 and a missing required pointer are argument errors: nothing is written
    none = device_run(engine, det, q, nr, nd, F=0)
    assert all((v == -3).all() if v.dtype == np.int32 else np.isnan(v).all() for v in none.values())
    with pytest.raises(FmcwError, match="E_ARG"):
        device_run(engine, det, q, nr, nd, F=-1)
    with pytest.raises(FmcwError, match="E_ARG"):
        device_run(engine, det, q, nr, nd, leave_out=("tgt_count",))
    # timing stage `cluster`: one event pair per launch, nothing when timing is off
    engine.timing_reset()
    _same(device_run(engine, det, q, nr, nd), want)
    assert engine.timing_read()["cluster"] == (0.0, 0)
    engine.timing(1)
    try:
        _same(device_run(engine, det, q, nr, nd), want)
        device_run(engine, det, q, nr, nd, F=1)
        engine.cluster(det, q, nr, nd)
        torch.cuda.synchronize()
        ms, n = engine.timing_read()["cluster"]
        assert n == 3 and ms > 0
    finally:
        engine.timing(0)
        engine.timing_reset()


def test_cluster_result_carries_metres_and_speed():
    """With the geometry's taps set, Engine.cluster adds range_m / speed_mps of the centroids
    (cfg.range_m, cfg.speed); NaN where unused.  Engine.targets is cfar then cluster."""
    from fmcw_radar_processing_amd.engine import Engine
    geo = (64, 16, 256, 16)
    cfg, p, wr, wd, cal = case(*geo)
    qc, qt = cfg_for(256, 1e-3, max_det=64), P.ClusterConfig(min_cells=2, max_tgt=8)
    eng = Engine(0)
    try:
        eng.set_taps(cfg, cal, wr, wd)
        got = eng.targets(rd_map(geo), qc, qt)
        det = eng.cfar(rd_map(geo), qc)
        again = eng.cluster(det, qt, 256, 16)
    finally:
        eng.close()
    _same(got, again)
    _same(got, det, IN_KEYS)
    used = got["cells"] > 0
    assert used.any() and not used.all()
    assert np.isnan(got["range_m"][~used]).all() and np.isnan(got["speed_mps"][~used]).all()
    np.testing.assert_array_equal(got["range_m"][used], cfg.range_m(got["range"][used]))
    np.testing.assert_array_equal(got["speed_mps"][used], cfg.speed(got["doppler"][used]))
    R.assert_matches(got, R.reference_of(det, qt, 16), 256, 16, keys=OUT_KEYS)
