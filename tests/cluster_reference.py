"""float64 reference of the clustering stage (include/fmcw.h, fmcw_cluster_params), written from its
definition; test-side code (the library's kernel is csrc/kernels_cluster.hip).

The partition is found by a breadth-first search over the link relation (the kernel propagates
minimum labels), on exactly the list bytes the device is given.  Everything that is decided by
integers or by comparisons of stored float32 values -- the partition, cells, the extents, the peak,
peak_power, peak_noise, tgt_count, the order, det_label -- is compared exactly; power and the two
centroids, which the device forms as n-term float32 sums, within

  power    rtol (n + 8) 2^-24
  range    (n + 8) 2^-24 (1 + max |r_i - r_pk|) + 2^-23 nr        absolute
  doppler  (n + 8) 2^-24 (1 + max |delta_i|) + 2^-23 nd           absolute, difference taken mod nd

with n the cluster's cell count.  All indices are 1-based, as in the library's outputs.
"""
from __future__ import annotations

from collections import deque

import numpy as np

U = 2.0 ** -24
INT_KEYS = ("cells", "peak_range_idx", "peak_doppler_idx", "extent_r", "extent_d")
FLOAT_KEYS = ("peak_power", "peak_noise", "power", "range", "doppler")


def link_matrix(r, d, nd, link) -> np.ndarray:
    """[n][n] bool: cells i, j are linked (every cell with itself)."""
    r = np.asarray(r, np.int64)
    d = np.asarray(d, np.int64)
    dr = np.abs(r[:, None] - r[None, :])
    dd = np.abs(d[:, None] - d[None, :])
    return (dr <= link[0]) & (np.minimum(dd, nd - dd) <= link[1])


def components(r, d, nd, link) -> np.ndarray:
    """label[i] = the smallest list index of the connected component of cell i (0-based), by BFS."""
    n = len(r)
    adj = link_matrix(r, d, nd, link)
    label = np.full(n, -1, np.int64)
    for s in range(n):
        if label[s] >= 0:
            continue
        label[s] = s                      # cells are visited in ascending order: s is its component's smallest
        todo = deque([s])
        while todo:
            i = todo.popleft()
            for j in np.nonzero(adj[i] & (label < 0))[0]:
                label[j] = s
                todo.append(j)
    return label


def cluster_reference(det_count, det_range_idx, det_doppler_idx, det_power, det_noise, nd, link, min_cells,
                      max_tgt) -> dict:
    """The library's outputs from the definition.  Returns tgt_count [F], the [F][max_tgt] arrays
    (INT_KEYS int64, peak_power / peak_noise float32, power / range / doppler float64), det_label
    [F][max_det], and for the tolerances tol_n, tol_r (max |r_i - r_pk|), tol_d (max |delta_i|)."""
    det_count = np.asarray(det_count)
    ridx, didx = np.asarray(det_range_idx, np.int64), np.asarray(det_doppler_idx, np.int64)
    power = np.asarray(det_power)
    assert power.dtype == np.float32
    F, K = ridx.shape
    M = max_tgt
    out = dict(tgt_count=np.zeros(F, np.int64), det_label=np.zeros((F, K), np.int64))
    for k in INT_KEYS + ("tol_n", "tol_r", "tol_d"):
        out[k] = np.zeros((F, M), np.int64)
    for k in ("peak_power", "peak_noise"):
        out[k] = np.zeros((F, M), np.float32)
    for k in ("power", "range", "doppler"):
        out[k] = np.zeros((F, M), np.float64)
    for f in range(F):
        n = int(min(max(int(det_count[f]), 0), K))
        r, d, p = ridx[f, :n], didx[f, :n], power[f, :n]
        label = components(r, d, nd, link)
        tg = []
        for root in np.unique(label):
            mem = np.nonzero(label == root)[0]            # ascending list order
            if len(mem) < min_cells:
                continue
            pk = mem[np.argmax(p[mem])]                   # the first of equal maxima
            tg.append((root, mem, pk))
        tg.sort(key=lambda t: (-float(p[t[2]]), t[0]))    # peak power descending, label ascending
        out["tgt_count"][f] = len(tg)
        for pos, (root, mem, pk) in enumerate(tg):
            out["det_label"][f, mem] = pos + 1
            if pos >= M:
                continue
            pm = p[mem].astype(np.float64)
            delta = (d[mem] - d[pk] + nd // 2) % nd - nd // 2
            tot = pm.sum()
            rng = float(r[pk]) + (float((pm * (r[mem] - r[pk])).sum() / tot) if tot > 0 else 0.0)
            dop = float(d[pk]) + (float((pm * delta).sum() / tot) if tot > 0 else 0.0)
            if dop < 0.5:
                dop += nd
            elif dop >= nd + 0.5:
                dop -= nd
            out["cells"][f, pos] = len(mem)
            out["peak_range_idx"][f, pos] = r[pk]
            out["peak_doppler_idx"][f, pos] = d[pk]
            out["extent_r"][f, pos] = r[mem].max() - r[mem].min() + 1
            out["extent_d"][f, pos] = delta.max() - delta.min() + 1
            out["peak_power"][f, pos] = p[pk]
            out["peak_noise"][f, pos] = 0.0 if det_noise is None else np.asarray(det_noise)[f, pk]
            out["power"][f, pos] = tot
            out["range"][f, pos] = rng
            out["doppler"][f, pos] = dop
            out["tol_n"][f, pos] = len(mem)
            out["tol_r"][f, pos] = np.abs(r[mem] - r[pk]).max()
            out["tol_d"][f, pos] = np.abs(delta).max()
    return out


def reference_of(det: dict, q, nd) -> dict:
    """The reference on a dict of detection lists (Engine.cfar's, or a test's) for a ClusterConfig."""
    return cluster_reference(det["det_count"], det["det_range_idx"], det["det_doppler_idx"], det["det_power"],
                             det.get("det_noise"), nd, (q.link_r, q.link_d), q.min_cells, q.max_tgt)


def assert_matches(got: dict, ref: dict, nr: int, nd: int, keys=None) -> None:
    """The library's outputs against the reference (the module's docstring has the rules).  `keys`:
    the outputs to compare (default: all that `got` holds)."""
    have = [k for k in ("tgt_count", "det_label") + INT_KEYS + FLOAT_KEYS if k in got and got[k] is not None]
    for k in have if keys is None else keys:
        g = np.asarray(got[k])
        if k in ("tgt_count", "det_label") or k in INT_KEYS:
            assert g.dtype == np.int32, k
            np.testing.assert_array_equal(g, ref[k], err_msg=k)
        elif k in ("peak_power", "peak_noise"):
            assert g.dtype == np.float32, k
            assert g.tobytes() == ref[k].tobytes(), k          # the stored float32 values, bit for bit
        else:
            assert g.dtype == np.float32, k
            used = ref["cells"] > 0
            assert np.all(g[~used] == 0), k
            n = ref["tol_n"][used].astype(np.float64)
            w, gg = ref[k][used], g[used].astype(np.float64)
            if k == "power":
                err, tol = np.abs(gg - w), (n + 8) * U * w
            elif k == "range":
                err, tol = np.abs(gg - w), (n + 8) * U * (1 + ref["tol_r"][used]) + 2.0 ** -23 * nr
            else:
                err = np.abs((gg - w + nd / 2) % nd - nd / 2)   # circular: a fold within rounding cannot fail
                tol = (n + 8) * U * (1 + ref["tol_d"][used]) + 2.0 ** -23 * nd
                assert np.all((gg >= 0.5) & (gg < nd + 0.5)), k
            assert np.all(err <= tol), (k, float((err - tol).max()))
