#!/usr/bin/env python3
"""Time the clustering stage (fmcw_cluster_device: k_cluster) on the CFAR lists of config 4's RD map.

    python tools/bench_cluster.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/cluster_bench.json]

The RD buffer ([F][1024][256] complex64) is filled once on the device (fmcw_synth_device +
fmcw_process_device) and run through fmcw_cfar_device with guard (2,2), train (4,4) over every range
row, in two cases: (a) pfa 1e-6 with max_det 64, the case of DESIGN.md 4.4, and (b) pfa 1e-3 with
max_det 1024, hundreds of cells per frame.  Both lists are clustered with link (1,1), min_cells 2,
max_tgt 16, every output and det_label written: HIP events around `reps` calls after 3 warm ones.
Reported per case, from the same run: ms per call; the yardstick fmcw_copy_device over a buffer of as
many bytes as the stage reads and writes (the lists' used entries and counts in, every output array
out; the copy moves that many bytes twice); and the fmcw_cfar_device call that produced the lists.
Four frames of each case are checked against the float64 reference of tests/cluster_reference.py.
Needs an MI355X; there is no fallback.
"""
import argparse
import datetime
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def timed(fn, stream, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C64
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import cluster_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_cluster: no GPU (there is no CPU fallback)")
    dev, F = "cuda", args.frames
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    qt = P.ClusterConfig(link_r=1, link_d=1, min_cells=2, max_tgt=16)
    T = qt.max_tgt
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    outs = dict(profile=torch.empty((F, NR), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                tgt_range_mag=torch.empty((F, M), device=dev),
                tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                slow_mag=torch.empty((F, C), device=dev))
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(),
               device=torch.cuda.get_device_name(0), frames=F, nr=NR, nd=ND, guard=[2, 2], train=[4, 4], link=[1, 1],
               min_cells=qt.min_cells, max_tgt=T, reps=args.reps, cases=[])
    with torch.cuda.stream(stream):
        d_iq = torch.empty((F, C, S, 2), dtype=torch.float32, device=dev)
        d_rd = torch.empty((F, NR, ND, 2), dtype=torch.float32, device=dev)
        eng.synth_device(d_iq, 0, F, FMCW_C64, stream=stream)
        eng.process_device(d_iq, F, FMCW_C64, outs, d_rd=d_rd, out_dtype=FMCW_C64, stream=stream)
        torch.cuda.synchronize()
        eng.synchronize()
        del d_iq
        for name, pfa, K in (("a", 1e-6, 64), ("b", 1e-3, 1024)):
            qc = P.CfarConfig(guard_r=2, guard_d=2, train_r=4, train_d=4, max_det=K)
            qc.alpha = P.CfarConfig.alpha_for(qc.n_train_full, pfa)
            co = dict(det_count=torch.empty(F, dtype=torch.int32, device=dev),
                      det_range_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
                      det_doppler_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
                      det_power=torch.empty((F, K), device=dev), det_noise=torch.empty((F, K), device=dev))
            to = dict(tgt_count=torch.empty(F, dtype=torch.int32, device=dev))
            for k in R.INT_KEYS:
                to[k] = torch.empty((F, T), dtype=torch.int32, device=dev)
            for k in R.FLOAT_KEYS:
                to[k] = torch.empty((F, T), dtype=torch.float32, device=dev)
            d_label = torch.empty((F, K), dtype=torch.int32, device=dev)
            cfar_ms = timed(lambda: eng.cfar_device(qc, d_rd, FMCW_C64, F, NR, ND, co, stream=stream), stream, args.reps)
            ms = timed(lambda: eng.cluster_device(qt, F, NR, ND, K, co, to, d_det_label=d_label, stream=stream), stream,
                       args.reps)
            cnt = co["det_count"].cpu().numpy()
            n = np.clip(cnt, 0, K).astype(np.int64)
            # read: the counts, r / d / P of the used entries; written: tgt_count, ten arrays, the labels
            nbytes = int(F * 4 + 12 * n.sum() + F * 4 + 10 * F * T * 4 + F * K * 4)
            cp = (nbytes + 15) // 16 * 16
            d_a = torch.empty(cp, dtype=torch.uint8, device=dev)
            d_b = torch.empty(cp, dtype=torch.uint8, device=dev)
            copy_ms = timed(lambda: eng.copy_device(d_a, d_b, cp, stream=stream), stream, args.reps)
            del d_a, d_b
            # four frames against the float64 reference, on the list bytes the device holds; a 4-frame
            # call of its own must give the timed call's bytes
            sel = slice(0, min(4, F))
            det = {k: v[sel].cpu().numpy() for k, v in co.items()}
            got = {k: v[sel].cpu().numpy() for k, v in to.items()}
            got["det_label"] = d_label[sel].cpu().numpy()
            R.assert_matches(got, R.reference_of(det, qt, ND), NR, ND)
            to4 = {k: torch.empty_like(v[sel]) for k, v in to.items()}
            l4 = torch.empty_like(d_label[sel])
            eng.cluster_device(qt, sel.stop, NR, ND, K, {k: v[sel] for k, v in co.items()}, to4, d_det_label=l4,
                               stream=stream)
            torch.cuda.synchronize()
            for k in to4:
                assert got[k].tobytes() == to4[k].cpu().numpy().tobytes(), k
            assert got["det_label"].tobytes() == l4.cpu().numpy().tobytes()
            tc = to["tgt_count"].cpu().numpy()
            case = dict(case=name, pfa=pfa, max_det=K, cluster_ms=round(ms, 4), copy_ms=round(copy_ms, 4),
                        cfar_ms=round(cfar_ms, 4), cluster_over_copy=round(ms / copy_ms, 3),
                        cluster_over_cfar=round(ms / cfar_ms, 4), bytes_read_and_written=nbytes,
                        cells_per_frame_mean=round(float(n.mean()), 2), cells_per_frame_max=int(n.max()),
                        lists_cut=int((cnt > K).sum()), targets_per_frame_mean=round(float(tc.mean()), 2),
                        targets_per_frame_max=int(tc.max()), spot_check_frames=list(range(sel.stop)))
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
