#!/usr/bin/env python3
"""Time the angle-of-arrival stage (fmcw_aoa_device: k_aoa) on the CFAR lists of config 4's RD map.

    python tools/bench_aoa.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/aoa_bench.json]

The RD buffer ([F][1024][256] complex64) is filled once on the device (fmcw_synth_device +
fmcw_process_device); channel a is that map turned by 0.6 a rad (torch, set-up only), kept as
complex64 and as fp16 storage (D / (nr nd)).  The lists come from fmcw_cfar_device on channel 0 with
guard (2,2), train (4,4) over every range row, in two cases: (a) pfa 1e-6 with max_det 64 and (b)
pfa 1e-3 with max_det 1024, as in tools/bench_cluster.py; the labels from fmcw_cluster_device with
link (1,1), min_cells 2, max_tgt 16.  The stage runs with A = 2 and A = 4 channels, both storages,
max_tgt 16, every output written: HIP events around `reps` calls after 3 warm ones.
Reported per case, from the same run: ms per call; the yardstick fmcw_copy_device over a buffer of as
many bytes as the stage reads and writes (the cells' A stored values, the counts and the used entries
of the two index lists and the labels in, every output array out; the copy moves that many bytes
twice); and the fmcw_cfar_device and fmcw_cluster_device calls that produced the lists.  Four frames
of each case are checked against the float32 reference of tests/aoa_reference.py.
Needs an MI355X; there is no fallback.
"""
import argparse
import datetime
import json
import math
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aoa_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import aoa_reference as R
    from tests import cluster_reference as CL

    if not torch.cuda.is_available():
        sys.exit("bench_aoa: no GPU (there is no CPU fallback)")
    dev, F = "cuda", args.frames
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    qt = P.ClusterConfig(link_r=1, link_d=1, min_cells=2, max_tgt=16)
    T, AMAX = qt.max_tgt, 4
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
        # the channels: the map and turned copies of it, in both storages (set-up, not timed)
        maps = {FMCW_C64: [d_rd], FMCW_C32H: []}
        z = torch.view_as_complex(d_rd)
        for a in range(1, AMAX):
            maps[FMCW_C64].append(torch.view_as_real(z * complex(math.cos(0.6 * a), math.sin(0.6 * a))).contiguous())
        for m in maps[FMCW_C64]:
            maps[FMCW_C32H].append((m / float(NR * ND)).to(torch.float16))
        del z
        torch.cuda.synchronize()
        for name, pfa, K in (("a", 1e-6, 64), ("b", 1e-3, 1024)):
            qc = P.CfarConfig(guard_r=2, guard_d=2, train_r=4, train_d=4, max_det=K)
            qc.alpha = P.CfarConfig.alpha_for(qc.n_train_full, pfa)
            co = dict(det_count=torch.empty(F, dtype=torch.int32, device=dev),
                      det_range_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
                      det_doppler_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
                      det_power=torch.empty((F, K), device=dev), det_noise=torch.empty((F, K), device=dev))
            to = dict(tgt_count=torch.empty(F, dtype=torch.int32, device=dev))
            for k in CL.INT_KEYS:
                to[k] = torch.empty((F, T), dtype=torch.int32, device=dev)
            for k in CL.FLOAT_KEYS:
                to[k] = torch.empty((F, T), dtype=torch.float32, device=dev)
            d_label = torch.empty((F, K), dtype=torch.int32, device=dev)
            cfar_ms = timed(lambda: eng.cfar_device(qc, d_rd, FMCW_C64, F, NR, ND, co, stream=stream), stream, args.reps)
            cluster_ms = timed(lambda: eng.cluster_device(qt, F, NR, ND, K, co, to, d_det_label=d_label, stream=stream),
                               stream, args.reps)
            cnt = co["det_count"].cpu().numpy()
            n = np.clip(cnt, 0, K).astype(np.int64)
            ao = {k: torch.empty((F, K), dtype=torch.float32, device=dev) for k in R.DET_KEYS}
            for k in R.TGT_KEYS:
                ao[k] = torch.empty((F, T), dtype=torch.int32 if k == "tgt_cells" else torch.float32, device=dev)
            sel = slice(0, min(4, F))
            det = {k: co[k][sel].cpu().numpy() for k in ("det_count", "det_range_idx", "det_doppler_idx")}
            lab = d_label[sel].cpu().numpy()
            for dt, dname, esz in ((FMCW_C64, "complex64", 8), (FMCW_C32H, "fp16", 4)):
                for A in (2, AMAX):
                    qa = P.AoaConfig(n_chan=A, spacing=0.5, max_tgt=T)
                    chans = maps[dt][:A]
                    ms = timed(lambda: eng.aoa_device(qa, chans, dt, F, NR, ND, K, co, ao, d_det_label=d_label,
                                                      stream=stream), stream, args.reps)
                    # read: the cells' A stored values, the counts, r / d / label of the used entries;
                    # written: four per-cell and eight per-target arrays
                    nbytes = int(A * esz * n.sum() + F * 4 + 12 * n.sum() + 4 * F * K * 4 + 8 * F * T * 4)
                    cp = (nbytes + 15) // 16 * 16
                    d_a = torch.empty(cp, dtype=torch.uint8, device=dev)
                    d_b = torch.empty(cp, dtype=torch.uint8, device=dev)
                    copy_ms = timed(lambda: eng.copy_device(d_a, d_b, cp, stream=stream), stream, args.reps)
                    del d_a, d_b
                    # four frames against the float32 reference, on the bytes the device holds
                    got = {k: v[sel].cpu().numpy() for k, v in ao.items()}
                    host = [c[sel].cpu().numpy() for c in chans]
                    if dt == FMCW_C64:
                        host = [np.ascontiguousarray(h).view(np.complex64)[..., 0] for h in host]
                    pool = []
                    R.assert_matches(got, R.reference_of(host, det, qa, labels=lab), qa.kinv, pool=pool)
                    e_dev, e_np, bound = R.phase_check_pool(pool, f"case {name} {dname} A = {A}")
                    case = dict(case=name, pfa=pfa, max_det=K, storage=dname, channels=A, aoa_ms=round(ms, 4),
                                copy_ms=round(copy_ms, 4), cfar_ms=round(cfar_ms, 4), cluster_ms=round(cluster_ms, 4),
                                aoa_over_copy=round(ms / copy_ms, 3), aoa_over_cfar=round(ms / cfar_ms, 4),
                                bytes_read_and_written=nbytes, cells_per_frame_mean=round(float(n.mean()), 2),
                                cells_per_frame_max=int(n.max()), lists_cut=int((cnt > K).sum()),
                                phase_ulps_device=round(e_dev, 3), phase_ulps_numpy=round(e_np, 3),
                                spot_check_frames=list(range(sel.stop)))
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
