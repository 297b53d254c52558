#!/usr/bin/env python3
"""Time the tracking stage (fmcw_track_device: k_track) on the cluster outputs of config 4's RD map.

    python tools/bench_track.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/track_bench.json]

The RD buffer ([F][1024][256] complex64) is filled once on the device (fmcw_synth_device +
fmcw_process_device), run through fmcw_cfar_device at the two settings of profiles/cluster_bench.json
(guard (2,2), train (4,4), every range row; pfa 1e-6 with max_det 64 and pfa 1e-3 with max_det 1024) and
through fmcw_cluster_device (link (1,1), min_cells 2, max_tgt 16).  The 4096 target rows are then tracked
with max_trk 16 as (a) S = 1 sequence of 4096 frames -- one wave walking a dependency chain -- and (b)
S = 64 sequences of 64 frames, every output and tgt_track written, each call from a zeroed state: HIP
events around `reps` calls after 3 warm ones.  Reported per case, from the same run: ms per call and
microseconds per frame step (ms / F: the steps of different sequences run side by side); the yardstick
fmcw_copy_device over a buffer of as many bytes as the stage reads and writes (the copy moves that many
bytes twice); and the fmcw_cluster_device and fmcw_cfar_device calls that produced the rows.  Every row
of every case is checked against the float32 reference of tests/track_reference.py.

The synthetic stream redraws its target every frame, so consecutive frames are unrelated: this times the
frame step on realistic list sizes and is no tracking scenario (tracks rarely live beyond a few frames).
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
    """fn(i) is call number i; every call gets its own i (its own zeroed state block)."""
    import torch
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for i in range(reps):
        fn(warm + i)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C64
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import cluster_reference as CR
    from tests import track_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_track: no GPU (there is no CPU fallback)")
    dev, F = "cuda", args.frames
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    qt = P.ClusterConfig(link_r=1, link_d=1, min_cells=2, max_tgt=16)
    qk = P.TrackConfig.for_config(cfg, max_trk=16, max_tgt=qt.max_tgt)
    T, N = qt.max_tgt, qk.max_trk
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    sb = eng.track_state_bytes(N)
    outs = dict(profile=torch.empty((F, NR), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                tgt_range_mag=torch.empty((F, M), device=dev),
                tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                slow_mag=torch.empty((F, C), device=dev))
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(),
               device=torch.cuda.get_device_name(0), frames=F, nr=NR, nd=ND, guard=[2, 2], train=[4, 4], link=[1, 1],
               min_cells=qt.min_cells, max_tgt=T, max_trk=N, gate=[qk.gate_r, qk.gate_d], alpha=[qk.alpha_r, qk.alpha_d],
               beta_r=qk.beta_r, confirm_hits=qk.confirm_hits, max_coast=qk.max_coast, state_bytes=sb, reps=args.reps,
               note="the synthetic stream redraws its target every frame: this times the frame step, it is no "
                    "tracking scenario", cases=[])
    with torch.cuda.stream(stream):
        d_iq = torch.empty((F, C, S, 2), dtype=torch.float32, device=dev)
        d_rd = torch.empty((F, NR, ND, 2), dtype=torch.float32, device=dev)
        eng.synth_device(d_iq, 0, F, FMCW_C64, stream=stream)
        eng.process_device(d_iq, F, FMCW_C64, outs, d_rd=d_rd, out_dtype=FMCW_C64, stream=stream)
        torch.cuda.synchronize()
        eng.synchronize()
        del d_iq
        for pfa, K in ((1e-6, 64), (1e-3, 1024)):
            qc = P.CfarConfig(guard_r=2, guard_d=2, train_r=4, train_d=4, max_det=K)
            qc.alpha = P.CfarConfig.alpha_for(qc.n_train_full, pfa)
            co = dict(det_count=torch.empty(F, dtype=torch.int32, device=dev),
                      det_range_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
                      det_doppler_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
                      det_power=torch.empty((F, K), device=dev), det_noise=torch.empty((F, K), device=dev))
            to = dict(tgt_count=torch.empty(F, dtype=torch.int32, device=dev))
            for k in CR.INT_KEYS:
                to[k] = torch.empty((F, T), dtype=torch.int32, device=dev)
            for k in CR.FLOAT_KEYS:
                to[k] = torch.empty((F, T), dtype=torch.float32, device=dev)
            cfar_ms = timed(lambda i: eng.cfar_device(qc, d_rd, FMCW_C64, F, NR, ND, co, stream=stream), stream, args.reps)
            cluster_ms = timed(lambda i: eng.cluster_device(qt, F, NR, ND, K, co, to, stream=stream), stream, args.reps)
            tg = {k: to[k].cpu().numpy() for k in R.IN_KEYS}
            n = np.clip(tg["tgt_count"], 0, T).astype(np.int64)
            ko = dict(trk_count=torch.empty(F, dtype=torch.int32, device=dev))
            for k in R.INT_KEYS:
                ko[k] = torch.empty((F, N), dtype=torch.int32, device=dev)
            for k in R.FLOAT_KEYS:
                ko[k] = torch.empty((F, N), dtype=torch.float32, device=dev)
            d_tt = torch.empty((F, T), dtype=torch.int32, device=dev)
            for name, nseq in (("a", 1), ("b", 64)):
                if F % nseq:
                    continue
                nf = F // nseq
                states = torch.zeros((args.reps + 3, nseq, sb), dtype=torch.uint8, device=dev)
                ms = timed(lambda i: eng.track_device(qk, nseq, nf, NR, ND, T, to, states[i], ko, d_tgt_track=d_tt,
                                                      stream=stream), stream, args.reps)
                # read: the counts, range / doppler / power of the used entries, the state; written:
                # trk_count, eight arrays, tgt_track, the state
                nbytes = int(F * 4 + 12 * n.sum() + F * 4 + 8 * F * N * 4 + F * T * 4 + 2 * nseq * sb)
                cp = (nbytes + 15) // 16 * 16
                d_a = torch.empty(cp, dtype=torch.uint8, device=dev)
                d_b = torch.empty(cp, dtype=torch.uint8, device=dev)
                copy_ms = timed(lambda i: eng.copy_device(d_a, d_b, cp, stream=stream), stream, args.reps)
                del d_a, d_b
                # every row against the float32 reference, on the target bytes the device holds
                got = {k: v.cpu().numpy() for k, v in ko.items()}
                got["tgt_track"] = d_tt.cpu().numpy()
                got["state"] = states[-1].cpu().numpy()
                R.assert_same(got, R.reference_of(tg, qk, NR, ND, n_seq=nseq))
                live = got["trk_status"] > 0
                case = dict(case=name, pfa=pfa, max_det=K, sequences=nseq, frames_per_sequence=nf, track_ms=round(ms, 4),
                            us_per_frame_step=round(1e3 * ms / nf, 4), copy_ms=round(copy_ms, 4),
                            cluster_ms=round(cluster_ms, 4), cfar_ms=round(cfar_ms, 4),
                            track_over_copy=round(ms / copy_ms, 2), track_over_cluster=round(ms / cluster_ms, 3),
                            track_over_cfar=round(ms / cfar_ms, 4), bytes_read_and_written=nbytes,
                            targets_per_frame_mean=round(float(n.mean()), 2), targets_per_frame_max=int(n.max()),
                            live_slots_per_frame_mean=round(float(live.sum(axis=1).mean()), 2),
                            confirmed_per_frame_mean=round(float(got["trk_count"].mean()), 3),
                            max_id=int(got["trk_id"].max()), rows_checked=F)
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
