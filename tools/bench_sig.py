#!/usr/bin/env python3
"""Time the signature stage (fmcw_sig_device: k_sig + k_sig_gather) at config 4's size.

    python tools/bench_sig.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/sig_bench.json]

The RD buffer ([F][1024][256]) is filled once on the device (fmcw_synth_device + fmcw_process_device),
in complex64 and in fp16 storage.  signature_device runs over every range row with both maps (the
yardstick case: the whole map is read once), over every row with the Doppler-time map only, and with
the tracked gate (track_half 2 about each frame's strongest target, dc_half 0): HIP events around
`reps` launches after 3 warm ones.  Reported per case: ms per call, the algorithmic bytes (the rows
read once plus the outputs), their share of the 8 TB/s HBM peak, and in the same process the
yardstick: fmcw_copy_device on the same RD bytes (it reads and writes them: twice the bytes, so a pass
that reads its input once and stays memory-bound finishes within the copy's time).  Four frames of
each case are checked against the float64 reference of tests/sig_reference.py.  Needs an MI355X;
there is no fallback.
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

HBM_PEAK = 8.0e12


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sig_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import sig_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_sig: no GPU (there is no CPU fallback)")
    dev, F = "cuda", args.frames
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    q_trk = P.SigConfig.for_config(cfg, track_half=2, dc_half=0)
    cases = (("all_rows_both_maps", P.SigConfig(dc_half=0), ("doppler_time", "range_time"), False),
             ("all_rows_doppler_time_only", P.SigConfig(dc_half=0), ("doppler_time",), False),
             ("tracked_gate_h2", q_trk, ("doppler_time", "range_time"), True))
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    outs = dict(profile=torch.empty((F, NR), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                tgt_range_mag=torch.empty((F, M), device=dev),
                tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                slow_mag=torch.empty((F, C), device=dev))
    d_dt, d_rt = torch.empty((F, ND), device=dev), torch.empty((F, NR), device=dev)
    d_mx = torch.zeros(2, device=dev)
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(), device=torch.cuda.get_device_name(0),
               frames=F, nr=NR, nd=ND, tracked_gate=[q_trk.r_lo, q_trk.r_hi], track_half=2, dc_half=0, reps=args.reps,
               hbm_peak_TBps=HBM_PEAK / 1e12, cases=[])
    with torch.cuda.stream(stream):
        for name, dt, tdt in (("c64", FMCW_C64, torch.float32), ("fp16", FMCW_C32H, torch.float16)):
            d_iq = torch.empty((F, C, S, 2), dtype=tdt, device=dev)
            d_rd = torch.empty((F, NR, ND, 2), dtype=tdt, device=dev)
            eng.synth_device(d_iq, 0, F, dt, stream=stream)
            eng.process_device(d_iq, F, dt, outs, d_rd=d_rd, out_dtype=dt, stream=stream)
            torch.cuda.synchronize()
            eng.synchronize()
            sclk, _ = eng.rdx_clock()
            del d_iq
            rd_bytes = d_rd.numel() * d_rd.element_size()
            d_cp = torch.empty_like(d_rd)
            copy_ms = timed(lambda: eng.copy_device(d_rd, d_cp, rd_bytes, stream=stream), stream, args.reps)
            del d_cp
            ctr_h = outs["tgt_range_idx"].cpu().numpy()
            for label, q, maps, tracked in cases:
                p_dt = d_dt if "doppler_time" in maps else None
                p_rt = d_rt if "range_time" in maps else None
                ctr = outs["tgt_range_idx"] if tracked else None

                def run(rd=d_rd, n=F, o_dt=p_dt, o_rt=p_rt, c=ctr):
                    eng.signature_device(q, rd, dt, n, NR, ND, o_dt, o_rt, d_mx[0:1], d_mx[1:2], d_center=c,
                                         center_stride=M, stream=stream)
                d_mx.zero_()
                ms = timed(run, stream, args.reps)
                # rows read: the whole map, or each frame's window
                ref_rows = [R.frame_rows(NR, q.r_lo, q.r_hi, ctr_h[f, 0] if tracked else None, q.track_half)
                            for f in range(F)]
                rows = sum(rb - ra for ra, rb in ref_rows)
                nbytes = rd_bytes // (F * NR) * rows + F * 4 * ((ND if p_dt is not None else 0) + (NR if p_rt is not None else 0))
                # four frames against the float64 reference; a 4-frame call of its own must give the timed call's bits
                sel = 4 if F >= 4 else F
                got = {k: v[:sel].cpu().numpy() for k, v in (("doppler_time", p_dt), ("range_time", p_rt)) if v is not None}
                full_mx = d_mx.cpu().numpy().copy()
                got4 = {k: torch.empty_like(v[:sel]) for k, v in (("doppler_time", p_dt), ("range_time", p_rt)) if v is not None}
                mx4 = torch.zeros(2, device=dev)
                eng.signature_device(q, d_rd[:sel], dt, sel, NR, ND, got4.get("doppler_time"), got4.get("range_time"),
                                     mx4[0:1], mx4[1:2], d_center=None if ctr is None else ctr[:sel], center_stride=M,
                                     stream=stream)
                torch.cuda.synchronize()
                for k in got:
                    assert got[k].tobytes() == got4[k].cpu().numpy().tobytes(), k
                rd_h = d_rd[:sel].cpu().numpy()
                rd_h = rd_h.view(np.complex64)[..., 0] if dt == FMCW_C64 else rd_h
                ref = R.sig_reference(rd_h, q.r_lo, q.r_hi, q.dc_half, ctr_h[:sel] if tracked else None, M, q.track_half)
                chk = dict(got, dt_max=mx4[0].item(), rt_max=mx4[1].item())
                R.assert_matches(chk, ref, maps=maps)
                if p_dt is not None:
                    assert full_mx[0] == p_dt.max().item()
                if p_rt is not None:
                    assert full_mx[1] == p_rt.max().item()
                case = dict(storage=name, case=label, maps=list(maps), rows_read=rows, sig_ms=round(ms, 4),
                            copy_ms=round(copy_ms, 4), sig_over_copy=round(ms / copy_ms, 3), algorithmic_bytes=nbytes,
                            algorithmic_TBps=round(nbytes / ms / 1e9, 3),
                            share_of_hbm_peak=round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                            copy_TBps=round(2 * rd_bytes / copy_ms / 1e9, 3), within_copy_time=bool(ms <= copy_ms),
                            shader_clock_mhz_of_the_fill=round(sclk, 1), frames_with_a_target=int(sum(rb > ra for ra, rb in ref_rows)),
                            spot_check_frames=list(range(sel)))
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
            del d_rd
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
