#!/usr/bin/env python3
"""Time the 2-D CA-CFAR stage (fmcw_cfar_device: k_cfar + k_cfar_gather) at config 4's size.

    python tools/bench_cfar.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/cfar_bench.json]

The RD buffer ([F][1024][256]) is filled once on the device (fmcw_synth_device + fmcw_process_device),
in complex64 and in fp16 storage.  cfar_device runs with guard (2,2), train (4,4), max_det 64 and alpha
for pfa 1e-6, over every range row (the yardstick case) and over the peak rule's gate (where only the
gated rows and their window rows are read), with and without the mask: HIP events around `reps` launches
after 3 warm ones.  Reported per case: ms per call, the algorithmic bytes (the rows read once plus
the outputs), their share of the 8 TB/s HBM peak, and in the same process the yardstick: fmcw_copy_device
on the same RD bytes (it reads and writes them: twice the bytes, so a CFAR that reads its input once and
stays memory-bound finishes within the copy's time).  Four frames are checked against the float64
reference of tests/cfar_reference.py.  Needs an MI355X; there is no fallback.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfar_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import cfar_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_cfar: no GPU (there is no CPU fallback)")
    dev, F = "cuda", args.frames
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    K = 64
    q = P.CfarConfig.for_config(cfg, pfa=1e-6, guard=(2, 2), train=(4, 4), max_det=K)
    gate_pk = (q.r_lo, q.r_hi)
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    outs = dict(profile=torch.empty((F, NR), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                tgt_range_mag=torch.empty((F, M), device=dev),
                tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                slow_mag=torch.empty((F, C), device=dev))
    co = dict(det_count=torch.empty(F, dtype=torch.int32, device=dev),
              det_range_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
              det_doppler_idx=torch.empty((F, K), dtype=torch.int32, device=dev),
              det_power=torch.empty((F, K), device=dev), det_noise=torch.empty((F, K), device=dev))
    d_mask = torch.empty((F, NR, ND), dtype=torch.uint8, device=dev)
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(), device=torch.cuda.get_device_name(0),
               frames=F, nr=NR, nd=ND, guard=[2, 2], train=[4, 4], max_det=K, peak_rule_gate=[q.r_lo, q.r_hi], alpha=q.alpha,
               reps=args.reps, hbm_peak_TBps=HBM_PEAK / 1e12, cases=[])
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
            for gate, with_mask in ((g, m) for g in ("all", "peak_rule") for m in (False, True)):
                # every row (the yardstick case: the whole map is read once), and the peak rule's gate,
                # where only the gated rows and their window rows are read
                q.r_lo, q.r_hi = (0, 0) if gate == "all" else gate_pk
                mk = d_mask if with_mask else None
                ms = timed(lambda: eng.cfar_device(q, d_rd, dt, F, NR, ND, co, d_mask=mk, stream=stream), stream,
                           args.reps)
                Wr = q.guard_r + q.train_r
                rows = NR if gate == "all" else min(NR, q.r_hi + Wr) - max(1, q.r_lo - Wr) + 1
                nbytes = rd_bytes // NR * rows + F * (4 + K * 16) + (F * NR * ND if with_mask else 0)
                # the whole gate's windows, checked on 4 frames against the float64 reference
                # (a 4-frame call of its own with a mask: the lists of the timed call must equal it bit for bit)
                sel = list(range(min(4, F)))
                got = {k: v[sel].cpu().numpy() for k, v in co.items()}
                co4 = {k: torch.empty_like(v[sel]) for k, v in co.items()}
                m4 = torch.empty((len(sel), NR, ND), dtype=torch.uint8, device=dev)
                eng.cfar_device(q, d_rd[sel[0]:sel[-1] + 1], dt, len(sel), NR, ND, co4, d_mask=m4, stream=stream)
                torch.cuda.synchronize()
                for k in got:
                    assert got[k].tobytes() == co4[k].cpu().numpy().tobytes(), k
                rd_h = d_rd[sel[0]:sel[-1] + 1].cpu().numpy()
                rd_h = rd_h.view(np.complex64)[..., 0] if dt == FMCW_C64 else rd_h
                ref = R.cfar_reference(rd_h, (2, 2), (4, 4), q.alpha, q.r_lo, q.r_hi)
                R.assert_matches(got, ref, K, m4.cpu().numpy())
                case = dict(storage=name, gate=gate, rows_read=rows, mask=with_mask, cfar_ms=round(ms, 4),
                            copy_ms=round(copy_ms, 4),
                            cfar_over_copy=round(ms / copy_ms, 3), algorithmic_bytes=nbytes,
                            algorithmic_TBps=round(nbytes / ms / 1e9, 3),
                            share_of_hbm_peak=round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                            copy_TBps=round(2 * rd_bytes / copy_ms / 1e9, 3), within_copy_time=bool(ms <= copy_ms),
                            shader_clock_mhz_of_the_fill=round(sclk, 1),
                            detections_total=int(co["det_count"].sum().item()), spot_check_frames=sel)
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
