#!/usr/bin/env python3
"""Time the clutter filter (fmcw_mti_device: k_mti + k_mti_seen) at config 4's size.

    python tools/bench_mti.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/mti_bench.json]

The RD buffer ([F][1024][256]) is filled once on the device (fmcw_synth_device + fmcw_process_device),
in complex64 and in fp16 storage.  Timed per call with HIP events, `reps` calls after 3 warm ones,
the state (bg, seen) zeroed before every call so that every call does the same work:
  out_of_place   one sequence of F frames, filtered to a second buffer
  in_place       the same, d_out == d_rd
  learn_only     d_out = NULL: the map is only read
  s64_out_of_place   64 sequences of F / 64 frames, to a second buffer
each at the ring depths 4, 8 and 16 (FMCW_MTI_RING) beside the shipped one.  The yardstick, in the
same process: fmcw_copy_device over the same RD bytes -- it reads and writes exactly what the filter
with an output reads and writes, so the ratio to aim for is 1, and 0.5 for learn_only.
Checked bit for bit against the numpy reference of tests/mti_reference.py, run over all F frames on
the RD bytes read back: frames 0, 1, F/2 and F-1 of the out-of-place output and the final bg / seen
(the frames past 2^32 bytes exercise the 64-bit offsets); the in-place and learn-only results equal
the out-of-place ones on the device; sequences 0 and 63 of the S = 64 case against the reference.
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

RINGS = (4, 8, 16)


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def timed(fn, reset, stream, reps, warm=3):
    """Mean ms of fn() over reps calls, each between its own event pair, reset() before each."""
    import torch
    for _ in range(warm):
        reset()
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        pairs.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mti_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import mti_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_mti: no GPU (there is no CPU fallback)")
    dev, F = "cuda", args.frames
    if F % 64:
        sys.exit("bench_mti: --frames must be a multiple of 64")
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    lam, flags = 0.05, R.RAMP
    q = P.MtiConfig(lam, ramp=True)
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    outs = dict(profile=torch.empty((F, NR), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                tgt_range_mag=torch.empty((F, M), device=dev),
                tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                slow_mag=torch.empty((F, C), device=dev))
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(), device=torch.cuda.get_device_name(0),
               frames=F, nr=NR, nd=ND, lambda_=lam, ramp=True, reps=args.reps, spot_check_frames=[0, 1, F // 2, F - 1],
               storages=[])
    os.environ.pop("FMCW_MTI_RING", None)
    with torch.cuda.stream(stream):
        for name, dt, tdt in (("c64", FMCW_C64, torch.float32), ("fp16", FMCW_C32H, torch.float16)):
            shipped = eng.mti_ring(dt)
            d_iq = torch.empty((F, C, S, 2), dtype=tdt, device=dev)
            d_rd = torch.empty((F, NR, ND, 2), dtype=tdt, device=dev)
            eng.synth_device(d_iq, 0, F, dt, stream=stream)
            eng.process_device(d_iq, F, dt, outs, d_rd=d_rd, out_dtype=dt, stream=stream)
            torch.cuda.synchronize()
            eng.synchronize()
            sclk, _ = eng.rdx_clock()
            del d_iq
            rd_bytes = d_rd.numel() * d_rd.element_size()
            d_out = torch.empty_like(d_rd)
            copy_ms = timed(lambda: eng.copy_device(d_rd, d_out, rd_bytes, stream=stream), lambda: None, stream, args.reps)
            d_bg = torch.zeros((64, NR, ND, 2), device=dev)
            d_seen = torch.zeros(64, dtype=torch.int32, device=dev)

            def reset():
                d_bg.zero_()
                d_seen.zero_()

            def call(nseq, out):
                eng.mti_device(q, d_rd, dt, nseq, F // nseq, NR, ND, d_bg, d_seen, d_out=out, stream=stream)

            # ---- the reference over all F frames, in chunks with the state carried (the split guarantee)
            sel = [0, 1, F // 2, F - 1]
            as_np = (lambda t: t.cpu().numpy()) if dt == FMCW_C32H else (lambda t: t.cpu().numpy().view(np.complex64)[..., 0])
            want, bg, seen = {}, None, None
            for f0 in range(0, F, 64):
                r = R.reference(as_np(d_rd[f0:f0 + 64]), lam, flags, bg=bg, seen=seen)
                bg, seen = r["bg"], r["seen"]
                for f in sel:
                    if f0 <= f < f0 + 64:
                        want[f] = r["out"][f - f0].copy()
            reset()
            call(1, d_out)
            torch.cuda.synchronize()
            for f in sel:
                assert as_np(d_out[f:f + 1])[0].tobytes() == want[f].tobytes(), f"{name}: frame {f} differs from the reference"
            bg_dev = d_bg[0].clone()
            assert bg_dev.cpu().numpy().tobytes() == np.ascontiguousarray(bg[0]).tobytes(), f"{name}: bg differs"
            assert d_seen[0].item() == int(seen[0]) == F
            # learn only: the same final state
            reset()
            call(1, None)
            torch.cuda.synchronize()
            assert torch.equal(d_bg[0].view(torch.int32), bg_dev.view(torch.int32)) and d_seen[0].item() == F
            # S = 64: sequences 0 and 63 against the reference
            reset()
            call(64, d_out)
            torch.cuda.synchronize()
            Fs = F // 64
            for s in (0, 63):
                r = R.reference(as_np(d_rd[s * Fs:(s + 1) * Fs]), lam, flags)
                assert as_np(d_out[s * Fs:(s + 1) * Fs]).tobytes() == r["out"].tobytes(), f"{name}: sequence {s} differs"
                assert d_bg[s].cpu().numpy().tobytes() == np.ascontiguousarray(r["bg"][0]).tobytes()
            assert (d_seen == Fs).all().item()

            entry = dict(storage=name, rd_bytes=rd_bytes, shipped_ring=shipped, copy_ms=round(copy_ms, 4),
                         copy_TBps=round(2 * rd_bytes / copy_ms / 1e9, 3), shader_clock_mhz_of_the_fill=round(sclk, 1),
                         reference_frames_equal=True, cases=[])
            for label, nseq, form in (("out_of_place", 1, "out"), ("learn_only", 1, "learn"), ("s64_out_of_place", 64, "out"),
                                      ("in_place", 1, "inplace")):
                if form == "inplace":                        # last: it overwrites the map.  Its first call, checked:
                    d_chk = d_out
                    reset()
                    call(1, d_chk)
                    reset()
                    call(1, d_rd)
                    torch.cuda.synchronize()
                    assert torch.equal(d_rd.view(torch.int16), d_chk.view(torch.int16)), f"{name}: in place differs"
                    assert torch.equal(d_bg[0].view(torch.int32), bg_dev.view(torch.int32))
                target = dict(out=d_out, learn=None, inplace=d_rd)[form]
                goal = 0.5 if form == "learn" else 1.0
                for rg in (shipped,) + tuple(r for r in RINGS if r != shipped):
                    os.environ["FMCW_MTI_RING"] = str(rg)
                    assert eng.mti_ring(dt) == rg
                    ms = timed(lambda: call(nseq, target), reset, stream, args.reps)
                    moved = rd_bytes * (1 if form == "learn" else 2)
                    case = dict(case=label, sequences=nseq, frames_per_sequence=F // nseq, ring=rg, shipped=rg == shipped,
                                mti_ms=round(ms, 4), mti_over_copy=round(ms / copy_ms, 3), goal_over_copy=goal,
                                meets_goal=bool(ms <= goal * copy_ms), bytes_moved=moved, TBps=round(moved / ms / 1e9, 3))
                    entry["cases"].append(case)
                    print(json.dumps(dict(storage=name, copy_ms=round(copy_ms, 4), **case)), flush=True)
                os.environ.pop("FMCW_MTI_RING", None)
            res["storages"].append(entry)
            del d_rd, d_out, d_bg, d_seen
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
