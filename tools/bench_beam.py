#!/usr/bin/env python3
"""Time the channel-combining stage (fmcw_beam_device: k_beam) at config 4's size.

    python tools/bench_beam.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/beam_bench.json]

One RD map ([F][1024][256]) is filled on the device (fmcw_synth_device + fmcw_process_device), in
complex64 and in fp16 storage; channel a is that map turned by 0.6 a rad, formed on the device.  All
maps are slices of one allocation of 16: the channels in the first eight, the outputs in the last
eight.  If 16 maps of F frames do not fit the card's free memory, the largest multiple of 64 frames
that does is used and recorded.  Timed per call with HIP events, `reps` calls after 3 warm ones:
  (A, B) = (2, 1) coherent, (2, 1) NCI, (4, 1), (4, 4), (8, 1), (8, 8) out of place, and (2, 1) coherent
  in place (out[0] == rd[0]).
The yardstick, in the same run: fmcw_copy_device over (A + B) / 2 maps' bytes -- it reads and writes
exactly the bytes the stage reads and writes, so the ratio to aim for is 1.
Checked bit for bit against the numpy reference of tests/beam_reference.py on the channel bytes read
back: frames 0, F/2 + 1 and F - 1 of every output of every case (in complex64 frame F/2 + 1 lies past
2^32 bytes of its map, which exercises the 64-bit offsets; in fp16 storage the whole map is 2^32
bytes at F = 4096 and the last frame ends there); the in-place result equals the out-of-place one on
the device.  Needs an MI355X; there is no fallback.
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

CASES = (("a2_b1", 2, 1, False), ("a2_b1_nci", 2, 1, True), ("a4_b1", 4, 1, False), ("a4_b4", 4, 4, False),
         ("a8_b1", 8, 1, False), ("a8_b8", 8, 8, False))
PSI = 0.6                      # rad per channel
SLOTS = 16                     # maps in the allocation


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def timed(fn, stream, reps, warm=3):
    """Mean ms of fn() over reps calls, each between its own event pair."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import beam_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_beam: no GPU (there is no CPU fallback)")
    dev = "cuda"
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(), device=torch.cuda.get_device_name(0),
               frames_asked=args.frames, nr=NR, nd=ND, psi_rad_per_channel=PSI, reps=args.reps, storages=[])
    with torch.cuda.stream(stream):
        for name, dt, tdt in (("c64", FMCW_C64, torch.float32), ("fp16", FMCW_C32H, torch.float16)):
            esz = 4 if dt == FMCW_C64 else 2
            fbytes = NR * ND * 2 * esz
            free, _ = torch.cuda.mem_get_info()
            # the allocation of 16 maps, the IQ of the fill and its outputs, with a tenth to spare
            per_frame = SLOTS * fbytes + C * S * 2 * esz + 64 * (NR + C + 4 * M)
            F = min(args.frames, int(0.9 * free / per_frame) // 64 * 64)
            if F < 64:
                sys.exit("bench_beam: not enough device memory")
            outs = dict(profile=torch.empty((F, NR), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                        tgt_range_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                        tgt_range_mag=torch.empty((F, M), device=dev),
                        tgt_doppler_idx=torch.empty((F, M), dtype=torch.int32, device=dev),
                        slow_mag=torch.empty((F, C), device=dev))
            maps = torch.empty((SLOTS, F, NR, ND, 2), dtype=tdt, device=dev)
            d_iq = torch.empty((F, C, S, 2), dtype=tdt, device=dev)
            eng.synth_device(d_iq, 0, F, dt, stream=stream)
            eng.process_device(d_iq, F, dt, outs, d_rd=maps[0], out_dtype=dt, stream=stream)
            torch.cuda.synchronize()
            eng.synchronize()
            del d_iq, outs
            for a in range(1, 8):                               # channel a = the map turned by PSI a rad
                rot = torch.tensor(complex(np.cos(PSI * a), np.sin(PSI * a)), dtype=torch.complex64, device=dev)
                for f0 in range(0, F, 128):
                    z = torch.view_as_complex(maps[0, f0:f0 + 128].float().contiguous()) * rot
                    maps[a, f0:f0 + 128] = torch.view_as_real(z).to(tdt)
            maps[8:].zero_()
            torch.cuda.synchronize()
            map_bytes = F * fbytes
            sel = sorted({0, min(F // 2 + 1, F - 1), F - 1})

            def host(t):
                h = t.cpu().numpy()
                return h if dt == FMCW_C32H else np.ascontiguousarray(h).view(np.complex64)[..., 0]
            chans_sel = [host(maps[a, sel]) for a in range(8)]
            entry = dict(storage=name, frames=F, frames_cut_to_fit=F < args.frames, map_bytes=map_bytes, checked_frames=sel,
                         reference_frames_equal=True, cases=[])
            first_out = None
            for label, A, B, nci in CASES + (("a2_b1_in_place", 2, 1, False),):
                inplace = label.endswith("in_place")
                sins = [PSI / np.pi + 0.25 * b for b in range(B)]
                sins = [s - 2 if s > 1 else s for s in sins]
                q = P.BeamConfig(Engine.beam_weights(A, sins, 0.5), nci=nci)
                d_in = [maps[a] for a in range(A)]
                d_out = [maps[0]] if inplace else [maps[8 + b] for b in range(B)]
                # the yardstick: (A + B) / 2 maps' bytes from the slots that end at slot 8 into the slots from 8 on
                # (the outputs' own, not yet written; channels 0 .. A-1 are not touched where A + B <= 8, and
                # only read otherwise)
                half_bytes = (A + B) * map_bytes // 2
                flat = maps.view(-1)
                per_map = flat.numel() // SLOTS

                def copy():                                   # one launch moves at most 2^34 bytes
                    s0, d0 = (8 - (A + B + 1) // 2) * per_map, 8 * per_map
                    for off in range(0, half_bytes, 1 << 34):
                        n = min(1 << 34, half_bytes - off)
                        eng.copy_device(flat[s0 + off // esz:], flat[d0 + off // esz:], n, stream=stream)
                copy_ms = timed(copy, stream, args.reps)

                def call():
                    eng.beam_device(q, d_in, dt, F, NR, ND, d_out, stream=stream)
                call()
                torch.cuda.synchronize()
                want = R.reference(chans_sel[:A], q.weights_f32(), nci)
                for b in range(B):
                    got = host(d_out[b][sel])
                    assert got.tobytes() == want[b].tobytes(), f"{name} {label}: beam {b} differs from the reference"
                if label == "a2_b1":
                    first_out = maps[8].clone()
                if inplace:
                    assert torch.equal(maps[0].view(torch.int16), first_out.view(torch.int16)), f"{name}: in place differs"
                ms = timed(call, stream, args.reps)
                moved = (A + B) * map_bytes
                case = dict(case=label, n_chan=A, n_beam=B, nci=nci, in_place=inplace, beam_ms=round(ms, 4),
                            copy_ms=round(copy_ms, 4), beam_over_copy=round(ms / copy_ms, 3), meets_copy_time=bool(ms <= copy_ms),
                            bytes_moved=moved, TBps=round(moved / ms / 1e9, 3), copy_TBps=round(moved / copy_ms / 1e9, 3),
                            gflop=round(F * NR * ND * (A * B * 8 - 2 * B if not nci else A * 9) / 1e9, 2))
                entry["cases"].append(case)
                print(json.dumps(dict(storage=name, frames=F, **case)), flush=True)
            res["storages"].append(entry)
            del maps, first_out
            torch.cuda.empty_cache()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
