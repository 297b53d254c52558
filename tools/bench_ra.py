#!/usr/bin/env python3
"""Time the range-angle stage (fmcw_cov_device: k_cov, fmcw_ra_device: k_ra) at config 4's size.

    python tools/bench_ra.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/ra_bench.json]

One RD map ([F][1024][256]) is filled on the device (fmcw_synth_device + fmcw_process_device), in
complex64 and in fp16 storage; channel a is that map turned by 0.6 a rad plus independent noise at a
tenth of the map's rms, formed on the device.  All maps are slices of one allocation of 13: the
channels in the first eight, the copy yardstick's destination in the last five.  If 13 maps of F
frames do not fit the card's free memory, the largest multiple of 64 frames that does is used and
recorded.  Timed per call with HIP events, `reps` calls after 3 warm ones, dc_half 0, all rows:
  k_cov at A = 2, 4, 8;
  k_ra at A = 2, 4, 8, n_ang = 64 and 256, Bartlett and Capon (load 1e-3), on the covariances k_cov wrote.
The yardsticks, in the same run: fmcw_copy_device over A / 2 maps' bytes plus half the cov bytes for
k_cov, and over half of (cov + ra) bytes for k_ra -- each reads and writes exactly the bytes the stage
reads and writes, so the ratio to aim for is 1.
Checked against the references of tests/ra_reference.py on the channel bytes read back, four frames
(0, 1, F/2 + 1, F - 1) of every timed case: cov within its error bound of the float64 sums, ra bit for
bit the float32 reference on the device's own cov bytes.  Needs an MI355X; there is no fallback.
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

CHANS = (2, 4, 8)
ANGLES = (64, 256)
PSI = 0.6                      # rad per channel
NOISE = 0.1                    # independent noise per channel, relative to the map's rms
SLOTS = 13                     # maps in the allocation
LOAD = 1e-3


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ra_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C32H, FMCW_C64, RaConfig
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import ra_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_ra: no GPU (there is no CPU fallback)")
    dev = "cuda"
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, M = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(), device=torch.cuda.get_device_name(0),
               frames_asked=args.frames, nr=NR, nd=ND, dc_half=0, psi_rad_per_channel=PSI, noise_rel_rms=NOISE, load=LOAD,
               reps=args.reps, storages=[])
    with torch.cuda.stream(stream):
        for name, dt, tdt in (("c64", FMCW_C64, torch.float32), ("fp16", FMCW_C32H, torch.float16)):
            esz = 4 if dt == FMCW_C64 else 2
            fbytes = NR * ND * 2 * esz
            Tmax, Kmax = 36, max(ANGLES)
            free, _ = torch.cuda.mem_get_info()
            # the allocation of 13 maps, cov and ra at their largest, the IQ of the fill and its outputs, a tenth to spare
            per_frame = SLOTS * fbytes + NR * (Tmax * 8 + Kmax * 4) + C * S * 2 * esz + 64 * (NR + C + 4 * M)
            F = min(args.frames, int(0.9 * free / per_frame) // 64 * 64)
            if F < 64:
                sys.exit("bench_ra: not enough device memory")
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
            rms = float(torch.view_as_complex(maps[0, :64].float().contiguous()).abs().pow(2).mean().sqrt())
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            for a in range(7, -1, -1):                          # channel a = the map turned by PSI a rad, plus its own noise
                rot = torch.tensor(complex(np.cos(PSI * a), np.sin(PSI * a)), dtype=torch.complex64, device=dev)
                for f0 in range(0, F, 128):
                    z = torch.view_as_complex(maps[0, f0:f0 + 128].float().contiguous()) * rot
                    v = torch.view_as_real(z) + torch.randn(z.shape + (2,), generator=gen, device=dev) * (NOISE * rms / np.sqrt(2))
                    maps[a, f0:f0 + 128] = v.to(tdt)
            maps[8:].zero_()
            torch.cuda.synchronize()
            map_bytes = F * fbytes
            sel = sorted({0, 1, min(F // 2 + 1, F - 1), F - 1})

            def host(t):
                h = t.cpu().numpy()
                return h if dt == FMCW_C32H else np.ascontiguousarray(h).view(np.complex64)[..., 0]
            chans_sel = [host(maps[a, sel]) for a in range(8)]
            flat = maps.view(-1)
            per_map = flat.numel() // SLOTS

            def copy_of(nbytes):
                """The yardstick: nbytes from the channels' slots into the slots from 8 on."""
                def copy():                                   # one launch moves at most 2^34 bytes
                    for off in range(0, nbytes, 1 << 34):
                        n = min(1 << 34, nbytes - off)
                        eng.copy_device(flat[off // esz:], flat[8 * per_map + off // esz:], n, stream=stream)
                return copy
            entry = dict(storage=name, frames=F, frames_cut_to_fit=F < args.frames, map_bytes=map_bytes, checked_frames=sel,
                         reference_frames_hold=True, cov=[], ra=[])
            for A in CHANS:
                T = A * (A + 1) // 2
                q = RaConfig(A, 64, dc_half=0)
                d_in = [maps[a] for a in range(A)]
                d_cov = torch.full((F, NR, T, 2), float("nan"), device=dev)
                cov_bytes = d_cov.numel() * 4
                half_bytes = (A * map_bytes + cov_bytes) // 2 // 16 * 16
                copy_ms = timed(copy_of(half_bytes), stream, args.reps)

                def call():
                    eng.cov_device(q, d_in, dt, F, NR, ND, d_cov, stream=stream)
                call()
                torch.cuda.synchronize()
                cov_sel = d_cov[sel].cpu().numpy()
                share = R.assert_cov_within_bound(cov_sel, chans_sel[:A], 0, name=f"{name} A{A}")
                ms = timed(call, stream, args.reps)
                moved = A * map_bytes + cov_bytes
                case = dict(case=f"cov_a{A}", n_chan=A, cov_ms=round(ms, 4), copy_ms=round(copy_ms, 4),
                            cov_over_copy=round(ms / copy_ms, 3), meets_copy_time=bool(ms <= copy_ms), bytes_moved=moved,
                            TBps=round(moved / ms / 1e9, 3), copy_TBps=round(moved / copy_ms / 1e9, 3),
                            gflop=round(F * NR * ND * A * A * 2 / 1e9, 2), error_over_bound=round(share, 4))
                entry["cov"].append(case)
                print(json.dumps(dict(storage=name, frames=F, **case)), flush=True)
                for K in ANGLES:
                    w = Engine.ra_weights(A, n_ang=K)
                    wf = R.weights_f32(w)
                    d_w = torch.from_numpy(wf).to(dev)
                    d_ra = torch.full((F, NR, K), float("nan"), device=dev)
                    d_mx = torch.zeros(1, device=dev)
                    ra_bytes = d_ra.numel() * 4
                    half_ra = (cov_bytes + ra_bytes) // 2 // 16 * 16
                    copy_ra_ms = timed(copy_of(half_ra), stream, args.reps)
                    for capon in (False, True):
                        qa = RaConfig(A, K, dc_half=0, capon=capon, load=LOAD)

                        def call_ra():
                            eng.range_angle_device(qa, d_cov, F, NR, d_w, d_ra, d_mx, stream=stream)
                        d_mx.zero_()
                        call_ra()
                        torch.cuda.synchronize()
                        want, _ = R.spectra_reference(cov_sel, wf, capon, LOAD)
                        R.assert_same_bytes(d_ra[sel].cpu().numpy(), want, f"{name} A{A} K{K} capon{capon}")
                        assert float(d_mx.cpu()[0]) == float(d_ra.max().cpu())
                        zero_rows = int((d_ra[sel].abs().amax(dim=-1) == 0).sum().cpu())
                        ms_ra = timed(call_ra, stream, args.reps)
                        moved_ra = cov_bytes + ra_bytes
                        case = dict(case=f"ra_a{A}_k{K}_{'capon' if capon else 'bartlett'}", n_chan=A, n_ang=K, capon=capon,
                                    ra_ms=round(ms_ra, 4), copy_ms=round(copy_ra_ms, 4), ra_over_copy=round(ms_ra / copy_ra_ms, 3),
                                    meets_copy_time=bool(ms_ra <= copy_ra_ms), bytes_moved=moved_ra,
                                    TBps=round(moved_ra / ms_ra / 1e9, 3), copy_TBps=round(moved_ra / copy_ra_ms / 1e9, 3),
                                    zero_rows_in_checked_frames=zero_rows)
                        entry["ra"].append(case)
                        print(json.dumps(dict(storage=name, frames=F, **case)), flush=True)
                    del d_ra, d_w
                del d_cov
                torch.cuda.empty_cache()
            res["storages"].append(entry)
            del maps, flat
            torch.cuda.empty_cache()
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
