#!/usr/bin/env python3
"""Time the direction-of-arrival stage (fmcw_doa_device: k_doa) at config 4's size.

    python tools/bench_doa.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/doa_bench.json]

The channel maps are tools/bench_ra.py's: one complex64 RD map ([F][1024][256]) filled on the device
(fmcw_synth_device + fmcw_process_device), channel a that map turned by 0.6 a rad plus independent
noise at a tenth of the map's rms, A = 8 channels.  All maps are slices of one allocation of 13: the
channels in the first eight, the copy yardstick's destination in the last five.  If they do not fit
the card's free memory, the largest multiple of 64 frames that does is used and recorded.  The
covariance is fmcw_cov_device's (dc_half 0, all rows); per n_ang in 64, 256 (a grid uniform in
sin(theta)) the Bartlett and Capon spectra are fmcw_ra_device's (load 1e-3) and the MUSIC spectrum
fmcw_music_device's (8 sweeps, the count estimated: max_src 7, src_thr 8).
Timed per call with HIP events, `reps` calls after 3 warm ones: fmcw_doa_device with all five outputs,
max_pk 4, FMCW_DOA_EDGES (and FMCW_DOA_INV on Capon and MUSIC), min_rel 0.05, without the prominence
rule (min_prom 0) and with it (min_prom 2).  Beside each case, in the same run: fmcw_copy_device over
half of exactly the bytes the case reads and writes, F nr (4 K + 4 + 16 max_pk) (a copy reads and
writes every byte it is given, so the ratio to aim for is 1).
The first and the last frame of every timed case are held to tests/doa_reference.py byte for byte on
the device's own spectrum bytes.  Needs an MI355X; there is no fallback.
"""
import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ra import LOAD, NOISE, PSI, SLOTS, commit_id  # noqa: E402

A = 8
ANGLES = (64, 256)
MAX_PK = 4
MIN_REL = 0.05
PROMS = (0.0, 2.0)
SWEEPS = 8
SRC_THR = 8.0


def timed(fn, stream, reps, warm=3):
    """(mean, median, min) ms of fn() over reps calls, each between its own event pair."""
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
    ms = [a.elapsed_time(b) for a, b in pairs]
    return sum(ms) / reps, statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doa_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C64, DoaConfig, MusicConfig, RaConfig
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import doa_reference as D
    from tests import ra_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_doa: no GPU (there is no CPU fallback)")
    dev = "cuda"
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, MT = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(), device=torch.cuda.get_device_name(0),
               frames_asked=args.frames, nr=NR, nd=ND, n_chan=A, dc_half=0, psi_rad_per_channel=PSI, noise_rel_rms=NOISE,
               load=LOAD, sweeps=SWEEPS, src_thr=SRC_THR, max_pk=MAX_PK, min_rel=MIN_REL, reps=args.reps, runs=1, cases=[])
    with torch.cuda.stream(stream):
        dt, tdt, esz = FMCW_C64, torch.float32, 4
        fbytes = NR * ND * 2 * esz
        free, _ = torch.cuda.mem_get_info()
        # the 13 maps, cov, one spectrum and the outputs at their largest, the IQ of the fill and its outputs, a tenth to spare
        per_frame = SLOTS * fbytes + NR * (36 * 8 + 256 * 4 + 4 + 16 * MAX_PK) + C * S * 2 * esz + 64 * (NR + C + 4 * MT)
        F = min(args.frames, int(0.9 * free / per_frame) // 64 * 64)
        if F < 64:
            sys.exit("bench_doa: not enough device memory")
        outs = dict(profile=torch.empty((F, NR), device=dev), tgt_count=torch.empty(F, dtype=torch.int32, device=dev),
                    tgt_range_idx=torch.empty((F, MT), dtype=torch.int32, device=dev),
                    tgt_range_mag=torch.empty((F, MT), device=dev),
                    tgt_doppler_idx=torch.empty((F, MT), dtype=torch.int32, device=dev),
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
        for a in range(A - 1, -1, -1):                      # channel a = the map turned by PSI a rad, plus its own noise
            rot = torch.tensor(complex(np.cos(PSI * a), np.sin(PSI * a)), dtype=torch.complex64, device=dev)
            for f0 in range(0, F, 128):
                z = torch.view_as_complex(maps[0, f0:f0 + 128].float().contiguous()) * rot
                v = torch.view_as_real(z) + torch.randn(z.shape + (2,), generator=gen, device=dev) * (NOISE * rms / np.sqrt(2))
                maps[a, f0:f0 + 128] = v.to(tdt)
        maps[8:].zero_()
        torch.cuda.synchronize()
        sel = sorted({0, F - 1})
        flat = maps.view(-1)
        per_map = flat.numel() // SLOTS
        res.update(frames=F, frames_cut_to_fit=F < args.frames, checked_frames=sel, reference_frames_hold=True)

        def copy_of(nbytes):
            """The yardstick: nbytes from the channels' slots into the slots from 8 on."""
            def copy():                                   # one launch moves at most 2^34 bytes
                for off in range(0, nbytes, 1 << 34):
                    n = min(1 << 34, nbytes - off)
                    eng.copy_device(flat[off // esz:], flat[8 * per_map + off // esz:], n, stream=stream)
            return copy

        rows = F * NR
        d_cov = torch.full((F, NR, A * (A + 1) // 2, 2), float("nan"), device=dev)
        eng.cov_device(RaConfig(A, 64, dc_half=0), [maps[a] for a in range(A)], dt, F, NR, ND, d_cov, stream=stream)
        torch.cuda.synchronize()
        d_count = torch.full((F, NR), -7, dtype=torch.int32, device=dev)
        d_idx = torch.full((F, NR, MAX_PK), -7, dtype=torch.int32, device=dev)
        d_pow, d_sin, d_base = (torch.full((F, NR, MAX_PK), float("nan"), device=dev) for _ in range(3))
        for K in ANGLES:
            u = np.linspace(-1.0, 1.0, K).astype(np.float32)
            d_u = torch.from_numpy(u).to(dev)
            d_w = torch.from_numpy(R.weights_f32(Engine.ra_weights(A, u))).to(dev)
            d_spec = torch.full((F, NR, K), float("nan"), device=dev)
            d_mx = torch.zeros(1, device=dev)
            for method in ("bartlett", "capon", "music"):
                if method == "music":
                    eng.music_device(MusicConfig(A, K, n_src=0, max_src=A - 1, sweeps=SWEEPS, src_thr=SRC_THR), d_cov, F, NR, d_w,
                                     None, None, None, d_spec, d_mx, stream=stream)
                else:
                    eng.range_angle_device(RaConfig(A, K, dc_half=0, capon=method == "capon", load=LOAD), d_cov, F, NR, d_w,
                                           d_spec, d_mx, stream=stream)
                torch.cuda.synchronize()
                spec_sel = d_spec[sel].cpu().numpy()
                for prom in PROMS:
                    q = DoaConfig(K, max_pk=MAX_PK, edges=True, inv=method != "bartlett", min_rel=MIN_REL, min_prom=prom)
                    q.check(NR)

                    def call():
                        eng.doa_device(q, d_spec, F, NR, d_u, d_count, d_idx, d_pow, d_sin, d_base, stream=stream)
                    call()
                    torch.cuda.synchronize()
                    got = {"count": d_count[sel].cpu().numpy(), "idx": d_idx[sel].cpu().numpy(), "pow": d_pow[sel].cpu().numpy(),
                           "sin": d_sin[sel].cpu().numpy(), "base": d_base[sel].cpu().numpy()}
                    want = D.doa_reference(spec_sel, u, MAX_PK, q.flags, 0.0, MIN_REL, prom)
                    D.assert_same_bytes(got, want, f"{method} K{K} prom {prom}")
                    moved = rows * (4 * K + 4 + 16 * MAX_PK)
                    copy_ms, copy_med, copy_min = timed(copy_of(moved // 2 // 16 * 16), stream, args.reps)
                    ms, med, mn = timed(call, stream, args.reps)
                    counts = want["count"].ravel()
                    case = dict(case=f"doa_{method}_k{K}_prom{prom:g}", spectrum=method, n_ang=K, min_prom=prom, flags=q.flags,
                                doa_ms=round(ms, 4), doa_ms_median=round(med, 4), doa_ms_min=round(mn, 4),
                                copy_ms=round(copy_ms, 4), copy_ms_median=round(copy_med, 4), copy_ms_min=round(copy_min, 4),
                                doa_over_copy=round(ms / copy_ms, 3), meets_copy_time=bool(ms <= copy_ms), bytes_moved=moved,
                                TBps=round(moved / ms / 1e9, 3), copy_TBps=round(moved / copy_ms / 1e9, 3),
                                ns_per_row=round(ms * 1e6 / rows, 3), mean_count_checked_rows=round(float(counts.mean()), 3),
                                max_count_checked_rows=int(counts.max()))
                    res["cases"].append(case)
                    print(json.dumps(case), flush=True)
            del d_u, d_w, d_spec, d_mx
            torch.cuda.empty_cache()
        del maps, flat
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
