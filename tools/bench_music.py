#!/usr/bin/env python3
"""Time the MUSIC stage (fmcw_music_device: k_music) at config 4's size.

    python tools/bench_music.py [--frames 4096] [--reps 20] [--commit ID] [--out profiles/music_bench.json]

The channel maps are tools/bench_ra.py's: one complex64 RD map ([F][1024][256]) filled on the device
(fmcw_synth_device + fmcw_process_device), channel a that map turned by 0.6 a rad plus independent
noise at a tenth of the map's rms.  All maps are slices of one allocation of 13: the channels in the
first eight, the copy yardstick's destination in the last five.  If they do not fit the card's free
memory, the largest multiple of 64 frames that does is used and recorded.  Per A in 2, 4, 8 the
covariance is fmcw_cov_device's (dc_half 0, all rows).  Timed per call with HIP events, `reps` calls
after 3 warm ones, sweeps 8, the count estimated (max_src A - 1, src_thr 8), no FB:
  eigen only          eval, evec and nsrc asked for, no spectrum;
  eigen + spectrum    all four outputs, n_ang = 64 and 256;
  spectrum alone      music asked for alone (the eigenvectors never leave LDS), n_ang = 64 and 256.
Beside them, in the same run: fmcw_copy_device over half of exactly the bytes the case reads and
writes (so the ratio to aim for is 1), and fmcw_ra_device's Capon spectrum (load 1e-3) on the same cov
and the same weight table.
Frames 0, 1, F/2 + 1 and F - 1 of every timed case are held to tests/music_reference.py byte for byte
on the device's own cov bytes.  Needs an MI355X; there is no fallback.
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_ra import LOAD, NOISE, PSI, SLOTS, commit_id, timed  # noqa: E402

CHANS = (2, 4, 8)
ANGLES = (64, 256)
SWEEPS = 8
SRC_THR = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "music_bench.json"))
    args = ap.parse_args()

    import torch
    from fmcw_radar_processing_amd import FMCW_C64, MusicConfig, RaConfig
    from fmcw_radar_processing_amd import params as P
    from fmcw_radar_processing_amd.engine import Engine
    from tests import music_reference as M
    from tests import ra_reference as R

    if not torch.cuda.is_available():
        sys.exit("bench_music: no GPU (there is no CPU fallback)")
    dev = "cuda"
    stream = torch.cuda.Stream()
    cfg = P.config(4)
    C, S, NR, ND, MT = cfg.pn, cfg.nts, cfg.nr, cfg.nd, cfg.max_targets
    eng = Engine(0)
    eng.set_taps(cfg, P.synth_calibration(S))
    res = dict(date=datetime.date.today().isoformat(), commit=args.commit or commit_id(), device=torch.cuda.get_device_name(0),
               frames_asked=args.frames, nr=NR, nd=ND, dc_half=0, psi_rad_per_channel=PSI, noise_rel_rms=NOISE, load=LOAD,
               sweeps=SWEEPS, src_thr=SRC_THR, reps=args.reps, cases=[])
    with torch.cuda.stream(stream):
        dt, tdt, esz = FMCW_C64, torch.float32, 4
        fbytes = NR * ND * 2 * esz
        free, _ = torch.cuda.mem_get_info()
        # the 13 maps, cov and every output at their largest, the IQ of the fill and its outputs, a tenth to spare
        per_frame = SLOTS * fbytes + NR * (36 * 8 + 8 * 4 + 128 * 4 + 4 + 2 * 256 * 4) + C * S * 2 * esz + 64 * (NR + C + 4 * MT)
        F = min(args.frames, int(0.9 * free / per_frame) // 64 * 64)
        if F < 64:
            sys.exit("bench_music: not enough device memory")
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
        for a in range(7, -1, -1):                          # channel a = the map turned by PSI a rad, plus its own noise
            rot = torch.tensor(complex(np.cos(PSI * a), np.sin(PSI * a)), dtype=torch.complex64, device=dev)
            for f0 in range(0, F, 128):
                z = torch.view_as_complex(maps[0, f0:f0 + 128].float().contiguous()) * rot
                v = torch.view_as_real(z) + torch.randn(z.shape + (2,), generator=gen, device=dev) * (NOISE * rms / np.sqrt(2))
                maps[a, f0:f0 + 128] = v.to(tdt)
        maps[8:].zero_()
        torch.cuda.synchronize()
        sel = sorted({0, 1, min(F // 2 + 1, F - 1), F - 1})
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
        for A in CHANS:
            T = A * (A + 1) // 2
            d_cov = torch.full((F, NR, T, 2), float("nan"), device=dev)
            eng.cov_device(RaConfig(A, 64, dc_half=0), [maps[a] for a in range(A)], dt, F, NR, ND, d_cov, stream=stream)
            torch.cuda.synchronize()
            cov_sel = d_cov[sel].cpu().numpy()
            d_eval = torch.full((F, NR, A), float("nan"), device=dev)
            d_evec = torch.full((F, NR, A, A, 2), float("nan"), device=dev)
            d_nsrc = torch.full((F, NR), -7, dtype=torch.int32, device=dev)
            cov_b, eig_b = rows * T * 8, rows * (A * 4 + A * A * 8 + 4)
            for K in (0,) + ANGLES:
                capon_ms = None
                q = MusicConfig(A, max(K, 1), n_src=0, max_src=A - 1, sweeps=SWEEPS, src_thr=SRC_THR)
                wf = d_w = d_mu = d_mx = None
                if K:
                    wf = R.weights_f32(Engine.ra_weights(A, n_ang=K))
                    d_w = torch.from_numpy(wf).to(dev)
                    d_mu = torch.full((F, NR, K), float("nan"), device=dev)
                    d_mx = torch.zeros(1, device=dev)
                want = M.music_reference(cov_sel, wf, n_src=0, max_src=A - 1, sweeps=SWEEPS, src_thr=SRC_THR)
                forms = [("eigen", True, False)] if not K else [("eigen_spectrum", True, True), ("spectrum_alone", False, True)]
                for form, eig, spec in forms:
                    def call():
                        eng.music_device(q, d_cov, F, NR, d_w, d_eval if eig else None, d_evec if eig else None,
                                         d_nsrc if eig else None, d_mu if spec else None, d_mx if spec else None, stream=stream)
                    if spec:
                        d_mx.zero_()
                        d_mu.fill_(float("nan"))
                    call()
                    torch.cuda.synchronize()
                    name = f"A{A} K{K} {form}"
                    if eig:
                        R.assert_same_bytes(d_eval[sel].cpu().numpy(), want["eval"], name + " eval")
                        R.assert_same_bytes(d_evec[sel].cpu().numpy(), want["evec"], name + " evec")
                        R.assert_same_bytes(d_nsrc[sel].cpu().numpy(), want["nsrc"], name + " nsrc")
                    if spec:
                        R.assert_same_bytes(d_mu[sel].cpu().numpy(), want["music"], name + " music")
                        assert float(d_mx.cpu()[0]) == float(d_mu.max().cpu())
                    moved = cov_b + (eig_b if eig else 0) + (rows * K * 4 if spec else 0)
                    copy_ms = timed(copy_of(moved // 2 // 16 * 16), stream, args.reps)
                    ms = timed(call, stream, args.reps)
                    case = dict(case=f"music_a{A}_k{K}_{form}", n_chan=A, n_ang=K, form=form, music_ms=round(ms, 4),
                                copy_ms=round(copy_ms, 4), music_over_copy=round(ms / copy_ms, 3),
                                meets_copy_time=bool(ms <= copy_ms), bytes_moved=moved, TBps=round(moved / ms / 1e9, 3),
                                copy_TBps=round(moved / copy_ms / 1e9, 3), ns_per_row=round(ms * 1e6 / rows, 3),
                                nsrc_histogram=np.bincount(want["nsrc"].ravel(), minlength=A).tolist())
                    if spec and form == "eigen_spectrum":
                        qa = RaConfig(A, K, dc_half=0, capon=True, load=LOAD)
                        d_ra = d_mu                                    # the same size; MUSIC's values were checked above

                        def call_ra():
                            eng.range_angle_device(qa, d_cov, F, NR, d_w, d_ra, d_mx, stream=stream)
                        capon_ms = timed(call_ra, stream, args.reps)
                    if capon_ms is not None:
                        case.update(capon_ms=round(capon_ms, 4), music_over_capon=round(ms / capon_ms, 3))
                    res["cases"].append(case)
                    print(json.dumps(case), flush=True)
                del d_w, d_mu, d_mx
            del d_cov, d_eval, d_evec, d_nsrc
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
