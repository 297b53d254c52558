"""CPU: the bench harness itself (bench.py), without a GPU.

* ``bench.py --gpus 2`` outside torchrun starts two ranks through its own child
  launcher; they meet over gloo (``--dry-dist``) and rank 0 reports n_gpus 2.
  A world size that disagrees with --gpus is an error.
* The full-size check of the oracle leg (check_rd_leg / check_cube_leg) passes
  on outputs that agree with the oracle to fp32 rounding and fails on a
  perturbed RD map, range cube, detection or STFT.  The "device" outputs here
  are the Python oracle's own, rounded to float32, held in CPU tensors.
* ``--full`` is off by default; ``--dump-outputs`` (dump_outputs) writes small
  arrays whole and large ones as a fixed seeded sample of rows, within 64 MB.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from fmcw_radar_processing_amd import params as P  # noqa: E402
from oracle import oracle as O  # noqa: E402


def _run_bench(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_gpus_2_launches_two_ranks():
    r = _run_bench(["--gpus", "2", "--dry-dist"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout             # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_reduced"] == 2


def test_gpus_2_names_config5_and_the_frame_total():
    """with N > 1 ranks the line names BASELINE config 5 and the frames the
    run covered; --stream-frames 65536 makes the run the whole config-5 stream (8 steps on 2)."""
    r = _run_bench(["--gpus", "2", "--dry-dist", "--stream-frames", "65536"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    c = d["config"]
    assert c["workload"].startswith("BASELINE config 5") and "65536-frame" in c["workload"]
    assert d["steps"] == 8 and c["frames_total_per_run"] == 65536 and c["covers_config5_stream"]
    assert c["parallelism"] == "frame-shard dp2" and c["frames_per_gpu"] == 4096
    one = bench.config_block(1, 4096, 20)
    assert one["workload"].startswith("BASELINE config 4") and one["frames_total_per_run"] == 81920
    assert bench.config_block(8, 4096, 2)["covers_config5_stream"]


@pytest.mark.parametrize("args", [["--gpus", "2", "--stream-frames", "65536"],
                                  ["--gpus", "3", "--frames", "512", "--steps", "2"],
                                  ["--gpus", "8", "--stream-frames", "65536"],
                                  ["--gpus", "8", "--frames", "256", "--steps", "2", "--dry-empty", "3,4"]],
                         ids=["2_ranks_config5", "3_ranks_empty_middle", "8_ranks_config5", "8_ranks_two_empty"])
def test_dry_dist_runs_the_step_exchange(args):
    """the ranks run exactly the step's collective sequence (bench.exchange_halo
    -> the STFT leg's max(P) all_reduce -> bench.exchange_rows) on CPU tensors of the step's
    shapes, every step of the run (65,536 frames over 2 ranks: 8 steps of 4096 frames; 3 ranks
    with an empty slow-time shard in the middle at step 0), and each rank checks what it received
    (halo, lengths, max, the range_speed rows on rank 0)."""
    r = _run_bench(args + ["--dry-dist"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    ex = d["exchange"]
    assert ex["all_ranks_ok"] and ex["halo"] and ex["lengths"] and ex["max"] and ex["rows"], ex
    n = int(args[1])
    assert ex["steps"] == d["steps"] and d["n_gpus"] == n
    if "--stream-frames" in args:                    # the whole config-5 stream: 65,536 / (n x 4096) steps
        assert d["config"]["covers_config5_stream"] and d["steps"] == 65536 // (n * 4096)
        assert d["config"]["workload"].startswith("BASELINE config 5")
        assert d["config"]["parallelism"] == f"frame-shard dp{n}"
    if "--dry-empty" in args:                        # two adjacent empty shards: rank 2's halo comes from rank 5
        assert ex["empty_shards_step0"] == [3, 4]
    fo = d["input_fanout"]                           # the fan-out leg's fields
    assert fo["dry"] and fo["frames_per_rank"] == 2 and fo["ms"] > 0 and fo["GBps_root_egress"] > 0


def test_stream_frames_must_divide():
    r = _run_bench(["--gpus", "2", "--dry-dist", "--stream-frames", "65537"])
    assert r.returncode == 2 and "not a multiple" in r.stderr


def test_world_size_must_match_gpus():
    r = _run_bench(["--gpus", "2", "--dry-dist"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2
    assert "WORLD_SIZE 1" in r.stderr


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def _dump_case(F, NR, ND, C, nseg, seed=5):
    g = np.random.default_rng(seed)
    outs = {"profile": torch.from_numpy(g.random((F, NR), np.float32)),
            "slow_mag": torch.from_numpy(g.random((F, C), np.float32)),
            "tgt_count": torch.from_numpy(g.integers(0, 2, F).astype(np.int32)),
            "tgt_range_idx": torch.from_numpy(g.integers(0, NR, (F, 1)).astype(np.int32)),
            "tgt_range_mag": torch.from_numpy(g.random((F, 1), np.float32)),
            "tgt_doppler_idx": torch.from_numpy(g.integers(0, ND, (F, 1)).astype(np.int32))}
    d_rd = torch.from_numpy(g.random((F, NR, ND, 2), np.float32))
    d_db = torch.from_numpy(g.random((F * C + 19, 33), np.float32))
    return outs, d_rd, d_db, torch.tensor([nseg])


def test_dump_outputs_small_arrays_are_whole(tmp_path):
    """--dump-outputs: arrays under their share of the 64 MB are written whole, as float32, the dB map
    cut at nseg; the fp16-storage RD map is widened, not reinterpreted."""
    outs, d_rd, d_db, nseg = _dump_case(6, 32, 8, 16, 70)
    info = bench.dump_outputs(str(tmp_path / "o"), outs, d_rd.half(), d_db, nseg)
    got = {n: np.load(tmp_path / "o" / (n + ".npy")) for n in info["arrays"]}
    for k, t in outs.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], t.numpy().astype(np.float32))
    assert np.array_equal(got["rd_frames"], d_rd.half().float().numpy())
    assert np.array_equal(got["rd_rows"], d_rd.half().float().numpy().reshape(6 * 32, 8, 2))
    assert np.array_equal(got["stft_db"], d_db.numpy()[:70])
    assert np.load(tmp_path / "o" / "stft_nseg.npy")[0] == 70
    assert info["bytes"] == sum(a.nbytes for a in got.values()) + 8


def test_dump_outputs_samples_large_arrays_within_budget(tmp_path, monkeypatch):
    """Over its share an array goes out as a fixed seeded sample of its rows: the same rows on
    every run, each row intact, and the total within the sum of the shares (< 64 MB)."""
    assert sum(bench.DUMP_BUDGET.values()) + 8 <= bench.DUMP_MAX_BYTES == 64 * 10 ** 6
    monkeypatch.setattr(bench, "DUMP_BUDGET", {k: (1 << 10) for k in bench.DUMP_BUDGET})
    outs, d_rd, d_db, nseg = _dump_case(40, 32, 8, 16, 500)
    a = bench.dump_outputs(str(tmp_path / "a"), outs, d_rd, d_db, nseg)
    b = bench.dump_outputs(str(tmp_path / "b"), outs, d_rd, d_db, nseg)
    assert a["arrays"] == b["arrays"] and a["bytes"] <= 9 * (1 << 10) + 8
    for n, shape in a["arrays"].items():
        x, y = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert x.dtype == np.float32 and list(x.shape) == shape and np.array_equal(x, y)
    prof = np.load(tmp_path / "a" / "profile.npy")            # 8 of the 40 rows, in frame order, whole
    full = outs["profile"].numpy()
    rows = [int(np.nonzero((full == r).all(1))[0][0]) for r in prof]
    assert prof.shape == (8, 32) and rows == sorted(set(rows))
    db = np.load(tmp_path / "a" / "stft_db.npy")              # sampled from the first nseg segments only
    src = d_db.numpy()[:500]
    assert db.shape == (7, 33) and all((src == r).all(1).any() for r in db)


def _config_small():
    # a throughput-mode geometry small enough for the pure-Python oracle
    cfg = P.derive_params(P.deployed_device(256, 64), nr=256, nd=64, mode=P.THROUGHPUT)
    return cfg


def _rd_leg(F=6, fp16=False):
    cfg = _config_small()
    p, wr, wd, cal = bench._oracle_setup(cfg)
    iq = O.synth_frames(F, cfg.pn, cfg.nts, cfg.nr, cfg.nd, p["dist_per_bin"], frame0=40)
    if fp16:
        iq = iq.astype(np.complex64)
        h = np.stack([iq.real, iq.imag], -1).astype(np.float16)
        iq = (h[..., 0].astype(np.float32) + 1j * h[..., 1].astype(np.float32)).astype(np.complex64)
    ref = O.process_frames(iq, cal, p, wr, wd, want_rd=True, rd_all_rows=True)
    d_iq = torch.from_numpy(np.stack([iq.real, iq.imag], -1).astype(np.float16 if fp16 else np.float32))
    outs = {k: torch.from_numpy(np.asarray(ref[k]).astype(np.int32 if "idx" in k or "count" in k else np.float32))
            for k in ("profile", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "slow_mag")}
    rd = ref["rd"]
    if fp16:
        rd = rd / (cfg.nr * cfg.nd)
        d_rd = torch.from_numpy(np.stack([rd.real, rd.imag], -1).astype(np.float16))
    else:
        d_rd = torch.from_numpy(np.stack([rd.real, rd.imag], -1).astype(np.float32))
    x = O.slow_time_signal(ref)
    _, _, _, Pw = O.spectrogram(x.astype(np.float32).astype(np.float64), O.stft_window("hann"),
                                bench.STFT_NOVERLAP, bench.STFT_NFFT, 1.0 / cfg.prt)
    db = O.psd_db(Pw).T.astype(np.float32)                  # [nseg][nfft/2+1]
    leg = dict(name="t", cfg=cfg, d_iq=d_iq, outs=outs, d_rd=d_rd, d_db=torch.from_numpy(db.copy()),
               d_nseg=torch.tensor([db.shape[0]]), fp16=fp16, world=1)
    return leg


@pytest.mark.parametrize("fp16", [False, True])
def test_check_rd_leg_passes_on_agreeing_outputs(fp16):
    leg = _rd_leg(fp16=fp16)
    res, busy, nfr, _ = bench.check_rd_leg(leg, 2)
    assert res["pass"], res
    assert nfr == leg["d_iq"].shape[0] and busy > 0
    assert res["stft_segments_compared"] == res["stft_segments_ref"] > 0
    assert res["detections_differing"] == 0


def test_check_rd_leg_fails_on_errors():
    leg = _rd_leg()
    leg["d_rd"][2, 17, 5, 0] += 1e-2 * float(leg["d_rd"][2].abs().max())
    res, *_ = bench.check_rd_leg(leg, 2)
    assert not res["pass"] and res["rd_rel_l2_raw_max"] > 1e-5
    leg = _rd_leg()
    has = np.nonzero(leg["outs"]["tgt_count"].numpy() > 0)[0]
    leg["outs"]["tgt_doppler_idx"][has[0], 0] += 1
    res, *_ = bench.check_rd_leg(leg, 2)
    assert not res["pass"] and res["detections_differing"] == 1
    leg = _rd_leg()
    leg["d_db"][3, 4] += 0.01
    res, *_ = bench.check_rd_leg(leg, 2)
    assert not res["pass"] and res["stft_max_abs_db"] >= 0.009


def test_check_cube_leg():
    cfg = P.derive_params(P.deployed_device(128, 32), nr=128, nd=16, mode=P.THROUGHPUT)
    p, wr, wd, cal = bench._oracle_setup(cfg)
    iq = O.synth_frames(5, cfg.pn, cfg.nts, cfg.nr, cfg.nd, p["dist_per_bin"])
    ref = O.process_frames(iq, cal, p, wr, wd, want_cube=True)
    cube = ref["cube"]
    leg = dict(name="c2", cfg=cfg, d_iq=torch.from_numpy(np.stack([iq.real, iq.imag], -1).astype(np.float32)),
               d_cube=torch.from_numpy(np.stack([cube.real, cube.imag], -1).astype(np.float32)),
               d_prof=torch.from_numpy(ref["profile"].astype(np.float32)))
    res = bench.check_cube_leg(leg, 2)
    assert res["pass"], res
    leg["d_cube"][1, 3, 7, 1] += 1e-2 * float(leg["d_cube"][1].abs().max())
    res = bench.check_cube_leg(leg, 2)
    assert not res["pass"]
