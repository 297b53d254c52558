"""GPU: one plain ``bench.py`` run (no ``--full``) at a small frame count.

The plain run times exactly ``--steps`` steps, carries none of the ``--full`` legs
(stage breakdown, copy ceiling, extra lines, CPU baseline, oracle check), and
``--dump-outputs`` writes the last timed step's outputs as float32 ``.npy`` files
that agree with the line's own ``frames_with_target``.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    F, steps = 24, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--frames", str(F), "--dump-outputs", str(tmp_path / "out")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(F / (d["ms_per_step"] * 1e-3), rel=1e-3)
    # nothing that takes a run of its own
    assert d["cpu_baseline"] is None and d["checked"] is None and d["stages_ms_per_step"] == {}
    assert not any(k in d for k in ("fp16_storage", "config2_range_fft", "host_path", "input_fanout"))
    assert "copy_ceiling_ms" not in (d["roofline"] or {})
    # the dominant kernel's event pair rides in the timed steps: one launch per step
    assert d["roofline"]["frames_per_launch"] == F
    info = d["dumped_outputs"]
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in info["arrays"]}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) + 8 == info["bytes"] <= 64 * 10 ** 6
    assert got["profile"].shape == (F, 1024) and got["slow_mag"].shape == (F, 256)
    # the RD map (2 MiB per frame) is over its shares: 4 whole frames and 8704 Doppler rows, seeded
    assert got["rd_frames"].shape == (4, 1024, 256, 2) and got["rd_rows"].shape == (8704, 256, 2)
    assert got["stft_db"].shape[1] == 33
    has = got["tgt_count"] > 0
    assert int(has.sum()) == d["frames_with_target"] > 0
    nseg = int(np.load(tmp_path / "out" / "stft_nseg.npy")[0])
    assert nseg == int(has.sum()) * 256 - 19 == got["stft_db"].shape[0]
    assert abs(float(got["stft_db"].max())) <= 1e-3                               # dB against the global max
    assert np.all(got["slow_mag"][~has] == 0) and np.all(got["profile"].max(axis=1) > 0)
