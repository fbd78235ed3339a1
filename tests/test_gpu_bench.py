"""GPU (-m gpu): the benchmark's command line.  A plain `bench.py --gpus 1 --steps N --warmup W` run does what its headline
figure needs -- set-up, warm-up, the timed steps, --dump-outputs, the line -- and everything measured or checked beside the
headline waits for --full.  Run here on a small stream (--events), so that the run is the interpreter's start and a few
thousand short calls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what bench.py reports beside its headline: all of it belongs to --full
MOVED = ("device_ms_per_step", "roofline", "infinity_cache_resident", "voxel_general_polarity_ms", "voxel_wide_polarity_ms",
         "voxel_live_ms", "public_api_ms", "internal_step_ms", "error_mode", "public_api_deferred_errors_ms", "c5_share",
         "prebucketed", "native_dtypes", "from_host_arrays", "voxel_structured", "image_10m", "image_c1", "cmax", "cpu_baseline",
         "oracle_self_check", "breakdown", "c5")


def test_plain_run_prints_the_headline_and_nothing_that_moved_behind_full(tmp_path):
    n, steps, warm = 300_000, 3, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warm),
                        "--events", str(n), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "Mevents/s (voxel 5-bin 640x480)" and line["unit"] == "Mevents/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == steps and line["warmup"] == warm and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    # value = events per step / the median repetition's time per step (both rounded in the line: 4 decimals of a millisecond)
    reps = line["repetitions"]
    assert reps["count"] == 7 and reps["steps_each"] == steps and len(reps["ms_per_step"]) == 7
    assert line["ms_per_step"] == reps["median"] == round(float(np.median(reps["ms_per_step"])), 4)
    lo, hi = (n / (line["ms_per_step"] + s * 1e-4) / 1e3 for s in (1, -1))
    assert lo - 0.1 <= line["value"] <= hi + 0.1, (line["value"], lo, hi)
    assert line["config"]["impl"] and line["config"]["events_per_gpu"] == n
    assert [k for k in MOVED if k in line] == []
    # --dump-outputs: the grid of the last timed step; every event puts its polarity, split over two bins, into it
    assert line["dumped_outputs"] == {"voxel": [[5, 480, 640], "float32"]}
    vox = np.load(tmp_path / "voxel.npy")
    assert vox.shape == (5, 480, 640) and vox.dtype == np.float32
    sys.path.insert(0, ROOT)
    import bench
    p = bench.synth(1000 * ((steps - 1) % bench.COLUMN_SETS) + 1, n, 0.0, 0.1)[3]
    assert abs(float(vox.astype(np.float64).sum()) - float(p.astype(np.float64).sum())) <= 1e-3 * np.sqrt(n)
