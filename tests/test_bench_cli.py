"""bench.py's command line: a plain run prints the headline line only (everything that takes runs
of its own waits for --full), --steps sets the number of timed steps, --dump-outputs writes what
the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# what only --full measures
FULL_ONLY = ("kernel_ms", "keys_pinned", "roofline", "roofline_cold", "cpu_baseline", "greedy", "host_parse",
             "matrix_config2", "matrix_config3", "select_config3", "dropin", "controller_hot_values")


def test_dump_outputs_unpacks_keys(tmp_path):
    keys = np.array([(85 << 32) | (0xFFFFFFFF - 61805), -1, (0 << 32) | 0xFFFFFFFF,
                     (300 << 32) | (0xFFFFFFFF - 3_999_999)], np.int64)
    d = tmp_path / "out" / "deeper"
    bench.dump_outputs(str(d), keys)
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["chosen_node", "keys", "score"]
    assert all(a.dtype == np.float64 and a.shape == (4,) for a in got.values())
    assert np.array_equal(got["keys"].astype(np.int64), keys)
    assert got["chosen_node"].tolist() == [61805, -1, 0, 3_999_999]
    assert got["score"].tolist() == [85, -1, 0, 300]


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "8",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "placements/sec" and line["unit"] == "placements/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 3 and line["warmup"] == 8 and line["full"] is False
    assert line["ms_per_step"] > 0
    pods = line["config"]["pods"]
    # value is the pods of a step over the step's time (ms_per_step is rounded to 4 places)
    assert line["value"] == pytest.approx(pods / (line["ms_per_step"] * 1e-3), rel=0.05)
    assert not [k for k in FULL_ONLY if k in line]
    keys, node, score = (np.load(out / f"{n}.npy") for n in ("keys", "chosen_node", "score"))
    assert keys.dtype == np.float64 and keys.shape == node.shape == score.shape == (pods,)
    k = keys.astype(np.int64)
    assert np.array_equal(node, np.where(k < 0, -1, 0xFFFFFFFF - (k & 0xFFFFFFFF)))
    assert np.array_equal(score, np.where(k < 0, -1, k >> 32))
    assert ((node >= -1) & (node < line["config"]["nodes_total"])).all()
    assert [int(x) for x in k[:4]] == line["chosen_sample"]
