"""bench.py --dump-outputs: what the last timed step returned is written as float32 / float64 .npy files, within 64 MB, a
fixed seeded sample of the problems where the whole would not fit (CPU: dump_outputs on synthetic results, in a child
process so that importing bench.py leaves this one's environment alone)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
from poselib_amd.api import CameraPose

n_problems, n_points, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
rng = np.random.default_rng(5)
results = []
for i in range(n_problems):
    q = rng.normal(size=4)
    info = {"iterations": 100000 + i, "refinements": i % 7, "num_inliers": i, "inlier_ratio": i / n_points,
            "model_score": 0.5 * i, "hypotheses": 3 * i, "inliers": (rng.uniform(size=n_points) < 0.3).astype(np.uint8)}
    results.append((CameraPose(q / np.linalg.norm(q), rng.normal(size=3)), info))
bench.dump_outputs(out, 0, results)
print(json.dumps({"q0": [float(v) for v in results[0][0].q], "masks": [r[1]["inliers"].tolist()[:50] for r in results]}))
"""


def _dump(tmp_path, n_problems, n_points, name):
    out = tmp_path / name
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(n_problems), str(n_points), str(out)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    import numpy as np

    files = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    return files, json.loads(r.stdout.splitlines()[-1]), sum(os.path.getsize(out / f) for f in os.listdir(out))


def test_dump_writes_every_output_of_a_small_step(tmp_path):
    import numpy as np

    files, ref, size = _dump(tmp_path, 12, 300, "small")
    assert set(files) == {"problem_index", "model", "inliers", "iterations", "refinements", "num_inliers", "inlier_ratio",
                          "model_score", "hypotheses"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert np.array_equal(files["problem_index"], np.arange(12))
    assert files["model"].shape == (12, 7) and files["inliers"].shape == (12, 300)
    assert np.array_equal(files["model"][0, :4], ref["q0"])
    assert np.array_equal(files["inliers"][:, :50], np.array(ref["masks"], dtype=np.float32))
    assert np.array_equal(files["iterations"], 100000 + np.arange(12)) and np.array_equal(files["hypotheses"], 3 * np.arange(12))


def test_dump_of_a_large_step_is_a_fixed_sample_within_64_mb(tmp_path):
    import numpy as np

    a, ref, size_a = _dump(tmp_path, 1200, 16000, "a")
    b, _, _ = _dump(tmp_path, 1200, 16000, "b")
    assert size_a <= 64 << 20
    idx = a["problem_index"].astype(int)
    assert 0 < len(idx) < 1200 and np.array_equal(idx, np.unique(idx))
    for k in a:
        assert np.array_equal(a[k], b[k]), k  # the same sample every time
    assert np.array_equal(a["inliers"][:, :50], np.array(ref["masks"], dtype=np.float32)[idx])
    assert np.array_equal(a["num_inliers"], idx)
