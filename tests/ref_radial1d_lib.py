"""Access to the reference's 1D-radial absolute-pose path through tests/ref_radial1d/ref_radial1d.cc - a small stand-alone
program of our own, run as a child process with binary files of doubles in and out.  It is compiled against the reference's
headers where they lie, together with the reference's solvers/p5lp_radial.cc (oracle/_ref/libposelib_ref.so was built without
that file and traps there; an executable's own definition is bound first, whatever the load order of a test session), and
linked to that library for everything else (tests/ref_lib.py builds it).  The program is built into a temporary directory
that lives as long as the process: nothing compiled is kept, nothing is written under oracle/.  Test infrastructure only."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

import ref_lib

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_radial1d", "ref_radial1d.cc")
_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
_exe = None
_tmp = None


def available():
    return os.path.isdir(os.path.join(ref_lib.REFERENCE_ROOT, "PoseLib")) and ref_lib.available()


def exe():
    """the driver, built once per process; its first run is the self-test (p5lp_radial on a fixed sample): a trap in the solver
    shows up here as an exit status"""
    global _exe, _tmp
    if _exe is None:
        ref_so = ref_lib.build()
        _tmp = tempfile.mkdtemp(prefix="ref_radial1d_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
        out = os.path.join(_tmp, "ref_radial1d")
        # the flags of oracle/Makefile.ref: the headers' inline arithmetic and the solver compile as in the reference build
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-w", "-I", os.path.join(_ORACLE, "eigen_shim"),
                               "-I", ref_lib.REFERENCE_ROOT, "-o", out, _SRC,
                               os.path.join(ref_lib.REFERENCE_ROOT, "PoseLib", "solvers", "p5lp_radial.cc"), ref_so,
                               "-Wl,-rpath," + os.path.dirname(ref_so)])
        r = subprocess.run([out, "selftest"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.startswith("selftest "), (r.returncode, r.stdout, r.stderr)
        _exe = out
    return _exe


def _run(cmd, values):
    prog = exe()
    fin = os.path.join(_tmp, "in.bin")
    fout = os.path.join(_tmp, "out.bin")
    np.ascontiguousarray(values, dtype=np.float64).tofile(fin)
    r = subprocess.run([prog, cmd, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (cmd, r.returncode, r.stderr)
    return np.fromfile(fout, dtype=np.float64)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def p5lp_radial(x, X):
    """x (S, 5, 2), X (S, 5, 3) -> (return values (S,), counts (S,), poses (S, 4, 7)) of p5lp_radial(x, X, &output)"""
    x, X = _f64(x, (-1, 5, 2)), _f64(X, (-1, 5, 3))
    S = x.shape[0]
    rec = np.concatenate([x.reshape(S, 10), X.reshape(S, 15)], axis=1)
    out = _run("solve", np.r_[float(S), rec.ravel()]).reshape(S, 30)
    return out[:, 0].astype(int), out[:, 1].astype(int), out[:, 2:].reshape(S, 4, 7)


def generate_models(x, X, samples):
    """x (n, 2) as the estimator holds them (NOT unit vectors), X (n, 3), samples (S, 5) -> (counts (S,), poses (S, 4, 7)) of
    Radial1DAbsolutePoseEstimator::generate_models with these samples in place of drawn ones"""
    x, X = _f64(x, (-1, 2)), _f64(X, (-1, 3))
    idx = np.asarray(samples, dtype=np.int64).reshape(-1, 5)
    out = _run("generate", np.r_[float(x.shape[0]), float(idx.shape[0]), x.ravel(), X.ravel(), idx.ravel().astype(np.float64)])
    out = out.reshape(idx.shape[0], 29)
    return out[:, 0].astype(int), out[:, 1:].reshape(-1, 4, 7)


def score(pose, x, X, max_error):
    """(score, count, mask) of compute_msac_score_1D_radial / get_inliers_1D_radial"""
    x, X = _f64(x, (-1, 2)), _f64(X, (-1, 3))
    n = x.shape[0]
    out = _run("score", np.r_[float(n), max_error * max_error, _f64(pose), x.ravel(), X.ravel()])
    return float(out[0]), int(out[1]), out[2:2 + n].astype(bool)


LOSS = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3}


def refine(pose, x, X, loss_type, loss_scale, max_iterations):
    """(pose, iterations, initial cost, cost) of bundle_adjust_1D_radial(x, X, &pose, camera {0, 0}, opt)"""
    x, X = _f64(x, (-1, 2)), _f64(X, (-1, 3))
    out = _run("refine", np.r_[float(x.shape[0]), float(LOSS[loss_type]), loss_scale, float(max_iterations), _f64(pose), x.ravel(), X.ravel()])
    return out[:7].copy(), int(out[7]), float(out[8]), float(out[9])


def _estimate(cmd, x, X, opt, initial_pose):
    x, X = _f64(x, (-1, 2)), _f64(X, (-1, 3))
    n = x.shape[0]
    r, b = opt.get("ransac", {}), opt.get("bundle", {})
    unknown = (set(opt) - {"max_error", "ransac", "bundle"}) | \
        (set(r) - {"seed", "max_iterations", "min_iterations", "success_prob", "progressive_sampling", "score_initial_model"}) | \
        (set(b) - {"loss_type", "loss_scale", "max_iterations"})
    assert not unknown, unknown
    head = [n, r.get("max_iterations", 100000), r.get("min_iterations", 1000), r.get("seed", 0), int(r.get("progressive_sampling", False)),
            int(r.get("score_initial_model", initial_pose is not None)), LOSS[b.get("loss_type", "CAUCHY")], b.get("max_iterations", 100),
            opt.get("max_error", 12.0), r.get("success_prob", 0.9999), b.get("loss_scale", 1.0)]
    pose = _f64([1, 0, 0, 0, 0, 0, 0] if initial_pose is None else initial_pose)
    out = _run(cmd, np.r_[np.array(head, dtype=np.float64), pose, x.ravel(), X.ravel()])
    stats = {"refinements": int(out[7]), "iterations": int(out[8]), "num_inliers": int(out[9]), "inlier_ratio": float(out[10]),
             "model_score": float(out[11])}
    return out[:7].copy(), out[12:12 + n].astype(bool), stats


def estimate_1D_radial_absolute_pose(x, X, opt, initial_pose=None):
    """estimate_1D_radial_absolute_pose(points2D, points3D, opt, &pose, &inliers) -> (pose (7,), mask, stats dict); every option not
    named in `opt` at the reference's default"""
    return _estimate("estimate", x, X, opt, initial_pose)


def ransac_1D_radial_pnp(x, X, opt, initial_pose=None):
    return _estimate("ransac", x, X, opt, initial_pose)
