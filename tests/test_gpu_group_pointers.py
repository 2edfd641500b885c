"""The group kernels read what their argument tables point to as GLOBAL memory (-m gpu).

Every kernel of a lock-step group fetches its pointers from a device-resident table (GroupArgs, SeqScoreArgs, MaskArgs,
SelectArgs, LMTask) and passes them through pl_global.h's globalised() before the shared body runs, so that the compiler
emits global_* instead of flat_* instructions.  The conversion must keep null pointers null and must reach every optional
member, so the groups here mix members whose optional pointers are set with members whose are not, in ONE launch:

* absolute pose: N = 1100 (the smallest size on the matrix-core path: 4 chunks, the last one partly valid; shadow16, points16,
  the live list and nan_bits set), N = 300 (fp32 queue scorer: none of those), a PROSAC member (explicit `samples`), and a member
  that stops after 200 iterations and is inactive in the steps behind that;
* relative pose, fundamental matrix, homography: N = 1024 (the smallest size their matrix-core scorers accept) next to N = 300;
* pl_estimate_batch over six small problems: k_lm with mask, start_record and gate_count set, k_mask_g and k_select_record_g
  with their pinned mirrors.

Every result equals its single-problem call bit for bit (model, mask, every statistic) and the oracle in iterations,
refinements, inlier count and mask.  2000 fixed iterations per run."""
import numpy as np
import pytest

import oracle_lib as O
from poselib_amd import synth

pytestmark = pytest.mark.gpu

ITERS = 2000
STATS = ("iterations", "refinements", "num_inliers", "inlier_ratio", "model_score", "hypotheses", "nan_hypotheses")


def _flat(m):
    return np.r_[m.q, m.t] if hasattr(m, "q") else np.ravel(m)


def _resident(kind, n, seed, iters=ITERS, prosac=False):
    """(a, b, options) of one device-resident problem in normalised coordinates"""
    if kind == 0:
        d = synth.absolute_pose_scene(n, 0.5, seed)
        a, b, thr = (np.asarray(d["p2d"]) - 500.0) / 1000.0, np.asarray(d["p3d"], float), 12.0 / 1000.0
    else:
        gen = {1: synth.relative_pose_scene, 2: synth.fundamental_scene, 3: synth.homography_scene}[kind]
        d = gen(n, 0.4, seed)
        a, b, thr = (np.asarray(d["x1"]) - 500.0) / 1000.0, (np.asarray(d["x2"]) - 500.0) / 1000.0, 1.0 / 1000.0
    ro = {"seed": seed, "max_iterations": iters, "min_iterations": iters}
    if prosac:  # (PROSAC expects the correspondences best first)
        order = np.argsort(~np.asarray(d["inlier_gt"]), kind="stable")
        a, b = a[order], b[order]
        ro["progressive_sampling"] = True
    return a, b, {"max_error": thr, "ransac": ro}


GROUPS = {
    "abs": [(0, 1100, 7101, ITERS, False), (0, 300, 7102, ITERS, False), (0, 1100, 7103, ITERS, True), (0, 1100, 7104, 200, False),
            (0, 300, 7105, 200, False)],
    "rel": [(1, 1024, 7201, ITERS, False), (1, 300, 7202, ITERS, False)],
    "fund": [(2, 1024, 7301, ITERS, False), (2, 300, 7302, ITERS, False)],
    "hom": [(3, 1024, 7401, ITERS, False), (3, 300, 7402, ITERS, False)],
}
ORACLE = {0: O.ransac_pnp, 1: O.ransac_relpose, 2: O.ransac_fundamental, 3: O.ransac_homography}


@pytest.mark.parametrize("name", list(GROUPS))
def test_one_group_mixes_set_and_null_optional_pointers(gpu, name):
    members = [_resident(*m) for m in GROUPS[name]]
    probs = [gpu.Problem(m[0], a, b) for m, (a, b, _) in zip(GROUPS[name], members)]
    opts = [o for _, _, o in members]
    want = [p.run(o) for p, o in zip(probs, opts)]
    got = gpu.ransac_batch(probs, opts, 1, 16)  # one worker, one group: every member in the same launches
    for m, (a, b, opt), (model, info), (wmodel, winfo) in zip(GROUPS[name], members, got, want):
        tag = (name,) + m[1:]
        for key in STATS:
            assert info[key] == winfo[key], (tag, key, info[key], winfo[key])
        assert (np.array(info["inliers"]) == np.array(winfo["inliers"])).all(), tag
        assert (_flat(model) == _flat(wmodel)).all(), tag  # bit for bit
        _, mask, st = ORACLE[m[0]](a, b, opt)
        assert info["iterations"] == st["iterations"] == m[3], tag
        assert info["refinements"] == st["refinements"], (tag, info["refinements"], st["refinements"])
        assert info["num_inliers"] == st["num_inliers"], (tag, info["num_inliers"], st["num_inliers"])
        assert (np.array(info["inliers"]) == mask).all(), tag
    for p in probs:
        p.close()


def _front_end_problems():
    out = []
    for i, (kind, n) in enumerate([("abs", 300), ("rel", 260), ("hom", 200), ("abs", 90), ("rel", 330), ("hom", 310)]):
        opt = {"ransac": {"seed": 7500 + i, "max_iterations": ITERS, "min_iterations": ITERS}}
        if kind == "abs":
            d = synth.absolute_pose_scene(n, 0.4, 7500 + i)
            out.append(("abs", d["p2d"], d["p3d"], d["camera"], opt))
        elif kind == "rel":
            d = synth.relative_pose_scene(n, 0.4, 7500 + i)
            out.append(("rel", d["x1"], d["x2"], d["camera1"], d["camera2"], opt))
        else:
            d = synth.homography_scene(n, 0.4, 7500 + i, noise_px=0.3)
            out.append(("hom", d["x1"], d["x2"], opt))
    return out


def test_estimate_batch_reaches_the_lm_mask_and_select_tables(gpu):
    probs = _front_end_problems()
    res = gpu.estimate_batch(probs, max_in_flight=1)
    rep = gpu.last_batch_report()
    assert rep["items"] == len(probs) and rep["grouped"] == len(probs) and rep["solo"] == 0, rep
    for pr, (model, info) in zip(probs, res):
        tag = (pr[0], len(pr[1]))
        if pr[0] == "abs":
            img, winfo = gpu.estimate_absolute_pose(*pr[1:])
            got, want = np.r_[model.pose.q, model.pose.t, model.camera.params], np.r_[img.pose.q, img.pose.t, img.camera.params]
            _, mask, st = O.estimate_absolute_pose(*pr[1:])
        elif pr[0] == "rel":
            pose, winfo = gpu.estimate_relative_pose(*pr[1:])
            got, want = _flat(model), _flat(pose)
            _, mask, st = O.estimate_relative_pose(*pr[1:])
        else:
            H, winfo = gpu.estimate_homography(*pr[1:])
            got, want = _flat(model), _flat(H)
            _, mask, st = O.estimate_homography(*pr[1:])
        assert np.array_equal(got, want), tag  # bit for bit
        for key in STATS:
            assert info[key] == winfo[key], (tag, key, info[key], winfo[key])
        assert info["inliers"] == winfo["inliers"], tag
        assert info["iterations"] == st["iterations"] == ITERS, tag
        assert info["refinements"] == st["refinements"], (tag, info["refinements"], st["refinements"])
        assert info["num_inliers"] == st["num_inliers"], (tag, info["num_inliers"], st["num_inliers"])
        assert (np.array(info["inliers"]) == mask).all(), tag
