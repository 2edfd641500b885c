"""Tangent-Sampson relative pose on the CPU: the device headers (pl_refine.h camera_unproject_with_jac and Refiner<EST_RELT>,
pl_score.h tangent_pose_inlier) compiled for the host (tests/hostmath_tangent) against the reference's own
Camera::unproject_with_jac, compute_tangent_sampson_msac_score / get_tangent_sampson_inliers and refine_relpose on bearings, bit
for bit.

The comparator is tests/golden/golden_tangent_v1.json, recorded from the reference build (oracle/_ref) by
tests/golden/make_golden_tangent.py; where that build is present the fixture is also held to it, entry for entry.
"""
import json

import numpy as np
import pytest

import hostmath_tangent_lib as HT
import ref_tangent_lib as RT
from golden import make_golden_tangent as GT
from golden.make_golden import digest
from golden.make_golden_cameras import reprs

G = json.load(open(GT.PATH))
LOSS_IDS = {"TRIVIAL": 0, "TRUNCATED": 1, "HUBER": 2, "CAUCHY": 3}


def hm_unproject(cam, pix):
    """the generator's `unproject` argument, served by the host build of the device headers"""
    d, M, ok = HT.unproject_with_jac(cam, pix)
    assert ok.all()
    return d, M, None


def pose_of(rec):
    return np.array([float(v) for v in rec["pose"]])


UNPROJECT = [(m, name) for m in sorted(GT.MODEL_IDS) for name in sorted(G["unproject"][m])]


@pytest.mark.parametrize("model,name", UNPROJECT)
def test_bearing_and_jacobian_equal_the_reference_bit_for_bit(model, name):
    """d and M of Camera::unproject_with_jac for the nine models and the identity camera: about 2000 pixels over the field of view,
    the rings around the principal point, and the field as estimate_relative_pose rescales it"""
    cam, pix = GT.unproject_inputs(model)[name]
    want = G["unproject"][model][name]
    assert digest([pix]) == want["input_sha256"], "the inputs changed: regenerate the fixture"
    assert len(pix) == (41 if name == "centre" else 2000)
    d, M, ok = HT.unproject_with_jac(cam, pix)
    assert ok.all()
    assert reprs(d[:16]) == want["d_head"]
    assert reprs(M[:16]) == want["M_head"]
    assert digest([d]) == want["d_sha256"]
    assert digest([M]) == want["M_sha256"]
    if model != "NULL":
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-15
    # M = J^T (J J^T)^-1 lies in the row space of J, and J d = 0 for a projection that does not depend on the bearing's length: d^T M = 0.
    # (Not around the principal point: the fisheye models' branch there takes the Jacobian of (fx X, fy Y), for which J d != 0.)
    if model != "NULL" and name != "centre":
        assert np.abs(np.einsum("ni,nij->nj", d, M.reshape(-1, 3, 2))).max() < 1e-9 * np.abs(M).max()


@pytest.mark.parametrize("case", GT.SCORE_SCENES, ids=[c[0] for c in GT.SCORE_SCENES])
def test_score_count_and_mask_equal_the_reference_bit_for_bit(case):
    """ground truth, two perturbations of it, t = 0 (E = 0: every r^2 is NaN, no inlier) and a pose with a NaN, on problems prepared by
    the host build of the device's un-projection"""
    want = G["scores"][case[0]]
    d, x1, x2, c1, c2, P, thr = GT.score_inputs(case, hm_unproject)
    assert digest([x1, x2]) == want["pixels_sha256"], "the inputs changed: regenerate the fixture"
    assert digest([P["d1"], P["d2"], P["M1"], P["M2"]]) == want["prepared_sha256"]
    assert repr(float(thr)) == want["max_error"]
    for name, rec in want["poses"].items():
        s, cnt, mask, _ = HT.score(pose_of(rec), P["d1"], P["d2"], P["M1"], P["M2"], thr)
        assert (repr(s), cnt, GT.mask_hex(mask)) == (rec["score"], rec["count"], rec["mask_hex"]), name
    assert want["poses"]["t0"]["count"] == 0 and want["poses"]["nan"]["count"] == 0
    if case[3] >= 64:
        assert want["poses"]["gt"]["count"] >= 0.6 * case[3]


@pytest.mark.parametrize("n", GT.REFINE_N)
@pytest.mark.parametrize("run", sorted(GT.REFINE_RUNS))
def test_refiner_equals_the_reference_bit_for_bit(n, run):
    """FixCameraRelativePoseRefiner under TRUNCATED (the local optimisation's loss) and CAUCHY (the final refinement's default) loss:
    pose, costs and iteration count, the sums in correspondence order"""
    P, thr, p0 = GT.refine_inputs(n, hm_unproject)
    assert digest([P["d1"], P["d2"], P["M1"], P["M2"], p0]) == G["refine"][f"{n}/input_sha256"]
    want = G["refine"][f"{n}/{run}"]
    loss, iters = GT.REFINE_RUNS[run]
    pose, it, c0, c1 = HT.refine(p0, P["d1"], P["d2"], P["M1"], P["M2"], HT.lm_options(iters, LOSS_IDS[loss], thr))
    assert it == want["iterations"]
    assert (repr(c0), repr(c1)) == (want["initial_cost"], want["cost"])
    assert reprs(pose) == want["pose"]
    assert want["iterations"] >= 1


@pytest.mark.skipif(not RT.available(), reason="oracle/_ref not built and the reference sources absent")
def test_fixture_equals_the_live_reference():
    """every section of the fixture, regenerated through the reference build"""
    live = GT.record()
    assert live == json.loads(json.dumps(G))
