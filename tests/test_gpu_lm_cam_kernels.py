"""The two pipelined refinement kernels option by option (-m gpu): k_lm_cam of lm_cam.hip through Problem.bundle_adjust and
k_sfocal_lm of sfocal.hip through refine_shared_focal_relpose, on the cases of tests/lm_cam_cases.py - all six losses x both lambda
updates x both dampings, the seven flag sets of every camera model (one refined parameter on column 6 and on column 9, more than 64
entries of the normal equations), rough starts from which the reference rejects steps, every stop rule, max_iterations 0 and 1, masks
that leave a third with 0, 7, 8 or 9 rows or a whole round without any, rows behind the camera, and point counts on the edges of the
rounds of 192 correspondences and of their thirds.

Both kernels add every sum in the reference's order at every n, so there is no tolerance anywhere: pose, camera parameters (focal
length) and iteration count must EQUAL the serial host model of the kernels with the device's cube (hostmath lm_cam / sfocal_lm with
device_cube=True) - no exceptions -, and the reference (the oracle, or for the camera models it does not know the fixture
tests/golden/golden_lm_cam_v1.json) except where the Nielsen update cubed an argument at which the device's cube and glibc's pow
differ: the cap of tests/test_lm_cam_cases.py, 2 % of the NIELSEN cases.  tests/test_lm_cam_cases.py checks on the CPU that the cases
reject steps, that the stop rules decide, that rows lie behind the camera in every third and what the masks leave."""
import time

import numpy as np
import pytest

import lm_cam_cases as CC

pytestmark = pytest.mark.gpu

_report = {"ran": set(), "seconds": {}, "cases": {}, "off_reference": {}}  # what test_zz_report prints: profiles/lm_cam_kernel_tests.md


def _note(c):
    _report["ran"].add((c.kind, c.model or "-", c.flags, c.loss, "FIXED_FACTOR" if c.update else "NIELSEN",
                        "MARQUARDT" if c.damping else "LEVENBERG", c.stop or "-", c.mask or "-", c.n))


def _bits(r):
    return (r.iterations, r.model.tobytes(), r.camera.tobytes())


def _check_scope(gpu, kind, model):
    cases = CC.cases(kind, model)
    assert 30 <= len(cases) <= 120
    nielsen = off_reference = 0
    problems = {}
    t0 = time.perf_counter()
    try:
        for k, c in enumerate(cases):
            cid = CC.case_id(c)
            got = CC.run_on_device(gpu, c, problems)
            want = CC.hostmath(c, True)
            assert CC.same(got, want), (cid, got.iterations, want.iterations, float(np.abs(got.model - want.model).max()),
                                        float(np.abs(got.camera - want.camera).max()))
            ref = CC.reference(c)  # (a masked case: the reference on the compacted subset)
            same = CC.same(got, ref)
            assert same or c.update == CC.NIELSEN, cid
            nielsen += c.update == CC.NIELSEN
            off_reference += not same
            start = np.asarray(CC.start_camera(c)["params"] if kind != "sfocal" else [CC.start_camera(c)], dtype=np.float64)
            refined = [0] if kind == "sfocal" else CC.refined_idx(c.model, c.flags)
            if CC.group(c) == "m0":  # no parameter selected: the pose-only kernel - Problem.refine with the camera, bit for bit
                plain, plain_it = CC.refine_plain_on_device(gpu, c)
                assert plain_it == got.iterations and np.array_equal(plain, got.model), cid
            elif c.max_iterations >= 1 and not np.array_equal(ref.model, CC.inputs(c)[2]):  # (the reference accepted a step)
                assert all(got.camera[j] != start[j] for j in refined), (cid, got.camera, start)
            assert all(got.camera[j] == start[j] for j in range(len(start)) if j not in refined), (cid, got.camera, start)
            if c.mask == "ones":  # a mask of ones is no mask, bit for bit
                assert _bits(CC.run_on_device(gpu, c._replace(mask=None), problems)) == _bits(got), cid
            if k % 10 == 0:  # the double-buffered ring leaves nothing behind: the same bits again
                assert _bits(CC.run_on_device(gpu, c, problems)) == _bits(got), cid
            _note(c)
    finally:
        for pr in problems.values():
            pr.close()
    assert off_reference <= 0.02 * nielsen, (off_reference, nielsen)
    scope = (kind, model or "-")
    _report["seconds"][scope], _report["cases"][scope], _report["off_reference"][scope] = time.perf_counter() - t0, len(cases), off_reference


@pytest.mark.parametrize("model", CC.ORACLE_MODELS + CC.FIXTURE_MODELS)
def test_cam_results_equal_the_host_model(gpu, model):
    """k_lm_cam at every size: the bits and the iteration count of the serial host model with the device's cube, on every case;
    against the oracle (SIMPLE_PINHOLE, PINHOLE, OPENCV) or the fixture the cap of tests/test_lm_cam_cases.py.  The refined parameters
    move where the reference accepted a step, the others keep their bits; a mask of ones is no mask; every tenth case twice."""
    _check_scope(gpu, "cam" if model in CC.ORACLE_MODELS else "camfix", model)


def test_sfocal_results_equal_the_host_model(gpu):
    """k_sfocal_lm through refine_shared_focal_relpose: pose, focal length and iteration count, as above"""
    _check_scope(gpu, "sfocal", None)


def test_zz_report(gpu):
    """prints (pytest -s) what the tests above ran: profiles/lm_cam_kernel_tests.md holds this output of a whole run of the module"""
    print("\n| kind | camera model | cases | differ from the reference (NIELSEN, device cube) | wall time of the test, s |\n|---|---|---|---|---|")
    for scope, seconds in sorted(_report["seconds"].items()):
        print(f"| {scope[0]} | {scope[1]} | {_report['cases'][scope]} | {_report['off_reference'][scope]} | {seconds:.2f} |")
    print("\n| kind | camera model | flags | loss | update | damping | stop rule | mask | rows |\n|---|---|---|---|---|---|---|---|---|")
    for row in sorted(_report["ran"], key=str):
        print("| " + " | ".join(str(v) for v in row) + " |")
