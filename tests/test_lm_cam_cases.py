"""The cases of the tests of k_lm_cam and k_sfocal_lm (tests/lm_cam_cases.py) on the CPU: the conditions under which the device
tests of tests/test_gpu_lm_cam_kernels.py mean something, checked on the reference (the oracle; for the camera models it does not
know the fixture tests/golden/golden_lm_cam_v1.json, held to the reference build where that is present) and on the serial host model
of the kernels (hostmath) alone.  No device."""
import collections

import numpy as np
import pytest

import hostmath_lib as HM
import lm_cam_cases as CC
import ref_lib
from golden import make_golden_lm_cam as GL
from lm_cam_cases import PROD, WAVE

SCOPES = [("cam", m) for m in CC.ORACLE_MODELS] + [("camfix", m) for m in CC.FIXTURE_MODELS] + [("sfocal", None)]


def test_sizes_come_from_the_kernels_constants():
    assert (CC.CAM_THREADS, CC.SF_THREADS, PROD) == (256, 256, 192)
    assert CC.CAM_NS == (8, 63, 64, 65, 129, 191, 192, 193, 384, 385, 577) and CC.FIX_NS == (65, 193, 385) and CC.N_SCENE == 577
    for model in CC.ORACLE_MODELS:
        assert {c.n for c in CC.cam_cases(model)} >= set(CC.CAM_NS)
    for model in CC.FIXTURE_MODELS:
        assert {c.n for c in CC.camfix_cases(model)} == set(CC.FIX_NS) and 30 <= len(CC.camfix_cases(model)) <= 45
    assert {c.n for c in CC.sfocal_cases()} >= set(CC.CAM_NS)
    assert len(set(CC.all_cases())) == len(CC.all_cases()) == len({CC.case_id(c) for c in CC.all_cases()})
    assert all(c.n <= CC.N_SCENE for c in CC.all_cases())
    for kind, model in SCOPES:  # (the device tests' run time: a parametrized test runs one scope)
        assert len(CC.cases(kind, model)) <= 120, (kind, model)


def test_flag_sets_reach_every_consumer():
    """the seven flag sets per model; with them jacobian_pass_m1 on column 6 (focal length) AND on column 9 (the extra parameter of
    the SIMPLE_RADIAL models alone), K = 10 with the columns 10 .. 13 (extra parameters alone, the OPENCV models), 65 entries (PINHOLE,
    focal lengths + principal point: one lane owns a high entry), and one k_lm case per pinhole model"""
    for kind, model in SCOPES[:-1]:
        cases = CC.cases(kind, model)
        assert {c.flags for c in cases} == set(CC.FLAG_SETS), (model, {c.flags for c in cases})
        plain = [c for c in cases if CC.group(c) == "m0"]
        assert len(plain) == (1 if model in ("SIMPLE_PINHOLE", "PINHOLE") else 0) and all(c.n <= CC.SEQ and c.flags == 4 for c in plain)
        for flags in CC.FLAG_SETS:
            if not CC.refined_idx(model, flags):
                continue
            mine = [c for c in cases if c.flags == flags]
            if kind == "cam":  # every flag set meets every loss: with and without a zero-weight loss
                assert {c.loss for c in mine} == set(CC.LOSSES), (model, flags)
            else:
                assert {c.loss in CC.ZERO_WEIGHT for c in mine if flags in (4, 6)} in ({True, False}, set()), (model, flags)
    for model in ("SIMPLE_RADIAL", "SIMPLE_RADIAL_FISHEYE"):  # M = 1 on column 6 + 3
        mine = [c for c in CC.camfix_cases(model) if c.flags == 4]
        assert all(CC.refined_idx(model, 4) == [3] and CC.group(c) == "m1" for c in mine)
        assert {c.loss for c in mine} == set(CC.LOSSES) and {c.update for c in mine} == {0, 1} and {c.damping for c in mine} == {0, 1}
        assert any(c.mask == "block" for c in mine) and any(CC.reference(c).invalid_steps >= 1 for c in mine)
        assert any(c.loss in CC.ZERO_WEIGHT and c.n > PROD and c.mask is None and CC.arranged(c) for c in mine)
        assert any(c.flags == 1 and CC.group(c) == "m1" for c in CC.camfix_cases(model))
    assert CC.refined_idx("OPENCV", 4) == CC.refined_idx("OPENCV_FISHEYE", 4) == [4, 5, 6, 7]
    assert len(CC.refined_idx("PINHOLE", 3)) == 4  # K = 10: 55 + 10 = 65 entries


@pytest.mark.parametrize("kind,model", SCOPES)
def test_every_option_runs(kind, model):
    cases = CC.cases(kind, model)
    assert {(c.loss, c.update, c.damping) for c in cases} == set(CC.COMBINATIONS), "a loss / update / damping combination has no case"
    assert {c.max_iterations for c in cases} >= {0, 1, 25} and {c.stop for c in cases} >= set(CC.STOP_RULES)
    assert {c.start for c in cases} == set(CC.STARTS)
    if kind != "sfocal":  # (refine_shared_focal_relpose takes no mask)
        assert {c.mask for c in cases} == {None} | set(CC.MASKS), (model, {c.mask for c in cases})
    else:
        assert {c.mask for c in cases} == {None}
    for loss in CC.LOSSES:
        assert max(CC.reference(c).iterations for c in cases if c.loss == loss) >= 2, (kind, model, loss)
    for c in cases:
        r = CC.reference(c)
        assert np.isfinite(r.model).all() and np.isfinite(r.camera).all(), CC.case_id(c)


@pytest.mark.parametrize("kind", CC.KINDS)
def test_steps_are_rejected_in_every_group(kind, capsys):
    """what follows a rejection - the kept normal equations solved again under a larger lambda, the trial camera dropped - happens in
    jacobian_pass_m1's cases, below and beyond 64 entries of the normal equations: per group two cases in which the reference
    rejects a step, one of them with a step accepted afterwards under a loss other than TRUNCATED_LE_ZACH"""
    groups = ("sfocal",) if kind == "sfocal" else ("m1", "lo", "hi")
    for g in groups:
        rejected = [c for c in CC.cases(kind) if CC.group(c) == g and CC.reference(c).invalid_steps >= 1]
        fused = [c for c in rejected if c.loss != "TRUNCATED_LE_ZACH"]
        assert len(rejected) >= 2, (kind, g, len(rejected))
        if kind == "camfix":
            after = [c for c in fused if CC.fixture()[CC.case_id(c)]["accepts_after_a_rejection"]]
        else:
            after = [c for c in fused if CC.probe_accepts_after_a_rejection(c)]
        assert after, (kind, g, "no step accepted after a rejection under a fused loss")
        with capsys.disabled():
            print(f"\nlm_cam cases {kind} {g}: {len(rejected)} with rejected steps, {len(after)} with a step accepted afterwards")


def test_every_stop_rule_decides_its_case():
    seen = collections.Counter()
    for c in CC.all_cases():
        if c.stop:
            if c.kind == "camfix":
                rec = CC.fixture()[CC.case_id(c)]
                with_rule, default = rec["iterations"], rec["iterations_without_the_rule"]
            else:
                with_rule, default = CC.oracle(c).iterations, CC.oracle(c._replace(stop=None)).iterations
            assert with_rule != default, (CC.case_id(c), with_rule)
            seen[(c.kind, c.model, c.stop)] += 1
    for kind, model in SCOPES:
        for stop in CC.STOP_RULES:
            assert seen[(kind, model, stop)] >= 1, (kind, model, stop)


def _thirds(flags):
    return [int(flags[k:k + WAVE].sum()) for k in range(0, PROD, WAVE)]


def test_masks():
    for c in CC.all_cases():
        a, b, model, _, mask = CC.inputs(c)
        if c.mask == "ones":
            assert mask.all()
        elif c.mask == "block":
            zero = np.flatnonzero(mask == 0)
            assert len(zero) == WAVE and zero[0] % WAVE == 0 and (np.diff(zero) == 1).all()
        elif c.mask == "round":
            assert c.n >= 2 * PROD + 1 and np.flatnonzero(mask == 0).tolist() == list(range(PROD, 2 * PROD))
        elif c.mask == "alternate":
            assert mask[::2].all() and not mask[1::2].any()
        elif c.mask in ("rows7", "rows8", "rows9"):  # counted per third as the consumer gets them: unmasked and in front of the camera
            kept = _thirds(CC.kept_at_start(c))
            _, depth = CC.residuals_and_depth(c, model, a, b)
            assert kept[1] == int(c.mask[4:]) and mask[:WAVE].all() and mask[2 * WAVE:].all(), (CC.case_id(c), kept)
            assert kept[0] > 9 and (np.abs(depth[WAVE:2 * WAVE][mask[WAVE:2 * WAVE] > 0]) > CC.DEPTH_MARGIN).all()
        elif c.mask == "few":
            _, depth = CC.residuals_and_depth(c, model, a, b)
            assert c.n > 256 and mask.sum() == len(CC.refined_idx(c.model, c.flags)) + 4 and (depth[mask > 0] > CC.DEPTH_MARGIN).all()


def test_rows_behind_the_camera_fall_in_every_third():
    """every unmasked absolute-pose case of a round or more has rows behind the camera at its start pose (numpy, beyond a margin of
    0.5 where the start moves the camera by some 1e-3 .. 0.4) in each third of the first round.  The exception the arrangement of
    the zero-weight losses makes: its first third is the FULL one, 64 rows that all reach the consumer - there the other two."""
    seen = 0
    for c in CC.cam_cases() + CC.camfix_cases():
        if c.mask is None and c.n >= PROD:
            a, b, model, _, _ = CC.inputs(c)
            _, depth = CC.residuals_and_depth(c, model, a, b)
            behind = _thirds(depth[:PROD] < -CC.DEPTH_MARGIN)
            if CC.arranged(c):
                assert behind[0] == 0 and behind[1] >= 1 and behind[2] >= 1, (CC.case_id(c), behind)
            else:
                assert min(behind) >= 1, (CC.case_id(c), behind)
            seen += 1
    assert seen >= 100


def test_zero_weight_cases_hold_an_empty_and_a_full_third():
    """beyond one round every unmasked case under a zero-weight loss (and the masks that keep whole thirds) has rows 0 .. 63 all
    kept at the start and rows 64 .. 127 none - numpy's residuals, the rows a factor of 2 from the threshold on either side -, from
    two rounds of rows on without exception"""
    seen, between = set(), set()
    for c in CC.all_cases():
        if c.loss in CC.ZERO_WEIGHT and c.n > PROD and c.mask in (None, "ones"):
            assert CC.arranged(c) or c.n < CC.ARRANGED_FROM, CC.case_id(c)
            if not CC.arranged(c):
                continue
            if c.n < CC.ARRANGED_FROM:
                between.add((c.kind, c.model))
            a, b, model, bo, _ = CC.inputs(c)
            r2, depth = CC.residuals_and_depth(c, model, a, b)
            assert (r2[:WAVE] < bo["loss_scale"] ** 2 / 2).all() and (depth[:WAVE] > CC.DEPTH_MARGIN).all()
            assert (r2[WAVE:2 * WAVE] > 2 * bo["loss_scale"] ** 2).all()
            kept = _thirds(CC.kept_at_start(c))
            assert kept[0] == WAVE and kept[1] == 0, (CC.case_id(c), kept)
            seen.add((c.kind, c.model))
    assert seen == set(SCOPES) and between == set(SCOPES[:-1])  # (one round + 1 row: a case of its own per camera model, lm_cam_cases._masks)


def test_device_log1p_is_glibcs_bit_for_bit():
    """pl_log1p (pl_libm.h), the Cauchy losses' cost term in every LM kernel, against the host's log1p on 2e7 arguments: a cost that
    differs in its last bit moves the Nielsen update's lambda after a mediocre step, and with it the last bits of the result - the
    device library's own log1p did that in two of this table's cases (CHANGELOG.md).  NaN results compare as equal."""
    bad, first = HM.log1p_mismatches(20_000_000, 7)
    assert bad == 0, (bad, first)


def test_host_model_refuses_flags_that_select_no_parameter():
    pix, X, cam0, truth = CC.camera_scene("PINHOLE")
    cols = [pix[:, 0], pix[:, 1], X[:, 0], X[:, 1], X[:, 2]]
    with pytest.raises(ValueError):
        HM.lm_cam(cols, truth, HM.lm_options(5, 3, 1.0), HM.camera_params(1, cam0["params"]), 4)


def test_host_model_with_pow_equals_the_reference_bit_for_bit():
    """the kernels' arithmetic, serial on the host with glibc's pow, IS the reference - on every case: pose, camera parameters or
    focal length, iteration count; masks against the reference on the compacted subset; the fixture's models against the fixture"""
    for c in CC.all_cases():
        got, want = CC.hostmath(c, False), CC.reference(c)
        assert CC.same(got, want), (CC.case_id(c), got.iterations, want.iterations)
        assert got.invalid_steps == want.invalid_steps or CC.group(c) == "m0", CC.case_id(c)
        if c.mask == "ones":
            bare = c._replace(mask=None)
            assert CC.same(got, CC.hostmath(bare, False)) and (c.kind == "camfix" or CC.same(got, CC.oracle(bare))), CC.case_id(c)


@pytest.mark.parametrize("kind", CC.KINDS)
def test_host_model_with_the_devices_cube_differs_only_after_a_differing_cube(kind):
    """HM.lm_cam / HM.sfocal_lm(device_cube=True) is what the kernels compute.  It may differ from the reference where the Nielsen
    update has cubed an argument at which lm_cube_fma and glibc's pow(x, 3) differ - nowhere else, never under FIXED_FACTOR (no
    cube), and in at most 2 % of the NIELSEN cases of a kind."""
    nielsen = differing = 0
    for c in CC.cases(kind):
        got = CC.hostmath.__wrapped__(c, True)
        args = HM.lm_cube_args()
        same = CC.same(got, CC.reference(c))
        if c.update == CC.FIXED_FACTOR:
            assert same and len(args) == 0, CC.case_id(c)
            continue
        nielsen += 1
        assert len(args) >= 1 or CC.reference(c).iterations == 0 or CC.reference(c).invalid_steps == CC.reference(c).iterations, CC.case_id(c)
        if not same:
            differing += 1
            assert (HM.lm_cube(args) != HM.glibc("pow3", args)).any(), CC.case_id(c)
    print(f"device cube, {kind}: {differing} of {nielsen} NIELSEN cases differ from the reference")
    assert differing <= 0.02 * nielsen, (differing, nielsen)


def test_fixture_inputs_are_the_tables():
    assert set(CC.fixture()) == {CC.case_id(c) for c in CC.camfix_cases()}
    for c in CC.camfix_cases():
        assert GL.input_digest(c) == CC.fixture()[CC.case_id(c)]["input_sha256"], "the inputs changed: regenerate the fixture"


@pytest.mark.skipif(not ref_lib.available(), reason="oracle/_ref not built and the reference sources absent")
def test_fixture_equals_the_live_reference():
    live = GL.record()["cases"]
    assert set(live) == set(CC.fixture())
    for key, rec in live.items():
        assert rec == CC.fixture()[key], key
