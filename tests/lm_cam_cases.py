"""Inputs of the tests of the two pipelined refinement kernels (tests/test_gpu_lm_cam_kernels.py on the device,
tests/test_lm_cam_cases.py on the CPU): k_lm_cam of lm_cam.hip (pose with camera intrinsics, Problem.bundle_adjust) and k_sfocal_lm of
sfocal.hip (pose with one shared focal length, refine_shared_focal_relpose).  A deterministic table of refinement cases in the manner
of tests/lm_cases.py, the reference's answer to each and the serial host model of the kernels (hostmath).  Everything here comes from
the oracle, a fixture, hostmath and numpy - no device.

Three kinds.  `cam`: SIMPLE_PINHOLE, PINHOLE and OPENCV, which the oracle knows - its answer is the reference.  `camfix`: the five
camera models the oracle does not know - the reference's answers are recorded in tests/golden/golden_lm_cam_v1.json by
tests/golden/make_golden_lm_cam.py; where a case has to be CHOSEN by what the reference does with it (a rejected step, a stop rule
that decides) the serial host model with pow chooses and the fixture's record is asserted.  `sfocal`: the shared-focal refiner.

Both kernels run rounds of kProd = threads - 64 correspondences: three producer wavefronts compact rows into their thirds of a
double-buffered ring, the fourth adds.  Point counts sit on those edges; a sixteenth of the absolute scene's 3-D points lies behind
the camera, which both passes skip."""
from __future__ import annotations

import collections
import functools
import json
import os
import re

import numpy as np

import hostmath_lib as HM
import lm_cases as LC
import oracle_lib as O
from golden import make_golden_cameras as GC
from golden import make_golden_fisheye as GF
from lm_cases import COMBINATIONS, FIXED_FACTOR, LEVENBERG, LOSSES, MARQUARDT, NIELSEN, STARTS, STOP_RULES, WAVE, ZERO_WEIGHT, _rng
from poselib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "golden_lm_cam_v1.json")


def _kernel_constant(source, pattern):
    return int(re.search(pattern, open(os.path.join(ROOT, "poselib_amd", "csrc", source)).read()).group(1))


CAM_THREADS = _kernel_constant("lm_cam.hip", r"constexpr int kCamThreads = (\d+);")  # 256
SF_THREADS = _kernel_constant("sfocal.hip", r"constexpr int kSfLMThreads = (\d+);")  # 256: k_sfocal_lm has the same pipeline
PROD = CAM_THREADS - WAVE                                                            # 192 correspondences per round (kProd)
# one row short of / on / beyond a third, two thirds + 1, the round boundary, a third round (rewrites buffer 0), a fourth (buffer 1)
CAM_NS = (8, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1, PROD - 1, PROD, PROD + 1, 2 * PROD, 2 * PROD + 1, 3 * PROD + 1)
FIX_NS = (WAVE + 1, PROD + 1, 2 * PROD + 1)
N_SCENE = 3 * PROD + 1
SEQ = LC.SEQ  # up to here k_lm, which serves a bundle whose flags select no parameter, adds in the reference's order

MODEL_ID = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5,
            "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9}
ORACLE_MODELS = ("SIMPLE_PINHOLE", "PINHOLE", "OPENCV")
FIXTURE_MODELS = ("SIMPLE_RADIAL", "RADIAL", "OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
TWO_FOCALS = ("PINHOLE", "OPENCV", "OPENCV_FISHEYE")
FLAG_SETS = (1, 2, 3, 4, 5, 6, 7)  # bit 0 refine_focal_length, bit 1 refine_principal_point, bit 2 refine_extra_params
KINDS = ("cam", "camfix", "sfocal")

Case = collections.namedtuple("Case", "kind model flags n loss update damping max_iterations start stop mask scale")
Case.__new__.__defaults__ = (25, "gentle", None, None, None)


def case_id(c):
    return "-".join(str(v) for v in (c.kind, c.model or "shared", f"f{c.flags}", c.n, c.loss, "FIXED" if c.update else "NIELSEN",
                                     "MARQUARDT" if c.damping else "LEVENBERG", f"it{c.max_iterations}", c.start, c.stop or "default",
                                     c.mask or "nomask") + (() if c.scale is None else (f"s{c.scale:g}",)))


def refined_idx(model, flags):
    """Camera::get_param_refinement_idx: focal, principal point, extra parameters, in that order"""
    two = model in TWO_FOCALS
    extra = {"SIMPLE_PINHOLE": [], "PINHOLE": [], "SIMPLE_RADIAL": [3], "RADIAL": [3, 4], "SIMPLE_RADIAL_FISHEYE": [3],
             "RADIAL_FISHEYE": [3, 4], "OPENCV": [4, 5, 6, 7], "OPENCV_FISHEYE": [4, 5, 6, 7]}[model]
    return ([0, 1] if two else [0]) * bool(flags & 1) + ([2, 3] if two else [1, 2]) * bool(flags & 2) + extra * bool(flags & 4)


def group(c):
    """what the consumer of k_lm_cam does: "m0" no refined parameter (k_lm), "m1" jacobian_pass_m1, "lo" up to 64 entries of the
    normal equations (K < 10), "hi" more (each consumer lane owns a second entry)"""
    if c.kind == "sfocal":
        return "sfocal"
    m = len(refined_idx(c.model, c.flags))
    return "m0" if m == 0 else "m1" if m == 1 else "lo" if 6 + m < 10 else "hi"


def flag_options(flags):
    return {k: True for b, k in ((1, "refine_focal_length"), (2, "refine_principal_point"), (4, "refine_extra_params")) if flags & b}


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
OUTLIERS = 0.3
BEHIND_EVERY, BEHIND_AT = 16, 5  # rows 5, 21, 37, ... of the absolute scene: four in every third of a round
DEPTH_MARGIN = 0.5               # "behind the camera by a clear margin": the scene's depths are 0.1 .. 10, its starts move t by <= 0.4 sigma


@functools.lru_cache(maxsize=None)
def _abs_scene():
    """synth.absolute_pose_scene with every sixteenth 3-D point mirrored through the true camera centre: it projects to the same
    pixel, at the negated depth"""
    d = synth.absolute_pose_scene(N_SCENE, OUTLIERS, 9300)
    X = np.asarray(d["p3d"]).copy()
    centre = -synth.quat_to_rotmat(np.asarray(d["q_gt"])).T @ np.asarray(d["t_gt"])
    behind = np.arange(N_SCENE) % BEHIND_EVERY == BEHIND_AT
    X[behind] = 2.0 * centre - X[behind]
    return d, np.ascontiguousarray(X), behind


@functools.lru_cache(maxsize=None)
def camera_scene(model):
    """(pixels, 3-D points, camera off its calibration, true pose): the scene as `model` sees it, cameras() and off_calibration of
    tests/test_gpu_intrinsics.py for the oracle's models, the fixtures' cameras for the others.  Cameras carry the model's NAME."""
    d, X, _ = _abs_scene()
    f, cx, cy = d["camera"]["params"]
    pin = np.asarray(d["p2d"])
    rs = np.random.RandomState(9310 + MODEL_ID[model])
    if model in ORACLE_MODELS:
        par = {"SIMPLE_PINHOLE": [f, cx, cy], "PINHOLE": [f, f, cx, cy], "OPENCV": [f, f, cx, cy, -0.05, 0.01, 1e-3, -5e-4]}[model]
        cam = dict(d["camera"], model=model, params=par)
        pix = synth.opencv_distort_pixels(pin, par) if model == "OPENCV" else pin
        nf = 1 if model == "SIMPLE_PINHOLE" else 2
        par0 = np.array(par, dtype=np.float64)
        par0[:nf] *= 1.0 + 0.02 * rs.randn(nf)
        par0[nf:nf + 2] += 3.0 * rs.randn(2)
        cam0 = dict(cam, params=[float(v) for v in par0])
    elif model in GC.MODELS:
        cam = GC.camera(model)
        pix = synth.radial_distort_pixels(pin, cam["params"])
        cam0 = GC.named(GC.off_calibration(cam, rs, 0.02, 3.0))
    else:
        cam = GF.camera(model)
        pix = GF.through(cam, pin)
        cam0 = GF.named(GF.off_calibration(cam, rs, 0.02, 3.0))
    return np.ascontiguousarray(pix), X, cam0, np.r_[d["q_gt"], d["t_gt"]]


SF_SCALE = 700.0


@functools.lru_cache(maxsize=None)
def sfocal_scene():
    """(a, b, true pose, true focal length): synth.relative_pose_scene, focal length 900, centred and divided by 700 as
    test_refine_shared_focal_relpose_bit_exact does"""
    d = synth.relative_pose_scene(N_SCENE, OUTLIERS, 9301, focal=900.0)
    f, cx, cy = d["camera1"]["params"]
    a, b = (np.asarray(d["x1"]) - [cx, cy]) / SF_SCALE, (np.asarray(d["x2"]) - [cx, cy]) / SF_SCALE
    return np.ascontiguousarray(a), np.ascontiguousarray(b), np.r_[d["q_gt"], d["t_gt"]], f / SF_SCALE


FOCAL_OFF = 1.1  # the shared-focal cases start 10 % off the focal length


def project(model, par, Zc):
    """numpy's projection of camera-frame points (the sign of the depth ignored, as the formulas do)"""
    nf = 2 if model in TWO_FOCALS else 1
    fx, fy, cx, cy = par[0], par[nf - 1], par[nf], par[nf + 1]
    pin = np.stack([fx * Zc[:, 0] / Zc[:, 2] + cx, fy * Zc[:, 1] / Zc[:, 2] + cy], axis=1)
    if model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return pin
    if model == "OPENCV":
        return synth.opencv_distort_pixels(pin, par)
    if model in GC.MODELS:
        return synth.radial_distort_pixels(pin, par)
    return synth.fisheye_distort_pixels(pin, model, par)


def residuals_and_depth(c, model, a, b):
    """numpy's squared residuals of the refiners' cost at `model` (pixels / Sampson) and the depths (absolute pose; ones otherwise):
    what arranges rows and builds masks, with a margin of 2 either side of a threshold"""
    if c.kind == "sfocal":
        f = sfocal_scene()[3] * FOCAL_OFF
        Kinv = np.diag([1.0 / f, 1.0 / f, 1.0])
        M = Kinv @ LC._skew(model[4:]) @ synth.quat_to_rotmat(model[:4]) @ Kinv
        x1, x2 = np.c_[a, np.ones(len(a))], np.c_[b, np.ones(len(b))]
        Fx1, Ftx2 = x1 @ M.T, x2 @ M
        e = (x2 * Fx1).sum(axis=1)
        return e * e / (Fx1[:, 0] ** 2 + Fx1[:, 1] ** 2 + Ftx2[:, 0] ** 2 + Ftx2[:, 1] ** 2), np.ones(len(a))
    Zc = b @ synth.quat_to_rotmat(model[:4]).T + model[4:]
    return ((project(c.model, camera_scene(c.model)[2]["params"], Zc) - a) ** 2).sum(axis=1), Zc[:, 2]


# ---- starts and options --------------------------------------------------------------------------------------------------------------
START = {"gentle": 1e-3, "rough": 0.05, "far": 0.4}  # lm_cases.START of poses
# loss scales as lm_cases.SCALE chooses them: the absolute pose's in pixels (a focal length of 1000), the shared focal length's in
# the units of its coordinates with the 10 % error of the focal length on top of the start's
SCALE = {"gentle": {"cam": 12.0, "sfocal": 0.06}, "rough": {"cam": 250.0, "sfocal": 0.1}, "far": {"cam": 500.0, "sfocal": 0.15}}


# From two rounds of rows on, start_model looks for a start at which _arranged_rows finds its two blocks.  (Between one and two
# rounds a third of the rows would have to lie a factor of 2 below the threshold and a third a factor of 2 above: only starts next
# to the truth spread the residuals that far, so there the blocks are taken where a start happens to offer them.)
ARRANGED_FROM = 2 * PROD


def stop_options(c):
    """lm_cases.STOP_RULES; the gradient of the absolute pose's cost in pixels is 1e6 times that in normalised coordinates"""
    return {"gradient_tol": 1e3} if c.stop == "gradient_tol" and c.kind != "sfocal" else STOP_RULES[c.stop]


def loss_scale(c):
    return SCALE[c.start]["sfocal" if c.kind == "sfocal" else "cam"] if c.scale is None else c.scale


def scene_rows(c):
    if c.kind == "sfocal":
        a, b, truth, _ = sfocal_scene()
    else:
        a, b, _, truth = camera_scene(c.model)
    return a, b, truth


def start_model(c):
    """lm_cases.start_model: the truth moved by the start's distance; for the truncated losses the first of ten fixed draws from which
    the loss keeps a quarter of the rows and drops a tenth (and fills _arranged_rows' two blocks), at 0.85 of the distance if none
    does, and so on"""
    a, b, truth = scene_rows(c)
    d = START[c.start]
    thr2 = loss_scale(c) ** 2
    for attempt in range(200):
        rs = _rng(c._replace(mask=None, stop=None), attempt)
        q = truth[:4] + d * rs.randn(4)
        model = np.r_[q / np.linalg.norm(q), truth[4:] + d * rs.randn(3)]
        if not c.loss.startswith("TRUNCATED") or (c.scale is not None and c.loss not in ZERO_WEIGHT):
            break
        r2, depth = residuals_and_depth(c, model, a[: c.n], b[: c.n])
        keeps, drops = (r2 < thr2 / 2) & (depth > DEPTH_MARGIN), (r2 > 2 * thr2) & (depth > 0)
        blocks = c.loss not in ZERO_WEIGHT or (c.n < ARRANGED_FROM and c.scale is None) or c.n <= PROD or (keeps.sum() >= WAVE and drops.sum() >= WAVE)  # (_arranged_rows)
        if keeps.mean() >= 0.25 and (r2 > 2 * thr2).mean() >= 0.1 and blocks:
            break
        if attempt % 10 == 9:
            d *= 0.85
    return model


def bundle_options(c):
    bo = {"loss_type": c.loss, "loss_scale": loss_scale(c), "max_iterations": c.max_iterations, "lambda_update": c.update,
          "damping": c.damping}
    if c.stop:
        bo.update(stop_options(c))
    bo.update(flag_options(c.flags))
    return bo


# ---- rows and masks ------------------------------------------------------------------------------------------------------------------
def _arranged_rows(c, a, b, model):
    """Zero-weight losses beyond one round: rows 0 .. 63 all kept at the start (in front of the camera, a factor of 2 below the
    threshold: a producer wavefront whose third fills), rows 64 .. 127 none kept (a factor of 2 above it - rows behind the camera
    first: a third without rows), the rest in the scene's order."""
    n = c.n
    if c.loss not in ZERO_WEIGHT or n <= PROD:
        return np.arange(n)
    thr2 = loss_scale(c) ** 2
    r2, depth = residuals_and_depth(c, model, a[:n], b[:n])
    kept = np.flatnonzero((r2 < thr2 / 2) & (depth > DEPTH_MARGIN))[:WAVE]
    above = r2 > 2 * thr2
    dropped = np.r_[np.flatnonzero(above & (depth < -DEPTH_MARGIN))[:4], np.flatnonzero(above & (depth > 0))][:WAVE]
    if len(kept) < WAVE or len(dropped) < WAVE:  # (no start of the list fills both blocks: tests/test_lm_cam_cases.py counts them)
        return np.arange(n)
    return np.r_[kept, np.sort(dropped), np.setdiff1d(np.arange(n), np.r_[kept, dropped])]


def arranged(c):
    """did _arranged_rows find a full and an empty third for the case?"""
    a, b, _ = scene_rows(c)
    return not np.array_equal(_arranged_rows(c, a, b, start_model(c)), np.arange(c.n))


def _mask(c, a, b, model):
    n = c.n
    if c.mask is None:
        return None
    m = np.ones(n, dtype=np.uint8)
    if c.mask == "ones":
        return m
    if c.mask == "block":  # one whole 64-aligned block zeroed: a producer wavefront leaves nothing in its third
        first = WAVE * ((n // WAVE) // 2)
        m[first:first + WAVE] = 0
        return m
    if c.mask == "round":  # the whole second round: the consumer gets a round without rows
        assert n >= 2 * PROD + 1
        m[PROD:2 * PROD] = 0
        return m
    if c.mask == "alternate":
        return (np.arange(n) % 2 == 0).astype(np.uint8)
    r2, depth = residuals_and_depth(c, model, a, b)
    if c.mask in ("rows7", "rows8", "rows9"):  # exactly 7 / 8 / 9 rows of the second third reach the consumer: its eight-row step
        assert n >= 2 * WAVE and c.loss not in ZERO_WEIGHT
        front = WAVE + np.flatnonzero(depth[WAVE:2 * WAVE] > DEPTH_MARGIN)
        m[WAVE:2 * WAVE] = 0
        m[front[: int(c.mask[4:])]] = 1
        return m
    assert c.mask == "few" and n > SEQ  # M + 4 rows of more than 256: inliers of the truth, in front of the camera, spread out
    _, _, truth = scene_rows(c)
    t2, tdepth = residuals_and_depth(c._replace(start="gentle"), truth, a, b)
    good = np.flatnonzero((t2 < (40.0 if c.kind != "sfocal" else 0.04) ** 2) & (tdepth > DEPTH_MARGIN))
    m[:] = 0
    m[good[np.linspace(0, len(good) - 1, len(refined_idx(c.model, c.flags)) + 4).astype(int)]] = 1
    return m


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(a, b, start pose, bundle options, mask or None) of a case; a: pixels / first image, b: 3-D points / second image"""
    a, b, _ = scene_rows(c)
    model = start_model(c)
    rows = _arranged_rows(c, a, b, model)
    a, b = np.ascontiguousarray(a[rows]), np.ascontiguousarray(b[rows])
    return a, b, model, bundle_options(c), _mask(c, a, b, model)


def start_camera(c):
    """the camera a case starts from: the model's camera off its calibration (named), or the focal length 10 % off"""
    return sfocal_scene()[3] * FOCAL_OFF if c.kind == "sfocal" else camera_scene(c.model)[2]


def kept_at_start(c):
    """numpy: which rows reach the consumer in the first Jacobian pass - unmasked, in front of the camera, weight not zero"""
    a, b, model, bo, mask = inputs(c)
    r2, depth = residuals_and_depth(c, model, a, b)
    keep = depth > 0
    if c.loss in ZERO_WEIGHT:
        keep &= r2 < bo["loss_scale"] ** 2
    if mask is not None:
        keep &= mask.astype(bool)
    return keep


# ---- the reference and the host model ------------------------------------------------------------------------------------------------
Result = collections.namedtuple("Result", "model camera iterations invalid_steps")


def _int_camera(cam):
    return dict(cam, model=MODEL_ID[cam["model"]])


def reference_run(c, a, b, model, bo, R=O):
    """the reference on the given rows: the oracle (R = oracle_lib) or, inside ref_lib.reference(), the reference build"""
    if c.kind == "sfocal":
        p, f, st = R.refine_shared_focal_relpose(a, b, model, start_camera(c), bo)
        return Result(p, np.array([f]), int(st.iterations), int(st.invalid_steps))
    p, cam, st = R.bundle_adjust_camera(a, b, _int_camera(start_camera(c)), model, bo)
    return Result(p, cam, int(st.iterations), int(st.invalid_steps))


def compacted(c):
    a, b, model, bo, mask = inputs(c)
    if mask is not None:
        a, b = a[mask.astype(bool)], b[mask.astype(bool)]
    return a, b, model, bo


@functools.lru_cache(maxsize=None)
def oracle(c):
    """the oracle's answer (cam, sfocal): for a mask, its refinement of the compacted subset"""
    assert c.kind != "camfix", "the oracle does not know these camera models"
    return reference_run(c, *compacted(c))


def accepts_after_a_rejection(c, run):
    """run(max_iterations) -> Result, iteration by iteration: was a step accepted after one had been rejected?"""
    prev = None
    for k in range(run(c.max_iterations).iterations + 1):
        r = run(k)
        if prev is not None and prev.invalid_steps >= 1 and r.invalid_steps == prev.invalid_steps and \
                not (np.array_equal(r.model, prev.model) and np.array_equal(r.camera, prev.camera)):
            return True
        prev = r
    return False


@functools.lru_cache(maxsize=None)
def hostmath(c, device_cube, max_iterations=None):
    """the kernels' algorithm serially on the host (every sum in the reference's order).  Flags that select no parameter: the
    pose-only model with the camera, HM.lm - k_lm serves such a bundle."""
    a, b, model, bo, mask = inputs(c)
    opt = HM.lm_options(bo["max_iterations"] if max_iterations is None else max_iterations, O.LOSS[bo["loss_type"]], bo["loss_scale"],
                        lambda_update=bo["lambda_update"], damping=bo["damping"],
                        **{k: v for k, v in bo.items() if k.endswith("_tol") or k.endswith("_lambda")})
    if c.kind == "sfocal":
        p, f, it, _, skipped = HM.sfocal_lm(a, b, model, start_camera(c), opt, mask=mask, device_cube=device_cube)
        assert not skipped
        return Result(p[:7].copy(), np.array([f]), it, HM.invalid_steps())
    cam0 = start_camera(c)
    cam = HM.camera_params(MODEL_ID[cam0["model"]], cam0["params"])
    cols = [a[:, 0], a[:, 1], b[:, 0], b[:, 1], b[:, 2]]
    if group(c) == "m0":
        p, it, _ = HM.lm("abs", cols, model, opt, cam, mask=mask, device_cube=device_cube)
        return Result(p[:7].copy(), np.array(cam0["params"]), it, -1)
    p, par, it, _ = HM.lm_cam(cols, model, opt, cam, c.flags, mask=mask, device_cube=device_cube)
    return Result(p[:7].copy(), par, it, HM.invalid_steps())


@functools.lru_cache(maxsize=None)
def fixture():
    return json.load(open(FIXTURE))["cases"]


def floats(v):
    return np.array([float(x) for x in v])


def reference(c):
    """the reference's answer: the oracle, or for the models it does not know the fixture's record"""
    if c.kind != "camfix":
        return oracle(c)
    r = fixture()[case_id(c)]
    return Result(floats(r["pose"]), floats(r["camera"]), r["iterations"], r["invalid_steps"])


def _probe(c):
    """what CHOOSES a case by the course of its refinement: the oracle, or for the fixture's models the host model with pow"""
    return hostmath(c, False) if c.kind == "camfix" else oracle(c)


def probe_accepts_after_a_rejection(c):
    if c.kind == "camfix":
        return accepts_after_a_rejection(c, lambda k: hostmath(c, False, k))
    a, b, model, bo = compacted(c)
    return accepts_after_a_rejection(c, lambda k: reference_run(c, a, b, model, dict(bo, max_iterations=k)))


def same(got, want):
    return got.iterations == want.iterations and np.array_equal(got.model, want.model) and np.array_equal(got.camera, want.camera)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
UPDATE_DAMPING = [(NIELSEN, LEVENBERG), (NIELSEN, MARQUARDT), (FIXED_FACTOR, LEVENBERG), (FIXED_FACTOR, MARQUARDT)]


def _cam_grid(model):
    """every loss with every flag set; the four update / damping pairs in turn so that every loss meets each of them; sizes and
    starts in turn.  A flag set that selects no parameter (extra parameters of a pinhole model) is k_lm's: one such case per model,
    at a size up to which k_lm adds in the reference's order."""
    out, j, plain = [], 0, False
    for li, loss in enumerate(LOSSES):
        for fi, flags in enumerate(FLAG_SETS):
            update, damping = UPDATE_DAMPING[(fi + li) % 4]
            c = Case("cam", model, flags, CAM_NS[j % len(CAM_NS)], loss, update, damping, 25, STARTS[j % 3])
            j += 1
            if not refined_idx(model, flags):
                live = [f for f in FLAG_SETS if refined_idx(model, f)]
                out.append(c._replace(flags=live[li % len(live)]))  # (the combination keeps a case)
                if plain:
                    continue
                plain, c = True, c._replace(n=PROD + 1, loss="CAUCHY", start="gentle")
            out.append(c)
    return out


def _sfocal_grid():
    return [Case("sfocal", None, 0, CAM_NS[i % len(CAM_NS)], loss, update, damping, 25, STARTS[i % 3])
            for i, (loss, update, damping) in enumerate(COMBINATIONS)]


FIX_ROTATION = (1, 2, 3, 5, 1, 7)


def _fix_grid(model):
    """the 24 combinations on the fixture's models: of the four cases of a loss the first and the last refine the extra parameters
    alone (flags 4: with one extra parameter jacobian_pass_m1's column 9), the second principal point + extra (6), the third the
    other sets in turn; flags 7 takes every second last place"""
    out = []
    for i, (loss, update, damping) in enumerate(COMBINATIONS):
        li, j = divmod(i, 4)
        flags = (4, 6, FIX_ROTATION[li], 4 if li % 2 == 0 or model.startswith("SIMPLE_") else 7)[j]
        out.append(Case("camfix", model, flags, FIX_NS[(i + li) % 3], loss, update, damping, 25, STARTS[(i + li) % 3]))
    return out


REJECTION_CASES = 5
# (model, flags) in turn for the rejection cases of a group
REJECTION_TARGETS = {"m1": [("SIMPLE_PINHOLE", 1)],
                     "lo": [("SIMPLE_PINHOLE", 3), ("PINHOLE", 2), ("OPENCV", 1), ("SIMPLE_PINHOLE", 2), ("PINHOLE", 1), ("OPENCV", 2)],
                     "hi": [("OPENCV", 7), ("PINHOLE", 3), ("OPENCV", 4), ("OPENCV", 6), ("OPENCV", 5), ("OPENCV", 3)]}


def _rejection_cases(kind, targets, sizes, count=REJECTION_CASES):
    """lm_cases._rejection_cases: the first `count` of a fixed list of far starts under the fused losses in which the reference
    rejects a step - one of them, if the list holds one, with a step accepted after the rejection (count = 1: the first case at all,
    the fixture's models take one per flag set)"""
    out, accepted_after = [], count == 1
    for i, (loss, update, damping) in enumerate(COMBINATIONS * 8):
        if loss == "TRUNCATED_LE_ZACH":
            continue
        model, flags = targets[i % len(targets)]
        c = Case(kind, model, flags, sizes[(i // len(COMBINATIONS) + i) % len(sizes)], loss, update, damping, 25 - i // len(COMBINATIONS), "far")
        r = _probe(c)
        if r.invalid_steps < 1 or not (np.isfinite(r.model).all() and np.isfinite(r.camera).all()):
            continue
        after = probe_accepts_after_a_rejection(c)
        if len(out) < count - 1 or accepted_after or after:
            out.append(c)
            accepted_after = accepted_after or after
        if len(out) == count:
            break
    return out


def _stop_case(kind, model, flags, sizes, stop):
    """lm_cases._stop_case: the first of a fixed list of candidates whose course in the reference the rule changes"""
    gentle_scale = SCALE["gentle"]["sfocal" if kind == "sfocal" else "cam"]
    if stop.endswith("lambda"):
        candidates = [Case(kind, model, flags, n, "TRUNCATED_LE_ZACH", FIXED_FACTOR if stop == "min_lambda" else update, damping, 25, start,
                           stop, None, gentle_scale)
                      for n in sizes for start in ("rough", "far") for damping in (LEVENBERG, MARQUARDT) for update in (NIELSEN, FIXED_FACTOR)]
        candidates += [Case(kind, model, flags, n, loss, FIXED_FACTOR if stop == "min_lambda" else update, damping, 25, start, stop)
                       for n in sizes for start in ("far", "rough") for damping in (LEVENBERG, MARQUARDT) for update in (NIELSEN, FIXED_FACTOR)
                       for loss in ("CAUCHY", "TRUNCATED", "HUBER", "TRIVIAL", "TRUNCATED_CAUCHY", "TRUNCATED_LE_ZACH")]
    else:
        candidates = [Case(kind, model, flags, n, loss, NIELSEN, LEVENBERG, 25, start, stop) for n in sizes for start in STARTS
                      for loss in ("CAUCHY", "TRUNCATED", "HUBER", "TRIVIAL", "TRUNCATED_CAUCHY", "TRUNCATED_LE_ZACH")]
    for c in candidates:
        if _probe(c).iterations != _probe(c._replace(stop=None)).iterations and _probe(c).iterations >= 1:
            return c
    return candidates[0]


def _stops_and_iterations(kind, model, flag_sets, n_small, n_large):
    out = [_stop_case(kind, model, flag_sets[i % len(flag_sets)], ((n_small, n_large), (n_large, n_small))[i % 2], stop)
           for i, stop in enumerate(STOP_RULES)]
    for i, (mi, loss) in enumerate(((0, "CAUCHY"), (1, "TRUNCATED"), (0, "TRUNCATED"), (1, "TRUNCATED_LE_ZACH"))):
        out.append(Case(kind, model, flag_sets[i % len(flag_sets)], (n_small, n_large)[i % 2], loss, NIELSEN, LEVENBERG, mi, "rough"))
    return out


def _masks(kind, model, flag_sets):
    f = lambda i: flag_sets[i % len(flag_sets)]  # noqa: E731
    return [Case(kind, model, f(0), PROD + 1, "CAUCHY", NIELSEN, LEVENBERG, 25, "gentle", None, "ones"),
            Case(kind, model, f(1), 2 * PROD + 1, "TRUNCATED", NIELSEN, LEVENBERG, 25, "gentle", None, "ones"),
            Case(kind, model, f(2), PROD + 1, "TRUNCATED", FIXED_FACTOR, LEVENBERG, 25, "rough", None, "block"),
            Case(kind, model, f(3), 2 * PROD + 1, "TRUNCATED", NIELSEN, LEVENBERG, 25, "far", None, "block"),
            Case(kind, model, f(4), 2 * PROD + 1, "TRUNCATED_CAUCHY", NIELSEN, MARQUARDT, 25, "gentle", None, "alternate"),
            Case(kind, model, f(5), PROD + 1, "HUBER", NIELSEN, LEVENBERG, 25, "far", None, "alternate"),
            Case(kind, model, f(6), 2 * PROD + 1, "HUBER", NIELSEN, LEVENBERG, 25, "rough", None, "round"),
            Case(kind, model, f(0), 3 * PROD + 1, "TRUNCATED", FIXED_FACTOR, MARQUARDT, 25, "gentle", None, "round"),
            Case(kind, model, f(1), PROD + 1, "CAUCHY", NIELSEN, LEVENBERG, 25, "gentle", None, "rows7"),
            Case(kind, model, f(2), 2 * PROD + 1, "HUBER", FIXED_FACTOR, LEVENBERG, 25, "gentle", None, "rows8"),
            Case(kind, model, f(3), PROD + 1, "TRIVIAL", NIELSEN, MARQUARDT, 25, "gentle", None, "rows9"),
            Case(kind, model, f(4), 2 * PROD + 1, "CAUCHY", NIELSEN, LEVENBERG, 25, "gentle", None, "few"),
            Case(kind, model, f(5), 3 * PROD + 1, "TRUNCATED", NIELSEN, LEVENBERG, 25, "gentle", None, "few"),
            # one round + 1 row with a full and an empty third: next to the truth a threshold of 25 pixels has a third of the rows a
            # factor of 2 below it and a third a factor of 2 above (ARRANGED_FROM)
            Case(kind, model, f(6), PROD + 1, "TRUNCATED", NIELSEN, LEVENBERG, 25, "gentle", None, None, 25.0)]


MASKS = ("ones", "block", "round", "alternate", "rows7", "rows8", "rows9", "few")
BEYOND_A_ROUND = CAM_NS[CAM_NS.index(PROD + 1):]


@functools.lru_cache(maxsize=None)
def cam_cases(model=None):
    if model is not None:
        return [c for c in cam_cases() if c.model == model]
    out = []
    for m in ORACLE_MODELS:
        live = [f for f in FLAG_SETS if refined_idx(m, f)]
        out += _cam_grid(m)
        out += _stops_and_iterations("cam", m, live[::-1], WAVE + 1, 2 * PROD + 1)
        out += _masks("cam", m, live)
    for g, sizes in (("m1", CAM_NS[1:]), ("lo", CAM_NS[1:]), ("hi", CAM_NS[1:])):
        out += _rejection_cases("cam", REJECTION_TARGETS[g], sizes)
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def camfix_cases(model=None):
    if model is not None:
        return [c for c in camfix_cases() if c.model == model]
    out = []
    for m in FIXTURE_MODELS:
        out += _fix_grid(m)
        out += _stops_and_iterations("camfix", m, (4, 6, 7, 1), WAVE + 1, 2 * PROD + 1)[:7]  # (max_iterations 0 and 1: one each)
        out += [c for c in _masks("camfix", m, (4, 6, 4, 7, 6, 1, 7)) if c.n <= 2 * PROD + 1 and (c.mask, c.loss) != ("ones", "TRUNCATED")]
        out += _rejection_cases("camfix", [(m, 4)], FIX_NS, 1) + _rejection_cases("camfix", [(m, 6)], FIX_NS, 1)
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def sfocal_cases():
    out = _sfocal_grid()
    out += _rejection_cases("sfocal", [(None, 0)], CAM_NS[1:])
    out += _stops_and_iterations("sfocal", None, (0,), WAVE + 1, 2 * PROD + 1)
    return list(dict.fromkeys(out))


def cases(kind, model=None):
    return cam_cases(model) if kind == "cam" else camfix_cases(model) if kind == "camfix" else sfocal_cases()


def all_cases():
    return cam_cases() + camfix_cases() + sfocal_cases()


# ---- the device ----------------------------------------------------------------------------------------------------------------------
def run_on_device(P, c, problems=None):
    """the case through Problem.bundle_adjust / refine_shared_focal_relpose of the product package P -> Result (invalid_steps -1: the
    C-ABI does not return them).  problems: a dict that keeps the Problem of a point set for the cases that follow (the caller
    closes them); without it the case's own problem is closed again."""
    a, b, model, bo, mask = inputs(c)
    start = P.CameraPose(model[:4], model[4:])
    if c.kind == "sfocal":
        pair, it = P.refine_shared_focal_relpose(a, b, P.ImagePair(start, P.Camera("SIMPLE_PINHOLE", [start_camera(c), 0, 0])), bo)
        return Result(np.r_[pair.pose.q, pair.pose.t], np.array([pair.camera1.params[0]]), it, -1)
    key = (c.model, a.tobytes(), b.tobytes())
    pr = problems.get(key) if problems is not None else None
    if pr is None:
        pr = P.Problem(P.KIND_ABS, a, b)
        if problems is not None:
            problems[key] = pr
    try:
        pose, cam, it = pr.bundle_adjust(start, start_camera(c), bo, mask=mask)
    finally:
        if problems is None:
            pr.close()
    return Result(np.r_[pose.q, pose.t], np.asarray(cam.params, dtype=np.float64), it, -1)


def refine_plain_on_device(P, c):
    """a case whose flags select no parameter through Problem.refine with the camera (pl_refine_model): (pose, iterations)"""
    a, b, model, bo, mask = inputs(c)
    pr = P.Problem(P.KIND_ABS, a, b)
    try:
        pose, it = pr.refine(P.CameraPose(model[:4], model[4:]), {k: v for k, v in bo.items() if not k.startswith("refine_")},
                             camera=start_camera(c), mask=mask)
    finally:
        pr.close()
    return np.r_[pose.q, pose.t], it
