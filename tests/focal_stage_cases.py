"""Inputs of the stage-level tests of the two focal-length estimators' kernels (tests/test_gpu_focal_stages.py on the device,
tests/test_focal_stage_cases.py on the CPU): focal.hip (ransac_pnpf) and sfocal.hip (ransac_shared_focal_relpose) - generator, the two
scorers and the mask kernel of each, single and group form, through pl_debug_focal_stage.  A deterministic table in the manner of
tests/score_cases.py and tests/lm_cam_cases.py; every expected value is the oracle's (oracle_lib.score_image / inliers_image /
score_shared_focal / inliers_shared_focal / generate_focal).  Everything here comes from the oracle, synth and numpy - no device.

`which` 0 is the absolute pose with unknown focal length (image points about the principal point in pixels, threshold 4 px), 1 the
shared-focal relative pose (both images' points about the principal point, divided by 500 as a front-end's normalisation would; the
true focal length is then 2).  A problem of n correspondences is the first n of the estimator's scene of 500.

What the sizes are for: a wavefront of the scorers walks 64 correspondences at a time, the workgroup form 192 per round through two
LDS buffers (a third round rewrites buffer 0), the solve kernels take 4 iterations per workgroup, and the score launchers switch
from the workgroup form to the wavefront form above 1024 slots."""
from __future__ import annotations

import collections
import functools
import os
import re

import numpy as np

import oracle_lib as O
from poselib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_constant(source, pattern):
    return int(re.search(pattern, open(os.path.join(ROOT, "poselib_amd", "csrc", source)).read()).group(1))


SCORE_THREADS = (_kernel_constant("focal.hip", r"constexpr int kFocalScoreThreads = (\d+);"),
                 _kernel_constant("sfocal.hip", r"constexpr int kSFocalScoreThreads = (\d+);"))                     # 256, 256
WAVE = _kernel_constant("focal.hip", r"constexpr int kScoreProd = kFocalScoreThreads - (\d+);")                    # 64
assert WAVE == _kernel_constant("sfocal.hip", r"constexpr int kSfScoreProd = kSFocalScoreThreads - (\d+);")
assert WAVE == _kernel_constant("focal.hip", r"for \(uint32_t base = 0; base < a\.n; base \+= (\d+)u\)")
assert WAVE == _kernel_constant("sfocal.hip", r"for \(uint32_t base = 0; base < a\.n; base \+= (\d+)u\)")
assert SCORE_THREADS[0] == SCORE_THREADS[1]
ROUND = SCORE_THREADS[0] - WAVE                                                                                    # 192
SOLVE_WAVES = _kernel_constant("focal.hip", r"constexpr int kSolveWaves = (\d+);")                                 # 4
assert SOLVE_WAVES == _kernel_constant("sfocal.hip", r"constexpr int kSolveWaves = (\d+),")
SWITCH = _kernel_constant("focal.hip", r"if \(a\.num_slots <= (\d+)u\)")                                           # 1024
assert SWITCH == _kernel_constant("sfocal.hip", r"if \(a\.num_slots <= (\d+)u\)")
MAX_MODELS = (_kernel_constant("pl_focal.h", r"constexpr int kFocalMaxModels = (\d+);"),
              _kernel_constant("pl_sfocal.h", r"constexpr int kSFocalMaxModels = (\d+);"))                         # 10, 60
SAMPLE = (_kernel_constant("pl_focal.h", r"constexpr int kFocalSample = (\d+);"),
          _kernel_constant("pl_sfocal.h", r"constexpr int kSFocalSample = (\d+);"))                                # 4, 6

WHICH = (0, 1)
NAMES = ("pnpf", "sfocal")
KIND = (0, 2)  # the resident problem's kind: absolute pose, two views
N_SCENE = 500
NS = (1, 63, 64, 65, 191, 192, 193, 384, 385, 500)
assert {WAVE - 1, WAVE, WAVE + 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND, 2 * ROUND + 1} <= set(NS) and max(NS) == N_SCENE
GEN_BS = (1, 3, 4, 5, 63, 64, 65, 257)
assert {SOLVE_WAVES - 1, SOLVE_WAVES, SOLVE_WAVES + 1, WAVE - 1, WAVE, WAVE + 1, 4 * WAVE + 1} <= set(GEN_BS)
GEN_NS = ((4, 5, 300), (6, 7, 300))  # the two smallest: the sampler redraws duplicates most of the time
SLOT_COUNTS = (1, 5, SWITCH, SWITCH + 1)
GATED_BS = ((102, 103), (17, 18))  # iterations whose slots lie on both sides of the switch: 1020 / 1030 and 1020 / 1080
for _w in WHICH:
    assert GATED_BS[_w][0] * MAX_MODELS[_w] <= SWITCH < GATED_BS[_w][1] * MAX_MODELS[_w]
GATE_NS = (WAVE + 1, N_SCENE)
SEED = 20240
REBASE = 7  # test 1: the iterations from here on, drawn with pos_base = their first position
SCALE = 500.0
THR2 = (16.0, (2.0 / SCALE) ** 2)
UNWRITTEN = 0xFFFFFFFF
FILL = float(np.frombuffer(b"\x5a" * 8, dtype=np.float64)[0])  # the prefill of everything that is no counter: a finite double
assert np.isfinite(FILL)


@functools.lru_cache(maxsize=None)
def scene(which, outliers=0.4, seed=None, noise=None):
    """(a, b, gt model [q t f]) of the estimator's scene of N_SCENE correspondences"""
    if which == 0:
        d = synth.absolute_pose_scene(N_SCENE, outliers, 6101 if seed is None else seed, noise_px=1.0 if noise is None else noise)
        f, cx, cy = d["camera"]["params"]
        a, b = np.asarray(d["p2d"]) - [cx, cy], np.asarray(d["p3d"])
    else:
        d = synth.relative_pose_scene(N_SCENE, outliers, 6200 if seed is None else seed, noise_px=0.5 if noise is None else noise)
        f, cx, cy = d["camera1"]["params"]
        a, b = (np.asarray(d["x1"]) - [cx, cy]) / SCALE, (np.asarray(d["x2"]) - [cx, cy]) / SCALE
        f = f / SCALE
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    a.setflags(write=False), b.setflags(write=False)
    return a, b, np.r_[d["q_gt"], d["t_gt"], f]


def points(which, n):
    a, b, _ = scene(which)
    return a[:n], b[:n]


def _perturbed(m, eps):
    q = m[:4] + eps * np.array([0.0, 1.0, -1.0, 0.5])
    return np.r_[q / np.linalg.norm(q), m[4:7] * (1.0 + 0.5 * eps) + eps * np.array([0.3, -0.2, 0.1]), m[7] * (1.0 - eps)]


MODEL_GROUPS = ("hypothesis", "truth", "behind", "focal", "nan")


@functools.lru_cache(maxsize=None)
def models(which):
    """(labels, (L, 8) models): the oracle's own hypotheses on the noisy scene (few inliers), the ground truth and perturbations of it
    (most points inliers), for pnpf the truth with t negated (part of the scene behind the camera), f = 0 / negative / +inf, a NaN in
    q, in t and in f"""
    a, b, gt = scene(which)
    samples, _ = O.sampler_draw_positions(SEED + 1, N_SCENE, SAMPLE[which], 200)
    counts, hyp = O.generate_focal(which, a, b, samples)
    out, labels = [], []
    for i in range(len(samples)):
        for m in range(min(int(counts[i]), 2)):
            if len(out) < 20:
                out.append(hyp[i, m].copy()), labels.append("hypothesis")
    for eps in (0.0, 1e-4, 3e-4, 5e-4):
        out.append(_perturbed(gt, eps)), labels.append("truth")
    if which == 0:
        out.append(np.r_[gt[:4], -gt[4:7], gt[7]]), labels.append("behind")
    for f in (0.0, -gt[7], np.inf):
        out.append(np.r_[gt[:7], f]), labels.append("focal")
    for at in (1, 4, 7):
        m = _perturbed(gt, 1e-3)
        m[at] = np.nan
        out.append(m), labels.append("nan")
    M = np.ascontiguousarray(out)
    M.setflags(write=False)
    return tuple(labels), M


Score = collections.namedtuple("Score", "count value r2")  # value: the inlier sum (pnpf) / the MSAC score (shared focal)


def score_of(which, model, a, b, thr2):
    """what the device's scorer returns for one model: (count, inlier sum | MSAC score, per-point r2)"""
    with np.errstate(all="ignore"):
        if which == 0:
            isum, cnt, r2, _ = O.score_image(model[:7], model[7], a, b, thr2)
            return Score(cnt, isum, r2)
        msac, cnt, r2 = O.score_shared_focal(model[:7], model[7], a, b, thr2)
        return Score(cnt, msac, r2)


def mask_of(which, model, a, b, thr2):
    """(mask, per-point r2 in the mask's own form)"""
    with np.errstate(all="ignore"):
        if which == 0:
            return O.inliers_image(model[:7], model[7], a, b, thr2)
        return O.inliers_shared_focal(model[:7], model[7], a, b, thr2)


@functools.lru_cache(maxsize=None)
def expected_scores(which, n):
    """(counts (L,), values (L,)) of models(which) on the first n correspondences at THR2"""
    a, b = points(which, n)
    sc = [score_of(which, m, a, b, THR2[which]) for m in models(which)[1]]
    return np.array([s.count for s in sc], dtype=np.uint32), np.array([s.value for s in sc])


@functools.lru_cache(maxsize=None)
def expected_masks(which, n):
    a, b = points(which, n)
    return np.array([mask_of(which, m, a, b, THR2[which])[0] for m in models(which)[1]]).reshape(len(models(which)[1]), n)


def padded(which, slots):
    """the model list repeated up to `slots` slots, and each slot's index into the list"""
    M = models(which)[1]
    idx = np.arange(slots) % len(M)
    return np.ascontiguousarray(M[idx]), idx


# ---------------------------------------------------------------------------------------- inlier patterns by index
Pattern = collections.namedtuple("Pattern", "which name n a b model inliers")
PATTERN_NS = (1, WAVE + 1, ROUND + 1, 2 * ROUND + 1, N_SCENE)


def _pattern_sets(n):
    sets = {"first": {0}, "last": {n - 1}, "all": set(range(n)), "none": set()}
    if n > WAVE:
        sets["wave edge"] = {WAVE - 1, WAVE}
    if n > ROUND:
        sets["round edge"] = {ROUND - 1, ROUND}
        sets["beyond the first round"] = set(range(ROUND, n))
    return sets


@functools.lru_cache(maxsize=None)
def patterns(which):
    """ground-truth scenes (no outliers) in which every correspondence outside the pattern is corrupted until the oracle calls it an
    outlier: the inliers lie exactly at the pattern's indices"""
    a0, b0, gt = scene(which, 0.0, 6300 + which, 0.25)  # (noise well inside the threshold: every untouched point is an inlier)
    rng = np.random.default_rng(77 + which)
    thr2 = THR2[which]
    out = []
    for n in PATTERN_NS:
        for name, keep in _pattern_sets(n).items():
            a = a0[:n].copy()
            bad = np.array([i not in keep for i in range(n)])
            amp = 300.0 if which == 0 else 300.0 / SCALE
            for _ in range(50):
                if not bad.any():
                    break
                a[bad] = a0[:n][bad] + rng.uniform(0.2, 1.0, (int(bad.sum()), 2)) * amp * rng.choice([-1.0, 1.0], (int(bad.sum()), 2))
                r2 = score_of(which, gt, a, b0[:n], thr2).r2
                bad = np.array([i not in keep for i in range(n)]) & (r2 < 4.0 * thr2)  # (well outside: the mask's form agrees)
            a.setflags(write=False)
            out.append(Pattern(which, name, n, a, b0[:n], gt, np.array(sorted(keep), dtype=np.int64)))
    return tuple(out)


# ---------------------------------------------------------------------------------------- thresholds on a residual
Tie = collections.namedtuple("Tie", "which stage n model k thr2 inside")  # stage "score" | "mask"; inside: point k is an inlier
TIE_N = 2 * ROUND + 1
TIE_POINTS = (WAVE - 1, ROUND, 2 * ROUND)  # last lane of a chunk, first correspondence of the second round, the third round's only one


def tie_model(which):
    return models(which)[1][models(which)[0].index("truth") + 1]


@functools.lru_cache(maxsize=None)
def ties(which):
    """thr2 = the oracle's r2 of point k (the comparison is strict: k is out), then the next double (k is in) - for the score with
    the score's residual and for the mask with the mask's own"""
    a, b = points(which, TIE_N)
    m = tie_model(which)
    out = []
    for stage, r2 in (("score", score_of(which, m, a, b, THR2[which]).r2), ("mask", mask_of(which, m, a, b, THR2[which])[1])):
        usable = [k for k in range(TIE_N) if np.isfinite(r2[k]) and r2[k] > 0]
        for want in TIE_POINTS:
            k = min(usable, key=lambda j: abs(j - want))
            out.append(Tie(which, stage, TIE_N, m, k, float(r2[k]), False))
            out.append(Tie(which, stage, TIE_N, m, k, float(np.nextafter(r2[k], np.inf)), True))
    return tuple(out)


Split = collections.namedtuple("Split", "n model k thr2 counted masked")
SPLIT_N = 2 * ROUND + 1
SPLITS_EACH_WAY = 8


@functools.lru_cache(maxsize=None)
def splits():
    """pnpf: the score multiplies by 1 / z, the mask divides by z, and the two residuals of a point differ in the last bits for a
    good part of the scene.  A threshold equal to the larger of the two takes the point on one side only.  Returns (cases, number of
    points counted-not-masked, number masked-not-counted) on the SPLIT_N correspondences of the scene."""
    a, b = points(0, SPLIT_N)
    m = tie_model(0)
    rs, rm = score_of(0, m, a, b, THR2[0]).r2, mask_of(0, m, a, b, THR2[0])[1]
    ok = np.isfinite(rs) & np.isfinite(rm)
    low_s, low_m = np.flatnonzero(ok & (rs < rm)), np.flatnonzero(ok & (rm < rs))
    out = [Split(SPLIT_N, m, int(k), float(rm[k]), True, False) for k in low_s[:SPLITS_EACH_WAY]]
    out += [Split(SPLIT_N, m, int(k), float(rs[k]), False, True) for k in low_m[:SPLITS_EACH_WAY]]
    return tuple(out), len(low_s), len(low_m)


# ---------------------------------------------------------------------------------------- the generator
Generated = collections.namedtuple("Generated", "which n a b samples positions counts models")
GEN_B = max(GEN_BS)


@functools.lru_cache(maxsize=None)
def generated(which, n, max_focal=-1.0):
    """the oracle estimator's generate on the sampler's first GEN_B samples of the first n correspondences (with the draws consumed
    before each: the device's positions)"""
    a, b = points(which, n)
    samples, positions = O.sampler_draw_positions(SEED, n, SAMPLE[which], GEN_B)
    with np.errstate(all="ignore"):
        counts, mods = O.generate_focal(which, a, b, samples, max_focal)
    return Generated(which, n, a, b, samples, positions, counts, mods)


@functools.lru_cache(maxsize=None)
def solver_output(n):
    """P3.5Pf on every sample of generated(0, n) with every solution kept: [(poses (m, 7), focals (m,))]"""
    g = generated(0, n)
    with np.errstate(all="ignore"):
        return tuple(O.p35pf(g.a[s.astype(np.int64)], g.b[s.astype(np.int64)]) for s in g.samples)


def solver_inputs(n):
    """the samples of generated(0, n) as explicit minimal problems [x 4 x 2 | X 4 x 3] (pl_solve_focal_batch)"""
    g = generated(0, n)
    idx = g.samples.astype(np.int64)
    return np.ascontiguousarray(np.c_[g.a[idx].reshape(len(idx), 8), g.b[idx].reshape(len(idx), 12)])


FILTER_N = 300


@functools.lru_cache(maxsize=None)
def max_focals():
    """{name: bound}: none, zero, the median of the focal lengths the unbounded estimator keeps, and a bound bit-equal to one kept
    solution's focal length (the comparison is strict: that solution stays)"""
    g = generated(0, FILTER_N)
    kept = np.sort(np.concatenate([g.models[i, : g.counts[i], 7] for i in range(GEN_B)]))
    median = float(kept[len(kept) // 2 - 1] + kept[len(kept) // 2]) / 2.0
    return {"none": -1.0, "zero": 0.0, "median": median, "equal": float(kept[len(kept) // 3])}


def apply_filter(poses, focals, max_focal):
    """the estimator's rule (absolute_pose.cc:89-95) on a solver's output"""
    keep = [i for i in range(len(focals)) if not focals[i] < 0 and not (max_focal >= 0 and focals[i] > max_focal)]
    return np.c_[poses[keep].reshape(len(keep), 7), focals[keep].reshape(len(keep), 1)]


# ---------------------------------------------------------------------------------------- gated score launches
GATE_CYCLE = ((0, 1, 10, 3, 0, 9, 4, 5, 2), (0, 1, 60, 4, 0, 5, 8, 9, 3, 59))  # models per iteration, repeated over the batch


def gated(which, B):
    """(models (B x max_models, 8), num_models (B,), slot -> index into models(which) or -1 for an empty slot).  Empty slots hold a
    model too - the ground truth - so a scorer that ignored the gate would leave a count there."""
    M = models(which)[1]
    maxm = MAX_MODELS[which]
    num = np.array([GATE_CYCLE[which][b % len(GATE_CYCLE[which])] for b in range(B)], dtype=np.uint32)
    idx = np.full(B * maxm, -1, dtype=np.int64)
    slots = np.tile(scene(which)[2], (B * maxm, 1))
    at = 0
    for b in range(B):
        for m in range(int(num[b])):
            idx[b * maxm + m] = at % len(M)
            slots[b * maxm + m] = M[at % len(M)]
            at += 1
    return np.ascontiguousarray(slots), num, idx


# ---------------------------------------------------------------------------------------- group members
GROUP_NS = (N_SCENE, ROUND + 1)  # the full member's problem and the short member's
