"""Inputs and the numpy model of the pruned matrix-core absolute-pose scorer (tests/test_score_prune_rule.py on the CPU,
tests/test_gpu_score_prune.py on the device).  Everything here comes from the oracle, numpy and the library's host-only entries.

The model restates steps 1, 3 and 5 of the scorer: the lead's best count and score with the incumbent's place the split chunk c*;
a hypothesis behind the lead that has seen the S correspondences of the chunks [0, c*) with cs inliers is pruned iff
cs + (N - S) <= lead_max and sum r^2 + (S - cs) thr^2 > lead_min (1 + margin); a pruned hypothesis reports (cs, sum + (N - cs)
thr^2).  Per-point residuals are numpy's; the inlier flags are the oracle's (O.inliers), and reference() checks that the two
together reproduce the oracle's score of every model."""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from poselib_amd import api, synth

THR = 0.012
FOCAL = 1000.0
LEAD = 2048          # kPruneLead
MARGIN_POINTS = 32   # kPruneMargin
MARGIN_SCORE = 1e-6  # kPruneScoreMargin
RECORDS_MARGIN = 1e-9  # records_body
N_MAX = 2600
DBL_MAX = float(np.finfo(np.float64).max)
SINGLE, GROUP = 0, 2


# ---- the rules ------------------------------------------------------------------------------------------------------------------
def records_rule(counts, scores, init_max=0, init_min=DBL_MAX):
    """hypothesis indices records_body lists: c > emax or s < emin (1 + 1e-9), emax / emin the running values in front of k"""
    out = []
    emax, emin = int(init_max), float(init_min)
    for k, (c, s) in enumerate(zip(counts, scores)):
        if c > emax or s < emin * (1.0 + RECORDS_MARGIN):
            out.append(k)
        emax, emin = max(emax, int(c)), min(emin, float(s))
    return out


def split_chunk(lead_max, lead_min, N, thr2, chunk_points, chunks):
    """c*: the fewest chunks whose correspondences number max(lead_min / thr^2, N - lead_max) + MARGIN_POINTS, in 1 .. chunks"""
    need = max(lead_min / thr2, float(N - min(int(lead_max), N))) + MARGIN_POINTS
    if not need < N:
        return chunks
    return max(1, min(int(np.ceil(need / chunk_points)), chunks))


def prune_gate(kind, n_points, iterations):
    """score_prune_gate: matrix-core absolute pose, >= 8192 iterations in the step, >= 3 chunks"""
    shape = api.score_shape(kind, n_points, True, False) if kind == 0 else None
    return kind == 0 and shape is not None and iterations >= 8192 and shape[0] >= 3


def prune_model(r2, inl, live, thr2, chunk_points, init_max=0, init_min=DBL_MAX, margin=MARGIN_SCORE, lead=LEAD):
    """r2, inl: (H, N) residuals and inlier flags; live: (H,) hypotheses without a NaN entry.  Returns a dict with cstar, chunks,
    lead_max, lead_min, kept (H,), counts, scores (what finalize reports) and full_counts, full_scores."""
    H, N = r2.shape
    chunks = (N + chunk_points - 1) // chunk_points
    val = np.where(inl, r2, 0.0)
    full_c = inl.sum(axis=1).astype(np.int64)
    full_s = val.sum(axis=1) + (N - full_c) * thr2
    full_c = np.where(live, full_c, 0)
    full_s = np.where(live, full_s, N * thr2)
    pos = np.cumsum(live) - 1  # live position of hypothesis k
    in_lead = live & (pos < lead)
    lead_max, lead_min = int(init_max), float(init_min)
    if in_lead.any():
        lead_max, lead_min = max(lead_max, int(full_c[in_lead].max())), min(lead_min, float(full_s[in_lead].min()))
    cstar = split_chunk(lead_max, lead_min, N, thr2, chunk_points, chunks)
    S = min(cstar * chunk_points, N)
    cs = inl[:, :S].sum(axis=1).astype(np.int64)
    ss = val[:, :S].sum(axis=1)
    pruned = live & ~in_lead & (cs + (N - S) <= lead_max) & (ss + (S - cs) * thr2 > lead_min * (1.0 + margin))
    if cstar == chunks:
        pruned[:] = False
    counts = np.where(pruned, cs, full_c)
    scores = np.where(pruned, ss + (N - cs) * thr2, full_s)
    return {"cstar": cstar, "chunks": chunks, "lead_max": lead_max, "lead_min": lead_min, "kept": ~pruned, "counts": counts,
            "scores": scores, "full_counts": full_c, "full_scores": full_s}


# ---- scenes, lists, references ----------------------------------------------------------------------------------------------------
class Scene:
    """N_MAX correspondences of synth.absolute_pose_scene (0.5 px noise, 12 px threshold), normalised; case N is the first N"""

    def __init__(self, outlier_ratio, seed):
        d = synth.absolute_pose_scene(N_MAX, outlier_ratio, seed)
        self.a = np.ascontiguousarray((np.asarray(d["p2d"]) - 500.0) / FOCAL)
        self.b = np.ascontiguousarray(np.asarray(d["p3d"], float))
        self.gt = np.r_[np.asarray(d["q_gt"], float), np.asarray(d["t_gt"], float)]
        self.inlier_gt = np.asarray(d["inlier_gt"])
        self.ratio = outlier_ratio

    def points(self, N):
        return self.a[:N], self.b[:N]

    def p3p_models(self, N, count, seed):
        """`count` oracle P3P models of random minimal samples of the first N correspondences, in sample order"""
        rs = np.random.RandomState(seed)
        out = []
        while len(out) < count:
            i = rs.choice(N, 3, replace=False)
            x = np.c_[self.a[i], np.ones(3)]
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            out.extend(O.p3p(x, self.b[i]))
        return np.array(out[:count])


SCENE_SEEDS = {0.1: 9101, 0.7: 9107, 1.0: 9110}


@functools.lru_cache(maxsize=None)
def scene(outlier_ratio):
    return Scene(outlier_ratio, SCENE_SEEDS[outlier_ratio])


def quat_to_rotmat(q):
    return synth.quat_to_rotmat(np.asarray(q, dtype=np.float64))


def reference(sc, N, models):
    """(r2, inl, live) of `models` on the first N correspondences of the scene: residuals as scoring.cc's msac_reproj forms them, the
    oracle's inlier flags; checked model by model against the oracle's count and score"""
    a, b = sc.points(N)
    H = len(models)
    thr2 = THR ** 2
    live = ~np.isnan(models).any(axis=1)
    r2 = np.full((H, N), np.inf)
    inl = np.zeros((H, N), bool)
    for k in np.flatnonzero(live):
        q, t = models[k][:4], models[k][4:]
        Z = b @ quat_to_rotmat(q).T + t
        with np.errstate(divide="ignore", invalid="ignore"):
            e0 = Z[:, 0] * (1.0 / Z[:, 2]) - a[:, 0]
            e1 = Z[:, 1] * (1.0 / Z[:, 2]) - a[:, 1]
        r2[k] = e0 * e0 + e1 * e1
        inl[k] = O.inliers("reproj", models[k], a, b, thr2)
        s, c = O.score("reproj", models[k], a, b, thr2)
        assert c == inl[k].sum(), (k, c, int(inl[k].sum()))
        mine = r2[k][inl[k]].sum() + (N - c) * thr2
        assert abs(mine - s) <= 1e-12 * abs(s), (k, mine, s)
    return r2, inl, live


def perturbed_gt(sc, size, seed):
    """the ground truth moved by `size`: keeps nearly all of its inliers for size <= 1e-5"""
    rs = np.random.RandomState(seed)
    q = sc.gt[:4] + size * rs.randn(4)
    return np.r_[q / np.linalg.norm(q), sc.gt[4:] + size * rs.randn(3)]


def nan_model(m, which):
    m = np.array(m, float)
    m[[1, 4, 6][which % 3]] = np.nan
    return m


def chunk_points(N, route):
    return 64 * api.score_shape(0, N, True, route == GROUP)[1]


@functools.lru_cache(maxsize=None)
def point_counts():
    """From pl_debug_score_shape.  The matrix-core scorer starts at 1024 correspondences, i.e. at four chunks: the smallest exact
    fills (single launch: 4 x 256; both forms: 4 x 320), an exact fill plus one correspondence = a last chunk of one correspondence,
    and a count of nine chunks whose c* falls in the middle at 70 % outliers."""
    exact4 = [n for n in range(1024, 1400) if api.score_shape(0, n, True, False) == (4, 4) and n == 4 * 256]
    exact5 = [n for n in range(1024, 1400) if api.score_shape(0, n, True, False) == (4, 5) and n == 4 * 320]
    assert exact4 == [1024] and exact5 == [1280], (exact4, exact5)
    assert api.score_shape(0, 1281, True, False) == (5, 5) and api.score_shape(0, 1281, True, True) == (5, 5)
    assert api.score_shape(0, N_MAX, True, False) == (9, 5)
    return (1024, 1280, 1281, N_MAX)
