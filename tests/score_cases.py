"""Inputs of the streaming-scorer tests (tests/test_gpu_score_stream.py on the device, tests/test_score_cases.py on the CPU): point
counts at the edges of the scorers' chunk shapes, scenes, one long model list per scene and the oracle's counts and scores of it.
Everything here comes from the oracle, numpy and the library's host-only shape entry (pl_debug_score_shape) - no device.

A case is (kind, path, route, N, slices, H): the first N correspondences of the kind's scene, scored against the first H models of
the kind's base list on a grid of `slices` workgroups per chunk.  Scenes and base lists are built once; the oracle scores a
(scene prefix, model) pair at most once."""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from poselib_amd import api, synth
from test_gpu_full_size import _plant_at_threshold

KINDS = (0, 1, 2, 3)
THR = {0: 0.012, 1: 1e-3, 2: 1e-3, 3: 1e-3}
OKIND = {0: "reproj", 1: "sampson_pose", 2: "sampson_F", 3: "homography"}
FOCAL = 1000.0
N_SCAN = 2600  # point counts are scanned up to here
N_MIN = 8      # the smallest problem (a minimal sample of every kind fits)
N_GROUP_QUEUE = 300  # the queue member of the group launches
QUEUE, MFMA = 1, 2   # path_used of pl_debug_score_stream
SINGLE, GROUP = 0, 2  # route of pl_debug_score_stream_ex
WAVES = 8  # wavefronts per workgroup of the streaming scorers: `slices` workgroups per chunk are w = 8 slices wavefronts


# ---- list lengths -------------------------------------------------------------------------------------------------------------------
def list_lengths(slices, fulls=None):
    """H = 64 (full + rest) - d: `full` units of 64 hypotheses in whole ticket rounds of w wavefronts, `rest` units behind them at
    the thresholds of the tail rule (rest * 4 <= w: sub-units of 16, rest * 2 <= w: of 32, else 64), a ragged last unit."""
    w = WAVES * slices
    out = {1, 31, 32, 33}
    for full in ((0, w, 2 * w) if fulls is None else fulls):
        for rest in (0, w // 4, w // 4 + 1, w // 2, w // 2 + 1, w - 1):
            for d in (0, 1, 33, 49):
                if 64 * (full + rest) - d > 0:
                    out.add(64 * (full + rest) - d)
    return sorted(out)


# slices -> lengths: the full set for 1 and 3 (3: whole rounds up to w), the `full` = w subset for 2 and 5
LENGTHS = {1: list_lengths(1), 3: list_lengths(3, (0, 24)), 2: list_lengths(2, (16,)), 5: list_lengths(5, (40,))}
BASE = max(max(v) for v in LENGTHS.values())  # models per base list: every list under test is a prefix
H_SWEEP = 1089  # the list of the point-count sweep: 17 units and one hypothesis
SWEEP_SLICES = 2


def round_straddles(slices):
    """lengths around the end of the first and the second ticket round of `slices` workgroups"""
    w = WAVES * slices
    return [64 * w * r + e for r in (1, 2) for e in (-1, 0, 1) if 64 * w * r + e <= BASE]


# ---- point counts -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_scan(kind, path, route):
    """{N: (chunks, points per lane)} for every N in N_MIN .. N_SCAN that a problem of `kind` takes on `path`"""
    out = {}
    for n in range(N_MIN, N_SCAN + 1):
        on_mfma = api.score_shape(kind, n, True, route == GROUP) is not None
        if on_mfma == (path == MFMA):
            out[n] = api.score_shape(kind, n, path == MFMA, route == GROUP)
    return out


@functools.lru_cache(maxsize=None)
def point_counts(kind, path, route):
    """The path's smallest N (and the last N of the queue path, the other side of the matrix-core path's first), and per points-per-lane
    value of the scan: the largest N that fills every chunk exactly and that N + 1, the largest whose last chunk holds exactly one
    valid correspondence, the largest whose last group of 32 holds 31."""
    scan = shape_scan(kind, path, route)
    ns = {min(scan)}
    if path == QUEUE:
        ns.add(max(scan))
        if route == GROUP:
            ns.add(N_GROUP_QUEUE)
    for P in sorted({p for _, p in scan.values()}):
        sel = [n for n, (_, p) in scan.items() if p == P]
        exact = [n for n in sel if n == scan[n][0] * 64 * P]
        if exact:
            ns.add(max(exact))
            if max(exact) + 1 in scan:
                ns.add(max(exact) + 1)
        one = [n for n in sel if scan[n][0] >= 2 and n == (scan[n][0] - 1) * 64 * P + 1]
        if one:
            ns.add(max(one))
        g31 = [n for n in sel if n % 32 == 31]
        if g31:
            ns.add(max(g31))
    return sorted(ns)


def all_point_counts(kind):
    return sorted({n for path in (QUEUE, MFMA) for route in (SINGLE, GROUP) for n in point_counts(kind, path, route)})


def fill_pair(kind, path, route=SINGLE):
    """two N of the path for the list-length sets: one that fills its chunks exactly and a ragged one (a last group of 31)"""
    scan = shape_scan(kind, path, route)
    ns = point_counts(kind, path, route)
    exact = [n for n in ns if n == scan[n][0] * 64 * scan[n][1]]
    ragged = [n for n in ns if n % 32 == 31]
    return max(exact), max(ragged)


def workgroup_pairs(kind):
    """(class, N, slices) with T = slices x chunks of the matrix-core single launch in each class of slice_chunk_of_workgroup's
    numbering: T < 8, and T > 8 with T mod 8 = 0, 1, 7"""
    scan = shape_scan(kind, MFMA, SINGLE)
    want = {"T<8": lambda T: T < 8, "0": lambda T: T > 8 and T % 8 == 0, "1": lambda T: T > 8 and T % 8 == 1,
            "7": lambda T: T > 8 and T % 8 == 7}
    out = []
    for name, ok in want.items():
        hit = [(n, s) for n in point_counts(kind, MFMA, SINGLE) for s in range(1, 9) if ok(s * scan[n][0])]
        if hit:
            out.append((name,) + hit[0])
    return out


# ---- scenes and base lists ------------------------------------------------------------------------------------------------------------
def _rot(q):
    return synth.quat_to_rotmat(np.asarray(q, dtype=np.float64))


def _essential(q, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ _rot(q)


GOOD_EVERY = 8


def is_good(k):
    """base model k is the ground truth (k = 0) or a perturbation of it by 1e-6 .. 1e-5, which keeps nearly all of its inliers: two
    in every run of 16.  (The perturbations of 1e-5 .. 1e-3 at k % 8 == 4 move the errors by up to a threshold; they fit, but the
    coverage conditions cannot lean on them.)"""
    return k % GOOD_EVERY == 0


def is_near(k):
    return k % 4 == 0


def _base_models(kind, d, a, b, rs):
    """BASE models: k % 4 == 0 the ground truth perturbed by 1e-6 .. 1e-3 (every other one by at most 1e-5: the good models,
    k = 0 the ground truth itself), k % 16 == 5 hostile (infinite translation, the zero
    matrix, huge and tiny scales), the others random"""
    q, t = np.asarray(d["q_gt"], float), np.asarray(d["t_gt"], float)
    if kind == 2:
        gt = _essential(q, t)
    elif kind == 3:  # a homography from the true inliers (least squares)
        inl = np.flatnonzero(d["inlier_gt"])[:200]
        rows = []
        for (u0, v0), (u1, v1) in zip(a[inl], b[inl]):
            p = np.array([u0, v0, 1.0])
            rows.append(np.r_[p, 0, 0, 0, -u1 * p])
            rows.append(np.r_[0, 0, 0, p, -v1 * p])
        gt = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    models = []
    for k in range(BASE):
        s = 0.0 if k == 0 else 10.0 ** (rs.uniform(-6, -5) if is_good(k) else rs.uniform(-5, -3))
        hostile = (k // 16) % 5
        if kind in (0, 1):
            if is_near(k):
                qq = q + s * rs.randn(4)
                m = np.r_[qq / np.linalg.norm(qq), t + s * rs.randn(3)]
            elif k % 16 == 5:
                m = [np.r_[q, 0.0, np.inf, 1.0], np.r_[q, 0.0, 0.0, 0.0], np.r_[q, t * 1e6], np.r_[q, t * 1e-6], np.r_[2.0 * q, t]][hostile]
            else:
                qq = rs.randn(4)
                m = np.r_[qq / np.linalg.norm(qq), rs.randn(3) * (3.0 if kind == 0 else 1.0)]
        else:
            if is_near(k):
                m = gt + s * np.abs(gt).max() * rs.randn(3, 3)
            elif k % 16 == 5:
                m = [np.diag([1.0, 1.0, np.inf]), np.zeros((3, 3)), gt * 1e15, gt * 1e-12, -gt * 1e4][hostile]
            else:
                m = rs.randn(3, 3)
        models.append(m)
    return np.array(models)


class Scene:
    """N_SCAN + 1 correspondences with 50 % outliers, normalised; case N is the first N of them.  The order is a shuffle in which the
    last correspondence of every case N is an inlier of every good model."""

    def __init__(self, kind):
        self.kind, self.thr = kind, THR[kind]
        n = N_SCAN + 1
        rs = np.random.RandomState(8100 + kind)
        if kind == 0:
            d = synth.absolute_pose_scene(n, 0.5, 8200)
            a, b = (np.asarray(d["p2d"]) - 500.0) / FOCAL, np.asarray(d["p3d"], float)
            # half of the correspondences sit at the decision boundary of the first model
            planted = _plant_at_threshold(d["q_gt"], np.asarray(d["t_gt"], float), b, self.thr, rs)
            self.planted = rs.rand(n) < 0.5
            a[self.planted] = planted[self.planted]
        else:
            gen = {1: synth.relative_pose_scene, 2: synth.fundamental_scene, 3: synth.homography_scene}[kind]
            d = gen(n, 0.5, 8200 + kind)
            a, b = (np.asarray(d["x1"], float) - 500.0) / FOCAL, (np.asarray(d["x2"], float) - 500.0) / FOCAL
            self.planted = np.zeros(n, bool)
        self.models = _base_models(kind, d, a, b, rs)
        mask = self._masks(a, b)
        solid = mask[[k for k in range(BASE) if is_good(k)]].all(axis=0)  # inliers of every good model
        order = rs.permutation(n)
        ends = [N - 1 for N in all_point_counts(kind)]
        free = [j for j in range(n) if j not in set(ends) and solid[order[j]]]
        for e in ends:
            if not solid[order[e]]:
                j = free.pop()
                order[e], order[j] = order[j], order[e]
        self.a, self.b = np.ascontiguousarray(a[order]), np.ascontiguousarray(b[order])
        self.planted = self.planted[order]
        self.mask = np.ascontiguousarray(mask[:, order])  # (BASE, n): the oracle's inlier flags
        self._ref = {}

    def _masks(self, a, b):
        return np.array([O.inliers(OKIND[self.kind], self.models[k], a, b, self.thr ** 2) for k in range(BASE)])

    def points(self, N):
        return self.a[:N], self.b[:N]

    def reference(self, N, H):
        """the oracle's (counts, scores) of the first H base models on the first N correspondences"""
        cnt, sc = self._ref.setdefault(N, (np.zeros(BASE, np.int64), np.zeros(BASE)))
        done = self._ref.setdefault(("done", N), [0])
        a, b = self.points(N)
        for k in range(done[0], H):
            sc[k], cnt[k] = O.score(OKIND[self.kind], self.models[k], a, b, self.thr ** 2)
        done[0] = max(done[0], H)
        return cnt[:H], sc[:H]


@functools.lru_cache(maxsize=None)
def scene(kind):
    return Scene(kind)


def chunk_inliers(kind, N, per_chunk):
    """(good models, chunks): the oracle's inliers of every good model in every chunk of `per_chunk` correspondences of case N"""
    m = scene(kind).mask[::GOOD_EVERY, :N]
    edges = np.arange(0, N, per_chunk)
    return np.add.reduceat(m.astype(np.int64), edges, axis=1)
