"""Inputs of the generator tests (tests/test_gpu_generators.py on the device, tests/test_generator_cases.py on the CPU): point sets,
sample streams and the oracle's generate_models on them.  Everything here comes from the oracle and numpy alone - no device."""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from poselib_amd import synth

# the wavefront (64), the workgroup of k_rel_poses and the pitch of the staged workspace (256), the accounting block (1024)
ITERATION_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500]
B_MAX = max(ITERATION_COUNTS)
K = O.GENERATE_K
MAX_MODELS = O.GENERATE_MAX
FOCAL = 1000.0
SEED = 20  # of every sample stream
SMALL_SETS = ["abs8", "abs11", "rel8", "rel11", "fund8", "fund11", "hom8", "hom11"]


@functools.lru_cache(maxsize=None)
def points(name):
    """(kind, a, b) of a named point set: normalised image points, 3-D points for kind 0"""
    if name == "abs":  # 300 correspondences, 30 % outliers
        d = synth.absolute_pose_scene(300, 0.3, 6101)
        return 0, (np.asarray(d["p2d"]) - 500.0) / FOCAL, np.asarray(d["p3d"], float)
    if name == "rel":
        d = synth.relative_pose_scene(300, 0.3, 6102)
        return 1, (d["x1"] - 500.0) / FOCAL, (d["x2"] - 500.0) / FOCAL
    if name == "fund":
        d = synth.fundamental_scene(350, 0.3, 6103)
        return 2, (d["x1"] - 500.0) / FOCAL, (d["x2"] - 500.0) / FOCAL
    if name == "hom":
        d = synth.homography_scene(250, 0.3, 6104)
        return 3, (d["x1"] - 500.0) / FOCAL, (d["x2"] - 500.0) / FOCAL
    if name in SMALL_SETS:  # a handful of correspondences: the sampler redraws an index in most samples
        base = name.rstrip("0123456789")
        kind, a, b = points(base)
        n = int(name[len(base):])
        return kind, np.ascontiguousarray(a[:n]), np.ascontiguousarray(b[:n])
    raise KeyError(name)


class Reference:
    """The oracle's generate_models on B_MAX samples of a point set; a case of B iterations is its first B samples."""

    def __init__(self, name, samples, positions=None, real_focal_check=False):
        self.name = name
        self.kind, self.a, self.b = points(name)
        self.samples = np.ascontiguousarray(samples, dtype=np.uint64)
        self.positions = positions  # draws consumed before each sample (stream of SEED), or None: no stream behind the samples
        self.real_focal_check = real_focal_check
        self.counts, self.models, self.sample_in = O.generate_models(self.kind, self.a, self.b, self.samples, real_focal_check)
        slot = np.arange(self.models.shape[1])[None, :] < self.counts[:, None]
        self.nan = np.isnan(self.models).any(axis=2) & slot  # (B, max_models): the model holds a NaN

    @property
    def B(self):
        return self.samples.shape[0]

    def block_sums(self, B, counts=None, nan=None):
        """models and NaN models per 1024 iterations of the first B"""
        counts = self.counts[:B] if counts is None else counts
        nan = self.nan[:B] if nan is None else nan
        edges = np.arange(0, B, 1024)
        return np.add.reduceat(counts.astype(np.int64), edges), np.add.reduceat(nan.sum(axis=1).astype(np.int64), edges)


@functools.lru_cache(maxsize=None)
def reference(name, real_focal_check=False):
    """the uniform sampler's stream of SEED on the point set"""
    kind, a, _ = points(name)
    idx, pos = O.sampler_draw_positions(SEED, a.shape[0], K[kind], B_MAX)
    assert (idx == O.sampler_draw(SEED, a.shape[0], K[kind], B_MAX)[0]).all()
    return Reference(name, idx, pos, real_focal_check)


@functools.lru_cache(maxsize=None)
def rel_rich():
    """The samples of reference("rel") with the ones that yield most poses first (a stable sort by the oracle's count): the first
    workgroup of k_rel_poses (256 iterations) then holds more poses than its LDS queue (512), the later ones fewer."""
    r = reference("rel")
    order = np.argsort(-r.counts.astype(np.int64), kind="stable")
    return Reference("rel", r.samples[order])


def workgroup_pose_totals(counts):
    return np.add.reduceat(counts.astype(np.int64), np.arange(0, len(counts), 256))


def essential_counts(ref, B=None):
    """real roots (essential matrices) per iteration of a 5-point reference"""
    B = ref.B if B is None else B
    return np.array([len(O.essential_5pt(ref.sample_in[i, :5], ref.sample_in[i, 5:])) for i in range(B)])


# ---- planted 5-point samples --------------------------------------------------------------------------------------------------------
# Samples of points("rel") whose determinant polynomial has 10 resp. 8 real roots, mined with the oracle: every sample of the
# sampler streams of seeds 100 .. 179 (2500 each, 200 000 samples) was solved; 31 had 10 real roots, 495 had 8.
TEN_ROOT_SAMPLES = [[91, 95, 30, 213, 147], [179, 115, 158, 207, 208], [268, 253, 145, 108, 219], [21, 147, 226, 80, 251],
                    [93, 299, 180, 129, 39], [53, 98, 179, 18, 196], [168, 243, 298, 13, 73], [277, 286, 95, 296, 125],
                    [62, 214, 162, 264, 115], [136, 112, 14, 114, 100], [176, 230, 22, 268, 112], [196, 244, 251, 11, 106]]
EIGHT_ROOT_SAMPLES = [[195, 178, 154, 214, 175], [283, 220, 196, 145, 193], [247, 49, 198, 38, 51], [267, 244, 155, 87, 9],
                      [203, 229, 33, 221, 92], [49, 234, 177, 100, 287], [22, 17, 58, 268, 258], [255, 170, 299, 100, 8]]


@functools.lru_cache(maxsize=None)
def many_roots():
    """the planted samples, each several times over and interleaved with ordinary ones (70 iterations: two wavefronts)"""
    plain = reference("rel").samples[:20].astype(np.int64).tolist()
    rows = []
    for i in range(25):
        rows.append(TEN_ROOT_SAMPLES[i % len(TEN_ROOT_SAMPLES)])
        rows.append(EIGHT_ROOT_SAMPLES[i % len(EIGHT_ROOT_SAMPLES)])
        if i < 20:
            rows.append(plain[i])
    return Reference("rel", np.array(rows, dtype=np.uint64))


def _project(X):
    return X[:, :2] / X[:, 2:3]


def _hard_scene(n, seed, planar=False, rotation_only=False):
    rs = np.random.RandomState(seed)
    X = np.c_[rs.uniform(-1.5, 1.5, (n, 2)), rs.uniform(4.0, 8.0, n)]
    if planar:
        X[:, 2] = 6.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    R = synth.quat_to_rotmat(np.array([0.98, 0.05, -0.12, 0.08]) / np.linalg.norm([0.98, 0.05, -0.12, 0.08]))
    t = np.zeros(3) if rotation_only else np.array([0.6, -0.1, 0.2])
    return np.ascontiguousarray(_project(X)), np.ascontiguousarray(_project(X @ R.T + t))


@functools.lru_cache(maxsize=None)
def hard_points(name):
    """small hand-built two-view point sets (exact projections, no noise) and the 5-point samples taken from them"""
    rs = np.random.RandomState(5)
    if name == "rotation":  # no translation: every essential matrix with that rotation fits
        a, b = _hard_scene(12, 1, rotation_only=True)
    elif name == "planar":  # all points on one plane
        a, b = _hard_scene(12, 2, planar=True)
    else:
        a, b = _hard_scene(12, 3)
    special = None
    if name == "coincident":  # correspondences 0 and 1 are the same point, sampled together
        a[1], b[1] = a[0], b[0]
        special = [0, 1]
    elif name == "nan":
        a[0, 1] = np.nan
        special = [0]
    elif name == "inf":
        b[0, 0] = np.inf
        special = [0]
    rows = []
    for _ in range(70):  # (two wavefronts)
        if special is None:
            rows.append(rs.permutation(12)[:5])
        else:
            rest = [i for i in rs.permutation(12) if i not in special][: 5 - len(special)]
            rows.append(rs.permutation(np.r_[special, rest].astype(np.int64)))
    return a, b, np.array(rows, dtype=np.uint64)


HARD_SETS = ["rotation", "planar", "coincident", "nan", "inf"]


class HardReference(Reference):
    def __init__(self, name):
        self.name = name
        self.kind = 1
        self.a, self.b, self.samples = hard_points(name)
        self.positions = None
        self.real_focal_check = False
        self.counts, self.models, self.sample_in = O.generate_models(1, self.a, self.b, self.samples)
        slot = np.arange(self.models.shape[1])[None, :] < self.counts[:, None]
        self.nan = np.isnan(self.models).any(axis=2) & slot


@functools.lru_cache(maxsize=None)
def hard_reference(name):
    return HardReference(name)
