"""The cases of the streaming-scorer tests (tests/score_cases.py) on the CPU: the point counts cover the shapes pl_debug_score_shape
reports, the base lists and scenes satisfy the coverage conditions that turn a dropped (sub-unit, chunk) partial into a count
mismatch, and a numpy restatement of the four errors agrees with the oracle on every (model, correspondence) pair.  No device."""
import numpy as np
import pytest

import score_cases as SC
from score_cases import GROUP, MFMA, QUEUE, SINGLE

COMBOS = [(k, p, r) for k in SC.KINDS for p in (QUEUE, MFMA) for r in (SINGLE, GROUP)]


@pytest.mark.parametrize("kind,path,route", COMBOS)
def test_point_counts_cover_every_shape_of_the_scan(kind, path, route):
    scan = SC.shape_scan(kind, path, route)
    ns = SC.point_counts(kind, path, route)
    assert ns and all(n in scan for n in ns)
    assert {scan[n][1] for n in ns} == {p for _, p in scan.values()}, "a points-per-lane value of the scan has no case"
    for n, (chunks, per_lane) in scan.items():  # the entry's own consistency: the chunks hold N and no chunk is empty
        assert (chunks - 1) * 64 * per_lane < n <= chunks * 64 * per_lane, (n, chunks, per_lane)
    if path == MFMA:
        assert min(ns) == 1024 and 1023 in SC.point_counts(kind, QUEUE, route)
    exact = [n for n in ns if n == scan[n][0] * 64 * scan[n][1]]
    assert exact and any(n % 32 == 31 for n in ns)
    # (the single launch balances its chunks: one correspondence is alone in the last one only at the largest points per lane)
    one = [n for n in scan if scan[n][0] >= 2 and n == (scan[n][0] - 1) * 64 * scan[n][1] + 1]
    assert (one or route == SINGLE) and (not one or set(one) & set(ns)), "no one-column last chunk"
    if route == GROUP and path == QUEUE:
        assert SC.N_GROUP_QUEUE in ns


def test_list_lengths():
    for s, lengths in SC.LENGTHS.items():
        w = 8 * s
        assert {1, 31, 32, 33} <= set(lengths) and max(lengths) <= SC.BASE
        assert 64 * w in lengths and 64 * w - 1 in lengths  # the end of the first ticket round
        for rest in (w // 4, w // 4 + 1, w // 2, w // 2 + 1, w - 1):  # both sides of the tail rule's two thresholds
            assert 64 * (w + rest) in lengths and 64 * (w + rest) - 49 in lengths
    assert 64 * (2 * 8 + 7) in SC.LENGTHS[1] and 64 * 7 - 33 in SC.LENGTHS[3]
    assert SC.BASE == 64 * (40 + 39)


@pytest.mark.parametrize("kind", SC.KINDS)
def test_workgroup_numbering_classes(kind):
    scan = SC.shape_scan(kind, MFMA, SINGLE)
    got = {name: s * scan[n][0] for name, n, s in SC.workgroup_pairs(kind)}
    assert set(got) == {"T<8", "0", "1", "7"}, got
    assert got["T<8"] < 8 and all(got[r] > 8 and got[r] % 8 == int(r) for r in ("0", "1", "7"))


@pytest.mark.parametrize("kind", SC.KINDS)
def test_coverage_conditions(kind):
    """On the reference alone: a good model in every run of 16, at least 5 of its inliers in every chunk of every case (1 in a last
    chunk of fewer than 32 correspondences - its last correspondence, an inlier of every good model)."""
    sc = SC.scene(kind)
    for k0 in range(0, SC.BASE - 15):
        assert any(SC.is_good(k) for k in range(k0, k0 + 16))
    good = sc.mask[::SC.GOOD_EVERY]
    assert len(good) == SC.BASE // SC.GOOD_EVERY and all(SC.is_good(k) for k in range(0, SC.BASE, SC.GOOD_EVERY))
    for path in (QUEUE, MFMA):
        for route in (SINGLE, GROUP):
            scan = SC.shape_scan(kind, path, route)
            for N in SC.point_counts(kind, path, route):
                chunks, per_lane = scan[N]
                per = SC.chunk_inliers(kind, N, 64 * per_lane)
                assert per.shape == (len(good), chunks)
                last = N - (chunks - 1) * 64 * per_lane
                assert per[:, :-1].min(initial=5) >= 5, (kind, path, route, N, int(per[:, :-1].min()))
                assert per[:, -1].min() >= (5 if last >= 32 else 1), (kind, path, route, N, last, int(per[:, -1].min()))
                assert good[:, N - 1].all(), (kind, N)
    # the oracle's two entries agree: the counts of its score are the sums of its inlier flags
    N = SC.point_counts(kind, MFMA, SINGLE)[-1]
    cnt, _ = sc.reference(N, 200)
    assert (cnt == sc.mask[:200, :N].sum(axis=1)).all()


# ---- the independent anchor -----------------------------------------------------------------------------------------------------------
def _rotmat(q):
    w, x, y, z = q
    return [[1 - (2 * y * y + 2 * z * z), 2 * y * x - 2 * z * w, 2 * z * x + 2 * y * w],
            [2 * y * x + 2 * z * w, 1 - (2 * x * x + 2 * z * z), 2 * z * y - 2 * x * w],
            [2 * z * x - 2 * y * w, 2 * z * y + 2 * x * w, 1 - (2 * x * x + 2 * y * y)]]


def _quat_rotate(q, p):
    q1, q2, q3, q4 = q
    a = -p[0] * q2 - p[1] * q3 - p[2] * q4
    b = p[0] * q1 - p[1] * q4 + p[2] * q3
    c = p[1] * q1 + p[0] * q4 - p[2] * q2
    d = p[1] * q2 - p[0] * q3 + p[2] * q1
    return [b * q1 - a * q2 - c * q4 + d * q3, c * q1 - a * q3 + b * q4 - d * q2, c * q2 - b * q3 - a * q4 + d * q1]


def _sampson(E, x1, x2):
    Ea = [E[i][0] * x1[0] + E[i][1] * x1[1] + E[i][2] for i in range(3)]
    Eb = [E[0][j] * x2[0] + E[1][j] * x2[1] + E[2][j] for j in range(2)]
    C = x2[0] * Ea[0] + x2[1] * Ea[1] + Ea[2]
    return C * C / (Ea[0] * Ea[0] + Ea[1] * Ea[1] + Eb[0] * Eb[0] + Eb[1] * Eb[1])


def squared_error(kind, M, a, b):
    """(squared error, gate) of model components M against point components a, b - arrays that broadcast against each other, in
    whatever precision they come.  reprojection with positive depth (0), Sampson with cheirality (1), Sampson (2), transfer (3)."""
    if kind == 0:
        R, t = _rotmat(M[:4]), M[4:7]
        Z = [R[i][0] * b[0] + R[i][1] * b[1] + R[i][2] * b[2] + t[i] for i in range(3)]
        e0, e1 = Z[0] / Z[2] - a[0], Z[1] / Z[2] - a[1]
        return e0 * e0 + e1 * e1, Z[2] > 0
    if kind == 1:
        R, t = _rotmat(M[:4]), M[4:7]
        z = np.zeros_like(t[0])
        Tx = [[z, -t[2], t[1]], [t[2], z, -t[0]], [-t[1], t[0], z]]
        E = [[sum(Tx[i][k] * R[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        r2 = _sampson(E, a, b)
        n1, n2 = np.sqrt(a[0] * a[0] + a[1] * a[1] + 1), np.sqrt(b[0] * b[0] + b[1] * b[1] + 1)
        u1, u2 = [a[0] / n1, a[1] / n1, 1 / n1], [b[0] / n2, b[1] / n2, 1 / n2]
        Rx1 = _quat_rotate(M[:4], u1)
        al = -sum(Rx1[i] * u2[i] for i in range(3))
        b1 = -sum(Rx1[i] * t[i] for i in range(3))
        b2 = sum(u2[i] * t[i] for i in range(3))
        md = 0.01 * (1 - al * al)
        return r2, (b1 - al * b2 > md) & (-al * b1 + b2 > md)
    Mm = [[M[3 * i + j] for j in range(3)] for i in range(3)]
    if kind == 2:
        r2 = _sampson(Mm, a, b)
        return r2, r2 == r2
    h = [Mm[i][0] * a[0] + Mm[i][1] * a[1] + Mm[i][2] for i in range(3)]
    inv = 1 / h[2]
    e0, e1 = h[0] * inv - b[0], h[1] * inv - b[1]
    return e0 * e0 + e1 * e1, inv == inv


def _components(x, dtype, shape):
    return [np.asarray(x[..., i], dtype=dtype).reshape(shape) for i in range(x.shape[-1])]


@pytest.mark.parametrize("kind", SC.KINDS)
def test_longdouble_restatement_reproduces_the_oracle(kind):
    """Every (base model, correspondence) pair of the scene.  fp64 decides the pairs whose squared error is farther than 1e-6
    (relative) from thr^2 - its own rounding moves a squared error by parts in 1e-13 of thr^2 at most there -, numpy longdouble
    decides the rest; pairs within 1e-12 of thr^2 are set aside, and exist only where they were planted."""
    sc = SC.scene(kind)
    thr2 = sc.thr ** 2
    models = sc.models.reshape(SC.BASE, -1)
    n = len(sc.a)
    inl = np.zeros((SC.BASE, n), bool)
    near = np.zeros((SC.BASE, n), bool)
    with np.errstate(all="ignore"):
        for k0 in range(0, SC.BASE, 512):
            blk = models[k0:k0 + 512]
            r2, gate = squared_error(kind, _components(blk, np.float64, (-1, 1)), _components(sc.a, np.float64, (1, -1)),
                                     _components(sc.b, np.float64, (1, -1)))
            inl[k0:k0 + 512] = (r2 < thr2) & gate
            near[k0:k0 + 512] = np.abs(r2 - thr2) <= 1e-6 * thr2
        km, ki = np.nonzero(near)
        r2, gate = squared_error(kind, _components(models[km], np.longdouble, (-1,)), _components(sc.a[ki], np.longdouble, (-1,)),
                                 _components(sc.b[ki], np.longdouble, (-1,)))
        inl[km, ki] = (r2 < np.longdouble(thr2)) & gate
        tie = np.abs(r2 - np.longdouble(thr2)) <= np.longdouble(1e-12) * np.longdouble(thr2)
    print("kind", kind, "pairs", inl.size, "near the threshold", len(km), "ties", int(tie.sum()))
    assert sc.planted[ki[tie]].all(), "a tie at a correspondence nobody planted"
    decided = np.ones((SC.BASE, n), bool)
    decided[km[tie], ki[tie]] = False
    bad = np.argwhere((inl != sc.mask) & decided)
    assert len(bad) == 0, (kind, bad[:5])
    assert ((inl & decided).sum(axis=1) == (sc.mask & decided).sum(axis=1)).all()
    if kind == 0:
        assert len(km) > 1000, "the planted correspondences are not at the boundary"
