"""The streaming scorers hypothesis by hypothesis (-m gpu): k_score_queue, k_score_mfma, k_score_mfma2, k_score_mfmah, their group
forms and k_finalize2(_g), through pl_debug_score_stream_ex - single launch and group form, with the grid in the test's hand.

Every hypothesis's count must equal the oracle's and its score agree to 1e-9 (tree-order sums), at list lengths that reach the
second and third ticket round and both thresholds of the tail rule of unit_of_ticket, at point counts on the edges of the chunk
shapes (tests/score_cases.py derives them from pl_debug_score_shape), and at grids whose workgroup count falls in every class of
slice_chunk_of_workgroup's numbering.  tests/test_score_cases.py checks on the CPU that a partial nobody wrote cannot hide: every
16 consecutive models hold one with inliers in every chunk."""
import numpy as np
import pytest

import score_cases as SC
from score_cases import GROUP, MFMA, QUEUE, SINGLE
from test_gpu_live_hypotheses import _nan_model

pytestmark = pytest.mark.gpu

REL = 1e-9  # scores: the bound of the existing streaming-scorer tests for sums in tree order
_problems = {}


def _problem(gpu, kind, N):
    if (kind, N) not in _problems:
        _problems[kind, N] = gpu.Problem(kind, *SC.scene(kind).points(N))
    return _problems[kind, N]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for p in _problems.values():
        p.close()
    _problems.clear()


def _compare(what, cnt, sc, ref_cnt, ref_sc, path, want_path):
    """what: (kind, route, N, slices, H)"""
    tag = "kind %d route %d N %d slices %s H %d" % what
    assert path == want_path, f"{tag}: path {path}, the case names {want_path}"
    bad = np.flatnonzero(np.asarray(cnt, np.int64) != ref_cnt)
    if len(bad):
        k = int(bad[0])
        raise AssertionError(f"{tag}: {len(bad)} counts differ, first at hypothesis {k}: {int(cnt[k])}, oracle {int(ref_cnt[k])}")
    err = np.abs(sc - ref_sc)
    bad = np.flatnonzero(~(err <= REL * np.abs(ref_sc)))
    if len(bad):
        k = int(bad[0])
        raise AssertionError(f"{tag}: {len(bad)} scores differ, first at hypothesis {k}: {sc[k]!r}, oracle {ref_sc[k]!r}")
    return float((err / np.abs(ref_sc)).max())


def _single(gpu, kind, path, N, s, H, models=None):
    sc = SC.scene(kind)
    cnt, score, got_path = _problem(gpu, kind, N).score_stream(sc.models[:H] if models is None else models, sc.thr, slices=s)
    return cnt, score, got_path


def _check_single(gpu, kind, path, N, s, H):
    cnt, score, got_path = _single(gpu, kind, path, N, s, H)
    ref_cnt, ref_sc = SC.scene(kind).reference(N, H)
    return _compare((kind, SINGLE, N, s, H), cnt, score, ref_cnt, ref_sc, got_path, path)


PATHS = [(k, p) for k in SC.KINDS for p in (QUEUE, MFMA)]


# ---- single route -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,path", PATHS)
def test_list_lengths_through_the_ticket_rounds_and_the_tail_rule(gpu, kind, path):
    """the full length sets at 1 and 3 slices, the one-round subsets at 2 and 5, on an exact fill and a ragged point count"""
    worst, runs = 0.0, 0
    for N in SC.fill_pair(kind, path):
        for s, lengths in SC.LENGTHS.items():
            for H in lengths:
                worst = max(worst, _check_single(gpu, kind, path, N, s, H))
                runs += 1
    print("kind", kind, "path", path, "N", SC.fill_pair(kind, path), "launches", runs, "largest relative score difference", worst)


@pytest.mark.parametrize("kind,path", PATHS)
def test_point_counts_at_the_edges_of_the_chunk_shapes(gpu, kind, path):
    worst = 0.0
    for N in SC.point_counts(kind, path, SINGLE):
        worst = max(worst, _check_single(gpu, kind, path, N, SC.SWEEP_SLICES, SC.H_SWEEP))
    print("kind", kind, "path", path, "N", SC.point_counts(kind, path, SINGLE), "largest relative score difference", worst)


@pytest.mark.parametrize("kind", SC.KINDS)
def test_every_class_of_the_workgroup_numbering(gpu, kind):
    """slice_chunk_of_workgroup deals T = slices x chunks pairs to 8 XCDs: T < 8, and T mod 8 = 0, 1, 7 beyond"""
    pairs = SC.workgroup_pairs(kind)
    assert len(pairs) == 4
    for _, N, s in pairs:
        _check_single(gpu, kind, MFMA, N, s, SC.H_SWEEP)


def test_nan_models_between_the_others(gpu):
    """absolute pose on the matrix cores: every 8th model holds a NaN (never a good one).  Those have no inliers - count 0 and the
    score N thr^2 exactly -, the others score as without them: the live list packs them, the partials are indexed by live position."""
    sc = SC.scene(0)
    N = SC.fill_pair(0, MFMA)[0]
    nan = np.arange(SC.BASE) % 8 == 3
    models = sc.models.copy()
    for k in np.flatnonzero(nan):
        models[k] = _nan_model(models[k], k // 8)
    ref_cnt, ref_sc = sc.reference(N, SC.BASE)
    ref_cnt, ref_sc = np.where(nan, 0, ref_cnt), np.where(nan, N * sc.thr ** 2, ref_sc)
    for s in (1, 3):
        for H in SC.LENGTHS[s]:
            cnt, score, path = _single(gpu, 0, MFMA, N, s, H, models[:H])
            _compare((0, SINGLE, N, s, H), cnt, score, ref_cnt[:H], ref_sc[:H], path, MFMA)
            assert (score[nan[:H]] == N * sc.thr ** 2).all(), (N, s, H)


# ---- group route --------------------------------------------------------------------------------------------------------------------
def _check_group(gpu, kind, members):
    """members: (N, H, slices, path)"""
    sc = SC.scene(kind)
    out, idle = gpu.score_stream_group([(_problem(gpu, kind, N), sc.models[:H], sc.thr, s) for N, H, s, _ in members])
    assert idle == 0, f"kind {kind} members {members}: the launch changed {idle} words of the inactive slot's buffers"
    for (N, H, s, path), got in zip(members, out):
        assert s == 0 or got["slices"] == s
        ref_cnt, ref_sc = sc.reference(N, H)
        _compare((kind, GROUP, N, s if s else "0 -> %d" % got["slices"], H), got["counts"], got["scores"], ref_cnt, ref_sc, got["path"], path)
    return out


@pytest.mark.parametrize("kind", SC.KINDS)
def test_group_launches_of_mixed_members(gpu, kind):
    """Launch 1: a matrix-core member with the longest list (1 slice), a queue member (3 slices), a matrix-core member of another
    chunk count with a third of the list (the group's own rule) - at lengths around the ends of the members' ticket rounds, every
    point count of the group shapes taking its turn.  Launch 2: one member alone."""
    gm, gq = SC.point_counts(kind, MFMA, GROUP), SC.point_counts(kind, QUEUE, GROUP)
    scan = SC.shape_scan(kind, MFMA, GROUP)
    long_lists = SC.round_straddles(1) + [SC.BASE]
    short_lists = SC.round_straddles(3)
    assert len(long_lists) >= max(len(gm), len(gq))
    for j, H in enumerate(long_lists):
        A = gm[j % len(gm)]
        C = next(n for n in gm[(j + 1) % len(gm):] + gm if scan[n][0] != scan[A][0])
        B = gq[j % len(gq)]
        out = _check_group(gpu, kind, [(A, H, 1, MFMA), (B, short_lists[j % len(short_lists)], 3, QUEUE), (C, max(1, H // 3), 0, MFMA)])
        assert out[0]["chunks"] == scan[A][0] and out[2]["chunks"] == scan[C][0]
    for H in (SC.H_SWEEP, SC.BASE):
        _check_group(gpu, kind, [(gm[-1], H, 0, MFMA)])
    _check_group(gpu, kind, [(SC.N_GROUP_QUEUE, SC.H_SWEEP, 0, QUEUE)])


# ---- independence from the cut --------------------------------------------------------------------------------------------------------
CUTS = (1, 2, 3, 5, 0)
H_CUT = 64 * (16 + 7) - 33  # two rounds of one workgroup, one of two, the tail of three and of five


def _unit_of(H, slices, min_sub):
    """(start, length) of the unit that holds hypothesis k = 0 .. H - 1 when `slices` workgroups share a chunk: units of 64 while
    whole rounds of 8 slices wavefronts remain, then sub-units of 16 (where the kernel cuts that fine), 32 or 64"""
    w = 8 * slices
    G = -(-H // 64)
    full = G // w * w
    rest = G - full
    sub = 16 if (min_sub <= 16 and rest * 4 <= w) else 32 if rest * 2 <= w else 64
    k = np.arange(H)
    start = np.where(k < 64 * full, k // 64 * 64, 64 * full + (k - 64 * full) // sub * sub)
    return start, np.minimum(np.where(k < 64 * full, 64, sub), H - start)


def _check_cuts(what, N, min_sub, runs):
    """runs: (slices, counts, scores) of one list on one problem.  Counts: the same whatever the cut.  Scores: the same bits
    wherever the hypothesis sits in the same unit under both cuts; elsewhere they agree to N 2^-52 - a hypothesis's at most N
    non-negative terms reach its sum in the drain batches of its wavefront's queue, and where a batch ends depends on the pairs the
    unit's other hypotheses queued before: two orders of one sum of N non-negative terms, each within (N - 1) 2^-53 of it."""
    s0, cnt0, sc0 = runs[0]
    u0 = _unit_of(len(sc0), s0, min_sub)
    for s, cnt, score in runs[1:]:
        assert (cnt == cnt0).all(), what + (N, s)
        u = _unit_of(len(score), s, min_sub)
        same_unit = (u[0] == u0[0]) & (u[1] == u0[1])
        diff = score != sc0
        print(*what, "N", N, "slices", s, "against", s0, ": hypotheses in another unit", int((~same_unit).sum()), "scores with other bits",
              int(diff.sum()), "largest relative difference", float((np.abs(score - sc0) / sc0).max()))
        assert not (diff & same_unit).any(), what + (N, s, int(np.flatnonzero(diff & same_unit)[0]))
        assert (np.abs(score - sc0) <= N * 2.0 ** -52 * sc0).all(), what + (N, s)


@pytest.mark.parametrize("kind", SC.KINDS)
def test_what_depends_on_the_slice_count(gpu, kind):
    """Within a route and a point count no count depends on the number of slices, and no score beyond the order of its sum: the
    bits are those of the hypothesis's unit (driver_group.inc, group_score_slices)."""
    sc = SC.scene(kind)
    for path in (QUEUE, MFMA):
        min_sub = 32 if (kind == 0 and path == MFMA) else 16  # (k_score_mfma cuts no finer than 32: unit_of_ticket<32>)
        N = SC.fill_pair(kind, path)[1]
        runs = [(s,) + _single(gpu, kind, path, N, s, H_CUT)[:2] for s in CUTS if s]
        _check_cuts(("kind", kind, "single, path", path), N, min_sub, runs)
        cnt, score, _ = _single(gpu, kind, path, N, 0, H_CUT)  # (the entry's own rule: as many slices as the launch takes)
        assert (cnt == runs[0][1]).all() and (np.abs(score - runs[0][2]) <= N * 2.0 ** -52 * runs[0][2]).all()
        Ng = SC.fill_pair(kind, path, GROUP)[1] if path == MFMA else SC.N_GROUP_QUEUE
        runs = []
        for s in CUTS:
            got = gpu.score_stream_group([(_problem(gpu, kind, Ng), sc.models[:H_CUT], sc.thr, s)])[0][0]
            runs.append((got["slices"], got["counts"], got["scores"]))
        _check_cuts(("kind", kind, "group, path", path), Ng, min_sub, runs)


# ---- tangent Sampson and 1D radial ------------------------------------------------------------------------------------------------------
def _small_kind(gpu, which):
    from poselib_amd import _lib

    if which == 4:
        import test_gpu_tangent_sampson as T

        n = 2 * int(_lib.lib().pl_debug_tangent_chunk()) + 1
        d, x1s, x2s, c1s, c2s, thr = T.stream_inputs(n)
        return gpu.TangentProblem(x1s, x2s, c1s, c2s), d, thr, T, n
    import test_gpu_radial1d as T

    n = 2 * int(_lib.lib().pl_debug_radial1d_chunk()) + 1
    d, x, thr = T.stream_inputs(n)
    return gpu.Problem(gpu.KIND_RAD1D, x, d["p3d"]), d, thr, T, n


@pytest.mark.parametrize("which", [4, 5])
def test_tangent_and_radial_scorers_through_the_ticket_rounds(gpu, which):
    """k_score_tangent / k_score_radial1d share unit_of_ticket: the length sets at 1 and 3 slices on two chunks and one correspondence,
    against the sequential scorer behind pl_score_model, hypothesis by hypothesis"""
    pr, d, thr, T, n = _small_kind(gpu, which)
    base = max(SC.LENGTHS[3])
    M = T.stream_models(d, base)
    ref = [pr.score(gpu.CameraPose(m[:4], m[4:]), thr) for m in M]
    ref_sc, ref_cnt = np.array([r[0] for r in ref]), np.array([r[1] for r in ref], np.int64)
    assert (ref_cnt > n // 3).sum() > base // 8, "the list holds too few models with inliers in both chunks"
    for s in (1, 3):
        for H in SC.LENGTHS[s]:
            cnt, score, path = pr.score_stream(M[:H], thr, slices=s)
            _compare((which, SINGLE, n, s, H), cnt, score, ref_cnt[:H], ref_sc[:H], path, QUEUE)
    pr.close()


# ---- rejections -----------------------------------------------------------------------------------------------------------------------
def test_new_entries_reject_what_they_cannot_take(gpu):
    sc0, sc3 = SC.scene(0), SC.scene(3)
    p0, p3 = _problem(gpu, 0, 1024), _problem(gpu, 3, 1024)
    M0, M3 = sc0.models[:40], sc3.models[:40]
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):  # 4 chunks on the matrix cores: at most 128 slices
        p0.score_stream(M0, sc0.thr, slices=129)
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.score_stream_group([(p0, M0, sc0.thr, 1536 // 4 + 1)])
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.score_stream_group([(p0, M0, sc0.thr, 1), (p3, M3, sc3.thr, 1)])
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.score_stream_group([(p0, M0, sc0.thr, 1)] * 5)
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.score_stream_group([])
    for which in (4, 5):
        pr, d, thr, T, n = _small_kind(gpu, which)
        M = T.stream_models(d, 40)
        with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
            gpu.score_stream_group([(pr, M, thr, 1)])
        with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
            pr.score_stream(M, thr, slices=1536 // 3 + 1)
        cnt, _, _ = pr.score_stream(M, thr, slices=1536 // 3)  # (three chunks: the limit itself is taken)
        assert (cnt == pr.score_stream(M, thr)[0]).all()
        pr.close()
    out, idle = gpu.score_stream_group([(p0, M0, sc0.thr, 1)] * 4)  # four members are taken
    assert idle == 0 and all((o["counts"] == out[0]["counts"]).all() for o in out)
