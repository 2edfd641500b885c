"""The kernels of the two focal-length estimators stage by stage against the oracle (-m gpu): focal.hip and sfocal.hip - setup, solve,
the wavefront and the workgroup scorer and the mask kernel of each, single and group form.

pl_debug_focal_stage (api.debug_focal_stage) runs ONE stage through the production launchers with the arguments wired as the
estimators' back ends wire them, and returns the whole output buffers, prefilled with a sentinel: what no lane wrote keeps it.  The
expected values are the oracle's (tests/focal_stage_cases.py; tests/test_focal_stage_cases.py proves on the CPU that the cases sit
where they are meant to, tests/test_focal_stage_oracle_vs_reference.py pins the oracle's side to the reference's sources).  Every
comparison is on bits, for every slot of every launch; a NaN must meet a NaN in the same place.  There are no tolerances: the scorers add
in correspondence order by construction."""
import numpy as np
import pytest

import focal_stage_cases as F

pytestmark = pytest.mark.gpu

UNWRITTEN, FILL = F.UNWRITTEN, F.FILL
FILL_BYTE = 0x5A


def bits_equal(got, want):
    """float64 arrays equal bit for bit, NaN against NaN whatever the payload"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


@pytest.fixture(scope="module")
def world(gpu):
    """resident problems, built on first use and shared by the tests of the module"""

    class World:
        def __init__(self):
            self.problems = {}

        def problem(self, which, n):
            return self.named((which, n), which, *F.points(which, n))

        def named(self, key, which, a, b):
            if key not in self.problems:
                self.problems[key] = gpu.Problem(F.KIND[which], a, b)
            return self.problems[key]

    w = World()
    yield w
    for p in w.problems.values():
        p.close()


# ---------------------------------------------------------------------------------------------------------------- expectations
def want_generated(g, B, capacity):
    """the buffers a generator launch over the first B samples of g must leave: the oracle's models in front, the prefill behind"""
    maxm = F.MAX_MODELS[g.which]
    models = np.full((capacity, maxm, 8), FILL)
    slot = np.arange(maxm)[None, :] < g.counts[:B, None]
    models[:B][slot] = g.models[:B][slot]
    num = np.full(capacity, UNWRITTEN, dtype=np.uint32)
    num[:B] = g.counts[:B]
    return models, num


def check_generated(out, g, B, tag):
    capacity = len(out["num_models"])
    models, num = want_generated(g, B, capacity)
    assert np.array_equal(out["num_models"], num), (tag, np.flatnonzero(out["num_models"] != num)[:8])
    assert bits_equal(out["models"], models), (tag, [i for i in range(capacity) if not bits_equal(out["models"][i], models[i])][:8])
    # the pinned mirrors hold what the device buffers hold
    assert np.array_equal(out["host_num_models"], out["num_models"]) and bits_equal(out["host_models"], out["models"]), tag


def want_scores(which, n, idx, capacity, empty=None):
    """counts and sums of a score launch whose slot s holds model idx[s] of the list (-1: an empty slot, which reads `empty`)"""
    ec, ev = F.expected_scores(which, n)
    counts = np.full(capacity, UNWRITTEN, dtype=np.uint32)
    sums = np.full(capacity, FILL)
    filled = idx >= 0
    counts[: len(idx)][filled], sums[: len(idx)][filled] = ec[idx[filled]], ev[idx[filled]]
    if empty is not None:
        counts[: len(idx)][~filled], sums[: len(idx)][~filled] = empty
    return counts, sums


def check_scores(out, want, tag):
    counts, sums = want
    assert np.array_equal(out["counts"], counts), (tag, np.flatnonzero(out["counts"] != counts)[:8])
    assert bits_equal(out["sums"], sums), (tag, np.flatnonzero(out["sums"].view(np.uint64) != sums.view(np.uint64))[:8])


def check_mask(out, mask, n, tag):
    want = np.full(len(out["mask"]), FILL_BYTE, dtype=np.uint8)
    want[:n] = mask
    assert np.array_equal(out["mask"], want), (tag, np.flatnonzero(out["mask"] != want)[:8])
    assert np.array_equal(out["host_mask"], want), (tag, np.flatnonzero(out["host_mask"] != want)[:8])


# ---------------------------------------------------------------------------------------------------------------- 1. generate
@pytest.mark.parametrize("B", F.GEN_BS)
@pytest.mark.parametrize("which", F.WHICH)
def test_generate_equals_the_oracle(gpu, world, which, B):
    """k_*_setup + k_*_solve: models, focal lengths, their order and the counts of every iteration; explicit samples and the device's
    own draws from the oracle's positions agree; rebased positions give the tail of the run; the mirrors equal the device buffers;
    slots beyond an iteration's count and iterations beyond the launch keep the prefill"""
    for n in F.GEN_NS[which]:
        g = F.generated(which, n)
        prob = world.problem(which, n)
        given = gpu.debug_focal_stage("generate", {"problem": prob, "samples": g.samples[:B], "capacity": B + 3})
        check_generated(given, g, B, (n, "samples"))
        drawn = gpu.debug_focal_stage("generate", {"problem": prob, "seed": F.SEED, "positions": g.positions[:B], "capacity": B + 3})
        check_generated(drawn, g, B, (n, "positions"))
        if B > F.REBASE:
            base = int(g.positions[F.REBASE])
            tail = gpu.debug_focal_stage("generate", {"problem": prob, "seed": F.SEED, "pos_base": base,
                                                      "positions": g.positions[F.REBASE:B] - g.positions[F.REBASE]})
            assert np.array_equal(tail["num_models"], drawn["num_models"][F.REBASE:B]), n
            assert bits_equal(tail["models"], drawn["models"][F.REBASE:B]), n


# ---------------------------------------------------------------------------------------------------------------- 2. the filter
@pytest.mark.parametrize("bound", list(F.max_focals()))
def test_focal_length_filter_of_the_solve_kernel(gpu, world, bound):
    """keep_all == 0 with max_focal: the solutions the estimator keeps, compacted in the order of the eigenvalues - the oracle's, and
    the keep_all solver output (pl_solve_focal_batch) after the estimator's rule is applied here"""
    max_focal = F.max_focals()[bound]
    g = F.generated(0, F.FILTER_N, max_focal)
    out = gpu.debug_focal_stage("generate", {"problem": world.problem(0, F.FILTER_N), "samples": g.samples, "max_focal": max_focal})
    check_generated(out, g, F.GEN_B, bound)
    solved, counts = gpu.solve_focal_batch("p35pf", F.solver_inputs(F.FILTER_N))
    for i in range(F.GEN_B):
        want = F.apply_filter(solved[i, : counts[i], :7], solved[i, : counts[i], 7], max_focal)
        assert out["num_models"][i] == len(want) and bits_equal(out["models"][i, : len(want)], want), (bound, i)


# ---------------------------------------------------------------------------------------------------------------- 3. score
@pytest.mark.parametrize("n", F.NS)
@pytest.mark.parametrize("which", F.WHICH)
def test_score_equals_the_oracle(gpu, world, which, n):
    """count and inlier sum (pnpf) / MSAC score (shared focal) of every model of the list at every size, through the workgroup kernel
    (up to 1024 slots) and the wavefront kernel (above); the same list as 1024 and as 1025 slots gives the same values per model; the
    models taken out of LM task records give what the models themselves give"""
    prob = world.problem(which, n)
    thr2 = F.THR2[which]
    runs = {}
    for slots in F.SLOT_COUNTS + (len(F.models(which)[1]),):
        models, idx = F.padded(which, slots)
        out = gpu.debug_focal_stage("score", {"problem": prob, "models": models, "thr2": thr2, "capacity": slots + 2})
        check_scores(out, want_scores(which, n, idx, slots + 2), (slots, "models"))
        runs[slots] = out
    assert np.array_equal(runs[F.SWITCH]["counts"][: F.SWITCH], runs[F.SWITCH + 1]["counts"][: F.SWITCH])
    assert bits_equal(runs[F.SWITCH]["sums"][: F.SWITCH], runs[F.SWITCH + 1]["sums"][: F.SWITCH])
    for slots in (len(F.models(which)[1]), F.SWITCH + 1):
        models, idx = F.padded(which, slots)
        out = gpu.debug_focal_stage("score", {"problem": prob, "models": models, "thr2": thr2, "as_tasks": True, "capacity": slots + 2})
        check_scores(out, want_scores(which, n, idx, slots + 2), (slots, "tasks"))
        assert np.array_equal(out["counts"], runs[slots]["counts"]) and bits_equal(out["sums"], runs[slots]["sums"])


@pytest.mark.parametrize("which", F.WHICH)
def test_score_and_mask_on_inlier_patterns(gpu, world, which):
    """inliers exactly at {0}, {n - 1}, {63, 64}, {191, 192}, everywhere from 192 on, everywhere and nowhere: both scorers and the
    mask kernel"""
    thr2 = F.THR2[which]
    for p in F.patterns(which):
        prob = world.named((which, p.name, p.n), which, p.a, p.b)
        sc = F.score_of(which, p.model, p.a, p.b, thr2)
        for slots in (1, F.SWITCH + 1):
            out = gpu.debug_focal_stage("score", {"problem": prob, "models": np.tile(p.model, (slots, 1)), "thr2": thr2})
            assert (out["counts"] == sc.count).all() and sc.count == len(p.inliers), (p.name, p.n, slots, out["counts"][:4], sc.count)
            assert bits_equal(out["sums"], np.full(slots, sc.value)), (p.name, p.n, slots)
        mask = np.zeros(p.n, dtype=np.uint8)
        mask[p.inliers] = 1
        check_mask(gpu.debug_focal_stage("mask", {"problem": prob, "model": p.model, "thr2": thr2, "capacity": p.n + 5}), mask, p.n,
                   (p.name, p.n))


# ---------------------------------------------------------------------------------------------------------------- 4. the gate
@pytest.mark.parametrize("n", F.GATE_NS)
@pytest.mark.parametrize("side", (0, 1))
@pytest.mark.parametrize("which", F.WHICH)
def test_num_models_gate(gpu, world, which, side, n):
    """slots beyond an iteration's count: both pnpf scorers write count 0 and sum 0.0 (the host copies the whole block), both
    shared-focal scorers write nothing (the host reads the filled slots only); filled slots as in test 3.  side 0: at most 1024 slots,
    the workgroup kernel; side 1: above, the wavefront kernel (shared focal: one workgroup per iteration)"""
    B = F.GATED_BS[which][side]
    models, num, idx = F.gated(which, B)
    assert (len(idx) <= F.SWITCH) == (side == 0)
    out = gpu.debug_focal_stage("score", {"problem": world.problem(which, n), "models": models, "num_models": num, "thr2": F.THR2[which],
                                          "capacity": len(idx) + 2})
    check_scores(out, want_scores(which, n, idx, len(idx) + 2, (0, 0.0) if which == 0 else (UNWRITTEN, FILL)), (B, n))


# ---------------------------------------------------------------------------------------------------------------- 5. mask
@pytest.mark.parametrize("n", F.NS)
@pytest.mark.parametrize("which", F.WHICH)
def test_mask_equals_the_oracle(gpu, world, which, n):
    """get_inliers of every model of the list at every size; the pinned mirror equals the device mask; bytes beyond n are untouched"""
    prob = world.problem(which, n)
    masks = F.expected_masks(which, n)
    for i, m in enumerate(F.models(which)[1]):
        out = gpu.debug_focal_stage("mask", {"problem": prob, "model": m, "thr2": F.THR2[which], "capacity": n + 5})
        check_mask(out, masks[i], n, (n, i))


# ---------------------------------------------------------------------------------------------------------------- 6. thresholds
@pytest.mark.parametrize("which", F.WHICH)
def test_a_threshold_on_a_residual(gpu, world, which):
    """thr2 equal to a point's residual leaves the point out (the comparison is strict), the next double takes it - the score with
    the score's residual, the mask with the mask's own, on the oracle's side of every such threshold"""
    prob = world.problem(which, F.TIE_N)
    a, b = F.points(which, F.TIE_N)
    for t in F.ties(which):
        sc = F.score_of(which, t.model, a, b, t.thr2)
        for slots in (1, F.SWITCH + 1):
            out = gpu.debug_focal_stage("score", {"problem": prob, "models": np.tile(t.model, (slots, 1)), "thr2": t.thr2})
            assert (out["counts"] == sc.count).all() and bits_equal(out["sums"], np.full(slots, sc.value)), (t, slots, out["counts"][:2])
        mask, _ = F.mask_of(which, t.model, a, b, t.thr2)
        if t.stage == "mask":
            assert bool(mask[t.k]) == t.inside
        check_mask(gpu.debug_focal_stage("mask", {"problem": prob, "model": t.model, "thr2": t.thr2}), mask, F.TIE_N, t)


def test_count_and_mask_disagree_where_the_reference_s_do(gpu, world):
    """pnpf: the score multiplies by the reciprocal of the depth, the mask divides by it.  With the threshold between a point's two
    residuals the count takes the point and the mask does not, or the other way round - each kernel on the oracle's side"""
    prob = world.problem(0, F.SPLIT_N)
    a, b = F.points(0, F.SPLIT_N)
    cases, _, _ = F.splits()
    assert sum(c.counted for c in cases) >= 8 and sum(c.masked for c in cases) >= 8
    for c in cases:
        sc = F.score_of(0, c.model, a, b, c.thr2)
        mask, _ = F.mask_of(0, c.model, a, b, c.thr2)
        assert (sc.r2[c.k] < c.thr2) == c.counted and bool(mask[c.k]) == c.masked and c.counted != c.masked
        for slots in (1, F.SWITCH + 1):
            out = gpu.debug_focal_stage("score", {"problem": prob, "models": np.tile(c.model, (slots, 1)), "thr2": c.thr2})
            assert (out["counts"] == sc.count).all() and bits_equal(out["sums"], np.full(slots, sc.value)), (c, slots, out["counts"][:2])
        check_mask(gpu.debug_focal_stage("mask", {"problem": prob, "model": c.model, "thr2": c.thr2}), mask, F.SPLIT_N, c)


# ---------------------------------------------------------------------------------------------------------------- 7. group forms
def untouched(out):
    """every buffer of a member still holds the prefill"""
    for key, v in out.items():
        if v.dtype == np.uint32:
            assert (v == UNWRITTEN).all(), key
        elif v.dtype == np.uint8:
            assert (v == FILL_BYTE).all(), key
        else:
            assert bits_equal(v, np.full(v.shape, FILL)), key


@pytest.mark.parametrize("which", F.WHICH)
def test_group_generate(gpu, world, which):
    """three members - full, short (another problem, fewer iterations, buffers of the full extent), idle: the grid is the full member's"""
    full, short = F.generated(which, 300), F.generated(which, F.GEN_NS[which][1])
    Bf, Bs = 65, 5
    members = [{"problem": world.problem(which, 300), "seed": F.SEED, "positions": full.positions[:Bf]},
               {"problem": world.problem(which, short.n), "samples": short.samples[:Bs], "capacity": Bf},
               {"problem": world.problem(which, 300), "idle": True, "capacity": Bf}]
    for order in ((0, 1, 2), (2, 1, 0)):
        outs = gpu.debug_focal_stage("generate", [members[k] for k in order], group=True)
        outs = [outs[order.index(k)] for k in range(3)]
        single = gpu.debug_focal_stage("generate", members[0])
        for key in single:
            assert bits_equal(outs[0][key], single[key]) if single[key].dtype == np.float64 else np.array_equal(outs[0][key], single[key]), key
        check_generated(outs[0], full, Bf, "full")
        check_generated(outs[1], short, Bs, "short")  # (the rest of its buffers keeps the prefill)
        untouched(outs[2])


@pytest.mark.parametrize("gate", (False, True))
@pytest.mark.parametrize("wg", (True, False))
@pytest.mark.parametrize("which", F.WHICH)
def test_group_score(gpu, world, which, wg, gate):
    """both group scorers (workgroup_per_model), with and without num_models; the full member equals the single launch bit for bit"""
    if which == 1 and not wg and not gate:
        with pytest.raises(gpu.PoseLibAmdError, match="error -3"):  # (the launcher's grid is one workgroup per iteration)
            gpu.debug_focal_stage("score", [{"problem": world.problem(1, 65), "models": F.padded(1, 4)[0], "thr2": F.THR2[1]}], group=True)
        return
    nf, ns = F.GROUP_NS
    thr2 = F.THR2[which]
    empty = (0, 0.0) if which == 0 else (UNWRITTEN, FILL)
    if gate:
        (mf, gf, idxf), (ms, gs, idxs) = F.gated(which, 13), F.gated(which, 3)
    else:
        (mf, idxf), (ms, idxs), gf, gs = F.padded(which, 70), F.padded(which, 9), None, None
    members = [{"problem": world.problem(which, nf), "models": mf, "num_models": gf, "thr2": thr2},
               {"problem": world.problem(which, ns), "models": ms, "num_models": gs, "thr2": thr2, "capacity": len(idxf)},
               {"problem": world.problem(which, nf), "idle": True, "capacity": len(idxf), "thr2": thr2}]
    for as_tasks in (False, True):
        for m in members[:2]:
            m["as_tasks"] = as_tasks
        for order in ((0, 1, 2), (2, 1, 0)):
            outs = gpu.debug_focal_stage("score", [members[k] for k in order], group=True, workgroup_per_model=wg)
            outs = [outs[order.index(k)] for k in range(3)]
            check_scores(outs[0], want_scores(which, nf, idxf, len(idxf), empty), ("full", as_tasks))
            check_scores(outs[1], want_scores(which, ns, idxs, len(idxf), empty), ("short", as_tasks))
            untouched(outs[2])
        single = gpu.debug_focal_stage("score", members[0])
        assert np.array_equal(outs[0]["counts"], single["counts"]) and bits_equal(outs[0]["sums"], single["sums"])


@pytest.mark.parametrize("which", F.WHICH)
def test_group_mask(gpu, world, which):
    nf, ns = F.GROUP_NS
    M = F.models(which)[1]
    thr2 = F.THR2[which]
    i, j = F.models(which)[0].index("truth"), 0
    members = [{"problem": world.problem(which, nf), "model": M[i], "thr2": thr2},
               {"problem": world.problem(which, ns), "model": M[j], "thr2": thr2, "capacity": nf},
               {"problem": world.problem(which, nf), "model": M[i], "thr2": thr2, "idle": True}]
    for order in ((0, 1, 2), (2, 1, 0)):
        outs = gpu.debug_focal_stage("mask", [members[k] for k in order], group=True)
        outs = [outs[order.index(k)] for k in range(3)]
        check_mask(outs[0], F.expected_masks(which, nf)[i], nf, "full")
        check_mask(outs[1], F.expected_masks(which, ns)[j], ns, "short")
        untouched(outs[2])
    single = gpu.debug_focal_stage("mask", members[0])
    assert np.array_equal(single["mask"], outs[0]["mask"]) and np.array_equal(single["host_mask"], outs[0]["host_mask"])


# ---------------------------------------------------------------------------------------------------------------- 8. rejections
def test_calls_that_do_not_fit_are_rejected(gpu, world):
    prob = world.problem(0, 65)
    g = F.generated(0, 300)
    samples = (g.samples[:4] % 65).astype(np.uint32)
    models = F.padded(0, 4)[0]
    bad = [("generate", {"problem": prob}),                                                              # neither samples nor positions
           ("generate", {"problem": prob, "samples": samples, "positions": np.zeros(4, dtype=np.uint32)}),  # both
           ("generate", {"problem": prob, "samples": np.full((1, 4), 65, dtype=np.uint32)}),             # a sample index >= n
           ("generate", {"problem": prob, "samples": np.zeros((0, 4), dtype=np.uint32)}),                # 0 iterations
           ("generate", {"problem": prob, "positions": np.zeros((1 << 20) + 1, dtype=np.uint32)}),       # more than 2^20 iterations
           ("generate", {"problem": world.problem(0, 1), "positions": np.zeros(2, dtype=np.uint32)}),    # fewer points than a sample
           ("score", {"problem": prob, "thr2": 1.0, "count": 4}),                                        # a null argument
           ("score", {"problem": prob, "models": models, "thr2": 1.0, "capacity": 2}),                   # buffers below the launch
           ("score", {"problem": prob, "models": models, "num_models": np.ones(1, dtype=np.uint32), "thr2": 1.0}),  # 4 slots, gate of 10
           ("mask", {"problem": prob, "thr2": 1.0})]                                                     # a null argument
    for stage, member in bad:
        with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
            gpu.debug_focal_stage(stage, member)
    a, b = F.points(1, 65)
    wrong = gpu.Problem(gpu.KIND_REL, a, b)  # a problem kind without focal-length kernels
    try:
        with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
            gpu.debug_focal_stage("score", {"problem": wrong, "models": models, "thr2": 1.0})
        with pytest.raises(gpu.PoseLibAmdError, match="error -3"):  # members of two kinds
            gpu.debug_focal_stage("score", [{"problem": prob, "models": models, "thr2": 1.0},
                                            {"problem": world.problem(1, 65), "models": models, "thr2": 1.0}], group=True)
    finally:
        wrong.close()
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):  # the single launch takes one member
        gpu.debug_focal_stage("score", [{"problem": prob, "models": models, "thr2": 1.0}] * 2)
