"""The bound tier of the pruned matrix-core absolute-pose scorer on the device (-m gpu), through pl_debug_score_bounded - the launch
sequence of a group's batch step: lead, split chunk, survivor counts, pre-selection, fp32 bounds of the pre-selected positions behind
the lead, second selection, exact scores of what is left (without the lead), finalize and the candidate scan - on the single
launches (route 0) and the group form (route 2).

Asserted per list: every bound is on the right side of the reference's count and score; positions with exact scores report the
plain streaming scorer's counts exactly and its scores up to the order in which c inliers' residuals are added (reorder_tol below:
on the device the lead launch alone - code this tier does not touch - differs from the plain launch in the last bit of some scores,
so bitwise equality with ANOTHER launch is not a property of the pruned form; the same launches twice, and a member alone against
the same member among others, are compared bit for bit); dropped ones report (0, N thr^2) exactly; the candidate list equals the
plain step's and pl_debug_score_pruned's; the two routes agree bit for bit in counts, dropped values and candidates, and in tiers
and bounds wherever their chunks are the same; the inactive slot and the guard words are unchanged.

Point counts.  The matrix-core scorer - the only one that prunes - starts at 1024 correspondences, which are four chunks: counts of
700 and 960 (three chunks) are refused by the entry (PL_ERR_UNSUPPORTED, asserted below).  The counts here are the smallest the
scorer takes: 1024 (single launches: four full chunks of 256, the 4-points-per-lane build of the bound kernel; group form: three
chunks of 320 and a last one with 64 real columns), 1280 (four full chunks of 320) and 1281 (a last chunk with ONE real column)."""
import functools

import numpy as np
import pytest

import prune_cases as PC
import test_gpu_score_prune as TP
from prune_cases import GROUP, SINGLE

pytestmark = pytest.mark.gpu

L = PC.LEAD
THR2 = PC.THR ** 2
NS = (1024, 1280, 1281)
NO_BOUND = 0xffffffff
# Scores of one hypothesis from two DIFFERENT launches.  Counts are integers and equal.  A score is the sum of the c inliers' fp64
# residuals, which the exact pass adds in the order its drains meet them - that depends on the launch's units (how many hypotheses
# share a wavefront's queue), and the lead launch, the exact launch on a selection and the plain launch cut the list differently -
# plus (N - c) thr^2, formed alike everywhere.  Two orders of the same c non-negative terms each stay within (c - 1) 2^-53 of the
# exact sum, relatively, so the two scores differ by less than c 2^-52 (+ one ulp of the final addition): a handful of ulp for a
# wrong hypothesis.  The SAME launches twice give the same bits, which bitwise() checks.
ULP = 2.0 ** -52


def reorder_tol(counts, scores):
    return (np.asarray(counts, np.float64) + 1.0) * ULP * np.abs(scores)


# ---- lists (no device) -----------------------------------------------------------------------------------------------------------------
def with_nans(models, ref, where):
    """NaN models inserted in front of the positions `where` of a list and of its reference"""
    r2, inl, live = ref
    where = np.asarray(where)
    nan_rows = np.array([PC.nan_model(models[min(w, len(models) - 1)], i) for i, w in enumerate(where)])
    return (np.insert(models, where, nan_rows, axis=0),
            (np.insert(r2, where, np.inf, axis=0), np.insert(inl, where, False, axis=0), np.insert(live, where, False)))


@functools.lru_cache(maxsize=None)
def lists_of(ratio, N):
    """{name: (models, reference)}: LEAD, LEAD + 1 and LEAD + 33 live models with NaN models in between, and about 2 x LEAD live
    models with the NaN models the solver gave"""
    models, ref = TP.short_list(ratio, N)
    out = {}
    for H in TP.LENGTHS:
        cut = (models[:H], tuple(a[:H] for a in ref))
        out[H] = with_nans(*cut, [0, 7, 7, L // 2, L - 1, H])
    lm, (r2, inl, live) = TP.long_list(ratio, 1281, 12 * L if ratio == 0.1 else 2 * L) if N == 1281 else (None, (None, None, None))
    if lm is not None:
        K = int(np.searchsorted(np.cumsum(live), 2 * L - 40)) + 1
        out["2L"] = (lm[:K], (r2[:K], inl[:K], live[:K]))
    return out


def incumbents(ref, N):
    """none; one that beats everything; one in between (the list's eighth-best count and score)"""
    r2, inl, live = ref
    c = np.where(live, inl.sum(axis=1), 0)
    s = np.where(live, np.where(inl, r2, 0.0).sum(axis=1) + (N - c) * THR2, N * THR2)
    k = max(1, int(live.sum()) // 8)
    return {"none": (0, PC.DBL_MAX), "best": (N, 0.0), "between": (int(np.sort(c)[-k]), float(np.sort(s)[k]))}


# ---- device ------------------------------------------------------------------------------------------------------------------------------
def _stream(gpu, p, models, route):
    if route == SINGLE:
        c, s, path = p.score_stream(models, PC.THR)
        assert path == 2
        return c, s
    (st,), idle = gpu.score_stream_group([(p, models, PC.THR, 0)])
    assert idle == 0
    return st["counts"], st["scores"]


def _check(tag, out, stream, ref, N, init, pruned_cand):
    r2, inl, live = ref
    full_c = np.where(live, inl.sum(axis=1), 0)
    full_s = np.where(live, np.where(inl, r2, 0.0).sum(axis=1) + (N - full_c) * THR2, N * THR2)
    tiers, bc, bs = out["tiers"], out["bound_counts"], out["bound_scores"]
    has = bc != NO_BOUND
    pos = np.cumsum(live) - 1
    behind = live & (pos >= L)
    print(tag, "c*", out["cstar"], "of", out["chunks"], "live", out["num_live"], "behind the lead", int(behind.sum()), "dropped on counts",
          int((tiers == 1).sum()), "bounded", int(has.sum()), "dropped on bounds", int((tiers == 2).sum()), "exact launch scored",
          out["num_preselected"])
    if has.any():
        print("    count bound - count: max", int((bc[has].astype(np.int64) - full_c[has]).max()), " score bound / score: min",
              float((bs[has] / full_s[has]).min()), "max", float((bs[has] / full_s[has]).max()))
    assert out["num_live"] == live.sum() and (tiers[~live] == 3).all() and (tiers[live] != 3).all(), tag
    assert (tiers[live & ~behind] == 0).all(), (tag, "a lead position without exact scores")
    assert not (has & ~behind).any() and np.isnan(bs[~has]).all() and not np.isnan(bs[has]).any(), tag
    # every bound on the right side of the reference
    assert (bc[has].astype(np.int64) >= full_c[has]).all(), (tag, np.flatnonzero(has & (bc < full_c))[:5])
    assert (bs[has] <= full_s[has]).all(), (tag, np.flatnonzero(has & ~(bs <= full_s))[:5])
    if out["cstar"] == out["chunks"]:
        assert not has.any() and (tiers[live] == 0).all(), (tag, "c* = chunks: everything is the exact launch's")
    else:
        assert (has == (behind & (tiers != 1))).all(), (tag, "bounds for the pre-selected positions behind the lead, and only for them")
        assert out["num_preselected"] == (behind & (tiers == 0)).sum(), (tag, "the exact launch scores the lead again, or not all that is kept")
        # the tier's decision is its rule on the bounds it reports
        beat = out["lead_min"] * (1.0 + PC.MARGIN_SCORE)
        rule = (bc[has] <= out["lead_max"]) & (bs[has] > beat)
        assert ((tiers[has] == 2) == rule).all(), tag
    assert (out["kept"] == ((tiers == 0) | (tiers == 3))).all(), tag
    kept = tiers == 0
    cnt, sc = out["counts"], out["scores"]
    assert (cnt[kept] == stream[0][kept]).all(), (tag, "exact counts differ from the plain scorer's")
    if kept.any():
        diff = np.abs(sc[kept] - stream[1][kept])
        print("    exact scores against the plain scorer's: max difference in ulp", float((diff / (ULP * stream[1][kept])).max()),
              "bitwise equal", int((sc[kept] == stream[1][kept]).sum()), "of", int(kept.sum()))
        assert (diff <= reorder_tol(cnt[kept], stream[1][kept])).all(), (tag, "exact scores differ from the plain scorer's by more than a reordered sum can")
    gone = (tiers == 1) | (tiers == 2)
    assert (cnt[gone] == 0).all() and (sc[gone] == N * THR2).all(), tag
    want = PC.records_rule(stream[0], stream[1], *init)
    got = sorted(out["cand"].tolist())
    assert out["num_cand"] == len(out["cand"]) and got == want, (tag, got[:8], want[:8])
    assert got == pruned_cand, (tag, "pl_debug_score_pruned lists other candidates")


def _same(tag, a, b, whole):
    """the two routes: bit for bit - everything where their chunks are the same, else what does not depend on c*"""
    assert sorted(a["cand"].tolist()) == sorted(b["cand"].tolist()) and a["lead_max"] == b["lead_max"], tag
    assert abs(a["lead_min"] - b["lead_min"]) <= (a["lead_max"] + 1.0) * ULP * abs(b["lead_min"]), tag
    both = (a["tiers"] == 0) & (b["tiers"] == 0)
    assert (a["counts"][both] == b["counts"][both]).all(), tag
    assert (np.abs(a["scores"][both] - b["scores"][both]) <= reorder_tol(b["counts"][both], b["scores"][both])).all(), tag
    gone = (a["tiers"] > 0) & (b["tiers"] > 0)
    assert (a["counts"][gone] == b["counts"][gone]).all() and (a["scores"][gone] == b["scores"][gone]).all(), tag
    assert ((a["tiers"] == 3) == (b["tiers"] == 3)).all(), tag
    # bounds are integer sums over the correspondences, and the first stage decides on them alone: an entry both routes bounded
    # went through the same stages and carries the same bounds, whatever the chunks
    hb = (a["bound_counts"] != NO_BOUND) & (b["bound_counts"] != NO_BOUND)
    assert (a["bound_counts"][hb] == b["bound_counts"][hb]).all() and (a["bound_scores"][hb] == b["bound_scores"][hb]).all(), tag
    assert (a["tiers"][hb] == b["tiers"][hb]).all(), tag
    if whole:  # the same chunks: the same c*, the same decisions
        for key in ("tiers", "counts", "bound_counts", "bound_scores"):
            assert (np.asarray(a[key]) == np.asarray(b[key]))[~np.isnan(np.asarray(a[key], np.float64))].all(), (tag, key)
        assert a["cstar"] == b["cstar"] and a["num_preselected"] == b["num_preselected"], tag


def bitwise(tag, a, b):
    """the same launches twice: every field bit for bit"""
    for key in ("tiers", "counts", "scores", "bound_counts", "bound_scores", "kept"):
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.tobytes() == y.tobytes(), (tag, key)
    assert a["cand"].tolist() == b["cand"].tolist() or sorted(a["cand"].tolist()) == sorted(b["cand"].tolist()), tag
    assert a["lead_min"] == b["lead_min"] and a["cstar"] == b["cstar"] and a["num_preselected"] == b["num_preselected"], tag


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("ratio", [0.1, 0.7, 1.0])
def test_bounded_step(gpu, ratio, N):
    p = TP._problem(gpu, ratio, N)
    dropped_on_bounds = 0
    for name, (models, ref) in lists_of(ratio, N).items():
        streams = {route: _stream(gpu, p, models, route) for route in (SINGLE, GROUP)}
        for iname, init in incumbents(ref, N).items():
            outs = {}
            for route in (SINGLE, GROUP):
                (out,), idle, guard = gpu.score_bounded([(p, models, PC.THR, init[0], init[1])], route)
                assert idle == 0 and guard == 0, (name, iname, route, idle, guard)
                (pr,), idle = gpu.score_pruned([(p, models, PC.THR, init[0], init[1])], route)
                assert idle == 0
                _check((ratio, N, name, iname, route), out, streams[route], ref, N, init, sorted(pr["cand"].tolist()))
                outs[route] = out
                if iname == "between":
                    (again,), _, _ = gpu.score_bounded([(p, models, PC.THR, init[0], init[1])], route)
                    bitwise((ratio, N, name, iname, route, "twice"), out, again)
                live = ref[2]
                behind = live & (np.cumsum(live) > L)
                if name == L:
                    assert not behind.any() and (out["bound_counts"] == NO_BOUND).all(), "the tier is idle"
                if iname == "none" and ratio == 1.0:
                    assert out["cstar"] == out["chunks"]
                if iname == "best":
                    assert out["num_cand"] == 0 and out["cstar"] < out["chunks"] and (out["tiers"][behind] > 0).all(), (name, route, "all dropped")
                dropped_on_bounds += int((out["tiers"] == 2).sum())
            _same((ratio, N, name, iname), outs[SINGLE], outs[GROUP], PC.chunk_points(N, SINGLE) == PC.chunk_points(N, GROUP))
    if N == 1281 and ratio < 1.0:
        assert dropped_on_bounds > 0, "no list of this scene gave the tier anything to drop"


def test_group_launch_of_mixed_members(gpu):
    """four members of one launch: three point counts, one list the tier is idle on, one incumbent that beats everything"""
    cases = [(0.7, 1024, L + 33, "between"), (0.1, 1281, "2L", "none"), (0.7, 1280, L, "none"), (0.7, 1281, "2L", "best")]
    members, refs, inits = [], [], []
    for ratio, N, name, iname in cases:
        models, ref = lists_of(ratio, N)[name]
        init = incumbents(ref, N)[iname]
        members.append((TP._problem(gpu, ratio, N), models, PC.THR, init[0], init[1]))
        refs.append(ref), inits.append(init)
    outs, idle, guard = gpu.score_bounded(members, GROUP)
    assert idle == 0 and guard == 0
    prs, idle = gpu.score_pruned(members, GROUP)
    assert idle == 0
    for (ratio, N, name, iname), m, out, pr, ref, init in zip(cases, members, outs, prs, refs, inits):
        _check(("mixed", ratio, N, name, iname), out, _stream(gpu, m[0], m[1], GROUP), ref, N, init, sorted(pr["cand"].tolist()))
        (alone,), _, _ = gpu.score_bounded([m], GROUP)
        bitwise(("mixed against alone", N, name), out, alone)


@pytest.mark.parametrize("N", [700, 960])
def test_three_chunk_problems_are_not_the_pruned_scorers(gpu, N):
    from poselib_amd import PoseLibAmdError

    sc = PC.scene(0.7)
    p = gpu.Problem(gpu.KIND_ABS, *sc.points(N))
    with pytest.raises(PoseLibAmdError):
        gpu.score_bounded([(p, TP.short_list(0.7, 1024)[0][:64], PC.THR, 0, PC.DBL_MAX)], SINGLE)
    p.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_batch_call_equals_the_single_runs_bit_for_bit(gpu):
    """group steps that pass the gate (>= 8192 iterations, >= 3 chunks) against pl_ransac_run, whose own steps score plainly; the
    second scene has little noise and few outliers, so that most hypotheses behind the lead are good ones that lose against the
    lead's best on their scores: the tier provably drops positions there, shown through the diagnostic entry on models of the kind"""
    from poselib_amd import synth

    runs = []
    for n, ratio, noise, seed, it in ((1100, 0.7, 0.5, 7100, TP.GATE), (1300, 0.2, 0.05, 7101, TP.GATE), (1100, 0.9, 0.5, 7102, 2 * TP.GATE)):
        d = synth.absolute_pose_scene(n, ratio, seed, noise_px=noise)
        x, X = (np.asarray(d["p2d"]) - 500.0) / PC.FOCAL, np.asarray(d["p3d"], float)
        assert gpu.score_prune_gate(0, n, it)
        runs.append((x, X, TP._opt(80 + len(runs), max_iterations=it, min_iterations=it)))
    probs = [gpu.Problem(gpu.KIND_ABS, x, X) for x, X, _ in runs]
    single = [p.run(opt) for p, (_, _, opt) in zip(probs, runs)]
    got = gpu.ransac_batch(probs, [opt for _, _, opt in runs], 2, len(runs))
    for i, ((m, info), (wm, winfo)) in enumerate(zip(got, single)):
        for key in TP.KEYS:
            assert info[key] == winfo[key], (i, key, info[key], winfo[key])
        assert info["inliers"] == winfo["inliers"], i
        assert (np.r_[m.q, m.t] == np.r_[wm.q, wm.t]).all(), i
    # the low-noise scene: oracle P3P models of random samples, as a step of the run generates them
    x, X, _ = runs[1]
    sc = PC.Scene.__new__(PC.Scene)
    sc.a, sc.b = np.ascontiguousarray(x), np.ascontiguousarray(X)
    models = sc.p3p_models(len(x), 2 * L + 600, 17)
    (out,), idle, guard = gpu.score_bounded([(probs[1], models, PC.THR, 0, PC.DBL_MAX)], GROUP)
    print("low-noise scene: c*", out["cstar"], "of", out["chunks"], "dropped on counts", int((out["tiers"] == 1).sum()), "on bounds",
          int((out["tiers"] == 2).sum()), "exact launch scored", out["num_preselected"])
    assert idle == 0 and guard == 0 and out["cstar"] < out["chunks"] and (out["tiers"] == 2).sum() > 0
    for p in probs:
        p.close()
