"""The fused bound launch and the early exit of the exact launch on the device (-m gpu), through pl_debug_score_bounded on the
single launches (route 0) and the group form (route 2).

The bound kernel gives a workgroup of 8 wavefronts a unit of 64 list entries behind the lead, wavefront w the chunks w, w + 8,
...; it decides the verdict stage inside the workgroup, compacts what is undecided and bounds the residuals of exactly those; the
list is rebuilt by a second launch, tile by tile of 1024.  The lists here are built so that the REFERENCE says how many entries stand
behind the lead and how many of them each stage leaves - a case that degenerates fails on the CPU side, before the device is asked:

  the lead: kPruneLead P3P models of random samples.  The incumbent (init_max, init_min) is chosen above the lead's best, so that
    lead_max = init_max and lead_min = init_min whatever the lead holds (asserted on the device's report);
  behind it, planted models, every one a perturbed ground truth, sorted into three kinds by the oracle's counts and scores
  (prune_cases.reference) and the host build of the tier's two per-pair functions (hostmath_bound_lib), with margins:
    keep:  score <= lead_min.  Every lower bound of its score is <= lead_min: no stage can drop it, the exact launch scores it;
    late:  the verdict stage cannot drop it (its proven outliers alone do not reach lead_min) but the residual stage does;
    early: the verdict stage drops it.
  All three have (S - cs) thr^2 <= lead_min on the chunks [0, c*) of BOTH routes, and the filter's survivors are at least the
  inliers: the pre-selection keeps every planted model, so the entries behind the lead are exactly the planted ones.

Entries behind the lead: 1, 63, 64, 65 (one unit, the unit's boundary, a second unit) and 1100 (a second tile of the rebuild); the
residual stage sees 0 (only `early`), 1 and more than 64 entries.  N = 1281: five chunks in both routes, the last with one real
column - every wavefront has at most one chunk and keeps it for all units.  N = 5120 and 5121, a scene of this file: 16 / 17
chunks of 320 in both routes (wavefronts walk two chunks each, with 17 wavefront 0 a third with one real column;
pl_debug_score_shape gives the single launches 5 points per lane at this size, not 21 chunks of 256).

Asserted: prune_cases' and test_gpu_score_bound's properties (_check, _same, bitwise: every bound on the right side of the
reference, tier 2 exactly where the rule holds on the reported bounds, exact counts the plain scorer's and scores within
reorder_tol, candidates the plain step's and pl_debug_score_pruned's, routes bit for bit in bounds and tiers, the same launches
twice the same bits), and the tiers the kinds predict."""
import functools

import numpy as np
import pytest

import hostmath_bound_lib as HB
import hostmath_lib as HM
import prune_cases as PC
import test_gpu_score_bound as TB
import test_gpu_score_prune as TP
from poselib_amd import synth
from prune_cases import GROUP, SINGLE

pytestmark = pytest.mark.gpu

L = PC.LEAD
THR2 = PC.THR ** 2
NO_BOUND = TB.NO_BOUND
KEEP, LATE, EARLY = 0, 1, 2
SLACK_COUNT = 20  # init_max = the ground truth's count + this: room for the pairs a count bound adds to the inliers
MARGIN_PAIRS = 3  # a kind holds with this many pairs (thr^2 each in the score, one each in the count) to spare
SLACK_SCORE = 3   # init_min = the ground truth's score + this many thr^2: room for MARGIN_PAIRS on both sides of the verdict stage
LEAD_CLEAR = 10   # pairs by which every lead model stays behind the ground truth, in count and in score
RATIO = 0.7


# ---- scenes and planted models (no device) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_scene():
    """5121 correspondences, normalised as prune_cases.Scene's"""
    d = synth.absolute_pose_scene(5121, RATIO, 9207)
    sc = PC.Scene.__new__(PC.Scene)
    sc.a = np.ascontiguousarray((np.asarray(d["p2d"]) - 500.0) / PC.FOCAL)
    sc.b = np.ascontiguousarray(np.asarray(d["p3d"], float))
    sc.gt = np.r_[np.asarray(d["q_gt"], float), np.asarray(d["t_gt"], float)]
    sc.ratio = RATIO
    return sc


def scene_of(N):
    return big_scene() if N > PC.N_MAX else PC.scene(RATIO)


@functools.lru_cache(maxsize=None)
def lead_of(N):
    """L live P3P models of random samples of the first N correspondences, without those that come within LEAD_CLEAR pairs of
    the ground truth's count or score (host build of the scorer): the incumbent below is the lead's best on every device"""
    sc = scene_of(N)
    a, b = sc.points(N)
    cols = (a[:, 0], a[:, 1], b[:, 0], b[:, 1], b[:, 2])
    s_gt, c_gt, _, _ = HM.score("abs", HM.pose_record(sc.gt[:4], sc.gt[4:]), cols, THR2)
    m = sc.p3p_models(N, 2 * L + 512, 500 + N)
    m = m[~np.isnan(m).any(axis=1)]
    sc_cnt = [HM.score("abs", HM.pose_record(k[:4], k[4:]), cols, THR2)[:2] for k in m]
    far = np.array([c + LEAD_CLEAR <= c_gt and s >= s_gt + LEAD_CLEAR * THR2 for s, c in sc_cnt])
    m = m[far][:L]
    assert len(m) == L
    return m


@functools.lru_cache(maxsize=None)
def pool(N):
    """{"init": the incumbent, "cand": perturbed ground truths, "kinds": {kind: indices into cand}, "r2", "inl": their reference}"""
    sc = scene_of(N)
    a, b = sc.points(N)
    cols = (a[:, 0], a[:, 1], b[:, 0], b[:, 1], b[:, 2])
    xy = float(np.abs(a).max())
    sizes = [1e-7] * 6 + list(np.geomspace(2e-4, 1e-3, 40)) + list(np.geomspace(1e-3, 1e-2, 30))
    cand = np.array([sc.gt] + [PC.perturbed_gt(sc, s, 40 + i) for i, s in enumerate(sizes)])
    r2, inl, live = PC.reference(sc, N, cand)
    assert live.all()
    c = inl.sum(axis=1)
    s = np.where(inl, r2, 0.0).sum(axis=1) + (N - c) * THR2
    init_max, init_min = int(c[0]) + SLACK_COUNT, float(s[0]) + SLACK_SCORE * THR2
    beat = init_min * (1.0 + PC.MARGIN_SCORE)
    # c* and S of both routes from the incumbent alone (lead_max = init_max, lead_min = init_min: asserted on the device)
    S = []
    for route in (SINGLE, GROUP):
        cp = PC.chunk_points(N, route)
        chunks = (N + cp - 1) // cp
        cstar = PC.split_chunk(init_max, init_min, N, THR2, cp, chunks)
        assert cstar < chunks, (N, route, "nothing would be pruned")
        S.append(min(cstar * cp, N))
    kinds = {KEEP: [], LATE: [], EARLY: []}
    for k in range(len(cand)):
        if not all((Sr - inl[k, :Sr].sum()) * THR2 <= init_min for Sr in S):
            continue  # (the pre-selection might drop it: not a planted model)
        if s[k] <= init_min:
            kinds[KEEP].append(k)
            continue
        rec = HM.pose_record(cand[k][:4], cand[k][4:])
        en, _, maybe0, q0 = HB.bound(rec, cols, THR2, xy, residual=False)
        en1, _, maybe1, q1 = HB.bound(rec, cols, THR2, xy, residual=True)
        assert en and en1
        out0 = int((~maybe0).sum())  # proven outliers: thr^2 each
        if int(maybe0.sum()) + MARGIN_PAIRS <= init_max and (out0 - MARGIN_PAIRS) * THR2 > beat:
            kinds[EARLY].append(k)
        elif ((out0 + MARGIN_PAIRS) * THR2 <= init_min and int(maybe1.sum()) + MARGIN_PAIRS <= init_max
              and (float(q1.astype(np.int64).sum()) / HB.SCALE - MARGIN_PAIRS) * THR2 > beat):
            kinds[LATE].append(k)
    print(f"N {N}: incumbent ({init_max}, {init_min / THR2:.2f} thr^2), S {S}, keep {len(kinds[KEEP])} late {len(kinds[LATE])} "
          f"early {len(kinds[EARLY])} of {len(cand)} perturbed ground truths")
    assert len(kinds[KEEP]) >= 3 and len(kinds[LATE]) >= 3 and len(kinds[EARLY]) >= 8, (N, {k: len(v) for k, v in kinds.items()})
    return {"init": (init_max, init_min), "cand": cand, "kinds": kinds, "r2": r2, "inl": inl}


def planted(N, kinds_behind):
    """(models, the planted models' indices into the pool, kinds (H,) with -1 in the lead): the lead, then one model of the pool
    per entry of kinds_behind, every kind's models taken round robin"""
    P = pool(N)
    idx = np.array([P["kinds"][kind][i % len(P["kinds"][kind])] for i, kind in enumerate(kinds_behind)], dtype=np.int64)
    models = np.concatenate([lead_of(N), P["cand"][idx]])
    return models, idx, np.r_[np.full(L, -1), np.asarray(kinds_behind, dtype=np.int64)]


# kinds behind the lead, and what the residual stage sees (entries undecided after the verdict stage = keep + late)
def _long():
    k = np.full(1100, EARLY)
    k[64 + 63] = KEEP            # second unit: one undecided entry, its last
    k[128:192] = LATE            # third unit: all 64 undecided, all dropped by the residual stage
    k[192:256:2] = KEEP          # fourth: every second one stays
    k[193:256:6] = LATE
    k[1023], k[1024], k[1030], k[1099] = KEEP, LATE, KEEP, KEEP  # the second tile of the rebuild starts with entries to move
    return k.tolist()


LISTS = {
    "1 keep": [KEEP], "1 early": [EARLY], "1 late": [LATE],
    "63 early": [EARLY] * 63,
    "64, one keep": [EARLY] * 63 + [KEEP],
    "65 undecided": ([KEEP, LATE] * 33)[:65],
    "65, one late": [EARLY] * 64 + [LATE],
    "1100": _long(),
}
UNDECIDED = {"1 keep": 1, "1 early": 0, "1 late": 1, "63 early": 0, "64, one keep": 1, "65 undecided": 65, "65, one late": 1, "1100": 1 + 64 + 32 + 11 + 4}


def test_lists_are_what_they_are_named():
    """(no device) the entries behind the lead and what the verdict stage leaves, from the kinds alone"""
    for name, kinds in LISTS.items():
        k = np.asarray(kinds)
        assert len(k) == int(name.split()[0].rstrip(",")), name
        assert int((k != EARLY).sum()) == UNDECIDED[name], (name, int((k != EARLY).sum()))
    assert sorted(set(UNDECIDED.values()))[:2] == [0, 1] and max(UNDECIDED.values()) > 64
    assert {len(k) for k in LISTS.values()} >= {1, 63, 64, 65, 1100}


# ---- device ------------------------------------------------------------------------------------------------------------------------------
_problems = {}


def _problem(gpu, N):
    if N not in _problems:
        _problems[N] = gpu.Problem(gpu.KIND_ABS, *scene_of(N).points(N))
    return _problems[N]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for p in _problems.values():
        p.close()
    _problems.clear()


def _check(tag, out, stream, N, idx, kinds, init, pruned_cand):
    """test_gpu_score_bound._check for a planted list: the reference covers the planted models, which are all that the tier sees"""
    P = pool(N)
    H = len(kinds)
    behind = kinds >= 0
    tiers, bc, bs = out["tiers"], out["bound_counts"], out["bound_scores"]
    has = bc != NO_BOUND
    full_c = np.zeros(H, dtype=np.int64)
    full_s = np.full(H, np.nan)
    inl, r2 = P["inl"][idx], P["r2"][idx]
    full_c[behind] = inl.sum(axis=1)
    full_s[behind] = np.where(inl, r2, 0.0).sum(axis=1) + (N - full_c[behind]) * THR2
    print(tag, "c*", out["cstar"], "of", out["chunks"], "behind the lead", int(behind.sum()), "dropped on counts", int((tiers == 1).sum()),
          "bounded", int(has.sum()), "dropped on bounds", int((tiers == 2).sum()), "exact launch scored", out["num_preselected"])
    assert out["num_live"] == H and (tiers != 3).all(), tag
    assert out["lead_max"] == init[0] and out["lead_min"] == init[1], (tag, "the lead beats the incumbent", out["lead_max"], out["lead_min"])
    assert out["cstar"] < out["chunks"], tag
    assert (tiers[~behind] == 0).all(), (tag, "a lead position without exact scores")
    # every planted model is pre-selected, bounded, and nothing else is
    assert (has == behind).all() and not (tiers == 1).any(), (tag, "the entries behind the lead are not the planted ones")
    assert np.isnan(bs[~has]).all() and not np.isnan(bs[has]).any(), tag
    assert (bc[has].astype(np.int64) >= full_c[has]).all(), (tag, np.flatnonzero(has & (bc < full_c))[:5])
    assert (bs[has] <= full_s[has]).all(), (tag, np.flatnonzero(has & ~(bs <= full_s))[:5])
    beat = out["lead_min"] * (1.0 + PC.MARGIN_SCORE)
    rule = (bc[has] <= out["lead_max"]) & (bs[has] > beat)
    assert ((tiers[has] == 2) == rule).all(), (tag, "the decision is not the rule on the reported bounds")
    # the kinds: what the reference says each stage does
    assert (tiers[kinds == KEEP] == 0).all(), (tag, "a model that cannot be dropped was")
    assert (tiers[kinds == EARLY] == 2).all(), (tag, "the verdict stage kept what it drops")
    assert (tiers[kinds == LATE] == 2).all(), (tag, "the residual stage did not see, or kept, what it drops")
    assert out["num_preselected"] == (kinds == KEEP).sum(), (tag, "the exact launch's list")
    assert (out["kept"] == (tiers == 0)).all(), tag
    kept = tiers == 0
    cnt, sc = out["counts"], out["scores"]
    assert (cnt[kept] == stream[0][kept]).all(), (tag, "exact counts differ from the plain scorer's")
    diff = np.abs(sc[kept] - stream[1][kept])
    assert (diff <= TB.reorder_tol(cnt[kept], stream[1][kept])).all(), (tag, "exact scores differ by more than a reordered sum can")
    assert (cnt[~kept] == 0).all() and (sc[~kept] == N * THR2).all(), tag
    want = PC.records_rule(stream[0], stream[1], *init)
    got = sorted(out["cand"].tolist())
    assert out["num_cand"] == len(out["cand"]) and got == want, (tag, got[:8], want[:8])
    assert got == pruned_cand, (tag, "pl_debug_score_pruned lists other candidates")


def _run(gpu, N, name, twice=False):
    """both routes of one list; returns {route: out}"""
    models, idx, kinds = planted(N, LISTS[name])
    init = pool(N)["init"]
    p = _problem(gpu, N)
    member = (p, models, PC.THR, init[0], init[1])
    outs = {}
    for route in (SINGLE, GROUP):
        stream = TB._stream(gpu, p, models, route)
        (out,), idle, guard = gpu.score_bounded([member], route)
        assert idle == 0 and guard == 0, (N, name, route, idle, guard)
        (pr,), idle = gpu.score_pruned([member], route)
        assert idle == 0
        _check((N, name, route), out, stream, N, idx, kinds, init, sorted(pr["cand"].tolist()))
        if twice:
            (again,), _, _ = gpu.score_bounded([member], route)
            TB.bitwise((N, name, route, "twice"), out, again)
        outs[route] = out
    TB._same((N, name), outs[SINGLE], outs[GROUP], PC.chunk_points(N, SINGLE) == PC.chunk_points(N, GROUP))
    # (planted lists: both routes bound every planted model, whatever their chunks)
    for key in ("tiers", "bound_counts"):
        assert (outs[SINGLE][key] == outs[GROUP][key]).all(), (N, name, key)
    assert outs[SINGLE]["bound_scores"].tobytes() == outs[GROUP]["bound_scores"].tobytes(), (N, name)
    return outs


@pytest.mark.parametrize("name", list(LISTS))
def test_units_and_stages(gpu, name):
    """1281 correspondences: five chunks in both routes, the last with one real column"""
    _run(gpu, 1281, name, twice=name in ("65 undecided", "1100"))


@pytest.mark.parametrize("N", [5120, 5121])
def test_more_than_sixteen_chunks(gpu, N):
    """16 / 17 chunks of 320 in both routes (the single launches take 5 points per lane at this size too): every wavefront walks
    two chunks, with 17 wavefront 0 a third one that has one real column"""
    outs = _run(gpu, N, "65 undecided", twice=True)
    for route in (SINGLE, GROUP):
        assert outs[route]["chunk_points"] == PC.chunk_points(N, route) == 320, route
        assert outs[route]["chunks"] == (16 if N == 5120 else 17), route
    _run(gpu, N, "64, one keep")


def test_exact_launch_without_units_and_with_one(gpu):
    """the exact launch behind the tier: a selection of length 0 (every workgroup returns before it stages anything) and one of a
    single entry (one unit: the workgroups of every slice but the first return early); counts the plain scorer's, scores within
    reorder_tol (_check)"""
    for name, length in (("63 early", 0), ("1 late", 0), ("1 keep", 1), ("64, one keep", 1)):
        for route, out in _run(gpu, 1281, name).items():
            assert out["num_preselected"] == length, (name, route)
            assert out["slices"] >= 1


def test_group_launch_whose_members_differ(gpu):
    """four members of one group launch: 5 chunks, 17 chunks, a list that is the lead alone (the tier is idle: no entry behind
    the lead, the list ends with length 0) and an incumbent nothing beats on 16 chunks (all dropped on counts or in the verdict
    stage) - each against the same member alone, bit for bit; the inactive slot and the guard words unchanged"""
    members = []
    for N, name in ((1281, "1100"), (5121, "65 undecided"), (1281, None), (5120, "64, one keep")):
        init = pool(N)["init"]
        if name is None:
            members.append((_problem(gpu, N), lead_of(N), PC.THR, init[0], init[1]))
        else:
            members.append((_problem(gpu, N), planted(N, LISTS[name])[0], PC.THR, init[0], init[1]))
    members[3] = members[3][:3] + (5120, 0.0)
    outs, idle, guard = gpu.score_bounded(members, GROUP)
    assert idle == 0 and guard == 0
    assert [o["chunks"] for o in outs] == [5, 17, 5, 16]
    assert (outs[2]["bound_counts"] == NO_BOUND).all() and outs[2]["num_preselected"] == 0 and (outs[2]["tiers"] == 0).all(), "the tier is idle"
    assert outs[3]["num_cand"] == 0 and (outs[3]["tiers"][L:] > 0).all() and outs[3]["num_preselected"] == 0
    assert (outs[0]["tiers"][L:] == np.where(np.asarray(LISTS["1100"]) == KEEP, 0, 2)).all()
    for i, m in enumerate(members):
        (alone,), idle, guard = gpu.score_bounded([m], GROUP)
        assert idle == 0 and guard == 0
        TB.bitwise(("among others against alone", i), outs[i], alone)


def test_batch_with_a_member_that_does_not_prune(gpu):
    """a group's batch steps in which one member stays below the gate (its step does not prune: both bound launches return at
    once for it, the exact launch scores its whole list) next to two that prune: every member equals its single run bit for bit"""
    runs = []
    for n, ratio, noise, seed, it in ((1100, 0.7, 0.5, 7100, TP.GATE), (1300, 0.2, 0.05, 7101, TP.GATE // 2), (5121, 0.7, 0.5, 7103, TP.GATE)):
        d = synth.absolute_pose_scene(n, ratio, seed, noise_px=noise)
        x, X = (np.asarray(d["p2d"]) - 500.0) / PC.FOCAL, np.asarray(d["p3d"], float)
        assert gpu.score_prune_gate(0, n, it) == (it >= TP.GATE)
        runs.append((x, X, TP._opt(90 + len(runs), max_iterations=it, min_iterations=it)))
    probs = [gpu.Problem(gpu.KIND_ABS, x, X) for x, X, _ in runs]
    single = [p.run(opt) for p, (_, _, opt) in zip(probs, runs)]
    got = gpu.ransac_batch(probs, [opt for _, _, opt in runs], 2, len(runs))
    for i, ((m, info), (wm, winfo)) in enumerate(zip(got, single)):
        for key in TP.KEYS:
            assert info[key] == winfo[key], (i, key, info[key], winfo[key])
        assert info["inliers"] == winfo["inliers"], i
        assert (np.r_[m.q, m.t] == np.r_[wm.q, wm.t]).all(), i
    for p in probs:
        p.close()
