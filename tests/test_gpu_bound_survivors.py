"""Stage S of the bound tier and the launch that feeds it, on the device (-m gpu), through pl_debug_score_bounded_columns on the single
launches (route 0) and the group form (route 2).

In front of the fp32 verdict the tier judges every pre-selected entry behind the lead on the matrix-core filter's survivor count
over ALL correspondences: the count launch left the words of the chunks [0, c*) in the entry's count column, a second count launch
on the selection (kScoreCountSel) adds the words of the chunks [c*, chunks), wavefront 0 of the bound kernel sums the column and
applies the tier's rule with c = the sum and (N - c) thr^2 for the score.  What stage S leaves goes through the verdict and the
residual stage as before.

Lists as tests/test_gpu_bound_fused.py plants them - a lead the incumbent beats, behind it perturbed ground truths sorted into
kinds by the REFERENCE and the host builds of the filter (hm_prefilter16_abs) and of the tier's per-pair bounds (hostmath_bound),
with margins, so that a case that degenerates fails on the CPU side:
    keep:   score <= lead_min: no stage can drop it;
    late:   neither the survivor count nor the verdict's proven outliers reach lead_min, the residual bounds do;
    early:  the survivor count does not reach lead_min (stage S leaves it), the verdict's proven outliers do;
    far:    the survivor count alone drops it (stage S) - yet the pre-selection, which sees the chunks [0, c*) only, keeps it.
The margins: MARGIN_PAIRS for the fp32 bounds (test_gpu_bound_fused's), MARGIN_SURV = 16 pairs for a survivor count - the device
may differ from the host form by 4 pairs in 4 cells of a list (tests/test_gpu_score_count_lanes.py), which is 16 pairs in one
column at the most.  The incumbent stands SLACK_SCORE = 24 thr^2 above the ground truth's score so that such margins fit.

Cases (point counts: the smallest at which the chunk walk w, w + 8, ..., the `pad` branch and the full-chunk path each occur):
    "one"   1281 correspondences, 10 % outliers: 5 chunks, the last with ONE row; c* = 1 - the new launch counts four chunks;
    "last"  1281 correspondences, 70 % outliers: c* = 4 = chunks - 1 - the new launch has the partial last chunk alone (no entry
            can be `far` there: the pre-selection has seen all rows but one);
    5120 / 5121 correspondences, 70 % outliers: 16 full chunks / 17 with one row in the last, c* = 12;
    "all"   1281 correspondences, all outliers, no incumbent: c* = chunks - the tier and the new launch are idle.

Asserted: the words of the columns [c*, chunks) - and [0, c*) - of every entry the tier dropped equal pl_debug_score_survivors'
words of the same list, word for word (the same tile on the same operands), and the host form's within 4 pairs in 4 cells; an entry
stage S dropped reports the sum of its column and decide's value of (N - c) 2^20 quanta; the kinds end in the tiers they predict;
every bound is on the right side of the reference, the decision is the rule on the reported bounds, kept entries carry the plain
scorer's counts and its scores within reorder_tol, the candidates are the plain step's and pl_debug_score_pruned's; routes agree
bit for bit; idle slot and guard words are unchanged; the same launch twice gives the same bytes."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import hostmath_bound_lib as HB
import hostmath_lib as HM
import prune_cases as PC
import test_gpu_bound_fused as BF
import test_gpu_score_bound as TB
import test_gpu_score_prune as TP
from prune_cases import GROUP, SINGLE

pytestmark = pytest.mark.gpu

L = PC.LEAD
THR2 = PC.THR ** 2
NO_BOUND = TB.NO_BOUND
KEEP, LATE, EARLY, FAR = 0, 1, 2, 3
SLACK_COUNT = 20
SLACK_SCORE = 24
MARGIN_PAIRS = BF.MARGIN_PAIRS
MARGIN_SURV = 16  # 4 pairs in 4 cells (test_gpu_score_count_lanes.MAX_PAIRS, MAX_CELLS), all in one column
MAX_PAIRS, MAX_CELLS = 4, 4
LEAD_CLEAR = BF.LEAD_CLEAR
LEAD_CLEAR_SCORE = SLACK_SCORE + 6  # the incumbent's score stays below every lead model's
# case -> (scene, N, c* the incumbent must give, kinds the pool must hold and how many of each at least)
CASES = {
    "one": (0.1, 1281, 1, {KEEP: 2, LATE: 2, EARLY: 1, FAR: 3}),
    "last": (0.7, 1281, 4, {KEEP: 2, LATE: 2, EARLY: 0, FAR: 0}),
    5120: ("big", 5120, 12, {KEEP: 2, LATE: 2, EARLY: 1, FAR: 3}),
    5121: ("big", 5121, 12, {KEEP: 2, LATE: 2, EARLY: 1, FAR: 3}),
}


# ---- scenes, leads and planted models (no device) ----------------------------------------------------------------------------------------
def scene_of(case):
    key = CASES[case][0]
    return BF.big_scene() if key == "big" else PC.scene(key)


def cols_of(case):
    a, b = scene_of(case).points(CASES[case][1])
    return (a[:, 0], a[:, 1], b[:, 0], b[:, 1], b[:, 2]), float(np.abs(a).max())


@functools.lru_cache(maxsize=None)
def lead_of(case):
    """L live P3P models of random samples that stay LEAD_CLEAR pairs behind the ground truth in count and LEAD_CLEAR_SCORE
    thr^2 in score (host build of the scorer): behind the incumbent on every device.  With 10 % outliers most random samples
    give the ground truth back, so that lead is drawn on the all-outlier scene: poses that have nothing to do with these
    correspondences."""
    key, N = CASES[case][:2]
    sc = scene_of(case)
    cols, _ = cols_of(case)
    s_gt, c_gt, _, _ = HM.score("abs", HM.pose_record(sc.gt[:4], sc.gt[4:]), cols, THR2)
    m = (PC.scene(1.0) if key == 0.1 else sc).p3p_models(N, 2 * L + 512, 700 + N)
    m = m[~np.isnan(m).any(axis=1)]
    sc_cnt = [HM.score("abs", HM.pose_record(k[:4], k[4:]), cols, THR2)[:2] for k in m]
    far = np.array([c + LEAD_CLEAR <= c_gt and s >= s_gt + LEAD_CLEAR_SCORE * THR2 for s, c in sc_cnt])
    m = m[far][:L]
    assert len(m) == L
    return m


@functools.lru_cache(maxsize=None)
def pool(case):
    """{"init", "cand", "kinds": {kind: indices into cand}, "r2", "inl", "surv": (cand, N) host survivor flags, "cstar"}"""
    key, N, want_cstar, need = CASES[case]
    sc = scene_of(case)
    cols, xy = cols_of(case)
    sizes = [1e-7] * 4 + list(np.geomspace(2e-4, 6e-3, 72))
    cand = np.array([sc.gt] + [PC.perturbed_gt(sc, s, 40 + i) for i, s in enumerate(sizes)])
    r2, inl, live = PC.reference(sc, N, cand)
    assert live.all()
    c = inl.sum(axis=1)
    s = np.where(inl, r2, 0.0).sum(axis=1) + (N - c) * THR2
    init_max, init_min = int(c[0]) + SLACK_COUNT, float(s[0]) + SLACK_SCORE * THR2
    beat = init_min * (1.0 + PC.MARGIN_SCORE)
    S = []
    for route in (SINGLE, GROUP):
        cp = PC.chunk_points(N, route)
        chunks = (N + cp - 1) // cp
        cstar = PC.split_chunk(init_max, init_min, N, THR2, cp, chunks)
        assert cstar == want_cstar < chunks, (case, route, cstar, chunks)
        S.append(min(cstar * cp, N))
    surv = np.zeros((len(cand), N), bool)
    kinds = {KEEP: [], LATE: [], EARLY: [], FAR: []}
    for k in range(len(cand)):
        rec = HM.pose_record(cand[k][:4], cand[k][4:])
        en, flt = HM.prefilter16_abs(rec, list(cols), THR2, xy, 0)
        assert en and not (inl[k] & flt).any()
        surv[k] = ~flt
        if not all((Sr - inl[k, :Sr].sum()) * THR2 <= init_min for Sr in S):
            continue  # (the pre-selection might drop it: not a planted model)
        if s[k] <= init_min:
            kinds[KEEP].append(k)
            continue
        cs = int(surv[k].sum())
        if cs + MARGIN_SURV <= init_max and (N - cs - MARGIN_SURV) * THR2 > beat:
            kinds[FAR].append(k)
            continue
        if not (N - cs + MARGIN_SURV) * THR2 <= init_min:
            continue  # (stage S might drop it, or not)
        en0, _, maybe0, q0 = HB.bound(rec, cols, THR2, xy, residual=False)
        en1, _, maybe1, q1 = HB.bound(rec, cols, THR2, xy, residual=True)
        assert en0 and en1
        out0 = int((~maybe0).sum())
        if int(maybe0.sum()) + MARGIN_PAIRS <= init_max and (out0 - MARGIN_PAIRS) * THR2 > beat:
            kinds[EARLY].append(k)
        elif ((out0 + MARGIN_PAIRS) * THR2 <= init_min and int(maybe1.sum()) + MARGIN_PAIRS <= init_max
              and (float(q1.astype(np.int64).sum()) / HB.SCALE - MARGIN_PAIRS) * THR2 > beat):
            kinds[LATE].append(k)
    print(f"{case}: incumbent ({init_max}, {init_min / THR2:.2f} thr^2), c* {want_cstar}, S {S}, "
          + ", ".join(f"{n} {len(kinds[k])}" for n, k in (("keep", KEEP), ("late", LATE), ("early", EARLY), ("far", FAR)))
          + f" of {len(cand)} perturbed ground truths")
    for kind, least in need.items():
        assert len(kinds[kind]) >= least, (case, kind, len(kinds[kind]), least)
    return {"init": (init_max, init_min), "cand": cand, "kinds": kinds, "r2": r2, "inl": inl, "surv": surv, "cstar": want_cstar}


def planted(case, kinds_behind):
    """(models, the planted models' indices into the pool, kinds (H,) with -1 in the lead); a kind the case's pool does not hold
    (far where c* = chunks - 1, possibly early) is replaced by late"""
    P = pool(case)
    kinds_behind = [kind if P["kinds"][kind] else LATE for kind in kinds_behind]
    idx = np.array([P["kinds"][kind][i % len(P["kinds"][kind])] for i, kind in enumerate(kinds_behind)], dtype=np.int64)
    return np.concatenate([lead_of(case), P["cand"][idx]]), idx, np.r_[np.full(L, -1), np.asarray(kinds_behind, dtype=np.int64)]


def _long():
    k = np.full(1100, FAR)
    k[0:64:3] = EARLY             # first unit: stage S leaves a third of it
    k[64 + 63] = KEEP             # second: one entry left, its last
    k[128:192] = LATE             # third: stage S leaves all 64, the verdict too
    k[192:256:2] = KEEP           # fourth: every second one stays to the end
    k[193:256:6] = EARLY
    # units 4 .. 15 are emptied by stage S; the second round of the 16 workgroups starts at entry 1024
    k[1023], k[1024], k[1030], k[1099] = KEEP, LATE, EARLY, KEEP
    return k.tolist()


LISTS = {
    "1 far": [FAR], "1 early": [EARLY], "1 late": [LATE], "1 keep": [KEEP],
    "63 far": [FAR] * 63,
    "64 mixed": ([FAR, EARLY, FAR, LATE, FAR, KEEP, FAR, FAR] * 8),
    "65 mixed": ([KEEP, FAR, LATE, EARLY, FAR] * 13),
    "128, emptied and full": [FAR] * 64 + [KEEP, LATE, EARLY, LATE] * 16,
    "128, full and emptied": [LATE, KEEP] * 32 + [FAR] * 64,
    "1100": _long(),
}


def test_lists_are_what_they_are_named():
    """(no device) lengths, and the units stage S empties or leaves whole"""
    for name, kinds in LISTS.items():
        assert len(kinds) == int(name.split()[0].rstrip(",")), name
    k = np.asarray(LISTS["128, emptied and full"])
    assert (k[:64] == FAR).all() and (k[64:] != FAR).all()
    k = np.asarray(LISTS["1100"])
    assert all((k[u * 64:(u + 1) * 64] == FAR).all() for u in range(4, 15)) and (k[128:192] == LATE).all()
    assert {len(v) for v in LISTS.values()} >= {1, 63, 64, 65, 1100}


def stage_s_score(N, c):
    """decide's value for q = (N - c) 2^20 quanta: thr^2 (N - c) rounded DOWN"""
    qd = float(N - c)
    s = THR2 * qd
    return float(np.nextafter(s, -np.inf)) if Fraction(s) > Fraction(THR2) * Fraction(qd) else s


# ---- device ------------------------------------------------------------------------------------------------------------------------------
_problems = {}


def _problem(gpu, case):
    key = CASES[case][:2] if case in CASES else case
    if key not in _problems:
        a, b = (scene_of(case) if case in CASES else PC.scene(key[0])).points(key[1])
        _problems[key] = gpu.Problem(gpu.KIND_ABS, a, b)
    return _problems[key]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for p in _problems.values():
        p.close()
    _problems.clear()


def _host_cells(case, idx, cp, chunks):
    """(chunks, len(idx)) survivors per cell of the host form"""
    flags = pool(case)["surv"][idx]
    pad = np.zeros((len(idx), chunks * cp), np.int64)
    pad[:, :flags.shape[1]] = flags
    return pad.reshape(len(idx), chunks, cp).sum(axis=2).T


def _check(tag, out, stream, sv, case, idx, kinds, pruned_cand):
    P = pool(case)
    N, init = CASES[case][1], P["init"]
    H = len(kinds)
    behind = kinds >= 0
    tiers, bc, bs, col = out["tiers"], out["bound_counts"], out["bound_scores"], np.asarray(out["columns"], np.int64)
    has = bc != NO_BOUND
    cstar, chunks = out["cstar"], out["chunks"]
    full_c = np.zeros(H, dtype=np.int64)
    full_s = np.full(H, np.nan)
    inl, r2 = P["inl"][idx], P["r2"][idx]
    full_c[behind] = inl.sum(axis=1)
    full_s[behind] = np.where(inl, r2, 0.0).sum(axis=1) + (N - full_c[behind]) * THR2
    colsum = col.sum(axis=0)
    beat = out["lead_min"] * (1.0 + PC.MARGIN_SCORE)
    by_s = has & (tiers == 2) & (bc == colsum) & (bs == np.array([stage_s_score(N, min(int(c), N)) for c in colsum]))
    print(tag, "c*", cstar, "of", chunks, "behind the lead", int(behind.sum()), "dropped by the tier", int((tiers == 2).sum()),
          "of them with stage S's bounds", int(by_s.sum()), "exact launch scored", out["num_preselected"])
    assert out["num_live"] == H and (tiers != 3).all(), tag
    assert out["lead_max"] == init[0] and out["lead_min"] == init[1], (tag, "the lead beats the incumbent", out["lead_max"], out["lead_min"])
    assert cstar == P["cstar"] and col.shape == (chunks, H), (tag, cstar, col.shape)
    assert (tiers[~behind] == 0).all(), (tag, "a lead position without exact scores")
    assert (has == behind).all() and not (tiers == 1).any(), (tag, "the entries behind the lead are not the planted ones")
    assert np.isnan(bs[~has]).all() and not np.isnan(bs[has]).any(), tag
    # general properties: bounds on the right side of the reference, the decision is the rule on the reported bounds
    assert (bc[has].astype(np.int64) >= full_c[has]).all(), (tag, np.flatnonzero(has & (bc < full_c))[:5])
    assert (bs[has] <= full_s[has]).all(), (tag, np.flatnonzero(has & ~(bs <= full_s))[:5])
    rule = (bc[has] <= out["lead_max"]) & (bs[has] > beat)
    assert ((tiers[has] == 2) == rule).all(), (tag, "the decision is not the rule on the reported bounds")
    # the columns of what the tier dropped: survivor words of EVERY chunk, pl_debug_score_survivors' word for word
    gone = tiers == 2
    assert (col[:, gone] == np.asarray(sv, np.int64)[:, gone]).all(), (tag, "a survivor word differs from the count launch's",
                                                                      np.argwhere(col[:, gone] != np.asarray(sv, np.int64)[:, gone])[:5])
    # ... and the host form's within MAX_PAIRS in MAX_CELLS cells (of the list's distinct models)
    cp = out["chunk_points"]
    host = _host_cells(case, idx, cp, chunks)
    diff = np.abs(col[:, behind] - host) * gone[behind][None, :]
    assert (diff <= MAX_PAIRS).all(), (tag, "device against host form", np.argwhere(diff > MAX_PAIRS)[:5])
    cells = {(int(ch), int(idx[e])) for ch, e in np.argwhere(diff > 0)}
    assert len(cells) <= MAX_CELLS, (tag, len(cells), "cells differ", sorted(cells)[:8])
    # stage S: what it dropped reports the column's sum and decide's value of (N - c) 2^20 quanta
    far, early, late, keep = (kinds == k for k in (FAR, EARLY, LATE, KEEP))
    assert by_s[far].all(), (tag, "a far entry without stage S's bounds", np.flatnonzero(far & ~by_s)[:5], bc[far][:3], colsum[far][:3])
    assert (tiers[far] == 2).all() and (tiers[early] == 2).all() and (tiers[late] == 2).all(), (tag, "a stage kept what it drops")
    assert (tiers[keep] == 0).all(), (tag, "a model that cannot be dropped was")
    # ... and what it left was seen by a later stage: on its column's sum the rule does not hold
    later = early | late
    s_of_col = np.array([stage_s_score(N, min(int(c), N)) for c in colsum])
    assert not ((colsum[later] <= out["lead_max"]) & (s_of_col[later] > beat)).any(), (tag, "stage S should have dropped these")
    assert not by_s[later].any(), (tag, "an entry stage S left reports stage S's bounds")
    assert out["num_preselected"] == keep.sum(), (tag, "the exact launch's list")
    assert (out["kept"] == (tiers == 0)).all(), tag
    kept = tiers == 0
    cnt, sc = out["counts"], out["scores"]
    assert (cnt[kept] == stream[0][kept]).all(), (tag, "exact counts differ from the plain scorer's")
    assert (col[:, kept].sum(axis=0) == cnt[kept]).all(), (tag, "a kept column does not hold the exact partial counts")
    assert (np.abs(sc[kept] - stream[1][kept]) <= TB.reorder_tol(cnt[kept], stream[1][kept])).all(), (tag, "exact scores")
    assert (cnt[~kept] == 0).all() and (sc[~kept] == N * THR2).all(), tag
    want = PC.records_rule(stream[0], stream[1], *init)
    got = sorted(out["cand"].tolist())
    assert out["num_cand"] == len(out["cand"]) and got == want, (tag, got[:8], want[:8])
    assert got == pruned_cand, (tag, "pl_debug_score_pruned lists other candidates")


def _bitwise(tag, a, b):
    TB.bitwise(tag, a, b)
    gone = a["tiers"] == 2
    assert a["columns"][:, gone].tobytes() == b["columns"][:, gone].tobytes(), (tag, "columns")


def _run(gpu, case, name, twice=False):
    models, idx, kinds = planted(case, LISTS[name])
    init = pool(case)["init"]
    p = _problem(gpu, case)
    member = (p, models, PC.THR, init[0], init[1])
    outs = {}
    for route in (SINGLE, GROUP):
        stream = TB._stream(gpu, p, models, route)
        (out,), idle, guard = gpu.score_bounded([member], route, columns=True)
        assert idle == 0 and guard == 0, (case, name, route, idle, guard)
        (sv,), idle, guard = gpu.score_survivors([member[:3]], route)
        assert idle == 0 and guard == 0
        (pr,), idle = gpu.score_pruned([member], route)
        assert idle == 0
        _check((case, name, route), out, stream, sv["survivors"], case, idx, kinds, sorted(pr["cand"].tolist()))
        if twice:
            (again,), _, _ = gpu.score_bounded([member], route, columns=True)
            _bitwise((case, name, route, "twice"), out, again)
        outs[route] = out
    N = CASES[case][1]
    assert PC.chunk_points(N, SINGLE) == PC.chunk_points(N, GROUP)
    _bitwise((case, name, "routes"), outs[SINGLE], outs[GROUP])
    TB._same((case, name), outs[SINGLE], outs[GROUP], True)
    return outs


@pytest.mark.parametrize("name", list(LISTS))
def test_cstar_one(gpu, name):
    """c* = 1 of 5 chunks, the last with one row: the new launch counts four chunks, stage S drops what is far"""
    _run(gpu, "one", name, twice=name in ("65 mixed", "1100"))


@pytest.mark.parametrize("name", ["1 late", "1 keep", "65 mixed", "128, full and emptied"])
def test_cstar_is_the_last_chunk(gpu, name):
    """c* = chunks - 1: the new launch has the partial last chunk - one row, 319 behind the end - alone"""
    outs = _run(gpu, "last", name, twice=name == "65 mixed")
    for out in outs.values():
        assert out["cstar"] == out["chunks"] - 1 == 4


@pytest.mark.parametrize("N", [5120, 5121])
def test_sixteen_and_seventeen_chunks(gpu, N):
    """16 full chunks / 17 with one row in the last, c* = 12: the wavefronts walk two chunks each (wavefront 0 a third)"""
    outs = _run(gpu, N, "65 mixed", twice=True)
    for out in outs.values():
        assert out["chunk_points"] == 320 and out["chunks"] == (16 if N == 5120 else 17)
    _run(gpu, N, "128, emptied and full")


def _idle_member(gpu):
    """all outliers, no incumbent: the lead's best count is a handful, so c* = chunks"""
    models = TP.list_of(1.0, 1281, TP.LENGTHS[-1])[0]
    return (_problem(gpu, (1.0, 1281)), models, PC.THR, 0, PC.DBL_MAX)


def _check_idle(tag, out, stream):
    assert out["cstar"] == out["chunks"], (tag, "the lead places c* in front of the end")
    live = out["tiers"] != 3
    assert (out["bound_counts"] == NO_BOUND).all() and (out["tiers"][live] == 0).all(), (tag, "the tier is not idle")
    assert (out["counts"] == stream[0]).all(), tag
    # every column holds the exact launch's partial counts: nothing of the count launches is left
    assert (np.asarray(out["columns"], np.int64).sum(axis=0) == out["counts"]).all(), tag


def test_cstar_is_chunks_everything_idle(gpu):
    member = _idle_member(gpu)
    for route in (SINGLE, GROUP):
        (out,), idle, guard = gpu.score_bounded([member], route, columns=True)
        assert idle == 0 and guard == 0, (route, idle, guard, "words behind the list's end or in the idle slot changed")
        _check_idle(("all", route), out, TB._stream(gpu, member[0], member[1], route))


def test_group_whose_members_differ_in_points_and_cstar(gpu):
    """c* = 1 of 5, 12 of 17, chunks of 5 (idle) and 4 of 5 in one group launch: each member equals the same member alone, bit for
    bit; the inactive slot and the guard words unchanged"""
    members = []
    for case, name in (("one", "1100"), (5121, "65 mixed"), (None, None), ("last", "65 mixed")):
        if case is None:
            members.append(_idle_member(gpu))
        else:
            init = pool(case)["init"]
            members.append((_problem(gpu, case), planted(case, LISTS[name])[0], PC.THR, init[0], init[1]))
    outs, idle, guard = gpu.score_bounded(members, GROUP, columns=True)
    assert idle == 0 and guard == 0
    assert [(o["cstar"], o["chunks"]) for o in outs] == [(1, 5), (12, 17), (5, 5), (4, 5)]
    want = np.asarray(planted("one", LISTS["1100"])[2][L:])
    assert (outs[0]["tiers"][L:] == np.where(want == KEEP, 0, 2)).all()
    for i, m in enumerate(members):
        (alone,), idle, guard = gpu.score_bounded([m], GROUP, columns=True)
        assert idle == 0 and guard == 0
        _bitwise(("among others against alone", i), outs[i], alone)
