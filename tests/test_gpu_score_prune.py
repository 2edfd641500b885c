"""The pruned form of the matrix-core absolute-pose scorer on the device (-m gpu): lead, split chunk, phase A, selection, phase B and
the finalize, through pl_debug_score_pruned - single launches and group form - and end to end through pl_ransac_batch on shapes that
pass the gate of a group's batch steps, against pl_ransac_run (whose own steps keep the plain launch) and the oracle.

Kept hypotheses carry the oracle's count exactly and its score to 1e-9; pruned ones a count no greater and a score no less; the
candidate list equals the one the records rule gives on pl_debug_score_stream(_ex)'s values of the same list; the inactive slot of the
group form is untouched; and the device prunes at least what the numpy model (tests/prune_cases.py) prunes with a doubled margin -
tests/test_score_prune_rule.py checks on the CPU that this is most of the lists.

Point counts: the matrix-core scorer starts at 1024 correspondences, which are four chunks already, so there is no two-chunk case;
the counts are the smallest exact fills of both launch shapes (1024 = 4 x 256, 1280 = 4 x 320), 1281 (an exact fill plus one
correspondence: a last chunk of one) and 2600 (nine chunks, c* in the middle at 70 % outliers).  A third ticket round of phase B
needs more than 2 x 64 x wavefronts-per-chunk kept hypotheses: the group form's slice rule reaches it with the long lists, the single
launch (816 wavefronts per chunk) cannot at a test's size."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import prune_cases as PC
from poselib_amd import api, synth
from prune_cases import GROUP, SINGLE

pytestmark = pytest.mark.gpu

REL = 1e-9
L = PC.LEAD
LENGTHS = (L, L + 1, L + 33)  # live hypotheses
NS = PC.point_counts()
# (outlier ratio, N, list length): NaN models as the solver gives them; the lists the model prunes more than half of
LONG = ((0.1, 1281, 12 * L), (0.7, PC.N_MAX, 3 * L))


# ---- lists and their references (no device) -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def short_list(ratio, N):
    """L + 33 live P3P models of random samples, with everything the oracle says of them"""
    sc = PC.scene(ratio)
    models = sc.p3p_models(N, 2 * L, 500 + N)
    models = models[~np.isnan(models).any(axis=1)][:LENGTHS[-1]]
    assert len(models) == LENGTHS[-1]
    return models, PC.reference(sc, N, models)


@functools.lru_cache(maxsize=None)
def long_list(ratio, N, H):
    sc = PC.scene(ratio)
    models = sc.p3p_models(N, H, 900 + N)
    return models, PC.reference(sc, N, models)


def list_of(ratio, N, H):
    models, (r2, inl, live) = long_list(ratio, N, H) if (ratio, N, H) in LONG else short_list(ratio, N)
    return models[:H], (r2[:H], inl[:H], live[:H])


def model_of(ratio, N, H, route, margin=PC.MARGIN_SCORE, init=(0, PC.DBL_MAX), ref=None):
    r2, inl, live = list_of(ratio, N, H)[1] if ref is None else ref
    return PC.prune_model(r2, inl, live, PC.THR ** 2, PC.chunk_points(N, route), init[0], init[1], margin=margin)


# ---- device ------------------------------------------------------------------------------------------------------------------------------
_problems = {}


def _problem(gpu, ratio, N):
    if (ratio, N) not in _problems:
        _problems[ratio, N] = gpu.Problem(gpu.KIND_ABS, *PC.scene(ratio).points(N))
    return _problems[ratio, N]


@pytest.fixture(scope="module", autouse=True)
def _close_problems():
    yield
    for p in _problems.values():
        p.close()
    _problems.clear()


def _check(tag, out, stream, ref, N, route, init=(0, PC.DBL_MAX), must_prune=True):
    """out: a member's result of score_pruned; stream: (counts, scores) of the plain streaming scorer on the same list"""
    r2, inl, live = ref
    full = model_of(None, N, None, route, init=init, ref=ref)
    twice = model_of(None, N, None, route, margin=2 * PC.MARGIN_SCORE, init=init, ref=ref)
    kept = out["kept"]
    print(tag, "c*", out["cstar"], "of", out["chunks"], "lead_max", out["lead_max"], "lead_min / thr^2", out["lead_min"] / PC.THR ** 2,
          "live", out["num_live"], "selected", out["num_selected"], "pruned", int((~kept).sum()), "model prunes", int((~twice["kept"]).sum()))
    assert out["lead"] == L and out["chunk_points"] == PC.chunk_points(N, route) and out["chunks"] == full["chunks"], tag
    assert out["num_live"] == live.sum(), tag
    assert out["lead_max"] == full["lead_max"], tag
    assert abs(out["lead_min"] - full["lead_min"]) <= REL * abs(full["lead_min"]), tag
    assert out["cstar"] == PC.split_chunk(out["lead_max"], out["lead_min"], N, PC.THR ** 2, out["chunk_points"], out["chunks"]), tag
    assert out["num_selected"] == (0 if out["cstar"] == out["chunks"] else (kept & live).sum()), tag
    cnt, sc = np.asarray(out["counts"], np.int64), out["scores"]
    rc, rs = full["full_counts"], full["full_scores"]
    assert (cnt[kept] == rc[kept]).all(), (tag, np.flatnonzero(kept & (cnt != rc))[:5])
    assert (np.abs(sc[kept] - rs[kept]) <= REL * np.abs(rs[kept])).all(), tag
    assert (cnt[~kept] <= rc[~kept]).all() and (sc[~kept] >= rs[~kept] * (1.0 - REL)).all(), tag
    lead_k = live & (np.cumsum(live) <= L)
    assert kept[lead_k].all() and kept[~live].all(), tag
    missed = np.flatnonzero(~twice["kept"] & kept)
    assert len(missed) == 0, (tag, "kept what the model prunes with a doubled margin", missed[:5])
    if must_prune:
        assert (~kept).any(), tag
    want = PC.records_rule(stream[0], stream[1], *init)
    assert out["num_cand"] == len(out["cand"]) and sorted(out["cand"].tolist()) == want, (tag, sorted(out["cand"].tolist())[:8], want[:8])


CASES = [(ratio, N, H) for ratio in (0.1, 0.7) for N in NS for H in LENGTHS] + [(1.0, 1281, H) for H in LENGTHS] + list(LONG)


@pytest.mark.parametrize("ratio", [0.1, 0.7, 1.0])
def test_single_route(gpu, ratio):
    for r, N, H in CASES:
        if r != ratio:
            continue
        models, ref = list_of(r, N, H)
        p = _problem(gpu, r, N)
        (out,), idle = gpu.score_pruned([(p, models, PC.THR, 0, PC.DBL_MAX)], SINGLE)
        cnt, sc, path = p.score_stream(models, PC.THR)
        assert path == 2 and idle == 0
        _check(("single", r, N, H), out, (cnt, sc), ref, N, SINGLE, must_prune=(r, N, H) in LONG)
        if r == 1.0:
            assert out["cstar"] == out["chunks"] and out["kept"].all()


@pytest.mark.parametrize("ratio", [0.1, 0.7, 1.0])
def test_group_route(gpu, ratio):
    """the point counts of a ratio as the members of one launch, list length by list length; then the long list"""
    for H in LENGTHS:
        cases = [c for c in CASES if c[0] == ratio and c[2] == H]
        members = [(_problem(gpu, r, N), list_of(r, N, H)[0], PC.THR, 0, PC.DBL_MAX) for r, N, _ in cases]
        outs, idle = gpu.score_pruned(members, GROUP)
        assert idle == 0, f"the launches changed {idle} words of the inactive slot's buffers"
        streams, idle = gpu.score_stream_group([(m[0], m[1], PC.THR, 0) for m in members])
        assert idle == 0
        for (r, N, _), out, st in zip(cases, outs, streams):
            _check(("group", r, N, H), out, (st["counts"], st["scores"]), list_of(r, N, H)[1], N, GROUP, must_prune=(r, N, H) in LONG)
    for r, N, H in LONG:
        if r != ratio:
            continue
        models, ref = list_of(r, N, H)
        p = _problem(gpu, r, N)
        (out,), idle = gpu.score_pruned([(p, models, PC.THR, 0, PC.DBL_MAX)], GROUP)
        (st,), idle2 = gpu.score_stream_group([(p, models, PC.THR, 0)])
        assert idle == 0 and idle2 == 0
        _check(("group", r, N, H), out, (st["counts"], st["scores"]), ref, N, GROUP)
        # phase B's list goes beyond the first ticket round of the launch's wavefronts; at 70 % outliers beyond the second, and its
        # tail is cut into units of 32 with a partial last one
        w = 8 * ((out["slices"] + 3) // 4)  # wavefronts per chunk of phase B
        G = (out["num_selected"] + 63) // 64
        assert G > w, (G, w)
        if r == 0.7:
            assert G > 2 * w, (G, w)
            rest = G - (G // w) * w
            assert 0 < rest and 2 * rest <= w and out["num_selected"] % 32 != 0, (out["num_selected"], w)


def test_planted_lists(gpu):
    sc = PC.scene(0.7)
    N = 1281
    p = _problem(gpu, 0.7, N)
    base, (r2, inl, live) = long_list(0.7, N, 2 * L)
    cnt = inl.sum(axis=1)
    wrong = np.flatnonzero(live & (cnt < 30))
    good = PC.perturbed_gt(sc, 1e-6, 5)
    best = int(np.argmax(np.where(live & (np.cumsum(live) <= L), cnt, -1)))
    gt_score, gt_count = O.score("reproj", sc.gt, *sc.points(N), PC.THR ** 2)
    lists = {
        # a lead without a good model, the only good one behind it
        "late": (np.vstack([base[wrong[:L + 40]], good[None], base[wrong[L + 40:L + 80]]]), (0, PC.DBL_MAX)),
        # a copy of the lead's best model behind the lead: its count equals lead_max exactly
        "tie": (np.vstack([base[:L + 600], base[best][None]]), (0, PC.DBL_MAX)),
        # an incumbent better than anything in the list
        "incumbent": (base[:L + 600], (int(gt_count) + 50, 0.5 * gt_score)),
        # NaN models only
        "nan": (np.array([PC.nan_model(base[k], k) for k in range(70)]), (0, PC.DBL_MAX)),
    }
    for name, (models, init) in lists.items():
        ref = PC.reference(sc, N, models)
        for route in (SINGLE, GROUP):
            (out,), idle = gpu.score_pruned([(p, models, PC.THR, init[0], init[1])], route)
            assert idle == 0
            if route == SINGLE:
                c, s, _ = p.score_stream(models, PC.THR)
            else:
                (st,), _ = gpu.score_stream_group([(p, models, PC.THR, 0)])
                c, s = st["counts"], st["scores"]
            _check((name, route), out, (c, s), ref, N, route, init=init, must_prune=name in ("tie", "incumbent"))
            if name == "late":
                assert out["cstar"] == out["chunks"] and out["kept"][L + 40] and L + 40 in out["cand"].tolist()
            if name == "tie":
                assert out["counts"][-1] == out["lead_max"] and out["kept"][-1]
            if name == "incumbent":
                # (the good models behind the lead stay: in front of c* they cannot be told from one that beats the incumbent's count)
                assert out["num_cand"] == 0 and (~out["kept"]).sum() > 0.9 * (ref[2] & (np.cumsum(ref[2]) > L)).sum()
            if name == "nan":
                assert out["num_live"] == 0 and out["num_selected"] == 0 and out["cstar"] == out["chunks"]


# ---- end to end: batch steps that pass the gate ----------------------------------------------------------------------------------------
KEYS = ("iterations", "refinements", "hypotheses", "nan_hypotheses", "num_inliers", "model_score", "inlier_ratio")
GATE = 8192


def _opt(seed, **ransac):
    return {"max_error": PC.THR, "ransac": dict(ransac, seed=seed)}


def _runs():
    """(points, options): N about 1100 (scored on the matrix cores: as members of a group their steps prune; pl_ransac_run's own
    steps never do) and about 700 (no step does), fixed lengths of the gate's threshold and twice it; and default options with a large
    min_iterations on a 90 % outlier scene, where the stop rule asks for more batches behind the first - steps with an incumbent.
    The batch call below therefore compares pruned steps with the plain ones of the single runs bit for bit, and the single runs
    with the oracle."""
    out = []
    for n, seed in ((1100, 6100), (700, 6101)):
        d = synth.absolute_pose_scene(n, 0.7, seed)
        x, X = (np.asarray(d["p2d"]) - 500.0) / PC.FOCAL, np.asarray(d["p3d"], float)
        for it in (GATE, 2 * GATE):
            out.append((x, X, _opt(60 + len(out), max_iterations=it, min_iterations=it)))
    d = synth.absolute_pose_scene(1100, 0.9, 6102)
    x, X = (np.asarray(d["p2d"]) - 500.0) / PC.FOCAL, np.asarray(d["p3d"], float)
    out.append((x, X, _opt(70, min_iterations=GATE + 8)))
    return out


@pytest.fixture(scope="module")
def single_runs(gpu):
    out = []
    for x, X, opt in _runs():
        prob = gpu.Problem(gpu.KIND_ABS, x, X)
        out.append(prob.run(opt))
        prob.close()
    return out


def test_gate_is_passed_without_a_switch():
    assert api.score_prune_gate(0, 1100, GATE) and api.score_prune_gate(0, 1100, GATE + 9) and not api.score_prune_gate(0, 700, 2 * GATE)


@pytest.mark.parametrize("i", range(5))
def test_run_matches_the_oracle(single_runs, i):
    from test_gpu_full_size import _model_diff

    x, X, opt = _runs()[i]
    model, info = single_runs[i]
    want, mask, st = O.ransac_pnp(x, X, opt)
    print("run", i, "iterations", info["iterations"], "hypotheses", info["hypotheses"], "inliers", info["num_inliers"])
    if i == 4:
        assert info["iterations"] > 2 * GATE  # more than one batch: the later ones start from an incumbent
    for key in ("iterations", "refinements", "hypotheses", "num_inliers"):
        assert info[key] == st[key], (key, info[key], st[key])
    assert (np.array(info["inliers"]) == mask).all()
    assert _model_diff(0, model, want) <= 1e-6


def test_batch_call_equals_the_single_runs_bit_for_bit(gpu, single_runs):
    runs = _runs()
    probs = [gpu.Problem(gpu.KIND_ABS, x, X) for x, X, _ in runs]
    got = gpu.ransac_batch(probs, [opt for _, _, opt in runs], 2, len(runs))
    for i, ((m, info), (wm, winfo)) in enumerate(zip(got, single_runs)):
        for key in KEYS:
            assert info[key] == winfo[key], (i, key, info[key], winfo[key])
        assert info["inliers"] == winfo["inliers"], i
        assert (np.r_[m.q, m.t] == np.r_[wm.q, wm.t]).all(), i
    for p in probs:
        p.close()
