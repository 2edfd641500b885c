"""The count launch of the two-tier pruned scorer on the device (-m gpu): the matrix-core filter without the exact pass, one survivor
count per (hypothesis, chunk), through pl_debug_score_survivors - single launch and group form - and the two-tier step end to end
through pl_ransac_batch.

Per (hypothesis, chunk): survivors >= the oracle's inliers of the chunk and <= the chunk's correspondences; both routes agree; the
words behind the live list's end and the inactive group slot are untouched.  Tightness: the device's total per list against the host
build of the same fp16 form in index order (tests/hostmath); the two differ only by the order in which fp32 products are
accumulated, and how much that matters is measured on the host form itself - see TIGHTNESS below.

Shapes (tests/prune_cases.py's lists): 1024 correspondences (8 point groups per chunk, exact fill), 1280 (10, exact fill), 1281 (a
last chunk of one correspondence), 2600 (nine chunks); lists of L, L + 1 and L + 33 hypotheses (a partial group of 32, a unit of 32
or 16), and the long lists, which go beyond two ticket rounds of the group form's wavefronts."""
import functools

import numpy as np
import pytest

import hostmath_lib as HM
import prune_cases as PC
import test_gpu_score_prune as TP
from poselib_amd import api
from prune_cases import GROUP, SINGLE

pytestmark = pytest.mark.gpu

# Measured on the CPU (host_totals with random_order = 0, 1, 2, 3 on the hypotheses that are compared - `compared` below: every live
# one of the 27 short lists, the sample and tail of the two long ones): the accumulation orders of the host form give the same total
# on 22 of the 29 lists and differ by one or two pairs on the others; (max - min) / min over the four orders is at most 1.34e-6 of a
# list's total (748405 against 748406 survivors at 1024 correspondences and 10 % outliers; 2114008 .. 2114010 at 2600; the 12 L
# list's subset: 2303918 against 2303919, 4.3e-7; whole long lists: 11401209 .. 11401212 and no difference).  The device may differ
# from the index-order form by four times that share, 5.4e-6 of the list's total: on a list of fewer than 186 000 compared
# survivors not at all.
HOST_ORDER_SHARE = 1.34e-6
TIGHTNESS = 4 * HOST_ORDER_SHARE


# The host form costs 0.8 ms a model at 1281 correspondences and 1.9 ms at 2600.  Every live hypothesis of the short lists is compared.
# Deviation for the two long lists (24 s and 11 s of host arithmetic otherwise): every LONG_STRIDE-th hypothesis, and EVERY one of the
# last LONG_TAIL[list] live ones - the whole last ticket round of the group launch, where unit_of_ticket cuts units of 32 or 16 and
# the partial last unit sits (asserted below from the launch's slice count), and at least 16 units of 64.  The single launch has
# more wavefronts per chunk than these lists have units, so there the whole list is one cut-up round: sampled in front of that tail.
LONG_STRIDE = 16
LONG_TAIL = {TP.LONG[0]: 3584, TP.LONG[1]: 1024}


def compared(ratio, N, H):
    """flags of the hypotheses whose survivors enter the totals"""
    live = TP.list_of(ratio, N, H)[1][2]
    if (ratio, N, H) not in TP.LONG:
        return live.copy()
    pos = np.cumsum(live) - 1
    return live & ((np.arange(H) % LONG_STRIDE == 0) | (pos >= live.sum() - LONG_TAIL[ratio, N, H]))


@functools.lru_cache(maxsize=None)
def _host_survivors(ratio, N, H, order):
    """survivors per compared hypothesis of the list under the host build of the fp16 form, 0 for the others"""
    models = TP.list_of(ratio, N, H)[0]
    a, b = PC.scene(ratio).points(N)
    cols = [a[:, 0], a[:, 1], b[:, 0], b[:, 1], b[:, 2]]
    xy = float(np.abs(a).max())
    out = np.zeros(len(models), np.int64)
    for k in np.flatnonzero(compared(ratio, N, H)):
        en, flt = HM.prefilter16_abs(HM.pose_record(models[k][:4], models[k][4:]), cols, PC.THR ** 2, xy, order)
        assert en
        out[k] = int((~flt).sum())
    return out


def host_survivors(ratio, N, H, order=0):
    """the short lists are prefixes of the longest one, computed once"""
    if (ratio, N, H) in TP.LONG:
        return _host_survivors(ratio, N, H, order)
    return _host_survivors(ratio, N, TP.LENGTHS[-1], order)[:H]


def host_totals(ratio, N, H, order=0):
    return int(host_survivors(ratio, N, H, order).sum())


def _chunk_inliers(inl, cp, chunks):
    H, N = inl.shape
    pad = np.zeros((H, chunks * cp), bool)
    pad[:, :N] = inl
    return pad.reshape(H, chunks, cp).sum(axis=2).T  # (chunks, H)


def _check(tag, out, ref, N, route, ratio, H):
    _, inl, live = ref
    cp = PC.chunk_points(N, route)
    chunks = (N + cp - 1) // cp
    sv = np.asarray(out["survivors"], np.int64)
    assert out["chunks"] == chunks and out["chunk_points"] == cp and sv.shape == (chunks, len(live)), tag
    assert out["num_live"] == live.sum(), tag
    want = _chunk_inliers(inl & live[:, None], cp, chunks)
    short = np.argwhere(sv < want)
    assert len(short) == 0, (tag, "fewer survivors than inliers at (chunk, hypothesis)", short[:5])
    valid = np.minimum(cp, np.maximum(0, N - cp * np.arange(chunks)))
    assert (sv <= valid[:, None]).all(), tag
    assert (sv[:, ~live] == 0).all(), tag
    host, total = host_totals(ratio, N, H), int(sv[:, compared(ratio, N, H)].sum())
    print(tag, "survivors", total, "host form", host, "inliers", int(want.sum()), "pairs", int(live.sum()) * N)
    assert abs(total - host) <= TIGHTNESS * host, (tag, total, host)


SHORT = sorted({(r, N) for r, N, H in TP.CASES if (r, N, H) not in TP.LONG})


def _both_routes(gpu, cases):
    """single launches list by list; the same lists as the members of one group launch; both agree word for word"""
    single = {}
    for r, N, H in cases:
        models, ref = TP.list_of(r, N, H)
        (out,), idle, guard = gpu.score_survivors([(TP._problem(gpu, r, N), models, PC.THR)], SINGLE)
        assert idle == 0 and guard == 0, (r, N, H, idle, guard)
        _check(("single", r, N, H), out, ref, N, SINGLE, r, H)
        single[r, N, H] = out["survivors"]
    members = [(TP._problem(gpu, r, N), TP.list_of(r, N, H)[0], PC.THR) for r, N, H in cases]
    outs, idle, guard = gpu.score_survivors(members, GROUP)
    assert idle == 0, f"the launch changed {idle} words of the inactive slot's buffers"
    assert guard == 0, f"the launch changed {guard} words behind the live lists' ends"
    for (r, N, H), out in zip(cases, outs):
        _check(("group", r, N, H), out, TP.list_of(r, N, H)[1], N, GROUP, r, H)
        if PC.chunk_points(N, SINGLE) == PC.chunk_points(N, GROUP):
            assert (out["survivors"] == single[r, N, H]).all(), ("single and group route differ", r, N, H)
        else:  # (1024 correspondences: chunks of 256 in the single launch, of 320 in a group) totals per hypothesis
            assert (out["survivors"].sum(axis=0) == single[r, N, H].sum(axis=0)).all(), ("single and group route differ", r, N, H)
    return outs


@pytest.mark.parametrize("ratio,N", SHORT)
def test_survivor_counts(gpu, ratio, N):
    """the three list lengths of a point count: one by one, and as the members of one group launch"""
    _both_routes(gpu, [(ratio, N, H) for H in TP.LENGTHS])


@pytest.mark.parametrize("case", TP.LONG)
def test_survivor_counts_of_a_long_list(gpu, case):
    (out,) = _both_routes(gpu, [case])
    # more than two ticket rounds of the group launch's wavefronts; its last, partial round lies inside the fully compared tail
    units, waves = (out["num_live"] + 63) // 64, 8 * out["slices"]
    assert units > 2 * waves, (out["num_live"], out["slices"])
    assert out["num_live"] - (units // waves) * waves * 64 <= LONG_TAIL[case], (out["num_live"], out["slices"])


def test_batch_call_equals_the_single_runs_bit_for_bit(gpu):
    """the two-tier steps of a group (the gate's shapes of tests/test_gpu_score_prune.py) against pl_ransac_run's plain steps; and two
    more members on the matrix cores whose steps stay below the gate: in a launch sequence with pruning members they are scored
    by the exact launch alone, without a selection"""
    runs = TP._runs()
    x, X, _ = runs[0]
    assert not api.score_prune_gate(0, len(x), TP.GATE // 2) and api.score_prune_gate(0, len(x), TP.GATE)
    runs += [(x, X, TP._opt(80 + i, max_iterations=it, min_iterations=it)) for i, it in enumerate((TP.GATE // 2, TP.GATE // 2 + 100))]
    probs = [gpu.Problem(gpu.KIND_ABS, x, X) for x, X, _ in runs]
    want = [p.run(opt) for p, (_, _, opt) in zip(probs, runs)]
    got = gpu.ransac_batch(probs, [opt for _, _, opt in runs], 2, len(runs))
    for i, ((m, info), (wm, winfo)) in enumerate(zip(got, want)):
        for key in TP.KEYS:
            assert info[key] == winfo[key], (i, key, info[key], winfo[key])
        assert info["inliers"] == winfo["inliers"], i
        assert (np.r_[m.q, m.t] == np.r_[wm.q, wm.t]).all(), i
    for p in probs:
        p.close()
