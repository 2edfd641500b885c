"""The count launch cell by cell (-m gpu): one survivor word per (hypothesis, chunk) of pl_debug_score_survivors against the host
build of the same fp16 filter (tests/hostmath: hm_prefilter16_abs, index order), hypothesis by hypothesis and chunk by chunk.

The count launch computes its tiles transposed - hypotheses on the matrix instruction's columns, a lane's verdicts all of one
hypothesis - and tests/test_gpu_score_count.py compares totals per LIST (and per cell only survivors >= inliers), which a
permutation of the hypotheses inside a tile of 32 would pass.  Here every live hypothesis of the lists is compared in every
chunk, so a count that lands in another hypothesis' word, or a correspondence counted for the wrong chunk, shows.

Tolerance.  The device and the host form differ only in the order in which fp32 products are accumulated.  What that is worth
per cell was measured on the CPU between the host form's own four accumulation orders (random_order = 0 .. 3) on these very
lists (`PYTHONPATH=. python tests/test_gpu_score_count_lanes.py` prints it; 2081 hypotheses x 4 or 5 chunks per list, orders
1 .. 3 against order 0):

    list (10 % outliers)               cells    largest cell difference D    most differing cells K
    1024 correspondences, 4 x 256       8324    1 pair                       1
    1024 correspondences, 4 x 320       8324    1 pair                       1
    1280 correspondences, 4 x 320       8324    0                            0
    1281 correspondences, 5 x 320      10405    0                            0

D = 1 pair, K = 1 cell of a list - as the list totals of tests/test_gpu_score_count.py suggest (one or two pairs per list).

The device may differ from the index-order form by four times each (the factor of test_gpu_score_count.TIGHTNESS), at least
1 pair in at least 4 cells: MAX_PAIRS per cell in at most MAX_CELLS cells of a list.

Shapes (the smallest the kernel can go wrong at): 1024 correspondences - 8 point groups per chunk in the single launch, chunks
of 320 with a last chunk of 64 columns in a group -, 1280 (10 point groups, exact fill), 1281 (a last chunk of ONE
correspondence: 319 rows behind the chunk's end); lists of L, L + 1 and L + 33 hypotheses (partial group of 32, units of 32 / 16); one list
with NaN models inside (live positions != indices); single launches and group launches of mixed members.  The pruned step on
the same lists (pl_debug_score_pruned: the count launch starts behind the lead there, 1 and 33 positions) must list the plain
step's candidates."""
import functools

import numpy as np
import pytest

import hostmath_lib as HM
import prune_cases as PC
import test_gpu_score_prune as TP
from prune_cases import GROUP, SINGLE

pytestmark = pytest.mark.gpu

RATIO = 0.1  # most pairs survive the filter: the counts are large and differ from hypothesis to hypothesis
NS = (1024, 1280, 1281)
HOST_ORDER_PAIRS = 1   # D
HOST_ORDER_CELLS = 1   # K
MAX_PAIRS = max(1, 4 * HOST_ORDER_PAIRS)
MAX_CELLS = max(4, 4 * HOST_ORDER_CELLS)
NAN_AT = (3, 31, 32, 100, 1500, TP.L - 1, TP.L + 12)  # in the first group of 32, on its edge, in the lead, behind it


@functools.lru_cache(maxsize=None)
def host_flags(N, order=0):
    """(L + 33, N) survivor flags of the host form for the longest list of N correspondences; the short lists are its prefixes"""
    models = TP.list_of(RATIO, N, TP.LENGTHS[-1])[0]
    a, b = PC.scene(RATIO).points(N)
    cols = [a[:, 0], a[:, 1], b[:, 0], b[:, 1], b[:, 2]]
    xy = float(np.abs(a).max())
    out = np.zeros((len(models), N), bool)
    for k, m in enumerate(models):
        en, flt = HM.prefilter16_abs(HM.pose_record(m[:4], m[4:]), cols, PC.THR ** 2, xy, order)
        assert en
        out[k] = ~flt
    out.setflags(write=False)
    return out


def host_cells(N, route, order=0):
    """(chunks, L + 33) survivors per (chunk, hypothesis) of the host form"""
    flags = host_flags(N, order)
    cp = PC.chunk_points(N, route)
    chunks = (N + cp - 1) // cp
    pad = np.zeros((flags.shape[0], chunks * cp), np.int64)
    pad[:, :N] = flags
    return pad.reshape(flags.shape[0], chunks, cp).sum(axis=2).T


@functools.lru_cache(maxsize=None)
def nan_list(N):
    """the longest list of N correspondences with NaN models planted: (models, reference, live flags)"""
    models, (r2, inl, live) = TP.list_of(RATIO, N, TP.LENGTHS[-1])
    models, r2, inl, live = models.copy(), r2.copy(), inl.copy(), live.copy()
    for i, k in enumerate(NAN_AT):
        models[k] = PC.nan_model(models[k], i)
    r2[list(NAN_AT)], inl[list(NAN_AT)], live[list(NAN_AT)] = np.inf, False, False
    return models, (r2, inl, live)


def _compare(tag, out, want, live):
    sv = np.asarray(out["survivors"], np.int64)
    assert sv.shape == want.shape, (tag, sv.shape, want.shape)
    assert out["num_live"] == live.sum(), tag
    assert (sv[:, ~live] == 0).all(), tag
    diff = np.abs(sv - want)[:, live]
    cells = int((diff > 0).sum())
    print(tag, "cells", diff.size, "differing", cells, "largest difference", int(diff.max()), "survivors", int(sv.sum()))
    worst = np.argwhere(np.abs(sv - want) * live[None, :] > MAX_PAIRS)
    assert len(worst) == 0, (tag, "device against host form at (chunk, hypothesis)", worst[:5], sv[tuple(worst[0])], want[tuple(worst[0])])
    assert cells <= MAX_CELLS, (tag, cells, "cells differ", np.argwhere((np.abs(sv - want) > 0) & live[None, :])[:8])


def _member(gpu, N, H, nan=False):
    """((problem, models, threshold), live flags)"""
    if nan:
        models, (_, _, live) = nan_list(N)
    else:
        models, (_, _, live) = TP.list_of(RATIO, N, H)
    return (TP._problem(gpu, RATIO, N), models, PC.THR), live


@pytest.mark.parametrize("N", NS)
def test_single_launch_cell_by_cell(gpu, N):
    for H in TP.LENGTHS:
        m, live = _member(gpu, N, H)
        (out,), idle, guard = gpu.score_survivors([m], SINGLE)
        assert idle == 0 and guard == 0, (N, H, idle, guard)
        _compare(("single", N, H), out, host_cells(N, SINGLE)[:, :H], live)
    m, live = _member(gpu, N, 0, nan=True)
    (out,), idle, guard = gpu.score_survivors([m], SINGLE)
    assert idle == 0 and guard == 0, (N, "nan", idle, guard)
    _compare(("single", N, "nan"), out, host_cells(N, SINGLE) * live[None, :], live)


@pytest.mark.parametrize("turn", range(3))
def test_group_launch_of_mixed_members_cell_by_cell(gpu, turn):
    """three point counts with three different list lengths and a list with NaN models as the four members of one launch; over
    the three turns every point count meets every length"""
    cases = [(N, TP.LENGTHS[(turn + j) % 3]) for j, N in enumerate(NS)]
    members = [_member(gpu, N, H) for N, H in cases] + [_member(gpu, NS[turn], 0, nan=True)]
    outs, idle, guard = gpu.score_survivors([m for m, _ in members], GROUP)
    assert idle == 0, f"the launch changed {idle} words of the inactive slot's buffers"
    assert guard == 0, f"the launch changed {guard} words behind the live lists' ends"
    for (N, H), (_, live), out in zip(cases, members, outs):
        _compare(("group", N, H), out, host_cells(N, GROUP)[:, :H], live)
    live = members[3][1]
    _compare(("group", NS[turn], "nan"), outs[3], host_cells(NS[turn], GROUP) * live[None, :], live)


@pytest.mark.parametrize("turn", range(3))
def test_pruned_step_lists_the_plain_steps_candidates(gpu, turn):
    """the same members through pl_debug_score_pruned as one group: the count launch starts behind the lead (0, 1, 33 and 26
    positions) and what it leaves must give the candidates of the plain step (TP._check: counts, scores, kept, candidates)"""
    cases = [(N, TP.LENGTHS[(turn + j) % 3]) for j, N in enumerate(NS)]
    lists = [TP.list_of(RATIO, N, H) for N, H in cases] + [nan_list(NS[turn])]
    ns = [N for N, _ in cases] + [NS[turn]]
    members = [(TP._problem(gpu, RATIO, N), models, PC.THR, 0, PC.DBL_MAX) for N, (models, _) in zip(ns, lists)]
    outs, idle = gpu.score_pruned(members, GROUP)
    assert idle == 0, f"the launches changed {idle} words of the inactive slot's buffers"
    streams, idle = gpu.score_stream_group([(m[0], m[1], PC.THR, 0) for m in members])
    assert idle == 0
    for N, (models, ref), out, st in zip(ns, lists, outs, streams):
        TP._check(("group", N, len(models)), out, (st["counts"], st["scores"]), ref, N, GROUP, must_prune=False)


def measure_host_orders():
    """D and K of the docstring: the host form's accumulation orders against order 0, per list"""
    for N in NS:
        for route in (SINGLE, GROUP):
            base = host_cells(N, route, 0)
            D = K = 0
            for order in (1, 2, 3):
                diff = np.abs(host_cells(N, route, order) - base)
                D, K = max(D, int(diff.max())), max(K, int((diff > 0).sum()))
            print(f"N = {N}, chunks of {PC.chunk_points(N, route)}: {base.size} cells, D = {D}, K = {K}")


if __name__ == "__main__":
    measure_host_orders()
