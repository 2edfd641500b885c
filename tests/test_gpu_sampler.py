"""The device sampler position by position: k_sample_delta<K>, k_sample_orbit<SMALL> and their group forms, through
pl_debug_sample_positions - single launches and the group form, with the orbit kernel's build in the test's hand.

Integers only, exact equality everywhere.  The expectation is tests/sampler_cases.py: the draw stream and the delta table restated in
numpy, and the sequential walk over a delta table as the model of the orbit kernel - positions, the position behind the batch and
the orbit_error predicate of the build that runs.  Drawn cases are real draw streams on every path of the kernel (flags over
capacity, one-lane walk, pointer doubling, either build); planted cases are delta tables at the edges of its tables, which no draw
stream reaches.  tests/test_sampler_cases.py shows on the CPU that every case sits where its name says."""
import numpy as np
import pytest

import sampler_cases as S

pytestmark = pytest.mark.gpu

PATTERN = np.uint64(0xA5A5A5A5A5A5A5A5)
OTHER = {"small": "large", "large": "small"}


def _check(o, delta, K, B, build, pos_base=0, what=""):
    """One member's outputs against the table it walked and the model of the build that ran."""
    assert o["build"] == build and o["M"] == delta.size, what
    assert (o["delta"] == delta).all(), what
    assert (o["flagbits"] == S.bitmap(delta, K)).all(), what
    assert o["guard"].size >= 1 and (o["guard"] == PATTERN).all() and o["delta_guard"], what
    assert o["ctl_clear"], what
    w = S.walk(delta, K, B, S.caps(build))
    assert o["orbit_error"] == int(w.error), (what, w.reasons, w.F, w.visited, w.end)
    if not w.error:
        bad = np.flatnonzero(o["positions"] != w.positions)
        assert bad.size == 0, (what, bad[:8], o["positions"][bad[:8]], w.positions[bad[:8]])
        assert o["pos_after"] == pos_base + w.end, what
    return w


# ------------------------------------------------------------------ drawn, single route
@pytest.mark.parametrize("choice", ["chosen", "small", "large"])
@pytest.mark.parametrize("name", sorted(S.DRAWN))
def test_drawn(gpu, name, choice):
    N, K, B, forced, _ = S.DRAWN[name]
    sh, _, delta, _ = S.drawn(name)
    build = sh["build"] if choice == "chosen" else choice
    (o,), _ = gpu.sample_positions(K, [{"seed": S.SEED, "N": N, "B": B}], build=None if choice == "chosen" else choice)
    w = _check(o, delta, K, B, build, what=(name, choice))
    if S.path(w.F, S.caps(build)) == "overflow":
        assert o["orbit_error"] == 1


@pytest.mark.parametrize("M", [200, 1000 + 37, 5 * 256 + 64 + 1, 4096, 4097])
def test_drawn_windows_that_end_inside_a_word_or_a_block(gpu, M):
    """k_sample_delta writes one bitmap word per wavefront and returns per block of 256: windows that end inside either, one below
    256 positions (where the walk can only report the window as too short), exact multiples and one more."""
    K, N, B = 5, 300, 60
    delta = S.delta_table(77, 1000, N, K, M)
    for build in S.BUILDS:
        (o,), _ = gpu.sample_positions(K, [{"seed": 77, "pos_base": 1000, "N": N, "B": B, "M": M}], build=build)
        w = _check(o, delta, K, B, build, pos_base=1000, what=(M, build))
        assert w.reasons == (("window",) if M == 200 else ())


@pytest.mark.parametrize("K", S.KS)
def test_drawn_from_the_middle_of_an_iteration_and_from_the_last_window_the_driver_accepts(gpu, K):
    N, B = 300, 2000
    M = S.shape(K, N, B)["window"]
    ref = S.walk(S.delta_table(S.SEED, 0, N, K, 4000), K, 100, S.caps("large"))
    mid = int(ref.positions[50]) + 1
    assert mid not in ref.positions.tolist()
    for pos_base in (mid, 2 ** 32 - 2 - M):
        delta = S.delta_table(S.SEED, pos_base, N, K, M)
        (o,), _ = gpu.sample_positions(K, [{"seed": S.SEED, "pos_base": pos_base, "N": N, "B": B}])
        w = _check(o, delta, K, B, S.shape(K, N, B)["build"], pos_base=pos_base, what=(K, pos_base))
        assert not w.error and w.visited > 0


# ------------------------------------------------------------------ planted, both builds
PLANTED = [(K, build, p) for K in S.KS for build in S.BUILDS for p in S.planted_cases(K, build)]


@pytest.mark.parametrize("K,build,p", PLANTED, ids=[f"{p.name}-K{K}-{build}" for K, build, p in PLANTED])
def test_planted(gpu, K, build, p):
    (o,), _ = gpu.sample_positions(K, [{"N": 1000, "B": p.B, "planted": p.delta, "pos_base": 4242}], build=build)
    w = _check(o, p.delta, K, p.B, build, pos_base=4242, what=p.name)
    assert (w.F, w.visited, w.error) == (p.F, p.visited, p.error)
    if not p.error:
        assert o["pos_after"] == 4242 + p.end


@pytest.mark.parametrize("K", S.KS)
def test_the_two_walks_agree_on_one_table(gpu, K):
    """The table at the doubling limit takes pointer doubling, the same table with one more flag that no iteration starts at takes the
    one-lane walk: the positions are the same."""
    by = {p.name: p for p in S.planted_cases(K, "large")}
    a, b = by["flags_at_doubling_limit"], by["flags_over_doubling_limit"]
    (oa,), _ = gpu.sample_positions(K, [{"N": 1000, "B": a.B, "planted": a.delta}], build="large")
    (ob,), _ = gpu.sample_positions(K, [{"N": 1000, "B": b.B, "planted": b.delta}], build="large")
    assert oa["orbit_error"] == ob["orbit_error"] == 0
    assert (oa["positions"] == ob["positions"]).all() and oa["pos_after"] == ob["pos_after"]


RANDOM = [(K, build, i) for K in S.KS for build in S.BUILDS for i in range(9)]


@pytest.mark.parametrize("K,build,i", RANDOM)
def test_random_tables(gpu, K, build, i):
    name, B, delta = S.random_tables(K, build)[i]
    (o,), _ = gpu.sample_positions(K, [{"N": 1000, "B": B, "planted": delta}], build=build)
    w = _check(o, delta, K, B, build, what=name)
    assert not w.error


# ------------------------------------------------------------------ group route
GROUPS = {
    # a window below 256 positions, a member whose flags overflow the tables, two that succeed; min N = 8 -> the large build
    "mixed": [{"seed": 1, "pos_base": 0, "N": 2000, "B": 1024}, {"seed": 2, "pos_base": 777, "N": 300, "B": 8, "M": 200},
              {"seed": 3, "pos_base": 5, "N": 8, "B": 64}, {"seed": 4, "pos_base": 123456, "N": 500, "B": 3000}],
    # few flags expected in the largest window of the smallest member -> the small build
    "sparse": [{"seed": 5, "pos_base": 9, "N": 2000, "B": 1024}, {"seed": 6, "pos_base": 0, "N": 5000, "B": 2048, "M": 20000 + 13},
               {"seed": 7, "pos_base": 31, "N": 2500, "B": 3, "M": 100}],
}


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_group_of_drawn_members(gpu, name):
    K = 7
    members = GROUPS[name]
    windows = [m.get("M") or S.shape(K, m["N"], m["B"])["window"] for m in members]
    build = S.shape(K, min(m["N"] for m in members), 1, max(windows))["build"]
    assert build == {"mixed": "large", "sparse": "small"}[name]
    outs, idle = gpu.sample_positions(K, members, group=True)
    assert idle == 0
    errors = []
    for m, M, o in zip(members, windows, outs):
        delta = S.delta_table(m["seed"], m["pos_base"], m["N"], K, M)
        w = _check(o, delta, K, m["B"], build, pos_base=m["pos_base"], what=(name, m))
        errors.append(w.reasons)
        (single,), _ = gpu.sample_positions(K, [m], build=build)  # the single route under the group's build: bit for bit
        for key in ("positions", "delta", "flagbits", "guard"):
            assert (o[key] == single[key]).all(), (name, m, key)
        for key in ("pos_after", "orbit_error", "M", "build", "delta_guard", "ctl_clear"):
            assert o[key] == single[key], (name, m, key)
    if name == "mixed":  # the members that fail fail alone, each for its own reason
        assert errors == [(), ("window",), ("flags",), ()]
    else:
        assert errors == [(), (), ("window",)]


@pytest.mark.parametrize("build", S.BUILDS)
def test_group_of_planted_members(gpu, build):
    K = 7
    by = {p.name: p for p in S.planted_cases(K, build)}
    picks = [by[n] for n in ("long_flagged_run", "flags_over_capacity", "segment_at_wave_start", "unflagged_B65")]
    members = [{"N": 1000, "B": p.B, "planted": p.delta, "pos_base": 1000 * i} for i, p in enumerate(picks)]
    outs, idle = gpu.sample_positions(K, members, build=build, group=True)
    assert idle == 0
    for i, (p, o) in enumerate(zip(picks, outs)):
        w = _check(o, p.delta, K, p.B, build, pos_base=1000 * i, what=p.name)
        assert w.error == p.error
    assert [o["orbit_error"] for o in outs] == [0, 1, 0, 0]
