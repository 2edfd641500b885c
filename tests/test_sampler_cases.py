"""The cases of the device sampler's tests (tests/sampler_cases.py) on the CPU: the numpy restatement of the draw stream and of the
sequential walk agrees with the oracle, every drawn case lands on the path of the orbit kernel its name claims - judged from its
flag count against the constants pl_debug_sampler_shape returns, so a changed constant fails here and not silently on the device -
and every planted table sits on the edge it was built for.  No device."""
import numpy as np
import pytest

import oracle_lib as O
import poselib_amd
import sampler_cases as S


def _window(N, K, B):
    """The driver's window, restated: B sum N / (N - i), 5 % on top, truncated, and 8192 positions of slack."""
    return int(B * sum(N / (N - i) for i in range(K)) * 1.05) + 8192


def test_shape_entry():
    sh = S.shape(7, 1000, 1)
    small, large = sh["small"], sh["large"]
    for c in (small, large):  # what the kernel's own layout needs of its constants
        assert 0 < c["doubling"] <= c["flags"] < 0xffff  # (flag_next: 16 bits, 0xffff = none)
        assert c["doubling"] % 1024 == 0 and c["segments"] > 1
    assert small["flags"] < large["flags"] and small["doubling"] == small["flags"] and large["doubling"] < large["flags"]
    assert sh["tile"] % (64 * 1024) == 0
    for K in S.KS:
        for N, B in ((K, 1), (K + 1, 7), (24, 1000), (300, 8192), (5000, 65536)):
            assert S.shape(K, N, B)["window"] == _window(N, K, B)
            assert S.shape(K, N, B, 777)["window"] == 777
    # the build follows the expected flag count of the window
    assert S.shape(7, 2000, 8192)["build"] == "small" and S.shape(7, 200, 4096)["build"] == "large"
    assert S.shape(7, 8, 1, 200)["build"] == "small" and S.shape(7, 8, 1)["build"] == "large"
    for bad in ((2, 10, 1), (6, 10, 1), (7, 6, 1), (3, 10, 0)):
        with pytest.raises(poselib_amd.PoseLibAmdError):
            poselib_amd.sampler_shape(*bad)


def test_the_sampler_entry_refuses_what_the_driver_refuses():
    """pl_debug_sample_positions checks its arguments before it looks for a device: PL_ERR_INVALID, here too."""
    ok = {"seed": 1, "pos_base": 0, "N": 100, "B": 10, "M": 1000}
    bad = [(6, [ok], {}), (2, [ok], {}), (7, [dict(ok, N=6)], {}), (7, [dict(ok, B=0)], {}), (7, [dict(ok, B=2 ** 20 + 1)], {}),
           (7, [dict(ok, M=2 ** 31)], {}), (7, [dict(ok, pos_base=2 ** 32 - 1 - 1000)], {}), (7, [], {}), (7, [ok] * 5, {}),
           (7, [ok, dict(ok, planted=np.full(1000, 7, dtype=np.uint8))], {"group": True})]
    for K, members, kw in bad:
        with pytest.raises(poselib_amd.PoseLibAmdError) as e:
            poselib_amd.sample_positions(K, members, **kw)
        assert f"error {poselib_amd._lib.PL_ERR_INVALID}:" in str(e.value), (K, members)
    with pytest.raises(KeyError):
        poselib_amd.sample_positions(7, [ok], build="medium")


@pytest.mark.parametrize("K", S.KS)
def test_restatement_matches_the_oracle(K):
    for N in (K, K + 1, 11, 300, 5000):
        n = 2000
        idx, pos = O.sampler_draw_positions(S.SEED, N, K, n + 1)
        pos = pos.astype(np.int64)
        M = int(pos[n]) + 255
        delta = S.delta_table(S.SEED, 0, N, K, M)
        w = S.walk(delta, K, n, {"flags": M, "segments": n + 1})
        used = np.diff(pos)
        if used.max() < 255:
            assert not w.saturated and (w.positions == pos[:n]).all() and w.end == pos[n], (K, N)
        else:  # (N = K: a sample can take 255 draws and more - the table clips there, and the model says so)
            first = int(np.argmax(used >= 255))
            assert w.saturated and (w.positions[:first + 1] == pos[:first + 1]).all(), (K, N)
        assert (delta[pos[:n]] == np.minimum(used, 255)).all(), (K, N)
        # the draws themselves: the first K distinct values behind every start are the oracle's sample
        d = S.draw_stream(S.SEED, 0, M, N)
        for i in (0, 1, n // 2, n - 1):
            seen = []
            for v in d[pos[i]:pos[i + 1]].tolist():
                if v not in seen:
                    seen.append(v)
            assert seen == idx[i].tolist(), (K, N, i)
    # a window that starts in the middle of the stream is the same table, shifted
    a = S.delta_table(S.SEED, 0, 300, K, 3000)
    b = S.delta_table(S.SEED, 1234, 300, K, 1000)
    assert (a[1234:2234] == b).all()
    assert (S.bitmap(b, K)[:15] == [sum(1 << k for k in range(64) if b[64 * w + k] != K) for w in range(15)]).all()


@pytest.mark.parametrize("name", sorted(S.DRAWN))
def test_drawn_cases_take_the_path_they_are_named_for(name):
    N, K, B, forced, want = S.DRAWN[name]
    sh, build, delta, w = S.drawn(name)
    assert sh["window"] == _window(N, K, B) == delta.size
    if name in S.DRAWN_BUILD:
        assert forced is None and sh["build"] == S.DRAWN_BUILD[name]
    if forced:
        assert sh["build"] != forced, "a forced build is the one the launcher would not pick"
    got = S.path(w.F, sh[build])
    print(f"{name}: N {N} K {K} B {B} M {delta.size} F {w.F} visited {w.visited} end {w.end} build {build} path {got} {w.reasons}")
    if want is not None:
        assert got == want
    assert w.error == (got == "overflow"), "a drawn case fails for its flag count alone or not at all"
    if got != "overflow":
        assert w.visited > 0 or B == 1


def test_the_window_slack_alone_overflows_the_tables_of_small_problems():
    """The finding recorded in DESIGN.md: where almost every position is flagged, the 8192 positions of slack hold nearly as many flags
    as the large build takes - a batch of ONE iteration still fits for N = 7 and 8, one of 64 iterations no longer does, and at the
    batch sizes a run reaches (a thousand iterations and more) N = 24 overflows as well, while N = 60 walks on the device."""
    large = S.caps("large")
    F = lambda N, K, B: int(np.count_nonzero(S.delta_table(S.SEED, 0, N, K, S.shape(K, N, B)["window"]) != K))  # noqa: E731
    assert 0.99 * large["flags"] < F(7, 7, 1) <= large["flags"]
    assert F(8, 7, 1) <= large["flags"] < F(8, 7, 64)
    assert F(24, 7, 1000) > large["flags"]
    assert F(60, 7, 2048) <= large["flags"]


@pytest.mark.parametrize("build", S.BUILDS)
@pytest.mark.parametrize("K", S.KS)
def test_planted_cases_hit_their_edges(K, build):
    c = S.caps(build)
    cases = S.planted_cases(K, build)
    names = [p.name for p in cases]
    assert len(set(names)) == len(names)
    by = dict(zip(names, cases))
    for p in cases:
        w = S.walk(p.delta, K, p.B, c)
        assert (w.F, w.visited, w.end, w.error) == (p.F, p.visited, p.end, p.error), (p.name, w)
    # ... and the edges themselves, in the shape entry's constants
    assert by["flags_at_capacity"].F == c["flags"] and by["flags_over_capacity"].F == c["flags"] + 1
    assert by["segments_below_capacity"].visited == c["segments"] - 1 and by["segments_at_capacity"].visited == c["segments"]
    assert S.path(by["segments_at_capacity"].F, c) == "doubling"
    if build == "large":
        assert by["flags_at_doubling_limit"].F == c["doubling"] and S.path(by["flags_over_doubling_limit"].F, c) == "serial"
        a, b = by["flags_at_doubling_limit"], by["flags_over_doubling_limit"]  # one table but for a flag no iteration starts at
        assert np.count_nonzero(a.delta != b.delta[:a.delta.size]) == 1 and b.delta.size == a.delta.size + K
        assert (S.walk(a.delta, K, a.B, c).positions == S.walk(b.delta, K, b.B, c).positions).all()
        for n in ("serial_segments_below_capacity", "serial_segments_at_capacity"):
            assert S.path(by[n].F, c) == "serial"
        assert by["serial_segments_at_capacity"].visited == c["segments"]
    assert S.walk(by["window_exact"].delta, K, by["window_exact"].B, c).reasons == ()
    assert S.walk(by["window_one_short"].delta, K, by["window_one_short"].B, c).reasons == ("window",)
    assert S.walk(by["delta_255_visited"].delta, K, 100, c).reasons == ("delta255",)
    assert S.walk(by["segments_at_capacity"].delta, K, by["segments_at_capacity"].B, c).reasons == ("segments",)
    assert S.walk(by["flags_over_capacity"].delta, K, 512, c).reasons == ("flags",)
    t = by["two_tiles"]
    T = S.tile()
    fl = np.flatnonzero(t.delta != K)
    assert t.delta.size > T and t.delta.size % 64 and (fl < T).any() and (fl >= T).any()
    assert ((fl >= T - 64) & (fl < T + 64)).all()
    w = S.walk(t.delta, K, t.B, c)
    assert w.positions[-1] > T + 64, "the batch walks through both flagged words"
    r = by["long_flagged_run"]
    w = S.walk(r.delta, K, r.B, c)
    steps = np.diff(w.positions.astype(np.int64))
    run = np.flatnonzero(steps != K)
    assert run.size >= 6 * 64 and (np.diff(run) == 1).all()
    s = S.walk(by["segment_at_wave_start"].delta, K, 4096, c)
    per_wave = ((4096 + 15) // 16 + 63) // 64 * 64
    assert by["segment_at_wave_start"].delta[s.positions[per_wave - 1]] != K


@pytest.mark.parametrize("build", S.BUILDS)
@pytest.mark.parametrize("K", S.KS)
def test_random_tables_stay_inside_the_tables(K, build):
    c = S.caps(build)
    tables = S.random_tables(K, build)
    assert len(tables) == 9
    for name, B, d in tables:
        w = S.walk(d, K, B, c)
        assert not w.error and w.visited > 0, (name, w.reasons)
        assert K < d[d != K].min() and d.max() <= K + 40
