"""Cases and the reference model of the device sampler's tests (tests/test_gpu_sampler.py, checked on the CPU by
tests/test_sampler_cases.py).

Everything here is numpy in exact integer arithmetic plus the library's host-only shape entry (pl_debug_sampler_shape) - no device.

* draw_stream / delta_table: pl_sampler.h's draw_at (splitmix64, truncated to a signed 32-bit value, sign-extended, `% N` unsigned) and
  the table k_sample_delta<K> fills - draws an iteration STARTING at each position of the window consumes, clipped at 255.
* walk: the sequential walk  p -> p + delta[p]  over such a table, as the MODEL of k_sample_orbit: positions[i], the position after
  the batch and the orbit_error predicate of a build.  Where the model reports an error the positions are unspecified.
* DRAWN: real draw streams, named after the path of the orbit kernel they take; PLANTED: delta tables no draw stream produces, at the
  edges of the kernel's tables.  Every capacity comes from the shape entry, never from a literal.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import poselib_amd

GAMMA = np.uint64(0x9E3779B97F4A7C15)
KS = (3, 4, 5, 7)
SEED = 12345
BUILDS = ("small", "large")


# ------------------------------------------------------------------ the draw stream
def draw_stream(seed, first, count, N):
    """draw_at(seed, j, N) for the 1-based draw counters j = first + 1 .. first + count."""
    with np.errstate(over="ignore"):
        j = np.uint64(first) + np.arange(1, count + 1, dtype=np.uint64)
        z = np.uint64(seed) + j * GAMMA
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    r = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).astype(np.int64).view(np.uint64)
    return r % np.uint64(N)


def delta_table(seed, pos_base, N, K, M):
    """delta[p], p < M: the draws a sample of K distinct indices consumes when it starts behind pos_base + p draws, at most 255."""
    d = draw_stream(seed, pos_base, M + 255, N)
    chosen = np.zeros((M, K), dtype=np.uint64)
    have = np.zeros(M, dtype=np.int64)
    used = np.full(M, 255, dtype=np.int64)
    act = np.arange(M)
    for t in range(255):  # the t-th draw of every sample that is still incomplete
        if act.size == 0:
            break
        v = d[act + t]
        h = have[act]
        fresh = np.ones(act.size, dtype=bool)
        for k in range(K):
            fresh &= ~((k < h) & (chosen[act, k] == v))
        a = act[fresh]
        chosen[a, have[a]] = v[fresh]
        have[a] += 1
        done = a[have[a] == K]
        used[done] = t + 1
        act = act[have[act] < K]
    return used.astype(np.uint8)


def bitmap(delta, K):
    """The bitmap k_sample_delta writes: bit p of word p / 64 set where delta[p] != K, no bit at or behind len(delta)."""
    M = delta.size
    f = np.zeros((M + 63) // 64 * 64, dtype=np.uint64)
    f[:M] = delta != K
    return (f.reshape(-1, 64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


# ------------------------------------------------------------------ the model
Walk = namedtuple("Walk", "positions end error F visited saturated reasons")


def walk(delta, K, B, caps):
    """The sequential walk over a delta table, and what a build of the orbit kernel with the capacities `caps` must report.
    positions[i]: draws consumed before iteration i (relative to the window's start); end: before iteration B; F: flagged positions
    in the window; visited: flagged positions an iteration below B starts at; saturated: one of those has delta 255.  Behind the
    window every iteration takes K draws (the kernel knows no flag there): then end + 255 > M holds anyway."""
    M = delta.size
    F = int(np.count_nonzero(delta != K))
    positions = np.zeros(B, dtype=np.uint32)
    p = visited = 0
    saturated = False
    dl = delta.tolist()
    for i in range(B):
        positions[i] = p
        d = dl[p] if p < M else K
        if d != K:
            visited += 1
            saturated |= d == 255
        p += d
    reasons = []
    if F > caps["flags"]:
        reasons.append("flags")
    if visited >= caps["segments"]:
        reasons.append("segments")
    if saturated:
        reasons.append("delta255")
    if p + 255 > M:
        reasons.append("window")
    return Walk(positions, p, bool(reasons), F, visited, saturated, tuple(reasons))


def path(F, caps):
    """Which way the orbit kernel produces its segments for F flags."""
    return "overflow" if F > caps["flags"] else "doubling" if F <= caps["doubling"] else "serial"


@functools.lru_cache(maxsize=None)
def shape(K, N, B, window=0):
    return poselib_amd.sampler_shape(K, N, B, window)


def caps(build):
    return shape(7, 1000, 1)[build]


def tile():
    return shape(7, 1000, 1)["tile"]


# ------------------------------------------------------------------ drawn cases
# name -> (N, K, B, forced build or None, the path the case is there for)
DRAWN = {
    "over_n8": (8, 7, 64, None, "overflow"),
    "over_n24": (24, 7, 1000, None, "overflow"),
    "serial_n8": (8, 7, 1, None, "serial"),
    "serial_n60": (60, 7, 2048, None, "serial"),
    "doubling_n200": (200, 7, 4096, None, "doubling"),
    "small_n2000": (2000, 7, 8192, None, "doubling"),
    "forced_small_fits": (300, 5, 8192, "small", "doubling"),
    "forced_small_overflows": (200, 5, 8192, "small", "overflow"),
    "forced_large_n2000": (2000, 7, 8192, "large", "doubling"),
    "forced_large_k4": (150, 4, 3000, "large", "doubling"),
}
DRAWN_BUILD = {"over_n8": "large", "over_n24": "large", "serial_n8": "large", "serial_n60": "large", "doubling_n200": "large",
               "small_n2000": "small"}  # what the launcher must pick by itself
for _k in KS:  # N = K: every sample of K draws but K! / K^K repeats an index
    DRAWN[f"n_equals_k{_k}"] = (_k, _k, 1, None, None)


@functools.lru_cache(maxsize=None)
def drawn(name, pos_base=0, M=0, seed=SEED):
    """(shape, build that runs, delta table, model) of a drawn case."""
    N, K, B, forced, _ = DRAWN[name]
    sh = shape(K, N, B, M)
    build = forced or sh["build"]
    delta = delta_table(seed, pos_base, N, K, sh["window"])
    return sh, build, delta, walk(delta, K, B, sh[build])


# ------------------------------------------------------------------ planted cases
Planted = namedtuple("Planted", "name K B delta build F visited end error")


def _table(M, K, flags):
    d = np.full(M, K, dtype=np.uint8)
    for p, v in flags.items():
        assert 0 <= p < M and v != K
        d[p] = v
    return d


def _on_orbit(K, V, first_iteration=0, d=None):
    """V flags at consecutive iterations from `first_iteration` on, each consuming d (K + 1) draws: {position: d}, the position
    behind the last of them."""
    d = d or K + 1
    p = first_iteration * K
    flags = {}
    for _ in range(V):
        flags[p] = d
        p += d
    return flags, p


def _off_orbit(K, count, stride, start):
    """`count` flags at start, start + stride, ... (delta K + 2) - the caller picks positions no iteration starts at."""
    return {start + stride * i: K + 2 for i in range(count)}


def planted_cases(K, build):
    """The planted tables of one K for one build of the orbit kernel, each with what it is there for: F, the visited flags, the
    position behind the batch and whether the kernel must report an error."""
    c = caps(build)
    Cf, Cd, Cs = c["flags"], c["doubling"], c["segments"]
    out = []

    def add(name, B, M, flags, F, visited, end, error):
        out.append(Planted(name, K, B, _table(M, K, flags), build, F, visited, end, error))

    # no flag at all: the batch sizes at which phase 3 cuts differently (per_wave = ceil(B / 16) rounded up to 64)
    for B in (1, 63, 64, 65, 1024, 1025, 3000, 8192):  # 3000: per_wave 192, the last wavefront ends 56 into its second stride
        add(f"unflagged_B{B}", B, B * K + 255 + 37, {}, 0, 0, B * K, False)
    # the flag capacity, one past; the doubling limit, one past (the same table but for one flag no iteration starts at).  100
    # visited flags at the iterations 0, 2, 4, ... (2 K draws each: the orbit stays on phase 0), the others on phase 1.
    vis = {2 * K * i: 2 * K for i in range(100)}
    for name, F in [("flags_at_capacity", Cf), ("flags_over_capacity", Cf + 1)] + \
                   ([("flags_at_doubling_limit", Cd), ("flags_over_doubling_limit", Cd + 1)] if Cd != Cf else []):
        flags = dict(vis)
        flags.update(_off_orbit(K, F - 100, K, 1))
        M = 1 + K * (F - 100) + 300
        add(name, 512, M, flags, F, 100, 512 * K + 100 * K, F > Cf)
    # no flag on phase 0 while others exist; flags at position 0 and at M - 1
    add("no_flag_on_phase_0", 300, 300 * K + 400, _off_orbit(K, 200, K, 1), 200, 0, 300 * K, False)
    M = 200 * K + 3 + 255 + 130
    add("flag_at_0_and_last", 200, M, {0: K + 3, M - 1: K + 1}, 2, 1, 200 * K + 3, False)
    # the segment table: one below its capacity and at it, every iteration flagged - on the doubling path ...
    for name, V in (("segments_below_capacity", Cs - 1), ("segments_at_capacity", Cs)):
        flags, p = _on_orbit(K, V)
        add(name, V + 10, p + 10 * K + 300, flags, V, V, p + 10 * K, V >= Cs)
    # ... and on the one-lane walk (F above the doubling limit; the flags between the orbit's never start an iteration)
    if Cd != Cf:
        for name, V in (("serial_segments_below_capacity", Cs - 1), ("serial_segments_at_capacity", Cs)):
            flags, p = _on_orbit(K, V)
            extra = Cd + 100 - V
            flags.update(_off_orbit(K, extra, K + 1, 1))
            add(name, V + 10, p + 10 * K + 300, flags, V + extra, V, p + 10 * K, V >= Cs)
    # delta saturation
    B = 100
    add("delta_254_visited", B, B * K + 600, {10 * K: 254}, 1, 1, B * K + 254 - K, False)
    add("delta_255_visited", B, B * K + 600, {10 * K: 255}, 1, 1, B * K + 255 - K, True)
    add("delta_255_unvisited", B, B * K + 600, {10 * K + 1: 255}, 1, 0, B * K, False)
    add("delta_255_behind_batch", B, B * K + 600, {(B + 3) * K: 255}, 1, 0, B * K, False)
    # the batch boundary
    add("flag_at_last_iteration", B, B * K + 600, {(B - 1) * K: K + 5}, 1, 1, B * K + 5, False)
    add("flag_at_iteration_B", B, B * K + 600, {B * K: K + 5}, 1, 0, B * K, False)
    # the window
    add("window_exact", B, B * K + 4 + 255, {5 * K: K + 4}, 1, 1, B * K + 4, False)
    add("window_one_short", B, B * K + 4 + 254, {5 * K: K + 4}, 1, 1, B * K + 4, True)
    # phase 3: 6 x 64 consecutive flagged iterations from iteration 300 on (per_wave = 256: every lane crosses 64 segments per
    # stride - past the four-step probe into the binary search), and a segment that starts at a wavefront's first iteration
    flags, p = _on_orbit(K, 384, 300)
    add("long_flagged_run", 4096, p + (4096 - 684) * K + 300, flags, 384, 384, p + (4096 - 684) * K, False)
    add("segment_at_wave_start", 4096, 4096 * K + 400, {255 * K: K + 2, 2047 * K + 2: K + 1}, 2, 2, 4096 * K + 3, False)
    # phase 1: a second tile with a ragged remainder; visited flags in the last word of tile one and the first word of tile two,
    # flags no iteration starts at on either side of the seam
    T = tile()
    p1 = (T - 1) // K * K          # the last phase-0 position of tile one
    p2 = p1 + K + 1                # ... and where its iteration leaves the orbit, in tile two
    assert T - 64 <= p1 < T <= p2 < T + 64
    B = p2 // K + 40
    flags = {p1: K + 1, p2: K + 3, T: K + 2}  # (p2 > T: no iteration starts at T)
    if p1 != T - 1:
        flags[T - 1] = K + 2       # ... nor at T - 1, behind p1
    its = p1 // K + 1              # iterations up to and including the one at p1
    end = p2 + (K + 3) + (B - its - 1) * K
    F = len(flags)
    add("two_tiles", B, T + 1000 + 37, flags, F, 2, end, False)
    return out


def random_tables(K, build):
    """Random planted tables: flag densities 0.001, 0.05 and 0.5, deltas K + 1 .. K + 40, three seeds; sized to stay inside the
    build's tables and the window, so the positions are compared."""
    c = caps(build)
    out = []
    for density in (0.001, 0.05, 0.5):
        M = min(40000, int(0.8 * c["flags"] / density))
        B = int((M - 300) / (K + density * 20.5) * 0.9)
        for seed in range(3):
            rng = np.random.default_rng(1000 * K + 10 * seed + int(density * 1000))
            d = np.full(M, K, dtype=np.uint8)
            f = rng.random(M) < density
            d[f] = rng.integers(K + 1, K + 41, size=int(f.sum()), dtype=np.uint8)
            out.append((f"random_d{density}_s{seed}", B, d))
    return out
