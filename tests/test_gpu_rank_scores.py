"""The ranking kernels position by position: rank_scores (pl_debug_rank_scores) against the rule's numpy statement
(poselib_amd.score_order: keep = s >= min_score; order = flatnonzero(keep)[argsort(-s[keep], kind="stable")]), in the kernels'
single form and in the grouped one, for every size at which the code takes another path - the two LDS tiles, their edges, the
merge passes beyond them -, for fp32 and fp64 scores, contiguous and as column 4 of an (N, 5) block, and for the score patterns in
which a sort can go wrong: ties, NaN, infinities, signed zeros, fp32 denormals."""
import numpy as np
import pytest

from device_arrays import DeviceArray, on_gpu

pytestmark = pytest.mark.gpu

SMALL_TILE, LARGE_TILE = 1024, 8192  # (asserted below against the library's own answer)
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, SMALL_TILE - 1, SMALL_TILE, SMALL_TILE + 1, 2 * SMALL_TILE + 1, LARGE_TILE - 1,
         LARGE_TILE, LARGE_TILE + 1, 16384, 2 * LARGE_TILE + 1, 40000)
DENORMAL = float(np.float32(2.0 ** -149))  # the smallest fp32 subnormal (exact in both dtypes)


def pattern(name, n, seed=0):
    rng = np.random.default_rng(1000 + 7 * n + seed)
    if name == "all_equal":
        return np.full(n, 0.25)
    if name == "ascending":
        return np.arange(n) / 64.0
    if name == "descending":
        return np.arange(n)[::-1] / 64.0
    if name == "two_values":
        return rng.choice([0.125, 0.875], n)
    if name == "duplicates":
        return rng.integers(0, max(2, n // 8), n) / 8.0
    if name == "nan_edges":
        s = rng.integers(0, max(2, n // 8), n) / 8.0
        if n:
            s[[0, n // 2, n - 1]] = np.nan
        return s
    if name == "all_nan":
        return np.full(n, np.nan)
    if name == "inf_and_zero":
        return rng.choice([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0], n)
    assert name == "denormals"
    return rng.integers(-4, 5, n) * DENORMAL + rng.choice([0.0, -0.0], n)


PATTERNS = ("all_equal", "ascending", "descending", "two_values", "duplicates", "nan_edges", "all_nan", "inf_and_zero", "denormals")
LAYOUTS = ((np.float32, 1), (np.float64, 1), (np.float32, 5), (np.float64, 5))


def upload(values, dtype, stride):
    """(device array, the host values it holds): contiguous, or column 4 of an (N, 5) block whose other columns would rank first"""
    host = np.asarray(values, dtype=dtype)
    if stride == 1:
        return on_gpu(host), host
    block = np.full((len(host), 5), 7e30, dtype=dtype)
    block[:, 4] = host
    return DeviceArray.upload(block)[:, 4], host


def thresholds(host):
    """-inf, a value between two scores, a value some rows tie with, +inf"""
    finite = np.unique(host[np.isfinite(host)].astype(np.float64))
    between = 0.5 * (finite[len(finite) // 2 - 1] + finite[len(finite) // 2]) if len(finite) >= 2 else 0.1
    tied = float(finite[len(finite) // 2]) if len(finite) else 0.25
    return (None, float(between), tied, np.inf)


def check(got, host, min_score, what):
    from poselib_amd import score_order

    want = score_order(host, min_score)
    assert got.dtype == np.uint32 and len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:5])


def test_the_tiles_are_the_ones_the_sizes_were_chosen_for(gpu):
    assert gpu.rank_tile(1) == SMALL_TILE and gpu.rank_tile(SMALL_TILE) == SMALL_TILE
    assert gpu.rank_tile(SMALL_TILE + 1) == LARGE_TILE and gpu.rank_tile(40000) == LARGE_TILE


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{np.dtype(l[0]).name}-stride{l[1]}")
def test_every_size_in_the_single_form(gpu, layout):
    for n in SIZES:
        dev, host = upload(pattern("duplicates", n), *layout)
        for m in thresholds(host)[:3]:
            check(gpu.rank_scores(dev, m), host, m, (n, m))


@pytest.mark.parametrize("name", PATTERNS)
def test_every_pattern_layout_and_threshold(gpu, name):
    for n in (3, 65, SMALL_TILE + 1, 2 * LARGE_TILE + 1):
        for layout in LAYOUTS:
            dev, host = upload(pattern(name, n), *layout)
            for m in thresholds(host):
                check(gpu.rank_scores(dev, m), host, m, (name, n, layout[1], m))


def members_of(sizes, seed):
    out = []
    for k, n in enumerate(sizes):
        dev, host = upload(pattern(PATTERNS[(k + seed) % len(PATTERNS)], n, seed), *LAYOUTS[(k + seed) % 4])
        out.append((dev, host, thresholds(host)[(k + seed) % 4]))
    return out


@pytest.mark.parametrize("sizes", [SIZES, tuple(n for n in SIZES if n <= SMALL_TILE), (40000, 5, LARGE_TILE + 1, 0, 16385, 300)],
                         ids=["all", "small_tile", "large_first"])
def test_ragged_members_of_both_dtypes_in_one_grouped_call(gpu, sizes):
    for seed in range(4):  # (every size meets every layout, and four patterns and thresholds)
        members = members_of(sizes, seed)
        got = gpu.rank_scores([m[0] for m in members], [m[2] for m in members])
        assert len(got) == len(members)
        for n, (dev, host, m), g in zip(sizes, members, got):
            check(g, host, m, ("grouped", seed, n, m))
            if seed == 0:  # ... and the single form says the same
                assert np.array_equal(gpu.rank_scores(dev, m), g), ("single", n)


def test_a_nan_threshold_is_refused(gpu):
    dev, _ = upload(pattern("duplicates", 64), np.float32, 1)
    with pytest.raises(ValueError):
        gpu.rank_scores(dev, float("nan"))
