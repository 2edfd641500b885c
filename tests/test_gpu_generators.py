"""The hypothesis generators of the main loop, hypothesis by hypothesis against the oracle (-m gpu).

pl_debug_generate runs the kernels a batch step launches - k_generate<EST> with the wave-wide second half of P3P, the staged 5-point
generator k_rel_front / k_rel_roots / k_rel_poses, its tangent front, the single-kernel 5-point generator, the group forms - wired as
a batch step wires them, and returns every iteration's records, counts, NaN flags and the per-block tables.  The reference is the
oracle estimators' generate_models on the same samples (tests/generator_cases.py; tests/test_generator_cases.py checks on the CPU that
the cases reach the paths they are there for).  Every comparison is on bits, for every iteration; NaN entries must be NaN in the same
places."""
import numpy as np
import pytest

import generator_cases as G
import oracle_lib as O

pytestmark = pytest.mark.gpu

# configuration -> (point set, real_focal_check, route of pl_debug_generate)
CONFIGS = {"abs": ("abs", False, 0), "rel_staged": ("rel", False, 0), "rel_single": ("rel", False, 1), "fund": ("fund", False, 0),
           "fund_rfc": ("fund", True, 0), "hom": ("hom", False, 0)}
GROUP_CONFIGS = ["abs", "rel_staged", "fund", "fund_rfc", "hom"]
UNWRITTEN = 0xFFFFFFFF  # counts and NaN flags before the launch


def bits_equal(got, want):
    """float64 arrays equal bit for bit, NaN against NaN whatever the payload"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def records_equal(got, want):
    """records of 24 doubles: the 16 fp64 fields and the 16 fp32 values of the shadow"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or not bits_equal(got[..., :16], want[..., :16]):
        return False
    gs, ws = np.ascontiguousarray(got[..., 16:]).view(np.float32), np.ascontiguousarray(want[..., 16:]).view(np.float32)
    return bool(((gs.view(np.uint32) == ws.view(np.uint32)) | (np.isnan(gs) & np.isnan(ws))).all())


class Expected:
    """What the generator must write for a Reference: the oracle's counts and models, and - for the whole records - what k_solve_batch
    writes for the oracle's solver input of every sample (that kernel is pinned to the oracle by tests/test_gpu_parity.py; here its
    counts and models are compared with the oracle's once more, for every sample)."""

    def __init__(self, gpu, ref, plain=None):
        self.ref = ref
        k = G.K[ref.kind]
        src = ref if plain is None else plain  # real_focal_check: the records of the models the check keeps
        rec, cnt = gpu.solve_batch(ref.kind, src.sample_in[:, :k], src.sample_in[:, k:], full_records=True)
        assert np.array_equal(cnt, src.counts)
        rec[np.arange(rec.shape[1])[None, :] >= cnt[:, None]] = 0.0  # (pl_solve_batch says nothing about the slots beyond the count)
        model = rec[:, :, :7] if ref.kind in (0, 1) else rec[:, :, 7:16]
        assert bits_equal(model, src.models)
        if plain is not None:
            kept = np.zeros_like(rec)
            for i in range(ref.B):
                at = 0
                for m in range(plain.counts[i]):
                    if at < ref.counts[i] and bits_equal(plain.models[i, m], ref.models[i, at]):
                        kept[i, at] = rec[i, m]
                        at += 1
                assert at == ref.counts[i]
            rec = kept
        slot = np.arange(rec.shape[1])[None, :] < ref.counts[:, None]
        self.records = rec
        # the NaN flag of a record: a NaN in t or in the matrix (pl_math.h store_shadow); the same models as the oracle's NaN ones
        self.nan = np.isnan(rec[:, :, 4:16]).any(axis=2) & slot
        assert np.array_equal(self.nan, ref.nan)


def check_against(out, exp, B, slots, tag, overflow_expected=False):
    """every output of one member of a launch over the first B samples of exp.ref with `slots` record slots per iteration"""
    ref = exp.ref
    counts = ref.counts[:B].astype(np.int64)
    fits = counts <= slots
    want_counts = np.where(fits, counts, 0)
    assert out["overflow"] == (0 if fits.all() else 1), tag
    assert (not fits.all()) == overflow_expected, tag
    assert np.array_equal(out["num_models"], want_counts), (tag, np.flatnonzero(out["num_models"] != want_counts)[:8])
    rec = out["records"]
    assert rec.shape == (B, slots, 24)
    want = exp.records[:B, :slots]
    assert records_equal(rec[fits], want[fits]), (tag, [i for i in np.flatnonzero(fits) if not records_equal(rec[i], want[i])][:8])
    # (an iteration with more models than slots counts 0; what it left in its slots is not read by anything)
    model = rec[:, :, :7] if ref.kind in (0, 1) else rec[:, :, 7:16]
    assert bits_equal(model[fits], ref.models[:B, :slots][fits]), tag
    nan = exp.nan[:B, :slots] & fits[:, None]
    tot, nansum = ref.block_sums(B, want_counts, nan)
    assert np.array_equal(out["blk_tot"], tot), (tag, out["blk_tot"], tot)
    assert np.array_equal(out["blk_nan"], nansum), (tag, out["blk_nan"], nansum)
    if ref.kind == 0:
        want_bits = (nan.astype(np.uint32) << np.arange(slots, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
        assert np.array_equal(out["nan_bits"], want_bits), (tag, np.flatnonzero(out["nan_bits"] != want_bits)[:8])
    flag = np.ascontiguousarray(rec[..., 16:]).view(np.float32)[..., 13]
    assert np.array_equal(flag[fits] != 0, np.isnan(rec[..., 4:16]).any(axis=-1)[fits]), tag


def outputs_identical(a, b, B=None):
    B = len(a["num_models"]) if B is None else B
    return (records_equal(a["records"][:B], b["records"][:B]) and np.array_equal(a["num_models"][:B], b["num_models"][:B])
            and np.array_equal(a["nan_bits"][:B], b["nan_bits"][:B]))


@pytest.fixture(scope="module")
def world(gpu):
    """resident problems and expected records, built on first use and shared by the tests of the module"""

    class World:
        def __init__(self):
            self.problems, self.expected = {}, {}

        def problem(self, name):
            if name not in self.problems:
                kind, a, b = G.points(name)
                self.problems[name] = gpu.Problem(kind, a, b)
            return self.problems[name]

        def expect(self, key, ref, plain=None):
            if key not in self.expected:
                self.expected[key] = Expected(gpu, ref, plain)
            return self.expected[key]

        def config(self, config):
            name, rfc, route = CONFIGS[config]
            ref = G.reference(name, rfc)
            return self.problem(name), self.expect((name, rfc), ref, G.reference(name) if rfc else None), rfc, route

    w = World()
    yield w
    for p in w.problems.values():
        p.close()


@pytest.mark.parametrize("B", G.ITERATION_COUNTS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_generator_equals_generate_models(gpu, world, config, B):
    """explicit samples and the device's own draws from the reference's positions: identical outputs, and the oracle's"""
    prob, exp, rfc, route = world.config(config)
    ref = exp.ref
    slots = G.MAX_MODELS[ref.kind]
    given, = gpu.debug_generate(prob, samples=ref.samples[:B], real_focal_check=rfc, route=route)
    drawn, = gpu.debug_generate(prob, seed=G.SEED, positions=ref.positions[:B], real_focal_check=rfc, route=route)
    check_against(given, exp, B, slots, (config, B, "samples"))
    check_against(drawn, exp, B, slots, (config, B, "positions"))
    assert outputs_identical(given, drawn)
    assert not given["records"][np.arange(slots)[None, :] >= ref.counts[:B, None]].any()  # slots beyond the count: still zero


@pytest.mark.parametrize("name", G.SMALL_SETS)
def test_device_draws_on_a_handful_of_correspondences(gpu, world, name):
    """8 and 11 correspondences: the sampler redraws in most iterations, the positions are far from K per iteration; and a non-zero
    pos_base with positions relative to it"""
    ref = G.reference(name)
    exp = world.expect((name, False), ref)
    prob = world.problem(name)
    routes = (0, 1) if ref.kind == 1 else (0,)
    for route in routes:
        for B in (65, 1025):
            slots = G.MAX_MODELS[ref.kind]
            given, = gpu.debug_generate(prob, samples=ref.samples[:B], route=route)
            drawn, = gpu.debug_generate(prob, seed=G.SEED, positions=ref.positions[:B], route=route)
            base = int(ref.positions[7])
            rebased, = gpu.debug_generate(prob, seed=G.SEED, pos_base=base, positions=ref.positions[7:B] - ref.positions[7], route=route)
            check_against(given, exp, B, slots, (name, route, B))
            assert outputs_identical(given, drawn)
            assert records_equal(rebased["records"], given["records"][7:]) and np.array_equal(rebased["num_models"], given["num_models"][7:])


@pytest.mark.parametrize("route", [0, 1])
def test_pose_queue_overflow_and_bucket_sort(gpu, world, route):
    """the samples with most poses first: the first workgroup of k_rel_poses has more poses than its LDS queue holds (the second write
    path), the later ones fewer; iterations with 8 roots next to iterations with 2 in the sorted workgroup"""
    ref = G.rel_rich()
    exp = world.expect("rel_rich", ref)
    prob = world.problem("rel")
    for B in (256, 257, 1025, G.B_MAX):
        out, = gpu.debug_generate(prob, samples=ref.samples[:B], route=route)
        check_against(out, exp, B, 40, ("rich", route, B))


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("case", ["rel", "rich"])
def test_slot_limit_of_the_5_point_generators(gpu, world, case, route):
    """one slot fewer than the largest count of the case: the overflow flag, count 0 for the iterations that do not fit, everything
    else unchanged; as many slots as the largest count: no overflow"""
    ref = G.reference("rel") if case == "rel" else G.rel_rich()
    exp = world.expect("rel_rich" if case == "rich" else ("rel", False), ref)
    prob = world.problem("rel")
    for B in (257, G.B_MAX):
        smax = int(ref.counts[:B].max())
        assert smax >= 3
        tight, = gpu.debug_generate(prob, samples=ref.samples[:B], slots_per_iter=smax - 1, route=route)
        check_against(tight, exp, B, smax - 1, (case, route, B, "one below"), overflow_expected=True)
        assert (tight["num_models"][ref.counts[:B] == smax] == 0).all()
        exact, = gpu.debug_generate(prob, samples=ref.samples[:B], slots_per_iter=smax, route=route)
        check_against(exact, exp, B, smax, (case, route, B, "equal"))


@pytest.mark.parametrize("B", G.ITERATION_COUNTS)
@pytest.mark.parametrize("config", GROUP_CONFIGS)
def test_group_form(gpu, world, config, B):
    """a table of three slots launched for B iterations: the inactive one writes nothing, the full member equals the single-problem
    launch, the short member (ceil(B / 3) iterations, buffers of its own) equals its prefix and leaves the rest of its buffers alone"""
    prob, exp, rfc, _ = world.config(config)
    ref = exp.ref
    slots = G.MAX_MODELS[ref.kind]
    single, = gpu.debug_generate(prob, samples=ref.samples[:B], real_focal_check=rfc, route=0)
    for source in ("samples", "positions"):
        kw = {"samples": ref.samples[:B]} if source == "samples" else {"seed": G.SEED, "positions": ref.positions[:B]}
        full, short = gpu.debug_generate(prob, real_focal_check=rfc, route=2, **kw)
        assert full["inactive_writes"] == 0
        check_against(full, exp, B, slots, (config, B, source, "member 1"))
        assert outputs_identical(full, single)
        assert np.array_equal(full["blk_tot"], single["blk_tot"]) and np.array_equal(full["blk_nan"], single["blk_nan"])
        B2 = (B + 2) // 3
        head = {k: (v[:B2] if k in ("records", "num_models", "nan_bits") else v[: (B2 + 1023) // 1024] if k in ("blk_tot", "blk_nan") else v)
                for k, v in short.items()}
        check_against(head, exp, B2, slots, (config, B, source, "member 2"))
        assert outputs_identical(head, single, B2)
        assert not short["records"][B2:].any() and (short["num_models"][B2:] == UNWRITTEN).all()
        assert not short["blk_tot"][(B2 + 1023) // 1024:].any() and not short["blk_nan"][(B2 + 1023) // 1024:].any()
        if ref.kind == 0:
            assert (short["nan_bits"][B2:] == UNWRITTEN).all()


@pytest.mark.parametrize("route", [0, 1])
def test_planted_samples_with_ten_and_eight_real_roots(gpu, world, route):
    ref = G.many_roots()
    exp = world.expect("many_roots", ref)
    out, = gpu.debug_generate(world.problem("rel"), samples=ref.samples, route=route)
    check_against(out, exp, ref.B, 40, ("many roots", route))


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("name", G.HARD_SETS)
def test_planted_hard_samples(gpu, name, route):
    """pure rotation, a planar scene, two coincident correspondences in one sample, a NaN and an infinite coordinate: count, order
    and bits of the oracle's recursion"""
    ref = G.hard_reference(name)
    exp = Expected(gpu, ref)
    prob = gpu.Problem(1, ref.a, ref.b)
    out, = gpu.debug_generate(prob, samples=ref.samples, route=route)
    prob.close()
    check_against(out, exp, ref.B, 40, (name, route))


def test_tangent_front_feeds_the_same_stages(gpu):
    """k_rel_front_tangent: the stored bearings of a tangent problem (the device's un-projection, restated bit for bit by the host
    compile of the same header, tests/hostmath_tangent) go into the solver as they stand"""
    import hostmath_tangent_lib as HT
    from poselib_amd import synth

    d = synth.relative_pose_scene(300, 0.3, 6105)
    cam = {"model": 1, "params": [1000.0, 1000.0, 500.0, 500.0]}  # PINHOLE
    d1, _, ok1 = HT.unproject_with_jac(cam, d["x1"])
    d2, _, ok2 = HT.unproject_with_jac(cam, d["x2"])
    assert ok1.all() and ok2.all()
    idx, pos = O.sampler_draw_positions(G.SEED, 300, 5, 1025)
    s = idx.astype(np.int64)
    rec, cnt = gpu.solve_batch(1, d1[s], d2[s], full_records=True)
    rec[np.arange(40)[None, :] >= cnt[:, None]] = 0.0
    for i in range(len(s)):  # the reference: relpose_5pt on the stored bearings
        want = O.relpose_5pt(d1[s[i]], d2[s[i]])
        assert cnt[i] == len(want) and bits_equal(rec[i, : cnt[i], :7], want), i
    prob = gpu.TangentProblem(d["x1"], d["x2"], cam, cam)
    for B in (63, 257, 1025):
        given, = gpu.debug_generate(prob, samples=idx[:B])
        drawn, = gpu.debug_generate(prob, seed=G.SEED, positions=pos[:B])
        assert np.array_equal(given["num_models"], cnt[:B]) and records_equal(given["records"], rec[:B])
        assert outputs_identical(given, drawn)
        assert np.array_equal(given["blk_tot"], np.add.reduceat(cnt[:B].astype(np.int64), np.arange(0, B, 1024)))
        assert given["overflow"] == 0 and not given["blk_nan"].any()
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.debug_generate(prob, samples=idx[:8], route=1)  # no single-kernel generator for the stored bearings
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.debug_generate(prob, samples=idx[:8], route=2)
    prob.close()


def test_calls_that_do_not_fit_are_rejected(gpu, world):
    prob = world.problem("rel")
    ref = G.reference("rel")
    bad = ref.samples[:4].copy()
    bad[2, 3] = 300  # == n
    for kw in ({"samples": bad}, {"samples": ref.samples[:0]}, {"samples": ref.samples[:4], "slots_per_iter": 0},
               {"samples": ref.samples[:4], "slots_per_iter": 41}, {"samples": ref.samples[:4], "route": 3},
               {"samples": ref.samples[:4], "positions": ref.positions[:4]}):
        with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
            gpu.debug_generate(prob, **kw)
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.debug_generate(world.problem("abs"), samples=G.reference("abs").samples[:4], route=1)
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.debug_generate(world.problem("hom"), samples=G.reference("hom").samples[:4], slots_per_iter=2)
    big = np.zeros(((1 << 20) + 1, 5), dtype=np.uint32) + np.arange(5, dtype=np.uint32)
    with pytest.raises(gpu.PoseLibAmdError, match="error -3"):
        gpu.debug_generate(prob, samples=big, slots_per_iter=1)
