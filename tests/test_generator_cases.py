"""What tests/test_gpu_generators.py feeds the generator kernels, checked without a device: the cases do reach the paths they are
there for - computed from the oracle alone - and the flat root isolation at the generator's list capacities equals the recursion."""
import numpy as np
import pytest

import generator_cases as G
import hostmath_lib as HM
import oracle_lib as O


def test_oracle_generate_models_is_the_solver_on_the_oracles_own_bearings():
    """orc_generate_models against the single-sample solver entries on the solver input it reports, and that input against the
    points: unit vectors along (x, y, 1) / the 3-D points as they are"""
    for name in ("abs", "rel", "fund", "hom"):
        r = G.reference(name)
        k = G.K[r.kind]
        for i in range(40):
            first, second = r.sample_in[i, :k], r.sample_in[i, k:]
            if r.kind == 0:
                want = O.p3p(first, second)
                assert np.array_equal(second, r.b[r.samples[i].astype(np.int64)])
            elif r.kind == 1:
                want = O.relpose_5pt(first, second)
            elif r.kind == 2:
                want = [F.reshape(9) for F in O.relpose_7pt(first, second)]
            else:
                n, H = O.homography_4pt(first, second)
                want = [H.reshape(9)] if n else []
            assert r.counts[i] == len(want)
            for m, w in enumerate(want):
                assert np.array_equal(r.models[i, m], np.asarray(w), equal_nan=True)
            assert not r.models[i, r.counts[i]:].any()
            xy = r.a[r.samples[i].astype(np.int64)]
            assert np.abs(first[:, :2] / first[:, 2:3] - xy).max() < 1e-15 and np.abs(np.linalg.norm(first, axis=1) - 1).max() < 1e-15


def test_real_focal_check_keeps_a_subsequence():
    plain, checked = G.reference("fund"), G.reference("fund", True)
    assert (checked.counts <= plain.counts).all() and (checked.counts < plain.counts).any() and checked.counts.max() == 3
    for i in range(plain.B):
        kept = [m for m in range(plain.counts[i]) if any(np.array_equal(plain.models[i, m], c) for c in checked.models[i, : checked.counts[i]])]
        assert len(kept) == checked.counts[i]
        assert np.array_equal(plain.models[i, kept], checked.models[i, : checked.counts[i]])


def test_positions_are_the_draws_consumed_before_each_sample():
    """the device draws iteration i from (seed, positions[i]): restate that with the host compile of the device's sampler"""
    for name in ["abs", "rel", "fund", "hom"] + G.SMALL_SETS:
        r = G.reference(name)
        idx, pos, _ = HM.draw_samples(G.SEED, r.a.shape[0], G.K[r.kind], G.B_MAX)
        assert np.array_equal(idx, r.samples.astype(np.uint32)) and np.array_equal(pos, r.positions.astype(np.uint32))
    for name in G.SMALL_SETS:  # the samples that redraw consume more than K draws: as many as K draws of n collide, most of them for K >= 5
        r = G.reference(name)
        n, k = r.a.shape[0], G.K[r.kind]
        redraws = (np.diff(r.positions.astype(np.int64)) > k).mean()
        expected = 1.0 - np.prod((n - np.arange(k)) / n)
        assert abs(redraws - expected) < 0.05, (name, redraws, expected)
        assert redraws > (0.5 if k >= 5 else 0.2), (name, redraws)


def test_the_5_point_cases_cover_an_overflowing_and_a_fitting_pose_queue():
    """k_rel_poses queues up to 512 poses per workgroup of 256 iterations and writes the rest from its root loop"""
    totals = G.workgroup_pose_totals(G.rel_rich().counts)
    assert totals[0] > 512 and (totals[1:] < 512).any() and (totals[1:] > 0).any(), totals
    assert (G.workgroup_pose_totals(G.reference("rel").counts) < 512).all()  # the sampler's own order: the queued path alone
    # the same multiset of samples: a permutation
    assert np.array_equal(np.sort(G.rel_rich().counts), np.sort(G.reference("rel").counts))


def test_the_5_point_cases_cover_the_root_counts_the_bucket_sort_permutes():
    ec = G.essential_counts(G.reference("rel"))
    per_group = [set(ec[w:w + 256].tolist()) for w in range(0, G.B_MAX, 256)]
    assert any({0, 2, 4, 6} <= s for s in per_group), per_group
    assert {2, 4, 6} <= set(ec[:63].tolist())  # (the short cases permute as well)


def test_the_planted_samples_have_ten_and_eight_real_roots():
    """Mined on the CPU with the oracle: all 200 000 samples of the sampler streams of seeds 100 .. 179 on points("rel") (2500 each)
    were solved; 31 have 10 real roots, 495 have 8.  Twelve resp. eight of them are planted."""
    kind, a, b = G.points("rel")
    for rows, want in ((G.TEN_ROOT_SAMPLES, 10), (G.EIGHT_ROOT_SAMPLES, 8)):
        ref = G.Reference("rel", np.array(rows, dtype=np.uint64))
        assert (G.essential_counts(ref) == want).all()
    ec = G.essential_counts(G.many_roots())
    assert (ec == 10).sum() == 25 and (ec == 8).sum() == 25 and (ec < 8).sum() == 20


def test_the_p3p_cases_cover_the_solution_counts_and_nan_records():
    r = G.reference("abs")
    assert {0, 1, 2, 4} <= set(r.counts[:255].tolist())  # (every case from 255 iterations on)
    assert r.nan[:63].any() and r.nan[:1023].sum() > 50  # NaN poses of inconsistent samples (30 % outliers: a third of the samples)
    tot, nan = r.block_sums(G.B_MAX)
    assert len(tot) == 3 and (nan > 0).all()
    # a wavefront's candidates exceed 64 somewhere (two rounds of the collective second half) and stay below elsewhere
    per_wave = np.add.reduceat(r.counts.astype(np.int64), np.arange(0, G.B_MAX, 64))
    assert (per_wave > 64).any() and (per_wave <= 64).any()


def test_slot_limit_cases_do_overflow():
    for ref in (G.reference("rel"), G.rel_rich()):
        smax = int(ref.counts.max())
        assert smax >= 3 and 0 < (ref.counts == smax).sum() < ref.B


@pytest.mark.parametrize("name", G.HARD_SETS)
def test_hard_samples_on_the_host_compile_of_the_device_solver(name):
    """the planted degenerate samples through the device headers compiled for the host: the oracle's count, order and bits; and the
    flat isolation at the generator's capacities on their determinant polynomials"""
    r = G.hard_reference(name)
    if name in ("nan", "inf"):
        assert (r.samples == 0).any(axis=1).all() and r.counts.max() == 0  # the bad coordinate is in every sample: no model survives
    elif name == "coincident":
        assert ((r.samples == 0).any(axis=1) & (r.samples == 1).any(axis=1)).all()
        assert r.counts.max() >= 2
    else:
        assert r.counts.max() >= 2
    polys = []
    for i in range(r.B):
        first, second = r.sample_in[i, :5], r.sample_in[i, 5:]
        rec = HM.solve("rel", first, second)
        assert len(rec) == r.counts[i] and np.array_equal(rec[:, :7], r.models[i, : r.counts[i]], equal_nan=True), i
        polys.append(HM.rel5_poly(first, second))
    bad, first_bad, pending, leaves = HM.sturm10_flat_generator_caps(np.array(polys))
    assert bad == 0, first_bad
    assert pending <= 5 and leaves <= 12


def test_flat_isolation_at_the_generators_capacities_equals_the_recursion():
    """sturm_roots_deg10_flat on a work type with the list capacities of gen_rel.hip (6 intervals to bisect, 12 leaves as found; the
    host's default work type has 12 and 16) against sturm_roots_deg10: number, order and bits of the roots - on the determinant
    polynomials of the 5-point cases, on 10^5 random polynomials and on clustered ones.  The lists never get longer than the
    generator's comment says: at most five intervals wait to be bisected."""
    rs = np.random.RandomState(177)
    sets = []
    for ref in (G.reference("rel"), G.many_roots()):
        sets.append(np.array([HM.rel5_poly(ref.sample_in[i, :5], ref.sample_in[i, 5:]) for i in range(ref.B)]))
    sets.append(rs.randn(100000, 11) * 10.0 ** rs.uniform(-3, 3, (100000, 11)))
    clustered = []
    for _ in range(3000):  # 0 .. 10 real roots, close pairs and double roots (the narrow-interval branch), any scale
        nr = 2 * rs.randint(0, 6)
        roots = list(rs.randn(nr) * 10.0 ** rs.uniform(-2, 2))
        if nr >= 2 and rs.rand() < 0.5:
            roots[1] = roots[0] + 10.0 ** rs.uniform(-13, -3)
        if nr >= 4 and rs.rand() < 0.3:
            roots[3] = roots[2]
        p = np.poly1d([1.0])
        for x in roots:
            p *= np.poly1d([1.0, -x])
        for _ in range((10 - nr) // 2):
            u, v = rs.randn(2)
            p *= np.poly1d([1.0, -2 * u, u * u + v * v + 1e-3])
        clustered.append(p.coeffs[::-1] * 10.0 ** rs.uniform(-8, 8))
    sets.append(np.array(clustered))
    longest = 0
    for polys in sets:
        bad, first_bad, pending, leaves = HM.sturm10_flat_generator_caps(polys)
        assert bad == 0, (first_bad, polys[first_bad])
        assert pending <= 5 and leaves <= 12, (pending, leaves)
        longest = max(longest, pending)
    assert longest >= 3  # (the lists are exercised: several intervals did wait at once)
