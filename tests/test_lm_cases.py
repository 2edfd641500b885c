"""The cases of the LM-kernel tests (tests/lm_cases.py) on the CPU: the conditions under which the device tests of
tests/test_gpu_lm_kernels.py mean something, checked on the reference (the oracle) and on the serial host model of the kernels
(hostmath) alone.  No device."""
import collections

import numpy as np
import pytest

import hostmath_lib as HM
import lm_cases as LC
from lm_cases import K_LM, K_LM2, K_LM_ORDERED

ROUTES = [(kind, route) for kind in LC.KINDS for route in (K_LM, K_LM_ORDERED, K_LM2) if route != K_LM2 or kind in LC.LM2_NS]


def all_cases():
    return LC.ordered_cases() + LC.tree_cases() + LC.lm2_cases()


def cases_of(kind, route):
    return [c for c in all_cases() if (c.kind, c.route) == (kind, route)]


def test_sizes_come_from_the_kernels_constants():
    assert (LC.SEQ, LC.STRIDE, LC.RING) == (256, 512, 448)
    ordered, tree = LC.ordered_cases(), LC.tree_cases()
    for kind in LC.KINDS:
        assert {c.n for c in ordered if (c.kind, c.route) == (kind, K_LM)} >= set(LC.SEQ_NS)
        assert {c.n for c in ordered if (c.kind, c.route) == (kind, K_LM_ORDERED)} >= set(LC.SEQ_NS + LC.RING_NS + LC.TREE_NS)
        assert {c.n for c in tree if c.kind == kind} >= set(LC.TREE_NS)
        assert all(c.n <= LC.SEQ for c in ordered if c.route == K_LM) and all(c.n > LC.SEQ for c in tree)
    for kind, ns in LC.LM2_NS.items():
        assert {c.n for c in LC.lm2_cases() if c.kind == kind} == set(ns) and min(ns) == LC.LM2_MIN[kind] and max(ns) <= 8192
    assert [LC.lm2_slices(n) for n in (2560, 2561, 3071, 3072, 8192)] == [5, 5, 5, 6, 16]
    assert len(set(all_cases())) == len(all_cases())


@pytest.mark.parametrize("kind,route", ROUTES)
def test_every_option_runs_and_steps_are_rejected(kind, route, capsys):
    cases = cases_of(kind, route)
    combos = {(c.loss, c.update, c.damping) for c in cases}
    if route != K_LM2:
        assert combos == set(LC.COMBINATIONS), "a loss / update / damping combination has no case"
        assert {c.max_iterations for c in cases} >= {0, 1, 25} and {c.stop for c in cases} >= set(LC.STOP_RULES)
        assert {c.mask for c in cases} >= {None, "ones", "block", "alternate"} and {c.start for c in cases} == set(LC.STARTS)
        # min-sample + 1 rows of more than 256: on k_lm_ordered and on k_lm's tree sums (up to 256 rows there is no such set)
        few = [c for c in cases if c.mask and c.mask.startswith("few")]
        assert {c.loss for c in few} >= {"CAUCHY", "TRUNCATED"} and all(c.n > LC.SEQ for c in few), (kind, route, few)
    else:
        assert {c.loss for c in cases} >= {"TRUNCATED", "TRUNCATED_LE_ZACH"} and "block" in {c.mask for c in cases}
    for loss in {c.loss for c in cases}:
        assert max(LC.oracle(c).iterations for c in cases if c.loss == loss) >= 2, (kind, route, loss)
    rejected = [c for c in cases if LC.oracle(c).invalid_steps >= 1]
    fused = [c for c in rejected if c.loss != "TRUNCATED_LE_ZACH"]
    assert len(rejected) >= 2 and len(fused) >= 1, (kind, route, len(rejected), len(fused))
    assert any(LC.oracle_accepts_after_a_rejection(c) for c in fused), "no step accepted after a rejection under a fused loss"
    assert all(np.isfinite(LC.oracle(c).model).all() for c in cases)
    if route == K_LM:  # (route 0 is two regimes: each of them has its rejected steps)
        for regime in ([c for c in rejected if c.n <= LC.SEQ], [c for c in rejected if c.n > LC.SEQ]):
            assert len(regime) >= 2 and any(LC.oracle_accepts_after_a_rejection(c) for c in regime if c.loss != "TRUNCATED_LE_ZACH")
    dropped = 0
    if route == K_LM2 or route == K_LM:
        candidates = [c for c in LC.tree_candidates() + LC.lm2_candidates() if (c.kind, c.route) == (kind, route)]
        dropped = len(candidates) - len([c for c in cases if c.n > LC.SEQ])
    with capsys.disabled():
        print(f"\nlm cases {kind} route {route}: {len(cases)} cases, {len(rejected)} with rejected steps ({len(fused)} under fused losses), "
              f"{dropped} candidates dropped for their sensitivity to the order of the sums")


def test_every_stop_rule_decides_its_case():
    seen = collections.Counter()
    for c in all_cases():
        if c.stop:
            with_rule, default = LC.oracle(c), LC.oracle(c._replace(stop=None))
            assert with_rule.iterations != default.iterations, (LC.case_id(c), with_rule.iterations)
            seen[(c.kind, c.route, c.stop)] += 1
    for kind in LC.KINDS:
        for route in (K_LM, K_LM_ORDERED):
            for stop in LC.STOP_RULES:
                assert seen[(kind, route, stop)] >= 1, (kind, route, stop)


def test_zero_weight_cases_hold_an_empty_and_a_full_block():
    """k_lm's queue of correspondences with a non-zero weight: beyond one stride of rows every unmasked case (and the masks that
    keep whole blocks) has a 64-row block from which nothing is kept at the start and one from which all 64 are - numpy's residuals,
    the rows a factor of 2 away from the threshold on either side"""
    seen = set()
    for c in all_cases():
        if c.loss in LC.ZERO_WEIGHT and c.n > LC.STRIDE and c.mask in (None, "ones", "block"):
            empty, full = LC.kept_blocks(c)
            assert empty >= 1 and full >= 1, (LC.case_id(c), empty, full)
            a, b, model, bo, _ = LC.inputs(c)
            r2 = LC.squared_residuals(c.kind, model, a, b)
            assert (r2[: LC.WAVE] < bo["loss_scale"] ** 2 / 2).all() and (r2[LC.WAVE: 2 * LC.WAVE] > 2 * bo["loss_scale"] ** 2).all()
            seen.add((c.kind, c.route))
    assert seen >= {(k, r) for k in LC.KINDS for r in (K_LM, K_LM_ORDERED)} | {(k, K_LM2) for k in LC.LM2_NS}


def test_masks():
    for c in all_cases():
        a, b, _, _, mask = LC.inputs(c)
        if c.mask == "ones":
            assert mask.all()
        elif c.mask == "block":
            zero = np.flatnonzero(mask == 0)
            assert len(zero) == LC.WAVE and zero[0] % LC.WAVE == 0 and (np.diff(zero) == 1).all()
        elif c.mask == "alternate":
            assert mask[::2].all() and not mask[1::2].any()
        elif c.mask and c.mask.startswith("few"):
            assert c.n > LC.SEQ and mask.sum() == LC.MIN_SAMPLE[c.kind] + 1


def _same(model, iterations, want):
    return iterations == want.iterations and np.array_equal(np.ravel(model), np.ravel(want.model))


def test_host_model_with_pow_equals_the_oracle_bit_for_bit():
    """today's standard: the kernels' arithmetic, serial on the host with glibc's pow, IS the reference - on every case, masks (the
    oracle on the compacted subset) and stop rules included"""
    for c in all_cases():
        model, it = LC.hostmath(c, device_cube=False)
        assert _same(model, it, LC.oracle(c)), (LC.case_id(c), it, LC.oracle(c).iterations)
        if c.mask == "ones":
            assert _same(model, it, LC.oracle(c._replace(mask=None))), LC.case_id(c)


def test_host_model_with_the_devices_cube_differs_only_after_a_differing_cube():
    """HM.lm(device_cube=True) is what k_lm_ordered computes.  It may differ from the oracle where the Nielsen update has cubed an
    argument at which lm_cube_fma and glibc's pow(x, 3) differ - nowhere else, never under FIXED_FACTOR (no cube), and in at most
    2 % of the NIELSEN cases."""
    nielsen = differing = 0
    for c in all_cases():
        model, it = LC.hostmath(c, device_cube=True)
        args = HM.lm_cube_args()
        same = _same(model, it, LC.oracle(c))
        if c.update == LC.FIXED_FACTOR:
            assert same and len(args) == 0, LC.case_id(c)
            continue
        nielsen += 1
        if not same:
            differing += 1
            assert (HM.lm_cube(args) != HM.glibc("pow3", args)).any(), LC.case_id(c)
    print(f"device cube: {differing} of {nielsen} NIELSEN cases differ from the oracle")
    assert differing <= 0.02 * nielsen, (differing, nielsen)


def test_the_cube_switch_of_the_host_build_is_live():
    """No case of the table cubes an argument at which the two forms differ, so the switch is checked directly: at such an argument
    (about one in a thousand) lm_cube of the host build returns lm_cube_fma's bits with the flag, pow's without, and records the
    argument.  A build without PL_LM_CUBE_HOST_SWITCH, or a flag that is not passed on, fails here."""
    x = np.random.RandomState(12).uniform(-1.0, 1.0, 200_000)
    fma, pw = HM.lm_cube(x), HM.glibc("pow3", x)
    differ = np.flatnonzero(fma != pw)
    assert 0 < len(differ) < 0.002 * x.size
    for i in differ[:20]:
        assert HM.lm_cube_switched(x[i], True) == fma[i] and HM.lm_cube_args().tolist() == [x[i]]
        assert HM.lm_cube_switched(x[i], False) == pw[i] and HM.lm_cube_args().tolist() == [x[i]]
    # and through the refinement: the flag reaches the LM's update (a NIELSEN case cubes once per accepted step, either way)
    c = next(c for c in LC.ordered_cases() if c.update == LC.NIELSEN and LC.oracle(c).iterations >= 3 and LC.oracle(c).invalid_steps == 0)
    for flag in (False, True):
        LC.hostmath(c, device_cube=flag)
        args = HM.lm_cube_args()
        assert 1 <= len(args) <= LC.oracle(c).iterations + 1 and (np.abs(args) < 10).all()


def test_tree_route_cases_do_not_depend_on_the_order_of_the_reference_sums():
    """k_lm beyond 256 rows and k_lm2 add in tree order, so their cases have to be insensitive to the order in the reference itself:
    on eight fixed permutations of the rows (lm_cases.PERMUTATIONS) the oracle takes the same number of iterations and its models agree within 1e-11 - two
    orders below the bound of the device tests.  At most a tenth of the candidates may fall to this."""
    candidates = LC.tree_candidates() + LC.lm2_candidates()
    kept = LC.tree_cases() + LC.lm2_cases()
    worst = max(LC.order_spread(c)[1] for c in kept)
    print(f"tree-route candidates: {len(candidates)}, dropped {len(candidates) - len(kept)}, largest spread kept {worst:.2e}")
    assert all(LC.order_stable(c) for c in kept) and worst <= LC.ORDER_TOL < LC.TREE_TOL / 99
    assert len(candidates) - len(kept) <= len(candidates) // 10
