"""The LM kernels option by option (-m gpu): k_lm, k_lm_ordered and k_lm2 of kernels.hip through Problem.refine, on the cases of
tests/lm_cases.py - all six losses x both lambda updates x both dampings, rough starts from which the reference rejects steps, every
stop rule, max_iterations 0 and 1, masks, and point counts on the edges of the kernels' structures (the 256-row switch to tree sums,
the 512-thread stride, one ring round of the ordered kernel's producers, the gate and the slice rule of k_lm2).

Every case first asserts pl_debug_lm_route, so a refinement that silently took another kernel fails.  Where the kernel adds in the
reference's order (k_lm_ordered, k_lm up to 256 rows) model and iteration count must EQUAL the serial host model of the kernels with
the device's cube (hostmath lm(device_cube=True)) - no exceptions; where it adds in tree order (k_lm beyond 256 rows, k_lm2) the
iteration count must equal the oracle's, the model agree within 1e-9, sign included, and a second run give the same bits.
tests/test_lm_cases.py checks on the CPU that the cases reject steps, that the stop rules decide, and that the tree-route cases do
not depend on the order of the sums in the reference itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lm_cases as LC
from lm_cases import K_LM, K_LM2, K_LM_ORDERED

pytestmark = pytest.mark.gpu

_report = {"worst": {}, "ran": set()}  # what test_zz_report prints: profiles/lm_kernel_tests.md is its output


def _note(c, route, dist=None):
    _report["ran"].add((c.kind, route, c.loss, "FIXED_FACTOR" if c.update else "NIELSEN", "MARQUARDT" if c.damping else "LEVENBERG",
                        c.stop or "-", c.mask or "-"))
    if dist is not None:
        key = (c.kind, route)
        _report["worst"][key] = max(_report["worst"].get(key, 0.0), dist)


def _mode_of(kind, route):
    """the LM mode (pl_set_lm_mode) under which a refinement of `kind` takes `route`: 1 orders every sum; 0 leaves k_lm to poses and
    homographies; fundamental matrices reach k_lm in mode 2 only"""
    return 1 if route == K_LM_ORDERED else 2 if kind == "fund" else 0


class _lm_mode:
    def __init__(self, gpu, mode):
        self.gpu, self.mode = gpu, mode

    def __enter__(self):
        self.prev = self.gpu.set_lm_mode(self.mode)

    def __exit__(self, *exc):
        self.gpu.set_lm_mode(self.prev)
        return False


@pytest.mark.parametrize("route", [K_LM, K_LM_ORDERED])
@pytest.mark.parametrize("kind", LC.KINDS)
def test_ordered_results_equal_the_host_model(gpu, kind, route):
    """k_lm up to 256 rows and k_lm_ordered at every size: the bits and the iteration count of the serial host model with the device's
    cube, on every case; against the oracle the cap of tests/test_lm_cases.py (2 % of the NIELSEN cases, no FIXED_FACTOR case)"""
    cases = [c for c in LC.ordered_cases() if (c.kind, c.route) == (kind, route)]
    assert len(cases) >= 40
    nielsen = off_oracle = 0
    with _lm_mode(gpu, _mode_of(kind, route)):
        for c in cases:
            assert gpu.lm_route(LC.KIND_ID[kind], c.n, c.max_iterations) == (route, 0), LC.case_id(c)
            got, it = LC.refine_on_device(gpu, c)
            want, want_it = LC.hostmath(c, device_cube=True)
            assert it == want_it and np.array_equal(got, want), (LC.case_id(c), it, want_it, LC.distance(kind, got, want))
            if c.mask == "ones":  # a mask of ones is no mask, bit for bit
                bare, bare_it = LC.refine_on_device(gpu, c._replace(mask=None))
                assert bare_it == it and np.array_equal(bare, got), LC.case_id(c)
            ref = LC.oracle(c)
            same = it == ref.iterations and np.array_equal(got, ref.model)
            assert same or c.update == LC.NIELSEN, LC.case_id(c)
            nielsen += c.update == LC.NIELSEN
            off_oracle += not same
            _note(c, route)
    assert off_oracle <= 0.02 * nielsen, (off_oracle, nielsen)


@pytest.mark.parametrize("kind", LC.KINDS)
def test_tree_results_agree_with_the_oracle(gpu, kind):
    """k_lm beyond 256 rows (tree sums; the queue of correspondences with a non-zero weight under the truncated losses), in mode 2
    and - poses and homographies - in mode 0: the oracle's iteration count, its model within 1e-9, the same bits twice - and the
    bits and the iteration count recorded in tests/golden/lm_tree_bits_v1.json (lm_cases.assert_pinned)"""
    cases = [c for c in LC.tree_cases() if c.kind == kind]
    assert len(cases) >= 40
    first = {}
    for mode in ((2,) if kind == "fund" else (0, 2)):
        with _lm_mode(gpu, mode):
            for c in cases:
                assert gpu.lm_route(LC.KIND_ID[kind], c.n, c.max_iterations) == (K_LM, 0), LC.case_id(c)
                want = LC.oracle(c)
                got, it = LC.refine_on_device(gpu, c)
                dist = LC.distance(kind, got, want.model)
                assert it == want.iterations, (LC.case_id(c), it, want.iterations, dist)
                assert dist <= LC.TREE_TOL, (LC.case_id(c), dist)
                again, it2 = LC.refine_on_device(gpu, c)  # (and the other mode runs the same kernel: the same bits again)
                assert it2 == it and np.array_equal(again, got) and np.array_equal(first.setdefault(c, got), got), LC.case_id(c)
                LC.assert_pinned("k_lm", LC.case_id(c), got, it)  # (the recorded bits: tests/golden/lm_tree_bits_v1.json)
                if c.mask == "ones":
                    bare, bare_it = LC.refine_on_device(gpu, c._replace(mask=None))
                    assert bare_it == it and np.array_equal(bare, got), LC.case_id(c)
                _note(c, K_LM, dist)
    print(f"k_lm tree sums, {kind}: {len(cases)} cases, largest distance from the oracle {_report['worst'][kind, K_LM]:.2e}")


def test_multi_workgroup_kernel_in_fresh_processes(gpu):
    """k_lm2 (tests/lm_kernels_child.py, POSELIB_AMD_LATENCY_MODE=1 read once per process): homographies at 2560, 2561, 3071 and 3072
    rows, fundamental matrices at 2560 (LM mode 2), absolute poses at 8192 - route 2 and the slice count asserted, then the
    tree-result conditions.  max_iterations = 33 leaves the gate's window: the child reports route 0 and its bits are k_lm's, which
    this process - without the latency setting - computes itself.  A failing child ends the test: no other is started."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, POSELIB_AMD_LATENCY_MODE="1")
    by_id = {LC.case_id(c): c for c in LC.lm2_candidates()}
    for kind, limit in (("hom", 120), ("fund", 120), ("abs", 180)):  # seconds: start-up, the oracle's runs, some fifty refinements
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "lm_kernels_child.py"), kind], capture_output=True, text=True,
                           timeout=limit, cwd=root, env=env)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("lm2 child ok ")]
        assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
        out = json.loads(line[0][len("lm2 child ok "):])
        assert set(out["ran"]) == {LC.case_id(c) for c in LC.lm2_cases(kind)}
        assert {"TRUNCATED", "TRUNCATED_LE_ZACH"} <= {by_id[i].loss for i in out["ran"]} and any(by_id[i].mask for i in out["ran"])
        assert sum(LC.oracle(by_id[i]).invalid_steps >= 1 for i in out["ran"]) >= 2
        for i in out["ran"]:
            _note(by_id[i], K_LM2, out["worst"])
        with _lm_mode(gpu, _mode_of(kind, K_LM)):
            for i, (bits, it) in out["route0"].items():
                c = by_id[i]
                assert gpu.lm_route(LC.KIND_ID[kind], c.n, LC.LM2_MAX_ITERATIONS + 1) == (K_LM, 0)
                assert gpu.lm_route(LC.KIND_ID[kind], c.n, c.max_iterations) == (K_LM, 0)  # (no latency setting here)
                mine, my_it = LC.refine_on_device(gpu, c, LC.LM2_MAX_ITERATIONS + 1)
                assert my_it == it and np.ascontiguousarray(mine).tobytes().hex() == bits, i
        print(f"k_lm2, {kind}: {len(out['ran'])} cases, largest distance from the oracle {out['worst']:.2e}")


def test_zz_report(gpu):
    """prints (pytest -s) what the tests above ran: profiles/lm_kernel_tests.md holds this output of a whole run of the module"""
    print("\n| kind | kernel | largest distance from the oracle |\n|---|---|---|")
    for (kind, route), worst in sorted(_report["worst"].items()):
        print(f"| {kind} | {('k_lm, more than 256 rows', '', 'k_lm2')[route]} | {worst:.2e} |")
    print("\n| kind | route | loss | update | damping | stop rule | mask |\n|---|---|---|---|---|---|---|")
    for row in sorted(_report["ran"]):
        print("| " + " | ".join(str(v) for v in row) + " |")
