"""Run by tests/test_gpu_lm_kernels.py in a process of its own with POSELIB_AMD_LATENCY_MODE=1 in its environment (the setting is read
once per process): the k_lm2 cases of one kind (tests/lm_cases.py lm2_cases) through Problem.refine.

Every case first asserts pl_debug_lm_route - route 2 and the slice count clamp(n / 512, 2, 16) -, then the tree-result conditions:
the oracle's iteration count, the oracle's model within 1e-9 (sign included), the same bits from a second run.  The same case with
max_iterations = 33, outside the gate's window, must report route 0; its bits go to the parent, which runs k_lm itself.
Prints one JSON line: {"worst": largest distance, "ran": [case ids], "route0": {case id: [hex bits, iterations]}}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import lm_cases as LC  # noqa: E402
import poselib_amd as P  # noqa: E402

OUTSIDE_THE_WINDOW = LC.LM2_MAX_ITERATIONS + 1


def main(kind):
    assert os.environ.get("POSELIB_AMD_LATENCY_MODE") == "1"
    P.set_lm_mode(2 if kind == "fund" else 0)  # fundamental matrices: k_lm2 needs k_lm's mode (the default orders their sums)
    cases = LC.lm2_cases(kind)
    assert cases, kind
    n_min = LC.LM2_MIN[kind]
    kid = LC.KIND_ID[kind]
    assert P.lm_route(kid, n_min - 1, 25) == (LC.K_LM, 0) and P.lm_route(kid, n_min, 25) == (LC.K_LM2, LC.lm2_slices(n_min))
    assert P.lm_route(kid, n_min, 0) == (LC.K_LM, 0) and P.lm_route(kid, n_min, 1)[0] == LC.K_LM2
    assert P.lm_route(kid, n_min, LC.LM2_MAX_ITERATIONS)[0] == LC.K_LM2 and P.lm_route(kid, n_min, OUTSIDE_THE_WINDOW) == (LC.K_LM, 0)
    assert P.lm_route(LC.KIND_ID["rel"], 8192, 25) == (LC.K_LM, 0)  # relative poses never take k_lm2
    worst, ran, route0 = 0.0, [], {}
    for c in cases:
        assert P.lm_route(kid, c.n, c.max_iterations) == (LC.K_LM2, LC.lm2_slices(c.n)), LC.case_id(c)
        want = LC.oracle(c)
        got, it = LC.refine_on_device(P, c)
        dist = LC.distance(kind, got, want.model)
        print(f"{LC.case_id(c)}: iterations {it} (oracle {want.iterations}, {want.invalid_steps} rejected), distance {dist:.2e}", flush=True)
        assert it == want.iterations, (LC.case_id(c), it, want.iterations)
        assert dist <= LC.TREE_TOL, (LC.case_id(c), dist)
        again, it2 = LC.refine_on_device(P, c)
        assert it2 == it and again.tobytes() == got.tobytes(), LC.case_id(c)
        worst = max(worst, dist)
        ran.append(LC.case_id(c))
    for c in (cases[0], next(x for x in cases if x.mask)):
        assert P.lm_route(kid, c.n, OUTSIDE_THE_WINDOW) == (LC.K_LM, 0)
        got, it = LC.refine_on_device(P, c, OUTSIDE_THE_WINDOW)
        route0[LC.case_id(c)] = [np.ascontiguousarray(got).tobytes().hex(), it]
    print("lm2 child ok " + json.dumps({"worst": worst, "ran": ran, "route0": route0}))


if __name__ == "__main__":
    main(sys.argv[1])
