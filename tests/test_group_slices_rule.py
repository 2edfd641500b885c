"""The slice count of a grouped scorer launch (driver_group.inc: group_score_slices), through pl_debug_group_slices.  No device.

A member's hypothesis stream is cut into `slices` workgroups per chunk of correspondences.  For absolute pose on the matrix
cores (k_score_mfma_g) the count follows the work of the whole launch: slices = clamp(ceil(W / launch_chunks), 1, solo), where
launch_chunks is the sum of the active members' chunks, W the target number of workgroups of a launch and `solo` the value a
member gets when it is alone in its launch - the rule every launch had before (restated below).  Every other scorer keeps
`solo` whatever the launch holds.  profiles/group_slices.md says where W comes from."""
import pytest

import poselib_amd as P
from poselib_amd import api

W = 3328  # target workgroups of a k_score_mfma_g launch (kGroupScoreWorkgroups)

N_POINTS = [1100, 5000, 20000]
ITERATIONS = [100, 5000, 100000]


def _chunks(n, per_lane=5):
    return max(1, -(-n // (64 * per_lane)))


def _solo_abs(n, iterations):
    """the rule of a member alone in its launch: one workgroup per 48 units of 64 expected hypotheses (P3P fills 1.3 of its 4
    slots per iteration: 1.5 per iteration expected), at most 1536 / chunks"""
    hcap = iterations * 4
    hexp = min(hcap, iterations + iterations // 2)
    return max(1, min((hexp // 64 + 47) // 48, 1536 // _chunks(n)))


def _launches(own):
    out = sorted({own * k for k in range(1, 65)} | {own + 1, own * 3 + 1, own * 17 - 1, own * 64 - 3})
    return [lc for lc in out if own <= lc <= 64 * own]


@pytest.mark.parametrize("n", N_POINTS)
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_absolute_pose_follows_the_work_of_the_launch(n, iterations):
    own = _chunks(n)
    solo = api.group_slices(P.KIND_ABS, n, iterations, own)
    assert solo == _solo_abs(n, iterations), (n, iterations, solo)
    prev = solo
    for lc in _launches(own):
        s = api.group_slices(P.KIND_ABS, n, iterations, lc)
        assert s >= 1, (n, iterations, lc, s)
        assert s <= solo, (n, iterations, lc, s, solo)
        assert s <= prev, (n, iterations, lc, s, prev)  # non-increasing in launch_chunks
        # ceil(W / lc) * lc < W + lc; one slice per (member, chunk) is the floor
        assert s * lc <= max(W + lc - 1, lc), (n, iterations, lc, s)
        assert s == max(1, min(-(-W // lc), solo)), (n, iterations, lc, s)
        prev = s


def test_the_flagship_launch_is_reduced_and_a_short_list_is_not():
    own = _chunks(5000)
    assert own == 16
    assert api.group_slices(P.KIND_ABS, 5000, 100000, own) == 49
    assert api.group_slices(P.KIND_ABS, 5000, 100000, 16 * own) == -(-W // 256) < 49
    # default options: a few hundred iterations per step - one slice however many members share the launch
    assert api.group_slices(P.KIND_ABS, 5000, 512, own) == api.group_slices(P.KIND_ABS, 5000, 512, 64 * own) == 1


@pytest.mark.parametrize("kind", ["KIND_REL", "KIND_FUND", "KIND_HOM", "KIND_RAD1D"])
def test_other_kinds_do_not_depend_on_the_launch(kind):
    k = getattr(P, kind)
    for n in N_POINTS + [500]:
        for iterations in ITERATIONS:
            own = api.group_slices(k, n, iterations, 1)
            assert own >= 1
            for lc in (2, 16, 64, 256, 1024, 4096):
                assert api.group_slices(k, n, iterations, lc) == own, (kind, n, iterations, lc)


def test_absolute_pose_below_the_matrix_core_size_keeps_its_rule():
    for iterations in ITERATIONS:
        own = api.group_slices(P.KIND_ABS, 1000, iterations, 1)  # fewer than 1024 correspondences: k_score_queue_g
        for lc in (4, 64, 1024):
            assert api.group_slices(P.KIND_ABS, 1000, iterations, lc) == own


def test_invalid_arguments_raise():
    with pytest.raises(P.PoseLibAmdError):
        api.group_slices(7, 1100, 100, 4)
    with pytest.raises(P.PoseLibAmdError):
        api.group_slices(P.KIND_ABS, 0, 100, 4)
