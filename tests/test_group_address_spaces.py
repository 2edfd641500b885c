"""No flat memory instruction in the group kernels of pipeline.hip (no device needed; skipped where hipcc is missing).

A kernel that reads through a pointer it fetched from a device-resident table gets flat_* instructions unless the pointer went
through pl_global.h's globalised() first.  scripts/isa_memory_ops.py compiles a file device-only with the
Makefile's flags and counts the memory instructions of every kernel by address space; pipeline.hip compiles in a few seconds,
the other files stay with the script and the committed table (profiles/group_address_spaces.md)."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_memory_ops  # noqa: E402

GROUP_KERNELS = 11  # k_sample_delta_g<3, 4, 5, 7>, k_sample_orbit_g<true, false>, k_compact2_g, k_finalize2_g, k_records_g,
                    # k_gather_shadow16_g, k_prepare_g


def _is_group(row):  # (the symbol is the mangled name: k_compact2_gEPK..., k_sample_delta_gILi3EE...)
    return re.search(r"k_[a-z0-9_]+_g[EI]", row["symbol"]) is not None


@pytest.fixture(scope="module")
def pipeline_kernels():
    if isa_memory_ops.find_hipcc() is None:
        pytest.skip("hipcc not found")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_memory_ops.py"), "--json", "pipeline"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)["pipeline"]


def test_group_kernels_of_pipeline_hip_have_no_flat_access(pipeline_kernels):
    group = [r for r in pipeline_kernels if r["kernel"] and _is_group(r)]
    assert len(group) == GROUP_KERNELS, [r["name"] for r in group]
    for r in group:
        assert (r["flat_ld"], r["flat_st"], r["flat_at"]) == (0, 0, 0), r
        assert r["glob_ld"] + r["glob_st"] + r["glob_at"] > 0, r  # (the counter does see the kernel's accesses)


def test_single_problem_kernels_are_the_yardstick(pipeline_kernels):
    """the single-problem forms take their pointers as kernel arguments: global from the start"""
    solo = [r for r in pipeline_kernels if r["kernel"] and not _is_group(r)]
    assert solo
    for r in solo:
        assert (r["flat_ld"], r["flat_st"], r["flat_at"]) == (0, 0, 0), r
