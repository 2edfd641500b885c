#!/usr/bin/env python
"""Generates tests/golden/focal_templates_ref_v1.json - digests of the reference's two focal-length elimination templates
(solvers/p35pf.cc, solvers/relpose_6pt_focal.cc): for every coefficient formula the SHA-256 of its terms (multiplier and
variable indices, in the written order), and the SHA-256 of the template's (row, column, coefficient) positions.  Only
digests are stored, nothing of the sources themselves.  tests/test_focal_templates.py checks the generator's tables
(scripts/gen_focal_templates.py) against them where the reference's sources are absent.  Re-run where they are present:
    python tests/golden/make_focal_template_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_focal_templates as T  # noqa: E402


def main():
    assert os.path.isdir(T.REF), "the digests are recorded from the reference's sources"
    out = {"provenance": "digests of the reference's sources (solvers/p35pf.cc, solvers/relpose_6pt_focal.cc), "
                         "parsed by tests/test_focal_templates.py; written by tests/golden/make_focal_template_digests.py"}
    for which in ("p35pf", "six"):
        out[which] = T._canonical(*T._reference_form(which))
    with open(os.path.join(HERE, "focal_templates_ref_v1.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
