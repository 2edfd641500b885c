"""The coefficient / elimination-template tables of the two focal-length solvers (poselib_amd/csrc/pl_focal_templates.h,
oracle/src/focal_templates.inc) are GENERATED from the solvers' equations by scripts/gen_focal_templates.py.  CPU tests:
  * the committed tables are what the generator writes (nobody edited them by hand, product and oracle hold the same data);
  * every one of the reference's 235 + 280 coefficient formulas (solvers/p35pf.cc:89-520, solvers/relpose_6pt_focal.cc:58-1030)
    is, term for term and in the written order, what the generator derived from the equations, and the reference's index tables
    place the same coefficients at the same matrix positions - the restatement is the reference's template, not merely a solver
    with the same roots.  Where the reference's sources are present they are parsed and compared directly; everywhere the
    generator's terms and positions are checked against digests recorded from those sources
    (tests/golden/focal_templates_ref_v1.json, written by tests/golden/make_focal_template_digests.py)."""
import hashlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gen_focal_templates as G  # noqa: E402

REF = "/root/reference/PoseLib/solvers"
GOLDEN = os.path.join(ROOT, "tests", "golden", "focal_templates_ref_v1.json")


def test_committed_tables_are_the_generators_output(tmp_path):
    tabs = [G.p35_tables(), G.six_tables()]
    body = "\n\n".join(G.emit(t, "") for t in tabs)
    product = open(os.path.join(ROOT, "poselib_amd", "csrc", "pl_focal_templates.h")).read()
    oracle = open(os.path.join(ROOT, "oracle", "src", "focal_templates.inc")).read()
    assert body in product and body in oracle
    assert [len(t["coeffs"]) for t in tabs] == [235, 280]
    assert [(t["nrows"], t["ncols"], len(t["entries"])) for t in tabs] == [(25, 35, 475), (31, 46, 814)]


def _formulas(src, decl, end):
    blk = src[src.index(decl):src.index(end)]
    out = {}
    for stmt in blk.split(";"):
        m = re.match(r"\s*coeffs\[(\d+)\]\s*=\s*(.*)$", stmt.strip(), re.S)
        if m:
            out[int(m.group(1))] = re.sub(r"\s+", " ", m.group(2))
    return out


def _terms(expr):
    """-> [(multiplier, (indices ...))] in the written order; pow(d[i], n) = n times the index i"""
    out = []
    for sign, body in re.findall(r"([+-]?)\s*((?:[^+-])+)", expr):
        body = body.strip()
        if not body:
            continue
        mult, idx = (-1 if sign == "-" else 1), []
        for f in (x.strip() for x in body.split("*")):
            if re.fullmatch(r"\d+", f):
                mult *= int(f)
            elif (m := re.fullmatch(r"d\[(\d+)\]", f)):
                idx.append(int(m.group(1)))
            elif (m := re.fullmatch(r"std::pow\(d\[(\d+)\], (\d)\)", f)):
                idx += [int(m.group(1))] * int(m.group(2))
            else:
                raise ValueError(f)
        out.append((mult, tuple(idx)))
    return out


def _table(src, name):
    m = re.search(name + r"\[\]\s*=\s*\{(.*?)\}", src, re.S)
    return [int(x) for x in m.group(1).replace("\n", " ").split(",")]


def _digest(obj):
    """SHA-256 (first 16 hex digits) of a term list / position list in a canonical JSON form"""
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()[:16]


def _canonical(formulas, entries):
    """{"coeffs": {k: digest of [[multiplier, [indices ...]], ...]}, "entries": digest of the sorted (row, col, coefficient)}"""
    return {"n_coeffs": len(formulas),
            "coeffs": {str(k): _digest([[m, list(idx)] for m, idx in terms]) for k, terms in sorted(formulas.items())},
            "n_entries": len(entries), "entries": _digest(sorted(list(e) for e in entries))}


def _reference_form(which):
    """the reference's coefficient formulas {k: terms} and template positions {(row, col, coefficient)}, parsed from its sources"""
    if which == "p35pf":
        src = open(os.path.join(REF, "p35pf.cc")).read()
        rows = 25
        formulas = _formulas(src, "double coeffs[235];", "static const int coeffs0_ind")
    else:
        src = open(os.path.join(REF, "relpose_6pt_focal.cc")).read()
        rows = 31
        formulas = _formulas(src, "Eigen::VectorXd coeffs(280);", "static const int coeffs0_ind")
    ref_entries = set()
    for ci, pos in zip(_table(src, "coeffs0_ind"), _table(src, "C0_ind")):
        ref_entries.add((pos % rows, pos // rows, ci))
    for ci, pos in zip(_table(src, "coeffs1_ind"), _table(src, "C1_ind")):
        ref_entries.add((pos % rows, rows + pos // rows, ci))
    return {k: _terms(expr) for k, expr in formulas.items()}, ref_entries


def _generated_form(which):
    tb = G.p35_tables() if which == "p35pf" else G.six_tables()
    formulas = {k: [(tb["coeffs"][k][t], t) for t in sorted(tb["coeffs"][k], key=G.term_key)] for k in range(len(tb["coeffs"]))}
    return formulas, set(tb["entries"])


@pytest.mark.parametrize("which", ["p35pf", "six"])
def test_generated_templates_are_the_references(which):
    mine, entries = _generated_form(which)
    if os.path.isdir(REF):  # the reference's sources themselves
        formulas, ref_entries = _reference_form(which)
        assert len(formulas) == len(mine)
        for k, terms in formulas.items():
            assert terms == mine[k], (which, k)
        assert ref_entries == entries
    rec = json.load(open(GOLDEN))[which]  # what those sources held when the digests were recorded
    got = _canonical(mine, entries)
    assert got["n_coeffs"] == rec["n_coeffs"] and got["n_entries"] == rec["n_entries"]
    for k, d in rec["coeffs"].items():
        assert got["coeffs"][k] == d, (which, k)
    assert got["entries"] == rec["entries"]
