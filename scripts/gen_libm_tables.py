#!/usr/bin/env python3
"""Generates poselib_amd/csrc/pl_libm_tables.h: the tables behind pl_cos / pl_acos / pl_atan2 / pl_tan (pl_libm.h), i.e.
behind glibc's IBM Accurate Mathematical Library routines (sysdeps/ieee754/dbl-64/s_sin.c, e_asin.c, e_atan2.c, s_tan.c),
from FIRST PRINCIPLES:

  sin / cos table   x_k = k / 128, k = 0 .. 127:  sin(x_k), cos(x_k) as double-double (hi = nearest double, lo = nearest
                    double of the remainder)                                                     [s_sin.c __sincostab]
  inverse roots     1 / sqrt(m) at the midpoints of 64 sub-intervals of [1/2, 1) and of [1, 2), 14 decimals
                                                                                                  [e_asin.c inroot]
  asin table        glibc's asincos.tbl: per interval (width 2^-8) of [1/8, 31/32) the midpoint x0, 6 .. 10 polynomial
                    coefficients and asin(x0) in two parts.  x0, c1, c2, asin(x0) follow from first principles, the
                    higher coefficients are IBM's minimax-adjusted values - constants of the published algorithm that
                    cannot be re-derived - and are read from the libm of this image (glibc 2.35, LGPL-2.1+), see
                    extract_asncs().  Run in a container with that glibc; the generated header is committed.
  atan table        glibc's uatan.tbl `cij`: per interval (width 2^-8) of [1/16, 1] a point x0 near the interval's middle -
                    IBM moved it until atan(x0) is a double to 58 bits and more -, atan(x0), and the coefficients c1 .. c5
                    of the expansion around x0.  atan(x0) and c1 = 1 / (1 + x0^2) are checked against
                    first principles; the points x0 and c2 .. c5 cannot be re-derived and are read from the libm of this
                    image, see extract_uatan().                                                  [e_atan2.c, s_atan.c]
  tan table         glibc's utan.tbl `xfg`: per interval (width 2^-8) of [0.0608, 0.787] a point x0 chosen the same way,
                    tan(x0) and cot(x0) (checked against first principles), see extract_utan().              [s_tan.c]

The first two are computed with 90-digit decimal arithmetic, nothing is read from a libm for them.
tests/test_libm_vs_glibc.py then checks pl_cos / pl_acos bit for bit against the host's libm on millions of arguments.
"""
import os
import sys
from decimal import Decimal, getcontext

getcontext().prec = 90
D = Decimal


def hexf(v: float) -> str:
    return float.hex(v)


def dd(v):  # double-double split of a Decimal
    hi = float(v)
    lo = float(v - D(hi))
    return hi, lo


def sin_cos(x):
    x2 = x * x
    t, c, k = D(1), D(1), 0
    while abs(t) > D(10) ** -85:
        k += 2
        t = -t * x2 / (D(k - 1) * D(k))
        c += t
    t, s, k = x, x, 1
    while abs(t) > D(10) ** -85:
        k += 2
        t = -t * x2 / (D(k - 1) * D(k))
        s += t
    return s, c


def sqrt_dec(v):
    return v.sqrt()


GLIBC_LIBM = "/lib/x86_64-linux-gnu/libm.so.6"
ASNCS_DOUBLES = 2568  # 96 rows of 11, 64 of 12, 44 of 13, 8 of 14, 4 of 15


def extract_asncs(libm_path=GLIBC_LIBM):
    """glibc's asincos.tbl (`asncs`, sysdeps/ieee754/dbl-64/asincos.tbl, LGPL-2.1+) as published in the libm of this
    image (glibc 2.35): per interval of the piecewise expansion of asin {midpoint x0, c1 .. cn, asin(x0) low part,
    asin(x0) high part, two entries the acos path does not read}.  x0, c1, c2 and asin(x0) are what first principles
    give (checked below), but c3 .. cn are IBM's minimax-adjusted coefficients (they differ from the Taylor
    coefficients by 1e-11 .. 1e-5 relative) and cannot be re-derived - they are constants of the published algorithm,
    like the polynomial of s_cbrt.c.  Located by the table's first two entries (x0 = 1/8 + 1/512, c1 = 1/sqrt(1 - x0^2))."""
    import struct

    blob = open(libm_path, "rb").read()
    x0 = D(1) / 8 + D(1) / 512
    key = struct.pack("<2d", float(x0), float(D(1) / (1 - x0 * x0).sqrt()))
    at = blob.find(key)
    assert at >= 0, "asncs table not found in " + libm_path
    T = struct.unpack("<%dd" % ASNCS_DOUBLES, blob[at:at + 8 * ASNCS_DOUBLES])
    nxt = blob.find(key, at + 1)
    while nxt >= 0:  # (every multiarch variant of e_asin.c carries its own copy: they must be the same table)
        assert blob[nxt:nxt + 8 * ASNCS_DOUBLES] == blob[at:at + 8 * ASNCS_DOUBLES]
        nxt = blob.find(key, nxt + 1)
    # sanity against first principles: every row's x0 is its interval's midpoint and c1 = asin'(x0)
    pos, idx = 0, 0
    for cnt, n in ((96, 6), (64, 7), (44, 8), (8, 9), (4, 10)):
        for _ in range(cnt):
            if idx < 32:
                mid = D(1) / 8 + D(2 * idx + 1) / 512
            elif idx < 96:
                mid = D(1) / 4 + D(2 * (idx - 32) + 1) / 512
            else:
                mid = D(1) / 2 + D(2 * (idx - 96) + 1) / 512
            assert T[pos] == float(mid), (idx, T[pos], float(mid))
            c1 = float(D(1) / (1 - mid * mid).sqrt())  # (the table's value is within an ulp of the nearest double)
            assert abs(T[pos + 1] - c1) <= 4e-16 * c1, idx
            pos += n + 5
            idx += 1
    assert pos == ASNCS_DOUBLES
    return T


def atan_dec(x):
    n = 0
    while abs(x) > D(1) / 64:  # atan(x) = 2 atan(x / (1 + sqrt(1 + x^2)))
        x = x / (1 + (1 + x * x).sqrt())
        n += 1
    x2, t, s, k = x * x, x, x, 1
    while abs(t) > D(10) ** -85:
        k += 2
        t = -t * x2
        s += t / k
    return s * (2 ** n)


UATAN_ROWS, UTAN_ROWS = 241, 186  # i = round(256 u) - 16, u in [1/16, 1]; i = trunc(256 w - 15.5), w in (0.0608, 0.787]


def _find_rows(blob, stride, rows, fits):
    """Every 8-aligned place of `blob` where a table of `rows` rows of `stride` doubles starts whose first row passes
    fits(row) - glibc's tables carry no symbol in a stripped libm, so they are found by what they must contain."""
    import struct

    hits = []
    for o in range(0, len(blob) - 8 * stride * rows + 1, 8):
        if blob[o + 6:o + 8] != b"\xb0\x3f":  # (top 16 bits of a double in [1/16, 1/8))
            continue
        row = struct.unpack_from("<%dd" % stride, blob, o)
        if fits(row):
            hits.append(o)
    return hits


def _same_copies(blob, hits, nbytes, what):
    assert hits, what + " not found"
    for h in hits[1:]:  # (every translation unit and multiarch variant carries its own copy: they must be the same table)
        assert blob[h:h + nbytes] == blob[hits[0]:hits[0] + nbytes], what
    return hits[0]


def extract_uatan(libm_path=GLIBC_LIBM):
    """glibc's uatan.tbl (`cij`, sysdeps/ieee754/dbl-64/uatan.tbl, LGPL-2.1+) as published in the libm of this image
    (glibc 2.35): rows {x0, atan(x0), c1, c2, c3, c4, c5}.  Found by its first row (x0 within 2e-3 of 1/16, then atan(x0)
    and 1 / (1 + x0^2)); every row is then checked: x0 within 2^-9 of (i + 16) / 256, atan(x0) the nearest double and in fact
    within 2^-58 relative, c1 = 1 / (1 + x0^2) within an ulp of first principles."""
    import math
    import struct

    blob = open(libm_path, "rb").read()

    def fits(r):
        return abs(r[0] - 0.0625) < 2e-3 and abs(r[1] - math.atan(r[0])) < 1e-16 and abs(r[2] - 1 / (1 + r[0] * r[0])) < 1e-15

    nb = 8 * 7 * UATAN_ROWS
    at = _same_copies(blob, _find_rows(blob, 7, UATAN_ROWS, fits), nb, "uatan.tbl")
    T = struct.unpack("<%dd" % (7 * UATAN_ROWS), blob[at:at + nb])
    for i in range(UATAN_ROWS):
        x0, a, c1 = (D(v) for v in T[7 * i:7 * i + 3])
        assert abs(x0 - D(i + 16) / 256) < D(2) ** -9, i
        exact = atan_dec(x0)
        assert float(exact) == T[7 * i + 1] and abs(a - exact) < exact * D(2) ** -58, i
        e1 = 1 / (1 + x0 * x0)
        assert abs(c1 - e1) <= e1 * D(2) ** -52, i
    return T


def extract_utan(libm_path=GLIBC_LIBM):
    """glibc's utan.tbl (`xfg`, sysdeps/ieee754/dbl-64/utan.tbl, LGPL-2.1+) as published in the libm of this image: rows
    {x0, tan(x0), cot(x0), low part of cot(x0)}; the first three are returned (the path restated here reads no more).  Every
    row is checked: x0 within 2^-12 of (i + 16) / 256, tan(x0) the nearest double and within 2^-58 relative, cot(x0) the
    nearest double."""
    import math
    import struct

    blob = open(libm_path, "rb").read()

    def fits(r):
        return (abs(r[0] - 0.0625) < 1e-6 and abs(r[1] - math.tan(r[0])) < 1e-16 and abs(r[2] * r[1] - 1.0) < 1e-15
                and abs(r[3]) < 1e-15)

    nb = 8 * 4 * UTAN_ROWS
    at = _same_copies(blob, _find_rows(blob, 4, UTAN_ROWS, fits), nb, "utan.tbl")
    T = struct.unpack("<%dd" % (4 * UTAN_ROWS), blob[at:at + nb])
    out = []
    for i in range(UTAN_ROWS):
        x0 = D(T[4 * i])
        assert abs(x0 - D(i + 16) / 256) < D(2) ** -12, i
        s, c = sin_cos(x0)
        assert float(s / c) == T[4 * i + 1] and abs(D(T[4 * i + 1]) - s / c) < (s / c) * D(2) ** -58, i
        assert float(c / s) == T[4 * i + 2], i
        out += T[4 * i:4 * i + 3]
    return out


def main(out_path):
    lines = ["// GENERATED by scripts/gen_libm_tables.py - do not edit.  Tables of pl_cos / pl_acos / pl_atan2 / pl_tan (pl_libm.h), computed from",
             "// first principles with 80-digit arithmetic; see the generator for what each table holds.",
             "#pragma once", "namespace pl {", ""]
    lines.append("// sin(k / 128), cos(k / 128) as double-double: {sin hi, sin lo, cos hi, cos lo}")
    lines.append("PL_TABLE double kSinCosTab[128][4] = {")
    for k in range(128):
        s, c = sin_cos(D(k) / 128)
        sh, sl = dd(s)
        ch, cl = dd(c)
        lines.append("    {%s, %s, %s, %s}," % (hexf(sh), hexf(sl), hexf(ch), hexf(cl)))
    lines.append("};")
    flat = list(extract_asncs())
    lines.append("")
    lines.append("// glibc 2.35 asincos.tbl `asncs` (LGPL-2.1+; constants of the published algorithm, see extract_asncs in the")
    lines.append("// generator): rows {x0, c1 .. cn, asin(x0) lo, asin(x0) hi, -, -} of 11 (n = 6: 96 rows), 12 (64), 13 (44), 14 (8), 15 (4) entries")
    lines.append("PL_TABLE double kAsinRows[%d] = {" % len(flat))
    for i in range(0, len(flat), 4):
        lines.append("    " + ", ".join(hexf(v) for v in flat[i:i + 4]) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// 1 / sqrt(m) at the midpoints of 64 sub-intervals of [1/2, 1) and 64 of [1, 2), 14 decimals (e_asin.c inroot)")
    lines.append("PL_TABLE double kInvRoot[128] = {")
    vals = []
    for i in range(128):
        m = D(1) / 2 + D(2 * i + 1) / 256 if i < 64 else D(1) + D(2 * (i - 64) + 1) / 128
        v = (D(1) / sqrt_dec(m)).quantize(D(10) ** -14)
        vals.append(float(v))
    for i in range(0, 128, 4):
        lines.append("    " + ", ".join(hexf(v) for v in vals[i:i + 4]) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// glibc 2.35 uatan.tbl `cij` (LGPL-2.1+; constants of the published algorithm, see extract_uatan in the generator):")
    lines.append("// rows {x0, atan(x0), c1 .. c5} for x0 near (i + 16) / 256, i = 0 .. 240")
    ua = list(extract_uatan())
    lines.append("PL_TABLE double kAtanRows[%d][7] = {" % UATAN_ROWS)
    for i in range(0, len(ua), 7):
        lines.append("    {" + ", ".join(hexf(v) for v in ua[i:i + 7]) + "},")
    lines.append("};")
    lines.append("")
    lines.append("// glibc 2.35 utan.tbl `xfg` (LGPL-2.1+, see extract_utan): rows {x0, tan(x0), cot(x0)} for x0 near (i + 16) / 256, i = 0 .. 185")
    ut = list(extract_utan())
    lines.append("PL_TABLE double kTanRows[%d][3] = {" % UTAN_ROWS)
    for i in range(0, len(ut), 3):
        lines.append("    {" + ", ".join(hexf(v) for v in ut[i:i + 3]) + "},")
    lines.append("};")
    lines.append("")
    lines.append("} // namespace pl")
    open(out_path, "w").write("\n".join(lines) + "\n")
    return flat, vals


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "poselib_amd", "csrc", "pl_libm_tables.h"))
