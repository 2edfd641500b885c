"""Every POSELIB_AMD_* environment switch the library or its Python binding reads is documented in INTEGRATION.md, and
INTEGRATION.md documents no switch that the code no longer reads."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"\bPOSELIB_AMD_[A-Z0-9_]+")


def names_in(paths):
    found = set()
    for p in paths:
        with open(p, encoding="utf-8") as f:
            found |= set(NAME.findall(f.read()))
    return found


def test_documented_switches_match_the_code():
    csrc = os.path.join(ROOT, "poselib_amd", "csrc")
    sources = [p for ext in ("hip", "cc", "h", "inc") for p in glob.glob(os.path.join(csrc, "*." + ext))]
    in_code = names_in(sources + glob.glob(os.path.join(ROOT, "poselib_amd", "*.py")))
    documented = names_in([os.path.join(ROOT, "INTEGRATION.md")])
    assert "POSELIB_AMD_NO_MFMA" in in_code  # (the scan sees the sources)
    assert in_code - documented == set(), "read by the code but not documented in INTEGRATION.md"
    assert documented - in_code == set(), "documented in INTEGRATION.md but not read by the code"
