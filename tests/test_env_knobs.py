"""The CGL_* environment variables the code reads are exactly the ones INTEGRATION.md documents.

Collected from text only: getenv("CGL_...") in cgl-gan_amd/csrc (*.hip, *.h) and os.environ ... "CGL_..." in
cgl-gan_amd/cglgan/*.py and bench.py, against the first column of the table under "Environment variables".
The switches of the removed GEMM / plan variants must not come back under their old names."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cgl-gan_amd")

REMOVED = {"CGL_SPLITK", "CGL_BN_FOLD", "CGL_XCD_BLOCK", "CGL_TWO_STREAMS", "CGL_GEMM_TILE", "CGL_BNB_FPW",
           "CGL_GEMM_PIPE"}

C_READ = re.compile(r'getenv\(\s*"(CGL_[A-Z0-9_]+)"')
# a variable name handed to getenv through a pointer (fuse_wgrad_adam picks one of two names)
C_NAME = re.compile(r'const char\*\s*\w+\s*=[^;]*?"CGL_[A-Z0-9_]+"[^;]*;')
PY_READ = re.compile(r'os\.environ[^\n"]*"(CGL_[A-Z0-9_]+)"')


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def names_read():
    names = set()
    csrc = os.path.join(PKG, "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        text = _read(path)
        names.update(C_READ.findall(text))
        for m in C_NAME.finditer(text):
            names.update(re.findall(r'"(CGL_[A-Z0-9_]+)"', m.group(0)))
    for path in sorted(glob.glob(os.path.join(PKG, "cglgan", "*.py"))) + [os.path.join(ROOT, "bench.py")]:
        names.update(PY_READ.findall(_read(path)))
    return names


def names_documented():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    m = re.search(r"^## [^\n]*Environment variables[^\n]*\n(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert m, "INTEGRATION.md has no 'Environment variables' section"
    rows = re.findall(r"^\|\s*`(CGL_[A-Z0-9_]+)`\s*\|([^|\n]*)\|([^|\n]*)\|([^|\n]*)\|\s*$", m.group(1), re.M)
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)), "a variable is listed twice"
    kinds = {"diagnostic", "off-switch", "opt-in", "configuration"}
    for name, default, selects, kind in rows:
        assert default.strip() and selects.strip(), f"{name}: default and meaning must be filled in"
        assert kind.strip() in kinds, f"{name}: kind {kind.strip()!r} is not one of {sorted(kinds)}"
    return set(names)


def test_env_knobs_match_the_documented_table():
    read, documented = names_read(), names_documented()
    assert len(read) > 20          # the patterns still find the code's reads
    assert read - documented == set(), "read by the code but missing from INTEGRATION.md's table"
    assert documented - read == set(), "listed in INTEGRATION.md's table but read by no code"
    assert read & REMOVED == set(), "a removed variant's switch is read again"
    assert documented & REMOVED == set()
