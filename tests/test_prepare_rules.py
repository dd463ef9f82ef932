"""The host rules of the prepare path (csrc/prepare_rules.h) on their own: a stand-alone host program
(tests/native/prepare_rules_check.cpp) applies them to the cases below, built plain and with AddressSanitizer and
UndefinedBehaviorSanitizer linked into the program itself.  The expected values are written out here, the tolerance as the
expression ctx_prepare_tableau and the batched scale kernel each carried before they shared problem_tol:
    tol = tol_rel * sqrt(max(y'y, 0)), or 1e-300 when that is not > 0."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partitionedls.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "prepare_rules_check.cpp")

NAN, INF = math.nan, math.inf
SUBNORMAL = 5e-324


def old_tol(tol_rel, yy):
    t = tol_rel * math.sqrt(yy if yy > 0.0 else 0.0)
    return t if t > 0.0 else 1e-300


def gram(M, **bad):
    """(M + 2)^2 Gram of ones, row by row, with the entries named "i_j" replaced"""
    n = M + 2
    g = [1.0] * (n * n)
    for at, v in bad.items():
        i, j = (int(x) for x in at.split("_"))
        g[i * n + j] = v
    return [M, n] + g


REF = 3.0
EDGE = 1e-14 * abs(REF)                     # the product the rule compares with: d == EDGE is a dead column

# name -> (rule, arguments, expected output words)
CASES = {
    "tol: y'y = 0": ("tol", [1e-11, 0.0], [1e-300]),
    "tol: y'y negative": ("tol", [1e-11, -4.0], [1e-300]),
    "tol: y'y subnormal": ("tol", [1e-11, SUBNORMAL], [old_tol(1e-11, SUBNORMAL)]),
    "tol: y'y subnormal, product underflows": ("tol", [1e-200, SUBNORMAL], [1e-300]),
    "tol: y'y = 1": ("tol", [1e-11, 1.0], [1e-11]),
    "tol: y'y = 1e300": ("tol", [1e-11, 1e300], [old_tol(1e-11, 1e300)]),
    "tol: tol_rel = 0": ("tol", [0.0, 1.0], [1e-300]),
    "tol: tol_rel = 0, y'y = 0": ("tol", [0.0, 0.0], [1e-300]),
    "live: d = 0": ("live", [0.0, REF], [0]),
    "live: d < 0": ("live", [-1.0, REF], [0]),
    "live: d = 1e-14 ref": ("live", [EDGE, REF], [0]),
    "live: the next double above": ("live", [math.nextafter(EDGE, INF), REF], [1]),
    "live: negative ref counts by magnitude": ("live", [EDGE, -REF], [0]),
    "diag: clean": ("diag", gram(3), [1]),
    "diag: NaN on a feature's diagonal": ("diag", gram(3, **{"1_1": NAN}), [0]),
    "diag: Inf at y'y": ("diag", gram(3, **{"4_4": INF}), [0]),
    "diag: NaN only on the ones column's diagonal": ("diag", gram(3, **{"3_3": NAN}), [1]),
    "diag: NaN off the diagonal": ("diag", gram(3, **{"0_1": NAN, "4_0": NAN}), [1]),
    # partials per block: negative flag, non-finite flag, sum, zero rows
    "fold: a negative weight in the last block": ("fold", [3, 0, 0, 1.5, 0, 0, 0, 2.5, 1, 1, 0, -0.5, 0], [0, 1, 3.5, 1]),
    "fold: an Inf": ("fold", [2, 0, 1, 2.0, 0, 0, 0, 1.0, 0], [1, 0, 3.0, 0]),
    "fold: all zeros": ("fold", [2, 0, 0, 0.0, 256, 0, 0, 0.0, 44], [0, 0, 0.0, 300]),
    "fold: a sum that overflows": ("fold", [2, 0, 0, 1e308, 0, 0, 0, 1e308, 0], [0, 0, INF, 0]),
    "fold: zero rows over several blocks": ("fold", [4, 0, 0, 1.0, 7, 0, 0, 2.0, 0, 0, 0, 3.0, 256, 0, 0, 0.25, 1], [0, 0, 6.25, 264]),
}
assert old_tol(1e-11, SUBNORMAL) > 1e-300 and old_tol(1e-11, 1e300) == 1e-11 * 1e150


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


def _line(rule, args):
    ints = {"diag": 2, "fold": 1}.get(rule, 0)            # leading integer arguments; the rest go as hex doubles
    return " ".join([rule] + [str(a) for a in args[:ints]] + [float(a).hex() for a in args[ints:]])


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def results(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prepare_rules") / "prepare_rules_check")
    cxx = _compiler()
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, SRC]
    if request.param == "sanitized":
        cmd[5:5] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        # the sanitizer runtimes linked into the program itself (clang's default; gcc needs to be told)
        if "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
            cmd += ["-static-libasan", "-static-libubsan"]
    subprocess.run(cmd, check=True)
    lines = [_line(rule, args) for rule, args, _ in CASES.values()]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = run.stdout.strip().split("\n")
    assert len(out) == len(CASES)
    return dict(zip(CASES, out))


@pytest.mark.parametrize("name", list(CASES))
def test_prepare_rule(results, name):
    rule, _, want = CASES[name]
    got = results[name].split()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, float):
            assert float.fromhex(g) == w, (g, w)         # bit for bit (no NaN among the expected values)
        else:
            assert int(g) == w
