"""The near-tie rule (csrc/near_tie.h) on its own: a stand-alone host program built with AddressSanitizer and
UndefinedBehaviorSanitizer feeds install_near_ties the cases below; the expected lists are written out here.

The rule: of the candidates (objective, reference pattern) those with another pattern than the winner's whose
objective^2 is <= lim2 are kept, sorted by (objective, pattern), duplicates once, at most `cap`; cand = winner
first, then the kept pairs; near_pat = the kept patterns; near_for = the winner's pattern."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partitionedls.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "near_tie_check.cpp")

EDGE = 2.0                                  # lim2 = 4.0: objective 2.0 sits exactly on the window's edge
OUT = math.nextafter(EDGE, math.inf)        # ... and the next double lies outside it

# name -> (lim2, cap, winner, candidates, expected near_pat, expected cand after the winner)
CASES = {
    "equal objectives, different reference indices":
        (4.0, 3, (1.0, 5), [(1.0, 9), (1.0, 7), (1.0, 6)], [6, 7, 9], [(1.0, 6), (1.0, 7), (1.0, 9)]),
    "window edge kept, just outside dropped":
        (4.0, 3, (1.0, 0), [(OUT, 1), (EDGE, 2)], [2], [(EDGE, 2)]),
    "duplicates":
        (4.0, 3, (1.0, 0), [(1.5, 4), (1.5, 4), (1.25, 3), (1.5, 4), (1.25, 3)], [3, 4], [(1.25, 3), (1.5, 4)]),
    "more than three inside the window":
        (4.0, 3, (1.0, 0), [(1.9, 11), (1.1, 12), (1.7, 13), (1.3, 14), (1.5, 15)], [12, 14, 15],
         [(1.1, 12), (1.3, 14), (1.5, 15)]),
    "the winner repeated among the candidates":
        (4.0, 3, (1.0, 8), [(1.0, 8), (1.2, 3), (1.0, 8), (1.4, 8)], [3], [(1.2, 3)]),
    "empty list":
        (4.0, 3, (1.0, 2), [], [], []),
}


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("near_tie") / "near_tie_check")
    cxx = _compiler()
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, "-o", exe, SRC]
    # the sanitizer runtimes linked into the program itself (clang's default; gcc needs to be told)
    ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    if "clang" not in ver:
        cmd += ["-static-libasan", "-static-libubsan"]
    subprocess.run(cmd, check=True)
    lines = []
    for lim2, cap, (wo, wp), cands, _, _ in CASES.values():
        words = [lim2.hex(), str(cap), wo.hex(), str(wp), str(len(cands))]
        for o, q in cands:
            words += [o.hex(), str(q)]
        lines.append(" ".join(words))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = run.stdout.strip().split("\n")
    assert len(out) == len(CASES)
    return dict(zip(CASES, out))


@pytest.mark.parametrize("name", list(CASES))
def test_near_tie_rule(results, name):
    _, _, winner, _, want_near, want_cand = CASES[name]
    near_for, near_pat, cand = (part.split() for part in results[name].split("|"))
    assert [int(near_for[0])] == [winner[1]]
    assert [int(q) for q in near_pat] == want_near
    got = [(float.fromhex(o), int(q)) for o, q in (w.rsplit(":", 1) for w in cand)]
    assert got == [winner] + want_cand
