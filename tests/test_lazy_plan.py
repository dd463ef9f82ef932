"""The LDS plan of the deferred-update sweep kernel (csrc/lazy_plan.h) on its own: a stand-alone host program
(tests/native/lazy_plan_check.cpp) prints the library's plan of every leading dimension ld = 2 .. 1025, built plain and with
AddressSanitizer and UndefinedBehaviorSanitizer linked into the program itself.  It is held against the Python restatement that
tests/test_gpu_lazy_plans.py draws its table of cases from, so the table cannot drift away from the kernel's classes unnoticed, and
against what the kernel needs of a plan: blocks of at least 2 pivots, a pool of at least three blocks (a block needs Rcur + 2 m <= rows),
and dynamic plus static LDS (4228 B: s_basm, s_inf[16], s_viol[1024]) within the 160 KB of a workgroup."""
import os
import shutil
import subprocess

import pytest

from test_gpu_lazy_plans import lazy_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partitionedls.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "lazy_plan_check.cpp")
STATIC_LDS = 4228                                          # s_basm (4), s_inf (16 x 8), s_viol (1024 x 4) of sweep_lazy_kernel


def _compiler():
    for cxx in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plans(request, tmp_path_factory):
    """ld -> (threads, mb, rows, shmem) as the library plans it, None where it refuses"""
    exe = str(tmp_path_factory.mktemp("lazy_plan") / "lazy_plan_check")
    cxx = _compiler()
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, SRC]
    if request.param == "sanitized":
        cmd[5:5] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        # the sanitizer runtimes linked into the program itself (clang's default; gcc needs to be told)
        if "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
            cmd += ["-static-libasan", "-static-libubsan"]
    subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = {}
    for line in run.stdout.strip().split("\n"):
        w = line.split()
        out[int(w[0])] = None if w[1] == "refused" else tuple(int(x) for x in w[1:])
    assert sorted(out) == list(range(2, 1026))
    return out


def test_the_restated_plan_is_the_library_s(plans):
    for ld, plan in plans.items():
        assert plan == lazy_plan(ld), ld


def test_every_plan_fits_the_kernel(plans):
    for ld in range(2, 1025):
        assert plans[ld] is not None, "ld = %d is refused" % ld
        threads, mb, rows, shmem = plans[ld]
        assert threads == (512 if ld <= 512 else 1024) and threads >= ld        # one thread per tableau row
        assert mb >= 2 and (rows >= 3 * mb or mb == 2), (ld, mb, rows)
        assert mb <= (16 if threads == 512 else 8) and rows <= 64
        assert shmem + STATIC_LDS <= 160 * 1024, (ld, shmem)
