"""The stream kernel's task queue arithmetic (blu_internal.h: task_deal / task_of_claim) on the CPU.

tests/task_claim_host.cpp — a program with its own main — is compiled with the address and undefined-behaviour sanitizers,
their runtimes linked statically, and run as a subprocess in the inherited environment; nothing is loaded into Python.  It
walks every block's queue in claim order for n_queries in 0 .. 20 000 and around n_waves * 64 * k +- 65 (k <= 4), for grids
of 11, 12, 16, 131 * 12, 256 * 11, 256 * 12 and 256 * 16 waves, and requires that the ranges partition the table, that the
tail pieces keep the tail rule (multiples of 8 queries, at least 16, but for the very last) and that they are, entry for
entry, what the strided loop dealt — cut at n_queries in exactly the tables whose last whole-round task is a partial one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "task_claim_host.cpp")


def _hip_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


def _compilers():
    """Host compilers to try, in order: the helper's header pulls in hip_runtime.h, which any C++17 host compiler reads."""
    out = []
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c) if c else None
        if p and p not in out:
            out.append(p)
    return out


def test_queues_partition_the_table_as_the_strided_deal_did(tmp_path):
    inc = _hip_include()
    assert inc is not None and _compilers(), "the helper's header needs the HIP headers and a host C++ compiler, as the build does"
    exe = str(tmp_path / "task_claim_host")
    flags = ["-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
             "-I" + inc, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "blutils_amd", "csrc"), SRC, "-o", exe]
    errors = []
    for cxx in _compilers():
        # the sanitizer runtimes are linked INTO the program (clang does so by itself), so it runs in whatever environment it is given
        static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
        p = subprocess.run([cxx] + static + flags, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode == 0:
            break
        errors.append(cxx + ":\n" + p.stdout[-3000:])
    else:
        pytest.fail("task_claim_host.cpp does not build:\n" + "\n".join(errors))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "task_claim_host ok" in r.stdout, r.stdout[-4000:]
