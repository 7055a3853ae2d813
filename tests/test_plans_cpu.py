"""The plan registry of a handle (dl-unet_amd/csrc/plans.hpp: which training forwards await their backward, which finished
ones are still kept, who leaves first) on the CPU.  tests/host/plans_main.cpp is a stand-alone program with its own main and
an int payload; it is compiled here with the host compiler, with the address and undefined-behaviour sanitizers where the
compiler has them, and run as a child process.  Nothing is loaded into this interpreter and no preload is set."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "plans_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
CASES = ["replacement at the same address", "one pending entry survives 16 finished ones", "one pending entry survives 17 finished ones",
         "one pending entry survives 1000 finished ones", "17 and PENDING_MAX pending at once", "finished entries leave oldest first",
         "forget, and addresses never inserted", "four threads, disjoint addresses", "plans OK"]


def compilers():
    seen = []
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        p = shutil.which(c) if c else None
        if p and p not in seen:
            seen.append(p)
    return seen


def compile_program(out):
    """(compiler, flags) of the first build that works: every compiler with the sanitizers first, then without."""
    tried = []
    # (the sanitizer runtimes linked statically where the compiler can: the program then needs nothing of its environment)
    for flags in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE + ["-static-libsan"], SANITIZE, []):
        for cxx in compilers():
            cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags + [SRC, "-o", out]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode == 0 and os.path.exists(out):
                return cxx, flags
            tried.append("%s: %s" % (" ".join(cmd), r.stderr[-2000:]))
    pytest.fail("no host compiler built tests/host/plans_main.cpp:\n" + "\n".join(tried))


def test_plan_registry_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "plans_main")
    cxx, flags = compile_program(exe)
    print("built with %s %s" % (cxx, " ".join(flags) or "(no sanitizer: none of the compilers here accepts the flags)"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout, r.stderr)
    assert r.stdout.splitlines() == CASES, r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
