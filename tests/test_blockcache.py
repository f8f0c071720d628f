"""The policy of the device allocator's cache -- csrc/blockcache.h: how a request is rounded, which free block serves it, what a release
gives back and what goes when the free blocks exceed their cap -- through tests/native/blockcache_harness.cpp: g++ and that header
alone, made-up pointers, no GPU.  devmem.hip makes the runtime calls around it.

The harness is built twice, plain and with the address and undefined-behaviour sanitizers (a stand-alone program), and every group of
checks runs in both."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("rounding", "take", "release", "evict", "drain")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blockcache") / ("blockcache_harness_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "native", "blockcache_harness.cpp"), "-o", exe])

    def run(case):
        return subprocess.run([exe, case], capture_output=True, text=True, timeout=60)
    return run


@pytest.mark.parametrize("case", CASES)
def test_the_cache_policy(harness, case):
    r = harness(case)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr

