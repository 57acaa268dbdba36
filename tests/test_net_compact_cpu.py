"""The compacted drain of the delta network store (csrc/net_delta.h) on the host: a
stand-alone program, built with the host compiler, plays one wave's batch with the helpers
the kernel uses (the flags of a record word, the list entry, a group's slot from the four
lane masks, the mapping entry -> row, float4 column, in range) for Wn in {1, 2, 3, 16, 17,
64, 65, 128}, every N % 4 == 0 of that Wn (N % 16 in {0, 4, 8, 12}), both batch forms,
and random, sparse, all-clean, all-dirty, single-dirty-group, value-only and forced
batches. The stored float4s must be exactly those of the groups net_group_dirty<64> calls
dirty: each once, none outside its row, no slot past 255. No device and nothing loaded
into Python."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "net_delta", "net_compact_check.cpp")
INC = os.path.join(ROOT, "gym-flock_amd", "csrc")


def host_compiler():
    for cc in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")


def test_drained_float4s_are_the_dirty_groups(tmp_path):
    exe = str(tmp_path / "net_compact_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    # 6 values of Wn with three batch lengths, 2 with two chunks; 16 values of N each;
    # 3 kinds of 8 seeded batches and 4 kinds of one
    assert "batches=%d " % ((6 * 3 + 2 * 2) * 16 * (3 * 8 + 4)) in r.stdout
    assert "bad=0" in r.stdout
    m = re.search(r"stored=(\d+) max_slot=(\d+)", r.stdout)
    assert m and int(m.group(1)) > 0
    assert int(m.group(2)) == 255  # the all-dirty batch of 64 words fills the list, and no more
