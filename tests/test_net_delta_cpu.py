"""The delta network store's group-flag helper (csrc/net_delta.h) on the host: a
stand-alone program around it, built with the host compiler, checks every (old nibble,
new nibble, value changed) case of 16-byte groups and 10^6 seeded random (old word, new
word, value changed) cases of all three group sizes against the definition: a group is
stored when its new bits differ from its recorded bits, or when it has a new bit set and
the row's value changed. No device and nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "net_delta", "net_delta_check.cpp")
INC = os.path.join(ROOT, "gym-flock_amd", "csrc")


def host_compiler():
    for cc in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")


def test_group_flags_match_their_definition(tmp_path):
    exe = str(tmp_path / "net_delta_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "cases16=%d" % (16 * 16 * 16 * 2 * 2) in r.stdout
    assert "cases_wide=1000000" in r.stdout and "bad=0" in r.stdout
