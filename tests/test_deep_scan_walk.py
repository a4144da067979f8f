"""The deep engine's walk of one run by one wave (mrz_deep_scan, modern-rzip_amd/csrc/mrz_seq_deep.hip) without a device.

tests/c/deep_scan_test.cpp compiles the engine source against the wave64 emulator's header twice -- as built (the next
group's loads ahead of the fold, quiet groups passed with one ballot) and with -DMRZ_DEEP_SCAN_NO_AHEAD
-DMRZ_DEEP_SCAN_NO_QUIET (the plain loop) -- and compares every field of the lane's record on seeded hand-built tables:
runs of 1 to 40 groups, the first empty slot at every position, tag-equal entries and chain-limit evictions in late
groups, due and lower-ranked stops early, late and nowhere, displacement, runs over the table's end, continuation scans
taken up inside groups that the full scan passed.  No GPU- or emulator-tier input reaches the skip at the masks a few MB
give (runs are shorter than one group there).  It is a plain program (its own main), built here with MRZ_DEEP_GROUP 2
(the emulator tier's) and 8 (the product's), and once more with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "deep_scan_test.cpp")
# (the emulator build's shape of the engine: Makefile, EMUFLAGS)
FLAGS = ["-std=c++17", "-g", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-Wno-strict-aliasing",
         "-DMRZ_HELPER_WGS=0", "-DMRZ_WIDE_WAVES=2", "-DMRZ_DEEP_WAVES=1", "-DMRZ_DEEP_LANES=24", "-DMRZ_DEEP_HELP_MIN=6",
         "-DMRZ_EMU_LDS_PER_BLOCK", "-DMRZ_POOL=40", "-x", "c++",
         "-I" + os.path.join(ROOT, "tests", "emu"), "-I" + os.path.join(ROOT, "modern-rzip_amd", "csrc")]
OLD = ["-DDST_OLD", "-DMRZ_DEEP_SCAN_NO_AHEAD", "-DMRZ_DEEP_SCAN_NO_QUIET"]


def _build(tmp_path, group, extra):
    flags = FLAGS + ["-DMRZ_DEEP_GROUP=%d" % group] + extra
    old, new, exe = (str(tmp_path / n) for n in ("old.o", "new.o", "deep_scan_test"))
    subprocess.run(["g++"] + flags + OLD + ["-c", SRC, "-o", old], check=True)
    subprocess.run(["g++"] + flags + ["-c", SRC, "-o", new], check=True)
    subprocess.run(["g++"] + [f for f in extra if f.startswith("-fsanitize")] + [old, new, "-o", exe], check=True)
    return exe


def _run(exe, cases):
    r = subprocess.run([exe, "--cases", str(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "deep_scan_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout)


@pytest.mark.parametrize("group,cases", [(2, 20000), (8, 6000)])
def test_walk_as_built_against_plain_loop(tmp_path, group, cases):
    _run(_build(tmp_path, group, ["-O1"]), cases)


def test_walk_under_sanitizers(tmp_path):
    exe = _build(tmp_path, 2, ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _run(exe, 5000)
