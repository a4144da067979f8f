"""The launch planner of mrz_rzip_chunk (modern-rzip_amd/csrc/mrz_chunk_plan.h) without a device.

tests/c/plan_test.cpp drives the planner with a toy matcher that emits as many matches as the room rule allows for, under
every retirement schedule, list capacity and pass span, in provider mode and across a wide-to-deep hand-over; it is a
plain program (its own main, no HIP), built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_program(tmp_path):
    exe = str(tmp_path / "plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "modern-rzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "plan_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
