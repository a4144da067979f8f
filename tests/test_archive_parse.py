"""The archive framing under the three runzip entry points (modern-rzip_amd/csrc/mrz_archive.h) without a device.

tests/c/archive_test.cpp builds small archives with a framing writer of its own and drives the header, the block-chain
walker, the chunk cursor, the record-length walk and the range arithmetic: accepted layouts, a table of refusals with
the codes the entry points returned before the parser existed, every truncation and every mutation of a framing byte;
it is a plain program (its own main, no HIP), built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_archive_program(tmp_path):
    exe = str(tmp_path / "archive_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "modern-rzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "archive_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "archive_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
