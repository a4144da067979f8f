"""The host-only halves of the member extractor without a device.

tests/c/range_plan_test.cpp drives mrz_arc_ranges (modern-rzip_amd/csrc/mrz_archive.h): the clipping of a list of ranges
against the chunks of an archive, the placement of the parts in the packed output, the early stop and the verdicts.
tests/c/ar_head_test.cpp drives mrz_ar_read_prefix (mrz_ar_index.h): the ARZIP parser over the head of an archive whose
payload the caller does not hold.  Both are plain programs (their own main, no HIP), built with the address and
undefined-behaviour sanitizers.  tests/c/capi_extract_test.c, the C99 caller of the four new entry points, is checked
against the public headers here; it runs against the library in the GPU tier."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["range_plan_test", "ar_head_test"])
def test_host_program(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "modern-rzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and name + " ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_c99_caller_is_valid_against_the_headers():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "capi_extract_test.c")], check=True)
