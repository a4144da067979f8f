"""The host-only halves of the ar-mrzip index (modern-rzip_amd/csrc/mrz_ar_index.h, mrz_tlsh_tables.h) without a
device.

tests/c/ar_index_test.cpp drives the collapse of duplicates, the size arithmetic, the ARZIP metadata writer and the
parser -- round trip, every truncation, bit flips in every metadata byte, the offset + size limit -- and the host half
of the TLSH digest (length code at all 170 thresholds, ratio arithmetic, hex layout); it is a plain program (its own
main, no HIP), built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ar_index_program(tmp_path):
    exe = str(tmp_path / "ar_index_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "modern-rzip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "ar_index_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "ar_index_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
