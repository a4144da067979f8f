"""The archive framing under the compress-side entry points (modern-rzip_amd/csrc/mrz_framing.h) without a device.

tests/c/framing_test.cpp drives the sizing rules, the stream cutter, the chunk writer in its -n and -l shapes, the
record writers, the two forms of the chunk loop's input and the archive sink, against the oracle's independent
restatement (oracle/mrz_oracle.c: mrzo_plan, mrzo_frame, mrzo_compress_stream, mrzo_rzip_chunk) and back through the
parser of mrz_archive.h; it is a plain program (its own main, no HIP), built with the address and undefined-behaviour
sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_framing_program(tmp_path):
    exe, obj = str(tmp_path / "framing_test"), str(tmp_path / "mrz_oracle.o")
    subprocess.run(["gcc", "-std=c11"] + SAN + ["-c", os.path.join(ROOT, "oracle", "mrz_oracle.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "modern-rzip_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "c", "framing_test.cpp"), obj,
                    "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "framing_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
