"""Generates tests/golden/tlsh.json from the reference's own TLSH library (vendor/tlsh, built as ar-mrzip builds it:
256 buckets, 3 checksum bytes), for mrz_tlsh_batch.  The three library sources are compiled with a small extern "C"
shim (below) into oracle/_ref/libtlsh_ref.so and driven exactly as compute_checksums drives them
(ar-mrzip/ar-mrzip.cpp:137-172): update in 4096-byte pieces, final(buf, 0, 0), getHash(buf, 137, 0) -- into a buffer
large enough to see all 138 characters it writes.  Recorded: the 138-character string (or "") of every seeded input of
tests/_ar_ref.py, and the smallest length of every length code.
Run:  python tests/golden/make_tlsh_golden.py [reference tree, default /root/reference]"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _ar_ref as R  # noqa: E402

SHIM = r"""
#include <string.h>
#include "tlsh.h"
unsigned char l_capturing(unsigned int len);
extern "C" int ref_tlsh(const unsigned char *data, unsigned long long n, char *out256) {
    Tlsh t;
    unsigned long long at = 0;
    while (n - at > 4096) {
        t.update(data + at, 4096);
        at += 4096;
    }
    t.final(data + at, (unsigned int)(n - at), 0);
    memset(out256, 0, 256);
    t.getHash(out256, TLSH_STRING_BUFFER_LEN, 0);
    return TLSH_STRING_BUFFER_LEN;
}
extern "C" int ref_len_code(unsigned int len) { return l_capturing(len); }
"""


def build(ref):
    out_dir = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(out_dir, exist_ok=True)
    shim = os.path.join(out_dir, "tlsh_shim.cpp")
    with open(shim, "w") as f:
        f.write(SHIM)
    so = os.path.join(out_dir, "libtlsh_ref.so")
    tl = os.path.join(ref, "vendor", "tlsh")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", os.path.join(tl, "include"), "-o", so, shim] +
                   [os.path.join(tl, "src", s) for s in ("tlsh.cpp", "tlsh_impl.cpp", "tlsh_util.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.ref_tlsh.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    lib.ref_len_code.argtypes = [ctypes.c_uint]
    return lib


def digest(lib, data):
    buf = ctypes.create_string_buffer(256)
    assert lib.ref_tlsh(data, len(data), buf) == 137
    s = buf.value.decode()
    assert len(s) in (0, 138), len(s)
    return s


def main():
    lib = build(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
    # the smallest length of every code: the code never falls as the length grows
    top = 4224281216
    assert lib.ref_len_code(top) == 169 and lib.ref_len_code(0) == 0
    min_len = []
    for code in range(170):
        lo, hi = 0, top
        while lo < hi:
            mid = (lo + hi) // 2
            if lib.ref_len_code(mid) >= code:
                hi = mid
            else:
                lo = mid + 1
        assert lib.ref_len_code(lo) == code and (lo == 0 or lib.ref_len_code(lo - 1) == code - 1)
        min_len.append(lo)
    out = {
        "_source": "vendor/tlsh, BUCKETS_256 CHECKSUM_3B, g++ -std=c++17 -O2; update in 4096-byte pieces, final, "
                   "getHash(buf, 137, 0)",
        "lvalue_min_len": min_len,
        "small": {name: digest(lib, data) for name, data in R.small_inputs().items()},
        "big_member": digest(lib, R.big_member()),
        "mixed_batch": [digest(lib, d) for d in R.mixed_batch()],
        "thresholds": {str(n): digest(lib, R.threshold_message(n))
                       for code, m in enumerate(min_len) if 50 < m <= 1 << 20 for n in (m - 1, m)},
    }
    with open(os.path.join(HERE, "tlsh.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("small:", len(out["small"]), "of which without a digest:", sum(not v for v in out["small"].values()),
          "| mixed:", len(out["mixed_batch"]), "without:", sum(not v for v in out["mixed_batch"]),
          "| thresholds:", len(out["thresholds"]))


if __name__ == "__main__":
    main()
