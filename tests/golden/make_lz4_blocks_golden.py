"""Generates tests/golden/lz4_blocks.json from the system liblz4.so.1 (1.9.3 in the build image), for the LZ4 block
decoder: two LZ4_compress_HC (level 7) payloads -- output of a compressor this library does not restate -- and
liblz4's verdict on every hand-built, malformed and fuzzed block of tests/_lz4_blocks.py, with the sha256 of what it
decoded.  A verdict is "LZ4_decompress_safe(src, dst, c_len, u_len) == u_len", which is what the reference demands
(src/stream.c:465-477).  Blocks in which the walk meets an offset of 0 are flagged: liblz4 accepts them and copies
bytes it has not written, this library rejects them, so their expected verdict is reject whatever liblz4 says.
Verdicts are strings of 0 / 1 in the order of the case lists; the outputs of the 2000 fuzz cases are pinned by one
digest per group of 100 and those of the hand-built cases by one digest (_lz4_blocks.group_digest: verdict and sha256 of
every case in turn), which keeps the file near its neighbours' size.  Run:  python tests/golden/make_lz4_blocks_golden.py"""
import base64
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import _lz4_blocks as B  # noqa: E402
from tests import _util  # noqa: E402


def hc_inputs():
    text = _util.zipf_text(4096, seed=3)
    return {"text_4096": text, "text_4096x2": text * 2}


def main():
    z = ctypes.CDLL("liblz4.so.1")
    z.LZ4_versionString.restype = ctypes.c_char_p

    def verdict(src, u_len):
        """(accepted, bytes, holds an offset 0)"""
        why = []
        B.ref_decode(src, u_len, why)
        dst = ctypes.create_string_buffer(u_len + 64)
        ok = z.LZ4_decompress_safe(src, dst, len(src), u_len) == u_len
        if why:
            return False, b"", True
        return ok, dst.raw[:u_len] if ok else b"", False

    out = {"_liblz4": z.LZ4_versionString().decode(), "hc": {}}
    for name, data in hc_inputs().items():
        dst = ctypes.create_string_buffer(len(data) + len(data) // 255 + 16)
        n = z.LZ4_compress_HC(data, dst, len(data), len(dst), 7)
        assert n > 0
        out["hc"][name] = {"payload": base64.b64encode(dst.raw[:n]).decode(), "sha256": B.sha(data)}
    res = [verdict(blk, u_len) for _, blk, u_len in B.handmade_cases()]
    out["handmade"] = {"accept": "".join("1" if r[0] else "0" for r in res),
                       "digest": B.group_digest([r[0] for r in res], [r[1] for r in res])}
    mal = B.malformed_cases()
    res = [verdict(blk, u_len) for _, blk, u_len in mal]
    out["malformed"] = {"accept": "".join("1" if r[0] else "0" for r in res),
                        "offset0": [c[0] for c, r in zip(mal, res) if r[2]],
                        "sha256": {c[0]: B.sha(r[1]) for c, r in zip(mal, res) if r[0]}}
    u_len = B.fuzz_block()[1]
    res = [verdict(m, u_len) for m in B.fuzz_mutations()]
    out["fuzz"] = {
        "accept": "".join("1" if r[0] else "0" for r in res),
        "offset0": [i for i, r in enumerate(res) if r[2]],
        "groups": [B.group_digest([r[0] for r in res[i:i + B.FUZZ_GROUP]], [r[1] for r in res[i:i + B.FUZZ_GROUP]])
                   for i in range(0, len(res), B.FUZZ_GROUP)],
    }
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lz4_blocks.json"), "w") as f:
        json.dump(out, f, indent=1)
    acc = out["fuzz"]["accept"].count("1")
    print("liblz4", out["_liblz4"], "| handmade accepted:", out["handmade"]["accept"].count("1"), "of",
          len(out["handmade"]["accept"]), "| malformed accepted:", out["malformed"]["accept"].count("1"), "of", len(mal),
          "| fuzz accepted:", acc, "of", len(out["fuzz"]["accept"]), "| offset 0:", len(out["fuzz"]["offset0"]))


if __name__ == "__main__":
    main()
