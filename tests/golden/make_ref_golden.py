"""Generates tests/golden/ref_outputs.json: what the reference's own blake2b.c and
rs-mrzip/reed-solomon.c (oracle/_ref, built by `make -C oracle ref` where the
reference tree is present) return on the seeded inputs of the tests that pin
against them.  The tests compare with these recorded outputs, so they run on a
checkout without the reference tree.  Run:  python tests/golden/make_ref_golden.py"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _util  # noqa: E402

ROWS, K, N = 8176, 223, 255
BURST = ROWS * N


def blake2b_cases():
    """(n, data): the inputs of test_oracle_golden.test_blake2b_against_reference_build."""
    for n in (0, 5, 128, 129, 223, 223 * 7, 10000):
        yield n, _util.xorshift_noise(n, seed=3 * n + 1)


def rs_decode_cases():
    """(data, damage): the encodings that test_rs_decoder_against_the_reference (emulated and GPU tier) decodes."""
    d = _util.xorshift_noise(300000, seed=5)
    dmg = [(1000, 4 * 8176, 0x5a)] + [((20 + 3 * k) * 8176 + 7, 1, 0x11) for k in range(16)]
    dmg += [((100 + 2 * k) * 8176 + 9, 1, 0x80) for k in range(17)]
    yield d, []
    yield d, dmg
    yield d, dmg[1:17]
    yield d, [(2084880 + 3, 1, 1)]
    d = _util.xorshift_noise(2 * 1823248 + 777, seed=15)
    dmg = [(5000, 16 * 8176, 0xa5), (2084880 + 999, 3 * 8176 + 100, 0x3c)]
    yield d, []
    yield d, dmg
    yield d, dmg + [(2 * 2084880, 17 * 8176, 0x77)]


def damaged(enc, damage):
    enc = bytearray(enc)
    for at, n, val in damage:
        for k in range(n):
            enc[at + k] ^= val
    return bytes(enc)


def blake2b_ref(R, pieces, outlen=64):
    class St(ctypes.Structure):
        _fields_ = [("h", ctypes.c_uint64 * 8), ("t", ctypes.c_uint64 * 2), ("f", ctypes.c_uint64 * 2),
                    ("buf", ctypes.c_uint8 * 128), ("buflen", ctypes.c_size_t), ("outlen", ctypes.c_size_t),
                    ("last_node", ctypes.c_uint8)]
    s = St()
    R.blake2b_init(ctypes.byref(s), ctypes.c_size_t(outlen))
    for p in pieces:
        R.blake2b_update(ctypes.byref(s), p, ctypes.c_size_t(len(p)))
    out = ctypes.create_string_buffer(64)
    R.blake2b_final(ctypes.byref(s), out, ctypes.c_size_t(outlen))
    return out.raw[:outlen]


def rs_decode_ref(R, enc):
    """`rs-mrzip -d` on `enc` with the reference's own rsd32 / gather and decode()'s loop (rs-mrzip/rs-mrzip.c:37-117)
    around them: (bytes, report)."""
    nb = len(enc) // BURST
    tail = enc[nb * BURST:]
    rows_out = bytearray()
    corrected = uncorrectable = 0
    for b in range(nb):
        tr = ctypes.create_string_buffer(enc[b * BURST:(b + 1) * BURST], BURST)
        ec = ctypes.create_string_buffer(BURST)
        R.gather(tr, ec, ROWS, N)
        eras = (ctypes.c_int * 32)()
        base = ctypes.addressof(ec)
        for i in range(ROWS):
            f = R.rsd32(ctypes.c_void_p(base + i * N), eras, 0)
            if f > 0:
                corrected += f
            elif f == -1:
                uncorrectable += 1
        raw = ec.raw
        for i in range(ROWS):
            rows_out += raw[i * N:i * N + K]
    rep = dict(corrected=corrected, uncorrectable=uncorrectable, checksum_ok=False, truncated=len(tail) != 68)
    out = bytes(rows_out)
    if len(tail) == 68:
        rep["checksum_ok"] = hashlib.blake2b(out).digest() == tail[:64]
        k_i, k_j = tail[64] | tail[65] << 8, tail[66] | tail[67] << 8
        if k_i < ROWS:
            out = out[:(nb - 1) * ROWS * K + k_i * K + k_j]
    return out, rep


def main():
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    B = ctypes.CDLL(os.path.join(ref_dir, "libblake2b_ref.so"))
    R = ctypes.CDLL(os.path.join(ref_dir, "librs_ref.so"))
    oracle = _util.Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))
    out = {"_source": "outputs of the reference's common/blake2b.c and rs-mrzip/reed-solomon.c (oracle/_ref) on the "
                      "seeded inputs of tests/golden/make_ref_golden.py",
           "blake2b": {}, "rse32_parity": [], "rs_decode": {}}
    for n, d in blake2b_cases():
        rows = [d[i:i + K] for i in range(0, len(d), K)]
        out["blake2b"][str(n)] = {"whole_64": blake2b_ref(B, [d]).hex(), "rows_64": blake2b_ref(B, rows).hex(),
                                  "whole_32": blake2b_ref(B, [d], 32).hex()}
    for trial in range(64):
        row = bytes(K) if trial == 0 else _util.xorshift_noise(K, seed=trial)
        buf = (ctypes.c_uint8 * N)(*row, *([0] * 32))
        R.rse32(buf, ctypes.byref(buf, K))
        out["rse32_parity"].append(bytes(buf)[K:].hex())
    # one whole burst through rse32 + scatter (the input of test_rs_encoder_against_reference_build)
    data = _util.xorshift_noise(ROWS * K - 1000, seed=9)
    padded = data + bytes(1000)
    ec = (ctypes.c_uint8 * BURST)()
    for r in range(ROWS):
        ctypes.memmove(ctypes.byref(ec, r * N), padded[r * K:(r + 1) * K], K)
        R.rse32(ctypes.byref(ec, r * N), ctypes.byref(ec, r * N + K))
    tr = (ctypes.c_uint8 * BURST)()
    R.scatter(ec, tr, ROWS, N)
    out["scatter_sha256"] = hashlib.sha256(bytes(tr)).hexdigest()
    # decodes, keyed by the sha256 of the (damaged) encoding handed to the decoder
    for d, damage in rs_decode_cases():
        enc = damaged(oracle.rs_encode(d), damage)
        got, rep = rs_decode_ref(R, enc)
        out["rs_decode"][hashlib.sha256(enc).hexdigest()] = {"len": len(got), "sha256": hashlib.sha256(got).hexdigest(),
                                                             "report": rep}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_outputs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
