"""Generates tests/golden/rs_repair.json: what the reference's own rsd32 / gather (rs-mrzip/reed-solomon.c, built into
oracle/_ref/librs_ref.so by `make -C oracle ref`) and decode()'s loop around them return on the damaged encodings of
tests/test_rs_repair_emu.py and tests/test_rs_repair_gpu.py -- output, report and the status of every codeword.  The
tests compare with these records, so they run on a checkout without the reference tree.
Run:  python tests/golden/make_rs_repair_golden.py

cases() is the one list of cases; the tests import it.  Encodings come from the oracle's rs_encode; where the damage
goes and what it is comes from _util.xorshift_noise, so the cases do not depend on the interpreter."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _util  # noqa: E402

ROWS, K, N = 8176, 223, 255
BURST = ROWS * N       # 2084880 encoded bytes
BURST_IN = ROWS * K    # 1823248 data bytes
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "rs_repair.json")

# case A: which rows are damaged.  Row r carries r % 19 errors: none, 1..16 (repairable), 17 and 18 (not).
A_ROWS = list(range(0, 256)) + list(range(8064, 8176)) + [300 + 157 * k for k in range(50)]
A_FIXED = {  # row -> [(column, xor value)]
    5000: [(223, 0x01), (230, 0x80), (254, 0xff)],  # parity columns only
    5001: [(0, 0x5a), (222, 0xa5), (254, 0x3c)],    # first data column, last data column, last parity column
    5002: [(100, 0x10)],                            # one bit
}


def row_errors(seed, count):
    """`count` errors of one codeword: distinct columns in 0..254 and non-zero values, from xorshift_noise(seed)."""
    raw = _util.xorshift_noise(192, seed=seed)
    cols = []
    for b in raw[:128]:
        c = b % 255
        if c not in cols:
            cols.append(c)
            if len(cols) == count:
                break
    assert len(cols) == count
    return [(c, raw[128 + i] % 255 + 1) for i, c in enumerate(cols)]


def put(enc, burst, row, errors):
    """byte c of row r of burst b sits at b * 2084880 + c * 8176 + r"""
    for c, v in errors:
        enc[burst * BURST + c * ROWS + row] ^= v


def case_a_damage():
    """row -> errors of case A (the tests use it to say what the reference must have done with each row)"""
    dmg = {r: row_errors(1000 + r, r % 19) for r in A_ROWS if r % 19}
    dmg.update(A_FIXED)
    return dmg


def cases(oracle, names=("A", "B", "C")):
    """name -> dict(data, enc): the data and its damaged encoding.
    A  one burst, every lane of two whole 128-row tiles and of the short last tile, every error count 0..18
    B  three bursts: a contiguous run of 16 x 8176 bytes, 16 errors in every row, 17 errors in 4096 rows
    C  A without its trailer"""
    out = {}
    if "A" in names or "C" in names:
        data = _util.xorshift_noise(BURST_IN - 1000, seed=31)
        enc = np.frombuffer(oracle.rs_encode(data), dtype=np.uint8).copy()
        assert len(enc) == BURST + 68
        for r, errors in case_a_damage().items():
            put(enc, 0, r, errors)
        enc = enc.tobytes()
        if "A" in names:
            out["A"] = dict(data=data, enc=enc)
        if "C" in names:
            out["C"] = dict(data=data, enc=enc[:-68])
    if "B" in names:
        data = _util.xorshift_noise(2 * BURST_IN + 777, seed=32)
        enc = np.frombuffer(oracle.rs_encode(data), dtype=np.uint8).copy()
        assert len(enc) == 3 * BURST + 68
        enc[5000:5000 + 16 * ROWS] ^= 0xa5
        for r in range(ROWS):
            put(enc, 1, r, row_errors(20000 + r, 16))
        for r in range(4096):
            put(enc, 2, r, row_errors(40000 + r, 17))
        out["B"] = dict(data=data, enc=enc.tobytes())
    return out


def status_record(status):
    """(sha256 of the little-endian int32 array, histogram value -> rows)"""
    status = np.asarray(status, dtype="<i4")
    vals, counts = np.unique(status, return_counts=True)
    return hashlib.sha256(status.tobytes()).hexdigest(), {str(int(v)): int(c) for v, c in zip(vals, counts)}


def decode_ref(R, enc):
    """`rs-mrzip -d` on `enc` by the reference's rsd32 / gather with decode()'s loop (rs-mrzip/rs-mrzip.c:37-117) around
    them: (bytes, report, int32 status of every codeword, the rows as decoded before the padding is stripped)."""
    nb = len(enc) // BURST
    tail = enc[nb * BURST:]
    rows_out = []
    status = np.zeros(nb * ROWS, dtype="<i4")
    for b in range(nb):
        tr = ctypes.create_string_buffer(enc[b * BURST:(b + 1) * BURST], BURST)
        ec = ctypes.create_string_buffer(BURST)
        R.gather(tr, ec, ROWS, N)
        eras = (ctypes.c_int * 32)()
        base = ctypes.addressof(ec)
        for i in range(ROWS):
            status[b * ROWS + i] = R.rsd32(ctypes.c_void_p(base + i * N), eras, 0)
        rows_out.append(np.frombuffer(ec.raw, dtype=np.uint8).reshape(ROWS, N)[:, :K].tobytes())
    full = b"".join(rows_out)
    rep = dict(corrected=int(status[status > 0].sum()), uncorrectable=int((status == -1).sum()), checksum_ok=False,
               truncated=len(tail) != 68)
    out = full
    if len(tail) == 68:
        rep["checksum_ok"] = hashlib.blake2b(full).digest() == tail[:64]
        k_i, k_j = tail[64] | tail[65] << 8, tail[66] | tail[67] << 8
        if k_i < ROWS:
            out = full[:(nb - 1) * BURST_IN + k_i * K + k_j]
    return out, rep, status, full


def check_case_a(enc, status, full):
    """What the case list promises about case A, checked against the reference's results."""
    clean = np.frombuffer(enc, dtype=np.uint8)[:BURST].reshape(N, ROWS)  # [column][row], damaged
    dmg = case_a_damage()
    for r in range(ROWS):
        errors = dmg.get(r, [])
        got_row = full[r * K:(r + 1) * K]
        as_it_came = clean[:K, r].tobytes()
        if len(errors) <= 16:
            assert status[r] == len(errors), (r, status[r], len(errors))  # repaired, every damaged byte counted
            want = bytearray(as_it_came)
            for c, v in errors:
                if c < K:
                    want[c] ^= v
            assert got_row == bytes(want), r  # parity-only damage changes no output byte
        else:
            assert status[r] == -1 and got_row == as_it_came, r  # left alone
    assert set(np.unique(status).tolist()) == set(range(-1, 17))


def main():
    R = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "librs_ref.so"))
    oracle = _util.Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))
    rec = {"_source": "results of the reference's rs-mrzip/reed-solomon.c (oracle/_ref/librs_ref.so: rsd32, gather) on the "
                      "damaged encodings of tests/golden/make_rs_repair_golden.py, keyed by their sha256"}
    for name, c in cases(oracle).items():
        out, rep, status, full = decode_ref(R, c["enc"])
        if name == "A":
            check_case_a(c["enc"], status, full)
        if name == "B":
            assert rep["uncorrectable"] == 4096 and rep["checksum_ok"] is False
            assert (status[:2 * ROWS] == 16).all() and (status[2 * ROWS:2 * ROWS + 4096] == -1).all()
        if name == "C":
            assert rep["truncated"] and len(out) == BURST_IN
        sha, hist = status_record(status)
        rec[hashlib.sha256(c["enc"]).hexdigest()] = {"case": name, "len": len(out), "sha256": hashlib.sha256(out).hexdigest(),
                                                     "report": rep, "status_sha256": sha, "status_hist": hist}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def recorded(enc):
    """the reference's record for `enc`"""
    with open(GOLDEN) as f:
        rec = json.load(f).get(hashlib.sha256(enc).hexdigest())
    assert rec is not None, "no recorded reference decode of this encoding (run tests/golden/make_rs_repair_golden.py)"
    return rec


if __name__ == "__main__":
    main()
