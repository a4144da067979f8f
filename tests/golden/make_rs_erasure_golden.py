"""Generates tests/golden/rs_erasure.json: what the reference's own rsd32 / gather (rs-mrzip/reed-solomon.c, built into
oracle/_ref/librs_ref.so by `make -C oracle ref`) return, row by row, when they are told which columns of a codeword
were lost (rsd32's eras_pos / no_eras, which the reference's own decode() never passes) -- output, report and the
status of every codeword of the damaged encodings of tests/test_rs_erasure_emu.py and tests/test_rs_erasure_gpu.py.
The tests compare mrz_rs_decode_lost with these records, so they run on a checkout without the reference tree.
Run:  python tests/golden/make_rs_erasure_golden.py

cases() is the one list of cases; the tests import it.  Encodings come from the oracle's rs_encode; where the damage
goes and what it is comes from _util.xorshift_noise, so the cases do not depend on the interpreter.

Two things are this project's definition and not the reference's (include/mrzgpu.h says so): a row with more than 32
erased columns and non-zero syndromes is -1 and stays as it came (rsd32 would write lambda[33]), and what a range covers
beyond the last whole burst is ignored."""
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
from tests.golden.make_rs_repair_golden import BURST, BURST_IN, K, N, ROWS, row_errors, status_record  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "rs_erasure.json")

# case L1: every mix of e erased columns and t errors up to one error beyond the code's reach (e + 2 t <= 32)
L1_COMBOS = [(e, t) for e in range(33) for t in range((32 - e) // 2 + 2)]
assert len(L1_COMBOS) == 322
L1_LAST = ROWS - len(L1_COMBOS)  # the combinations again on the last 322 rows: they reach the short last tile
L1_OVER = {4000: (33, 0), 4001: (33, 1), 4002: (34, 0), 4003: (34, 1)}  # more erasures than the code has parity
L1_INTACT = 4004   # 5 columns declared lost that hold the right bytes, and 1 error
L1_PARITY = 4005   # columns 223..254 erased
# case L2: contiguous runs
L2_RUN0 = (5000, 32 * ROWS)                         # burst 0: 32 columns in every row
L2_RUN1 = (BURST + 10 * ROWS, 29 * ROWS + 4000)     # burst 1: with the seam's 3 columns 33 in rows 0..3999, 32 in the rest
L2_SEAM = (2 * BURST - 3 * ROWS, 5 * ROWS)          # the last 3 parity columns of burst 1, the first 2 columns of burst 2
L2_RUN2 = (2 * BURST + 100 * ROWS, 22 * ROWS)       # burst 2: with the seam's 2 columns 24 in every row, and 4 errors
L2_TRAILER = (3 * BURST, 68)                        # declared lost, untouched, ignored


def l1_damage():
    """row -> (erased columns: zero-filled and declared lost, [(column, xor value)], columns declared lost but intact)"""
    dmg = {}
    for base, seed in ((0, 50000), (L1_LAST, 60000)):
        for i, (e, t) in enumerate(L1_COMBOS):
            errs = row_errors(seed + i, e + t) if e + t else []
            dmg[base + i] = ([c for c, _ in errs[:e]], errs[e:], [])
    for r, (e, t) in L1_OVER.items():
        errs = row_errors(70000 + r, e + t)
        dmg[r] = ([c for c, _ in errs[:e]], errs[e:], [])
    errs = row_errors(70000 + L1_INTACT, 6)
    dmg[L1_INTACT] = ([], errs[5:], [c for c, _ in errs[:5]])
    dmg[L1_PARITY] = (list(range(K, N)), [], [])
    return dmg


def l2_errors(r):
    """the 4 errors of row r of burst 2, outside the 24 erased columns (0, 1 and 100..121)"""
    errs = [(c, v) for c, v in row_errors(80000 + r, 32) if c > 1 and not 100 <= c < 122]
    return errs[:4]


def cases(oracle, names=("L1", "L2", "L3")):
    """name -> dict(data, enc, lost): the data, its damaged encoding and the sorted (offset, len) ranges declared lost.
    L1  one burst: every mix of e erasures and t errors with t up to one beyond the limit, on the first and the last 322
        rows; 33 and 34 erasures; erased but intact columns; all parity columns erased.  One-byte ranges.
    L2  three bursts: zero-filled runs of 32 columns, of 32 and 33 columns, of 24 columns with 4 errors in every row;
        one range across the seam of two bursts, one over the trailer
    L3  L1 without its trailer"""
    out = {}
    if "L1" in names or "L3" in names:
        data = _util.xorshift_noise(BURST_IN - 1000, seed=31)
        enc = np.frombuffer(oracle.rs_encode(data), dtype=np.uint8).copy()
        assert len(enc) == BURST + 68
        lost = []
        for r, (erased, errors, intact) in l1_damage().items():
            for c in erased:
                enc[c * ROWS + r] = 0
            for c, v in errors:
                enc[c * ROWS + r] ^= v
            lost += [(c * ROWS + r, 1) for c in erased + intact]
        lost.sort()
        enc = enc.tobytes()
        if "L1" in names:
            out["L1"] = dict(data=data, enc=enc, lost=lost)
        if "L3" in names:
            out["L3"] = dict(data=data, enc=enc[:-68], lost=lost)
    if "L2" in names:
        data = _util.xorshift_noise(2 * BURST_IN + 777, seed=32)
        enc = np.frombuffer(oracle.rs_encode(data), dtype=np.uint8).copy()
        assert len(enc) == 3 * BURST + 68
        lost = [L2_RUN0, L2_RUN1, L2_SEAM, L2_RUN2, L2_TRAILER]
        assert lost == sorted(lost) and all(a + n <= b for (a, n), (b, _) in zip(lost, lost[1:]))
        for off, n in lost[:-1]:
            enc[off:off + n] = 0
        for r in range(ROWS):
            for c, v in l2_errors(r):
                enc[2 * BURST + c * ROWS + r] ^= v
        out["L2"] = dict(data=data, enc=enc.tobytes(), lost=lost)
    return out


def lost_bytes(lost):
    """the ranges as little-endian int64 pairs (mrz_rs_range[])"""
    return np.asarray(lost, dtype="<i8").reshape(-1, 2).tobytes()


def key(enc, lost):
    return hashlib.sha256(enc + lost_bytes(lost)).hexdigest()


def erased_columns(lost, nb):
    """bool [burst][column][row]: the byte lies in a lost range (what lies beyond the last whole burst is dropped)"""
    mask = np.zeros(nb * BURST, dtype=bool)
    for off, n in lost:
        mask[off:off + n] = True
    return mask.reshape(nb, N, ROWS)


def decode_ref(R, enc, lost):
    """`rs-mrzip -d` on `enc` by the reference's gather and, row by row, rsd32(row, eras_pos = the row's erased columns,
    no_eras) with decode()'s loop (rs-mrzip/rs-mrzip.c:37-117) around them: (bytes, report, int32 status of every
    codeword, the rows as decoded before the padding is stripped).  A row with more than 32 erased columns is not
    given to rsd32: 0 if it is a codeword (its syndromes vanish: rse32 of its data gives its parity), else -1, and it
    stays as it came."""
    nb = len(enc) // BURST
    tail = enc[nb * BURST:]
    mask = erased_columns(lost, nb)
    rows_out = []
    status = np.zeros(nb * ROWS, dtype="<i4")
    for b in range(nb):
        tr = ctypes.create_string_buffer(enc[b * BURST:(b + 1) * BURST], BURST)
        ec = ctypes.create_string_buffer(BURST)
        R.gather(tr, ec, ROWS, N)
        eras = (ctypes.c_int * 32)()
        base = ctypes.addressof(ec)
        per_row = mask[b].sum(axis=0)
        for i in range(ROWS):
            if per_row[i] > 32:
                again = ctypes.create_string_buffer(ec.raw[i * N:(i + 1) * N], N)
                R.rse32(again, ctypes.byref(again, K))
                status[b * ROWS + i] = 0 if again.raw == ec.raw[i * N:(i + 1) * N] else -1
                continue
            cols = np.nonzero(mask[b][:, i])[0] if per_row[i] else []
            for j, c in enumerate(cols):  # refilled for every row: rsd32 writes the locations it found over it
                eras[j] = int(c)
            status[b * ROWS + i] = R.rsd32(ctypes.c_void_p(base + i * N), eras, len(cols))
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


def rows_of(data, nb):
    """the zero-padded data as [row][223]"""
    return np.frombuffer(data + bytes(nb * BURST_IN - len(data)), dtype=np.uint8).reshape(-1, K)


def check_l1(c, clean_enc, status, full):
    """What the case list promises about L1, checked against the reference's results.  Returns how the rows one error
    beyond the limit ended: (uncorrectable, miscorrected)."""
    want = rows_of(c["data"], 1)
    got = np.frombuffer(full, dtype=np.uint8).reshape(-1, K)
    came = np.frombuffer(c["enc"], dtype=np.uint8)[:BURST].reshape(N, ROWS)
    clean = np.frombuffer(clean_enc, dtype=np.uint8)[:BURST].reshape(N, ROWS)
    dmg = l1_damage()
    beyond = [0, 0]
    for r in range(ROWS):
        erased, errors, intact = dmg.get(r, ([], [], []))
        e, t = len(erased) + len(intact), len(errors)
        touched = (came[:, r] != clean[:, r]).any()  # (a zero-filled column may have held a zero: the padded last rows)
        if not touched:
            assert status[r] == 0 and (got[r] == want[r]).all(), r  # syndromes vanish: rsd32 does not look at eras_pos
        elif e > 32:
            assert status[r] == -1 and (got[r] == came[:K, r]).all(), r  # by definition: left alone
        elif e + 2 * t <= 32:
            # restored; every erased column is counted, also where the byte was right
            assert status[r] == e + t and (got[r] == want[r]).all(), (r, e, t, status[r])
        else:  # one error too many: rsd32 gives up, or finds another codeword within its reach
            assert e + 2 * t in (33, 34)
            if status[r] == -1:
                assert (got[r] == came[:K, r]).all(), r
                beyond[0] += 1
            else:
                assert status[r] > 0 and (got[r] != want[r]).any(), (r, e, t, status[r])
                beyond[1] += 1
    assert status[L1_INTACT] == 6 and status[L1_PARITY] == 32
    assert all(status[r] == -1 for r in L1_OVER)
    assert beyond[0] > 0 and beyond[1] > 0, beyond  # both ends are in the records
    return tuple(beyond)


def check_l2(c, status, full, rep):
    want = rows_of(c["data"], 3)
    got = np.frombuffer(full, dtype=np.uint8).reshape(-1, K)
    per_row = erased_columns(c["lost"], 3).sum(axis=1).reshape(-1)  # erased columns of every codeword
    assert (per_row[:ROWS] == 32).all() and (status[:ROWS] == 32).all()
    assert (per_row[ROWS:ROWS + 4000] == 33).all() and (status[ROWS:ROWS + 4000] == -1).all()
    assert (per_row[ROWS + 4000:2 * ROWS] == 32).all() and (status[ROWS + 4000:2 * ROWS] == 32).all()
    assert (per_row[2 * ROWS:] == 24).all() and (status[2 * ROWS:] == 28).all()  # 24 erasures + 4 errors: 24 + 8 = 32
    good = status >= 0
    assert (got[good] == want[good]).all()
    assert rep["uncorrectable"] == 4000 and rep["checksum_ok"] is False and not rep["truncated"]


def main():
    R = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "librs_ref.so"))
    oracle = _util.Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))
    rec = {"_source": "results of the reference's rs-mrzip/reed-solomon.c (oracle/_ref/librs_ref.so: gather, and rsd32 with "
                      "each row's erased columns as eras_pos) on the damaged encodings and lost ranges of "
                      "tests/golden/make_rs_erasure_golden.py, keyed by the sha256 of the encoding followed by the ranges "
                      "as little-endian int64 pairs"}
    for name, c in cases(oracle).items():
        out, rep, status, full = decode_ref(R, c["enc"], c["lost"])
        extra = {}
        if name in ("L1", "L3"):
            clean_enc = oracle.rs_encode(c["data"])
            extra["beyond_limit"] = dict(zip(("uncorrectable", "miscorrected"), check_l1(c, clean_enc, status, full)))
            assert rep["truncated"] == (name == "L3")
            if name == "L3":
                assert len(out) == BURST_IN
        if name == "L2":
            check_l2(c, status, full, rep)
        sha, hist = status_record(status)
        rec[key(c["enc"], c["lost"])] = {"case": name, "len": len(out), "sha256": hashlib.sha256(out).hexdigest(),
                                         "report": rep, "status_sha256": sha, "status_hist": hist, **extra}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def recorded(enc, lost):
    """the reference's record for `enc` with `lost`"""
    with open(GOLDEN) as f:
        rec = json.load(f).get(key(enc, lost))
    assert rec is not None, "no recorded reference decode of this input (run tests/golden/make_rs_erasure_golden.py)"
    return rec


if __name__ == "__main__":
    main()
