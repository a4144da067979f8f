"""Shared checks of mrz_rs_decode_lost (tests/test_rs_erasure_emu.py on the wave64 emulator, tests/test_rs_erasure_gpu.py
on the GPU) against the reference's recorded results (tests/golden/rs_erasure.json: rsd32 with eras_pos / no_eras)."""
import ctypes
import hashlib

import numpy as np

from modern_rzip_amd import binding
from tests.golden import make_rs_erasure_golden as G
from tests.golden import make_rs_repair_golden as G0

MRZ_E_ARG = -1


def compare(want, got, rep, status, rows):
    """(bytes, report, status) == a record of the reference: length and sha256, report, status sha256 and histogram"""
    assert status.dtype == np.int32 and len(status) == rows
    sha, hist = G0.status_record(status)
    assert hist == want["status_hist"], (hist, want["status_hist"])
    assert sha == want["status_sha256"]
    assert rep == want["report"], (rep, want["report"])
    assert len(got) == want["len"] and hashlib.sha256(got).hexdigest() == want["sha256"]


def decode_and_compare(ctx, c):
    """rs_decode_lost(enc, lost) == the reference told the same columns"""
    got, rep, status = ctx.rs_decode_lost(c["enc"], c["lost"])
    compare(G.recorded(c["enc"], c["lost"]), got, rep, status, ctx.lib.mrz_rs_codewords(len(c["enc"])))
    return got, rep, status


def check_l1(got, rep, status):
    """every count of erasures and errors, the rows beyond the limit as the reference left them"""
    assert set(np.unique(status).tolist()) == set(range(-1, 33))
    assert status[G.L1_INTACT] == 6    # 5 erased columns that held the right bytes are counted with the 1 error
    assert status[G.L1_PARITY] == 32   # the 32 parity columns: nothing of the output changes
    assert all(status[r] == -1 for r in G.L1_OVER)  # 33 and 34 erased columns
    for base in (0, G.L1_LAST):
        for i, (e, t) in enumerate(G.L1_COMBOS):
            if e + 2 * t <= 32:
                assert status[base + i] in (0, e + t), (base, e, t)  # (0: zero fill of a padded row of zeros)
    assert rep["checksum_ok"] is False and rep["uncorrectable"] == int((status == -1).sum())
    assert rep["corrected"] == int(status[status > 0].sum())


def check_rows_restored(data, got, status):
    """every codeword that was clean or repaired holds the data's bytes again (cases without miscorrections)"""
    padded = np.frombuffer(data + bytes(len(status) * G0.K - len(data)), dtype=np.uint8).reshape(-1, G0.K)
    rows = np.frombuffer(got + bytes(len(status) * G0.K - len(got)), dtype=np.uint8).reshape(-1, G0.K)
    good = status >= 0
    assert good.sum() > 0 and (rows[good] == padded[good]).all()


def l2_burst0(c, oracle=None, rows=None):
    """burst 0 of case L2 on its own (no trailer) with its one lost run of 32 x 8176 bytes: (enc, lost, data, the rows
    that are damaged).  With `rows`, the run is zero-filled in those rows only and the other rows hold their bytes, lost
    as they are declared: fewer codewords to repair where a codeword is slow (the emulator)."""
    enc, data = c["enc"][:G0.BURST], c["data"][:G0.BURST_IN]
    damaged = np.ones(G0.ROWS, dtype=bool)
    if rows is not None:
        damaged[:] = False
        damaged[list(rows)] = True
        thin = np.frombuffer(oracle.rs_encode(c["data"])[:G0.BURST], dtype=np.uint8).reshape(G0.N, G0.ROWS).copy()
        thin[:, damaged] = np.frombuffer(enc, dtype=np.uint8).reshape(G0.N, G0.ROWS)[:, damaged]
        enc = thin.tobytes()
    return enc, [G.L2_RUN0], data, damaged


def check_hints_double_the_reach(ctx, enc, lost, data, damaged):
    """a lost run of 32 x 8176 bytes: restored when it is declared, -1 in every damaged row without"""
    got, rep, status = ctx.rs_decode_lost(enc, lost)
    assert (status[damaged] == 32).all() and not status[~damaged].any()  # (intact rows: their syndromes vanish)
    assert rep["corrected"] == 32 * int(damaged.sum()) and rep["uncorrectable"] == 0 and rep["truncated"]
    assert got == data
    got0, rep0, status0 = ctx.rs_decode_ex(enc)
    assert (status0[status == 32] == -1).all() and not status0[status == 0].any()
    assert rep0["uncorrectable"] == int(damaged.sum()) and got0 != data


def check_no_ranges_is_decode_ex(ctx, oracle):
    """n_lost = 0: bytes, report and status of rs_decode_ex, on case A of rs_repair.json"""
    enc = G0.cases(oracle, names=("A",))["A"]["enc"]
    got, rep, status = ctx.rs_decode_lost(enc, [])
    got0, rep0, status0 = ctx.rs_decode_ex(enc)
    assert got == got0 and rep == rep0 and (status == status0).all()
    compare(G0.recorded(enc), got, rep, status, G0.ROWS)


def raw_call(ctx, enc, ranges, n_lost=None):
    """mrz_rs_decode_lost's return code for `ranges` (host input and output)"""
    cap = (len(enc) // G0.BURST) * G0.BURST_IN
    buf = ctypes.create_string_buffer(cap)
    out_len = ctypes.c_int64()
    rep = binding.RsReport()
    arr = (binding.RsRange * max(len(ranges), 1))(*[binding.RsRange(o, n) for o, n in ranges]) if ranges is not None else None
    return ctx.lib.mrz_rs_decode_lost(ctx.ctx, enc, len(enc), binding.MEM_HOST, buf, binding.MEM_HOST, cap,
                                      ctypes.byref(out_len), arr, len(ranges) if n_lost is None else n_lost, None, 0, 1,
                                      ctypes.byref(rep))


def check_arguments(ctx, enc):
    """ranges must be non-empty, inside the input, ascending and disjoint; adjacent ones are fine"""
    n = len(enc)
    assert raw_call(ctx, enc, [(100, 10), (50, 10)]) == MRZ_E_ARG      # unsorted
    assert raw_call(ctx, enc, [(100, 10), (109, 10)]) == MRZ_E_ARG     # overlapping
    assert raw_call(ctx, enc, [(100, 10), (100, 10)]) == MRZ_E_ARG     # twice
    assert raw_call(ctx, enc, [(100, 0)]) == MRZ_E_ARG                 # empty
    assert raw_call(ctx, enc, [(100, -5)]) == MRZ_E_ARG                # negative length
    assert raw_call(ctx, enc, [(-1, 10)]) == MRZ_E_ARG                 # negative offset
    assert raw_call(ctx, enc, [(n - 5, 6)]) == MRZ_E_ARG               # past the end
    assert raw_call(ctx, enc, [(n, 1)]) == MRZ_E_ARG
    assert raw_call(ctx, enc, [(0, 2 ** 63 - 1)]) == MRZ_E_ARG         # offset + len overflows
    assert raw_call(ctx, enc, None, n_lost=1) == MRZ_E_ARG             # NULL with a count
    assert raw_call(ctx, enc, [(0, 1)], n_lost=-1) == MRZ_E_ARG
    assert raw_call(ctx, enc, [(100, 10), (110, 10), (n - 1, 1)]) == 0  # adjacent, and up to the last byte
    assert raw_call(ctx, enc, None, n_lost=0) == 0                     # NULL and no ranges
