"""Shared checks of mrz_rs_decode_ex (tests/test_rs_repair_emu.py on the wave64 emulator, tests/test_rs_repair_gpu.py
on the GPU) against the reference's recorded results (tests/golden/rs_repair.json)."""
import ctypes
import hashlib

import numpy as np

from modern_rzip_amd import binding
from tests import _util
from tests.golden import make_rs_repair_golden as G

MRZ_E_ARG = -1


def decode_and_compare(ctx, enc):
    """rs_decode_ex(enc) == the reference: output length and sha256, report, status sha256 and histogram."""
    want = G.recorded(enc)
    got, rep, status = ctx.rs_decode_ex(enc)
    assert status.dtype == np.int32 and len(status) == ctx.lib.mrz_rs_codewords(len(enc))
    sha, hist = G.status_record(status)
    assert hist == want["status_hist"], (hist, want["status_hist"])
    assert sha == want["status_sha256"]
    assert rep == want["report"], (rep, want["report"])
    assert len(got) == want["len"] and hashlib.sha256(got).hexdigest() == want["sha256"]
    return got, rep, status


def check_old_entry(ctx, enc, got, rep):
    """mrz_rs_decode: the same bytes and the same four report fields"""
    old, old_rep = ctx.rs_decode(enc)
    assert old == got
    assert old_rep == rep, (old_rep, rep)


def check_rows_round_trip(data, got, status):
    """every codeword that was clean or repaired holds the data's bytes again"""
    padded = np.frombuffer(data + bytes(len(status) * G.K - len(data)), dtype=np.uint8).reshape(-1, G.K)
    rows = np.frombuffer(got + bytes(len(status) * G.K - len(got)), dtype=np.uint8).reshape(-1, G.K)
    good = status >= 0
    assert good.sum() > 0 and (rows[good] == padded[good]).all()


def check_out_cap(ctx, enc):
    """out_cap one byte short: MRZ_E_ARG"""
    lib = ctx.lib
    cap = (len(enc) // G.BURST) * G.BURST_IN
    buf = ctypes.create_string_buffer(cap)
    out_len = ctypes.c_int64()
    rep = binding.RsReport()
    args = (ctx.ctx, enc, len(enc), binding.MEM_HOST, buf, binding.MEM_HOST)
    rc = lib.mrz_rs_decode_ex(*args, cap - 1, ctypes.byref(out_len), None, 0, 1, ctypes.byref(rep))
    assert rc == MRZ_E_ARG


def check_codewords(lib):
    assert lib.mrz_rs_codewords(2084880 * 3 + 68) == 3 * 8176
    assert lib.mrz_rs_codewords(100) == 0


def undamaged_three_bursts(oracle):
    data = _util.xorshift_noise(2 * G.BURST_IN + 777, seed=32)
    return data, oracle.rs_encode(data)


def check_undamaged(ctx, data, enc):
    got, rep, status = ctx.rs_decode_ex(enc)
    assert len(status) == 3 * G.ROWS and not status.any()
    assert rep == dict(corrected=0, uncorrectable=0, checksum_ok=True, truncated=False)
    assert got == data
