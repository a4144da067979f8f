"""The checks of mrz_runzip_buffer_ranges (many ranges of an archive in one call), shared by the emulator tier
(test_archive_ranges_emu.py) and the GPU tier (test_archive_ranges_gpu.py).  Archives and framings are those of
tests/_lz4_range_checks.py: the four-chunk archive cut into blocks of 4096 or 8192 bytes, all CTYPE_NONE (-n), every block
LZ4 (-l), only stream 1's, alternating; the header with and without the size.  The bytes must be the concatenation of
mrz_runzip_buffer_range_ex over the ranges; the accounting is derived from the origins of the single calls."""
import ctypes

import numpy as np
import torch

import modern_rzip_amd as m
from modern_rzip_amd import binding
from tests import _lz4_blocks as B
from tests import _lz4_checks as C
from tests import _lz4_range_checks as R

E_ARG = -1
FRAMINGS = ("none",) + R.FRAMINGS
# (archive, framing, the header carries the size)
VARIANTS = [("four8192", f, True) for f in FRAMINGS] + [("four4096", "all", False), ("four8192", "none", False)]
SYMBOLS = ("mrz_runzip_buffer_ranges",)
KEYS = ("chunks_in_range", "total_hops", "max_hops", "s0_lz4_bytes", "s1_blocks_touched", "s1_lz4_bytes",
        "s1_bytes_uploaded")


def check_abi(lib):
    assert lib.mrz_abi_version() == 4
    assert all(hasattr(lib, s) for s in SYMBOLS)


def archive_of(name, framing, oracle, with_size):
    arc = R.source(name, oracle)[0] if framing == "none" else R.framed(name, framing, oracle)
    if not with_size:
        arc = arc[:6] + bytes(8) + arc[14:]
    return arc


def range_lists(n, seams):
    a, b, c = seams
    return {
        "in_one_chunk": [(10, 300), (a - 2000, 100), (200, 50), (a - 1, 1)],
        "straddling": [(a - 100, 200), (b - 1, 2), (c - 500, 900)],
        # both cross the first seam: chunk 0 holds [A0 B0], the output wants [A0 A1 B0 B1]
        "interleaved": [(a - 300, 600), (a - 200, 500)],
        "last_chunk_only": [(c + 10, 100), (n - 50, 50), (c + 10, 100)],
        "middle_untouched": [(n - 900, 900), (0, 0), (5, 700), (c + 1, 64), (a - 64, 64)],
        "descending_and_empty": [(n, 0), (c, 10), (b, 10), (a, 10), (0, 10), (0, 0)],
        "identical_and_overlapping": [(b - 400, 800), (b - 400, 800), (b - 100, 300)],
        "nothing": [(7, 0), (n, 0)],
    }


def touched_chunks(ranges, edges):
    """chunks that hold a byte of a range, counted in Python"""
    return [k for k, (lo, hi) in enumerate(zip(edges, edges[1:]))
            if any(cnt > 0 and max(first, lo) < min(first + cnt, hi) for first, cnt in ranges)]


def expect_info(plan, ranges):
    """R.Plan.expect for a list: hops summed / maxed over the parts, blocks and bytes per chunk from the union of the
    parts' origins"""
    exp = dict.fromkeys(KEYS, 0)
    total_count = sum(cnt for _, cnt in ranges)
    if plan.size_known and total_count == 0:
        return exp
    last_end = max([first + cnt for first, cnt in ranges if cnt > 0] + [0])
    total = 0
    for k, c in enumerate(plan.chunks):
        exp["s0_lz4_bytes"] += c["s0_lz4"]
        orgs = []
        for first, cnt in ranges:
            lo, hi = max(first, total), min(first + cnt, total + c["out_len"])
            if cnt > 0 and lo < hi:
                org, inf = plan.origins(k, lo - total, hi - lo)
                orgs.append(org)
                exp["total_hops"] += inf["total_hops"]
                exp["max_hops"] = max(exp["max_hops"], inf["max_hops"])
        if orgs:
            exp["chunks_in_range"] += 1
            org = np.concatenate(orgs)
            which = np.searchsorted(c["starts"], org, side="right") - 1
            for t in np.unique(which):
                blk, off = c["blocks"][t], org[which == t] - c["starts"][t]
                low, high = int(off.min()), int(off.max())
                exp["s1_blocks_touched"] += 1
                if blk["ctype"] == B.CTYPE_LZ4:
                    exp["s1_lz4_bytes"] += high + 1
                    exp["s1_bytes_uploaded"] += blk["c_len"]
                else:
                    exp["s1_bytes_uploaded"] += high - low + 1
        total += c["out_len"]
        if (plan.size_known and total >= last_end) or c["eof"]:
            break
    return exp


def to_device(lib, arc, ranges, emu):
    total = sum(cnt for _, cnt in ranges)
    t = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cpu" if emu else "cuda")
    _, file_len, info = m.runzip_buffer_ranges(arc, ranges, out=(t.data_ptr(), total + 64), lib=lib)
    raw = t.cpu().numpy().tobytes()
    return raw[:total], raw[total:] == b"\xa5" * 64, file_len, info


def check_archive(lib, ctx, oracle, emu, name, framing, with_size):
    cut, data, seams, bs = R.source(name, oracle)
    arc = archive_of(name, framing, oracle, with_size)
    assert (C.lz4_count(arc) > 0) == (framing != "none")
    plan = R.Plan(ctx, cut, arc, name)
    assert plan.size_known == with_size
    edges = [0] + list(seams) + [len(data)]
    for k, (label, ranges) in enumerate(range_lists(len(data), seams).items()):
        what = (name, framing, with_size, label)
        want = b"".join(m.runzip_buffer_range_ex(arc, first, cnt, lib=lib)[0] for first, cnt in ranges)
        assert want == b"".join(data[first:first + cnt] for first, cnt in ranges), what
        got, file_len, info = m.runzip_buffer_ranges(arc, ranges, lib=lib)
        assert file_len == len(data), what
        assert got == want, what
        touched = touched_chunks(ranges, edges)
        assert info["chunks_in_range"] == len(touched), (what, info, touched)
        assert info == expect_info(plan, ranges), (what, info, expect_info(plan, ranges))
        if label == "middle_untouched":
            assert touched == [0, 3]
            # what the two touched chunks cost when each is asked for alone is all the call has cost
            alone = [m.runzip_buffer_ranges(arc, [r for r in ranges if touched_chunks([r], edges) == [c]], lib=lib)[2]
                     for c in touched]
            for key in ("chunks_in_range", "total_hops", "s1_blocks_touched", "s1_lz4_bytes", "s1_bytes_uploaded"):
                assert info[key] == alone[0][key] + alone[1][key], (what, key)
        if label == "last_chunk_only":
            assert touched == [3]
        if label in ("interleaved", "middle_untouched"):   # the same into device memory
            dev, intact, file_len2, info2 = to_device(lib, arc, ranges, emu)
            assert dev == got and intact and file_len2 == file_len and info2 == info, what


def check_single_is_the_old_call(lib, oracle):
    arc = archive_of("four8192", "all", oracle, True)
    _, data, seams, _ = R.source("four8192", oracle)
    for first, cnt in ((seams[0] - 700, 1500), (seams[2] + 5, 1), (3, 0)):
        assert m.runzip_buffer_ranges(arc, [(first, cnt)], lib=lib) == m.runzip_buffer_range_ex(arc, first, cnt, lib=lib)


def check_refusals(lib, oracle):
    """R.check_refusals with lists: a defect is seen exactly where one of the ranges reaches it; argument errors carry
    the length; a header without a size walks to the end first"""
    parsed, lits, data = R.two_chunk_archive(oracle)
    blk, u_len = B.fuzz_block()
    good = B.frame_mrz(parsed)
    both = data + data
    lists = ([(0, 2 * u_len)], [(u_len - 3, 6), (5, 1)], [(u_len, u_len), (0, 3), (u_len - 3, 6)])
    for ranges in lists:
        got, file_len, _ = m.runzip_buffer_ranges(good, ranges, lib=lib)
        assert got == b"".join(both[a:a + k] for a, k in ranges) and file_len == 2 * u_len

    def rc(arc, ranges):
        return C.rc_of(m.runzip_buffer_ranges, arc, ranges, lib=lib)

    # a mutation of the second chunk's block whose reject lies behind a usable prefix of w bytes (found as there)
    from tests import _lz4_prefix as P
    fx, muts = C.fixture()["fuzz"], B.fuzz_mutations()
    best = None
    for i, mut in enumerate(muts):
        if fx["accept"][i] == "1" or i in fx["offset0"]:
            continue
        for w in range(u_len - 1, 0, -1):
            p = P.ref_prefix(mut, u_len, w)
            if p is not None:
                if p == data[:w] and (best is None or w > best[1]):
                    best = (i, w)
                break
    i, w = best
    lits[1]["payload"] = muts[i]
    bad = B.frame_mrz(parsed)
    assert rc(bad, [(0, 5), (u_len + w, 1)]) == B.E_CORRUPT and rc(bad, [(u_len, u_len)]) == B.E_CORRUPT
    got, _, info = m.runzip_buffer_ranges(bad, [(u_len + 3, w - 3), (10, 20), (u_len, 2)], lib=lib)
    assert got == data[3:w] + data[10:30] + data[:2] and info["s1_lz4_bytes"] == w + 30 and info["chunks_in_range"] == 2
    got, _, info = m.runzip_buffer_ranges(bad, [(10, u_len - 10), (0, 1)], lib=lib)   # the walk stops behind chunk 0
    assert got == data[10:] + data[:1] and info["chunks_in_range"] == 1
    lits[1]["payload"] = blk
    # ctype 6, c_len beyond the archive
    cb = parsed["chunks"][0]["cb"]
    at = good.index(bytes([B.CTYPE_LZ4]) + len(blk).to_bytes(cb, "little") + u_len.to_bytes(cb, "little"))
    other = bytearray(good)
    other[at] = 6
    assert rc(bytes(other), [(0, 10)]) == B.E_UNSUPPORTED
    beyond = bytearray(good)
    beyond[at + 1:at + 1 + cb] = (len(good) + 5).to_bytes(cb, "little")
    assert rc(bytes(beyond), [(0, 10)]) == B.E_CORRUPT
    assert rc(b"MRZX" + good[4:], [(0, 10)]) == B.E_CORRUPT
    # one bad range at each position, against a header with the size and without
    nosize = good[:6] + bytes(8) + good[14:]
    ok = [(0, 4), (u_len, 4), (7, 0)]
    for arc in (good, nosize):
        for bad_range in ((2 * u_len, 1), (0, 2 * u_len + 1), (-1, 2), (3, -1), (2 ** 62, 2 ** 62)):
            for p in range(3):
                ranges = list(ok)
                ranges[p] = bad_range
                try:
                    m.runzip_buffer_ranges(arc, ranges, lib=lib)
                except m.MrzError as e:
                    assert e.rc == E_ARG and e.file_len == 2 * u_len, (bad_range, p)
                else:
                    raise AssertionError((bad_range, p))
    got, file_len, _ = m.runzip_buffer_ranges(nosize, [(u_len - 3, 6), (2 * u_len, 0)], lib=lib)
    assert got == both[u_len - 3:u_len + 3] and file_len == 2 * u_len
    arr, k = binding._byte_ranges(ok)
    fl = ctypes.c_int64(-1)
    call = lib.mrz_runzip_buffer_ranges
    assert call(0, ctypes.c_char_p(good), len(good), arr, k, None, 0, ctypes.byref(fl), None) == E_ARG and fl.value == 2 * u_len
    assert call(0, ctypes.c_char_p(nosize), len(nosize), arr, k, None, 0, ctypes.byref(fl), None) == E_ARG
    assert call(0, ctypes.c_char_p(good), len(good), arr, k, None, 7, None, None) == E_ARG
    assert call(0, ctypes.c_char_p(good), len(good), None, 1, None, 0, None, None) == E_ARG
    assert call(0, ctypes.c_char_p(good), len(good), None, 0, None, 0, ctypes.byref(fl), None) == 0 and fl.value == 2 * u_len
