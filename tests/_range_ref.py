"""Reference for the range decode (mrz_runzip_range / mrz_runzip_origins): where single output bytes of a record stream
come from.  Plain Python over the record lists of tests/_records.py, no GPU.

resolve() is the walk the kernel makes, byte by byte: find the record that holds x; a literal ends the walk at its
stream-1 offset; a match sends x to out_pos - dist + (x - out_pos) % min(len, dist) and counts one hop.
table() reaches the same numbers the other way round -- one forward pass that copies origins the way the decoder copies
bytes -- and serves the whole-output comparisons; tests/test_runzip_range_emu.py checks the two against each other and
against the decoded bytes before any kernel is judged."""
import bisect
import ctypes
import functools

import numpy as np

from modern_rzip_amd import binding
from tests import _records as R

MRZ_E_STATE = -6


Info = binding.RangeInfo   # mrz_range_info


def literal_offsets(records):
    """stream-1 offset of every record's first literal byte (meaningless for matches)"""
    offs, at = [], 0
    for r in records:
        offs.append(at)
        if len(r) == 1:
            at += r[0]
    return offs


def resolve(records, first, count):
    """-> [(origin, hops)] for the output bytes [first, first + count)"""
    pos, total = R.out_positions(records)
    lit = literal_offsets(records)
    assert 0 <= first and first + count <= total
    res = []
    for x in range(first, first + count):
        hops, hi = 0, len(records) - 1
        while True:
            r = bisect.bisect_right(pos, x, 0, hi + 1) - 1
            rec = records[r]
            if len(rec) == 1:
                res.append((lit[r] + x - pos[r], hops))
                break
            ln, dist = rec[0], rec[1]
            x = pos[r] - dist + (x - pos[r]) % min(ln, dist)
            hi = r
            hops += 1
            assert hops <= len(records)
    return res


@functools.lru_cache(maxsize=None)
def table(name):
    """-> (origins int64[out_len], hops int32[out_len]) of a named case, by one forward pass.  Shared; nobody changes it."""
    recs = R.case(name)["records"]
    pos, total = R.out_positions(recs)
    lit = literal_offsets(recs)
    org = np.empty(total, dtype=np.int64)
    hops = np.empty(total, dtype=np.int32)
    for r, a, lo in zip(recs, pos, lit):
        ln = r[0]
        if len(r) == 1:
            org[a:a + ln] = np.arange(lo, lo + ln, dtype=np.int64)
            hops[a:a + ln] = 0
        else:
            n = min(ln, r[1])
            idx = a - r[1] + np.arange(ln, dtype=np.int64) % n   # all of them lie in front of a
            org[a:a + ln] = org[idx]
            hops[a:a + ln] = hops[idx] + 1
    org.setflags(write=False)
    hops.setflags(write=False)
    return org, hops


def expect(name, first, count):
    """-> (origins int64 array, total_hops, max_hops) of a range of a named case"""
    org, hops = table(name)
    h = hops[first:first + count]
    return org[first:first + count], int(h.sum(dtype=np.int64)), int(h.max()) if count else 0


# ---- the ranges the tiers ask for -----------------------------------------------------------------------------------

def wrap_ranges(records):
    """for every match with len > dist: a range inside it that begins behind its first `dist` bytes, where the modulo
    wraps -> [(dist, first, count)]"""
    pos, _ = R.out_positions(records)
    return [(r[1], a + r[1] + 5, min(300, r[0] - r[1] - 5)) for r, a in zip(records, pos)
            if len(r) == 3 and r[0] > r[1] + 5]


@functools.lru_cache(maxsize=None)
def case_ranges(name, randoms=100, seed=1):
    """the (first, count) list of a named case: the whole output, [0, 1), the last byte, an empty range, ranges that begin
    and end on, one before and one after record boundaries, the places where a replicated match wraps (a few), and
    `randoms` seeded random ranges of up to 300 bytes (more than a workgroup's 256)"""
    recs = R.case(name)["records"]
    pos, total = R.out_positions(recs)
    g = R.Rng(seed * 1000 + len(recs))
    out = [(0, total), (0, 1), (total - 1, 1), (total // 2, 0), (total, 0)]
    inner = pos[1:]
    for _ in range(4 if len(inner) > 8 else 1):
        i = g.below(len(inner))
        j = min(len(inner) - 1, i + g.between(0, 5))
        for d1 in (-1, 0, 1):
            for d2 in (-1, 0, 1):
                a, b = inner[i] + d1, min(total, inner[j] + d2)
                out.append((a, max(0, b - a)))
    out += [(a, n) for _, a, n in wrap_ranges(recs)[:12]]
    for _ in range(randoms):
        a = g.below(total)
        out.append((a, g.between(1, min(300, total - a))))
    return tuple(out)


def spans(records, first, count):
    """(literal records, match records) that the range touches"""
    pos, _ = R.out_positions(records)
    lo = bisect.bisect_right(pos, first) - 1
    hi = bisect.bisect_right(pos, first + count - 1) - 1
    kinds = [len(r) for r in records[lo:hi + 1]]
    return kinds.count(1), kinds.count(3)


# ---- the library through ctypes: verdicts included --------------------------------------------------------------------

def _ptr(b):
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) if b else None


def run_range(ctx, s0, s1, cb, first, count, where=0):
    """mrz_runzip_range on host buffers -> (rc, bytes, chunk_len, total_hops, max_hops); chunk_len is -1 where the library
    did not set it.  `where` only tells the library where the streams are (on the emulator both are the same memory)."""
    size = max(0, count) + 16
    buf = ctypes.create_string_buffer(b"\xa5" * size, size)
    info = Info(-1, -1, -1)
    rc = ctx.lib.mrz_runzip_range(ctx.ctx, _ptr(s0), len(s0), _ptr(s1), len(s1), where, cb, first, count, buf, where,
                                  ctypes.byref(info))
    raw = buf.raw
    assert raw[max(0, count):] == b"\xa5" * 16, "bytes behind the range were written"
    return rc, raw[:max(0, count)] if rc == 0 else b"", info.chunk_len, info.total_hops, info.max_hops


def run_origins(ctx, s0, s1_len, cb, first, count, where=0):
    """mrz_runzip_origins -> (rc, int64 array, chunk_len, total_hops, max_hops)"""
    arr = np.full(max(0, count) + 2, -7, dtype=np.int64)
    info = Info(-1, -1, -1)
    rc = ctx.lib.mrz_runzip_origins(ctx.ctx, _ptr(s0), len(s0), s1_len, where, cb, first, count,
                                    ctypes.c_void_p(arr.ctypes.data), where, ctypes.byref(info))
    assert (arr[max(0, count):] == -7).all(), "entries behind the range were written"
    return rc, arr[:max(0, count)], info.chunk_len, info.total_hops, info.max_hops


def check_range(ctx, name, first, count, where=0):
    """bytes, origins and hop statistics of one range of a named case, all exact"""
    c = R.case(name)
    want_org, want_total, want_max = expect(name, first, count)
    what = (name, first, count, where)
    rc, got, n, total, top = run_range(ctx, c["s0"], c["s1"], c["cb"], first, count, where)
    assert rc == R.MRZ_OK and n == len(c["out"]), (what, rc, n)
    if got != c["out"][first:first + count]:
        raise AssertionError(f"{what}: {R.first_difference(got, c['out'][first:first + count], None)}")
    assert (total, top) == (want_total, want_max), (what, total, top, want_total, want_max)
    rc, org, n, total, top = run_origins(ctx, c["s0"], len(c["s1"]), c["cb"], first, count, where)
    assert rc == R.MRZ_OK and n == len(c["out"]), (what, rc, n)
    if not np.array_equal(org, want_org):
        k = int(np.nonzero(org != want_org)[0][0])
        raise AssertionError(f"{what}: origin of byte {first + k}: got {org[k]}, want {want_org[k]}")
    assert (total, top) == (want_total, want_max), (what, total, top, want_total, want_max)


def check_chain_range(ctx, name, first, count, where=0, stats=True):
    """a range of a dependence-chain case against resolve() itself (no table of 8 MiB)"""
    c = R.case(name)
    rc, got, n, total, top = run_range(ctx, c["s0"], c["s1"], c["cb"], first, count, where)
    assert rc == R.MRZ_OK and n == len(c["out"]), (name, rc, n)
    if got != c["out"][first:first + count]:
        raise AssertionError(f"{name} [{first}, +{count}): {R.first_difference(got, c['out'][first:first + count], None)}")
    if stats:
        want = chain_expect(name, first, count)
        assert (total, top) == want[1:], (name, first, count, total, top, want[1:])
        rc, org, n, total, top = run_origins(ctx, c["s0"], len(c["s1"]), c["cb"], first, count, where)
        assert rc == R.MRZ_OK and np.array_equal(org, want[0]) and (total, top) == want[1:], (name, first, count, rc)


@functools.lru_cache(maxsize=None)
def chain_expect(name, first, count):
    res = resolve(R.case(name)["records"], first, count)
    org = np.array([o for o, _ in res], dtype=np.int64)
    org.setflags(write=False)
    return org, sum(h for _, h in res), max(h for _, h in res)


CHAIN_TAIL = 4096
CHAIN_MID = (3 * 8192 - 100, 257)


# ---- the multi-block archive ------------------------------------------------------------------------------------------

ARCHIVE_CHUNKS = ("chunk_cb3", "tiles8k", "chunk_cb5", "overlap8k")


def archive(oracle, ramsize=24576):
    """-> (archive bytes, data, chunk seams): the four chunks framed by the oracle; with the small ramsize the streams are
    cut into blocks of 8192 bytes"""
    import hashlib
    chunks = [R.case(n) for n in ARCHIVE_CHUNKS]
    data = b"".join(c["out"] for c in chunks)
    arch = oracle.frame(len(data), [(1 << 8 * (c["cb"] - 1), c["s0"], c["s1"]) for c in chunks], hashlib.md5(data).digest(),
                        ramsize=ramsize)
    seams, at = [], 0
    for c in chunks[:-1]:
        at += len(c["out"])
        seams.append(at)
    return arch, data, seams


def archive_blocks(arch):
    """walks the headers -> per chunk (cb, [stream-0 block lengths], [stream-1 block lengths]); the empty head that opens
    each chain is not counted"""
    at = 20 + arch[19]
    out = []
    while True:
        cb, eof = arch[at], arch[at + 1]
        at += 2 + cb
        initial = at
        end = initial + 2 * (1 + 3 * cb)
        lens = ([], [])
        for s in (0, 1):
            h = initial + s * (1 + 3 * cb)
            while True:
                assert arch[h] == 3
                c_len = int.from_bytes(arch[h + 1:h + 1 + cb], "little")
                nxt = int.from_bytes(arch[h + 1 + 2 * cb:h + 1 + 3 * cb], "little")
                if h != initial + s * (1 + 3 * cb):
                    lens[s].append(c_len)
                else:
                    assert c_len == 0
                end = max(end, h + 1 + 3 * cb + c_len)
                if not nxt:
                    break
                h = initial + nxt
        out.append((cb, lens[0], lens[1]))
        at = end
        if eof:
            return out


def archive_ranges(data_len, seams, block_seam, randoms=50, seed=5):
    """(first, count): inside each chunk, across each chunk seam, across a block seam of stream 1 (`block_seam` is an
    output position whose origin lies there), the whole file, an empty range, `randoms` random ones"""
    g = R.Rng(seed)
    edges = [0] + list(seams) + [data_len]
    out = [(0, data_len), (data_len, 0), (0, 0)]
    for a, b in zip(edges, edges[1:]):
        out.append((a + (b - a) // 3, min(1000, (b - a) // 3)))
        out.append((a, 1))
        out.append((b - 1, 1))
    for s in seams:
        out += [(s - 1, 2), (s - 700, 1500), (s, 300), (s - 300, 300)]
    out.append((seams[0] - 10, seams[2] - seams[0] + 20))   # two whole chunks and a little of their neighbours
    out.append((block_seam - 200, 400))
    for _ in range(randoms):
        a = g.below(data_len)
        out.append((a, g.between(1, min(20000, data_len - a))))
    return out
