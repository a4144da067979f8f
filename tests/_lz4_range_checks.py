"""The checks of mrz_runzip_buffer_range_ex (range decode over archives with LZ4 blocks), shared by the emulator tier and
the GPU tier.  Archives: the oracle's -n output of tests/_lz4_checks.archive_inputs and the four-chunk archive of
tests/_range_ref.archive, re-cut and re-framed by tests/_lz4_blocks.reframe.  Every comparison is exact, the accounting
included: what a range must touch is derived from the origins mrz_runzip_origins gives on the -n streams."""
import ctypes
import functools
import hashlib

import numpy as np
import torch

import modern_rzip_amd as m
from tests import _lz4_blocks as B
from tests import _lz4_checks as C
from tests import _lz4_prefix as P
from tests import _range_ref as RR
from tests import _records
from tests import _util

E_ARG = -1
FRAMINGS = ("all", "stream1", "alternating")
ARCHIVES = sorted(C.archive_inputs(False)) + ["four4096", "four8192"]
_cache = {}


def source(name, oracle):
    """-> (the -n archive cut into blocks, all CTYPE_NONE; data; chunk seams; block size)"""
    if name not in _cache:
        if name.startswith("four"):
            arch, data, seams = RR.archive(oracle, ramsize=60 << 30)
            bs = int(name[4:])
        else:
            data, seams, bs = C.archive_inputs(False)[name], [], 4096
            arch = oracle.compress(data)[0]
        _cache[name] = (B.reframe(arch, oracle, block_size=bs, choose=lambda i, d: False), data, seams, bs)
    return _cache[name]


def framed(name, framing, oracle):
    """the three framings of an archive: every block of >= 64 bytes LZ4; only stream 1's (non-empty) blocks; alternating
    LZ4 / NONE by the block's index in its chunk"""
    key = (name, framing)
    if key not in _cache:
        cut, _, _, bs = source(name, oracle)
        if framing == "all":
            choose = None
        elif framing == "alternating":
            choose = lambda i, d: i % 2 == 0 and len(d) > 0  # noqa: E731
        else:  # reframe() lists a chunk's stream-0 blocks first
            n0 = [sum(b["stream"] == 0 for b in ch["blocks"]) for ch in B.parse_mrz(cut)["chunks"]]
            chunk = [-1]

            def choose(i, d):
                chunk[0] += i == 0
                return i >= n0[chunk[0]] and len(d) > 0
        _cache[key] = B.reframe(cut, oracle, block_size=bs, choose=choose)
    return _cache[key]


@functools.lru_cache(maxsize=None)
def four_block_seam(bs):
    """a position inside tiles8k (the second chunk) whose byte is the first of stream 1's second block of `bs` bytes"""
    org, _ = RR.table("tiles8k")
    return int(np.nonzero((org[1:] == bs) & (org[:-1] == bs - 1))[0][0]) + 1


def ranges_of(name, data, seams, bs, chunk_origins):
    n = len(data)
    if seams:
        return RR.archive_ranges(n, seams, seams[0] + four_block_seam(bs), randoms=2)
    out = [(0, n), (n, 0), (0, 0)]
    if n:
        out += [(0, 1), (n - 1, 1), (n // 3, min(1000, n // 3))]
        hit = np.nonzero(chunk_origins == bs)[0]  # a byte whose origin opens stream 1's second block
        if len(hit):
            a = max(0, int(hit[0]) - 200)
            out.append((a, min(400, n - a)))
        g = _records.Rng(len(data) + 3)
        for _ in range(8):
            a = g.below(n)
            out.append((a, g.between(1, min(20000, n - a))))
    return out


class Plan:
    """what a range must cost: per chunk of the -n form the streams and the decoded length, per chunk of the framed
    archive the stream-1 block table"""

    def __init__(self, ctx, cut, arc, name):
        self.ctx = ctx
        self.name = name
        self.size_known = int.from_bytes(arc[6:14], "little") > 0
        self.chunks = []
        for chn, chf in zip(B.parse_mrz(cut)["chunks"], B.parse_mrz(arc)["chunks"]):
            s0, s1 = B.streams_of(chn)
            _, inf = ctx.runzip_origins(s0, len(s1), chn["cb"], 0, 0)
            lit = [b for b in chf["blocks"] if b["stream"] == 1]
            self.chunks.append(dict(
                s0=s0, s1_len=len(s1), cb=chn["cb"], eof=chn["eof"], out_len=inf["chunk_len"], blocks=lit,
                starts=np.cumsum([0] + [b["u_len"] for b in lit[:-1]]).astype(np.int64),
                s0_lz4=sum(b["u_len"] for b in chf["blocks"] if b["stream"] == 0 and b["ctype"] == B.CTYPE_LZ4)))

    def origins(self, k, lo, cnt):
        """computed once per archive and range, shared by the framings (the -n streams are the same); nobody changes it"""
        key = ("origins", id(self.ctx.lib), self.name, k, lo, cnt)
        if key not in _cache:
            c = self.chunks[k]
            org, inf = self.ctx.runzip_origins(c["s0"], c["s1_len"], c["cb"], lo, cnt)
            org.setflags(write=False)
            _cache[key] = (org, inf)
        return _cache[key]

    def expect(self, first, count):
        exp = dict.fromkeys(("chunks_in_range", "total_hops", "max_hops", "s0_lz4_bytes", "s1_blocks_touched",
                             "s1_lz4_bytes", "s1_bytes_uploaded"), 0)
        if self.size_known and count == 0:
            return exp
        total = 0
        for k, c in enumerate(self.chunks):
            exp["s0_lz4_bytes"] += c["s0_lz4"]
            a, b = max(first, total), min(first + count, total + c["out_len"])
            if count > 0 and a < b:
                org, inf = self.origins(k, a - total, b - a)
                exp["chunks_in_range"] += 1
                exp["total_hops"] += inf["total_hops"]
                exp["max_hops"] = max(exp["max_hops"], inf["max_hops"])
                which = np.searchsorted(c["starts"], org, side="right") - 1
                for t in np.unique(which):
                    blk, off = c["blocks"][t], org[which == t] - c["starts"][t]
                    low, high = int(off.min()), int(off.max())
                    assert 0 <= low <= high < blk["u_len"]
                    exp["s1_blocks_touched"] += 1
                    if blk["ctype"] == B.CTYPE_LZ4:
                        exp["s1_lz4_bytes"] += high + 1
                        exp["s1_bytes_uploaded"] += blk["c_len"]
                    else:
                        exp["s1_bytes_uploaded"] += high - low + 1
            total += c["out_len"]
            if (self.size_known and total >= first + count) or c["eof"]:
                break
        return exp


def to_device(lib, arc, first, count, emu):
    """the range into `device` memory of count + 64 pattern bytes -> (bytes, the 64 behind them untouched, file_len, info)"""
    t = torch.full((count + 64,), 0xA5, dtype=torch.uint8, device="cpu" if emu else "cuda")
    _, file_len, info = m.runzip_buffer_range_ex(arc, first, count, out=(t.data_ptr(), count + 64), lib=lib)
    raw = t.cpu().numpy().tobytes()
    return raw[:count], raw[count:] == b"\xa5" * 64, file_len, info


def check_archive(lib, ctx, oracle, emu, name, framing):
    cut, data, seams, bs = source(name, oracle)
    arc = framed(name, framing, oracle)
    lz4 = C.lz4_count(arc)
    if lz4:
        assert C.rc_of(m.runzip_buffer_range, arc, 0, min(1, len(data)), lib=lib) == B.E_UNSUPPORTED  # the old call's contract
    if framing == "stream1":
        assert all(b["ctype"] == B.CTYPE_NONE for ch in B.parse_mrz(arc)["chunks"] for b in ch["blocks"] if b["stream"] == 0)
    if len(data) >= 4096:
        assert lz4 > 0
    plan = Plan(ctx, cut, arc, name)
    assert sum(c["out_len"] for c in plan.chunks) == len(data)
    whole0 = plan.origins(0, 0, plan.chunks[0]["out_len"])[0] if plan.chunks[0]["out_len"] else np.zeros(0, np.int64)
    for k, (first, count) in enumerate(ranges_of(name, data, seams, bs, whole0)):
        what = (name, framing, first, count)
        got, file_len, info = m.runzip_buffer_range_ex(arc, first, count, lib=lib)
        assert file_len == len(data), what
        assert got == data[first:first + count], what
        assert (got, file_len) == m.runzip_buffer_range(cut, first, count, lib=lib), what
        assert info == plan.expect(first, count), (what, info, plan.expect(first, count))
        if k % 6 == 3:  # the same into device memory
            dev, intact, file_len2, info2 = to_device(lib, arc, first, count, emu)
            assert dev == got and intact and file_len2 == file_len and info2 == info, what


def check_one_byte(lib, ctx, oracle):
    """one byte: one block, decoded as far as that byte; the chunks in front of it add nothing to the s1 fields"""
    cut, data, seams, bs = source("four8192", oracle)
    arc = framed("four8192", "all", oracle)
    plan = Plan(ctx, cut, arc, "four8192")
    x = four_block_seam(bs) + 300   # in the second chunk, in the second block of its stream 1
    org, _ = plan.origins(1, x, 1)
    t, off = divmod(int(org[0]), bs)
    blk = plan.chunks[1]["blocks"][t]
    assert blk["ctype"] == B.CTYPE_LZ4 and t >= 1 and plan.chunks[1]["starts"][t] == t * bs
    got, _, info = m.runzip_buffer_range_ex(arc, seams[0] + x, 1, lib=lib)
    assert got == data[seams[0] + x:seams[0] + x + 1]
    assert (info["chunks_in_range"], info["s1_blocks_touched"], info["s1_lz4_bytes"], info["s1_bytes_uploaded"]) == \
        (1, 1, off + 1, blk["c_len"]), info
    # the first byte of the file: the walk ends behind the first chunk, whose stream 0 alone was decoded
    got, _, info = m.runzip_buffer_range_ex(arc, 0, 1, lib=lib)
    assert got == data[:1] and info["s0_lz4_bytes"] == plan.chunks[0]["s0_lz4"] and info["s1_blocks_touched"] == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------

def two_chunk_archive(oracle):
    """The fuzz block as the only literal block of a chunk (tests/_lz4_checks.check_archive_errors), and that chunk twice:
    -> (parsed archive, its two literal blocks, data of one chunk).  One literal record covers all of stream 1, so output
    byte x of a chunk has origin x."""
    blk, u_len = B.fuzz_block()
    data = B.ref_decode(blk, u_len)
    noise = _util.xorshift_noise(u_len, seed=3)
    parsed = B.parse_mrz(oracle.compress(noise)[0])
    ch = parsed["chunks"][0]
    lits = [b for b in ch["blocks"] if b["stream"] == 1]
    assert len(parsed["chunks"]) == 1 and len(lits) == 1 and lits[0]["payload"] == noise
    lits[0].update(ctype=B.CTYPE_LZ4, payload=blk)
    second = dict(ch, blocks=[dict(b) for b in ch["blocks"]])
    ch["eof"] = 0
    parsed["chunks"].append(second)
    head = bytearray(parsed["head"])
    head[6:14] = (2 * u_len).to_bytes(8, "little")
    parsed["head"] = bytes(head)
    parsed["tail"] = hashlib.md5(data + data).digest()
    return parsed, [lits[0], next(b for b in second["blocks"] if b["stream"] == 1)], data


def check_refusals(lib, oracle):
    parsed, lits, data = two_chunk_archive(oracle)
    blk, u_len = B.fuzz_block()
    good = B.frame_mrz(parsed)
    assert m.runzip_buffer(good, lib=lib) == data + data
    for first, count in ((0, 2 * u_len), (u_len - 3, 6), (u_len, u_len), (5, 1)):
        got, file_len, _ = m.runzip_buffer_range_ex(good, first, count, lib=lib)
        assert got == (data + data)[first:first + count] and file_len == 2 * u_len
    assert C.rc_of(m.runzip_buffer_range, good, 0, 10, lib=lib) == B.E_UNSUPPORTED   # the old call keeps its contract

    def rc(arc, first, count):
        return C.rc_of(m.runzip_buffer_range_ex, arc, first, count, lib=lib)

    # a rejected mutation whose reject lies behind a usable prefix: ref_prefix says where the cut may be
    fx = C.fixture()["fuzz"]
    muts = B.fuzz_mutations()
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
    assert 64 < w < u_len and P.ref_prefix(muts[i], u_len, w + 1) is None and B.ref_decode(muts[i], u_len) is None
    # ... in the second chunk: a range that reaches its byte w is refused, one that ends at byte w - 1 is not; nor is a
    # range in the first chunk; the whole-archive decode refuses
    lits[1]["payload"] = muts[i]
    bad = B.frame_mrz(parsed)
    assert C.rc_of(m.runzip_buffer, bad, lib=lib) == B.E_CORRUPT
    assert rc(bad, u_len, u_len) == B.E_CORRUPT and rc(bad, u_len + w, 1) == B.E_CORRUPT and rc(bad, 0, 2 * u_len) == B.E_CORRUPT
    got, _, info = m.runzip_buffer_range_ex(bad, u_len, w, lib=lib)
    assert got == data[:w] and info["s1_lz4_bytes"] == w
    got, _, info = m.runzip_buffer_range_ex(bad, 10, u_len - 10, lib=lib)
    assert got == data[10:] and info["chunks_in_range"] == 1
    # ... in the first chunk, the range in the second
    lits[0]["payload"], lits[1]["payload"] = muts[i], blk
    bad = B.frame_mrz(parsed)
    got, _, _ = m.runzip_buffer_range_ex(bad, u_len, u_len, lib=lib)
    assert got == data and rc(bad, u_len - 1, 2) == B.E_CORRUPT
    lits[0]["payload"] = muts[fx["offset0"][0]]   # the deliberate difference to liblz4
    assert rc(B.frame_mrz(parsed), 0, u_len) == B.E_CORRUPT
    lits[0]["payload"] = blk
    # ctype 6, c_len beyond the archive, a range beyond the file
    cb = parsed["chunks"][0]["cb"]
    at = good.index(bytes([B.CTYPE_LZ4]) + len(blk).to_bytes(cb, "little") + u_len.to_bytes(cb, "little"))
    other = bytearray(good)
    other[at] = 6
    assert rc(bytes(other), 0, 10) == B.E_UNSUPPORTED
    beyond = bytearray(good)
    beyond[at + 1:at + 1 + cb] = (len(good) + 5).to_bytes(cb, "little")
    assert rc(bytes(beyond), 0, 10) == B.E_CORRUPT
    for first, count in ((2 * u_len, 1), (0, 2 * u_len + 1), (-1, 2), (3, -1)):
        try:
            m.runzip_buffer_range_ex(good, first, count, lib=lib)
        except m.MrzError as e:
            assert e.rc == E_ARG and e.file_len == 2 * u_len
        else:
            raise AssertionError((first, count))
    nosize = bytearray(good)   # a header without a size: the walk runs to the end and still answers with the length
    nosize[6:14] = bytes(8)
    got, file_len, _ = m.runzip_buffer_range_ex(bytes(nosize), u_len - 3, 6, lib=lib)
    assert got == (data + data)[u_len - 3:u_len + 3] and file_len == 2 * u_len
    try:
        m.runzip_buffer_range_ex(bytes(nosize), 2 * u_len, 1, lib=lib)
    except m.MrzError as e:
        assert e.rc == E_ARG and e.file_len == 2 * u_len
    else:
        raise AssertionError("a range beyond a file without a size in its header")
    assert lib.mrz_runzip_buffer_range_ex(0, ctypes.c_char_p(good), len(good), 0, 4, None, 0, None, None) == E_ARG
    assert lib.mrz_runzip_buffer_range_ex(0, ctypes.c_char_p(good), len(good), 0, 4, None, 7, None, None) == E_ARG
