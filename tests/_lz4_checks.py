"""The checks of the LZ4 block codec and of LZ4 archives, shared by the emulator tier (test_lz4_*_emu.py) and the GPU
tier (test_lz4_*_gpu.py).  Every comparison is exact.  Expectations: Oracle.lz4_compress (liblz4 1.9.3's bytes) for the
compressor, tests/_lz4_blocks.ref_decode and tests/golden/lz4_blocks.json (liblz4's own verdicts) for the decoder."""
import base64
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import torch

import modern_rzip_amd as m
from tests import _lz4_blocks as B
from tests import _util
from tests.golden import make_lz4_golden

HERE = os.path.dirname(os.path.abspath(__file__))
CANARY = 0xC5
GAP = 64
CAP_KINDS = ("bound", "n+1", "size+8", "size", "size-1")
# (inputs, outputs) in host or device memory: every combination occurs
CAP_MEMORY = {"bound": ("host", "host"), "n+1": ("device", "device"), "size+8": ("host", "device"),
              "size": ("device", "host"), "size-1": ("host", "host")}
MULTI_CHUNK_RAM = 3 * 16384 // 2 + 3000  # max_chunk = ramsize / 3 * 2, page-rounded: 16 KiB chunks


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "lz4_blocks.json")) as f:
        return json.load(f)


class Slab:
    """`sizes[i]` bytes per slot in one allocation, GAP canary bytes before, between and behind the slots.  where:
    "host" or "device"; on the emulator device memory is host memory handed over as (address, length)."""

    def __init__(self, sizes, where, emu):
        self.sizes = [int(s) for s in sizes]
        self.at, pos = [], GAP
        for s in self.sizes:
            self.at.append(pos)
            pos += s + GAP
        self.t = torch.full((pos,), CANARY, dtype=torch.uint8, device="cuda" if where == "device" and not emu else "cpu")
        if where == "host":
            self.refs = [self.t[a:a + s] for a, s in zip(self.at, self.sizes)]
        else:
            self.refs = [(self.t.data_ptr() + a, s) for a, s in zip(self.at, self.sizes)]

    @classmethod
    def of(cls, blocks, where, emu):
        slab = cls([len(b) for b in blocks], where, emu)
        img = np.full(slab.t.numel(), CANARY, dtype=np.uint8)
        for a, b in zip(slab.at, blocks):
            img[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
        slab.t.copy_(torch.from_numpy(img))
        return slab

    def read(self):
        """(the slots' bytes, canaries intact)"""
        img = self.t.cpu().numpy()
        keep = np.ones(img.size, dtype=bool)
        for a, s in zip(self.at, self.sizes):
            keep[a:a + s] = False
        return [img[a:a + s].tobytes() for a, s in zip(self.at, self.sizes)], bool((img[keep] == CANARY).all())


# ---- compressor ------------------------------------------------------------------------------------------------------

def boundary_input(lit, ml):
    """`lit` literals, then a match of exactly `ml` bytes (a copy from lit - 1 bytes back, so it overlaps itself when
    ml >= lit), then bytes that continue neither"""
    noise = _util.xorshift_noise(lit + 64, seed=1000 * lit + ml)
    d = bytearray(noise[:lit])
    for _ in range(ml):
        d.append(d[-(lit - 1)])
    d.append(d[-(lit - 1)] ^ 0x5A)
    return bytes(d + noise[lit:lit + 24])


def first_sequence(block):
    """(literal length, match length) of a block's first sequence"""
    token, ip = block[0], 1
    lit, ml = token >> 4, token & 15
    if lit == 15:
        while True:
            lit += block[ip]
            ip += 1
            if block[ip - 1] != 255:
                break
    ip += lit + 2
    if ml == 15:
        while True:
            ml += block[ip]
            ip += 1
            if block[ip - 1] != 255:
                break
    return lit, ml + 4


BOUNDARIES = [(14, 24), (15, 24), (16, 24), (270, 24), (20, 18), (20, 19), (20, 20), (20, 274)]


@functools.lru_cache(maxsize=None)
def compress_inputs():
    ins = dict(make_lz4_golden.cases())
    text = _util.zipf_text(13, seed=2)
    for n in (0, 1, 12, 13):
        ins[f"n{n}"] = text[:n]
    for lit, ml in BOUNDARIES:
        ins[f"lit{lit}_match{ml}"] = boundary_input(lit, ml)
    return ins


def cap_of(kind, n, size):
    return {"bound": n + n // 255 + 16, "n+1": n + 1, "size+8": size + 8, "size": size, "size-1": size - 1}[kind]


def check_boundary_inputs(oracle):
    """the hand-made inputs are what they are meant to be: the token fields of the oracle's first sequence"""
    for lit, ml in BOUNDARIES:
        d = compress_inputs()[f"lit{lit}_match{ml}"]
        r, blk = oracle.lz4_compress(d, len(d) + len(d) // 255 + 16)
        assert r > 0 and first_sequence(blk) == (lit, ml), (lit, ml, first_sequence(blk))
        assert (blk[0] >> 4, blk[0] & 15) == (min(lit, 15), min(ml - 4, 15))


def check_compress(ctx, oracle, emu, kind):
    """one batch of all inputs with capacity `kind`: return values, bytes, canaries; then every block that fitted goes
    back through the decoder"""
    ins = compress_inputs()
    names = list(ins)
    sizes = {k: oracle.lz4_size(ins[k], len(ins[k]) + len(ins[k]) // 255 + 16) for k in names}
    caps = [cap_of(kind, len(ins[k]), sizes[k]) for k in names]
    want = [oracle.lz4_compress(ins[k], c) for k, c in zip(names, caps)]
    in_where, out_where = CAP_MEMORY[kind]
    src = Slab.of([ins[k] for k in names], in_where, emu)
    dst = Slab(caps, out_where, emu)
    got = ctx.lz4_compress(src.refs, caps, outs=dst.refs)
    data, intact = dst.read()
    assert intact, f"{kind}: bytes at or beyond a capacity were written"
    for k, g, d, (r, blk) in zip(names, got, data, want):
        assert g == r, (kind, k, g, r)
        assert d[:r] == blk, (kind, k)
    assert src.read()[0] == [ins[k] for k in names]
    fitted = [i for i, g in enumerate(got) if g > 0]
    assert kind != "bound" or len(fitted) == len(names)
    if not fitted:
        return
    back = Slab([len(ins[names[i]]) for i in fitted], in_where, emu)
    _, st = ctx.lz4_decompress([(dst.refs[i][0], got[i]) if out_where == "device" else dst.refs[i][:got[i]]
                                for i in fitted], back.sizes, outs=back.refs)
    data, intact = back.read()
    assert intact and st == [0] * len(fitted), (kind, st)
    assert data == [ins[names[i]] for i in fitted], kind


# ---- decoder ---------------------------------------------------------------------------------------------------------

def decode_batch(ctx, emu, blocks, u_lens, where):
    """-> (outputs or None per block, statuses); canaries around every output and every input checked"""
    src = Slab.of(blocks, where, emu)
    dst = Slab(u_lens, where, emu)
    _, st = ctx.lz4_decompress(src.refs, u_lens, outs=dst.refs)
    data, intact = dst.read()
    assert intact, "the decoder wrote outside an output"
    assert all(s in (0, B.E_CORRUPT) for s in st)
    return [d if s == 0 else None for d, s in zip(data, st)], st


def check_handmade(ctx, emu, where):
    cases = B.handmade_cases()
    fx = fixture()["handmade"]
    assert fx["accept"] == "1" * len(cases)
    outs, st = decode_batch(ctx, emu, [c[1] for c in cases], [c[2] for c in cases], where)
    for (name, blk, u_len), o, s in zip(cases, outs, st):
        assert s == 0 and o == B.ref_decode(blk, u_len), name
    assert B.group_digest([True] * len(cases), outs) == fx["digest"]


def check_hc(ctx, emu):
    from tests.golden import make_lz4_blocks_golden
    ins = make_lz4_blocks_golden.hc_inputs()
    blocks = [base64.b64decode(fixture()["hc"][k]["payload"]) for k in ins]
    for where in ("host", "device"):
        outs, st = decode_batch(ctx, emu, blocks, [len(d) for d in ins.values()], where)
        assert st == [0, 0] and outs == list(ins.values())
    assert [B.sha(d) for d in ins.values()] == [fixture()["hc"][k]["sha256"] for k in ins]


def check_rejects(ctx, emu, where):
    """every malformed block between two good ones, in one batch"""
    mal = B.malformed_cases()
    fx = fixture()["malformed"]
    assert fx["accept"] == "0" * len(mal) and not fx["sha256"]
    assert set(fx["offset0"]) == {"offset0", "offset0_first"}
    good, good_u = B.fuzz_block()
    want_good = B.ref_decode(good, good_u)
    blocks, u_lens = [good], [good_u]
    for _, blk, u_len in mal:
        blocks += [blk, good]
        u_lens += [u_len, good_u]
    outs, st = decode_batch(ctx, emu, blocks, u_lens, where)
    for i, (name, blk, u_len) in enumerate(mal):
        assert st[2 * i + 1] == B.E_CORRUPT and B.ref_decode(blk, u_len) is None, name
    assert st[0::2] == [0] * (len(mal) + 1) and all(o == want_good for o in outs[0::2])


def check_fuzz(ctx, emu, where):
    """2000 single-bit mutations in one batch: liblz4's verdict (offset 0: reject) and the digests of what it decoded"""
    fx = fixture()["fuzz"]
    muts = B.fuzz_mutations()
    u_len = B.fuzz_block()[1]
    assert len(muts) == len(fx["accept"]) == 2000
    outs, st = decode_batch(ctx, emu, muts, [u_len] * len(muts), where)
    verdicts = [s == 0 for s in st]
    wrong = [i for i, v in enumerate(verdicts) if v != (fx["accept"][i] == "1")]
    assert not wrong, f"verdicts differ from liblz4's at mutations {wrong[:10]}"
    assert all(not verdicts[i] for i in fx["offset0"])
    for i in range(0, len(muts), B.FUZZ_GROUP):
        got = B.group_digest(verdicts[i:i + B.FUZZ_GROUP], [o or b"" for o in outs[i:i + B.FUZZ_GROUP]])
        assert got == fx["groups"][i // B.FUZZ_GROUP], f"outputs of mutations {i}..{i + B.FUZZ_GROUP - 1}"
    assert 0 < sum(verdicts) < len(verdicts)


def check_args(ctx):
    """lengths above 0x7E000000 and null buffers with non-zero lengths"""
    lib = ctx.lib
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.cast(buf, vp)
    out_lens, status = (i64 * 1)(), (ctypes.c_int32 * 1)()
    for src, n, dst, room in ((ptr, 0x7E000001, ptr, 64), (vp(None), 8, ptr, 64), (ptr, 8, vp(None), 64),
                              (ptr, -1, ptr, 64), (ptr, 8, ptr, -1)):
        a, b, c, d = (vp * 1)(src), (i64 * 1)(n), (vp * 1)(dst), (i64 * 1)(room)
        assert lib.mrz_lz4_compress_batch(ctx.ctx, a, b, 1, m.MEM_HOST, c, d, m.MEM_HOST, out_lens) == -1
        assert lib.mrz_lz4_decompress_batch(ctx.ctx, a, b, 1, m.MEM_HOST, c, d, m.MEM_HOST, status) == -1
    a, b, c, d = (vp * 1)(ptr), (i64 * 1)(8), (vp * 1)(ptr), (i64 * 1)(0x7E000001)
    assert lib.mrz_lz4_decompress_batch(ctx.ctx, a, b, 1, m.MEM_HOST, c, d, m.MEM_HOST, status) == -1
    assert lib.mrz_lz4_compress_batch(ctx.ctx, a, b, 0, m.MEM_HOST, c, d, m.MEM_HOST, out_lens) == 0
    assert buf.raw == bytes(64)


def check_abi(lib):
    assert lib.mrz_abi_version() == 4
    for name in ("mrz_lz4_bound", "mrz_lz4_compress_batch", "mrz_lz4_decompress_batch"):
        assert hasattr(lib, name), name
    assert [lib.mrz_lz4_bound(n) for n in (0, 255, 0x7E000000)] == [16, 255 + 1 + 16, 0x7E000000 + 0x7E000000 // 255 + 16]
    assert lib.mrz_lz4_bound(0x7E000001) < 0 and lib.mrz_lz4_bound(1 << 40) < 0


# ---- archives --------------------------------------------------------------------------------------------------------

def archive_inputs(big):
    g = _util.golden_inputs()
    ins = {k: g[k] for k in ("empty", "range30", "a1000", "range256x64", "seed42x64")}
    ins["text"] = _util.zipf_text(150000, seed=8)
    if big:
        ins["syn64_4m"] = g["syn64"][:4 << 20]
    return ins


def rc_of(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except m.MrzError as e:
        return e.rc
    return 0


def lz4_count(mrz):
    return sum(b["ctype"] == B.CTYPE_LZ4 for ch in B.parse_mrz(mrz)["chunks"] for b in ch["blocks"])


def check_reframed(lib, oracle, data, **kw):
    """all blocks of >= 64 bytes as LZ4 in streams re-cut at 4096 bytes, then alternating LZ4 / NONE"""
    arc = oracle.compress(data, **kw)[0]
    assert m.runzip_buffer(arc, lib=lib) == data
    every = B.reframe(arc, oracle, block_size=4096)
    assert m.runzip_buffer(every, lib=lib) == data
    if len(data) >= 64:
        assert lz4_count(every) > 0
    other = B.reframe(arc, oracle, block_size=4096, choose=lambda i, d: i % 2 == 0 and len(d) > 0)
    assert m.runzip_buffer(other, lib=lib) == data
    return every


def check_expanding(lib, oracle, n=30000):
    data = _util.xorshift_noise(n, seed=77)
    arc = B.reframe(oracle.compress(data)[0], oracle)
    blocks = [b for ch in B.parse_mrz(arc)["chunks"] for b in ch["blocks"] if b["ctype"] == B.CTYPE_LZ4]
    assert any(b["c_len"] > b["u_len"] for b in blocks)
    assert m.runzip_buffer(arc, lib=lib) == data


def check_archive_errors(lib, oracle):
    # The fuzz block as the only literal block of an archive: the archive of u_len bytes of noise has one literal
    # record over all of stream 1, so swapping that block for the fuzz block (and the MD5 for that of what it decodes
    # to) gives a valid archive of those bytes, and its mutations give the fixture's verdicts a whole-archive form.
    blk, u_len = B.fuzz_block()
    data = B.ref_decode(blk, u_len)
    noise = _util.xorshift_noise(u_len, seed=3)
    parsed = B.parse_mrz(oracle.compress(noise)[0])
    lits = [b for b in parsed["chunks"][0]["blocks"] if b["stream"] == 1]
    assert len(parsed["chunks"]) == 1 and len(lits) == 1 and lits[0]["payload"] == noise
    lits[0].update(ctype=B.CTYPE_LZ4, payload=blk)
    parsed["tail"] = hashlib.md5(data).digest()
    good = B.frame_mrz(parsed)
    assert m.runzip_buffer(good, lib=lib) == data
    fx = fixture()["fuzz"]
    muts = B.fuzz_mutations()
    i = next(i for i in range(len(muts)) if fx["accept"][i] == "0" and i not in fx["offset0"])
    lits[0]["payload"] = muts[i]
    assert rc_of(m.runzip_buffer, B.frame_mrz(parsed), lib=lib) == B.E_CORRUPT
    lits[0]["payload"] = muts[fx["offset0"][0]]
    assert rc_of(m.runzip_buffer, B.frame_mrz(parsed), lib=lib) == B.E_CORRUPT
    # c_len beyond the archive, c_len beyond LZ4_compressBound(u_len), an unknown ctype
    lits[0]["payload"] = blk
    cb = parsed["chunks"][0]["cb"]
    at = good.index(bytes([B.CTYPE_LZ4]) + len(blk).to_bytes(cb, "little") + u_len.to_bytes(cb, "little"))
    beyond = bytearray(good)
    beyond[at + 1:at + 1 + cb] = (len(good) + 5).to_bytes(cb, "little")
    assert rc_of(m.runzip_buffer, bytes(beyond), lib=lib) == B.E_CORRUPT
    short = bytearray(good)
    short[at + 1 + cb:at + 1 + 2 * cb] = (len(blk) - len(blk) // 255 - 17).to_bytes(cb, "little")
    assert rc_of(m.runzip_buffer, bytes(short), lib=lib) == B.E_CORRUPT
    other = bytearray(good)
    other[at] = 6
    assert rc_of(m.runzip_buffer, bytes(other), lib=lib) == B.E_UNSUPPORTED
    # range decode stays with CTYPE_NONE
    assert rc_of(m.runzip_buffer_range, good, 0, 10, lib=lib) == B.E_UNSUPPORTED


def lz4_block_size(n, ramsize, threads, page=4096):
    """open_stream_out with a back-end, as include/mrzgpu_host.h states it"""
    up = lambda v: (v + page - 1) // page * page  # noqa: E731
    max_chunk = ramsize // 3 * 2
    if max_chunk < n:
        max_chunk = max_chunk // page * page
    chunk_limit = max(min(n, max_chunk), page)
    limit = ramsize // 3 // 2
    if 0 < n < limit:
        limit = max(n, 10 << 20)
    elif limit > chunk_limit:
        limit = chunk_limit
    nthreads = threads + 1 if threads > 1 else 1
    return up(min(limit, max(limit // nthreads, 10 << 20)))


def check_writer(lib, oracle, data, level=2, threads=1, ramsize=60 << 30):
    """an independent parse of what mrz_rzip_buffer_lz4 wrote, against the -n path with the same control"""
    arc, st, md5 = m.rzip_buffer_lz4(data, level=level, threads=threads, ramsize=ramsize, lib=lib)
    plain, pst, pmd5 = m.rzip_buffer(data, level=level, ramsize=ramsize, lib=lib)
    assert md5 == pmd5 == hashlib.md5(data).digest() and st.as_dict() == pst.as_dict()
    got, want = B.parse_mrz(arc), B.parse_mrz(plain)
    assert got["head"] == want["head"] and got["tail"] == want["tail"] and arc[-16:] == md5
    assert got["head"][18] == (level << 4 | level)
    assert len(got["chunks"]) == len(want["chunks"])
    bs = lz4_block_size(len(data), ramsize, threads)
    for g, w in zip(got["chunks"], want["chunks"]):
        assert (g["cb"], g["eof"], g["size_field"]) == (w["cb"], w["eof"], w["size_field"])
        for b in g["blocks"]:
            if b["u_len"] >= 64:
                assert b["ctype"] == B.CTYPE_LZ4
                held = B.ref_decode(b["payload"], b["u_len"])
                assert held is not None
                r, blk = oracle.lz4_compress(held, b["u_len"] + b["u_len"] // 255 + 16)
                assert b["payload"] == blk and b["c_len"] == r
            else:
                assert b["ctype"] == B.CTYPE_NONE and b["c_len"] == b["u_len"]
        assert B.streams_of(g, B.ref_decode) == B.streams_of(w)
        for s in range(2):  # every block of a stream but its last is one full buffer
            lens = [b["u_len"] for b in g["blocks"] if b["stream"] == s]
            assert all(n == bs for n in lens[:-1]) and 0 <= lens[-1] <= bs, (s, lens, bs)
    assert m.runzip_buffer(arc, lib=lib) == data
    return got
