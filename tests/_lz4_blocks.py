"""Shared by the LZ4 codec and archive tests (both tiers) and by golden/make_lz4_blocks_golden.py: a builder of LZ4
blocks from sequences, a byte-wise reference decoder with liblz4 1.9.3's accept rules (offset 0 rejected), the
hand-built / malformed / fuzz cases, and a parser and re-framer of .mrz archives (layout: SURVEY section 8 f-1)."""
import hashlib
import random

from tests import _util

CTYPE_NONE, CTYPE_LZ4 = 3, 5
E_UNSUPPORTED, E_CORRUPT = -8, -7


# ---- blocks ----------------------------------------------------------------------------------------------------------

def _ext(v):
    """the bytes that follow a 15 in a token nibble"""
    return b"\xff" * (v // 255) + bytes([v % 255])


def build_block(seqs, last):
    """seqs: [(literals, offset, match_len)], match_len >= 4; last: the literals of the closing sequence."""
    out = bytearray()
    for lit, offset, ml in seqs:
        assert ml >= 4 and 0 <= offset <= 0xFFFF
        out.append(min(len(lit), 15) << 4 | min(ml - 4, 15))
        if len(lit) >= 15:
            out += _ext(len(lit) - 15)
        out += lit
        out += bytes([offset & 255, offset >> 8])
        if ml - 4 >= 15:
            out += _ext(ml - 4 - 15)
    out.append(min(len(last), 15) << 4)
    if len(last) >= 15:
        out += _ext(len(last) - 15)
    out += last
    return bytes(out)


def expand(seqs, last):
    """what a block of these sequences decodes to"""
    out = bytearray()
    for lit, offset, ml in seqs:
        out += lit
        assert 0 < offset <= len(out)
        for _ in range(ml):
            out.append(out[-offset])
    return bytes(out + last)


def ref_decode(src, u_len, why=None):
    """LZ4_decompress_safe(src, dst, len(src), u_len) of liblz4 1.9.3, byte by byte: the bytes when it returns u_len,
    None otherwise -- and None for an offset of 0, which liblz4 accepts (why, a list, then receives "offset0")."""
    n = len(src)
    if n == 0:
        return None
    if u_len == 0:
        return b"" if src == b"\0" else None
    out = bytearray()
    ip = 0
    while True:
        if ip >= n:
            return None
        token = src[ip]
        ip += 1
        lit, ml = token >> 4, token & 15
        unchecked = False
        if lit != 15 and ip < n - 16 and len(out) <= u_len - 32:  # liblz4's shortcut
            out += src[ip:ip + lit]
            ip += lit
            offset = src[ip] | src[ip + 1] << 8
            ip += 2
            unchecked = ml != 15 and 8 <= offset <= len(out)
        else:
            if lit == 15:
                if ip >= n - 15:
                    return None
                while True:
                    s = src[ip]
                    ip += 1
                    lit += s
                    if ip >= n - 15 or s != 255:
                        break
            if lit > n - ip or lit > u_len - len(out):
                return None
            if len(out) + lit > u_len - 12 or ip + lit > n - 8:
                if ip + lit != n:
                    return None
                out += src[ip:ip + lit]
                return bytes(out) if len(out) == u_len else None
            out += src[ip:ip + lit]
            ip += lit
            offset = src[ip] | src[ip + 1] << 8
            ip += 2
        if ml == 15:
            while True:
                if ip >= n - 5:
                    return None
                s = src[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += 4
        if offset == 0:
            if why is not None:
                why.append("offset0")
            return None
        if offset > len(out) or ml > u_len - len(out):
            return None
        if not unchecked and len(out) + ml > u_len - 5:
            return None
        if offset >= ml:
            out += out[len(out) - offset:len(out) - offset + ml]
        else:
            period = bytes(out[len(out) - offset:])
            out += (period * (ml // offset + 1))[:ml]


# ---- cases -----------------------------------------------------------------------------------------------------------

OFFSETS = (1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256)
MATCH_LENS = (4, 5, 18, 19, 20, 273, 274, 275, 1000)
_TEXT = None


def _text(n, at=0):
    global _TEXT
    if _TEXT is None:
        _TEXT = _util.zipf_text(1 << 17, seed=11)
    return _TEXT[at:at + n]


def handmade_cases():
    """[(name, block, u_len)]: 148 well-formed blocks"""
    cases = []
    for off in OFFSETS:
        for ml in MATCH_LENS:
            seqs, last = [(_text(max(off, 3), off * 7 + ml), off, ml)], _text(12, 900 + ml)
            cases.append((f"off{off}_len{ml}", build_block(seqs, last), len(expand(seqs, last))))
    seqs, last = [(_text(65535), 65535, 70000)], _text(12, 5)
    cases.append(("off65535_len70000", build_block(seqs, last), len(expand(seqs, last))))
    seqs = [(_text(1, i), 1, 4) for i in range(10000)]
    cases.append(("seq10000", build_block(seqs, last), len(expand(seqs, last))))
    cases.append(("lit271", build_block([], _text(271, 40)), 271))
    cases.append(("empty", b"\0", 0))
    assert len(cases) == 148
    return cases


def fuzz_block():
    """(block, u_len): 12 sequences in 301 bytes -- long and short literal runs, extended match lengths (one with a
    255), overlapping and distant matches"""
    shape = [(20, 3, 7), (5, 1, 30), (0, 16, 4), (14, 8, 18), (3, 40, 300), (1, 2, 5), (15, 64, 19), (30, 100, 12),
             (2, 17, 33), (8, 255, 6), (40, 7, 20)]
    seqs, at = [], 0
    for lit, off, ml in shape:
        seqs.append((_text(lit, 3000 + at), off, ml))
        at += lit
    head = build_block(seqs, b"")[:-1]
    last = _text(301 - len(head) - 2, 3000 + at)
    blk = build_block(seqs, last)
    assert len(blk) == 301 and len(seqs) == 11
    return blk, len(expand(seqs, last))


def fuzz_mutations(count=2000, seed=20240):
    """`count` seeded single-bit mutations of fuzz_block()"""
    blk, _ = fuzz_block()
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        bit = rng.randrange(len(blk) * 8)
        m = bytearray(blk)
        m[bit >> 3] ^= 1 << (bit & 7)
        out.append(bytes(m))
    return out


def malformed_cases():
    """[(name, block, u_len)]: every one is a reject"""
    blk, u = fuzz_block()
    cases = [(f"prefix{k}", blk[:k], u) for k in range(1, len(blk))]
    for t in range(5):  # a match, then 0..4 closing literals
        seqs, last = [(_text(20, 77), 5, 9)], _text(t, 200)
        cases.append((f"tail{t}", build_block(seqs, last), len(expand(seqs, last))))
    cases.append(("ulen_plus1", blk, u + 1))
    cases.append(("ulen_minus1", blk, u - 1))
    seqs, last = [(_text(10, 9), 11, 8)], _text(12, 300)
    cases.append(("offset_beyond", build_block(seqs, last), 10 + 8 + 12))
    seqs = [(_text(10, 9), 0, 8)]
    cases.append(("offset0", build_block(seqs, last), 10 + 8 + 12))
    cases.append(("offset0_first", build_block([(b"", 0, 8)], last), 8 + 12))
    cases.append(("lit_beyond_input", bytes([0xF0, 200]) + _text(100, 50), 215))
    cases.append(("lit_chain_to_end", bytes([0xF0]) + b"\xff" * 40, 4096))
    cases.append(("match_chain_to_end", bytes([0x4F]) + _text(4, 1) + b"\x02\x00" + b"\xff" * 40, 16384))
    cases.append(("clen0", b"", 16))
    cases.append(("clen0_ulen0", b"", 0))
    return cases


def sha(b):
    return hashlib.sha256(b).hexdigest()


def group_digest(verdicts, outputs):
    """one sha256 over a group of cases: per case its verdict byte and the sha256 of its output (zeros on reject)"""
    h = hashlib.sha256()
    for ok, out in zip(verdicts, outputs):
        h.update(bytes([1 if ok else 0]))
        h.update(hashlib.sha256(out).digest() if ok else bytes(32))
    return h.hexdigest()


FUZZ_GROUP = 100


# ---- .mrz archives ---------------------------------------------------------------------------------------------------

def _le(v, width):
    return int(v).to_bytes(width, "little")


def parse_mrz(mrz):
    """-> dict(head, chunks, tail); a chunk: dict(cb, eof, size_field, blocks); a block: dict(stream, ctype, c_len,
    u_len, payload), in file order, without the two empty heads that open the chains"""
    at = 20 + mrz[19]
    head, chunks = mrz[:at], []
    while True:
        cb, eof = mrz[at], mrz[at + 1]
        size_field = int.from_bytes(mrz[at + 2:at + 2 + cb], "little")
        at += 2 + cb
        initial_pos, blocks, end = at, [], at + 2 * (1 + 3 * cb)
        for s in range(2):
            pos = initial_pos + s * (1 + 3 * cb)
            first = True
            while True:
                ctype = mrz[pos]
                c_len, u_len, nxt = (int.from_bytes(mrz[pos + 1 + i * cb:pos + 1 + (i + 1) * cb], "little")
                                     for i in range(3))
                pay = pos + 1 + 3 * cb
                if first:
                    assert ctype == CTYPE_NONE and c_len == 0 and u_len == 0
                else:
                    blocks.append(dict(stream=s, ctype=ctype, c_len=c_len, u_len=u_len,
                                       payload=mrz[pay:pay + c_len], at=pos))
                    end = max(end, pay + c_len)
                first = False
                if not nxt:
                    break
                pos = initial_pos + nxt
        blocks.sort(key=lambda b: b["at"])
        chunks.append(dict(cb=cb, eof=eof, size_field=size_field, blocks=blocks))
        at = end
        if eof:
            break
    return dict(head=head, chunks=chunks, tail=mrz[at:])


def frame_mrz(parsed):
    out = bytearray(parsed["head"])
    for ch in parsed["chunks"]:
        cb = ch["cb"]
        out += bytes([cb, ch["eof"]]) + _le(ch["size_field"], cb)
        body, last_head = bytearray(), [0, 0]
        for s in range(2):
            last_head[s] = len(body) + 1 + 2 * cb
            body += bytes([CTYPE_NONE]) + _le(0, cb) * 3
        for b in ch["blocks"]:
            s = b["stream"]
            body[last_head[s]:last_head[s] + cb] = _le(len(body), cb)
            last_head[s] = len(body) + 1 + 2 * cb
            body += bytes([b["ctype"]]) + _le(len(b["payload"]), cb) + _le(b["u_len"], cb) + _le(0, cb) + b["payload"]
        out += body
    return bytes(out + parsed["tail"])


def streams_of(chunk, decode=None):
    """the two de-blocked streams of a parsed chunk; decode(payload, u_len) -> bytes for CTYPE_LZ4 blocks"""
    s = [bytearray(), bytearray()]
    for b in chunk["blocks"]:
        if b["ctype"] == CTYPE_LZ4:
            data = decode(b["payload"], b["u_len"])
            assert data is not None and len(data) == b["u_len"]
        else:
            assert b["ctype"] == CTYPE_NONE and b["c_len"] == b["u_len"]
            data = b["payload"]
        s[b["stream"]] += data
    return bytes(s[0]), bytes(s[1])


def reframe(mrz, oracle, block_size=None, choose=None):
    """A -n archive with the same streams: every stream re-cut into blocks of block_size bytes (None: as they are), the
    blocks that choose(index in the chunk, block bytes) picks (default: all of at least 64 bytes) rewritten as CTYPE_LZ4
    with the payload Oracle.lz4_compress gives them -- expanding ones too, as the reference writes them -- and the
    `next` fields re-linked."""
    if choose is None:
        choose = lambda i, data: len(data) >= 64  # noqa: E731
    parsed = parse_mrz(mrz)
    for ch in parsed["chunks"]:
        if block_size:
            cut = []
            for s, data in enumerate(streams_of(ch)):
                pieces = [data[i:i + block_size] for i in range(0, len(data), block_size)] or [b""]
                cut += [dict(stream=s, payload=p) for p in pieces]
        else:
            cut = [dict(stream=b["stream"], payload=b["payload"]) for b in ch["blocks"]]
            assert all(b["ctype"] == CTYPE_NONE for b in ch["blocks"])
        for i, b in enumerate(cut):
            data = b["payload"]
            b["u_len"], b["ctype"] = len(data), CTYPE_NONE
            if choose(i, data):
                n, comp = oracle.lz4_compress(data, len(data) + len(data) // 255 + 16)
                assert n > 0
                b["ctype"], b["payload"] = CTYPE_LZ4, comp
        ch["blocks"] = cut
    return frame_mrz(parsed)
