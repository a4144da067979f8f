"""Reference and checks for the prefix decode of LZ4 blocks (mrz_lz4_decompress_prefix_batch), shared by the emulator
tier and the GPU tier.

ref_prefix() is tests/_lz4_blocks.ref_decode with the early stop: the same walk and the same accept rules against the
block's real lengths; the copy (literal run or match) with which the output reaches `want` is validated as the full
decoder validates it before it copies -- a closing literal run must also end at u_len --, then cut.  A reject behind
that copy is not seen: that is the contract.  want == u_len is the full decoder; want == 0 < u_len is b"".
tests/test_lz4_range_emu.py pins it to liblz4's recorded verdicts before any kernel is judged by it."""
from tests import _lz4_blocks as B
from tests import _lz4_checks as C


def ref_prefix(src, u_len, want):
    """the first `want` bytes, or None for a reject"""
    assert 0 <= want <= u_len
    if want == 0 and u_len > 0:
        return b""
    cut = want if want < u_len else u_len + 1   # a whole block is walked to the end of its input
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
            if len(out) + lit >= cut:
                return bytes(out + src[ip:ip + cut - len(out)])
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
                if len(out) + lit >= cut:
                    if len(out) + lit != u_len:
                        return None
                    return bytes(out + src[ip:ip + cut - len(out)])
                out += src[ip:ip + lit]
                return bytes(out) if len(out) == u_len else None
            if len(out) + lit >= cut:
                return bytes(out + src[ip:ip + cut - len(out)])
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
        if offset == 0 or offset > len(out) or ml > u_len - len(out):
            return None
        if not unchecked and len(out) + ml > u_len - 5:
            return None
        ml = min(ml, cut - len(out))
        if offset >= ml:
            out += out[len(out) - offset:len(out) - offset + ml]
        else:
            period = bytes(out[len(out) - offset:])
            out += (period * (ml // offset + 1))[:ml]
        if len(out) >= cut:
            return bytes(out)


# ---- which prefixes -------------------------------------------------------------------------------------------------

def layout(src, limit=3):
    """A lenient walk over the first `limit` sequences, no rule applied: [(output position, literals, match length or
    None for a closing sequence)].  Ends where the block does."""
    res, ip, op, n = [], 0, 0, len(src)
    while len(res) < limit and ip < n:
        token = src[ip]
        ip += 1
        lit, ml = token >> 4, token & 15
        if lit == 15:
            while ip < n:
                lit += src[ip]
                ip += 1
                if src[ip - 1] != 255:
                    break
        ip += lit
        if ip + 2 > n:
            res.append((op, lit, None))
            break
        ip += 2
        if ml == 15:
            while ip < n:
                ml += src[ip]
                ip += 1
                if src[ip - 1] != 255:
                    break
        res.append((op, lit, ml + 4))
        op += lit + ml + 4
    return res


def wants_of(src, u_len):
    """0, 1, u_len, u_len - 1, u_len - 5, u_len - 12; one byte before, at and after every boundary of the first three
    sequences (start of the literals, start of the match, end of the match); the middle of the first literal run and of
    the first match -- those that lie in [0, u_len], ascending"""
    w = {0, 1, u_len, u_len - 1, u_len - 5, u_len - 12}
    seqs = layout(src)
    for at, lit, ml in seqs:
        for edge in (at, at + lit, at + lit + (ml or 0)):
            w |= {edge - 1, edge, edge + 1}
    first_lit = next(((at, lit) for at, lit, _ in seqs if lit > 1), None)
    if first_lit:
        w.add(first_lit[0] + first_lit[1] // 2)
    first_match = next(((at + lit, ml) for at, lit, ml in seqs if ml), None)
    if first_match:
        w.add(first_match[0] + first_match[1] // 2)
    return sorted(x for x in w if 0 <= x <= u_len)


def extra_cases():
    """Hand-built shapes the 148 do not hold: sequences in the middle of a block, away from both ends -- a shortcut
    sequence whose offset is below 8 (its match is checked after all), a sequence without literals, a literal run with a
    length byte followed by a long periodic match, and a shortcut sequence proper -- cut everywhere wants_of() says."""
    t = B._text
    last = t(40, 200)
    cases = []
    for name, seqs in (("mixed", [(t(20, 11), 3, 10), (b"", 16, 4), (t(5, 60), 2, 300), (t(14, 90), 8, 18)]),
                       ("shortcut_first", [(t(9, 400), 9, 18), (t(3, 420), 12, 6), (b"", 1, 40)])):
        blk, data = B.build_block(seqs, last), B.expand(seqs, last)
        assert B.ref_decode(blk, len(data)) == data
        cases.append((name, blk, len(data)))
    return cases


def groups():
    """name -> [(case name, block, u_len)]; the fuzzed blocks in the fixture's groups of 100"""
    u_len = B.fuzz_block()[1]
    muts = B.fuzz_mutations()
    res = {"handmade": B.handmade_cases() + extra_cases(), "malformed": B.malformed_cases()}
    for g in range(0, len(muts), B.FUZZ_GROUP):
        res[f"fuzz{g // B.FUZZ_GROUP:02d}"] = [(f"mut{i}", muts[i], u_len) for i in range(g, g + B.FUZZ_GROUP)]
    return res


GROUPS = ["handmade", "malformed"] + [f"fuzz{g:02d}" for g in range(2000 // B.FUZZ_GROUP)]


# ---- the kernel against it ------------------------------------------------------------------------------------------

def check_prefix(ctx, emu, where, group):
    """every block of the group at every want of wants_of(), in one batch: status and bytes against ref_prefix, 64
    pattern bytes behind every output intact (C.Slab keeps C.GAP = 64 canary bytes behind every slot), monotonicity"""
    assert C.GAP == 64
    cases = groups()[group]
    jobs = [(name, blk, u_len, w) for name, blk, u_len in cases for w in wants_of(blk, u_len)]
    src = C.Slab.of([j[1] for j in jobs], where, emu)
    dst = C.Slab([j[3] for j in jobs], where, emu)
    _, st = ctx.lz4_decompress_prefix_batch(src.refs, [j[2] for j in jobs], [j[3] for j in jobs], outs=dst.refs)
    data, intact = dst.read()
    assert intact, "bytes at or behind `want` were written"
    assert src.read()[0] == [j[1] for j in jobs]
    full = {}
    for (name, blk, u_len, w), s, d in zip(jobs, st, data):
        want = ref_prefix(blk, u_len, w)
        assert s == (0 if want is not None else B.E_CORRUPT), (name, w, s)
        if want is not None:
            assert d == want, (name, w)
            if name not in full:
                full[name] = B.ref_decode(blk, u_len)
            if full[name] is not None:  # liblz4 accepts the block: the prefix is the full decode's
                assert d == full[name][:w], (name, w)
    # a block accepted at `want` is accepted at every smaller tested want, with prefix-equal bytes
    longer = {}  # per block: the bytes of the next larger accepted want
    for (name, blk, u_len, w), s, d in reversed(list(zip(jobs, st, data))):
        if name in longer:
            assert s == 0 and longer[name].startswith(d), (name, w)
        if s == 0:
            longer[name] = d


def check_prefix_args(ctx):
    """want < 0, want > u_len, null buffers, a `where` that is neither host nor device; the Python layer refuses mixed
    memory"""
    import ctypes
    import modern_rzip_amd as m
    lib = ctx.lib
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    blk, u_len = B.fuzz_block()
    src = ctypes.create_string_buffer(blk, len(blk))
    out = ctypes.create_string_buffer(u_len)
    sp, op = ctypes.cast(src, vp), ctypes.cast(out, vp)
    status = (ctypes.c_int32 * 1)()

    def call(s=sp, c=len(blk), o=op, u=u_len, w=10, where=m.MEM_HOST, out_where=m.MEM_HOST, count=1, wants=True):
        return lib.mrz_lz4_decompress_prefix_batch(ctx.ctx, (vp * 1)(s), (i64 * 1)(c), count, where, (vp * 1)(o),
                                                   (i64 * 1)(u), (i64 * 1)(w) if wants else None, out_where, status)
    assert call() == 0 and status[0] == 0 and out.raw[:10] == B.ref_decode(blk, u_len)[:10]
    assert out.raw[10:] == bytes(u_len - 10)
    for kw in (dict(w=-1), dict(w=u_len + 1), dict(s=vp(None)), dict(o=vp(None)), dict(c=-1), dict(u=-1),
               dict(u=0x7E000001, w=1), dict(c=0x7E000001), dict(where=2), dict(out_where=2), dict(where=-1),
               dict(count=-1), dict(wants=False)):
        assert call(**kw) == -1, kw
    assert call(o=vp(None), w=0) == 0 and status[0] == 0   # nothing to write: no buffer needed
    assert call(count=0) == 0
    assert lib.mrz_lz4_decompress_prefix_batch(None, None, None, 1, 0, None, None, None, 0, None) == -1
    try:
        ctx.lz4_decompress_prefix_batch([blk, (ctypes.addressof(src), len(blk))], [u_len] * 2, [1, 1])
    except m.MrzError:
        pass
    else:
        raise AssertionError("mixed host / device blocks were taken")
