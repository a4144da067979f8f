"""Hand-built record streams for mrz_runzip_chunk: a generator, a byte-wise reference decoder and the named cases of
tests/test_runzip_records_emu.py / tests/test_runzip_records_gpu.py.  Plain Python, no GPU.

Stream 0 (include/mrzgpu.h, src/runzip.c:277-308): records {head:u8, len:u16le}, a match (head != 0) carries a
chunk_bytes-wide little-endian distance; a zero-length literal ends the stream and the CRC-32 of the output follows, most
significant byte first.  Stream 1 holds the literal bytes.

A record is a tuple: (len,) is a literal, (len, dist, head) a match.  Everything is a pure function of the seeds below
(an xorshift64* generator and _util.xorshift_noise); nothing depends on the interpreter's hash seed."""
import ctypes
import functools
import hashlib
import zlib

from tests import _util

PT = 1024            # stream-0 parse tile of the decoder
TSHIFT_MIN, TSHIFT_MAX = 13, 17
HEADS = (1, 0x80, 0xFF)
SHORT_LENS = (1, 1, 2, 3, 7, 30, 31, 32, 255, 256, 257)
MRZ_OK, MRZ_E_ARG, MRZ_E_CORRUPT = 0, -1, -7


class Rng:
    """xorshift64* -- the same numbers on every interpreter"""

    def __init__(self, seed):
        self.s = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & 0xFFFFFFFFFFFFFFFF or 1

    def next(self):
        s = self.s
        s ^= s >> 12
        s ^= (s << 25) & 0xFFFFFFFFFFFFFFFF
        s ^= s >> 27
        self.s = s
        return (s * 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF

    def below(self, n):
        return (self.next() >> 11) % n

    def between(self, lo, hi):
        return lo + self.below(hi - lo + 1)

    def pick(self, seq):
        return seq[self.below(len(seq))]


# ---- writing streams --------------------------------------------------------------------------------------------

def pack(records, cb):
    """the bytes of the records in stream 0, without terminator; nothing is validated (a distance wider than cb bytes
    loses its top)"""
    s0 = bytearray()
    for r in records:
        if len(r) == 1:
            s0 += bytes((0, r[0] & 0xFF, r[0] >> 8))
        else:
            ln, dist, head = r
            s0 += bytes((head, ln & 0xFF, ln >> 8)) + (dist & ((1 << 8 * cb) - 1)).to_bytes(cb, "little")
    return bytes(s0)


def terminator(out):
    return b"\0\0\0" + (zlib.crc32(out) & 0xFFFFFFFF).to_bytes(4, "big")


def build(records, cb, literal_bytes):
    """-> (s0, s1, out) of a VALID record list.  `out` restates unzip_literal / unzip_match byte for byte: a literal takes
    the next bytes of `literal_bytes`, a match the first min(len, dist) history bytes, repeated."""
    out = bytearray()
    taken = 0
    for r in records:
        if len(r) == 1:
            ln = r[0]
            assert 1 <= ln <= 0xFFFF and taken + ln <= len(literal_bytes), r
            out += literal_bytes[taken:taken + ln]
            taken += ln
        else:
            ln, dist, head = r
            assert 1 <= ln <= 0xFFFF and 1 <= dist <= len(out) and dist < 1 << 8 * cb and 1 <= head <= 255, (r, len(out))
            n = min(ln, dist)
            first = len(out) - dist
            if n >= 64 or ln <= n:
                pattern = bytes(out[first:first + n])
                out += (pattern * (ln // n + 1))[:ln]
            else:
                for k in range(ln):
                    out.append(out[first + k % n])
    out = bytes(out)
    return pack(records, cb) + terminator(out), bytes(literal_bytes[:taken]), out


def decode_ref(s0, s1, cb, cap):
    """The record loop of runzip_chunk with the rejection rules of include/mrzgpu.h, written on its own (the way the
    reference does it: the min(len, dist) history bytes are read once and written until len is used up).
    -> ("ok", out, crc_stored) | ("corrupt",) | ("cap", out_len).  A record is judged before the capacity is."""
    out = bytearray()
    total = 0          # output bytes so far; `out` stops growing once total > cap
    i = j = 0
    n0 = len(s0)
    while True:
        if i + 3 > n0:
            return ("corrupt",)      # a record header past the end of stream 0 / no terminator
        head, ln = s0[i], s0[i + 1] | s0[i + 2] << 8
        if head == 0 and ln == 0:
            if i + 7 > n0:
                return ("corrupt",)  # the stored CRC runs past the end
            stored = int.from_bytes(s0[i + 3:i + 7], "big")
            break
        if head == 0:
            if j + ln > len(s1):
                return ("corrupt",)  # more literal bytes than stream 1 holds
            if total <= cap:
                out += s1[j:j + ln]
            j += ln
            i += 3
        else:
            if i + 3 + cb > n0:
                return ("corrupt",)
            dist = int.from_bytes(s0[i + 3:i + 3 + cb], "little")
            if ln < 1 or dist < 1 or dist > total:
                return ("corrupt",)  # empty match, distance 0, distance beyond the history
            if total <= cap:
                n = min(ln, dist)
                buf = bytes(out[total - dist:total - dist + n])
                left = ln
                while left:
                    n = min(left, dist)
                    out += buf[:n]
                    left -= n
            i += 3 + cb
        total += ln
    if total > cap:
        return ("cap", total)
    return ("ok", bytes(out), stored)


def run_lib(ctx, s0, s1, cb, cap):
    """mrz_runzip_chunk through ctypes on host memory -> (rc, bytes, out_len, crc_calc, crc_stored); out_len is what the
    library wrote to *out_len (-1: nothing), also when it refuses."""
    buf = ctypes.create_string_buffer(max(1, cap))
    got = ctypes.c_int64(-1)
    cc, cs = ctypes.c_uint32(), ctypes.c_uint32()
    p1 = ctypes.cast(ctypes.c_char_p(s1), ctypes.c_void_p) if s1 else None
    rc = ctx.lib.mrz_runzip_chunk(ctx.ctx, ctypes.cast(ctypes.c_char_p(s0), ctypes.c_void_p), len(s0), p1, len(s1), 0, cb,
                                  buf, 0, cap, ctypes.byref(got), ctypes.byref(cc), ctypes.byref(cs))
    return rc, (buf.raw[:got.value] if rc == 0 else b""), got.value, cc.value, cs.value


def check_against_ref(ctx, s0, s1, cb, cap, what=""):
    """library and decode_ref give the same verdict class; where accepted the same bytes, length and stored CRC, and the
    computed CRC is zlib's; where the capacity is short MRZ_E_ARG with the needed size.  -> the verdict"""
    want = decode_ref(s0, s1, cb, cap)
    rc, got, n, cc, cs = run_lib(ctx, s0, s1, cb, cap)
    if want[0] == "corrupt":
        assert rc == MRZ_E_CORRUPT, (what, rc)
    elif want[0] == "cap":
        assert rc == MRZ_E_ARG and n == want[1], (what, rc, n, want[1])
    else:
        assert rc == MRZ_OK, (what, rc)
        assert n == len(want[1]), (what, n, len(want[1]))
        if got != want[1]:
            raise AssertionError(f"{what}: {first_difference(got, want[1], None)}")
        assert cs == want[2] and cc == (zlib.crc32(want[1]) & 0xFFFFFFFF), (what, cc, cs, want[2])
    return want[0]


def check_case(ctx, name):
    """the library on a named case from host memory: bytes, out_len and both CRCs, all exact"""
    c = case(name)
    rc, got, n, cc, cs = run_lib(ctx, c["s0"], c["s1"], c["cb"], len(c["out"]))
    assert rc == MRZ_OK, (name, rc)
    assert n == len(c["out"]), (name, n)
    if got != c["out"]:
        raise AssertionError(f"{name}: {first_difference(got, c['out'], expected_tshift(c['records']))}")
    assert cc == cs == (zlib.crc32(c["out"]) & 0xFFFFFFFF), (name, cc, cs)


def first_difference(got, want, tshift):
    n = min(len(got), len(want))
    step = 1 << 16
    for a in range(0, n, step):
        if got[a:a + step] != want[a:a + step]:
            k = next(a + i for i in range(min(step, n - a)) if got[a + i] != want[a + i])
            tile = "" if tshift is None else f" (decode tile {k >> tshift} of {1 << tshift} bytes, byte {k & ((1 << tshift) - 1)} of it)"
            return f"first difference at offset {k}{tile}: got {got[k]:#04x}, want {want[k]:#04x}"
    return f"lengths differ: got {len(got)}, want {len(want)}"


# ---- looking at streams -----------------------------------------------------------------------------------------

def record_starts(records, cb):
    """offset in stream 0 of every record and of the terminator"""
    at, starts = 0, []
    for r in records:
        starts.append(at)
        at += 3 if len(r) == 1 else 3 + cb
    starts.append(at)
    return starts


def entry_offsets(records, cb):
    """the set of offsets at which the parse tiles are entered (first record start of the tile, mod 1024)"""
    seen, tile = set(), 0
    for s in record_starts(records, cb):
        while s >= tile * PT:
            seen.add(s - tile * PT)
            tile += 1
    return seen


def out_positions(records):
    pos, at = [], 0
    for r in records:
        pos.append(at)
        at += r[0]
    return pos, at


def expected_tshift(records):
    """the documented rule: about 32 records per tile, out_total / nrec * 32 rounded up to 8 .. 128 KiB"""
    _, total = out_positions(records)
    target = total // max(1, len(records)) * 32
    t = TSHIFT_MIN
    while t < TSHIFT_MAX and (1 << t) < target:
        t += 1
    return t


def shapes(records):
    """which of the shapes the decode-tile tests ask for a record list holds, at its own tile size"""
    T = 1 << expected_tshift(records)
    pos, total = out_positions(records)
    f = dict(tiles=(total + T - 1) // T, lit_whole_tiles=0, match_whole_tiles=0, on_boundaries=0, starts_on=0, ends_on=0,
             ends_before=0, ends_after=0, overlap_crossings=0, prev_tile_tail=0)
    for r, a in zip(records, pos):
        b = a + r[0]
        whole = max(0, b // T - (a + T - 1) // T)
        if r[0] == 0xFFFF and len(r) == 1:
            f["lit_whole_tiles"] = max(f["lit_whole_tiles"], whole)
        if r[0] == 0xFFFF and len(r) == 3:
            f["match_whole_tiles"] = max(f["match_whole_tiles"], whole)
        f["on_boundaries"] += a % T == 0 and b % T == 0
        f["starts_on"] += a % T == 0 and a > 0
        f["ends_on"] += b % T == 0
        f["ends_before"] += b % T == T - 1
        f["ends_after"] += b % T == 1 and a < b - 1
        if len(r) == 3 and r[0] > r[1]:
            f["overlap_crossings"] += (b - 1) // T - a // T
            f["prev_tile_tail"] += a % T == 0 and a > 0
    return f


# ---- record mixes -----------------------------------------------------------------------------------------------

def _special_dists(cb):
    """distances that show the byte order and the top byte of a cb-wide field"""
    return {1: (255,), 2: (256, 65535), 3: (65536,)}.get(cb, (256, 65536))


def mix_short(cb, seed, nrec=3000, lens=SHORT_LENS, s0_bytes=None):
    """short records: a third literals; distances 1, 2, 3, the whole history, near, random, and the special ones.
    With s0_bytes records are added until stream 0 (terminator and CRC included) is exactly that long, if it can be."""
    g = Rng(seed)
    recs = [(g.pick(lens) + 3,)]
    hist = recs[0][0]
    dmax = (1 << 8 * cb) - 1
    size = 3
    forced = None  # the kinds of the last records when the stream has to land on s0_bytes
    while (len(recs) < nrec) if s0_bytes is None else (size + 7 < s0_bytes):
        ln = g.pick(lens)
        want_lit = g.below(3) == 0
        if s0_bytes is not None:
            left = s0_bytes - 7 - size
            if forced is None and left < 4 * (3 + cb):
                b = next(b for b in range(4) if left >= (3 + cb) * b and (left - (3 + cb) * b) % 3 == 0)
                forced = [False] * b + [True] * ((left - (3 + cb) * b) // 3)
            if forced is not None:
                want_lit = forced.pop()
        if want_lit:
            recs.append((ln,))
            size += 3
        else:
            kind = g.below(8)
            if kind == 0:
                d = 1
            elif kind == 1:
                d = 2
            elif kind == 2:
                d = 3
            elif kind == 3:
                d = hist
            elif kind == 4:
                d = g.between(1, 64)
            elif kind == 5:
                d = g.pick(_special_dists(cb))
            else:
                d = g.between(1, hist)
            d = max(1, min(d, hist, dmax))
            recs.append((ln, d, g.pick(HEADS)))
            size += 3 + cb
        hist += ln
    return recs


def mix_terminator(cb, term_at, seed):
    """records of 3 and 3 + cb bytes that put the terminator at stream-0 offset term_at, or None when
    3a + (3 + cb)b = term_at has no solution with a literal in front"""
    sols = [(a, b) for b in range(0, term_at // (3 + cb) + 1) for a in [(term_at - (3 + cb) * b) // 3]
            if a >= 1 and 3 * a + (3 + cb) * b == term_at]
    if not sols:
        return None
    a, b = sols[len(sols) // 2]
    g = Rng(seed)
    recs = [(g.between(1, 3),)]
    hist = recs[0][0]
    a -= 1
    while a or b:
        if b and (not a or g.below(a + b) < b):
            ln = g.between(1, 5)
            recs.append((ln, max(1, min(g.between(1, hist), (1 << 8 * cb) - 1)), g.pick(HEADS)))
            b -= 1
        else:
            ln = g.between(1, 3)
            recs.append((ln,))
            a -= 1
        hist += ln
    return recs


def mix_tiles(tshift, avg, nrec, marks, big, seed):
    """records for one decode-tile size: `nrec` of up to 2 * avg bytes and, at `marks` places, the shapes that sit on the
    tile boundaries: a record that ends on a boundary, one that begins there (and ends on the next, where a tile fits a
    record), one that ends a byte before a boundary, one that ends a byte after, and a plain and a replicated match whose
    source is the tail of the tile before; with `big` a 65535-byte literal and a 65535-byte match."""
    g = Rng(seed)
    T = 1 << tshift
    recs = [(min(0xFFFF, avg + 64),)]
    hist = recs[0][0]
    count = 0

    def add(ln, overlap=False):
        nonlocal hist, count
        assert 1 <= ln <= 0xFFFF
        count += 1
        if count % 3 == 0 and not overlap:
            recs.append((ln,))
        else:
            d = (1, g.between(1, 64), T, g.between(1, hist), g.between(1, hist))[g.below(5)]
            if overlap:
                d = g.between(1, 15)
            recs.append((ln, max(1, min(d, hist)), g.pick(HEADS)))
        hist += ln

    def reach(off):  # the next record ends `off` bytes behind a tile boundary (off <= 0)
        while True:
            to = T - hist % T + off
            if to <= 0:
                to += T
            if to <= 0xFFFF:
                return add(to)
            add(min(to - 0xFFFF, 0xFFFF))

    at = {(k + 1) * nrec // (marks + 1) for k in range(marks)}
    for k in range(nrec):
        add(g.between(1, 2 * avg))
        if k in at:
            reach(0)                    # ends on a boundary
            add(min(T, 0xFFFF))         # begins on it; a whole tile where one fits a record
            reach(-1)                   # ends one byte before a boundary
            add(2)                      # ends one byte after it
            reach(0)
            add(16, overlap=True)       # the source is the tail of the tile before: 16 >= distance, then replicated
            add(300, overlap=True)
        if big and k == nrec // 3:
            recs.append((0xFFFF,))
            hist += 0xFFFF
            recs.append((0xFFFF, g.between(0xFFFF, hist), g.pick(HEADS)))
            hist += 0xFFFF
    return recs


OVERLAP_DISTS = (1, 2, 3, 15, 16, 17, 997)


def mix_overlap(pad):
    """a literal, then a 65535-byte match at each of the distances; `pad` one-byte literals in front pull the decode tile
    down to 8 KiB, so that every match runs across many tiles.  Then a tile-aligned pair whose source is the tail of the
    tile before."""
    recs = [(1,)] * pad
    for d in OVERLAP_DISTS:
        recs += [(max(d, 5),), (0xFFFF, d, HEADS[d % 3])]
    T = 1 << expected_tshift(recs + [(1,)] * 8)

    def literals(n):
        while n > 0:
            recs.append((min(n, 0xFFFF),))
            n -= recs[-1][0]

    literals(T - out_positions(recs)[1] % T)
    recs.append((16, 16, 1))
    literals(T - 16)
    recs.append((300, 7, 0x80))
    assert expected_tshift(recs) == T.bit_length() - 1
    return recs


def mix_chain(kind, tiles=1024, seed=1):
    """8 KiB decode tiles, `tiles` of them: the dependence graphs that only concurrent workgroups can get wrong.
      prev    every tile is matches from the tail of the tile before (distance = tile size +- a few bytes)
      far     sources anywhere in the history, tile 0 included
      window  sources exactly 62, 63, 64, 65 tiles back, and 1 tile back
      intile  a literal, at once a match that copies it, at once a match that copies that match, many times a tile"""
    g = Rng(seed)
    T = 8192
    recs, hist = [], 0

    def lit(n):
        nonlocal hist
        recs.append((n,))
        hist += n

    def mat(n, d):
        nonlocal hist
        assert 1 <= d <= hist, (n, d, hist)
        recs.append((n, d, g.pick(HEADS)))
        hist += n

    if kind == "intile":
        while hist < tiles * T:
            n = g.between(8, 60)
            lit(n)
            mat(n, n)
            mat(n, n)
            mat(g.between(n + 1, 3 * n), g.between(1, n))      # the copy of the copy, replicated
        return recs
    for _ in range(T // 128):                                   # tile 0: literals only
        lit(128)
    back = (62, 63, 64, 65, 1)
    while hist < tiles * T:
        t = hist // T
        left = T - hist % T
        n = min(left, g.between(100, 250))
        if g.below(16) == 0:
            lit(min(n, 24))                                     # fresh bytes, so that tiles keep differing
            continue
        if kind == "prev":
            d = T + g.between(-4, 4)
        elif kind == "far":
            d = hist - g.below(hist - n + 1) if hist > n else hist
        else:
            k = back[g.below(5)]
            if k > t:
                k = 1
            # the source lies wholly in tile t - k: at the same offset as the record, or anywhere in that tile
            d = k * T if g.below(2) else hist - ((t - k) * T + g.below(T - n + 1))
        mat(n, max(1, min(d, hist)))
    return recs


# ---- named cases ------------------------------------------------------------------------------------------------

SHORT_SEEDS = {1: 12, 2: 12, 3: 13, 4: 14, 5: 15, 6: 16, 7: 11, 8: 18}  # seeds whose streams meet the conditions the tests assert
TERM_CBS = (1, 2, 3, 5, 8)
# name -> (tile shift, avg, records, marks, big); the averages that come out are about 170, 430, 850, 1600 and 25000
TILE_MIXES = {"tiles8k": (13, 100, 3000, 3, True), "tiles16k": (14, 330, 3000, 3, True), "tiles32k": (15, 600, 1000, 2, False),
              "tiles64k": (16, 1200, 600, 1, False), "tiles128k": (17, 30000, 20, 3, True)}
CHAINS = {"chain_prev": "prev", "chain_far": "far", "chain_window": "window", "chain_intile": "intile"}


def _case_records(name):
    """-> (cb, records)"""
    if name.startswith("short_cb"):
        cb = int(name[8:])
        return cb, mix_short(cb, SHORT_SEEDS[cb])
    if name.startswith("term_"):
        _, cb, at = name.split("_")
        return int(cb[2:]), mix_terminator(int(cb[2:]), int(at), seed=int(at) * 8 + int(cb[2:]))
    if name == "scan256":
        return 2, mix_short(2, 21, lens=(1, 1, 2, 3, 7, 30), s0_bytes=256 * PT)
    if name == "scan129":
        return 2, mix_short(2, 22, lens=(1, 1, 2, 3, 7, 30), s0_bytes=128 * PT + 1)
    if name in TILE_MIXES:
        tshift, avg, nrec, marks, big = TILE_MIXES[name]
        return 4, mix_tiles(tshift, avg, nrec, marks, big, seed=31 + tshift)
    if name == "overlap128k":
        return 3, mix_overlap(0)
    if name == "overlap8k":
        return 3, mix_overlap(2500)
    if name in CHAINS:
        return 4, mix_chain(CHAINS[name], seed=41 + len(name))
    if name.startswith("chunk_cb"):
        cb = int(name[8:])
        return cb, mix_short(cb, 50 + cb, nrec=400)
    if name == "tiny17":
        return 1, [(3,), (10, 3, 1), (4, 13, 0xFF)]
    raise KeyError(name)


def term_names():
    """terminator placements: every offset from 12 before to 12 after the seams at 1024 and 2048"""
    return [f"term_cb{cb}_{seam + d}" for cb in TERM_CBS for seam in (PT, 2 * PT) for d in range(-12, 13)]


def case_names():
    return ([f"short_cb{cb}" for cb in range(1, 9)] + term_names() + ["scan256", "scan129"] + list(TILE_MIXES)
            + ["overlap128k", "overlap8k"] + list(CHAINS) + ["chunk_cb3", "chunk_cb4", "chunk_cb5", "tiny17"])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(cb, records, s0, s1, out), or None for a terminator placement that whole records cannot reach.  Built
    once per process and shared; nobody changes it."""
    cb, recs = _case_records(name)
    if recs is None:
        return None
    need = sum(r[0] for r in recs if len(r) == 1)
    s0, s1, out = build(recs, cb, _util.xorshift_noise(need, seed=1000 + zlib.crc32(name.encode()) % 1000))
    return dict(cb=cb, records=recs, s0=s0, s1=s1, out=out)


def golden_names():
    """the entries of tests/golden/runzip_records.json: every case, the terminator placements of a width as one"""
    return [n for n in case_names() if not n.startswith("term_")] + [f"term_cb{cb}" for cb in TERM_CBS]


def fingerprint(name):
    """what tests/golden/runzip_records.json keeps of a case: parameters and hashes, no streams.  For term_cb<w>: the
    placements that whole records reach and the hashes of their streams' hashes, in order."""
    if name.startswith("term_"):
        group = [(n, case(n)) for n in term_names() if n.startswith(name + "_")]
        f = {"cb": int(name[7:]), "reached": [int(n.split("_")[2]) for n, c in group if c is not None]}
        for part in ("s0", "s1", "out"):
            f[part] = hashlib.sha256(b"".join(hashlib.sha256(c[part]).digest() for _, c in group if c is not None)).hexdigest()
        return f
    c = case(name)
    return {"cb": c["cb"], "records": len(c["records"]), "s0_len": len(c["s0"]), "s1_len": len(c["s1"]),
            "out_len": len(c["out"]), "s0": hashlib.sha256(c["s0"]).hexdigest(), "s1": hashlib.sha256(c["s1"]).hexdigest(),
            "out": hashlib.sha256(c["out"]).hexdigest()}


# ---- streams the decoder must refuse ----------------------------------------------------------------------------

def invalid_cases():
    """(name, s0, s1, cb, verdict class) of single bad records behind a three-byte literal, and their valid neighbours"""
    lit = b"abc"
    out = []

    def one(name, cb, recs, verdict, s1=lit, tail=None):
        s0 = pack(recs, cb) + (b"\0\0\0" + bytes(4) if tail is None else tail)
        out.append((name, s0, s1, cb, verdict))

    for cb in (1, 3, 8):
        one(f"distance0_cb{cb}", cb, [(3,), (4, 0, 1)], "corrupt")
        one(f"distance_history_plus_1_cb{cb}", cb, [(3,), (4, 4, 1)], "corrupt")
        one(f"distance_is_history_cb{cb}", cb, [(3,), (4, 3, 1)], "ok")
        one(f"empty_match_cb{cb}", cb, [(3,), (0, 1, 1)], "corrupt")
        one(f"empty_match_then_more_cb{cb}", cb, [(3,), (0, 2, 0xFF), (2, 1, 1)], "corrupt")
        one(f"literal_one_beyond_stream1_cb{cb}", cb, [(3,), (2, 1, 1), (1,)], "corrupt")
        one(f"literal_to_the_end_of_stream1_cb{cb}", cb, [(2,), (2, 1, 1), (1,)], "ok")
        one(f"no_terminator_cb{cb}", cb, [(3,), (4, 3, 1)], "corrupt", tail=b"")
        one(f"crc_cut_cb{cb}", cb, [(3,), (4, 3, 1)], "corrupt", tail=b"\0\0\0" + bytes(3))
        one(f"match_cut_cb{cb}", cb, [(3,), (4, 3, 1)], "corrupt", tail=bytes([1, 4, 0]) + bytes(cb - 1))
    one("distance_bit63_cb8", 8, [(3,), (4, (1 << 63) | 3, 1)], "corrupt")
    one("distance_bit63_only_cb8", 8, [(3,), (4, 1 << 63, 0x80)], "corrupt")
    one("distance_top_byte_cb2", 2, [(3,), (4, 0x0103, 1)], "corrupt")
    return out


def damaged_set(count=400, seed=7):
    """(name, s0, s1, cb, out_cap): seeded damage to small valid streams -- bit flips in stream 0, truncation of either
    stream, the wrong distance width, an output capacity that is too small"""
    g = Rng(seed)
    bases = []
    for k, cb in enumerate((1, 2, 3, 4, 8)):
        recs = mix_short(cb, 70 + k, nrec=60, lens=(1, 2, 3, 7, 30, 31, 255))
        need = sum(r[0] for r in recs if len(r) == 1)
        bases.append((cb,) + build(recs, cb, _util.xorshift_noise(need, seed=80 + k)))
    out = []
    for c in range(count):
        cb, s0, s1, data = bases[c % len(bases)]
        cap = 2 * len(data) + 100
        s0 = bytearray(s0)
        kind = ("flip", "cut0", "cut1", "width", "cap")[(c // len(bases)) % 5]
        if kind == "flip":
            for _ in range(g.between(1, 3)):
                s0[g.below(len(s0))] ^= 1 << g.below(8)
        elif kind == "cut0":
            s0 = s0[:g.between(7, len(s0) - 1)]
        elif kind == "cut1":
            s1 = s1[:g.below(len(s1))]
        elif kind == "width":
            cb = g.pick([w for w in range(1, 9) if w != cb])
        else:
            cap = g.below(len(data))
        out.append((f"{c}_{kind}_cb{cb}", bytes(s0), s1, cb, cap))
    return out
