"""mrz_runzip_range / mrz_runzip_origins / mrz_runzip_buffer_range on the wave64 emulator: bytes [first, first + count)
of a chunk or an archive without decoding the rest.  The streams are the hand-built ones of tests/_records.py; what every
byte's origin and hop count must be comes from tests/_range_ref.py, which is checked first, without any kernel.  Every
comparison is exact."""
import hashlib

import numpy as np
import pytest

import modern_rzip_amd as m
from tests import _range_ref as RR
from tests import _records as R

CASES = [f"short_cb{cb}" for cb in range(1, 9)] + ["tiles8k", "tiles128k", "overlap8k", "overlap128k", "tiny17"]
CHAINS = ("chain_prev", "chain_far", "chain_window", "chain_intile")


@pytest.fixture(scope="module")
def ctx(emu_lib):
    with m.RzipContext(level=7, max_chunk=64, lib=emu_lib) as c:
        yield c


# ---- the reference itself: no kernel involved -------------------------------------------------------------------------

def test_reference_agrees_with_the_decoded_bytes():
    """s1[origin] == out[x] for every byte of every case; the byte-by-byte walk and the forward table agree on the
    first 200 bytes of sixty of the tested ranges and on 500 bytes spread over the whole output; the inputs hold the shapes the other tests lean on."""
    seen_wrap, seen_mixed = set(), 0
    for name in CASES:
        c = R.case(name)
        org, hops = RR.table(name)
        s1, out = np.frombuffer(c["s1"], dtype=np.uint8), np.frombuffer(c["out"], dtype=np.uint8)
        assert org.min() >= 0 and org.max() < len(s1) and np.array_equal(s1[org], out), name
        pos, total = R.out_positions(c["records"])
        for first, count in RR.case_ranges(name)[1:60]:
            count = min(count, 200)
            got = RR.resolve(c["records"], first, count)
            assert [o for o, _ in got] == org[first:first + count].tolist(), (name, first, count)
            assert [h for _, h in got] == hops[first:first + count].tolist(), (name, first, count)
        step = max(1, total // 500)
        got = [RR.resolve(c["records"], x, 1)[0] for x in range(0, total, step)]
        assert got == list(zip(org[::step].tolist(), hops[::step].tolist())), name
        for first, count in RR.case_ranges(name)[1:]:
            lits, mats = RR.spans(c["records"], first, count) if count else (0, 0)
            seen_mixed += lits >= 1 and mats >= 1 and lits + mats >= 3
        if name == "overlap8k":
            ranges = set(RR.case_ranges(name))
            for dist, first, count in RR.wrap_ranges(c["records"]):
                r = next(r for r, a in zip(c["records"], pos) if len(r) == 3 and a <= first < a + r[0])
                assert r[0] > r[1] == dist and first - pos[c["records"].index(r)] >= dist and count > 0
                if (first, count) in ranges:
                    seen_wrap.add(dist)
    assert seen_wrap >= set(R.OVERLAP_DISTS), seen_wrap
    assert seen_mixed >= 1
    for name in CHAINS:
        c = R.case(name)
        n = len(c["out"])
        for first, count in ((n - RR.CHAIN_TAIL, RR.CHAIN_TAIL), RR.CHAIN_MID):
            org, total, top = RR.chain_expect(name, first, count)
            assert bytes(np.frombuffer(c["s1"], dtype=np.uint8)[org]) == c["out"][first:first + count], name
    n = len(R.case("chain_prev")["out"])
    _, total, top = RR.chain_expect("chain_prev", n - 4096, 4096)
    assert top >= 500, (total, top)            # 889, sum 472,850
    assert RR.chain_expect("chain_window", len(R.case("chain_window")["out"]) - 4096, 4096)[2] >= 50   # 86
    assert RR.chain_expect("chain_far", len(R.case("chain_far")["out"]) - 4096, 4096)[2] >= 10         # 16


# ---- the kernel --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", [m.binding.MEM_HOST, m.binding.MEM_DEVICE])
@pytest.mark.parametrize("name", CASES)
def test_ranges_of_every_case(ctx, name, where):
    """the whole output, [0, 1), the last byte, count == 0, ranges on and around record boundaries, the wrap of a
    replicated match, 100 random ranges: bytes, origins, total_hops and max_hops.  where == host resolves origins and
    gathers on the host; where == device reads stream 1 in the kernel."""
    total = len(R.case(name)["out"])
    ranges = RR.case_ranges(name)
    assert ranges[0] == (0, total) and (0, 1) in ranges and (total - 1, 1) in ranges and len(ranges) >= 105
    assert any(n == 0 for _, n in ranges)
    for first, count in ranges:
        RR.check_range(ctx, name, first, count, where)


def test_sizing_call_takes_no_buffer(ctx):
    """count == 0: MRZ_OK, chunk_len set, out may be NULL -- at the start, in the middle and at the very end"""
    c = R.case("short_cb3")
    n = len(c["out"])
    info = RR.Info(-1, -1, -1)
    for first in (0, n // 2, n):
        for where in (0, 1):
            rc = ctx.lib.mrz_runzip_range(ctx.ctx, c["s0"], len(c["s0"]), c["s1"], len(c["s1"]), where, 3, first, 0, None,
                                          where, RR.ctypes.byref(info))
            assert rc == 0 and info.chunk_len == n and info.total_hops == 0 and info.max_hops == 0
            rc = ctx.lib.mrz_runzip_origins(ctx.ctx, c["s0"], len(c["s0"]), len(c["s1"]), where, 3, first, 0, None, where,
                                            None)
            assert rc == 0
    got, info = ctx.runzip_range(c["s0"], c["s1"], 3, 5, 0)
    assert got == b"" and info["chunk_len"] == n


@pytest.mark.parametrize("name", CHAINS)
def test_chains(ctx, name):
    """the last 4096 bytes (up to 889 hops a byte) and 257 bytes in the fourth tile: bytes, origins, hop statistics"""
    n = len(R.case(name)["out"])
    RR.check_chain_range(ctx, name, n - RR.CHAIN_TAIL, RR.CHAIN_TAIL, where=1)
    RR.check_chain_range(ctx, name, *RR.CHAIN_MID, where=0)


def range_verdicts(ctx, s0, s1, cb, cap, what):
    """the range calls judge a stream as decode_ref does; on an accepted stream a range one byte beyond the end is an
    argument error that still reports chunk_len -> the verdict class"""
    want = R.decode_ref(s0, s1, cb, cap)
    for first, count in ((0, 0), (0, 1)):
        for where in (0, 1):
            rc, got, n, _, _ = RR.run_range(ctx, s0, s1, cb, first, count, where)
            rco, org, no, _, _ = RR.run_origins(ctx, s0, len(s1), cb, first, count, where)
            if want[0] == "corrupt":
                assert rc == rco == R.MRZ_E_CORRUPT and n == no == -1, (what, first, count, rc, rco)
            elif want[0] == "cap":  # longer than decode_ref was told to follow: accepted, and the length is its
                assert n == no == want[1] and rc == rco == R.MRZ_OK, (what, rc, rco, n, no)
            else:
                out = want[1]
                assert n == no == len(out), (what, n, no)
                if count > len(out):
                    assert rc == rco == R.MRZ_E_ARG, (what, rc, rco)
                else:
                    assert rc == rco == R.MRZ_OK and got == out[:count], (what, rc, rco)
                    assert all(s1[o] == out[k] for k, o in enumerate(org.tolist())), what
    if want[0] == "ok":
        out = want[1]
        for first, count in ((0, len(out) + 1), (len(out), 1), (len(out) + 1, 0), (-1, 1), (0, -1)):
            rc, _, n, _, _ = RR.run_range(ctx, s0, s1, cb, first, count)
            rco, _, no, _, _ = RR.run_origins(ctx, s0, len(s1), cb, first, count)
            assert rc == rco == R.MRZ_E_ARG and n == no == len(out), (what, first, count, rc, rco, n)
        if out:
            rc, got, _, _, _ = RR.run_range(ctx, s0, s1, cb, 0, len(out))
            assert rc == R.MRZ_OK and got == out, what
    return want[0]


def test_refused_records(ctx):
    seen = set()
    for name, s0, s1, cb, verdict in R.invalid_cases():
        assert range_verdicts(ctx, s0, s1, cb, 64, name) == verdict, name
        seen.add(verdict)
    assert seen == {"ok", "corrupt"}


def test_verdicts_on_damaged_streams(ctx):
    """every fourth stream of the damaged set; a range call has no capacity, so the set's `cap` stays at the value of
    its 'flip' kind and the verdict is ok or corrupt"""
    whole = R.damaged_set()
    flip_cap = {int(name.split("_")[0]) % 5: cap for name, _, _, _, cap in whole if "_flip_" in name}   # per base stream
    seen = {}
    for name, s0, s1, cb, _ in whole[::4]:
        v = range_verdicts(ctx, s0, s1, cb, flip_cap[int(name.split("_")[0]) % 5], name)
        seen[v] = seen.get(v, 0) + 1
    assert {"ok", "corrupt"} <= set(seen) and min(seen["ok"], seen["corrupt"]) >= 10, seen


def test_range_calls_between_whole_decodes(ctx):
    """range, mrz_runzip_chunk, range, a 17-byte case, range on one context: they share the scratch"""
    RR.check_range(ctx, "tiles8k", 70000, 3000)
    R.check_case(ctx, "overlap8k")
    RR.check_range(ctx, "overlap8k", 100000, 3000, where=1)
    R.check_case(ctx, "tiny17")
    RR.check_range(ctx, "tiny17", 0, 17)
    RR.check_range(ctx, "tiles8k", 1, 5000, where=1)


# ---- the archive layer -------------------------------------------------------------------------------------------------

def block_seam_position(seams):
    """a file position inside tiles8k whose byte is the first of stream 1's second block, right behind the byte that is
    the last of its first block"""
    org, _ = RR.table("tiles8k")
    x = int(np.nonzero((org[1:] == 8192) & (org[:-1] == 8191))[0][0]) + 1
    return seams[0] + x


@pytest.mark.parametrize("ramsize", [24576, 60 << 30])
def test_archive_ranges(emu_lib, oracle, ramsize):
    """four chunks of distance widths 3, 4, 5 and 3; with ramsize 24576 the oracle cuts the streams into blocks of 8192
    bytes (tiles8k: 25 of stream 1, 3 of stream 0), with the default one block per stream.  Ranges inside each chunk,
    across each chunk seam, across a block seam of stream 1, the whole file, 50 random ones; a range beyond the file."""
    arch, data, seams = RR.archive(oracle, ramsize)
    rc, back = oracle.decompress(arch)
    assert rc == 0 and back == data
    blocks = RR.archive_blocks(arch)
    assert [b[0] for b in blocks] == [3, 4, 5, 3]
    if ramsize == 24576:
        assert len(blocks[1][2]) >= 3, blocks[1]
        assert blocks[1][1] == [8192, 8192, len(R.case("tiles8k")["s0"]) - 16384]
        assert blocks[1][2] == [8192] * 24 + [len(R.case("tiles8k")["s1"]) - 24 * 8192]
    else:
        assert all(len(b[1]) == len(b[2]) == 1 for b in blocks)
    assert m.runzip_buffer(arch, lib=emu_lib) == data
    for first, count in RR.archive_ranges(len(data), seams, block_seam_position(seams)):
        got, file_len = m.runzip_buffer_range(arch, first, count, lib=emu_lib)
        assert file_len == len(data)
        if got != data[first:first + count]:
            raise AssertionError(f"[{first}, +{count}): {R.first_difference(got, data[first:first + count], None)}")
    for first, count in ((0, len(data) + 1), (len(data), 1), (len(data) + 1, 0), (-1, 1), (5, -1)):
        with pytest.raises(m.MrzError) as e:
            m.runzip_buffer_range(arch, first, count, lib=emu_lib)
        assert e.value.rc == R.MRZ_E_ARG and e.value.file_len == len(data), (first, count)


def test_archive_without_a_size_and_refusals(emu_lib, oracle):
    """a header that carries no size: the chunks are walked to the end for file_len, and a range beyond it is an argument
    error.  The refusals are mrz_runzip_buffer's; the MD5 is not looked at."""
    arch, data, seams = RR.archive(oracle)
    nosize = bytearray(arch)
    nosize[6:14] = bytes(8)
    for first, count in ((0, len(data)), (seams[1] - 50, 100), (len(data) - 1, 1), (len(data), 0)):
        got, file_len = m.runzip_buffer_range(bytes(nosize), first, count, lib=emu_lib)
        assert file_len == len(data) and got == data[first:first + count]
    with pytest.raises(m.MrzError) as e:
        m.runzip_buffer_range(bytes(nosize), len(data) - 1, 2, lib=emu_lib)
    assert e.value.rc == R.MRZ_E_ARG and e.value.file_len == len(data)
    bad_md5 = bytearray(arch)
    bad_md5[-1] ^= 1
    with pytest.raises(m.MrzError):
        m.runzip_buffer(bytes(bad_md5), lib=emu_lib)
    assert m.runzip_buffer_range(bytes(bad_md5), 10, 20, lib=emu_lib)[0] == data[10:30]   # not checked: needs every byte
    for at, value, rc in ((0, ord("X"), R.MRZ_E_CORRUPT), (15, 1, -8), (14, 7, -8)):
        bad = bytearray(arch)
        bad[at] = value
        with pytest.raises(m.MrzError) as e:
            m.runzip_buffer_range(bytes(bad), 0, 10, lib=emu_lib)
        assert e.value.rc == rc, (at, e.value.rc)
    ctype = bytearray(arch)
    ctype[20 + arch[19] + 2 + 3] = 4   # the first block header of the first chunk: a back-end codec's block
    with pytest.raises(m.MrzError) as e:
        m.runzip_buffer_range(bytes(ctype), 0, 10, lib=emu_lib)
    assert e.value.rc == -8
    # a damaged record inside the range is refused; the same damage outside the range is not looked at on the device
    c = R.case("chunk_cb3")
    recs = list(c["records"])
    k = next(i for i, r in enumerate(recs) if len(r) == 3 and i > 10)
    recs[k] = (recs[k][0], 1 << 23, recs[k][2])   # a distance beyond the history, same lengths
    s0 = R.pack(recs, 3) + c["s0"][-7:]
    chunks = [(1 << 16, s0, c["s1"]), (1 << 16, c["s0"], c["s1"])]
    both = oracle.frame(2 * len(c["out"]), chunks, hashlib.md5(b"").digest())
    with pytest.raises(m.MrzError) as e:
        m.runzip_buffer_range(both, 0, 10, lib=emu_lib)
    assert e.value.rc == R.MRZ_E_CORRUPT
    assert m.runzip_buffer_range(both, len(c["out"]) + 5, 50, lib=emu_lib)[0] == c["out"][5:55]
