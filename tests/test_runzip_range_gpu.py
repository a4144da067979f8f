"""mrz_runzip_range / mrz_runzip_origins / mrz_runzip_buffer_range on the MI355X: the CPU tier's ranges through the real
library, deep match chains, more bytes than the device holds threads, device-resident streams and output at odd
addresses, calls mixed with whole decodes on one context and two contexts at once.  Every comparison is exact; what is
expected comes from tests/_range_ref.py, which tests/test_runzip_range_emu.py checks without any kernel."""
import threading

import numpy as np
import pytest

import modern_rzip_amd as m
from tests import _range_ref as RR
from tests import _records as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    with m.RzipContext(level=7, max_chunk=64, lib=gpu_lib) as c:
        yield c


def on_device(data, offset=0):
    """the bytes as a slice of a cuda tensor that begins `offset` bytes into its allocation"""
    import torch
    t = torch.zeros(offset + len(data) + 16, dtype=torch.uint8, device="cuda")
    t[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[offset:offset + len(data)]


def check_resident(ctx, c, s0, s1, first, count, want_stats, what):
    """device-resident streams: the bytes come back to the host, the origins stay on the device"""
    import torch
    got, info = ctx.runzip_range(s0, s1, c["cb"], first, count)
    if got != c["out"][first:first + count]:
        raise AssertionError(f"{what}: {R.first_difference(got, c['out'][first:first + count], None)}")
    assert info["chunk_len"] == len(c["out"]), (what, info)
    org = torch.full((count + 2,), -7, dtype=torch.int64, device="cuda")
    _, info2 = ctx.runzip_origins(s0, len(c["s1"]), c["cb"], first, count, out=org[1:1 + count] if count else None)
    torch.cuda.synchronize()
    org = org.cpu().numpy()
    assert org[0] == -7 and org[-1] == -7, what
    if want_stats is not None:
        assert np.array_equal(org[1:1 + count], want_stats[0]), what
        for i in (info, info2):
            assert (i["total_hops"], i["max_hops"]) == tuple(want_stats[1:]), (what, i, want_stats[1:])
    else:
        s1h = np.frombuffer(c["s1"], dtype=np.uint8)
        assert bytes(s1h[org[1:1 + count]]) == c["out"][first:first + count], what


@pytest.mark.parametrize("name", ["short_cb3", "tiles8k", "overlap8k"])
def test_cpu_tier_ranges(ctx, name):
    """the whole output, [0, 1), the last byte, count == 0, record boundaries, the wrap of replicated matches, 100 random
    ranges: from host streams (origins on the device, gathered on the host) and from device-resident ones"""
    c = R.case(name)
    s0, s1 = on_device(c["s0"]), on_device(c["s1"])
    for first, count in RR.case_ranges(name):
        RR.check_range(ctx, name, first, count)
        check_resident(ctx, c, s0, s1, first, count, RR.expect(name, first, count), (name, first, count))


@pytest.mark.parametrize("name", ["chain_prev", "chain_far", "chain_window", "chain_intile"])
def test_chain_tails(ctx, name):
    """the last 4096 bytes of 8 MiB of chained matches (chain_prev: up to 889 hops a byte): bytes, origins, statistics"""
    c = R.case(name)
    n = len(c["out"])
    RR.check_chain_range(ctx, name, n - RR.CHAIN_TAIL, RR.CHAIN_TAIL)
    check_resident(ctx, c, on_device(c["s0"]), on_device(c["s1"]), n - RR.CHAIN_TAIL, RR.CHAIN_TAIL,
                   RR.chain_expect(name, n - RR.CHAIN_TAIL, RR.CHAIN_TAIL), name)


def test_deep_chain_256k(ctx):
    """the last 256 KiB of chain_prev, several hundred hops a byte: bytes"""
    c = R.case("chain_prev")
    n = len(c["out"])
    RR.check_chain_range(ctx, "chain_prev", n - (256 << 10), 256 << 10, stats=False)


def test_more_bytes_than_threads(ctx):
    """the whole 8 MiB of chain_far: the grid is capped below that, so every lane makes several passes"""
    c = R.case("chain_far")
    n = len(c["out"])
    assert n >= 8 << 20
    RR.check_chain_range(ctx, "chain_far", 0, n, stats=False)
    got, info = ctx.runzip_range(on_device(c["s0"]), on_device(c["s1"]), c["cb"], 0, n)
    if got != c["out"]:
        raise AssertionError(R.first_difference(got, c["out"], None))
    assert info["chunk_len"] == n and info["max_hops"] >= 10


@pytest.mark.parametrize("name", ["tiles8k", "overlap8k"])
def test_device_resident_streams_and_output(ctx, name):
    """s0 and s1 are slices of cuda tensors at byte offsets 1 and 3, `out` a slice at offset 7 with 64 guard bytes of 0xA5
    on either side that stay as they are; counts of 1, 63, 64, 65 and 4097.  Then host output from device streams and
    device output from host streams."""
    import torch
    c = R.case(name)
    n = len(c["out"])
    s0, s1 = on_device(c["s0"], 1), on_device(c["s1"], 3)
    for count in (1, 63, 64, 65, 4097):
        for first in (0, n // 2 + 1, n - count):
            want = c["out"][first:first + count]
            stats = RR.expect(name, first, count)[1:]
            for streams in ((s0, s1), (c["s0"], c["s1"])):
                whole = torch.full((7 + 64 + count + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                _, info = ctx.runzip_range(streams[0], streams[1], c["cb"], first, count, out=whole[71:71 + count])
                torch.cuda.synchronize()
                host = whole.cpu().numpy().tobytes()
                assert host[71:71 + count] == want, (name, first, count)
                assert host[:71] == b"\xa5" * 71 and host[71 + count:] == b"\xa5" * 64, (name, first, count)
                assert (info["chunk_len"], info["total_hops"], info["max_hops"]) == (n,) + stats, (name, first, count, info)
            got, info = ctx.runzip_range(s0, s1, c["cb"], first, count)
            assert got == want and (info["total_hops"], info["max_hops"]) == stats, (name, first, count)


def test_one_context_many_calls(ctx):
    """range, whole decode, range, a 17-byte case, range: the calls share one scratch"""
    import zlib
    far, prev = R.case("chain_far"), R.case("chain_prev")
    n = len(far["out"])
    RR.check_chain_range(ctx, "chain_far", n - 4096, 4096)
    back, got, cc, cs = ctx.runzip_chunk(prev["s0"], prev["s1"], prev["cb"], len(prev["out"]))
    assert back == prev["out"] and cc == cs == zlib.crc32(prev["out"]) & 0xFFFFFFFF
    RR.check_chain_range(ctx, "chain_prev", len(prev["out"]) - 4096, 4096)
    R.check_case(ctx, "tiny17")
    RR.check_range(ctx, "tiny17", 0, 17)
    RR.check_range(ctx, "tiny17", 16, 1)
    RR.check_chain_range(ctx, "chain_far", n - 4096, 4096)


def test_two_contexts_at_once(gpu_lib):
    """two host threads, a context each: one resolves the tail of the previous-tile chain, the other of the far one"""
    names = ["chain_prev", "chain_far"]
    for name in names:                     # what is expected, before the threads start
        RR.chain_expect(name, len(R.case(name)["out"]) - 4096, 4096)
    ctxs = [m.RzipContext(level=7, max_chunk=64, lib=gpu_lib) for _ in names]
    failed = [None] * len(names)

    def work(i):
        try:
            for _ in range(3):
                RR.check_chain_range(ctxs[i], names[i], len(R.case(names[i])["out"]) - 4096, 4096)
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            failed[i] = e

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(names))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in ctxs:
        c.close()
    for e in failed:
        if e is not None:
            raise e


def test_archive_ranges(gpu_lib, oracle):
    """the four-chunk archive whose streams the oracle cut into blocks of 8192 bytes, through mrz_runzip_buffer_range"""
    arch, data, seams = RR.archive(oracle)
    blocks = RR.archive_blocks(arch)
    assert len(blocks) == 4 and len(blocks[1][2]) >= 3
    org, _ = RR.table("tiles8k")
    x = int(np.nonzero((org[1:] == 8192) & (org[:-1] == 8191))[0][0]) + 1
    for first, count in RR.archive_ranges(len(data), seams, seams[0] + x):
        got, file_len = m.runzip_buffer_range(arch, first, count, lib=gpu_lib)
        assert file_len == len(data)
        if got != data[first:first + count]:
            raise AssertionError(f"[{first}, +{count}): {R.first_difference(got, data[first:first + count], None)}")
    with pytest.raises(m.MrzError) as e:
        m.runzip_buffer_range(arch, len(data) - 1, 2, lib=gpu_lib)
    assert e.value.rc == R.MRZ_E_ARG and e.value.file_len == len(data)
