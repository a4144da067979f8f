"""mrz_runzip_chunk on the MI355X against hand-built record streams (tests/_records.py).  The cases of the CPU tier go
through the real library, and then the shapes that only concurrent workgroups can get wrong: dependence chains over about
1024 decode tiles of 8 KiB -- more tiles than the grid has workgroups -- that pin the per-tile done flags, prefix_done,
the 64-tile window of tiles already seen and the ordering of stores inside a tile.  Every comparison is bit-exact, and a
mismatch is reported by its first offset and decode tile."""
import json
import os
import threading
import zlib

import pytest

import modern_rzip_amd as m
from tests import _records as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runzip_records.json")
T = 8192


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    with m.RzipContext(level=7, max_chunk=64, lib=gpu_lib) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def chain(name, golden):
    """a dependence-chain case, checked to be the stream the CPU tier has verified (three readings of the format agree
    there on exactly these bytes)"""
    c = R.case(name)
    assert R.fingerprint(name) == golden[name], name
    return c


def decode_exact(ctx, c, what):
    back, n, cc, cs = ctx.runzip_chunk(c["s0"], c["s1"], c["cb"], len(c["out"]))
    assert n == len(c["out"]), (what, n)
    if back != c["out"]:
        raise AssertionError(f"{what}: {R.first_difference(back, c['out'], R.expected_tshift(c['records']))}")
    assert cc == cs == (zlib.crc32(c["out"]) & 0xFFFFFFFF), (what, cc, cs)


# ---- the CPU tier's cases on the device ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", [f"short_cb{cb}" for cb in range(1, 9)] + list(R.TILE_MIXES) + ["overlap128k", "overlap8k"])
def test_cpu_tier_cases(ctx, name):
    R.check_case(ctx, name)


def test_refused_records(ctx):
    for name, s0, s1, cb, verdict in R.invalid_cases():
        assert R.check_against_ref(ctx, s0, s1, cb, 64, name) == verdict, name


def test_verdicts_on_damaged_streams(ctx):
    """every fourth stream of the CPU tier's damaged set: the verdict and, where accepted, the bytes"""
    subset = R.damaged_set()[::4]
    assert len(subset) == 100
    seen = {R.check_against_ref(ctx, s0, s1, cb, cap, name) for name, s0, s1, cb, cap in subset}
    assert seen == {"ok", "corrupt", "cap"}


# ---- dependence chains --------------------------------------------------------------------------------------------

def tile_gaps(records):
    """for every match: how many tiles its first source byte lies behind its first byte; (gap histogram, matches)"""
    pos, _ = R.out_positions(records)
    gaps = {}
    for r, p in zip(records, pos):
        if len(r) == 3:
            g = p // T - (p - r[1]) // T
            gaps[g] = gaps.get(g, 0) + 1
    return gaps, sum(gaps.values())


def test_chain_inputs_have_the_shapes_they_claim(golden):
    """Conditions on the inputs, not on the kernel."""
    for name in R.CHAINS:
        c = chain(name, golden)
        assert R.expected_tshift(c["records"]) == 13 and len(c["out"]) >= 1024 * T, name
    recs = R.case("chain_prev")["records"]
    gaps, n = tile_gaps(recs)
    assert set(gaps) <= {0, 1, 2} and gaps[1] > 0.9 * n              # the tile before, a few bytes either side of its tail
    assert all(abs(r[1] - T) <= 4 for r in recs if len(r) == 3)
    pos, _ = R.out_positions(recs)
    per_tile = [0] * 1024
    for r, p in zip(recs, pos):
        per_tile[p // T] += r[0] if len(r) == 3 else 0
    assert min(per_tile[1:]) > T // 2                                 # every tile is mostly matches
    recs = R.case("chain_far")["records"]
    gaps, n = tile_gaps(recs)
    assert len(gaps) > 900 and sum(v for g, v in gaps.items() if g > 128) > n // 2
    pos, _ = R.out_positions(recs)
    assert sum(1 for r, p in zip(recs, pos) if len(r) == 3 and p - r[1] < T) >= 10   # tile 0 is among the sources
    gaps, n = tile_gaps(R.case("chain_window")["records"])
    assert set(gaps) == {1, 62, 63, 64, 65} and all(gaps[g] > n // 20 for g in (62, 63, 64, 65))
    recs = R.case("chain_intile")["records"]
    triples = sum(1 for a, b, c3 in zip(recs, recs[1:], recs[2:])
                  if len(a) == 1 and len(b) == 3 and len(c3) == 3 and b[:2] == (a[0], a[0]) and c3[:2] == (a[0], a[0]))
    assert triples > 20 * 1024                                        # many times per tile
    assert any(len(r) == 3 and r[0] > r[1] for r in recs)


@pytest.mark.parametrize("name", list(R.CHAINS))
def test_dependence_chains(ctx, golden, name):
    """prev: no tile can complete before the one before it.  far: most waits resolve through prefix_done.  window: the
    sources lie 62..65 tiles back, around the edge of the 64-tile window.  intile: stores and loads of one tile.
    Three runs on one context; the first mismatch stops the test."""
    c = chain(name, golden)
    for run in range(3):
        decode_exact(ctx, c, f"{name}, run {run}")


def test_one_context_many_calls(ctx, golden):
    """large, 17 bytes, large, large on one context: done flags or scratch left by an earlier call must not matter"""
    for k, name in enumerate(("chain_far", "tiny17", "chain_prev", "chain_far")):
        c = R.case(name) if name == "tiny17" else chain(name, golden)
        decode_exact(ctx, c, f"call {k}: {name}")


def test_two_contexts_at_once(gpu_lib, golden):
    """two host threads, a context each: one decodes the previous-tile chain, the other the far-history one"""
    cases = [chain("chain_prev", golden), chain("chain_far", golden)]
    ctxs = [m.RzipContext(level=7, max_chunk=64, lib=gpu_lib) for _ in cases]
    got = [None] * len(cases)

    def work(i):
        try:
            for _ in range(2):
                got[i] = ctxs[i].runzip_chunk(cases[i]["s0"], cases[i]["s1"], cases[i]["cb"], len(cases[i]["out"]))
        except Exception as e:  # noqa: BLE001 -- handed to the main thread
            got[i] = e

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(cases))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in ctxs:
        c.close()
    for i, c in enumerate(cases):
        assert not isinstance(got[i], Exception), got[i]
        back, n, cc, cs = got[i]
        assert n == len(c["out"])
        if back != c["out"]:
            raise AssertionError(f"context {i}: {R.first_difference(back, c['out'], 13)}")
        assert cc == cs == (zlib.crc32(c["out"]) & 0xFFFFFFFF)


# ---- device-resident streams and output ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiles8k", "overlap8k", "chain_window"])
def test_device_resident_streams_and_output(ctx, name):
    """s0, s1 and out are slices of cuda tensors at byte offsets 1, 3 and 7; 64 guard bytes of 0xA5 on either side of
    `out` stay as they are -- with out_cap exact, with room to spare, and with the output going to the host."""
    import torch
    c = R.case(name)
    n = len(c["out"])
    crc = zlib.crc32(c["out"]) & 0xFFFFFFFF

    def on_device(data, offset):
        t = torch.zeros(offset + len(data) + 16, dtype=torch.uint8, device="cuda")
        t[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        return t[offset:offset + len(data)]

    s0, s1 = on_device(c["s0"], 1), on_device(c["s1"], 3)
    for spare in (0, 1000):
        cap = n + spare
        whole = torch.full((7 + 64 + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = whole[7 + 64:7 + 64 + cap]
        _, got, cc, cs = ctx.runzip_chunk(s0, s1, c["cb"], cap, out=out)
        torch.cuda.synchronize()
        host = whole.cpu().numpy().tobytes()
        assert got == n and cc == cs == crc, (spare, got, cc, cs)
        if host[71:71 + n] != c["out"]:
            raise AssertionError(f"{name}, spare {spare}: {R.first_difference(host[71:71 + n], c['out'], 13)}")
        assert host[:71] == b"\xa5" * 71 and host[71 + cap:] == b"\xa5" * 64, (name, spare)
    back, got, cc, cs = ctx.runzip_chunk(s0, s1, c["cb"], n)  # device streams, host output
    assert got == n and back == c["out"] and cc == cs == crc
    whole = torch.full((7 + 64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")  # host streams, device output
    _, got, cc, cs = ctx.runzip_chunk(c["s0"], c["s1"], c["cb"], n, out=whole[71:71 + n])
    torch.cuda.synchronize()
    host = whole.cpu().numpy().tobytes()
    assert got == n and cc == cs == crc and host[71:71 + n] == c["out"]
    assert host[:71] == b"\xa5" * 71 and host[71 + n:] == b"\xa5" * 64
