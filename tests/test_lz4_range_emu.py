"""Range decode over LZ4 archives on the wave64 emulator: the Python reference of the prefix contract pinned to liblz4's
recorded verdicts (no kernel involved), then mrz_lz4_decompress_prefix_batch against it (tests/_lz4_prefix.py) and
mrz_runzip_buffer_range_ex over re-framed archives with exact accounting (tests/_lz4_range_checks.py)."""
import pytest

import modern_rzip_amd as m
from tests import _lz4_blocks as B
from tests import _lz4_checks as C
from tests import _lz4_prefix as P
from tests import _lz4_range_checks as R

EMU = True


@pytest.fixture(scope="module")
def lib(emu_lib):
    return emu_lib


@pytest.fixture(scope="module")
def ctx(lib):
    with m.RzipContext(lib=lib) as c:
        yield c


# ---- the yardstick itself (CPU only) ----------------------------------------------------------------------------------

def test_ref_prefix_is_liblz4_at_full_length():
    """want == u_len: verdicts and digests of tests/golden/lz4_blocks.json for the 148 hand-built, 315 malformed and 2000
    fuzzed blocks (offset 0 rejected, as flagged there), and equality with _lz4_blocks.ref_decode"""
    fx = C.fixture()
    hand, mal, muts = B.handmade_cases(), B.malformed_cases(), B.fuzz_mutations()
    assert (len(hand), len(mal), len(muts)) == (148, 315, 2000)
    outs = [P.ref_prefix(blk, u, u) for _, blk, u in hand]
    assert all(o is not None for o in outs) and fx["handmade"]["accept"] == "1" * 148
    assert B.group_digest([True] * 148, outs) == fx["handmade"]["digest"]
    assert outs == [B.ref_decode(blk, u) for _, blk, u in hand]
    assert fx["malformed"]["accept"] == "0" * 315
    assert all(P.ref_prefix(blk, u, u) is None and B.ref_decode(blk, u) is None for _, blk, u in mal)
    u = B.fuzz_block()[1]
    outs = [P.ref_prefix(blk, u, u) for blk in muts]
    assert outs == [B.ref_decode(blk, u) for blk in muts]
    verdicts = [o is not None for o in outs]
    assert verdicts == [c == "1" for c in fx["fuzz"]["accept"]]
    assert all(not verdicts[i] for i in fx["fuzz"]["offset0"])
    for i in range(0, 2000, B.FUZZ_GROUP):
        got = B.group_digest(verdicts[i:i + B.FUZZ_GROUP], [o or b"" for o in outs[i:i + B.FUZZ_GROUP]])
        assert got == fx["fuzz"]["groups"][i // B.FUZZ_GROUP]


def test_ref_prefix_cuts_and_is_monotone():
    """on every tested want: an accepted prefix of a block liblz4 accepts is the full decode's; acceptance at one want
    implies acceptance at every smaller one with prefix-equal bytes; some rejected blocks have accepted prefixes"""
    seen_partial = 0
    for cases in P.groups().values():
        for name, blk, u in cases:
            full, longer = B.ref_decode(blk, u), None
            for w in reversed(P.wants_of(blk, u)):
                r = P.ref_prefix(blk, u, w)
                assert r is None or len(r) == w
                if longer is not None:
                    assert r is not None and longer.startswith(r), (name, w)
                if r is not None:
                    longer = r
                    assert full is None or r == full[:w], (name, w)
                    seen_partial += full is None and w > 0
    assert seen_partial > 100


def test_wants_cover_the_listed_cuts():
    """the hand-built set holds the shapes the contract names, and wants_of() cuts them there"""
    cases = {name: (blk, u) for name, blk, u in P.groups()["handmade"]}
    for off in (1, 2, 3, 7, 63, 64, 65):  # periodic: inside and beyond the first period of the match
        blk, u = cases[f"off{off}_len1000"]
        at, lit, ml = P.layout(blk)[0]
        ws = P.wants_of(blk, u)
        assert ml == 1000 and at + lit + 1 in ws and any(w > at + lit + off for w in ws if w < at + lit + ml)
    blk, u = cases["off8_len18"]  # the shortcut, taken: cut inside its literals and inside its match
    at, lit, ml = P.layout(blk)[0]
    assert lit < 15 and 1 < len(blk) - 16 and u >= 32 and {lit // 2, lit + ml // 2} <= set(P.wants_of(blk, u))
    blk, u = cases["off65535_len70000"]  # 256 length bytes of 255 in front of the literals, cut inside the run
    assert blk[0] >> 4 == 15 and blk[1:257] == b"\xff" * 256 and 65535 // 2 in P.wants_of(blk, u)
    assert all({u - 1, u - 5, u - 12} <= set(P.wants_of(blk, u)) for blk, u in cases.values() if u >= 12)


# ---- the prefix kernel ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("group", P.GROUPS)
def test_prefix(ctx, group, where):
    P.check_prefix(ctx, EMU, where, group)


def test_prefix_arguments(ctx):
    P.check_prefix_args(ctx)


def test_abi_unchanged(lib):
    assert lib.mrz_abi_version() == 4
    assert hasattr(lib, "mrz_lz4_decompress_prefix_batch") and hasattr(lib, "mrz_runzip_buffer_range_ex")


# ---- archives ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("framing", R.FRAMINGS)
@pytest.mark.parametrize("name", R.ARCHIVES)
def test_archive_ranges(lib, ctx, oracle, name, framing):
    R.check_archive(lib, ctx, oracle, EMU, name, framing)


def test_one_byte_and_outside_chunks(lib, ctx, oracle):
    R.check_one_byte(lib, ctx, oracle)


def test_refusals(lib, oracle):
    R.check_refusals(lib, oracle)
