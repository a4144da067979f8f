"""mrz_runzip_chunk on the wave64 emulator against hand-built record streams (tests/_records.py): the stream shapes that
the project's own encoder never writes -- short matches, every distance width, replicated matches, terminators on the
parse-tile seams, every decode-tile size -- and the verdicts on damaged streams.  Every comparison is bit-exact.

The generator is checked first: build()'s output, decode_ref() and the oracle's decoder are three separate readings of
the format, and tests/golden/runzip_records.json pins the streams themselves."""
import ctypes
import hashlib
import json
import os
import zlib

import pytest

import modern_rzip_amd as m
from tests import _records as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runzip_records.json")


@pytest.fixture(scope="module")
def ctx(emu_lib):
    with m.RzipContext(level=7, max_chunk=64, lib=emu_lib) as c:
        yield c


decode_case = R.check_case


def oracle_decode(oracle, cb, s0, s1, out_len):
    """(rc, bytes) of the oracle's decoder on one chunk framed with the distance width cb"""
    md5 = hashlib.md5(b"").digest()  # the verdict on the records comes before the hash is looked at
    return oracle.decompress(oracle.frame(out_len, [(1 << 8 * (cb - 1), s0, s1)], md5))


# ---- the generator itself: no kernel involved ---------------------------------------------------------------------

GROUPS = ("short", "term", "scan", "tiles", "overlap", "chain_prev", "chain_far", "chain_window", "chain_intile", "chunk",
          "tiny")


def test_golden_lists_every_case():
    with open(GOLDEN) as f:
        golden = json.load(f)["cases"]
    assert sorted(golden) == sorted(R.golden_names())
    assert all(any(n.startswith(g) for g in GROUPS) for n in R.case_names())


@pytest.mark.parametrize("group", GROUPS)
def test_generator_matches_golden_hashes(group):
    """A drifting generator would silently change what both tiers test."""
    with open(GOLDEN) as f:
        golden = json.load(f)["cases"]
    names = [n for n in R.golden_names() if n.startswith(group)]
    assert names
    for name in names:
        assert R.fingerprint(name) == golden[name], name


@pytest.mark.parametrize("group", GROUPS)
def test_three_readings_of_the_format_agree(oracle, group):
    """build() == decode_ref() == the oracle's decoder, wherever a stream's block lengths fit the cb-wide fields."""
    for name in (n for n in R.case_names() if n.startswith(group)):
        c = R.case(name)
        if c is None:
            continue
        cb, s0, s1, out = c["cb"], c["s0"], c["s1"], c["out"]
        assert s0[-7:-4] == b"\0\0\0" and int.from_bytes(s0[-4:], "big") == zlib.crc32(out) & 0xFFFFFFFF
        want = R.decode_ref(s0, s1, cb, len(out))
        assert want[0] == "ok" and want[1] == out and want[2] == zlib.crc32(out) & 0xFFFFFFFF, name
        if len(out) < 1 << 20:
            assert R.decode_ref(s0, s1, cb, len(out) - 1) == ("cap", len(out)), name
        if len(s0) + len(s1) + 64 < 1 << 8 * cb:
            arch = oracle.frame(len(out), [(1 << 8 * (cb - 1), s0, s1)], hashlib.md5(out).digest())
            rc, back = oracle.decompress(arch)
            assert rc == 0 and back == out, (name, rc)
        else:
            assert cb < 3, name  # at least every stream of three-byte fields and wider is cross-checked


def test_refused_records_three_ways(ctx, oracle):
    """Single bad records: decode_ref, the oracle (where the frame can carry the width) and the emulated kernel agree.
    The empty match is among them: the reference's MIN(len, offset) < 1 (src/runzip.c:175-176)."""
    seen_empty = 0
    for name, s0, s1, cb, verdict in R.invalid_cases():
        assert R.decode_ref(s0, s1, cb, 64)[0] == verdict, name
        assert R.check_against_ref(ctx, s0, s1, cb, 64, name) == verdict
        # the oracle's frame replays the records and wants whole streams: it takes every case but the cut ones
        if "cut" in name or "no_terminator" in name or "stream1" in name:
            continue
        rc, back = oracle_decode(oracle, cb, s0, s1, 7)
        if verdict == "corrupt":
            assert rc == -5, (name, rc)
            seen_empty += name.startswith("empty_match")
        else:
            assert rc == -6 and back == R.decode_ref(s0, s1, cb, 64)[1], (name, rc)  # the records pass, the zero CRC does not
    assert seen_empty >= 6


def test_short_stream_is_an_argument_error(ctx):
    """fewer than the 7 bytes of terminator and CRC: refused before anything is parsed"""
    for n in range(1, 7):
        rc, _, got, _, _ = R.run_lib(ctx, bytes(n), b"", 1, 64)
        assert rc == R.MRZ_E_ARG and got == -1


# ---- the kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cb", range(1, 9))
def test_every_distance_width(ctx, cb):
    """3000 short records; the stream itself must enter its parse tiles at every one of the 3 + cb offsets and hold the
    distances that show the byte order and the top byte of the field."""
    c = R.case(f"short_cb{cb}")
    recs = c["records"]
    assert R.entry_offsets(recs, cb) == set(range(3 + cb))
    dists = {r[1] for r in recs if len(r) == 3}
    assert {1, 2, 3} <= dists and set(R._special_dists(cb)) <= dists
    assert {r[0] for r in recs} >= set(R.SHORT_LENS) and {r[2] for r in recs if len(r) == 3} == set(R.HEADS)
    assert any(len(r) == 3 and r[0] > r[1] for r in recs) and any(len(r) == 3 and r[0] < r[1] for r in recs)
    pos, _ = R.out_positions(recs)
    if cb >= 2:  # the whole history (a one-byte field ends at 255, which is asked for above)
        assert any(len(r) == 3 and r[1] == p and p > 1000 for r, p in zip(recs, pos))
    decode_case(ctx, f"short_cb{cb}")


@pytest.mark.parametrize("seam", [R.PT, 2 * R.PT])
@pytest.mark.parametrize("cb", R.TERM_CBS)
def test_terminator_on_the_parse_tile_seams(ctx, cb, seam):
    """The terminator begins at every offset from 12 before to 12 after a parse-tile seam: it straddles the seam, leaves
    the CRC alone in the last tile, makes s0_len exactly 1024 and 1031."""
    lens = set()
    for d in range(-12, 13):
        name = f"term_cb{cb}_{seam + d}"
        c = R.case(name)
        if c is None:  # only a length that whole records cannot reach may be left out
            assert not any((seam + d - (3 + cb) * b) % 3 == 0 and seam + d - (3 + cb) * b >= 3
                           for b in range((seam + d) // (3 + cb) + 1)), name
            assert (3 + cb) % 3 == 0 and (seam + d) % 3 != 0, name
            continue
        assert R.record_starts(c["records"], cb)[-1] == seam + d and len(c["s0"]) == seam + d + 7
        assert any(len(r) == 3 for r in c["records"]) and any(len(r) == 1 for r in c["records"][1:])
        lens.add(len(c["s0"]))
        decode_case(ctx, name)
    if cb != 3:
        assert lens == set(range(seam - 5, seam + 20)) and {seam, seam + 7} <= lens
    else:
        assert lens == {n + 7 for n in range(seam - 12, seam + 13) if n % 3 == 0}


@pytest.mark.parametrize("name,tiles", [("scan256", 256), ("scan129", 129)])
def test_scan_with_several_tiles_per_thread(ctx, name, tiles):
    """More than 128 parse tiles: every thread of the scan composes a run of tiles.  256 tiles fill all runs; 129 leave
    half of the threads without one and the last run short."""
    c = R.case(name)
    assert (len(c["s0"]) + R.PT - 1) // R.PT == tiles and c["cb"] == 2
    assert R.entry_offsets(c["records"], 2) == set(range(5))
    decode_case(ctx, name)


def test_tile_mixes_select_all_five_sizes():
    """A condition on the inputs: by the documented rule (out_total / nrec * 32) the five mixes pick 8, 16, 32, 64 and
    128 KiB, each over at least three tiles, and hold the boundary shapes."""
    picked = {}
    for name, (tshift, *_) in R.TILE_MIXES.items():
        recs = R.case(name)["records"]
        assert R.expected_tshift(recs) == tshift, name
        picked[tshift] = f = R.shapes(recs)
        assert f["tiles"] >= 3, name
        assert f["starts_on"] >= 2 and f["ends_on"] >= 2 and f["ends_before"] >= 1 and f["ends_after"] >= 1, (name, f)
        assert f["prev_tile_tail"] >= 1, (name, f)
        if tshift <= 15:  # a record of up to 65535 bytes can fill a tile
            assert f["on_boundaries"] >= 1, (name, f)
    assert sorted(picked) == [13, 14, 15, 16, 17]
    for tshift in (13, 14):
        assert picked[tshift]["lit_whole_tiles"] >= 3 and picked[tshift]["match_whole_tiles"] >= 3


@pytest.mark.parametrize("name", list(R.TILE_MIXES))
def test_decode_tile_sizes(ctx, name):
    decode_case(ctx, name)


@pytest.mark.parametrize("name", ["overlap128k", "overlap8k"])
def test_replicated_matches_across_tiles(ctx, name):
    """65535-byte matches at distances 1, 2, 3, 15, 16, 17 and 997 that run across tile boundaries, and a match whose
    source is the last `dist` bytes of the tile before -- at 128 KiB tiles and, behind 2500 one-byte literals, at 8 KiB."""
    recs = R.case(name)["records"]
    assert [r[1] for r in recs if len(r) == 3 and r[0] == 0xFFFF] == list(R.OVERLAP_DISTS)
    f = R.shapes(recs)
    assert R.expected_tshift(recs) == (17 if name == "overlap128k" else 13)
    assert f["overlap_crossings"] >= (3 if name == "overlap128k" else 50) and f["prev_tile_tail"] >= 1
    decode_case(ctx, name)


def test_verdicts_on_damaged_streams(ctx):
    """400 seeded damaged streams, judged differentially: the same verdict class as decode_ref and, where accepted, the
    same bytes and the same stored CRC."""
    seen = {}
    for name, s0, s1, cb, cap in R.damaged_set():
        v = R.check_against_ref(ctx, s0, s1, cb, cap, name)
        seen[(name.split("_")[1], v)] = seen.get((name.split("_")[1], v), 0) + 1
    # the set is worth something only if every verdict occurs and damage is not always fatal
    assert {v for _, v in seen} == {"ok", "corrupt", "cap"}
    assert seen.get(("flip", "ok"), 0) >= 10 and seen.get(("flip", "corrupt"), 0) >= 10 and seen.get(("width", "ok"), 0) >= 5


def test_out_cap_too_small_reports_the_size(ctx):
    """MRZ_E_ARG with *out_len = the needed size (the Python wrapper drops the latter): straight through ctypes."""
    c = R.case("short_cb3")
    need = len(c["out"])
    for cap in (0, 1, need - 1):
        buf = ctypes.create_string_buffer(max(1, cap))
        got = ctypes.c_int64(-1)
        rc = ctx.lib.mrz_runzip_chunk(ctx.ctx, c["s0"], len(c["s0"]), c["s1"], len(c["s1"]), m.binding.MEM_HOST, 3, buf,
                                      m.binding.MEM_HOST, cap, ctypes.byref(got), None, None)
        assert rc == R.MRZ_E_ARG and got.value == need, (cap, rc, got.value)
    rc, out, n, cc, cs = R.run_lib(ctx, c["s0"], c["s1"], 3, need + 1000)  # room to spare changes nothing
    assert rc == 0 and n == need and out == c["out"] and cc == cs


def test_whole_archive_of_three_widths(emu_lib, oracle):
    """Three hand-made chunks with distance widths 3, 4 and 5 in one archive, through mrz_runzip_buffer."""
    chunks = [R.case(f"chunk_cb{cb}") for cb in (3, 4, 5)]
    data = b"".join(c["out"] for c in chunks)
    arch = oracle.frame(len(data), [(1 << 8 * (c["cb"] - 1), c["s0"], c["s1"]) for c in chunks], hashlib.md5(data).digest())
    assert [oracle.L.mrzo_chunk_bytes(1 << 8 * (c["cb"] - 1)) for c in chunks] == [3, 4, 5]  # what the frame derives
    assert arch[20 + arch[19]] == 3
    rc, back = oracle.decompress(arch)
    assert rc == 0 and back == data
    assert m.runzip_buffer(arch, lib=emu_lib) == data
