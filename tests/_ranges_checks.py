"""The checks of mrz_runzip_ranges / mrz_runzip_origins_multi (many ranges of a chunk after one parse), shared by the
emulator tier (test_runzip_ranges_emu.py) and the GPU tier (test_runzip_ranges_gpu.py).  The streams are the hand-built
ones of tests/_records.py.  What a list of ranges must give is the concatenation of what mrz_runzip_range /
mrz_runzip_origins give for each range in turn -- total_hops their sum, max_hops their maximum -- and, for the cases
that have a table, what tests/_range_ref.py says.  Every comparison is exact; the buffers carry guard entries behind the
packed output."""
import ctypes
import functools

import numpy as np
import torch

from modern_rzip_amd import binding
from tests import _range_ref as RR
from tests import _records as R

E_ARG = -1
# records shorter than a wave (lengths 1..257, distance width 3); matches with dist < len (1, 2, 3, 15, 16, 17, 997);
# matches that copy matches, 86 hops deep at the end
CASES = ("short_cb3", "overlap8k", "chain_window")
TABLED = ("short_cb3", "overlap8k")
GRID = 16 * 256   # flat indices one pass of the emulator's grid covers
SYMBOLS = ("mrz_runzip_ranges", "mrz_runzip_origins_multi")


def check_abi(lib):
    assert lib.mrz_abi_version() == 4
    assert all(hasattr(lib, s) for s in SYMBOLS)


def split(total, parts, first, step):
    """`parts` ranges whose counts sum to `total`, `step` apart from `first` on"""
    base, out = total // parts, []
    for k in range(parts):
        n = base + (total - base * parts if k == parts - 1 else 0)
        out.append((first + k * step, n))
    return out


@functools.lru_cache(maxsize=None)
def range_lists(name):
    c = R.case(name)
    pos, total = R.out_positions(c["records"])
    g = R.Rng(len(c["records"]) + 77)
    deep = total - 4096   # where the chain cases are deepest
    lists = {"single": [(deep + 100, 300)], "single_first_byte": [(0, 1)], "single_whole_tail": [(total - 700, 700)]}
    lists["one_byte_ranges"] = [(g.below(total), 1) for _ in range(40)]
    small = [(g.below(total - 5), g.between(0, 5)) for _ in range(70)]
    for k in (0, 1, 30, 31, 32, 68, 69):   # empty ranges at the front, in the middle and at the end
        small[k] = (small[k][0], 0)
    assert sum(n for _, n in small) > 64
    lists["seventy_small"] = small
    lists["descending"] = [(total - 100 * k - 90, 80) for k in range(1, 12)]
    lists["overlapping_and_identical"] = [(deep, 200), (deep + 100, 200), (deep, 200), (deep + 50, 1), (deep, 200)]
    k = len(pos) // 2
    lists["across_a_record_boundary"] = [(pos[k] - 3, 6), (pos[k + 1] - 1, 2), (pos[k - 1] - 70, 140)]
    for t in (63, 64, 65, 255, 256, 257):
        lists[f"total_{t}"] = split(t, 3, deep + 7, 500)
    lists["second_pass_of_the_grid"] = [(deep - 1000, 3000), (10, 1500), (deep, 700)]
    assert sum(n for _, n in lists["second_pass_of_the_grid"]) > GRID
    for rl in lists.values():
        assert all(0 <= a and a + n <= total for a, n in rl)
    return lists


_single = {}


def single(ctx, name, first, count):
    """mrz_runzip_range and mrz_runzip_origins of one range, host streams: computed once, shared, never changed"""
    key = (id(ctx.lib), name, first, count)
    if key not in _single:
        c = R.case(name)
        rc, got, n, total, top = RR.run_range(ctx, c["s0"], c["s1"], c["cb"], first, count)
        rco, org, no, total_o, top_o = RR.run_origins(ctx, c["s0"], len(c["s1"]), c["cb"], first, count)
        assert rc == rco == 0 and n == no == len(c["out"]) and (total, top) == (total_o, top_o)
        assert got == c["out"][first:first + count]
        org.setflags(write=False)
        _single[key] = (got, org, total, top)
    return _single[key]


def expected(ctx, name, ranges):
    parts = [single(ctx, name, a, n) for a, n in ranges]
    org = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64)
    total, top = sum(p[2] for p in parts), max([p[3] for p in parts] + [0])
    if name in TABLED:   # the independent reference says the same
        ref = [RR.expect(name, a, n) for a, n in ranges]
        assert np.array_equal(org, np.concatenate([r[0] for r in ref]))
        assert (total, top) == (sum(r[1] for r in ref), max(r[2] for r in ref))
    return b"".join(p[0] for p in parts), org, total, top


def _place(data, emu, device):
    """-> (pointer, keepalive) of `data` in host memory, or in device memory (on the emulator: the same memory)"""
    if not device:
        return ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), data
    t = torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8)
    if not emu:
        t = t.cuda()
    return ctypes.c_void_p(t.data_ptr()), t


def call(ctx, emu, name, ranges, where, out_where, origins, null_out=False, room=None):
    """one raw call with a guard-filled buffer (of `room` entries where the counts do not say) -> (rc, packed result,
    RangeInfo, guard intact)"""
    c = R.case(name)
    arr, n = binding._byte_ranges(ranges)
    total = sum(max(0, k) for _, k in ranges) if room is None else room
    item = 8 if origins else 1
    p0, k0 = _place(c["s0"], emu, where)
    p1, k1 = _place(c["s1"], emu, where)
    dev = "cuda" if out_where and not emu else "cpu"
    buf = torch.full(((total + 8) * item,), 0xA5, dtype=torch.uint8, device=dev)
    po = None if null_out else ctypes.c_void_p(buf.data_ptr())
    info = binding.RangeInfo(-1, -1, -1)
    if origins:
        rc = ctx.lib.mrz_runzip_origins_multi(ctx.ctx, p0, len(c["s0"]), len(c["s1"]), where, c["cb"], arr, n, po,
                                              out_where, ctypes.byref(info))
    else:
        rc = ctx.lib.mrz_runzip_ranges(ctx.ctx, p0, len(c["s0"]), p1, len(c["s1"]), where, c["cb"], arr, n, po, out_where,
                                       ctypes.byref(info))
    raw = buf.cpu().numpy().tobytes()
    res = raw[:total * item]
    if origins:
        res = np.frombuffer(res, dtype=np.int64)
    return rc, res, info, raw[total * item:] == b"\xa5" * (8 * item)


def check_lists(ctx, emu, name, where, out_where):
    n_out = len(R.case(name)["out"])
    for label, ranges in range_lists(name).items():
        ranges = list(ranges)
        what = (name, label, where, out_where)
        data, org, total, top = expected(ctx, name, ranges)
        rc, got, info, intact = call(ctx, emu, name, ranges, where, out_where, origins=False)
        assert rc == 0 and intact and info.chunk_len == n_out, (what, rc)
        if got != data:
            raise AssertionError(f"{what}: {R.first_difference(got, data, None)}")
        assert (info.total_hops, info.max_hops) == (total, top), (what, info.total_hops, info.max_hops, total, top)
        rc, got, info, intact = call(ctx, emu, name, ranges, where, out_where, origins=True)
        assert rc == 0 and intact and info.chunk_len == n_out, (what, rc)
        if not np.array_equal(got, org):
            k = int(np.nonzero(got != org)[0][0])
            raise AssertionError(f"{what}: origin of packed byte {k}: got {got[k]}, want {org[k]}")
        assert (info.total_hops, info.max_hops) == (total, top), what


def check_binding(ctx, name):
    ranges = list(range_lists(name)["seventy_small"])
    data, org, total, top = expected(ctx, name, ranges)
    c = R.case(name)
    got, info = ctx.runzip_ranges(c["s0"], c["s1"], c["cb"], ranges)
    assert got == data and info == dict(chunk_len=len(c["out"]), total_hops=total, max_hops=top)
    got, info = ctx.runzip_origins_multi(c["s0"], len(c["s1"]), c["cb"], ranges)
    assert np.array_equal(got, org) and info == dict(chunk_len=len(c["out"]), total_hops=total, max_hops=top)


def check_bad_ranges(ctx, emu, name):
    """one bad range at each position of a list of three: MRZ_E_ARG after the parse (chunk_len set), nothing written"""
    n_out = len(R.case(name)["out"])
    good = [(5, 10), (100, 20), (n_out - 7, 7)]
    for bad in ((-1, 2), (3, -1), (n_out - 5, 6), (n_out + 1, 0), (2 ** 62, 2 ** 62), (1, 2 ** 63 - 1)):
        for p in range(3):
            ranges = list(good)
            ranges[p] = bad
            for origins in (False, True):
                for where in (0, 1):
                    rc, got, info, _ = call(ctx, emu, name, ranges, where, where, origins, room=64)
                    raw = got.tobytes() if origins else got
                    assert rc == E_ARG and info.chunk_len == n_out, (bad, p, rc, info.chunk_len)
                    assert raw == b"\xa5" * len(raw), (bad, p)
    rc, _, info, _ = call(ctx, emu, name, good, 0, 0, False)
    assert rc == 0 and info.chunk_len == n_out
    assert call(ctx, emu, name, good, 0, 0, False, null_out=True)[0] == E_ARG   # bytes asked for, nowhere to put them


def check_empty(ctx, emu, name):
    """sum(count) == 0: MRZ_OK with out == NULL, chunk_len set, no hops; so is an empty list"""
    n_out = len(R.case(name)["out"])
    for ranges in ([(5, 0), (0, 0), (n_out, 0)], []):
        for origins in (False, True):
            for where in (0, 1):
                rc, _, info, intact = call(ctx, emu, name, ranges, where, where, origins, null_out=True)
                assert rc == 0 and intact and (info.chunk_len, info.total_hops, info.max_hops) == (n_out, 0, 0)
    c = R.case(name)
    assert ctx.lib.mrz_runzip_ranges(ctx.ctx, c["s0"], len(c["s0"]), c["s1"], len(c["s1"]), 0, c["cb"], None, 0, None, 0,
                                     None) == 0
    assert ctx.lib.mrz_runzip_ranges(ctx.ctx, c["s0"], len(c["s0"]), c["s1"], len(c["s1"]), 0, c["cb"], None, 1, None, 0,
                                     None) == E_ARG
    assert ctx.lib.mrz_runzip_ranges(ctx.ctx, c["s0"], len(c["s0"]), c["s1"], len(c["s1"]), 0, c["cb"], None, -1, None, 0,
                                     None) == E_ARG


def check_corrupt(ctx, emu):
    """a stream the single calls refuse is refused alike, before any range is looked at"""
    seen = 0
    for name, s0, s1, cb, verdict in R.invalid_cases():
        if verdict != "corrupt":
            continue
        arr, n = binding._byte_ranges([(0, 1), (-5, 3)])
        info = binding.RangeInfo(-1, -1, -1)
        buf = ctypes.create_string_buffer(16)
        rc = ctx.lib.mrz_runzip_ranges(ctx.ctx, s0, len(s0), s1 or None, len(s1), 0, cb, arr, n, buf, 0, ctypes.byref(info))
        assert rc == R.MRZ_E_CORRUPT and info.chunk_len == -1, (name, rc)
        seen += 1
    assert seen >= 3
