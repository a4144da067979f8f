"""The checks of the ar-mrzip index (mrz_tlsh_batch, mrz_ar_order, mrz_ar_create / parse / verify), shared by the
emulator tier (test_ar_*_emu.py) and the GPU tier (test_ar_*_gpu.py).  Every comparison is exact.  Expectations: the
reference library's own strings (tests/golden/tlsh.json) for the digest; tests/_ar_ref.py, an independent restatement,
for the order, the collapse and the framing."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import modern_rzip_amd as m
from tests import _ar_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_CORRUPT, E_UNSUPPORTED = -1, -7, -8


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "tlsh.json")) as f:
        return json.load(f)


def on_device(data, emu):
    """(what the binding takes as device memory, keepalive); on the emulator device memory is host memory handed over
    as (address, length)"""
    t = torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8)
    if not emu:
        t = t.cuda()
    return (t.data_ptr(), len(data)), t


# ---- TLSH ------------------------------------------------------------------------------------------------------------

def check_ref_restatement():
    """tests/_ar_ref.tlsh gives the reference's strings (it is what ar_create's expectations are made with)"""
    g = fixture()
    for name, data in R.small_inputs().items():
        assert R.tlsh(data, g["lvalue_min_len"], None) == g["small"][name], name


def check_small(ctx, emu, segment_len, where):
    g, inp = fixture(), R.small_inputs()
    names = list(inp)
    if where == "host":
        msgs, keep = [inp[k] for k in names], None
    else:
        pairs = [on_device(inp[k], emu) for k in names]
        msgs, keep = [p[0] for p in pairs], [p[1] for p in pairs]
    got = ctx.tlsh_batch(msgs, segment_len=segment_len)
    bad = [k for k, s in zip(names, got) if s != g["small"][k]]
    assert not bad, (segment_len, bad[:8])
    assert sum(1 for s in got if s) == sum(1 for v in g["small"].values() if v) >= 60
    del keep


def check_thresholds(ctx, max_len):
    """the length code steps where the fixture says: the full string at the last length of a code and the first of the
    next (every code whose first length is above 50 and at most max_len)"""
    g = fixture()
    lens = sorted(int(k) for k in g["thresholds"] if int(k) <= max_len)
    assert len(lens) >= 40
    got = ctx.tlsh_batch([R.threshold_message(n) for n in lens])
    for n, s in zip(lens, got):
        assert s == g["thresholds"][str(n)] and len(s) == 138, n
    # the code itself: byte 3 of the digest, nibbles swapped
    mins = g["lvalue_min_len"]
    for n, s in zip(lens, got):
        code = int(s[7] + s[6], 16)
        assert mins[code] <= n and (code == 169 or n < mins[code + 1]), n


def check_length_code(lib):
    """the host function at every threshold, including those no test message reaches"""
    mins = fixture()["lvalue_min_len"]
    assert len(mins) == 170 and mins[0] == 0
    for code, n in enumerate(mins):
        assert lib.mrz_tlsh_length_code(n) == code
        if n:
            assert lib.mrz_tlsh_length_code(n - 1) == code - 1
    assert lib.mrz_tlsh_length_code(4224281216) == 169
    assert lib.mrz_tlsh_length_code(4224281217) == E_UNSUPPORTED
    assert lib.mrz_tlsh_length_code(-1) == E_ARG


def check_big_member(ctx, emu):
    data = R.big_member()
    ref, keep = on_device(data, emu)
    assert ctx.tlsh_batch([ref]) == [fixture()["big_member"]]
    assert ctx.tlsh_batch([ref], segment_len=1 << 20) == [fixture()["big_member"]]
    del keep


def check_mixed_batch(ctx, emu):
    batch = R.mixed_batch()
    pairs = [on_device(d, emu) for d in batch]
    got = ctx.tlsh_batch([p[0] for p in pairs])
    exp = fixture()["mixed_batch"]
    assert [i for i, (a, b) in enumerate(zip(got, exp)) if a != b] == []
    assert ctx.tlsh_batch(batch[:40]) == exp[:40]


def check_tlsh_args(ctx):
    # a length of 4 GiB is refused before the (invalid) pointer is followed, in host and in device memory
    for n in (1 << 32, 4224281217):
        with pytest.raises(m.MrzError) as e:
            ctx.tlsh_batch([(0x1000, n)])
        assert e.value.rc == E_UNSUPPORTED
    msg = R.make_input("noise", 600)
    for bad in (1, 63, (1 << 30) + 1, -64):
        with pytest.raises(m.MrzError) as e:
            ctx.tlsh_batch([msg], segment_len=bad)
        assert e.value.rc == E_ARG
    assert ctx.tlsh_batch([]) == []
    assert ctx.tlsh_batch([b"", b"abcd", msg], segment_len=1 << 30)[:2] == ["", ""]


# ---- order -----------------------------------------------------------------------------------------------------------

def hex_digests():
    return [v.encode()[:R.STORED] for _, v in sorted(fixture()["small"].items()) if v]


def handmade_orders():
    """(digests, expected order or None = only compared with _ar_ref)"""
    h, z = hex_digests(), R.ZERO
    a = b"A" * 137

    def near(k, fill=b"B"):
        """equal to `a` in all but the last k bytes"""
        return a[:137 - k] + fill * k

    return {
        "n0": ([], []), "n1": ([h[0]], [0]), "n2": ([h[0], h[1]], [0, 1]), "n3": ([h[0], h[1], h[2]], None),
        # nothing in common with anything: the step swaps with position 0 and moves the head of the list
        "hex_zero_zero": ([h[0], z, z], [2, 0, 1]), "zero_hex_hex": ([z, h[0], h[1]], None),
        "all_zero": ([z, z, z, z], [0, 1, 2, 3]),
        # equal scores: the first one wins
        # (every candidate ends in a letter of its own, so two candidates share their common prefix of "A" only)
        "tie": ([a, near(87), near(87, b"C"), near(90, b"D")], [0, 1, 2, 3]),
        "tie_later_best": ([a, near(90), near(50, b"C"), near(50, b"D")], [0, 2, 3, 1]),
        # two candidates above 130: the earlier one wins though the later one scores higher
        "two_above_130": ([a, near(100), near(6, b"C"), near(0), near(3, b"D")], [0, 2, 3, 4, 1]),
        "exactly_130_is_not_above": ([a, near(7), near(6, b"C")], [0, 2, 1]),
    }


def check_order_handmade(ctx, name):
    digests, expect = handmade_orders()[name]
    ref = R.order(digests)
    if expect is not None:
        assert ref == expect
    assert ctx.ar_order(digests) == ref


@functools.lru_cache(maxsize=None)
def many_digests(n=700):
    """digests that differ from one of three bases in a few positions: many scores above 130, many ties"""
    h = hex_digests()
    rng = np.random.default_rng(700)
    out = []
    for i in range(n):
        b = np.frombuffer(h[(i * 7) % 3], dtype=np.uint8).copy()
        for p in rng.integers(0, 137, size=int(rng.integers(0, 12))):
            b[p] = rng.integers(48, 58)
        out.append(b.tobytes() if i % 50 else R.ZERO)
    return tuple(out), tuple(R.order(out))


def check_order_many(ctx):
    digests, ref = many_digests()
    got = ctx.ar_order(list(digests))
    assert sorted(got) == list(range(len(digests)))
    assert got == list(ref)


# ---- archives --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def member_set():
    """(members, expected archive, expected records): exact duplicates next to each other and far apart, empty members
    and duplicate empty ones, members of 500 bytes or less, names of 0 and 300 bytes"""
    sizes = [0, 10, 600, 0, 5000, 4097, 500, 501, 700, 1281, 499, 2000]
    mem = [(b"dir/member%d" % i, 1700000000 + i, R.make_input(R.KINDS[i % 5], n, seed=i)) for i, n in enumerate(sizes)]
    mem.insert(5, (b"adjacent-duplicate", 5, mem[4][2]))
    mem.append((b"distant-duplicate", 2 ** 63 + 5, mem[2][2]))
    mem.append((b"", 0, R.make_input("text", 900, seed=3)))
    mem.append((b"n" * 300, 1, R.make_input("text", 900, seed=4)))
    mem.append((b"small-duplicate", 2, mem[1][2]))
    mins = fixture()["lvalue_min_len"]
    digests = [R.stored_digest(R.tlsh(d, mins, None), len(d)) for _, _, d in mem]
    exp, recs = R.create(mem, digests)
    return tuple(mem), exp, tuple(recs)


def check_create(ctx, emu, where, out_where):
    mem, exp, recs = member_set()
    keep = []
    if where == "device":
        pairs = [on_device(d, emu) for _, _, d in mem]
        keep.append(pairs)
        mem = [(n, t, p[0]) for (n, t, _), p in zip(mem, pairs)]
    if out_where == "host":
        got, info = ctx.ar_create(list(mem))
    else:
        buf = torch.full((len(exp) + 64,), 0xC5, dtype=torch.uint8, device="cpu" if emu else "cuda")
        n, info = ctx.ar_create(list(mem), out=(buf.data_ptr(), len(exp)) if emu else buf[:len(exp)])
        img = buf.cpu().numpy().tobytes()
        assert n == len(exp) and img[len(exp):] == b"\xc5" * 64
        got = img[:n]
    assert got == exp
    uniq = sum(r["size"] for i, r in enumerate(recs) if all(q["checksum"] != r["checksum"] for q in recs[:i]))
    assert info == {"unique_bytes": uniq, "duplicate_bytes": sum(r["size"] for r in recs) - uniq,
                    "members_hashed": sum(1 for r in recs if r["size"] > 500),
                    "metadata_size": sum(len(r["name"]) + 229 for r in recs)}
    assert info["duplicate_bytes"] > 5000


def check_roundtrip(ctx, emu):
    mem, exp, recs = member_set()
    got = m.ar_parse(exp, ctx.lib)
    assert [(r["name"], r["mtime"], r["size"], r["offset"], r["checksum"], r["digest"], r["data"]) for r in got] == \
           [(r["name"], r["mtime"], r["size"], r["offset"], r["checksum"], r["digest"], r["data"]) for r in recs]
    assert sorted((r["name"], r["data"]) for r in got) == sorted((n, d) for n, _, d in mem)
    assert ctx.ar_verify(exp) == (0, -1)
    ref, keep = on_device(exp, emu)
    assert ctx.ar_verify(ref) == (0, -1)
    assert m.ar_parse(ctx.ar_create([])[0], ctx.lib) == [] and ctx.ar_create([])[0] == b"ARZIP" + bytes(8)


def check_verify_names_the_member(ctx, emu):
    _, exp, recs = member_set()
    pay = len(exp) - max(r["offset"] + r["size"] for r in recs)
    victim = next(i for i, r in enumerate(recs) if r["name"] == b"dir/member2")
    sharing = [i for i, r in enumerate(recs) if r["checksum"] == recs[victim]["checksum"]]
    assert len(sharing) == 2
    bad = bytearray(exp)
    bad[pay + recs[victim]["offset"] + 17] ^= 0x20
    n_bad, first = ctx.ar_verify(bytes(bad))
    assert (n_bad, first) == (2, min(sharing))
    assert m.ar_parse(bytes(bad), ctx.lib)[first]["name"] in (b"dir/member2", b"distant-duplicate")
    ref, keep = on_device(bytes(bad), emu)
    assert ctx.ar_verify(ref) == (2, min(sharing))


def check_corrupt(ctx, emu):
    _, exp, recs = member_set()
    meta = int.from_bytes(exp[5:13], "big")
    cases = {"truncated metadata": exp[:13 + meta - 1], "magic": b"ARZIQ" + exp[5:], "short": exp[:12],
             "metadata not consumed exactly": exp[:5] + (meta - 1).to_bytes(8, "big") + exp[13:]}
    beyond = bytearray(exp)
    beyond[13 + 16:13 + 24] = (len(exp)).to_bytes(8, "big")  # the first record's offset
    cases["offset beyond the payload"] = bytes(beyond)
    huge = bytearray(exp)
    huge[13 + 8:13 + 16] = (2 ** 64 - 1).to_bytes(8, "big")  # its size
    cases["size wraps"] = bytes(huge)
    for what, ar in cases.items():
        with pytest.raises(m.MrzError) as e:
            m.ar_parse(ar, ctx.lib)
        assert e.value.rc == E_CORRUPT, what
        for arg in (ar, on_device(ar, emu)):
            with pytest.raises(m.MrzError) as e:
                ctx.ar_verify(arg if isinstance(arg, bytes) else arg[0])
            assert e.value.rc == E_CORRUPT, what


def check_create_args(ctx):
    with pytest.raises(m.MrzError) as e:
        ctx.ar_create([(b"big", 0, (0x1000, 1 << 32))])
    assert e.value.rc == E_UNSUPPORTED
    mem = [(b"a", 1, b"x" * 700)]
    small = bytearray(100)
    with pytest.raises(m.MrzError) as e:
        ctx.ar_create(mem, out=small)
    assert e.value.rc == E_ARG and small == bytearray(100)
