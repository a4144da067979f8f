"""The checks of mrz_ar_extract / mrz_ar_extract_mrz (members out of an ARZIP archive in memory, or straight out of the
.mrz that holds it), shared by the emulator tier (test_ar_extract_emu.py) and the GPU tier (test_ar_extract_gpu.py).
Archives: one written by mrz_ar_create over members of 0, 1, 500, 501 and a few thousand bytes with exact duplicates and
names of 0 and 300 bytes, and the one tests/_ar_ref.py frames (tests/_ar_checks.member_set).  What a selection must give
is the members' own bytes as mrz_ar_parse shows them, packed in selection order.  Every comparison is exact."""
import ctypes
import functools

import pytest
import torch

import modern_rzip_amd as m
from modern_rzip_amd import binding
from tests import _ar_checks as A
from tests import _ar_ref as R
from tests import _lz4_blocks as B
from tests import _lz4_checks as C

E_ARG, E_CORRUPT = -1, -7
SYMBOLS = ("mrz_ar_extract", "mrz_ar_extract_mrz", "mrz_copy_device_batch", "mrz_runzip_buffer_ranges")
_cache = {}


def check_abi(lib):
    assert lib.mrz_abi_version() == 4
    assert all(hasattr(lib, s) for s in SYMBOLS)


def members():
    sizes = [0, 1, 500, 501, 3000, 4097, 700, 5200, 2600]
    mem = [(b"dir/file%d" % i, 1700000000 + i, R.make_input(R.KINDS[i % 5], n, seed=40 + i)) for i, n in enumerate(sizes)]
    mem.insert(2, (b"", 7, mem[4][2]))                    # an exact duplicate in front of its original, without a name
    mem.append((b"n" * 300, 8, mem[5][2]))                # ... and one behind it, with a long name
    mem.append((b"one-byte-again", 9, mem[1][2]))
    mem.append((b"empty-again", 10, b""))
    return mem


def archive(ctx, which):
    """-> (archive bytes, records as mrz_ar_parse shows them).  Made once per library; nobody changes them."""
    key = (id(ctx.lib), which)
    if key not in _cache:
        ar = ctx.ar_create(members())[0] if which == "created" else A.member_set()[1]
        _cache[key] = (ar, m.ar_parse(ar, ctx.lib))
    return _cache[key]


def selections(recs):
    n = len(recs)
    by_sum = {}
    for i, r in enumerate(recs):
        if r["size"] > 1:
            by_sum.setdefault(r["checksum"], []).append(i)
    shared = next(v for v in by_sum.values() if len(v) >= 2)
    big = max(range(n), key=lambda i: recs[i]["size"])
    return {"all": None, "one": [big], "reversed": list(range(n - 1, -1, -1)), "twice": [big, 0, big],
            "both_copies": [shared[-1], shared[0]], "none": []}


def expected(recs, which):
    idx = list(range(len(recs))) if which is None else which
    offs = [0]
    for i in idx:
        offs.append(offs[-1] + recs[i]["size"])
    distinct = len({(recs[i]["offset"], recs[i]["size"]) for i in idx})
    return b"".join(recs[i]["data"] for i in idx), offs, dict(members=len(idx), distinct_payloads=distinct,
                                                                bytes_out=offs[-1], n_bad=0, first_bad=-1)


def extract(ctx, emu, ar, which, where, out_where, verify=False, n_recs=None):
    """ctx.ar_extract with the archive and the output in the memory spaces asked for -> (bytes, offsets, info)"""
    src, keep = (ar, None) if where == "host" else A.on_device(ar, emu)
    if which is None and where == "device":
        which = list(range(n_recs))
    if out_where == "host":
        return ctx.ar_extract(src, which, verify=verify)
    probe = ctx.ar_extract(ar, which)[2]["bytes_out"]
    buf = torch.full((probe + 64,), 0xC5, dtype=torch.uint8, device="cpu" if emu else "cuda")
    _, offs, info = ctx.ar_extract(src, which, out=(buf.data_ptr(), probe), verify=verify)
    img = buf.cpu().numpy().tobytes()
    assert img[probe:] == b"\xc5" * 64, "bytes behind the output were written"
    return img[:probe], offs, info


def check_extract(ctx, emu, which_archive, where, out_where):
    ar, recs = archive(ctx, which_archive)
    assert {0, 500, 501} <= {r["size"] for r in recs} and {0, 300} <= {len(r["name"]) for r in recs}
    assert which_archive != "created" or 1 in {r["size"] for r in recs}
    for label, which in selections(recs).items():
        data, offs, info = expected(recs, which)
        got = extract(ctx, emu, ar, which, where, out_where, n_recs=len(recs))
        assert got == (data, offs, info), (which_archive, label, where, out_where, got[1:], offs, info)
    assert expected(recs, selections(recs)["both_copies"])[2]["distinct_payloads"] == 1


def check_verify(ctx, emu, where):
    ar, recs = archive(ctx, "created")
    pay = len(ar) - max(r["offset"] + r["size"] for r in recs)
    by_sum = {}
    for i, r in enumerate(recs):
        by_sum.setdefault(r["checksum"], []).append(i)
    sharing = next(v for v in by_sum.values() if len(v) == 3 and recs[v[0]]["size"] > 1)
    # a payload byte: every selected member that shares the payload is named, and the bytes are delivered as they are
    bad = bytearray(ar)
    bad[pay + recs[sharing[0]]["offset"] + 17] ^= 0x20
    bad = bytes(bad)
    others = [i for i in range(len(recs)) if i not in sharing]
    which = [others[0], sharing[2], others[1], sharing[0], sharing[2]]
    data, offs, info = expected(m.ar_parse(bad, ctx.lib), which)
    got, goffs, ginfo = extract(ctx, emu, bad, which, where, where, verify=True)
    assert got == data and goffs == offs and got != expected(recs, which)[0]
    assert ginfo == dict(info, n_bad=3, first_bad=1), ginfo
    got, _, ginfo = extract(ctx, emu, bad, None, where, where, verify=True, n_recs=len(recs))
    assert ginfo["n_bad"] == 3 and ginfo["first_bad"] == sharing[0] and got == expected(m.ar_parse(bad, ctx.lib), None)[0]
    assert extract(ctx, emu, bad, which, where, where, verify=False)[2]["n_bad"] == 0   # not asked, not checked
    ok = [i for i in range(len(recs)) if i not in sharing]
    assert extract(ctx, emu, bad, ok, where, where, verify=True)[2]["n_bad"] == 0
    # a stored checksum byte instead: that record alone
    victim = sharing[1]
    bad = bytearray(ar)
    at = ar.index(recs[victim]["checksum"] + recs[victim]["digest"] + len(recs[victim]["name"]).to_bytes(4, "big")
                  + recs[victim]["name"])
    bad[at + 5] ^= 1
    which = [sharing[0], victim, sharing[2], victim]
    got, _, ginfo = extract(ctx, emu, bytes(bad), which, where, where, verify=True)
    assert got == expected(recs, which)[0] and (ginfo["n_bad"], ginfo["first_bad"]) == (2, 1), ginfo
    assert extract(ctx, emu, ar, None, where, where, verify=True, n_recs=len(recs))[2]["n_bad"] == 0


def corrupt_archives(ar):
    meta = int.from_bytes(ar[5:13], "big")
    beyond = bytearray(ar)
    beyond[13 + 16:13 + 24] = len(ar).to_bytes(8, "big")   # the first record's offset: offset + size leaves the payload
    return {"magic": b"ARZIQ" + ar[5:], "metadata beyond the file": ar[:5] + (len(ar) - 12).to_bytes(8, "big") + ar[13:],
            "offset + size beyond the payload": bytes(beyond), "short": ar[:12],
            "metadata not consumed exactly": ar[:5] + (meta - 1).to_bytes(8, "big") + ar[13:]}


def check_corrupt_and_arguments(ctx, emu):
    ar, recs = archive(ctx, "created")
    for what, bad in corrupt_archives(ar).items():
        for where in ("host", "device"):
            with pytest.raises(m.MrzError) as e:
                extract(ctx, emu, bad, [0], where, "host")
            assert e.value.rc == E_CORRUPT, (what, where)
    for which in ([len(recs)], [0, -1], [2 ** 40]):
        with pytest.raises(m.MrzError) as e:
            ctx.ar_extract(ar, which)
        assert e.value.rc == E_ARG
    # the sizing call fills only the offsets and bytes_out; a capacity one byte short fills them too and writes nothing
    which = [3, 1, 3]
    data, offs, info = expected(recs, which)
    lib, i64 = ctx.lib, ctypes.c_int64
    idx, got_offs, xinfo = (i64 * 3)(*which), (i64 * 4)(), binding.ArExtractInfo()
    assert lib.mrz_ar_extract(ctx.ctx, ar, len(ar), 0, idx, 3, None, 0, 0, got_offs, 1, ctypes.byref(xinfo)) == 0
    assert list(got_offs) == offs and xinfo.as_dict() == info
    buf = ctypes.create_string_buffer(b"\xa5" * len(data), len(data))
    got_offs = (i64 * 4)()
    assert lib.mrz_ar_extract(ctx.ctx, ar, len(ar), 0, idx, 3, buf, 0, len(data) - 1, got_offs, 0, None) == E_ARG
    assert list(got_offs) == offs and buf.raw == b"\xa5" * len(data)
    assert lib.mrz_ar_extract(ctx.ctx, ar, len(ar), 0, idx, 3, buf, 0, len(data), got_offs, 0, None) == 0 and buf.raw == data
    assert lib.mrz_ar_extract(ctx.ctx, ar, len(ar), 0, idx, 3, buf, 0, len(data), got_offs, 2, None) == E_ARG   # flags
    assert lib.mrz_ar_extract(ctx.ctx, ar, len(ar), 0, idx, 3, buf, 0, len(data), None, 0, None) == E_ARG
    assert lib.mrz_ar_extract(ctx.ctx, ar, len(ar), 5, idx, 3, buf, 0, len(data), got_offs, 0, None) == E_ARG


# ---- straight out of a .mrz -------------------------------------------------------------------------------------------

def packed(ctx, kind, ar=None, tag="created"):
    """the archive as a -n or a -l .mrz, at a window that cuts it into chunks of 16 KiB"""
    key = (id(ctx.lib), "mrz", kind, tag)
    if key not in _cache:
        ar = archive(ctx, "created")[0] if ar is None else ar
        fn = m.rzip_buffer if kind == "n" else m.rzip_buffer_lz4
        _cache[key] = fn(ar, ramsize=C.MULTI_CHUNK_RAM, lib=ctx.lib)[0]
    return _cache[key]


def check_extract_mrz(ctx, emu, kind, out_where):
    ar, recs = archive(ctx, "created")
    mrz = packed(ctx, kind)
    chunks = B.parse_mrz(mrz)["chunks"]
    assert len(chunks) >= 2 and m.runzip_buffer(mrz, lib=ctx.lib) == ar
    assert (C.lz4_count(mrz) > 0) == (kind == "l")
    for label, which in selections(recs).items():
        plain = ctx.ar_extract(ar, which, verify=True)
        if out_where == "host":
            data, offs, info, rinfo = m.ar_extract_mrz(mrz, which, verify=True, lib=ctx.lib)
        else:
            total = plain[2]["bytes_out"]
            buf = torch.full((total + 64,), 0xC5, dtype=torch.uint8, device="cpu" if emu else "cuda")
            _, offs, info, rinfo = m.ar_extract_mrz(mrz, which, out=(buf.data_ptr(), total), verify=True, lib=ctx.lib)
            img = buf.cpu().numpy().tobytes()
            assert img[total:] == b"\xc5" * 64
            data = img[:total]
        assert (data, offs, info) == plain, (kind, label, out_where)
        assert (data, offs, info) == expected(recs, which), (kind, label)


def check_one_small_member(ctx, kind):
    """one member of 500 bytes: the three range calls upload less of stream 1 than the archive holds"""
    ar, recs = archive(ctx, "created")
    mrz = packed(ctx, kind)
    small = next(i for i, r in enumerate(recs) if r["size"] == 500)
    data, _, info, rinfo = m.ar_extract_mrz(mrz, [small], lib=ctx.lib)
    print(kind, "archive", len(ar), "mrz", len(mrz), rinfo)
    assert data == recs[small]["data"] and info["bytes_out"] == 500
    assert 0 < rinfo["s1_bytes_uploaded"] < len(ar), (rinfo, len(ar))
    assert 3 <= rinfo["chunks_in_range"] <= 3 * 2


def check_mrz_verify_and_corrupt(ctx, kind):
    ar, recs = archive(ctx, "created")
    pay = len(ar) - max(r["offset"] + r["size"] for r in recs)
    victim = next(i for i, r in enumerate(recs) if r["size"] == 3000)
    sharing = [i for i, r in enumerate(recs) if r["checksum"] == recs[victim]["checksum"]]
    assert len(sharing) == 3
    bad = bytearray(ar)
    bad[pay + recs[victim]["offset"] + 2000] ^= 1
    bad = bytes(bad)
    which = [next(i for i in range(len(recs)) if i not in sharing)] + sharing
    data, _, info, _ = m.ar_extract_mrz(packed(ctx, kind, bad, "flipped"), which, verify=True, lib=ctx.lib)
    assert data == expected(m.ar_parse(bad, ctx.lib), which)[0]
    assert (info["n_bad"], info["first_bad"]) == (len(sharing), 1)
    for what, broken in corrupt_archives(ar).items():
        if what in ("short", "metadata not consumed exactly"):   # the plain call's cases; each .mrz costs a compression
            continue
        with pytest.raises(m.MrzError) as e:
            m.ar_extract_mrz(packed(ctx, kind, broken, what), [0], lib=ctx.lib)
        assert e.value.rc == E_CORRUPT, what
    noise = R.make_input("noise", 3000, seed=9)   # a .mrz that is not an ARZIP
    with pytest.raises(m.MrzError) as e:
        m.ar_extract_mrz(packed(ctx, kind, noise, "noise"), [0], lib=ctx.lib)
    assert e.value.rc == E_CORRUPT
    with pytest.raises(m.MrzError) as e:
        m.ar_extract_mrz(packed(ctx, kind), [len(recs)], lib=ctx.lib)
    assert e.value.rc == E_ARG
    with pytest.raises(m.MrzError) as e:
        m.ar_extract_mrz(b"MRZX" + packed(ctx, kind)[4:], [0], lib=ctx.lib)
    assert e.value.rc == E_CORRUPT
