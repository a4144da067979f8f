"""CPU tier: the reproducible streams of include/mrzgpu_synth.h.  The host reference (workloads.synth_*) is pinned by
committed hashes; the kernels of csrc/mrz_synth.hip, compiled for the wave64 emulator, must agree with it byte for byte
for any start and length; the member plan has the S3 mix; libmrzgpu.so exports the header's symbols."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

import modern_rzip_amd as m
from modern_rzip_amd import workloads as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "synth_streams.json")))
VS = 12  # a vocabulary seed


@pytest.fixture(scope="module")
def ectx(emu_lib):
    with m.RzipContext(level=1, lib=emu_lib) as ctx:
        yield ctx


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]} of {got.size}"


# ---- the host reference ------------------------------------------------------------------------------------------------

def test_mixer_constants():
    assert int(w.synth_rnd(1, 0, 0)[0]) == GOLDEN["rnd"]["rnd(1,0,0)"] == 0x5e41ab087439611e
    assert int(w.synth_rnd(2 ** 64 - 1, 9, 12345678901234)[0]) == GOLDEN["rnd"]["rnd(2^64-1,9,12345678901234)"]
    assert int(w.synth_zipf_table()[-1]) == GOLDEN["rnd"]["zipf_total"] == 2441286195


@pytest.mark.parametrize("case", GOLDEN["streams"], ids=lambda c: c["gen"] + "-" + "-".join(str(v) for v in c["args"].values()))
def test_host_reference_matches_committed_hashes(case):
    data = getattr(w, case["gen"])(**case["args"])
    assert data.dtype == np.uint8 and len(data) == case["args"]["nbytes"]
    assert hashlib.sha256(data.tobytes()).hexdigest() == case["sha256"]


def test_host_reference_is_what_the_definition_says():
    """The vectorised reference against a word-by-word, byte-by-byte reading of the definition."""
    rnd = lambda seed, stream, i: int(w.synth_rnd(seed, stream, i)[0])  # noqa: E731
    assert bytes(w.synth_noise(21, 5, start=3)) == bytes((rnd(5, w.SYN_NOISE, j >> 3) >> 8 * (j & 7)) & 255 for j in range(3, 24))
    cum, c = [], 0
    for i in range(5000):
        c += (1 << 28) // (i + 1)
        cum.append(c)
    words = [bytes(97 + rnd(VS, w.SYN_VCHAR, 10 * k + c) % 26 for c in range(2 + rnd(VS, w.SYN_VLEN, k) % 9)) for k in range(5000)]
    text = bytearray()
    for k in range(400):
        u = rnd(3, w.SYN_WORD, k) % cum[-1]
        text += words[next(r for r in range(5000) if cum[r] > u)] + b" "
    assert bytes(w.synth_text(len(text), 3, VS)) == bytes(text)
    # the separator of every 20000th word is a newline
    t = w.synth_text(200000, 3, VS)
    seps = np.nonzero((t == 32) | (t == 10))[0]
    assert t[seps[19999]] == 10 and t[seps[19998]] == 32 and t[seps[20000]] == 32 and (t == 10).sum() == len(seps) // 20000


def test_host_ranges_are_independent_of_what_precedes_them():
    whole = w.synth_tar(3 << 20, 5)
    for start, n in ((0, 1), (511, 2), (100001, 555555), ((3 << 20) - 7, 7)):
        same(w.synth_tar(n, 5, start=start), whole[start:start + n])
    same(w.synth_noise(1001, 5, start=77), w.synth_noise(2000, 5)[77:1078])


def test_plan_at_1gib_has_the_s3_mix():
    n = 1 << 30
    plan = w.synth_tar_plan(n, 2026)
    cnt = len(plan)
    assert 1500 < cnt < 2600
    dup = plan["origin"] >= 0
    text = (plan["kind"] == w.SYN_KIND_TEXT) & ~dup
    noise = (plan["kind"] == w.SYN_KIND_NOISE) & ~dup
    for share, p in ((text.sum() / cnt, 0.60), (noise.sum() / cnt, 0.25), (dup.sum() / cnt, 0.15)):
        assert abs(share - p) <= 3 * (p * (1 - p) / cnt) ** 0.5, (share, p, cnt)
    assert (plan["dst"] % 512 == 0).all() and plan["dst"][0] == 0 and plan["dst"][-1] < n
    assert (plan["size"] >= 1 << 10).all() and (plan["size"] < 4 << 20).all()
    ends = (plan["dst"] + plan["size"] + 511) & ~511
    assert (plan["dst"][1:] == ends[:-1]).all() and ends[-1] >= n
    o = plan["origin"][dup]
    assert (o < np.nonzero(dup)[0]).all() and (plan["origin"][o] == -1).all()  # an original is never a duplicate
    for f in ("size", "seed", "kind"):
        assert (plan[f][dup] == plan[f][o]).all()
    assert plan.dtype.itemsize == 32


DUP_SEED = 14  # member 3 of tar(14) duplicates member 2, which duplicates member 1


def test_a_duplicate_of_a_duplicate_resolves_to_the_original():
    plan = w.synth_tar_plan(3 << 20, DUP_SEED)
    drawn = int(w.synth_rnd(DUP_SEED, w.SYN_DUP, 3)[0] % np.uint64(3))
    assert (drawn, int(plan["origin"][2]), int(plan["origin"][3])) == (2, 1, 1)
    data = w.synth_tar(3 << 20, DUP_SEED)
    a, b, c = (int(plan["dst"][i]) for i in (1, 2, 3))
    size = int(plan["size"][1])
    same(data[b:b + size], data[a:a + size])
    same(data[c:c + size], data[a:a + size])


# ---- the kernels on the emulator ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,seed,start", [(1, 3, 0), (15, 3, 1), (16, 3, 16), (17, 3, 15), (1000, 3, 13),
                                          ((1 << 20) + 77, 9, 5), ((2 << 20) + 1, 9, (1 << 33) + 3), (4099, 2 ** 64 - 1, 7)])
def test_emulated_noise(ectx, n, seed, start):
    same(w.synth_noise_device(n, "cpu", seed, start=start, ctx=ectx).numpy(), w.synth_noise(n, seed, start))


def test_emulated_noise_into_an_unaligned_buffer(ectx):
    import torch
    buf = torch.zeros(5000 + 64, dtype=torch.uint8)
    for shift in (1, 7, 8, 15):
        buf.zero_()
        ectx.synth_noise(buf[shift:], 5000, 21, start=3)
        same(buf[shift:shift + 5000].numpy(), w.synth_noise(5000, 21, 3))
        assert not buf[:shift].any() and not buf[shift + 5000:].any()  # nothing outside the range is written


@pytest.mark.parametrize("n", [1, 15, 16, 17, 5000, 100000, (1 << 20) + 3])
def test_emulated_text(ectx, n):
    same(w.synth_text_device(n, "cpu", 11, VS, ctx=ectx).numpy(), w.synth_text(n, 11, VS))


def test_emulated_text_longer_than_one_tile_scan(ectx):
    """2 MiB is 342 tiles by the size / 3 bound: more than the 256 the scan kernel takes per round."""
    n = 2 << 20
    same(w.synth_text_device(n, "cpu", 2 ** 63 + 5, 0, ctx=ectx).numpy(), w.synth_text(n, 2 ** 63 + 5, 0))


def test_emulated_tar_whole_and_in_ranges(ectx):
    n = (5 << 20) + 5
    ref = w.synth_tar(n, 13)
    plan = w.synth_tar_plan(n, 13)
    assert {0, 1} <= set(plan["kind"].tolist()) and (plan["origin"] >= 0).any()
    same(w.synth_tar_device(n, "cpu", 13, ctx=ectx).numpy(), ref)
    cuts = [0, 1, 511, 512, 513, 100001, int(plan["dst"][2]) + 1, int(plan["dst"][3]) - 1, (2 << 20) + 333, n - 100, n]
    cuts = sorted(set(cuts))
    parts = [w.synth_tar_device(b - a, "cpu", 13, start=a, ctx=ectx).numpy() for a, b in zip(cuts, cuts[1:])]
    same(np.concatenate(parts), ref)


def test_emulated_tar_with_a_duplicate_of_a_duplicate(ectx):
    n = 3 << 20
    same(w.synth_tar_device(n, "cpu", DUP_SEED, ctx=ectx).numpy(), w.synth_tar(n, DUP_SEED))


def test_emulated_tar_on_a_hand_made_plan(ectx):
    """Members that are not 512-aligned, a gap in front, the same text twice: what no member covers is zero."""
    import torch
    plan = np.zeros(4, dtype=w.SYNTH_MEMBER)
    plan["dst"], plan["size"] = [3, 70001, 90000, 200000], [70000 - 3, 1, 100001, 50000]
    plan["seed"], plan["kind"], plan["origin"] = [5, 6, 5, 8], [0, 1, 0, 1], [-1, -1, 0, -1]
    n = 250000
    ref = w.synth_tar(n, 0, plan=plan)
    same(ref[90000:90000 + 69997], ref[3:70000])
    assert not ref[:3].any() and not ref[70002:90000].any() and ref[70001] == w.synth_noise(1, 6)[0]
    vs = w.synth_tar_vocab_seed(0)
    for start, ln in ((0, n), (2, 5), (69999, 20002), (123457, 99999)):
        out = torch.full((ln,), 0xAA, dtype=torch.uint8)
        ectx.synth_tar(out, ln, plan, vs, start=start)
        same(out.numpy(), ref[start:start + ln])


def test_bad_arguments_are_refused(ectx):
    import torch
    out = torch.zeros(4096, dtype=torch.uint8)
    plan = w.synth_tar_plan(3 << 20, DUP_SEED)
    end = (int(plan["dst"][-1] + plan["size"][-1]) + 511) & ~511
    with pytest.raises(m.MrzError):
        ectx.synth_tar(out, 4096, plan, 1, start=end - 4095)  # ends beyond the plan
    with pytest.raises(m.MrzError):
        ectx.synth_tar(out, 4096, plan[::-1], 1)  # not ascending
    with pytest.raises(m.MrzError):
        ectx.synth_noise(out, 4097, 1)  # more than the buffer holds
    with pytest.raises(m.MrzError):
        ectx.synth_noise(out, 16, 1, start=-1)
    ectx.synth_text(out, 0, 1, 2)  # nothing asked for, nothing done


# ---- the library --------------------------------------------------------------------------------------------------------

def test_library_exports_the_synth_header():
    path = m.lib_path()
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    src = open(os.path.join(ROOT, "include", "mrzgpu_synth.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(mrz_[a-z0-9_]+)\s*\(", src)))
    assert names == ["mrz_synth_noise", "mrz_synth_tar", "mrz_synth_text"]
    lib = ctypes.CDLL(path)
    assert not [s for s in names if not hasattr(lib, s)]
    assert lib.mrz_abi_version() == 4
    assert ctypes.sizeof(ctypes.c_int64) * 3 + 8 == w.SYNTH_MEMBER.itemsize  # mrz_synth_member
