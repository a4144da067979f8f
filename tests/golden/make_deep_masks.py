"""Generates tests/golden/deep_masks.json: what the repository's oracle (oracle/liboracle.so, level 7, victim_round 0)
returns on whole chunks of the reproducible streams of modern_rzip_amd.workloads (synth_tar, synth_noise) that are large
enough to end beyond 8 bits of tag mask -- the regime of the deep engine, which no smaller committed vector reaches.  Only
hashes, lengths and counters are recorded; the GPU tier rebuilds the inputs on the device (test_synth_gpu.py).

The inputs are built by the host reference, in parallel over byte ranges (any range of a stream is a pure function of the
seed), into one shared buffer; the oracle reads it through a pointer and its two streams are hashed in place, so 16 GiB
and its 14 GB literal stream fit a 62 GB host.  Run:  python tests/golden/make_deep_masks.py [case ...]"""
import ctypes
import hashlib
import json
import mmap
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from modern_rzip_amd import workloads  # noqa: E402

GIB = 1 << 30
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deep_masks.json")
STATS = ("inserts", "literals", "literal_bytes", "matches", "match_bytes", "tag_hits", "tag_misses")

# name -> (generator, N, seed, least number of one-bits of min_mask, tar-shaped).  The conditions (asserted below) are what
# the cases are for: masks beyond the 8 bits smaller vectors reach, and for tar a match share between noise (0) and a
# copy-fest.  Measured on tar(2026): 8 GiB, 12 GiB and 16 GiB all end at 10 bits (min_mask 1023), 24 GiB at 11 (2047); so
# the 11-bit case is 24 GiB, the smallest size tried that reaches it (32 GiB does not fit a 62 GB host beside its literals).
CASES = {
    "s3_8gib": ("synth_tar", 8 * GIB, 2026, 10, True),
    "s3_24gib": ("synth_tar", 24 * GIB, 2026, 11, True),
    "noise_16gib": ("synth_noise", 16 * GIB, 99, 12, False),
}


class Buf(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("len", ctypes.c_int64), ("cap", ctypes.c_int64)]


class OStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in STATS]


def load_oracle():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    L.mrzo_matcher_new.restype = ctypes.c_void_p
    L.mrzo_matcher_new.argtypes = [ctypes.c_int]
    L.mrzo_matcher_free.argtypes = [ctypes.c_void_p]
    L.mrzo_matcher_stats.restype = ctypes.POINTER(OStats)
    L.mrzo_matcher_stats.argtypes = [ctypes.c_void_p]
    for f in ("mrzo_matcher_get_victim_round", "mrzo_matcher_min_mask", "mrzo_matcher_hash_count"):
        getattr(L, f).restype = ctypes.c_int64
        getattr(L, f).argtypes = [ctypes.c_void_p]
    L.mrzo_matcher_set_victim_round.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    L.mrzo_rzip_chunk.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(Buf),
                                  ctypes.POINTER(Buf), ctypes.POINTER(ctypes.c_uint32)]
    L.mrzo_chunk_bytes.argtypes = [ctypes.c_int64]
    L.mrzo_buf_free.argtypes = [ctypes.POINTER(Buf)]
    return L


def sha256_at(addr, n):
    """sha256 of n bytes at an address, without copying them (whole, in 1 GiB updates)."""
    h = hashlib.sha256()
    for a in range(0, n, GIB):
        k = min(GIB, n - a)
        h.update((ctypes.c_uint8 * k).from_address(addr + a))
    return h.hexdigest()


def oracle_chunk(L, addr, n, level=7, victim_round=0):
    """mrzo_rzip_chunk over n bytes at addr: hashes, lengths and counters of the result (the streams are freed)."""
    m = ctypes.c_void_p(L.mrzo_matcher_new(level))
    assert m
    s0, s1, crc = Buf(), Buf(), ctypes.c_uint32()
    try:
        L.mrzo_matcher_set_victim_round(m, victim_round)
        t0 = time.time()
        rc = L.mrzo_rzip_chunk(m, ctypes.c_void_p(addr), n, L.mrzo_chunk_bytes(n), ctypes.byref(s0), ctypes.byref(s1),
                               ctypes.byref(crc))
        wall = time.time() - t0
        assert rc == 0, rc
        st = L.mrzo_matcher_stats(m).contents
        return dict(s0_len=s0.len, s0_sha256=sha256_at(s0.p, s0.len), s1_len=s1.len, s1_sha256=sha256_at(s1.p, s1.len),
                    crc=crc.value, stats={k: getattr(st, k) for k in STATS}, level=level, victim_round_in=victim_round,
                    victim_round=L.mrzo_matcher_get_victim_round(m), min_mask=L.mrzo_matcher_min_mask(m),
                    hash_count=L.mrzo_matcher_hash_count(m), oracle_seconds=round(wall, 1))
    finally:
        L.mrzo_buf_free(ctypes.byref(s0))
        L.mrzo_buf_free(ctypes.byref(s1))
        L.mrzo_matcher_free(m)


_arr = _plan = None


def _fill(job):
    gen, seed, a, b = job
    if gen == "synth_tar":
        _arr[a:b] = workloads.synth_tar(b - a, seed, start=a, plan=_plan)
    else:
        _arr[a:b] = workloads.synth_noise(b - a, seed, start=a)
    return b - a


def build_input(arr, gen, n, seed, piece=64 << 20):
    """Fills arr[:n] with the first n bytes of the stream, one worker per byte range."""
    global _arr, _plan
    _arr, _plan = arr, workloads.synth_tar_plan(n, seed) if gen == "synth_tar" else None
    jobs = [(gen, seed, a, min(n, a + piece)) for a in range(0, n, piece)]
    with multiprocessing.get_context("fork").Pool(min(16, os.cpu_count() or 1)) as pool:
        assert sum(pool.imap_unordered(_fill, jobs)) == n


def main(names):
    L = load_oracle()
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    out["_source"] = ("oracle/liboracle.so (level 7) on modern_rzip_amd.workloads streams, made by "
                      "tests/golden/make_deep_masks.py; hashes are sha256 of the whole input / stream")
    biggest = max(CASES[k][1] for k in names)
    shared = mmap.mmap(-1, biggest)
    arr = np.frombuffer(shared, dtype=np.uint8)
    addr = arr.ctypes.data
    built = None
    for name in sorted(names, key=lambda k: (CASES[k][0], CASES[k][2], -CASES[k][1])):
        gen, n, seed, bits, tar = CASES[name]
        if not (built and built[0] == (gen, seed) and built[1] >= n):  # a prefix of what is there already?
            t0 = time.time()
            build_input(arr, gen, n, seed)
            built = ((gen, seed), n)
            print(f"{name}: input built in {time.time() - t0:.0f} s", flush=True)
        r = dict(generator=gen, N=n, seed=seed, call=f"workloads.{gen}({n}, {seed})", input_sha256=sha256_at(addr, n))
        r.update(oracle_chunk(L, addr, n))
        print(name, json.dumps(r), flush=True)
        assert bin(r["min_mask"]).count("1") >= bits, (name, "mask bits", bin(r["min_mask"]).count("1"), "<", bits)
        if tar:
            assert r["stats"]["matches"] > 0 and 0.05 * n <= r["stats"]["match_bytes"] <= 0.40 * n, (name, r["stats"])
        out[name] = r
        with open(OUT, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:] or sorted(CASES))
