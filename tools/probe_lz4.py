"""Rates of the LZ4 block codec (mrz_lz4_compress_batch / mrz_lz4_decompress_batch), device memory in and out:
MB/s of ONE wave (a batch of one block) and of a batch of 130 blocks, compress and decompress, on text, noise and
zeros.  MB are 10^6 bytes of UNCOMPRESSED data per second of wall time around the call (which ends with a stream
synchronisation); best of 3 after a warm-up.  No threshold: the numbers go into DESIGN 4.5.
usage: probe_lz4.py [lib.so] [block KiB, default 1024]
Every kind of data runs in a child process of its own under a time limit; the first one that fails ends the probe.
One JSON line per kind.

usage: probe_lz4.py --range [lib.so] [--parent parent_lib.so] [MiB, default 256]
Range decode over -l archives (mrz_runzip_buffer_range_ex): a text and a noise file of that size, written by
mrz_rzip_buffer_lz4 with as many threads as give 10 MiB LZ4 blocks; wall time (best of 3 after a warm-up) of ranges of
4 KiB and 1 MiB at the start, in the middle and at the end, each with its mrz_archive_range_info, against the wall time
of mrz_runzip_buffer on the same archive -- with this build and, where --parent names a build of the parent commit, with
that one in the same process.  No threshold: the table goes into DESIGN 4.8."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("text", "noise", "zeros")
BATCH = 130
STEP_LIMIT_S = 240


def step(kind, lib_path, kib):
    import torch

    import modern_rzip_amd as m
    from modern_rzip_amd import workloads as w
    n = kib << 10
    lib = m.load_library(lib_path)
    blocks = []
    for i in range(BATCH):  # different bytes in every block
        blocks.append({"text": lambda: w.zipf_text(n, seed=100 + i), "noise": lambda: w.noise(n, seed=100 + i),
                       "zeros": lambda: bytes(n)}[kind]())
    bound = lib.mrz_lz4_bound(n)
    src = torch.frombuffer(bytearray(b"".join(blocks)), dtype=torch.uint8).cuda()
    packed = torch.zeros(BATCH * bound, dtype=torch.uint8, device="cuda")
    back = torch.zeros(BATCH * n, dtype=torch.uint8, device="cuda")
    ins = [(src.data_ptr() + i * n, n) for i in range(BATCH)]
    outs = [(packed.data_ptr() + i * bound, bound) for i in range(BATCH)]
    res = {"kind": kind, "block_bytes": n}

    def best(fn):
        fn()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return min(t)

    with m.RzipContext(lib=lib) as ctx:
        for count in (1, BATCH):
            lens = []
            dt = best(lambda: lens.__setitem__(slice(None), ctx.lz4_compress(ins[:count], [bound] * count, outs=outs[:count])))
            assert all(k > 0 for k in lens)
            res[f"compress_MBps_{count}"] = round(count * n / dt / 1e6, 2)
            comp = [(outs[i][0], lens[i]) for i in range(count)]
            dst = [(back.data_ptr() + i * n, n) for i in range(count)]
            st = []
            dt = best(lambda: st.__setitem__(slice(None), ctx.lz4_decompress(comp, [n] * count, outs=dst)[1]))
            assert st == [0] * count
            res[f"decompress_MBps_{count}"] = round(count * n / dt / 1e6, 2)
            res[f"ratio_{count}"] = round(sum(lens) / (count * n), 4)
        assert torch.equal(back, src)
    print(json.dumps(res), flush=True)


RANGE_KINDS = ("text", "noise")
RANGE_LIMIT_S = 420


def range_step(kind, lib_path, parent_path, mib):
    import torch

    import modern_rzip_amd as m
    n = mib << 20
    lib = m.load_library(lib_path)
    with m.RzipContext(lib=lib) as ctx:
        t = torch.empty(n, dtype=torch.uint8, device="cuda")
        if kind == "text":
            ctx.synth_text(t, n, 7, 11)
        else:
            ctx.synth_noise(t, n, 7)
        torch.cuda.synchronize()
        data = t.cpu().numpy().tobytes()
        del t
    arc, _, _ = m.rzip_buffer_lz4(data, threads=max(1, n // (10 << 20)), lib=lib)
    res = {"kind": kind, "bytes": n, "archive_bytes": len(arc), "ranges": []}

    def best(fn, reps=3):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return min(t)

    got = []
    res["whole_s"] = round(best(lambda: got.__setitem__(slice(None), [m.runzip_buffer(arc, lib=lib)]), 2), 4)
    assert got[0] == data
    if parent_path:
        parent = m.load_library(parent_path)
        assert not hasattr(parent, "mrz_runzip_buffer_range_ex"), "--parent names a build that has the new call"
        res["whole_parent_s"] = round(best(lambda: got.__setitem__(slice(None), [m.runzip_buffer(arc, lib=parent)]), 2), 4)
        assert got[0] == data
    for size in (4 << 10, 1 << 20):
        for where, first in (("start", 0), ("middle", (n - size) // 2), ("end", n - size)):
            dt = best(lambda: got.__setitem__(slice(None), m.runzip_buffer_range_ex(arc, first, size, lib=lib)))
            assert got[0] == data[first:first + size] and got[1] == n
            res["ranges"].append({"size": size, "where": where, "s": round(dt, 5), "info": got[2]})
    print(json.dumps(res), flush=True)


def range_main(args):
    parent = ""
    if "--parent" in args:
        i = args.index("--parent")
        parent = args[i + 1]
        del args[i:i + 2]
    lib_path = next((a for a in args if not a.isdigit()), "")
    mib = next((int(a) for a in args if a.isdigit()), 256)
    for kind in RANGE_KINDS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--range-step", kind, lib_path, parent, str(mib)],
                               timeout=RANGE_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"probe_lz4: {kind} ran into its time limit; stopping", file=sys.stderr)
            return 1
        if r.returncode:
            print(f"probe_lz4: {kind} failed with {r.returncode}; stopping", file=sys.stderr)
            return 1
    return 0


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(args[1], args[2] or None, int(args[3]))
    if args and args[0] == "--range-step":
        return range_step(args[1], args[2] or None, args[3] or None, int(args[4]))
    if args and args[0] == "--range":
        return range_main(args[1:])
    lib_path = args[0] if args and not args[0].isdigit() else ""
    kib = next((int(a) for a in args if a.isdigit()), 1024)
    for kind in KINDS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, lib_path, str(kib)],
                               timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"probe_lz4: {kind} ran into its time limit; stopping", file=sys.stderr)
            return 1
        if r.returncode:
            print(f"probe_lz4: {kind} failed with {r.returncode}; stopping", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
