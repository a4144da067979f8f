"""Rates of the LZ4 block codec (mrz_lz4_compress_batch / mrz_lz4_decompress_batch), device memory in and out:
MB/s of ONE wave (a batch of one block) and of a batch of 130 blocks, compress and decompress, on text, noise and
zeros.  MB are 10^6 bytes of UNCOMPRESSED data per second of wall time around the call (which ends with a stream
synchronisation); best of 3 after a warm-up.  No threshold: the numbers go into DESIGN 4.5.
usage: probe_lz4.py [lib.so] [block KiB, default 1024]
Every kind of data runs in a child process of its own under a time limit; the first one that fails ends the probe.
One JSON line per kind."""
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


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(args[1], args[2] or None, int(args[3]))
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
