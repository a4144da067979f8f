"""Times of the member extractor on the device against what the library offered before it
(profiles/ar_extract/README.md):
  copy_small   mrz_copy_device_batch of 10^5 payloads of 2 KiB against 10^5 mrz_copy_device calls
  copy_big     mrz_copy_device_batch (mrz_seg_copy_kernel) over the members of 1 MiB: GB/s read + written
  extract:n    an ARZIP of --members x 1 MiB members (text, noise, 15 % exact duplicates) as a -n .mrz:
               mrz_ar_extract_mrz of 1, 64 and all members, against mrz_runzip_buffer of the whole archive plus host
               slicing, and against one mrz_runzip_buffer_range_ex call per member (at most 64 members: more are scaled)
  extract:l    the same as a -l .mrz
Wall time around each call (every call ends with a stream synchronisation); one warm-up, then 5 runs: min, median, max.
GB are 10^9 bytes.  No threshold.
usage: probe_ar_extract.py [--members N] [--only step[,step]] [lib.so]
Every step runs in a child process of its own under a time limit; the first one that fails ends the probe.  One JSON
line per step."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("copy_small", "copy_big", "extract:n", "extract:l")
STEP_LIMIT_S = 500
RUNS = 5
MEMBER = 1 << 20


def timed(fn):
    fn()
    t = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"min_s": min(t), "median_s": statistics.median(t), "max_s": max(t)}


def member_mix(count):
    """text, noise and 15 % exact duplicates, 1 MiB each: slices of two pools, as profiles/ar_index has them"""
    import numpy as np

    from modern_rzip_amd import workloads
    rng = np.random.default_rng(11)
    text = np.frombuffer(workloads.zipf_text(32 << 20, seed=3), dtype=np.uint8)
    noise = np.frombuffer(workloads.noise(32 << 20, seed=4), dtype=np.uint8)
    mem = []
    for i in range(count):
        if mem and rng.random() < 0.15:
            mem.append((b"dup%d" % i, i, mem[int(rng.integers(0, len(mem)))][2]))
        else:
            pool = text if i % 2 else noise
            off = int(rng.integers(0, len(pool) - MEMBER))
            mem.append((b"member%d" % i, i, pool[off:off + MEMBER].tobytes()))
    return mem


def step(name, members, lib_path):
    import numpy as np
    import torch

    import modern_rzip_amd as m
    lib = m.load_library(lib_path)
    name, _, kind = name.partition(":")
    res = {"step": name + (":" + kind if kind else ""), "members": members}
    with m.RzipContext(lib=lib) as ctx:
        if name == "copy_small":
            n, each = 10 ** 5, 2048
            src = torch.randint(0, 256, (n * each,), dtype=torch.uint8, device="cuda")
            dst = torch.zeros(n * each, dtype=torch.uint8, device="cuda")
            order = np.random.default_rng(1).permutation(n)
            segs = [(src.data_ptr() + int(order[i]) * each, dst.data_ptr() + i * each, each) for i in range(n)]
            src_a = (m.binding.ctypes.c_void_p * n)(*[s[0] for s in segs])
            dst_a = (m.binding.ctypes.c_void_p * n)(*[s[1] for s in segs])
            len_a = (m.binding.ctypes.c_int64 * n)(*[s[2] for s in segs])
            res["batch"] = timed(lambda: lib.mrz_copy_device_batch(ctx.ctx, src_a, dst_a, len_a, n))
            same = bool(torch.equal(dst.view(n, each), src.view(n, each)[torch.from_numpy(order).cuda()]))

            def loop():
                for s, d, k in segs:
                    lib.mrz_copy_device(ctx.ctx, d, s, k)
            dst.zero_()
            res["loop"] = timed(loop)
            res.update(segments=n, bytes=n * each, same_bytes=same,
                       loop_over_batch=res["loop"]["median_s"] / res["batch"]["median_s"])
        elif name == "copy_big":
            n = members
            src = torch.randint(0, 256, (n * MEMBER,), dtype=torch.uint8, device="cuda")
            dst = torch.zeros(n * MEMBER, dtype=torch.uint8, device="cuda")
            segs = [(src.data_ptr() + (n - 1 - i) * MEMBER, dst.data_ptr() + i * MEMBER, MEMBER) for i in range(n)]
            res.update(timed(lambda: ctx.copy_device_batch(segs)), bytes=n * MEMBER)
            res["GBps_read_plus_written"] = 2 * n * MEMBER / res["median_s"] / 1e9
            res["same_bytes"] = bool(torch.equal(dst.view(n, MEMBER), src.view(n, MEMBER).flip(0)))
        elif name == "extract":
            mem = member_mix(members)
            ar, info = ctx.ar_create(mem)
            recs = m.ar_parse(ar, lib)
            pack = m.rzip_buffer if kind == "n" else m.rzip_buffer_lz4
            t0 = time.perf_counter()
            mrz = pack(ar, lib=lib)[0]
            res.update(archive_bytes=len(ar), mrz_bytes=len(mrz), pack_s=time.perf_counter() - t0, **info)
            pay = len(ar) - info["unique_bytes"]
            out = torch.empty(sum(r["size"] for r in recs) + 64, dtype=torch.uint8, device="cuda")
            for label, which in (("one", [len(recs) // 2]), ("sixty_four", list(range(0, len(recs), max(1, len(recs) // 64)))[:64]),
                                 ("all", list(range(len(recs))))):
                got = {}

                def new_way():
                    got["r"] = m.ar_extract_mrz(mrz, which, out=out, lib=lib)
                r = timed(new_way)
                _, offs, xinfo, rinfo = got["r"]
                want = b"".join(recs[i]["data"] for i in which[:4])
                r.update(selected=len(which), bytes_out=xinfo["bytes_out"], range_info=rinfo,
                         same_bytes=out[:len(want)].cpu().numpy().tobytes() == want)

                def whole():
                    data = m.runzip_buffer(mrz, lib=lib)
                    return [data[pay + recs[i]["offset"]:pay + recs[i]["offset"] + recs[i]["size"]] for i in which]
                r["whole_decode_and_slice"] = timed(whole)
                some = which[:64]

                def per_member():
                    for i in some:
                        m.runzip_buffer_range_ex(mrz, pay + recs[i]["offset"], recs[i]["size"], out=out, lib=lib)
                pm = timed(per_member)
                pm["calls_timed"] = len(some)
                pm["median_s_scaled"] = pm["median_s"] * len(which) / len(some)
                r["range_ex_per_member"] = pm
                res[label] = r
    return res


def main():
    args = sys.argv[1:]
    members = 4096
    if "--members" in args:
        k = args.index("--members")
        members = int(args[k + 1])
        del args[k:k + 2]
    if args and args[0] == "--step":
        print(json.dumps(step(args[1], members, args[2] if len(args) > 2 and args[2] else None)), flush=True)
        return
    only = None
    if "--only" in args:
        k = args.index("--only")
        only = args[k + 1].split(",")
        del args[k:k + 2]
    lib_path = args[0] if args else ""
    for name in STEPS:
        if only and name not in only:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--members", str(members), "--step", name, lib_path],
                           timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            print(json.dumps({"step": name, "failed": r.returncode}), flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
