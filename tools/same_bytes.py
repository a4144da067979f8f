"""GPU over CPU on IDENTICAL bytes, on the S3-faithful stream: builds workloads.synth_tar_device(16 GiB) (fresh text per
member, every byte a function of the seed), times mrz_rzip_chunk on it as one chunk (one warm-up, then three runs with
victim_round reset; host clock around a call that ends in a synchronise), times the oracle once on the same bytes on
this host, checks the two results equal, and times the generator next to tar_like_device for the same size (same process,
alternating).  Writes profiles/synth/same_bytes_s3_16g.json (or --out).  Run as one bounded command:
    timeout -k 10 1100 python tools/same_bytes.py --commit "$(git rev-parse --short HEAD)"
usage: python tools/same_bytes.py [--gib 16] [--seed 2026] [--runs 3] [--commit ID] [--out FILE]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import modern_rzip_amd as m  # noqa: E402
from modern_rzip_amd import workloads as w  # noqa: E402
from tests.golden import make_deep_masks as dm  # noqa: E402  (the oracle wrapper that hashes its buffers in place)

PIECE = 1 << 30


def sha_device(ctx, ptr, n):
    h = hashlib.sha256()
    stage = torch.empty(min(PIECE, max(n, 1)), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    for a in range(0, n, PIECE):
        k = min(PIECE, n - a)
        ctx.copy_to(stage.data_ptr(), (ptr + a, k))
        h.update(stage[:k].cpu().numpy())
    return h.hexdigest()


def commit_id(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], check=True, stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, text=True).stdout.strip()
    except Exception:  # noqa: BLE001 -- a tree without its history
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=16.0)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth", "same_bytes_s3_16g.json"))
    a = ap.parse_args()
    n = int(a.gib * (1 << 30))
    lib = m.load_library()
    out = {"stream": f"workloads.synth_tar({n}, {a.seed})", "N": n, "level": 7, "commit": commit_id(a.commit),
           "device": torch.cuda.get_device_name(0)}

    # the generators, alternating: set-up cost, not timed path
    gen_new, gen_old = [], []
    with m.RzipContext(level=1, lib=lib) as gctx:
        plan = w.synth_tar_plan(n, a.seed)
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t = w.synth_tar_device(n, "cuda", a.seed, ctx=gctx, plan=plan)
            torch.cuda.synchronize()
            gen_new.append(time.perf_counter() - t0)
            del t
            t0 = time.perf_counter()
            t = w.tar_like_device(n, "cuda")
            torch.cuda.synchronize()
            gen_old.append(time.perf_counter() - t0)
            del t
        t0 = time.perf_counter()
        plan = w.synth_tar_plan(n, a.seed)
        out["generator"] = {"synth_tar_device_s": gen_new, "tar_like_device_s": gen_old, "members": len(plan),
                            "synth_tar_plan_host_s": time.perf_counter() - t0}
        t = w.synth_tar_device(n, "cuda", a.seed, ctx=gctx, plan=plan)
    print(json.dumps(out["generator"]), flush=True)

    with m.RzipContext(lib=lib, max_chunk=n) as ctx:
        times = []
        for i in range(a.runs + 1):  # the first is the warm-up
            ctx.victim_round = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, _, _ = ctx.rzip_chunk(t, fetch=False)  # returns after its own synchronise
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            print("gpu run", i, f"{times[-1]:.2f} s", flush=True)
        tm = ctx.timings()
        gpu = dict(s0_len=res.s0_len, s0_sha256=sha_device(ctx, res.d_s0, res.s0_len), s1_len=res.s1_len,
                   s1_sha256=sha_device(ctx, res.d_s1, res.s1_len), crc=res.crc32, stats=res.stats.as_dict(),
                   victim_round=ctx.victim_round, min_mask=res.min_mask, hash_count=res.hash_count)
        out["gpu"] = {"warmup_s": times[0], "runs_s": times[1:], "result": gpu,
                      "launches": {"segments": tm.n_segments, "narrow": tm.n_narrow, "deep": tm.n_deep,
                                   "wide": tm.n_segments - tm.n_narrow - tm.n_deep, "event_flushes": tm.n_event_flushes}}
    host = t.cpu().numpy()
    del t
    torch.cuda.empty_cache()
    want = dm.oracle_chunk(dm.load_oracle(), host.ctypes.data, n)
    print("oracle", want["oracle_seconds"], "s", flush=True)
    out["oracle"] = {"seconds": want["oracle_seconds"], "result": {k: want[k] for k in gpu}}
    out["equal"] = all(gpu[k] == want[k] for k in gpu)
    best = min(times[1:])
    st = gpu["stats"]
    out.update(gpu_best_s=best, gpu_gib_per_s=n / best / (1 << 30), oracle_gib_per_s=n / want["oracle_seconds"] / (1 << 30),
               gpu_over_cpu_same_bytes=want["oracle_seconds"] / best, match_byte_share=st["match_bytes"] / n,
               literal_byte_share=st["literal_bytes"] / n, final_mask_bits=bin(gpu["min_mask"]).count("1"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("gpu_best_s", "gpu_over_cpu_same_bytes", "equal", "final_mask_bits")}), flush=True)
    if not out["equal"]:
        first = next(k for k in gpu if gpu[k] != want[k])
        sys.exit(f"MISMATCH: {first}: gpu {gpu[first]} oracle {want[first]}")


if __name__ == "__main__":
    main()
