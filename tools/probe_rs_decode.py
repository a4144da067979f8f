"""Device time of the RS(255,223) decoder (device in, device out, checksum skipped) on four damage profiles:
    clean      nothing damaged: every codeword ends with its syndromes
    scattered  1 % of the codewords, 1..16 byte errors each
    burst      in every 8th burst a contiguous run of 16 x 8176 damaged bytes: 16 errors in each of its codewords
    lost-run   in every 8th burst a zero-filled run of 32 x 8176 bytes, declared lost (mrz_rs_decode_lost): 32 erasures
               in each of its codewords.  A library without mrz_rs_decode_lost is not run on it.
usage: probe_rs_decode.py [lib.so [parent.so]] [GiB]
One JSON line per library and profile: the median of 5 timed runs after a warm-up.  timings_ms is what the library
reports (mrz_timings.encode_ms); kernel_ms is the sum of its decode kernels' durations as torch.profiler sees them
(repair_ms: the repair kernel's share of it),
which also works for a library without mrz_rs_decode_ex (a build of an earlier commit: it is called through
mrz_rs_decode with device input, and its copy to the host and its hash are not part of kernel_ms).  With a second
library both must produce the same bytes and totals, and a line with the ratio new / parent follows for every profile."""
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

import modern_rzip_amd as m  # noqa: E402

ROWS, K, N = 8176, 223, 255
BURST = ROWS * N
RUNS = 5


def damage(enc, nbursts, kind, gen):
    """the damaged copy of `enc` (a cuda uint8 tensor)"""
    enc = enc.clone()
    if kind == "scattered":
        rows = nbursts * ROWS
        k = rows // 100
        pick = torch.randperm(rows, device="cuda", generator=gen)[:k]
        nerr = torch.randint(1, 17, (k,), device="cuda", generator=gen)
        cols = torch.rand((k, N), device="cuda", generator=gen).argsort(dim=1)[:, :16]  # distinct columns per row
        vals = torch.randint(1, 256, (k, 16), device="cuda", generator=gen).to(torch.uint8)
        use = torch.arange(16, device="cuda")[None, :] < nerr[:, None]
        pos = ((pick // ROWS) * BURST + pick % ROWS)[:, None] + cols * ROWS
        pos, vals = pos[use], vals[use]
        enc[pos] = enc[pos] ^ vals
    elif kind == "burst":
        for b in range(0, nbursts, 8):
            enc[b * BURST + 5000:b * BURST + 5000 + 16 * ROWS] ^= 0xa5
    elif kind == "lost-run":
        for off, n in lost_runs(nbursts):
            enc[off:off + n] = 0
    return enc


def lost_runs(nbursts):
    """the (offset, len) ranges of the lost-run profile"""
    return [(b * BURST + 5000, 32 * ROWS) for b in range(0, nbursts, 8)]


def kernel_ms(fn):
    """device time of the rs decode kernels that fn() launches and of the repair kernel among them, by the profiler;
    (None, None) if it saw none"""
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    us = [(getattr(e, "device_time_total", 0) or getattr(e, "cuda_time_total", 0), "mrz_rs_repair_kernel" in e.name)
          for e in prof.events() if "mrz_rs_decode_kernel" in e.name or "mrz_rs_repair_kernel" in e.name]
    return (sum(u for u, _ in us) / 1e3, sum(u for u, rep in us if rep) / 1e3) if us else (None, None)


def main():
    libs = [a for a in sys.argv[1:] if a.endswith(".so")]
    args = [a for a in sys.argv[1:] if not a.endswith(".so")]
    gib = float(args[0]) if args else 1.0
    n = int(gib * (1 << 30))
    new = m.load_library(libs[0]) if libs else m.load_library()
    named = [("new", new)] + ([("parent", m.load_library(libs[1]))] if len(libs) > 1 else [])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    total = new.mrz_rs_encoded_size(n)
    nbursts = total // BURST
    clean = torch.empty(total, dtype=torch.uint8, device="cuda")
    with m.RzipContext(lib=new) as ctx:
        rc = new.mrz_rs_encode(ctx.ctx, ctypes.c_void_p(src.data_ptr()), n, 1, ctypes.c_void_p(clean.data_ptr()), 1, total)
        assert rc == 0, rc
    del src
    cap = nbursts * ROWS * K
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    medians = {}
    for kind in ("clean", "scattered", "burst", "lost-run"):
        enc = damage(clean, nbursts, kind, gen)
        runs_lost = lost_runs(nbursts)
        ranges = (m.binding.RsRange * len(runs_lost))(*[m.binding.RsRange(o, ln) for o, ln in runs_lost])
        for name, lib in named:
            if kind == "lost-run" and not hasattr(lib, "mrz_rs_decode_lost"):
                print(json.dumps(dict(lib=name, profile=kind, note="this library has no mrz_rs_decode_lost")), flush=True)
                continue
            ex = hasattr(lib, "mrz_rs_decode_ex")
            host_out = None if ex else ctypes.create_string_buffer(cap)
            with m.RzipContext(lib=lib) as ctx:
                ctx.set_profiling(True)
                out_len, rep = ctypes.c_int64(), m.binding.RsReport()

                def call():
                    if kind == "lost-run":
                        rc = lib.mrz_rs_decode_lost(ctx.ctx, ctypes.c_void_p(enc.data_ptr()), total, 1,
                                                    ctypes.c_void_p(d_out.data_ptr()), 1, cap, ctypes.byref(out_len), ranges,
                                                    len(runs_lost), None, 0, 1, ctypes.byref(rep))
                    elif ex:
                        rc = lib.mrz_rs_decode_ex(ctx.ctx, ctypes.c_void_p(enc.data_ptr()), total, 1,
                                                  ctypes.c_void_p(d_out.data_ptr()), 1, cap, ctypes.byref(out_len), None, 0,
                                                  1, ctypes.byref(rep))
                    else:
                        rc = lib.mrz_rs_decode(ctx.ctx, ctypes.c_void_p(enc.data_ptr()), total, 1, host_out, cap,
                                               ctypes.byref(out_len), ctypes.byref(rep))
                    assert rc == 0, rc

                call()  # warm-up
                runs = []
                for _ in range(RUNS):
                    t0 = time.perf_counter()
                    k_ms, r_ms = kernel_ms(call)
                    runs.append(dict(kernel_ms=k_ms, repair_ms=r_ms, call_ms=(time.perf_counter() - t0) * 1e3,
                                     timings_ms=ctx.timings().encode_ms if ex else None))
                produced = d_out.cpu().numpy().data if ex else memoryview(host_out).cast("B")
                digest = hashlib.blake2b(produced[:out_len.value], digest_size=8).hexdigest()
            k = [r["kernel_ms"] for r in runs]
            measured = all(v is not None for v in k)
            line = dict(lib=name, profile=kind, n=n, bursts=nbursts, corrected=rep.corrected,
                        uncorrectable=rep.uncorrectable, out_len=out_len.value, out_blake2b=digest,
                        kernel_ms_runs=[round(v, 3) for v in k] if measured else None,
                        kernel_ms_median=round(statistics.median(k), 3) if measured else None,
                        kernel_ms_spread=round(max(k) - min(k), 3) if measured else None,
                        repair_ms_median=round(statistics.median(r["repair_ms"] for r in runs), 3) if measured else None,
                        timings_ms_median=round(statistics.median(r["timings_ms"] for r in runs), 3) if ex else None,
                        call_ms_median=round(statistics.median(r["call_ms"] for r in runs), 1))
            if measured:
                line["input_GBps"] = round(total / line["kernel_ms_median"] / 1e6, 1)
            medians[(name, kind)] = line
            print(json.dumps(line), flush=True)
        if len(named) > 1 and ("parent", kind) in medians:
            a, b = medians[("new", kind)], medians[("parent", kind)]
            assert all(a[f] == b[f] for f in ("corrected", "uncorrectable", "out_len", "out_blake2b")), (a, b)
            if a["kernel_ms_median"] is not None and b["kernel_ms_median"] is not None:
                print(json.dumps(dict(profile=kind, new_ms=a["kernel_ms_median"], parent_ms=b["kernel_ms_median"],
                                      parent_spread_ms=b["kernel_ms_spread"],
                                      ratio_new_over_parent=round(a["kernel_ms_median"] / b["kernel_ms_median"], 4))),
                      flush=True)
            else:
                print(json.dumps(dict(profile=kind, ratio_new_over_parent=None, note="kernel times unmeasured")), flush=True)
        del enc


if __name__ == "__main__":
    main()
