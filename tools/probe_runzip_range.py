"""Range-decode probe (GPU box): encode a stream on the GPU and, with everything resident in HBM, time mrz_runzip_range
on a 1 MiB range at the end and in the middle of the chunk against mrz_runzip_chunk on the same streams in the same
process.  Per range: call time (best of 3 after a warm-up, host clock around the blocking call), total_hops, max_hops,
hops per second and the ratio range time / whole-decode time.  Cost follows total_hops: where matches copy matches many
times over (rep64k: depth = position / period) the range can lose to the whole decode, and the ratio says so.

usage: python tools/probe_runzip_range.py [tar] [text] [rep1g] [--out profiles/runzip_range/probe.jsonl]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import modern_rzip_amd as m  # noqa: E402
from modern_rzip_amd import workloads as w  # noqa: E402

RANGE = 1 << 20


def best(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), r


def run(name, t, sink):
    n = t.numel()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    piece = torch.empty(RANGE, dtype=torch.uint8, device="cuda")
    with m.RzipContext(level=7, max_chunk=n) as ctx:
        res, _, _ = ctx.rzip_chunk(t, fetch=False)
        cb = m.chunk_bytes(n)
        s0, s1 = (res.d_s0, res.s0_len), (res.d_s1, res.s1_len)
        whole_s, (_, got, cc, cs) = best(lambda: ctx.runzip_chunk(s0, s1, cb, n, out=out))
        ok_whole = got == n and cc == cs and bool(torch.equal(out, t))
        for where, first in (("end", n - RANGE), ("middle", (n // 2) & ~4095)):
            dt, (_, info) = best(lambda: ctx.runzip_range(s0, s1, cb, first, RANGE, out=piece))
            rec = {"name": name, "n": n, "s0": res.s0_len, "s1": res.s1_len, "range": where, "first": first, "count": RANGE,
                   "range_s": round(dt, 6), "whole_decode_s": round(whole_s, 6), "total_hops": info["total_hops"],
                   "max_hops": info["max_hops"], "hops_per_s": round(info["total_hops"] / dt, 1),
                   "range_over_whole": round(dt / whole_s, 4),
                   "ok": ok_whole and bool(torch.equal(piece, t[first:first + RANGE]))}
            line = json.dumps(rec)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
    del out, piece


def main(argv):
    path = None
    if "--out" in argv:
        k = argv.index("--out")
        path = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    which = argv or ["tar", "text", "rep1g"]
    sink = None
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        sink = open(path, "a")
    if "text" in which:
        run("synth_text-32MiB", w.synth_text_device(32 << 20, "cuda", 7, 11), sink)
    if "rep1g" in which:
        run("rep64k-1GiB", w.rep64k_device(16384, "cuda"), sink)
    if "tar" in which:
        run("synth_tar-1GiB", w.synth_tar_device(1 << 30, "cuda", 2026), sink)
    if sink:
        sink.close()


if __name__ == "__main__":
    main(sys.argv[1:])
