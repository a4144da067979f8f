"""Generates tests/golden/synth_streams.json: sha256 of the host reference's reproducible streams
(modern_rzip_amd.workloads.synth_noise / synth_text / synth_tar, defined in include/mrzgpu_synth.h) at a handful of small
sizes, seeds and start offsets, odd lengths included, so that the definition cannot drift silently.
Run:  python tests/golden/make_synth_streams.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from modern_rzip_amd import workloads  # noqa: E402

CASES = [
    ("synth_noise", dict(nbytes=1, seed=0)),
    ("synth_noise", dict(nbytes=4096, seed=1)),
    ("synth_noise", dict(nbytes=1000003, seed=99)),
    ("synth_noise", dict(nbytes=65537, seed=99, start=7)),
    ("synth_noise", dict(nbytes=333, seed=2 ** 64 - 1, start=(1 << 40) + 5)),
    ("synth_text", dict(nbytes=1, seed=1, vocab_seed=2)),
    ("synth_text", dict(nbytes=100000, seed=1, vocab_seed=2)),
    ("synth_text", dict(nbytes=1500001, seed=7, vocab_seed=2)),
    ("synth_text", dict(nbytes=4 << 20, seed=2 ** 63 + 11, vocab_seed=0)),
    ("synth_tar", dict(nbytes=1 << 20, seed=5)),
    ("synth_tar", dict(nbytes=(16 << 20) + 13, seed=5)),
    ("synth_tar", dict(nbytes=777777, seed=5, start=(8 << 20) + 511)),
    ("synth_tar", dict(nbytes=(8 << 20) + 1, seed=2026)),
    ("synth_tar", dict(nbytes=4099, seed=2026, start=(1 << 30) + 3)),
]


def main():
    out = {"_source": "sha256 of modern_rzip_amd.workloads.<gen>(**args), made by tests/golden/make_synth_streams.py",
           "rnd": {"rnd(1,0,0)": int(workloads.synth_rnd(1, 0, 0)[0]),
                   "rnd(2^64-1,9,12345678901234)": int(workloads.synth_rnd(2 ** 64 - 1, 9, 12345678901234)[0]),
                   "zipf_total": int(workloads.synth_zipf_table()[-1])},
           "streams": []}
    for gen, args in CASES:
        data = getattr(workloads, gen)(**args)
        assert len(data) == args["nbytes"]
        out["streams"].append({"gen": gen, "args": args, "sha256": hashlib.sha256(data.tobytes()).hexdigest()})
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "synth_streams.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
