"""Generates tests/golden/runzip_records.json: for every named case of tests/_records.py its parameters and the sha256 of
stream 0, stream 1 and the output -- hashes only, no streams.  tests/test_runzip_records_emu.py regenerates every case
and compares, so a generator that drifts is caught instead of silently changing what the GPU tier tests.
Run:  python tests/golden/make_runzip_records.py   (after a deliberate change to a generator or a seed)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _records as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "runzip_records.json")


def main():
    rec = {"_source": "tests/_records.py: fingerprint() of every entry of golden_names(); build()'s output agrees with "
                      "decode_ref() and the oracle's decoder (tests/test_runzip_records_emu.py)",
           "cases": {}}
    for name in R.case_names():
        c = R.case(name)
        if c is not None:
            want = R.decode_ref(c["s0"], c["s1"], c["cb"], len(c["out"]))
            assert want[0] == "ok" and want[1] == c["out"], name
    for name in R.golden_names():
        rec["cases"][name] = R.fingerprint(name)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
