"""GPU tier: the deep engine's walk (mrz_deep_scan: the next group's loads ahead of the fold, quiet groups passed with one
ballot) at the smallest shape where quiet groups exist on the device.  Level 1 has a 2 MiB table, so 192 MiB of input
reach 11 mask bits: runs of about 1,365 slots, nearly three groups of 8 blocks.  Both inputs against the oracle, the whole
table included; the oracle's answer is computed once per input."""
import numpy as np
import pytest

import modern_rzip_amd as m
from modern_rzip_amd import workloads
from tests import _parity, _util

pytestmark = pytest.mark.gpu

HEAD = 176 << 20


@pytest.fixture(scope="module")
def head():
    return workloads.noise(HEAD, seed=42)


@pytest.fixture(scope="module")
def sparse_matches(head, oracle):
    """176 MiB of noise, then 1024 x (8 KiB of it from anywhere, 8 KiB of fresh noise): 192 MiB, few matches, long quiet
    runs.  The oracle: 11 bits, 997 matches, 1004 tag hits."""
    at = np.random.default_rng(41).integers(0, HEAD - 8192, size=1024)
    fresh = workloads.noise(1024 * 8192, seed=43)
    data = head + b"".join(head[int(a):int(a) + 8192] + fresh[k * 8192:(k + 1) * 8192] for k, a in enumerate(at))
    assert len(data) == 192 << 20
    return data, oracle.rzip_chunk(data, level=1, want_table=True)


@pytest.fixture(scope="module")
def chains_at_the_limit(head, oracle):
    """The same head, then a text block of 997 bytes 8000 times over and 8 MiB of noise: chains at max_chain and evictions
    inside long runs.  The oracle: 11 bits, 7,751 matches, 15,503 tag hits, victim_round ends at 1."""
    data = head + _util.rep64k(8000, seed=9, period=997) + workloads.noise(8 << 20, seed=44)
    return data, oracle.rzip_chunk(data, level=1, want_table=True)


def _check(lib, data, want):
    """_parity.check_chunk's body on an answer the oracle has given already; returns the launch counters."""
    with m.RzipContext(level=1, max_chunk=len(data), lib=lib) as ctx:
        res, s0, s1 = ctx.rzip_chunk(data)
        assert res.crc32 == want["crc"]
        assert res.stats.as_dict() == want["stats"]
        assert ctx.victim_round == want["victim_round"]
        assert res.min_mask == want["min_mask"]
        assert res.hash_count == want["hash_count"]
        assert s1 == want["s1"]
        assert s0 == want["s0"]
        assert ctx.fetch_table() == want["table"]
        t = ctx.timings()
        _parity.check_runzip(ctx, data, want["s0"], want["s1"])
    return t


@pytest.mark.parametrize("scanners", ["0", "63"])
def test_quiet_runs_at_11_bits(gpu_lib, sparse_matches, scanners, monkeypatch):
    monkeypatch.setenv("MRZ_DEEP_SCANNERS", scanners)
    monkeypatch.setenv("MRZ_DEEP_MIN_BITS", "3")  # (the host's own engine choice)
    data, want = sparse_matches
    assert bin(want["min_mask"]).count("1") >= 11 and want["stats"]["matches"] >= 900
    assert _check(gpu_lib, data, want).n_deep >= 1


def test_chains_at_the_limit_at_11_bits(gpu_lib, chains_at_the_limit, monkeypatch):
    monkeypatch.setenv("MRZ_DEEP_MIN_BITS", "3")
    data, want = chains_at_the_limit
    st = want["stats"]
    assert bin(want["min_mask"]).count("1") >= 11 and st["tag_hits"] >= 2 * st["matches"] - 100 and want["victim_round"] == 1
    assert _check(gpu_lib, data, want).n_deep >= 1
