"""GPU tier: the hand-off between the deep engine's committer and its scan helpers (job down, packed scan records
back) at 1, 7 and 63 helpers, on the smallest inputs at which a batch reaches MRZ_DEEP_HELP_MIN lanes, culls run and
records with tag-equal entries travel; every case against the oracle, the whole table included."""
import pytest

import modern_rzip_amd as m
from modern_rzip_amd import workloads as w
from tests import _parity, _util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deep_mix():
    """The recipe of test_emulated_kernels._deep_mix: at level 1 and victim_round 1 the oracle reaches min_mask 31 with
    72 matches."""
    noise = _util.xorshift_noise(2600000, seed=3)
    return noise + _util.zipf_text(420000, seed=4) + noise[300000:420000] + _util.xorshift_noise(150000, seed=8)


@pytest.fixture(scope="module")
def short_period():
    return _util.rep64k(40, seed=9, period=997)


@pytest.mark.parametrize("scanners", ["1", "7", "63"])
def test_level1_mix_through_helpers(gpu_lib, oracle, deep_mix, scanners, monkeypatch):
    monkeypatch.setenv("MRZ_SEQ_ENGINE", "deep")
    monkeypatch.setenv("MRZ_DEEP_SCANNERS", scanners)
    want = _parity.check_chunk(gpu_lib, oracle, deep_mix, level=1, table=True, victim_round=1)
    assert want["min_mask"] == 31 and want["stats"]["matches"] == 72


@pytest.mark.parametrize("scanners", ["1", "7", "63"])
def test_level2_chains_through_helpers(gpu_lib, oracle, short_period, scanners, monkeypatch):
    monkeypatch.setenv("MRZ_SEQ_ENGINE", "deep")
    monkeypatch.setenv("MRZ_DEEP_SCANNERS", scanners)
    _parity.check_chunk(gpu_lib, oracle, short_period, level=2, table=True)


def test_level7_with_the_hosts_own_engine_choice(gpu_lib, oracle, monkeypatch):
    monkeypatch.setenv("MRZ_DEEP_MIN_BITS", "3")
    data = w.noise(48 << 20, seed=21) + w.tar_like_fast(16 << 20, seed=22, pool_bytes=4 << 20)
    want = oracle.rzip_chunk(data, level=7, want_table=True)
    with m.RzipContext(level=7, lib=gpu_lib, max_chunk=len(data)) as ctx:
        res, s0, s1 = ctx.rzip_chunk(data)
        assert (s0, s1) == (want["s0"], want["s1"]) and res.stats.as_dict() == want["stats"] and res.crc32 == want["crc"]
        assert res.min_mask == want["min_mask"] and res.hash_count == want["hash_count"]
        assert ctx.fetch_table() == want["table"]
        t = ctx.timings()
        assert 1 <= t.n_deep < t.n_segments
