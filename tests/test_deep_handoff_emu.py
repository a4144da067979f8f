"""CPU tier: scan records with tag-equal entries crossing device memory between the deep engine's scan helpers and its
committer (the emulator's co-resident mode).  test_emulated_kernels.py feeds the helpers noise only, whose records carry
no entries; here the helper-scanned records hold chains up to and beyond MRZ_SMAX, culls, real matches and record
replay, and the whole table is compared with the oracle's."""
import pytest

from tests import _parity, _util


@pytest.fixture()
def deep_with_helpers(monkeypatch):
    monkeypatch.setenv("MRZ_EMU_CORESIDENT", "1")
    monkeypatch.setenv("MRZ_DEEP_SCANNERS", "2")
    monkeypatch.setenv("MRZ_SEQ_ENGINE", "deep")


def test_records_with_entries_at_the_chain_limit(emu_lib, oracle, deep_with_helpers):
    """A short period at level 2: chains at max_chain_len, nsame up to and beyond what a record holds."""
    want = _parity.check_chunk(emu_lib, oracle, _util.rep64k(40, seed=9, period=997), level=2, table=True)
    assert want["stats"]["tag_hits"] > 0


@pytest.mark.slow
def test_records_of_a_tar_like_mix(emu_lib, oracle, deep_with_helpers):
    """Level 1 (2 MiB table): culls, real matches and record replay, all from helper-scanned records."""
    want = _parity.check_chunk(emu_lib, oracle, _util.tar_like(1 << 19, seed=4), level=1, table=True)
    assert want["stats"]["matches"] == 11 and want["stats"]["tag_hits"] == 11 and want["min_mask"] == 15
