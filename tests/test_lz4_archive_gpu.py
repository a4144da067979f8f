"""LZ4 archives on the MI355X: mrz_runzip_buffer over -n archives whose blocks were rewritten as CTYPE_LZ4
(tests/_lz4_blocks.reframe: payloads from the oracle's liblz4 restatement), refusals, and the -l writer
mrz_rzip_buffer_lz4 against an independent parse.  The checks are those of tests/_lz4_checks.py."""
import pytest

import modern_rzip_amd as m
from tests import _lz4_checks as C
from tests import _util

pytestmark = pytest.mark.gpu


LIB = "gpu_lib"


@pytest.fixture(scope="module")
def lib(request):
    return request.getfixturevalue(LIB)


@pytest.mark.parametrize("name", sorted(C.archive_inputs(True)))
def test_reframed(lib, oracle, name):
    C.check_reframed(lib, oracle, C.archive_inputs(True)[name])


def test_reframed_multi_chunk(lib, oracle):
    data = _util.rep64k(6, seed=13, period=4096)
    arc = C.check_reframed(lib, oracle, data, ramsize=C.MULTI_CHUNK_RAM)
    assert len(C.B.parse_mrz(arc)["chunks"]) > 1


def test_expanding_block(lib, oracle):
    C.check_expanding(lib, oracle)


def test_errors(lib, oracle):
    C.check_archive_errors(lib, oracle)


@pytest.mark.parametrize("name", ["empty", "range30", "a1000", "seed42x64", "text"])
def test_writer(lib, oracle, name):
    C.check_writer(lib, oracle, C.archive_inputs(False)[name])


def test_writer_threads_and_small_ram(lib, oracle):
    """ramsize / 6 = 8 KiB per block (the -n path has ramsize / 3), several chunks; -p4 against -p1"""
    data = _util.zipf_text(100000, seed=9)
    got = C.check_writer(lib, oracle, data, threads=4, ramsize=6 * 8192)
    assert C.lz4_block_size(len(data), 6 * 8192, 4) == 8192 and len(got["chunks"]) > 1
    C.check_writer(lib, oracle, data, threads=1, ramsize=6 * 8192)
    assert C.lz4_block_size(300 << 20, 60 << 30, 4) == 60 << 20 and C.lz4_block_size(300 << 20, 60 << 30, 1) == 300 << 20


def test_writer_refuses_hc(lib):
    for level in (3, 7):
        assert C.rc_of(m.rzip_buffer_lz4, b"x" * 100, level=level, lib=lib) == C.B.E_UNSUPPORTED
    assert C.rc_of(m.rzip_buffer_lz4, b"x" * 100, level=1, lib=lib) == 0


def test_two_real_blocks(gpu_lib, oracle):
    """11 MiB of noise, its streams cut at the 10 MiB floor of the -l block size: stream 1 is two blocks of real size
    (10 MiB and 1 MiB), both expanding"""
    from tests import _util
    data = _util.xorshift_noise(11 << 20, seed=5)
    arc = C.B.reframe(oracle.compress(data)[0], oracle, block_size=10 << 20)
    lits = [b for b in C.B.parse_mrz(arc)["chunks"][0]["blocks"] if b["stream"] == 1]
    assert [b["u_len"] for b in lits] == [10 << 20, 1 << 20]
    assert all(b["ctype"] == 5 and b["c_len"] > b["u_len"] for b in lits)
    assert m.runzip_buffer(arc, lib=gpu_lib) == data
