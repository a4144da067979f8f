"""Range decode over LZ4 archives on the MI355X: mrz_lz4_decompress_prefix_batch against the Python reference of the
prefix contract (tests/_lz4_prefix.py; tests/test_lz4_range_emu.py pins that reference to liblz4's verdicts) and
mrz_runzip_buffer_range_ex over re-framed archives with exact accounting (tests/_lz4_range_checks.py)."""
import pytest

import modern_rzip_amd as m
from tests import _lz4_prefix as P
from tests import _lz4_range_checks as R

pytestmark = pytest.mark.gpu

EMU = False


@pytest.fixture(scope="module")
def lib(gpu_lib):
    return gpu_lib


@pytest.fixture(scope="module")
def ctx(lib):
    with m.RzipContext(lib=lib) as c:
        yield c


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("group", P.GROUPS)
def test_prefix(ctx, group, where):
    P.check_prefix(ctx, EMU, where, group)


def test_prefix_arguments(ctx):
    P.check_prefix_args(ctx)


def test_abi_unchanged(lib):
    assert lib.mrz_abi_version() == 4
    assert hasattr(lib, "mrz_lz4_decompress_prefix_batch") and hasattr(lib, "mrz_runzip_buffer_range_ex")


@pytest.mark.parametrize("framing", R.FRAMINGS)
@pytest.mark.parametrize("name", R.ARCHIVES)
def test_archive_ranges(lib, ctx, oracle, name, framing):
    R.check_archive(lib, ctx, oracle, EMU, name, framing)


def test_one_byte_and_outside_chunks(lib, ctx, oracle):
    R.check_one_byte(lib, ctx, oracle)


def test_refusals(lib, oracle):
    R.check_refusals(lib, oracle)
