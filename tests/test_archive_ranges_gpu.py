"""mrz_runzip_buffer_ranges on the MI355X: tests/_arc_ranges_checks.py."""
import pytest

import modern_rzip_amd as m
from tests import _arc_ranges_checks as A

pytestmark = pytest.mark.gpu

EMU = False


@pytest.fixture(scope="module")
def lib(gpu_lib):
    return gpu_lib


@pytest.fixture(scope="module")
def ctx(lib):
    with m.RzipContext(lib=lib) as c:
        yield c


def test_abi_unchanged(lib):
    A.check_abi(lib)


@pytest.mark.parametrize("name,framing,with_size", A.VARIANTS)
def test_range_lists(lib, ctx, oracle, name, framing, with_size):
    A.check_archive(lib, ctx, oracle, EMU, name, framing, with_size)


def test_a_list_of_one_range_is_the_single_call(lib, oracle):
    A.check_single_is_the_old_call(lib, oracle)


def test_refusals(lib, oracle):
    A.check_refusals(lib, oracle)
