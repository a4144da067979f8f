"""mrz_runzip_ranges / mrz_runzip_origins_multi on the MI355X: tests/_ranges_checks.py."""
import pytest

import modern_rzip_amd as m
from tests import _ranges_checks as C

pytestmark = pytest.mark.gpu

EMU = False


@pytest.fixture(scope="module")
def lib(gpu_lib):
    return gpu_lib


@pytest.fixture(scope="module")
def ctx(lib):
    with m.RzipContext(level=7, max_chunk=64, lib=lib) as c:
        yield c


def test_abi_unchanged(lib):
    C.check_abi(lib)


@pytest.mark.parametrize("where", [(0, 0), (1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("name", C.CASES)
def test_range_lists(ctx, name, where):
    C.check_lists(ctx, EMU, name, *where)


def test_binding(ctx):
    C.check_binding(ctx, "short_cb3")


def test_a_bad_range_at_each_position(ctx):
    C.check_bad_ranges(ctx, EMU, "short_cb3")


def test_nothing_asked_for(ctx):
    C.check_empty(ctx, EMU, "overlap8k")


def test_refused_streams(ctx):
    C.check_corrupt(ctx, EMU)
