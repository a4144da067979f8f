"""mrz_copy_device_batch on the wave64 emulator: tests/_segcopy_checks.py.  The emulator's grid is 16 workgroups, so every
call with more than 16 tiles also runs the kernel's loop over tiles."""
import pytest

import modern_rzip_amd as m
from tests import _segcopy_checks as S

EMU = True


@pytest.fixture(scope="module")
def lib(emu_lib):
    return emu_lib


@pytest.fixture(scope="module")
def ctx(lib):
    with m.RzipContext(level=7, max_chunk=64, lib=lib) as c:
        yield c


def test_abi_unchanged(lib):
    S.check_abi(lib)


@pytest.mark.parametrize("mis", [(0, 0), (5, 5), (16, 4), (3, 11), (1, 2)])
def test_lengths(ctx, mis):
    S.check_lengths(ctx, EMU, *mis)


def test_every_pair_of_misalignments(ctx):
    S.check_misalignments(ctx, EMU)


def test_shared_and_overlapping_sources(ctx):
    S.check_shared_source(ctx, EMU)


def test_many_small_segments(ctx):
    S.check_many_segments(ctx, EMU)


def test_arguments(ctx):
    S.check_arguments(ctx, EMU)
