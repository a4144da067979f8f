"""The C ABI after the LZ4 block codec: still version 4, three new symbols, mrz_lz4_bound's values (libmrzgpu.so)."""
import pytest

from tests import _lz4_checks as C

pytestmark = pytest.mark.gpu


def test_abi(gpu_lib):
    C.check_abi(gpu_lib)
