"""The C ABI after the LZ4 block codec: still version 4, three new symbols, mrz_lz4_bound's values (emulator build)."""
from tests import _lz4_checks as C


def test_abi(emu_lib):
    C.check_abi(emu_lib)
