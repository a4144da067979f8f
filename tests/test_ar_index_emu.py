"""The ar-mrzip index (mrz_tlsh_batch, mrz_ar_order, mrz_ar_create / parse / verify) on the wave64 emulator: the checks
of tests/_ar_checks.py.  TLSH: the reference library's strings for five kinds of input at 22 lengths (around 50, 500,
4096 and around the segment lengths 64 and 256), at three segment lengths, host and device memory; the length code at
every threshold (through messages up to 64 KiB here -- the emulator walks every lane of every byte; the GPU tier goes
to 1 MiB -- and through the host function for all 170).  Order: the hand-made cases and 700 digests against
tests/_ar_ref.py.  Archives: bit-identical to tests/_ar_ref.py for host and device inputs and outputs, round trip,
verification, refusals."""
import pytest

import modern_rzip_amd as m
from tests import _ar_checks as C


@pytest.fixture(scope="module")
def ctx(emu_lib):
    with m.RzipContext(lib=emu_lib) as c:
        yield c


def test_reference_restatement_matches_the_fixture():
    C.check_ref_restatement()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("segment_len", [0, 64, 256])
def test_tlsh_small(ctx, segment_len, where):
    C.check_small(ctx, True, segment_len, where)


def test_tlsh_length_thresholds(ctx):
    C.check_thresholds(ctx, 1 << 16)


def test_tlsh_length_code_host(emu_lib):
    C.check_length_code(emu_lib)


def test_tlsh_arguments(ctx):
    C.check_tlsh_args(ctx)


@pytest.mark.parametrize("name", sorted(C.handmade_orders()))
def test_order_handmade(ctx, name):
    C.check_order_handmade(ctx, name)


def test_order_700(ctx):
    C.check_order_many(ctx)


@pytest.mark.parametrize("out_where", ["host", "device"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_create(ctx, where, out_where):
    C.check_create(ctx, True, where, out_where)


def test_parse_roundtrip_and_verify(ctx):
    C.check_roundtrip(ctx, True)


def test_verify_names_the_member(ctx):
    C.check_verify_names_the_member(ctx, True)


def test_corrupt_archives(ctx):
    C.check_corrupt(ctx, True)


def test_create_arguments(ctx):
    C.check_create_args(ctx)


def test_abi_symbols(emu_lib):
    lib = m.load_library()  # the product, as tests/test_abi.py loads it
    for name in ("mrz_tlsh_batch", "mrz_tlsh_length_code", "mrz_ar_order", "mrz_ar_create", "mrz_ar_parse",
                 "mrz_ar_verify"):
        assert hasattr(lib, name) and hasattr(emu_lib, name), name
    assert lib.mrz_abi_version() == 4 and emu_lib.mrz_abi_version() == 4
