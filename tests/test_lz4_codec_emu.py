"""The LZ4 block codec (mrz_lz4_compress_batch / mrz_lz4_decompress_batch) on the wave64 emulator: the checks of
tests/_lz4_checks.py.  Compressor: return value and bytes of liblz4 1.9.3 (through the oracle's restatement) for every
input of lz4_sizes.json, the smallest inputs and the token-field boundaries, at five capacities each, canaries behind
every capacity, host and device memory.  Decoder: hand-built blocks, LZ4_compress_HC payloads, the compressor's own
output, malformed blocks among good ones, 2000 single-bit mutations against liblz4's recorded verdicts."""
import pytest

import modern_rzip_amd as m
from tests import _lz4_checks as C

@pytest.fixture(scope="module")
def ctx(emu_lib):
    with m.RzipContext(lib=emu_lib) as c:
        yield c


def test_boundary_inputs_are_boundaries(oracle):
    C.check_boundary_inputs(oracle)


@pytest.mark.parametrize("kind", C.CAP_KINDS)
def test_compress(ctx, oracle, kind):
    C.check_compress(ctx, oracle, True, kind)


@pytest.mark.parametrize("where", ["host", "device"])
def test_decode_handmade(ctx, where):
    C.check_handmade(ctx, True, where)


def test_decode_hc_payloads(ctx):
    C.check_hc(ctx, True)


@pytest.mark.parametrize("where", ["host", "device"])
def test_decode_rejects(ctx, where):
    C.check_rejects(ctx, True, where)


@pytest.mark.parametrize("where", ["host", "device"])
def test_decode_fuzz(ctx, where):
    C.check_fuzz(ctx, True, where)


def test_arguments(ctx):
    C.check_args(ctx)
