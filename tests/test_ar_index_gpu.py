"""The ar-mrzip index (mrz_tlsh_batch, mrz_ar_order, mrz_ar_create / parse / verify) on the MI355X: the checks of
tests/_ar_checks.py.  TLSH: the reference library's strings for five kinds of input at 22 lengths, at three segment
lengths, host and device memory; one 8 MiB member; a batch of 300 members of mixed sizes; the length code at every
threshold up to 1 MiB.  Order: the hand-made cases and 700 digests (three workgroups a step) against tests/_ar_ref.py.
Archives: bit-identical to tests/_ar_ref.py for host and device inputs and outputs, round trip, verification,
refusals."""
import pytest

import modern_rzip_amd as m
from tests import _ar_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    with m.RzipContext(lib=gpu_lib) as c:
        yield c


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("segment_len", [0, 64, 256])
def test_tlsh_small(ctx, segment_len, where):
    C.check_small(ctx, False, segment_len, where)


def test_tlsh_big_member(ctx):
    C.check_big_member(ctx, False)


def test_tlsh_mixed_batch(ctx):
    C.check_mixed_batch(ctx, False)


def test_tlsh_length_thresholds(ctx):
    C.check_thresholds(ctx, 1 << 20)


def test_tlsh_length_code_host(gpu_lib):
    C.check_length_code(gpu_lib)


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
    C.check_create(ctx, False, where, out_where)


def test_parse_roundtrip_and_verify(ctx):
    C.check_roundtrip(ctx, False)


def test_verify_names_the_member(ctx):
    C.check_verify_names_the_member(ctx, False)


def test_corrupt_archives(ctx):
    C.check_corrupt(ctx, False)


def test_create_arguments(ctx):
    C.check_create_args(ctx)
