"""mrz_rs_decode_lost on the wave64 emulator: the erasure-aware repair kernel (the caller's lost ranges become erased
columns, the erasure locator seeds Berlekamp-Massey) against the reference's own rsd32 with eras_pos / no_eras
(tests/golden/rs_erasure.json)."""
import ctypes

import numpy as np
import pytest

import modern_rzip_amd as m
from tests import _rs_erasure as E
from tests.golden import make_rs_erasure_golden as G
from tests.golden.make_rs_repair_golden import BURST_IN, ROWS


@pytest.fixture(scope="module")
def ctx(emu_lib):
    with m.RzipContext(lib=emu_lib) as c:
        yield c


@pytest.fixture(scope="module")
def cases(oracle):
    return G.cases(oracle, names=("L1", "L3"))


@pytest.fixture(scope="module")
def decoded(ctx, cases):
    """name -> (bytes, report, status) of rs_decode_lost, compared with the reference on the way"""
    return {name: E.decode_and_compare(ctx, c) for name, c in cases.items()}


def test_every_mix_of_erasures_and_errors(decoded):
    """Case L1: e erasures and t errors up to one error beyond e + 2 t <= 32, 33 and 34 erasures, intact erasures."""
    E.check_l1(*decoded["L1"])


def test_trailer_missing(decoded):
    """Case L3: nothing is stripped, the statuses are those of L1."""
    got, rep, status = decoded["L3"]
    assert rep["truncated"] is True and len(got) == BURST_IN
    assert (status == decoded["L1"][2]).all()


def test_lost_run_of_32_columns(ctx, oracle):
    """Burst 0 of case L2, its run zero-filled in two whole tiles, around the row where the run moves on by a column, and
    in the short last tile: what the decoder without hints loses in every such row."""
    rows = list(range(256)) + list(range(4990, 5010)) + list(range(ROWS - 112, ROWS))
    E.check_hints_double_the_reach(ctx, *E.l2_burst0(G.cases(oracle, names=("L2",))["L2"], oracle, rows))


def test_no_ranges_is_decode_ex(ctx, oracle):
    E.check_no_ranges_is_decode_ex(ctx, oracle)


def test_skip_checksum_and_no_status(ctx, cases, decoded):
    got, rep, status = decoded["L1"]
    c = cases["L1"]
    got2, rep2, none = ctx.rs_decode_lost(c["enc"], c["lost"], status=False, skip_checksum=True)
    assert none is None and rep2.pop("checksum_ok") == -1
    assert rep2 == {k: v for k, v in rep.items() if k != "checksum_ok"} and got2 == got


def test_buffers_in_the_ctx_memory_space(ctx, cases, decoded):
    """output and status where the ctx keeps its memory (the emulator's is the host's)"""
    got, rep, status = decoded["L1"]
    c = cases["L1"]
    out = ctypes.create_string_buffer(BURST_IN)
    st = np.full(ROWS, 99, dtype=np.int32)
    src = ctypes.create_string_buffer(c["enc"], len(c["enc"]))
    _, rep2, _ = ctx.rs_decode_lost((ctypes.addressof(src), len(c["enc"])), c["lost"],
                                    out=(ctypes.addressof(out), BURST_IN), status=(st.ctypes.data, st.nbytes))
    assert rep2.pop("out_len") == len(got) and rep2 == rep
    assert out.raw[:len(got)] == got and (st == status).all()


def test_arguments(ctx, cases):
    E.check_arguments(ctx, cases["L1"]["enc"])
