"""mrz_rs_decode_ex on the wave64 emulator: the cooperative repair kernel (one wave per damaged codeword) and the
status of every codeword against the reference's own rsd32 / gather (tests/golden/rs_repair.json)."""
import ctypes

import numpy as np
import pytest

import modern_rzip_amd as m
from tests import _rs_repair as R
from tests.golden import make_rs_repair_golden as G


@pytest.fixture(scope="module")
def ctx(emu_lib):
    with m.RzipContext(lib=emu_lib) as c:
        yield c


@pytest.fixture(scope="module")
def cases(oracle):
    return G.cases(oracle, names=("A", "C"))


@pytest.fixture(scope="module")
def decoded(ctx, cases):
    """name -> (bytes, report, status) of rs_decode_ex, compared with the reference on the way"""
    return {name: R.decode_and_compare(ctx, c["enc"]) for name, c in cases.items()}


def test_every_lane_every_count(decoded, cases):
    """Case A: all lanes of two whole tiles and of the short last tile, 0..18 errors per codeword."""
    got, rep, status = decoded["A"]
    assert set(np.unique(status).tolist()) == set(range(-1, 17))
    assert rep["checksum_ok"] is False and rep["uncorrectable"] == int((status == -1).sum())
    R.check_rows_round_trip(cases["A"]["data"], got, status)


def test_trailer_missing(decoded):
    """Case C: nothing is stripped, the statuses are those of case A."""
    got, rep, status = decoded["C"]
    assert rep["truncated"] is True and len(got) == G.BURST_IN
    assert (status == decoded["A"][2]).all()


@pytest.mark.parametrize("name", ["A", "C"])
def test_old_entry_point_agrees(ctx, cases, decoded, name):
    got, rep, _ = decoded[name]
    R.check_old_entry(ctx, cases[name]["enc"], got, rep)


def test_skip_checksum(ctx, cases, decoded):
    got, rep, status = decoded["A"]
    got2, rep2, status2 = ctx.rs_decode_ex(cases["A"]["enc"], skip_checksum=True)
    assert rep2.pop("checksum_ok") == -1
    assert rep2 == {k: v for k, v in rep.items() if k != "checksum_ok"}
    assert got2 == got and (status2 == status).all()


def test_status_not_asked_for_and_device_side_buffers(ctx, cases, decoded):
    """row_status = NULL is accepted; output and status in the ctx's memory space (the emulator's is the host's)."""
    got, rep, status = decoded["A"]
    enc = cases["A"]["enc"]
    got2, rep2, none = ctx.rs_decode_ex(enc, status=False)
    assert none is None and got2 == got and rep2 == rep
    out = ctypes.create_string_buffer(G.BURST_IN)
    st = np.full(G.ROWS, 99, dtype=np.int32)
    src = ctypes.create_string_buffer(enc, len(enc))
    _, rep3, _ = ctx.rs_decode_ex((ctypes.addressof(src), len(enc)), out=(ctypes.addressof(out), G.BURST_IN),
                                  status=(st.ctypes.data, st.nbytes))
    assert rep3.pop("out_len") == len(got) and rep3 == rep
    assert out.raw[:len(got)] == got and (st == status).all()


def test_arguments(ctx, cases, emu_lib):
    R.check_out_cap(ctx, cases["A"]["enc"])
    R.check_codewords(emu_lib)


def test_undamaged_input(ctx, oracle):
    R.check_undamaged(ctx, *R.undamaged_three_bursts(oracle))
