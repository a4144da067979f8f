"""mrz_rs_decode_ex on the GPU: the cooperative repair kernel (one wave per damaged codeword), device output and the
status of every codeword against the reference's own rsd32 / gather (tests/golden/rs_repair.json)."""
import numpy as np
import pytest

import modern_rzip_amd as m
from tests import _rs_repair as R
from tests.golden import make_rs_repair_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    with m.RzipContext(lib=gpu_lib) as c:
        yield c


@pytest.fixture(scope="module")
def cases(oracle):
    return G.cases(oracle)


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


def test_whole_bursts_at_the_limit(decoded, cases):
    """Case B: a contiguous run of 16 x 8176 bytes, a burst whose every codeword has 16 errors, 4096 codewords lost."""
    got, rep, status = decoded["B"]
    assert rep["uncorrectable"] == 4096 and rep["checksum_ok"] is False
    assert (status[:2 * G.ROWS] == 16).all() and (status[2 * G.ROWS:2 * G.ROWS + 4096] == -1).all()
    assert not status[2 * G.ROWS + 4096:].any()
    R.check_rows_round_trip(cases["B"]["data"], got, status)


def test_trailer_missing(decoded):
    """Case C: nothing is stripped, the statuses are those of case A."""
    got, rep, status = decoded["C"]
    assert rep["truncated"] is True and len(got) == G.BURST_IN
    assert (status == decoded["A"][2]).all()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_old_entry_point_agrees(ctx, cases, decoded, name):
    got, rep, _ = decoded[name]
    R.check_old_entry(ctx, cases[name]["enc"], got, rep)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_in_device_out(ctx, cases, decoded, name):
    import torch
    got, rep, status = decoded[name]
    enc = cases[name]["enc"]
    d_in = torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda()
    d_out = torch.zeros((len(enc) // G.BURST) * G.BURST_IN, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(status),), 99, dtype=torch.int32, device="cuda")
    none, rep2, st = ctx.rs_decode_ex(d_in, out=d_out, status=d_status)
    assert none is None and st is d_status
    assert rep2.pop("out_len") == len(got) and rep2 == rep
    assert d_out[:len(got)].cpu().numpy().tobytes() == got
    assert (d_status.cpu().numpy() == status).all()


def test_skip_checksum(ctx, cases, decoded):
    import torch
    got, rep, status = decoded["B"]
    enc = cases["B"]["enc"]
    got2, rep2, status2 = ctx.rs_decode_ex(enc, skip_checksum=True)
    assert rep2.pop("checksum_ok") == -1
    assert rep2 == {k: v for k, v in rep.items() if k != "checksum_ok"}
    assert got2 == got and (status2 == status).all()
    d_out = torch.zeros(3 * G.BURST_IN, dtype=torch.uint8, device="cuda")  # device output: nothing is hashed at all
    _, rep3, status3 = ctx.rs_decode_ex(enc, out=d_out, skip_checksum=True)
    assert rep3["checksum_ok"] == -1 and rep3["out_len"] == len(got) and (status3 == status).all()
    assert d_out[:len(got)].cpu().numpy().tobytes() == got


def test_status_not_asked_for(ctx, cases, decoded):
    got, rep, _ = decoded["A"]
    got2, rep2, none = ctx.rs_decode_ex(cases["A"]["enc"], status=False)
    assert none is None and got2 == got and rep2 == rep


def test_arguments(ctx, cases, gpu_lib):
    R.check_out_cap(ctx, cases["A"]["enc"])
    R.check_codewords(gpu_lib)


def test_undamaged_input(ctx, oracle):
    R.check_undamaged(ctx, *R.undamaged_three_bursts(oracle))
