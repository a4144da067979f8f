"""mrz_rs_decode_lost on the GPU: the erasure-aware repair kernel (the caller's lost ranges become erased columns, the
erasure locator seeds Berlekamp-Massey), host and device buffers, against the reference's own rsd32 with eras_pos /
no_eras (tests/golden/rs_erasure.json)."""
import numpy as np
import pytest

import modern_rzip_amd as m
from tests import _rs_erasure as E
from tests.golden import make_rs_erasure_golden as G
from tests.golden.make_rs_repair_golden import BURST, BURST_IN, ROWS

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
    """name -> (bytes, report, status) of rs_decode_lost, compared with the reference on the way"""
    return {name: E.decode_and_compare(ctx, c) for name, c in cases.items()}


def test_every_mix_of_erasures_and_errors(decoded):
    """Case L1: e erasures and t errors up to one error beyond e + 2 t <= 32, 33 and 34 erasures, intact erasures."""
    E.check_l1(*decoded["L1"])


def test_contiguous_runs(decoded, cases):
    """Case L2: 24,528 listed codewords (the repair grid's waves stride); runs of 32 columns, of 33 in 4000 rows, of 24
    with 4 errors in every row; a range across the seam of two bursts and one over the trailer."""
    got, rep, status = decoded["L2"]
    assert (status[:ROWS] == 32).all()
    assert (status[ROWS:ROWS + 4000] == -1).all() and (status[ROWS + 4000:2 * ROWS] == 32).all()
    assert (status[2 * ROWS:] == 28).all()
    assert rep["uncorrectable"] == 4000 and rep["checksum_ok"] is False and rep["truncated"] is False
    E.check_rows_restored(cases["L2"]["data"], got, status)


def test_trailer_missing(decoded):
    """Case L3: nothing is stripped, the statuses are those of L1."""
    got, rep, status = decoded["L3"]
    assert rep["truncated"] is True and len(got) == BURST_IN
    assert (status == decoded["L1"][2]).all()


def test_lost_run_of_32_columns(ctx, cases):
    """Burst 0 of case L2: restored with the run declared, -1 in every row without."""
    E.check_hints_double_the_reach(ctx, *E.l2_burst0(cases["L2"]))


def test_no_ranges_is_decode_ex(ctx, oracle):
    E.check_no_ranges_is_decode_ex(ctx, oracle)


@pytest.mark.parametrize("name", ["L1", "L2", "L3"])
def test_device_in_device_out(ctx, cases, decoded, name):
    import torch
    got, rep, status = decoded[name]
    enc = cases[name]["enc"]
    d_in = torch.frombuffer(bytearray(enc), dtype=torch.uint8).cuda()
    d_out = torch.zeros((len(enc) // BURST) * BURST_IN, dtype=torch.uint8, device="cuda")
    d_status = torch.full((len(status),), 99, dtype=torch.int32, device="cuda")
    none, rep2, st = ctx.rs_decode_lost(d_in, cases[name]["lost"], out=d_out, status=d_status)
    assert none is None and st is d_status
    assert rep2.pop("out_len") == len(got) and rep2 == rep
    assert d_out[:len(got)].cpu().numpy().tobytes() == got
    assert (d_status.cpu().numpy() == status).all()


def test_mixed_memory_spaces(ctx, cases, decoded):
    """device input with host output and status; host input with device output and host status"""
    import torch
    got, rep, status = decoded["L1"]
    c = cases["L1"]
    d_in = torch.frombuffer(bytearray(c["enc"]), dtype=torch.uint8).cuda()
    got2, rep2, status2 = ctx.rs_decode_lost(d_in, c["lost"])
    assert got2 == got and rep2 == rep and (status2 == status).all()
    d_out = torch.zeros(BURST_IN, dtype=torch.uint8, device="cuda")
    _, rep3, status3 = ctx.rs_decode_lost(c["enc"], c["lost"], out=d_out)
    assert rep3.pop("out_len") == len(got) and rep3 == rep and (status3 == status).all()
    assert d_out[:len(got)].cpu().numpy().tobytes() == got


def test_skip_checksum(ctx, cases, decoded):
    import torch
    got, rep, status = decoded["L2"]
    c = cases["L2"]
    got2, rep2, status2 = ctx.rs_decode_lost(c["enc"], c["lost"], skip_checksum=True)
    assert rep2.pop("checksum_ok") == -1
    assert rep2 == {k: v for k, v in rep.items() if k != "checksum_ok"}
    assert got2 == got and (status2 == status).all()
    d_out = torch.zeros(3 * BURST_IN, dtype=torch.uint8, device="cuda")  # device output: nothing is hashed at all
    _, rep3, status3 = ctx.rs_decode_lost(c["enc"], c["lost"], out=d_out, skip_checksum=True)
    assert rep3["checksum_ok"] == -1 and rep3["out_len"] == len(got) and (status3 == status).all()
    assert d_out[:len(got)].cpu().numpy().tobytes() == got


def test_status_not_asked_for(ctx, cases, decoded):
    got, rep, _ = decoded["L1"]
    got2, rep2, none = ctx.rs_decode_lost(cases["L1"]["enc"], cases["L1"]["lost"], status=False)
    assert none is None and got2 == got and rep2 == rep


def test_ranges_are_those_of_the_call(ctx, cases, decoded):
    """one ctx, calls with different range lists in turn: a long list, a short one, the long one again, none"""
    for name in ("L1", "L2", "L1"):
        got, rep, status = E.decode_and_compare(ctx, cases[name])
        assert got == decoded[name][0] and (status == decoded[name][2]).all()
    _, rep0, status0 = ctx.rs_decode_lost(cases["L2"]["enc"], [])  # no hints: every run is beyond 16 errors
    assert (status0[:2 * ROWS] == -1).all() and rep0["uncorrectable"] >= 2 * ROWS
    got, rep, status = E.decode_and_compare(ctx, cases["L2"])
    assert (status == decoded["L2"][2]).all()


def test_arguments(ctx, cases):
    E.check_arguments(ctx, cases["L1"]["enc"])
