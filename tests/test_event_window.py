"""The match list in pieces (mrz_set_event_capacity): a chunk that emits more matches than the device list holds is
encoded piece by piece -- the list is drained into the two streams whenever it runs short of room -- and the streams,
CRC, counters and final matcher state are still exactly the oracle's.  CPU tier on the emulator, GPU tier on gfx950.

Every test on a dense-match input checks that the run really drained: the oracle's match count is at least 4 x the
capacity, and timings().n_event_flushes >= 3."""
import ctypes
import random

import pytest

import modern_rzip_amd as m
from tests import _parity, _util

MRZ_E_ARG = -1
MRZ_E_STATE = -6


def phrases(nbytes, seed, vocab=200, lo=31, hi=40):
    """Dense matches: phrases of lo..hi random bytes drawn from a vocabulary of `vocab`, concatenated in seeded random
    order (one match per ~50 bytes once every phrase has been seen)."""
    r = random.Random(seed)
    words = [bytes(r.getrandbits(8) for _ in range(r.randint(lo, hi))) for _ in range(vocab)]
    out = bytearray()
    while len(out) < nbytes:
        out += r.choice(words)
    return bytes(out[:nbytes])


def check_capacity(lib, oracle, data, capacity, level=7, seg_positions=None, cand_cap=None, min_flushes=3,
                   min_matches=None):
    """_parity.check_chunk at a given list capacity: both streams, CRC, the seven counters, victim_round, mask,
    hash_count, table; the streams decode back.  Returns (oracle result, timings)."""
    want = oracle.rzip_chunk(data, level=level, want_table=True)
    assert want["stats"]["matches"] >= (4 * capacity if min_matches is None else min_matches)
    with m.RzipContext(level=level, max_chunk=len(data), lib=lib) as ctx:
        ctx.set_event_capacity(capacity)
        if seg_positions:
            ctx.set_segment_positions(seg_positions)
        if cand_cap:
            ctx.set_candidate_capacity(cand_cap)
        res, s0, s1 = ctx.rzip_chunk(data)
        t = ctx.timings()
        assert res.crc32 == want["crc"]
        assert res.stats.as_dict() == want["stats"]
        assert ctx.victim_round == want["victim_round"]
        assert res.min_mask == want["min_mask"]
        assert res.hash_count == want["hash_count"]
        assert s1 == want["s1"]
        assert s0 == want["s0"]
        assert ctx.fetch_table() == want["table"]
        assert t.n_event_flushes >= min_flushes
        _parity.check_runzip(ctx, data, s0, s1)
    return want, t


# ---- the progress hook through ctypes (the binding does not wrap it) ----
class Match(ctypes.Structure):
    _fields_ = [("p", ctypes.c_int64), ("ofs", ctypes.c_int64), ("len", ctypes.c_int64)]


PROGRESS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int)


def _declare_hook(lib):
    lib.mrz_set_progress.argtypes = [ctypes.c_void_p, PROGRESS_FN, ctypes.c_void_p]
    lib.mrz_fetch_events.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(Match)]


def matches_through_hook(lib, data, capacity):
    """Every match, fetched inside the progress hook as the chunk runs; plus the timings and what
    mrz_fetch_events(0, 1) returns after the chunk."""
    _declare_hook(lib)
    got, errors = [], []
    with m.RzipContext(level=7, max_chunk=len(data), lib=lib) as ctx:
        if capacity:
            ctx.set_event_capacity(capacity)

        def hook(user, n_events, last_match, done):
            k = n_events - len(got)
            if k > 0:
                buf = (Match * k)()
                rc = lib.mrz_fetch_events(ctx.ctx, len(got), k, buf)
                if rc:
                    errors.append(rc)
                    return 1
                got.extend((e.p, e.ofs, e.len) for e in buf)
            return 0

        cb = PROGRESS_FN(hook)
        assert lib.mrz_set_progress(ctx.ctx, cb, None) == 0
        res, _, _ = ctx.rzip_chunk(data)
        lib.mrz_set_progress(ctx.ctx, PROGRESS_FN(), None)
        one = (Match * 1)()
        after = lib.mrz_fetch_events(ctx.ctx, 0, 1, one)
        t = ctx.timings()
    assert not errors
    assert len(got) == res.n_events
    return got, t, after


def check_hook(lib, oracle, data, capacity):
    want = oracle.rzip_chunk(data, level=7)
    assert want["stats"]["matches"] >= 4 * capacity
    got, t, after = matches_through_hook(lib, data, capacity)
    assert t.n_event_flushes >= 3
    every, t0, _ = matches_through_hook(lib, data, 0)  # the default capacity: one piece
    assert t0.n_event_flushes == 0
    assert got == every
    assert after == MRZ_E_STATE  # the first match has left the list


def check_arguments(lib):
    with m.RzipContext(lib=lib) as ctx:
        for bad in (1, 1000, 1023, (1 << 31) + 1):
            assert lib.mrz_set_event_capacity(ctx.ctx, bad) == MRZ_E_ARG
            with pytest.raises(m.MrzError):
                ctx.set_event_capacity(bad)
        for ok in (1024, 4096, 1 << 31, 0, -1):
            assert lib.mrz_set_event_capacity(ctx.ctx, ok) == 0
        assert lib.mrz_set_event_capacity(None, 4096) == MRZ_E_ARG
        ctx.set_event_capacity(0)
        data = _util.zipf_text(20000, seed=2)
        res, s0, s1 = ctx.rzip_chunk(data)  # back at the default: one piece
        assert ctx.timings().n_event_flushes == 0


def check_window_of_one(lib, oracle, data, capacity):
    """Provider mode (the host drives the geometry; one rank scans for itself) at a small capacity."""
    from modern_rzip_amd import shard
    want = oracle.rzip_chunk(data, level=7)
    assert want["stats"]["matches"] >= 4 * capacity
    with m.RzipContext(level=7, max_chunk=len(data), lib=lib) as ctx:
        ctx.set_event_capacity(capacity)
        res, s0, s1 = shard.rzip_chunk_window(ctx, data, 0, len(data), 0, 1, None)
        assert (s0, s1) == (want["s0"], want["s1"])
        assert res.stats.as_dict() == want["stats"] and res.crc32 == want["crc"]
        assert res.min_mask == want["min_mask"] and res.hash_count == want["hash_count"]
        assert ctx.timings().n_event_flushes >= 3


# ======================================================================== CPU tier (emulator)
DENSE_CPU = 240000  # 4741 matches: > 4 x 1024


@pytest.fixture(scope="module")
def dense():
    return phrases(DENSE_CPU, seed=5)


@pytest.mark.parametrize("engine", ["wide", "narrow", "deep"])
def test_drains_on_each_engine(emu_lib, oracle, dense, engine, monkeypatch):
    monkeypatch.setenv("MRZ_SEQ_ENGINE", engine)
    check_capacity(emu_lib, oracle, dense, 1024)


def test_drains_with_short_passes_and_small_lists(emu_lib, oracle, dense):
    check_capacity(emu_lib, oracle, dense, 1024, seg_positions=4096, cand_cap=4096)


def test_noise_at_small_capacity(emu_lib, oracle):
    """No matches, but the passes are bounded by the capacity: the loop still reaches the end."""
    noise = _util.xorshift_noise(400000, seed=21)
    want, t = check_capacity(emu_lib, oracle, noise, 1024, min_flushes=0, min_matches=0)
    assert want["stats"]["matches"] == 0 and t.n_event_flushes == 0
    assert t.n_segments >= 400000 // (31 * 512)


def test_progress_hook_sees_every_match(emu_lib, oracle, dense):
    check_hook(emu_lib, oracle, dense, 1024)


def test_set_event_capacity_arguments(emu_lib):
    check_arguments(emu_lib)


def test_environment_knob_through_host_drivers(emu_lib, oracle, dense, monkeypatch):
    """MRZ_EVENT_CAPACITY reaches the ctxs the host drivers open: the archive and the pipeline's blocks are the
    oracle's."""
    monkeypatch.setenv("MRZ_EVENT_CAPACITY", "1024")
    _parity.check_file(emu_lib, oracle, dense)
    _parity.check_pipeline(emu_lib, oracle, dense)


def test_provider_mode_window_of_one(emu_lib, oracle, dense):
    check_window_of_one(emu_lib, oracle, dense, 1024)


# ======================================================================== GPU tier
DENSE_GPU = 4 << 20


@pytest.fixture(scope="module")
def dense_gpu():
    return phrases(DENSE_GPU, seed=6)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["wide", "narrow", "deep"])
def test_gpu_drains_on_each_engine(gpu_lib, oracle, dense_gpu, engine, monkeypatch):
    monkeypatch.setenv("MRZ_SEQ_ENGINE", engine)
    check_capacity(gpu_lib, oracle, dense_gpu, 4096)


@pytest.mark.gpu
def test_gpu_drains_with_short_passes_and_small_lists(gpu_lib, oracle, dense_gpu):
    check_capacity(gpu_lib, oracle, dense_gpu, 1024, seg_positions=4096, cand_cap=4096)


@pytest.mark.gpu
def test_gpu_noise_at_small_capacity(gpu_lib, oracle):
    check_capacity(gpu_lib, oracle, _util.xorshift_noise(8 << 20, seed=21), 1024, min_flushes=0, min_matches=0)


@pytest.mark.gpu
def test_gpu_progress_hook_sees_every_match(gpu_lib, oracle, dense_gpu):
    check_hook(gpu_lib, oracle, dense_gpu, 4096)


@pytest.mark.gpu
def test_gpu_set_event_capacity_arguments(gpu_lib):
    check_arguments(gpu_lib)


@pytest.mark.gpu
def test_gpu_environment_knob_through_host_drivers(gpu_lib, oracle, dense_gpu, monkeypatch):
    monkeypatch.setenv("MRZ_EVENT_CAPACITY", "4096")
    _parity.check_file(gpu_lib, oracle, dense_gpu)
    _parity.check_pipeline(gpu_lib, oracle, dense_gpu)


@pytest.mark.gpu
def test_gpu_provider_mode_window_of_one(gpu_lib, oracle, dense_gpu):
    check_window_of_one(gpu_lib, oracle, dense_gpu, 4096)


@pytest.mark.gpu
def test_gpu_text_drains(gpu_lib, oracle):
    """zipf_text (one match per few KB): 32 MiB at capacity 1024."""
    check_capacity(gpu_lib, oracle, _util.zipf_text(32 << 20, seed=11), 1024)


@pytest.mark.gpu
def test_gpu_tar_like_drains_on_the_deep_engine(gpu_lib, oracle, monkeypatch):
    """tar_like with the deep engine from a 2-bit mask on: the deep engine's launches drain too."""
    monkeypatch.setenv("MRZ_DEEP_MIN_BITS", "2")
    data = _util.tar_like(64 << 20, seed=5)
    want, t = check_capacity(gpu_lib, oracle, data, 1024, min_flushes=1, min_matches=0)
    assert t.n_deep >= 1
