"""Exact under every retirement schedule.

mrz_rzip_chunk keeps up to four segment launches queued and learns what they did only when it retires them, so the
matcher state it plans with -- mask, position, engine hints, resume point -- lags by 0..3 launches, as the host's timing
has it.  The lag may change which engine runs a segment, how far its front-end pass spans, where a provider-mode
stretch begins and where the match list is drained; it must never change the output.  mrz_set_retire_schedule /
MRZ_RETIRE_SCHEDULE pin the lag (hold, all): once `hold` launches are in flight the host retires the oldest one, or all of
them.  On the emulator, whose launches are synchronous, a ring slot holds what its launch left however late the host
reads it, so the stale schedules are reproducible on the CPU tier; on the GPU the knob is what makes a failure
repeatable.

Every case compares with the oracle (both streams, CRC, the seven counters, victim_round, mask, hash_count, the table
where asked for; the decoder on the oracle's streams) and asserts from mrz_schedule_info / timings() that it reached its
regime: a schedule test that ran synchronously fails."""
import os

import pytest

import modern_rzip_amd as m
from modern_rzip_amd import shard
from tests import _parity, _util
from tests.test_emulated_kernels import _deep_mix
from tests.test_event_window import DENSE_GPU, phrases

MRZ_E_ARG = -1
MRZ_SEG_AHEAD = 4
ONE, ALL = False, True
SCHEDULES = [(1, ALL), (2, ONE), (2, ALL), (3, ONE), (3, ALL), (4, ONE), (4, ALL)]
SCHEDULES_FEW = [(1, ALL), (2, ALL), (4, ONE), (4, ALL)]  # synchronous; the pair retired together; three stale; bursts


def _sid(s):
    return "%d%s" % (s[0], "all" if s[1] else "one")


_WANT = {}


def want_of(oracle, name, data, level, victim_round=0):
    """The oracle's result for an input, computed once per module run (with the table)."""
    key = (name, level, victim_round)
    if key not in _WANT:
        _WANT[key] = oracle.rzip_chunk(data, level=level, victim_round=victim_round, want_table=True)
    return _WANT[key]


def run_schedule(lib, oracle, name, data, sched, level=7, victim_round=0, provider=False, table=False, seg_positions=None,
                 cand_cap=None, capacity=None, decode=True):
    """One chunk under a schedule against the oracle.  Returns (timings, schedule_info); every assertion names the
    schedule and what the host loop did."""
    want = want_of(oracle, name, data, level, victim_round)
    with m.RzipContext(level=level, max_chunk=len(data), lib=lib) as ctx:
        if sched is not None:
            ctx.set_retire_schedule(*sched)
        if seg_positions:
            ctx.set_segment_positions(seg_positions)
        if cand_cap:
            ctx.set_candidate_capacity(cand_cap)
        if capacity:
            ctx.set_event_capacity(capacity)
        if provider:
            res, s0, s1 = shard.rzip_chunk_window(ctx, data, 0, len(data), 0, 1, None, victim_round=victim_round)
        else:
            ctx.victim_round = victim_round
            res, s0, s1 = ctx.rzip_chunk(data)
        t, info = ctx.timings(), ctx.schedule_info()
        said = "%s, %s%s under (hold, all) = %r: retired %d, most per poll %d, largest lag %d, idle launches %d; %d segments, " \
               "%d narrow, %d deep, %d flushes" % ((name, "provider mode, " if provider else "", "level %d" % level, sched)
                                                   + info + (t.n_segments, t.n_narrow, t.n_deep, t.n_event_flushes))
        assert res.crc32 == want["crc"], said
        assert res.stats.as_dict() == want["stats"], said
        assert ctx.victim_round == want["victim_round"], said
        assert res.min_mask == want["min_mask"], said
        assert res.hash_count == want["hash_count"], said
        assert s1 == want["s1"], said
        assert s0 == want["s0"], said
        if table:
            assert ctx.fetch_table() == want["table"], said
        if decode:
            _parity.check_runzip(ctx, data, want["s0"], want["s1"])
    return t, info, said


def assert_lagged(sched, t, info, said, room=MRZ_SEG_AHEAD):
    """The schedule was in force: launches were planned on news hold - 1 launches old, and an `all` schedule retired
    several launches by one poll.  room: launches the room rule lets the host queue at most (a bounded match list)."""
    hold, every = sched
    assert info[0] >= 1 and info[0] <= t.n_segments, said
    if hold == 1:
        assert info[1] == 1 and info[2] == 0, said
    else:
        assert t.n_segments > 2 * hold, said  # (a condition on the input: enough launches for the queue to fill)
        assert info[2] >= min(hold, room) - 1, said
        if every and room >= hold:
            assert info[1] >= 2, said


# ---- the inputs -----------------------------------------------------------------------------------------------------
HANDOVER_SEG = 65536  # positions per pass: a dozen launches lie beyond the hand-over of either input


@pytest.fixture(scope="module")
def noise33():
    return _util.xorshift_noise(3300000, seed=3)


@pytest.fixture(scope="module")
def deep_mix():
    return _deep_mix()


DENSE = 165000  # 3256 matches: more than three lists of 1024 hold, so whatever the schedule the list is drained three
# times before the end of the chunk (an emulated chunk costs by the byte: test_event_window's 240000 cost half as much again)


@pytest.fixture(scope="module")
def dense():
    return phrases(DENSE, seed=5)


@pytest.fixture(scope="module")
def dense_gpu():
    return phrases(DENSE_GPU, seed=6)


def narrow_flip():
    """Text, a stretch of short periods (one long match after another: the narrow engine's regime), noise: with short
    passes the engine choice flips to narrow and back while launches are in flight.  12 passes of one tile: 5 of them
    narrow under (1, all); 8 KiB + 16 periods + 8 KiB flips too (3 of 8), but 8 launches do not fill the queue twice."""
    return _util.zipf_text(12288, seed=4) + _util.rep64k(24, seed=9, period=1024) + _util.xorshift_noise(12288, seed=3)


def chunk_end(n):
    """noise + its repeat, n bytes: the chunk ends inside (or right behind) a long match."""
    blk = _util.xorshift_noise((n + 1) // 2, seed=12)
    return (blk + blk)[:n]


# ---- the checks (lib = the emulator's or the GPU's) -------------------------------------------------------------------
def check_handover(lib, oracle, name, data, sched, provider, seg_positions=HANDOVER_SEG):
    """(a) / (b): the wide engine ends its launch where the mask reaches MRZ_DEEP_MIN_BITS, the launches queued behind it
    were planned for the wide engine and for stretches further on."""
    t, info, said = run_schedule(lib, oracle, name, data, sched, level=1, provider=provider, table=not provider,
                                 seg_positions=seg_positions)
    assert 1 <= t.n_deep < t.n_segments, said
    assert_lagged(sched, t, info, said)
    if sched[0] >= 2:
        assert info[3] >= 1, said  # a launch queued before the host knew of the hand-over sequenced nothing
    return t, info, said


def check_drains(lib, oracle, name, data, sched, capacity, provider=False, seg_positions=None, cand_cap=None):
    """(c): the room rule waits, drains and shortens passes on what the host knows.  It also bounds the lag: a pass is
    queued only if the list has room for every match the queued passes can emit, and a pass of the default span covers
    half the list's worth of positions (31 x capacity / 2) -- two of those fill the list, so the rule waits for the oldest
    launch long before four are in flight (room = 2: a lag of one launch is all that is asked for); passes of one tile (4096 / 31 = 132 matches) leave room for a full queue after every
    drain."""
    want = want_of(oracle, name, data, 7)
    assert want["stats"]["matches"] > 3 * capacity  # (a condition on the input: three drains at the least)
    t, info, said = run_schedule(lib, oracle, name, data, sched, provider=provider, table=not provider, capacity=capacity,
                                 seg_positions=seg_positions, cand_cap=cand_cap)
    assert t.n_event_flushes >= 3, said
    assert_lagged(sched, t, info, said, room=MRZ_SEG_AHEAD if seg_positions == 4096 else 2)


def check_narrow_flip(lib, oracle, sched, seg_positions=4096):
    """(d): the narrow engine's hint lags like everything else."""
    t, info, said = run_schedule(lib, oracle, "narrow_flip", narrow_flip(), sched, table=True, seg_positions=seg_positions)
    assert 0 < t.n_narrow < t.n_segments, said
    assert_lagged(sched, t, info, said)


def check_chunk_ends(lib, oracle, sched):
    """(e): launches queued past the end of the chunk (`finished`, everything queued, stretches beyond the end).  The
    70000 bytes end in one match of 35000: the launch that finds it reports the end, and the launches queued behind it
    -- hold - 1 of them, planned before the host knew -- run on a finished matcher and are never retired."""
    def past_the_end(t, info, said):
        assert_lagged(sched, t, info, said)
        assert t.n_segments - info[0] >= sched[0] - 1, said

    for n in (0, 1, 31, 4097, 70000):
        for vr in (0, 3):
            t, info, said = run_schedule(lib, oracle, "end%d" % n, chunk_end(n), sched, victim_round=vr, seg_positions=4096)
            assert t.n_segments <= (n + 4095) // 4096 and info[0] <= t.n_segments, said
            if n >= 70000:
                past_the_end(t, info, said)
    for n in (4097, 70000):
        t, info, said = run_schedule(lib, oracle, "end%d" % n, chunk_end(n), sched, provider=True, seg_positions=4096)
        if n >= 70000:
            past_the_end(t, info, said)


def check_host_drivers(lib, oracle, data, monkeypatch, sched, capacity, stream_bytes, ramsize):
    """(f): MRZ_RETIRE_SCHEDULE reaches the ctxs the host drivers open (mrz_open reads it, as it reads
    MRZ_EVENT_CAPACITY, which bounds the passes here so that the drivers' chunks take many launches)."""
    monkeypatch.setenv("MRZ_RETIRE_SCHEDULE", "%d:%s" % (sched[0], "all" if sched[1] else "one"))
    monkeypatch.setenv("MRZ_EVENT_CAPACITY", str(capacity))
    with m.RzipContext(lib=lib) as ctx:  # (a ctx opened now runs under the schedule without being told)
        ctx.set_segment_positions(4096)
        ctx.rzip_chunk(data[:60000])
        info = ctx.schedule_info()
        assert info[2] >= sched[0] - 1 and info[1] >= (2 if sched[1] else 1), info
    _parity.check_file(lib, oracle, data)
    _parity.check_pipeline(lib, oracle, data)
    _parity.check_stream(lib, oracle, data[:stream_bytes], to_stdout=True, ramsize=ramsize)  # (several chunks)


def check_knob(lib, oracle):
    """(g)"""
    data = _util.zipf_text(60000, seed=4)
    emulated = os.path.basename(getattr(lib, "_name", "")).startswith("libmrzgpu_emu")
    with m.RzipContext(lib=lib) as ctx:
        for hold, every in ((5, 0), (100, 1), (1, 2), (4, -1), (2, 7)):
            assert lib.mrz_set_retire_schedule(ctx.ctx, hold, every) == MRZ_E_ARG
        with pytest.raises(m.MrzError):
            ctx.set_retire_schedule(5)
        assert lib.mrz_set_retire_schedule(None, 1, 1) == MRZ_E_ARG
        assert lib.mrz_schedule_info(ctx.ctx, None) == MRZ_E_ARG
        for hold, every in ((1, 0), (1, 1), (4, 0), (4, 1), (0, 0), (-1, 5)):
            assert lib.mrz_set_retire_schedule(ctx.ctx, hold, every) == 0
        ctx.set_segment_positions(4096)
        ctx.rzip_chunk(data)
        unset = ctx.timings().n_segments
        assert unset >= 3 * MRZ_SEG_AHEAD and ctx.schedule_info()[0] >= 1
        ctx.set_retire_schedule(1, ALL)
        ctx.rzip_chunk(data)
        info = ctx.schedule_info()
        assert info[1] == 1 and info[2] == 0 and info[3] == 0 and info[0] == ctx.timings().n_segments
        if emulated:
            assert ctx.timings().n_segments == unset  # (the emulator's events have always completed: its own schedule)
        for hold in (2, 3, 4):
            for every in (ONE, ALL):
                ctx.set_retire_schedule(hold, every)
                ctx.rzip_chunk(data)
                info = ctx.schedule_info()
                assert info[2] >= hold - 1 and info[1] >= (2 if every else 1), (hold, every, info)
        ctx.set_retire_schedule(0)  # back to polling the events
        res, s0, s1 = ctx.rzip_chunk(data)
        if emulated:
            assert ctx.schedule_info()[1:3] == (1, 0)
        want = oracle.rzip_chunk(data)
        assert (s0, s1) == (want["s0"], want["s1"])


# ======================================================================== CPU tier (emulator)
# Every schedule for the hand-over of the noise and for both inputs in provider mode, where the host lays out the stretches
# and every `all` schedule retires the launch that handed over together with the stale ones behind it; SCHEDULES_FEW for
# the rest.  An emulated chunk costs 25 s (hand-over) and 20 to 60 s (dense matches, by the engine).
@pytest.fixture
def handover_env(monkeypatch):
    monkeypatch.setenv("MRZ_DEEP_MIN_BITS", "5")


@pytest.mark.parametrize("sched", SCHEDULES, ids=_sid)
def test_handover_noise(emu_lib, oracle, noise33, handover_env, sched):
    check_handover(emu_lib, oracle, "noise33", noise33, sched, provider=False)


@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_handover_deep_mix(emu_lib, oracle, deep_mix, handover_env, sched):
    check_handover(emu_lib, oracle, "deep_mix", deep_mix, sched, provider=False)


@pytest.mark.parametrize("sched", SCHEDULES, ids=_sid)
def test_handover_noise_provider_mode(emu_lib, oracle, noise33, handover_env, sched):
    check_handover(emu_lib, oracle, "noise33", noise33, sched, provider=True)


@pytest.mark.parametrize("sched", SCHEDULES, ids=_sid)
def test_handover_deep_mix_provider_mode(emu_lib, oracle, deep_mix, handover_env, sched):
    check_handover(emu_lib, oracle, "deep_mix", deep_mix, sched, provider=True)


@pytest.mark.parametrize("engine", [None, "wide", "narrow", "deep"])
@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_drains_under_lag(emu_lib, oracle, dense, sched, engine, monkeypatch):
    """Passes of the default span: the room rule keeps the lag below the schedule's (see check_drains)."""
    if engine:
        monkeypatch.setenv("MRZ_SEQ_ENGINE", engine)
    check_drains(emu_lib, oracle, "dense", dense, sched, 1024)


@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_drains_under_lag_provider_mode(emu_lib, oracle, dense, sched):
    check_drains(emu_lib, oracle, "dense", dense, sched, 1024, provider=True)


@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_drains_under_lag_short_passes_small_lists(emu_lib, oracle, dense, sched):
    """Passes of one tile: the queue fills after every drain, and the room rule counts the launches in flight."""
    check_drains(emu_lib, oracle, "dense", dense, sched, 1024, seg_positions=4096, cand_cap=4096)


@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_narrow_hint_lags(emu_lib, oracle, sched):
    check_narrow_flip(emu_lib, oracle, sched)


@pytest.mark.parametrize("sched", [(4, ALL), (4, ONE)], ids=_sid)
def test_chunk_ends(emu_lib, oracle, sched):
    check_chunk_ends(emu_lib, oracle, sched)


def test_environment_variable_through_host_drivers(emu_lib, oracle, dense, monkeypatch):
    check_host_drivers(emu_lib, oracle, dense[:80000], monkeypatch, (4, ALL), 1024, stream_bytes=80000, ramsize=6 * 30000)


def test_malformed_environment_variable_means_the_default(emu_lib, monkeypatch):
    data = _util.zipf_text(20000, seed=4)
    for bad in ("", "2", "5:all", "0:one", "2:some", "2:all:", "x:all"):
        monkeypatch.setenv("MRZ_RETIRE_SCHEDULE", bad)
        with m.RzipContext(lib=emu_lib) as ctx:
            ctx.set_segment_positions(4096)
            ctx.rzip_chunk(data)
            info = ctx.schedule_info()
            assert info[1] == 1 and info[2] == 0, (bad, info)  # the emulator's default: every launch retired at once


def test_retire_schedule_knob(emu_lib, oracle):
    check_knob(emu_lib, oracle)


# ======================================================================== GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("provider", [False, True], ids=["", "provider"])
@pytest.mark.parametrize("name", ["noise33", "deep_mix"])
@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_gpu_handover(gpu_lib, oracle, noise33, deep_mix, handover_env, sched, name, provider):
    check_handover(gpu_lib, oracle, name, noise33 if name == "noise33" else deep_mix, sched, provider=provider)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", [None, "wide", "narrow", "deep"])
@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_gpu_drains_under_lag(gpu_lib, oracle, dense_gpu, sched, engine, monkeypatch):
    if engine:
        monkeypatch.setenv("MRZ_SEQ_ENGINE", engine)
    check_drains(gpu_lib, oracle, "dense_gpu", dense_gpu, sched, 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_gpu_drains_under_lag_provider_mode(gpu_lib, oracle, dense_gpu, sched):
    check_drains(gpu_lib, oracle, "dense_gpu", dense_gpu, sched, 4096, provider=True)


@pytest.mark.gpu
@pytest.mark.parametrize("sched", SCHEDULES_FEW, ids=_sid)
def test_gpu_drains_under_lag_short_passes_small_lists(gpu_lib, oracle, dense_gpu, sched):
    check_drains(gpu_lib, oracle, "dense_gpu", dense_gpu, sched, 1024, seg_positions=4096, cand_cap=4096)


@pytest.mark.gpu
def test_gpu_narrow_hint_lags(gpu_lib, oracle):
    check_narrow_flip(gpu_lib, oracle, (4, ALL))


@pytest.mark.gpu
def test_gpu_chunk_ends(gpu_lib, oracle):
    check_chunk_ends(gpu_lib, oracle, (4, ALL))


@pytest.mark.gpu
def test_gpu_environment_variable_through_host_drivers(gpu_lib, oracle, dense_gpu, monkeypatch):
    check_host_drivers(gpu_lib, oracle, dense_gpu, monkeypatch, (4, ALL), 4096, stream_bytes=3 << 20, ramsize=6 << 20)


@pytest.mark.gpu
def test_gpu_retire_schedule_knob(gpu_lib, oracle):
    check_knob(gpu_lib, oracle)
