// tests/c/plan_test.cpp -- TEST: the launch planner of mrz_rzip_chunk (mrz_chunk_plan.h) on its own, against a toy device.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imodern-rzip_amd/csrc tests/c/plan_test.cpp -o plan_test
//
// No HIP: every launch is synchronous and leaves a snapshot in a ring slot; the host reads a slot as late as the
// retirement schedule under test says, exactly as the driver in mrz_capi.hip does.  The toy matcher is a legal matcher
// (disjoint matches of >= 31 bytes, each emitted at a position of a queued pass and starting no later than it) that
// emits as many matches as the room rule's derivation allows for:
//   - it starts with a match pending (cur_len > 0), and every launch leaves one pending for the next;
//   - one match reaches back before the matcher's position v (counted, once per chunk, in the launch `back_at`);
//   - every position is a candidate and a 31-byte match is found wherever none is pending: one per 31 positions of
//     every stretch covered;
//   - every `late_every`-th launch ends in a great match that carries the matcher whole tiles beyond its pass: the next
//     pass begins late, and the launch over it emits one match more.
// It can also hand over from the wide to the deep engine (a launch ends early where the mask tightens, scan_next goes
// back to p's tile, and the wide launches queued behind it sequence nothing and report the same resume point) and cut
// passes short (a full candidate list).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mrz_chunk_plan.h"

#define MRZ_EVENT_MIN 1024ll  // (mrz_capi.hip)
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "plan_test: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                             \
            fprintf(stderr, "\n  in %s\n", g_case);                   \
            exit(1);                                                  \
        }                                                             \
    } while (0)
static char g_case[512];

enum { POLL_EAGER = 0, POLL_LAZY = -1 };  // hold == 0: every event has completed when polled / none ever has

struct toy_case {
    int64_t n, ev_cap, seg_positions, cand_cap;
    bool provider;
    int hold, hold_all, lazy;
    int engine_pin, deep_min_bits, narrow_max_bits;
    int late_every;      // 0: no great matches
    int cut_every;       // 0: no pass is cut short
    int64_t handover_at; // launch that hands over to the deep engine; -1: none
    int64_t back_at;     // launch that emits the match reaching back
    int64_t narrow_from, narrow_to;  // launches that report the narrow engine's regime in their hint
};

struct toy_device {
    mrz_seq_state st;
    int64_t launches, max_listed;
    bool handed;  // the wide engine has handed over to the deep one
    const toy_case *tc;

    void emit() {
        st.n_events++;
        if (st.n_events - st.ev_base > max_listed) max_listed = st.n_events - st.ev_base;
    }
    // the matcher over [lo, hi) of a pass or stretch
    void sequence(int64_t lo, int64_t hi, mrz_plan_engine engine, bool late) {
        const int64_t idx = launches++;
        const int64_t p0 = st.p, ev0 = st.n_events;
        st.hint_positions = st.hint_matched = 0;
        if (st.finished) return;
        const int bits = __builtin_popcountll((unsigned long long)st.min_mask);
        if (engine == MRZ_ENGINE_WIDE && !tc->engine_pin && bits >= tc->deep_min_bits) {
            st.scan_next = st.p / MRZ_TILE * MRZ_TILE;  // (stale: planned before the host knew of the hand-over)
            return;
        }
        int64_t lim = hi - 1 < st.end ? hi - 1 : st.end;
        const bool handover = tc->handover_at >= 0 && idx >= tc->handover_at && !handed && lim > st.p + 100;
        if (handover) lim = st.p + (lim - st.p) / 3;  // the launch ends early, where the mask reaches the deep regime
        if (lim > st.p) {
            if (late) emit();  // (the pass began late: one match more, see the room rule)
            if (idx == tc->back_at) emit();  // (the match reaching back before v)
            for (;;) {
                if (!st.cur_len) st.cur_p = st.p + 1 > lo ? st.p + 1 : lo, st.cur_len = MRZ_MIN_MATCH;
                const int64_t e = st.cur_p + st.cur_len;  // where the pending match is emitted and the next one found
                if (e > lim) break;
                emit();
                st.last_match = e, st.p = e - 1;
                st.cur_len = 0;
            }
            st.p = lim;
            st.inserts += lim - p0;
            if (tc->late_every && idx % tc->late_every == tc->late_every - 1 && !handover && lim < st.end) {
                // a great match found at the pass's last position replaces the pending one and is emitted at once: the
                // matcher goes on whole tiles further on
                emit();
                st.p = lim + 2 * MRZ_TILE + 77;
                if (st.p > st.end) st.p = st.end;
                st.last_match = st.p;
                st.cur_len = 0;
            }
        }
        if (handover) {
            handed = true;
            st.min_mask = (1ll << tc->deep_min_bits) - 1;
            st.scan_next = st.p / MRZ_TILE * MRZ_TILE;
        }
        if (st.p >= st.end) {
            if (st.cur_len) emit(), st.cur_len = 0;  // (the end of the chunk: the pending match goes out)
            st.finished = 1;
        }
        st.hint_positions = st.p - p0;
        st.hint_matched = idx >= tc->narrow_from && idx < tc->narrow_to ? st.p - p0 : (st.n_events - ev0) * 3;
    }
    // a front-end pass of max_tiles tiles, behind the last one and never before the tile of the matcher's position
    bool pass(int64_t max_tiles, mrz_plan_engine engine) {
        if (st.finished) {
            sequence(0, 0, engine, false);
            return false;
        }
        const int64_t pt = (st.p + 1) / MRZ_TILE * MRZ_TILE;
        const bool late = pt > st.scan_next;
        int64_t T = max_tiles;
        bool cut = false;
        if (tc->cut_every && launches % tc->cut_every == tc->cut_every - 1 && T > 1) T = (T + 1) / 2, cut = true;
        st.seg_start = late ? pt : st.scan_next;
        st.scan_next = st.seg_start + T * MRZ_TILE;
        st.seg_end = st.scan_next < st.end + 1 ? st.scan_next : st.end + 1;
        if (st.seg_end < st.seg_start) st.seg_end = st.seg_start;
        sequence(st.seg_start, st.seg_end, engine, late);
        return cut || late;
    }
};

static int run_case(const toy_case &tc) {
    snprintf(g_case, sizeof(g_case),
             "n=%lld ev_cap=%lld seg=%lld cand=%lld provider=%d hold=%d all=%d lazy=%d pin=%d late=%d cut=%d handover=%lld",
             (long long)tc.n, (long long)tc.ev_cap, (long long)tc.seg_positions, (long long)tc.cand_cap, tc.provider, tc.hold,
             tc.hold_all, tc.lazy, tc.engine_pin, tc.late_every, tc.cut_every, (long long)tc.handover_at);
    mrz_plan_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.end = tc.n - MRZ_MIN_MATCH;
    cfg.ev_cap = tc.ev_cap;
    cfg.bounded = tc.ev_cap < tc.n / MRZ_MIN_MATCH + 2;
    cfg.pass_cap = mrz_plan_pass_cap(tc.ev_cap);
    cfg.cand_cap = tc.cand_cap;
    cfg.seg_positions = tc.seg_positions;
    cfg.fe_tiles_cap = cfg.end / MRZ_TILE + 2 < tc.seg_positions / MRZ_TILE ? cfg.end / MRZ_TILE + 2 : tc.seg_positions / MRZ_TILE;
    cfg.provider = tc.provider;
    cfg.engine_pin = tc.engine_pin;
    cfg.deep_min_bits = tc.deep_min_bits;
    cfg.narrow_max_bits = tc.narrow_max_bits;
    cfg.hold = tc.hold;
    cfg.hold_all = tc.hold_all;

    toy_device dev;
    memset(&dev, 0, sizeof(dev));
    dev.tc = &tc;
    dev.st.n = tc.n;
    dev.st.end = cfg.end;
    dev.st.min_mask = 1;
    dev.st.event_cap = tc.ev_cap;
    dev.st.cur_len = MRZ_MIN_MATCH;  // a match is pending from the start
    mrz_seq_state ring[MRZ_SEG_AHEAD];
    mrz_seq_state news = dev.st;  // what the host has last read (the engine choice is checked against it)
    news.hint_positions = news.hint_matched = 0;

    mrz_chunk_plan plan;
    plan.init(cfg, dev.st.min_mask);
    CHECK(!plan.finished, "a chunk of %lld bytes has positions to look up", (long long)tc.n);
    bool exact = true;  // no pass cut short, begun late or handed over so far: the host's book-keeping is the device's
    int64_t n_drains = 0, steps = 0, want_narrow = 0, want_deep = 0;
    int64_t last_start = -1, went_back = 0;  // provider mode: stretches asked for from before the start of the last one
    const int64_t max_steps = 16 * (cfg.end / MRZ_TILE + 64);
    auto retire = [&]() {
        news = ring[plan.retired % MRZ_SEG_AHEAD];
        const mrz_plan_news r = plan.retire(news);
        CHECK(r.n_events == news.n_events && r.last_match == news.last_match, "the hook's news");
    };
    while (!plan.finished) {
        CHECK(++steps <= max_steps, "no end after %lld steps (launched %lld, retired %lld, device p %lld of %lld)",
              (long long)steps, (long long)plan.launched, (long long)plan.retired, (long long)dev.st.p, (long long)cfg.end);
        const int64_t retired0 = plan.retired;
        if (!tc.hold && !tc.lazy)
            while (plan.retired < plan.launched && !plan.finished) retire();
        CHECK(tc.hold || !plan.due(), "no schedule: nothing is due");
        for (const int64_t upto = plan.retired + plan.due(); plan.retired < upto && !plan.finished;) retire();
        plan.polled(plan.retired - retired0);
        if (plan.finished) break;
        if (exact && !tc.provider && !dev.st.finished) {
            int64_t est = plan.known_next;
            for (int64_t k = plan.retired; k < plan.launched; k++) est += plan.span_of[k % MRZ_SEG_AHEAD];
            CHECK(est == dev.st.scan_next, "span_of: the host expects the next pass at %lld, the device begins it at %lld",
                  (long long)est, (long long)dev.st.scan_next);
        }
        const mrz_plan_step st = plan.next();
        CHECK(st.what != MRZ_PLAN_FAIL, "the planner gave up (overflow)");
        if (st.what == MRZ_PLAN_WAIT) {
            CHECK(plan.retired < plan.launched, "waits for a launch that is not there");
            retire();
            continue;
        }
        if (st.what == MRZ_PLAN_DRAIN) {
            CHECK(plan.launched == plan.retired && plan.known_events > plan.ev_base && cfg.bounded, "drains with launches in flight");
            plan.drained();
            dev.st.ev_base = plan.ev_base;
            CHECK(dev.st.ev_base == dev.st.n_events, "nothing in flight: the drain empties the list");
            n_drains++;
            continue;
        }
        // ---- a launch: the engine follows the pin, else the hint and the thresholds, as last heard of
        const int bits = __builtin_popcountll((unsigned long long)news.min_mask);
        mrz_plan_engine want = MRZ_ENGINE_WIDE;
        if (news.hint_positions > 0 && news.hint_matched * 10 >= news.hint_positions * 8 && bits < tc.narrow_max_bits)
            want = MRZ_ENGINE_NARROW;
        else if (bits >= tc.deep_min_bits)
            want = MRZ_ENGINE_DEEP;
        if (tc.engine_pin) want = tc.engine_pin == 2 ? MRZ_ENGINE_NARROW : tc.engine_pin == 3 ? MRZ_ENGINE_DEEP : MRZ_ENGINE_WIDE;
        CHECK(st.engine == want, "engine %d, expected %d (mask of %d bits, hint %lld/%lld)", (int)st.engine, (int)want, bits,
              (long long)news.hint_matched, (long long)news.hint_positions);
        want_narrow += want == MRZ_ENGINE_NARROW, want_deep += want == MRZ_ENGINE_DEEP;
        CHECK(plan.launched - plan.retired < MRZ_SEG_AHEAD, "more than MRZ_SEG_AHEAD launches in flight");
        if (st.what == MRZ_PLAN_PASS) {
            CHECK(!tc.provider, "a pass in provider mode");
            CHECK(st.max_tiles >= 1 && st.span == st.max_tiles * MRZ_TILE && st.max_tiles <= cfg.fe_tiles_cap &&
                      st.span <= tc.seg_positions && (!cfg.bounded || st.span <= cfg.pass_cap),
                  "a pass of %lld positions, %lld tiles", (long long)st.span, (long long)st.max_tiles);
            if (exact) CHECK(dev.st.scan_next <= cfg.end, "a pass beyond the end of the chunk (at %lld)", (long long)dev.st.scan_next);
            if (dev.pass(st.max_tiles, st.engine) || dev.handed) exact = false;
        } else {
            CHECK(tc.provider, "a stretch without a provider");
            CHECK(st.seg_start % MRZ_TILE == 0 && st.span % MRZ_TILE == 0, "stretch [%lld, +%lld)", (long long)st.seg_start, (long long)st.span);
            if (!st.span) {
                CHECK(st.seg_start > cfg.end, "an empty stretch at %lld, before the end", (long long)st.seg_start);
                plan.stretch_ends(st.seg_start);
                dev.sequence(0, 0, st.engine, false);
            } else {
                CHECK(st.seg_start <= cfg.end && st.seg_start + st.span < cfg.end + 1 + MRZ_TILE && st.span <= tc.seg_positions,
                      "stretch [%lld, +%lld) beyond the end", (long long)st.seg_start, (long long)st.span);
                // the stretches go on, but for the one asked for from the resume point of the hand-over -- once: the stale
                // launches behind it report that point again
                if (st.seg_start <= last_start) went_back++;
                CHECK(went_back <= (dev.handed ? 1 : 0), "stretch [%lld, +%lld) asked for again", (long long)st.seg_start, (long long)st.span);
                last_start = st.seg_start;
                int64_t nx = st.seg_start + st.span;
                if (tc.cut_every && dev.launches % tc.cut_every == tc.cut_every - 1 && st.span > MRZ_TILE)
                    nx = st.seg_start + (st.span / MRZ_TILE + 1) / 2 * MRZ_TILE;
                const bool late = st.seg_start > dev.st.scan_next && dev.st.p + 1 >= st.seg_start;
                dev.st.seg_start = st.seg_start;
                dev.st.seg_end = nx < cfg.end + 1 ? nx : cfg.end + 1;
                dev.st.scan_next = nx;
                dev.sequence(dev.st.seg_start, dev.st.seg_end, st.engine, late);
                plan.stretch_ends(nx);
            }
        }
        CHECK(dev.max_listed <= tc.ev_cap, "the list holds %lld matches, more than its %lld entries", (long long)dev.max_listed,
              (long long)tc.ev_cap);
        ring[plan.launched % MRZ_SEG_AHEAD] = dev.st;
        plan.launch_queued(st);
    }
    CHECK(dev.st.finished && !dev.st.error && dev.st.p >= cfg.end, "the planner ends before the device (p %lld of %lld)",
          (long long)dev.st.p, (long long)cfg.end);
    CHECK(plan.launched == dev.launches && plan.retired <= plan.launched, "launch count");
    CHECK(plan.n_narrow == want_narrow && plan.n_deep == want_deep, "engine counters");
    if (tc.engine_pin) CHECK(plan.n_narrow == (tc.engine_pin == 2 ? plan.launched : 0) && plan.n_deep == (tc.engine_pin == 3 ? plan.launched : 0), "pinned");
    if (!cfg.bounded) CHECK(!n_drains, "an unbounded list is never drained");
    // the schedule was in force (tests/test_retire_schedules.py: assert_lagged)
    CHECK(plan.max_lag < MRZ_SEG_AHEAD && plan.max_burst <= MRZ_SEG_AHEAD, "lag %lld, burst %lld", (long long)plan.max_lag, (long long)plan.max_burst);
    if (tc.hold == 1 || (!tc.hold && !tc.lazy))
        CHECK(plan.max_burst == 1 && plan.max_lag == 0, "synchronous: lag %lld, burst %lld", (long long)plan.max_lag, (long long)plan.max_burst);
    else if (plan.launched > 2 * MRZ_SEG_AHEAD) {
        // launches the room rule lets the host queue: all four when the list is unbounded or the passes are one tile
        // (132 matches each); two passes of the default span fit a drained list of these capacities (see run_all)
        const int64_t room = !cfg.bounded || tc.seg_positions == MRZ_TILE ? MRZ_SEG_AHEAD : 2;
        const int64_t hold = tc.hold ? tc.hold : MRZ_SEG_AHEAD;
        CHECK(plan.max_lag >= (hold < room ? hold : room) - 1, "lag %lld under hold %lld, room %lld", (long long)plan.max_lag,
              (long long)hold, (long long)room);
        if (tc.hold && tc.hold_all && room >= hold) CHECK(plan.max_burst >= 2, "burst %lld", (long long)plan.max_burst);
    }
    return (int)n_drains;
}

int main() {
    static const int schedules[][2] = { { 1, 1 }, { 2, 0 }, { 2, 1 }, { 3, 0 }, { 3, 1 }, { 4, 0 }, { 4, 1 },  // SCHEDULES
                                        { 0, POLL_EAGER }, { 0, POLL_LAZY } };
    // capacities: two passes of the default span (31 x cap / 2 positions, whole tiles) fit each of them with the five
    // matches the rule adds -- 1024: 2 x 12288 / 31 + 5 = 797; 1500: 2 x 20480 / 31 + 5 = 1326; 4096: 2 x 61440 / 31 + 5 = 3968
    static const int64_t caps[] = { MRZ_EVENT_MIN, 1500, 4096, 1ll << 20 };
    static const int64_t segs[] = { MRZ_TILE, 3 * MRZ_TILE, 16 * MRZ_TILE, 1ll << 30 };
    static const int64_t sizes[] = { 40000, 8 * MRZ_TILE + MRZ_MIN_MATCH, 700001 };
    int64_t cases = 0, drains = 0;
    for (const auto &s : schedules)
        for (int64_t cap : caps)
            for (int64_t seg : segs)
                for (int64_t n : sizes)
                    for (int provider = 0; provider < 2; provider++)
                        for (int variant = 0; variant < 6; variant++) {
                            toy_case tc;
                            memset(&tc, 0, sizeof(tc));
                            tc.n = n, tc.ev_cap = cap, tc.seg_positions = seg, tc.provider = provider != 0;
                            tc.cand_cap = seg == MRZ_TILE ? 4096 : 8ll << 20;
                            tc.hold = s[0], tc.hold_all = s[0] ? s[1] : 0, tc.lazy = !s[0] && s[1] == POLL_LAZY;
                            tc.deep_min_bits = 6, tc.narrow_max_bits = 6;
                            tc.handover_at = -1, tc.back_at = 1;
                            if (variant == 1) tc.late_every = 3, tc.back_at = 4;
                            if (variant == 2) tc.cut_every = 2, tc.late_every = 5;
                            if (variant == 3) tc.handover_at = 5, tc.back_at = 6;                      // wide -> deep
                            if (variant == 4) tc.narrow_from = 3, tc.narrow_to = 9, tc.handover_at = 12;  // narrow, back, deep
                            if (variant == 5) tc.engine_pin = 1 + (int)(cases % 3), tc.handover_at = 4, tc.narrow_to = 1 << 30;
                            drains += run_case(tc);
                            cases++;
                        }
    if (!drains) {
        fprintf(stderr, "plan_test: no case drained its list\n");
        return 1;
    }
    printf("plan_test ok: %lld cases, %lld drains\n", (long long)cases, (long long)drains);
    return 0;
}
