// mrz_chunk_plan.h -- the launch planner of mrz_rzip_chunk: which segment the host queues next, and when it waits,
// drains the match list or shortens a pass instead.  Pure arithmetic on the mrz_seq_state snapshots the launches leave
// behind, read late; host code without a HIP call or include, so that tests/c/plan_test.cpp drives it on its own.
// The driver (mrz_capi.hip) owns the stream, the events and the buffers, and tells the planner what it has done.
#pragma once
#include <stdint.h>

#include "mrz_common.h"

#define MRZ_SEG_AHEAD 4  // segment launches the host keeps queued ahead of the device

// what is fixed for the whole chunk
struct mrz_plan_config {
    int64_t end;            // last position that is looked up (src/rzip.c:544)
    int64_t ev_cap;         // entries the sequencers may fill
    bool bounded;           // ... fewer than the chunk could emit: the list is drained in pieces (the room rule)
    int64_t pass_cap;       // the span of one pass at most when the list is bounded (mrz_plan_pass_cap)
    int64_t cand_cap;       // entries a pass may fill
    int64_t seg_positions;  // positions per front-end pass at most
    int64_t fe_tiles_cap;   // tiles the front end's buffers hold
    bool provider;          // window sharding: a candidate provider lays out the stretches
    int engine_pin;         // 0 per-segment choice, 1 wide, 2 narrow, 3 deep
    int deep_min_bits, narrow_max_bits;
    int hold, hold_all;     // the retirement schedule (mrz_set_retire_schedule: a test knob; 0 = poll the events)
};

// the span of one pass when the list is bounded: half the list's worth of positions, so that a drained list always
// has room for the next pass (the room rule)
static inline int64_t mrz_plan_pass_cap(int64_t ev_cap) {
    const int64_t pass_cap = MRZ_MIN_MATCH * (ev_cap / 2) / MRZ_TILE * MRZ_TILE;
    return pass_cap < MRZ_TILE ? MRZ_TILE : pass_cap;
}

enum mrz_plan_what {
    MRZ_PLAN_WAIT,     // wait for the oldest launch and retire it
    MRZ_PLAN_DRAIN,    // nothing in flight: encode what the list holds and empty it
    MRZ_PLAN_PASS,     // a front-end pass of max_tiles tiles, then the sequencer
    MRZ_PLAN_STRETCH,  // provider mode: ask for [seg_start, seg_start + span), then the sequencer; span 0: the empty
                       // stretch behind `end` (nothing to ask for: the matcher is about to report the end)
    MRZ_PLAN_FAIL      // MRZ_E_OVERFLOW
};
enum mrz_plan_engine { MRZ_ENGINE_WIDE, MRZ_ENGINE_NARROW, MRZ_ENGINE_DEEP };

struct mrz_plan_step {
    mrz_plan_what what;
    int64_t seg_start, span, max_tiles;
    mrz_plan_engine engine;
};

struct mrz_plan_news {  // what the progress hook is told of a retired launch
    int64_t n_events, last_match;
};

// ---- the segments: a front-end pass (candidate list of the next stretch) and a sequencer launch over it, again
// and again until the matcher reports the end of the chunk.  WHERE a pass begins and ends is device state (it goes
// on behind the last one, skips what an emitted match has covered, and stops where its list is full); the host
// only bounds the span of a pass -- from the mask the matcher has reached: the tighter the mask, the more
// positions a list of the same size covers -- and keeps MRZ_SEG_AHEAD segments queued.  Every launch leaves a
// snapshot of the matcher state in a ring of pinned host slots (ONE copy per launch: position, masks, progress and
// the `finished` flag belong together); the host reads a slot once the launch's event has completed.
struct mrz_chunk_plan {
    mrz_plan_config cfg;
    int64_t launched, retired, n_narrow, n_deep;
    int64_t span_of[MRZ_SEG_AHEAD];  // positions the pass of an in-flight launch may cover
    int64_t known_next;              // where the pass after the last retired launch begins, as far as the host knows
    int64_t known_mask, known_p;
    int64_t hint_pos, hint_matched;
    int64_t known_events, known_last;  // matches emitted by the last retired launch, and where the last one ended
    int64_t resume_seen;  // (window sharding) launches before this one were prepared before the last resume point was known
    int64_t ev_base;      // absolute index of the list's first entry (> 0 once the list has been drained)
    bool finished;
    // what mrz_schedule_info reports
    int64_t max_burst, max_lag, n_idle, prev_p, prev_events, prev_inserts;

    void init(const mrz_plan_config &c, int64_t min_mask) {
        *this = mrz_chunk_plan();
        cfg = c;
        known_mask = min_mask;
        finished = c.end <= 0;
    }

    // a launch whose event has completed: its snapshot is final
    mrz_plan_news retire(const mrz_seq_state &sn) {
        const int64_t idx = retired++;
        if (!sn.finished && sn.p == prev_p && sn.n_events == prev_events && sn.inserts == prev_inserts) n_idle++;
        prev_p = sn.p, prev_events = sn.n_events, prev_inserts = sn.inserts;
        known_p = sn.p;
        known_mask = sn.min_mask;
        known_events = sn.n_events;
        known_last = sn.last_match;
        if (!cfg.provider)
            known_next = sn.scan_next;
        else if (sn.seg_end > sn.seg_start && sn.scan_next < sn.seg_end && idx >= resume_seen) {
            // (window sharding, where the host drives the geometry: the wide engine has ended this launch where the mask
            // reached the deep engine's regime and taken scan_next back to its position -- the next stretch is asked for
            // from there.  The launches in flight right now were prepared for stretches beyond the one that was cut
            // short: they sequence nothing and report the same resume point, which by then is old news -- a stretch from
            // it has been queued, and known_next is where that one ends.)
            known_next = sn.scan_next;
            resume_seen = launched;
        }
        hint_pos = sn.hint_positions;
        hint_matched = sn.hint_matched;
        if (sn.finished || sn.error) finished = true;
        return { sn.n_events, sn.last_match };
    }

    // (the schedule of mrz_set_retire_schedule: the oldest launch, or all of them, once `hold` are in flight)
    // launches the host has to wait for and retire before it plans on; 0 under hold == 0, where it polls the events
    int64_t due() const {
        if (!cfg.hold || launched - retired < cfg.hold) return 0;
        return cfg.hold_all ? launched - retired : 1;
    }
    // `n` launches were retired by one poll (or one turn of the schedule) at the top of the segment loop
    void polled(int64_t n) {
        if (n > max_burst) max_burst = n;
    }

    // positions a front-end pass should look at under a mask of k bits so that its list comes out about 3/4 full
    int64_t span_for_mask(int64_t mask) const {
        const int k = __builtin_popcountll((unsigned long long)mask);
        int64_t span = (cfg.cand_cap - cfg.cand_cap / 4) << (k < 24 ? k : 24);
        if (span > cfg.seg_positions) span = cfg.seg_positions;
        span = span / MRZ_TILE * MRZ_TILE;
        return span < MRZ_TILE ? MRZ_TILE : span;
    }

    // Which engine: the wide one (512 candidates per batch) unless the segments before were one long match after
    // another (>= 80 % of the positions a launch advanced over lay inside the matches it emitted): then the
    // narrow engine's shorter chain per match wins.  The hint lags behind like everything the host knows; the first
    // two launches are waited for so that it arrives early.  MRZ_SEQ_ENGINE=wide|narrow pins the choice (tests,
    // measurements).
    mrz_plan_engine engine() const {
        const int mask_bits = __builtin_popcountll((unsigned long long)known_mask);
        bool narrow = hint_pos > 0 && hint_matched * 10 >= hint_pos * 8 && mask_bits < cfg.narrow_max_bits;
        // ... and the deep engine once the cull sweeps have tightened the mask: the table then consists of a few long
        // runs (2^(hash_bits - k) of about 2/3 x 2^k slots under a k-bit mask) that every look-up reads to the end --
        // streaming scans, not the short walks the wide engine's lanes are made for
        bool deep = !narrow && mask_bits >= cfg.deep_min_bits;
        if (cfg.engine_pin) narrow = cfg.engine_pin == 2, deep = cfg.engine_pin == 3;
        return narrow ? MRZ_ENGINE_NARROW : deep ? MRZ_ENGINE_DEEP : MRZ_ENGINE_WIDE;
    }

    // what the host does next (not finished, the poll of the events done)
    mrz_plan_step next() {
        mrz_plan_step st = { MRZ_PLAN_WAIT, 0, 0, 0, MRZ_ENGINE_WIDE };
        // where the queued passes will have got to if none of them is cut short
        int64_t ahead = 0;
        for (int64_t k = retired; k < launched; k++) ahead += span_of[k % MRZ_SEG_AHEAD];
        const int64_t est_next = known_next + ahead;
        const bool queue_full = launched - retired >= MRZ_SEG_AHEAD;
        const bool all_queued = est_next > cfg.end;  // (only a list that fills up -- or the provider -- can prove this wrong)
        if (queue_full || (all_queued && launched > retired)) return st;  // wait for the oldest launch
        if (all_queued) {
            // nothing in flight and, by the host's book-keeping, nothing left -- yet the matcher has not reported the end:
            // cannot happen (a pass always covers its span unless its list fills, and then known_next says so)
            st.what = MRZ_PLAN_FAIL;
            return st;
        }
        // ---- one more segment
        int64_t span = span_for_mask(known_mask);
        if (cfg.bounded && span > cfg.pass_cap) span = cfg.pass_cap;
        int64_t max_tiles = span / MRZ_TILE;
        if (max_tiles > cfg.fe_tiles_cap) max_tiles = cfg.fe_tiles_cap;
        span = max_tiles * MRZ_TILE;
        // where the pass after S begins: scan_next, or the tile of v + 1 when an emitted match has carried the matcher
        // further (provider mode: where the stretch to ask for begins)
        const int64_t pt = (known_p + 1) / MRZ_TILE * MRZ_TILE;
        const int64_t start = known_next > pt ? known_next : pt;
        if (cfg.bounded) {
            // The room rule: queue a pass only if the list can take every match the launches after the latest retired
            // one (snapshot S: n_events_S matches, matcher at v = known_p) can emit.  Every position <= v has been looked
            // at under the mask of S (a launch that used up its list leaves p at its pass's last position, lim; one that
            // ended early, as on the wide-to-deep hand-over, leaves its real p and scan_next goes back to p's tile), and
            // masks only tighten, so the matches emitted after S are
            //   - the match pending in S (cur_len > 0), or a longer one that replaces it, and one match found beyond v
            //     whose backward extension reaches before it: 2;
            //   - matches that start at or after v: disjoint, >= 31 bytes, each emitted at a candidate -- a position of
            //     one of the queued passes, so at or before F, the last position of the furthest one (clamped to end)
            //     -- and starting no later than that candidate (src/rzip.c:586-599: cur_p <= p, and p returns to
            //     last_match): at most 1 + (F - v) / 31.
            // F is estimated from where the pass after S begins (scan_next, or the tile of v + 1 when an emitted match
            // has carried the matcher further) plus the spans of the passes in flight.  A pass begins later than that
            // only where a match emitted by the launch before carried p beyond its end: the positions skipped lie
            // inside that one match, so each launch adds at most one match to the estimate -- counted below as one per
            // launch after S.  (Passes cut short by a full candidate list, or scanned again after a hand-over, only
            // end earlier.)  Provider mode: known_next is already where the furthest queued stretch ends.
            const int64_t from = start + ahead;
            const int64_t fixed = known_events - ev_base + 2 + 1 + (launched - retired + 1);
            int64_t F = from + span - 1;
            if (F > cfg.end) F = cfg.end;
            if (fixed + (F - known_p) / MRZ_MIN_MATCH > cfg.ev_cap) {
                if (launched > retired) return st;  // wait for the oldest launch: S moves on
                if (known_events > ev_base) {       // nothing in flight: encode what the list holds and empty it
                    st.what = MRZ_PLAN_DRAIN;
                    return st;
                }
                // Nothing in flight and nothing to drain: shorten the pass to what fits.  No stall: here v + 1 >= the
                // start of the pass after S less one pass at most (v is lim, or p behind a match, or p with scan_next
                // taken back to its tile -- from is v + 1 or a tile start <= v + 1, or at most pass_cap beyond), so
                // the room left is 31 x (ev_cap - 4) + 30 - pass_cap >= 31 x ev_cap / 2 - 94 positions: more than one
                // tile for every capacity >= MRZ_EVENT_MIN.
                const int64_t fit = (cfg.ev_cap - fixed) * MRZ_MIN_MATCH + MRZ_MIN_MATCH - 1 - (from - 1 - known_p);
                if (fit < MRZ_TILE) {  // (cannot happen, see above)
                    st.what = MRZ_PLAN_FAIL;
                    return st;
                }
                if (span > fit) span = fit / MRZ_TILE * MRZ_TILE;
                max_tiles = span / MRZ_TILE;
            }
        }
        if (launched - retired > max_lag) max_lag = launched - retired;  // (this launch is planned on news that old)
        st.engine = engine();
        if (!cfg.provider) {
            st.what = MRZ_PLAN_PASS;
            st.span = span;
            st.max_tiles = max_tiles;
            return st;
        }
        // window sharding: the stretch's owner scans it (with the mask this rank has last heard of); the host drives
        // the geometry here, and hands it to the sequencer through the matcher state
        st.what = MRZ_PLAN_STRETCH;
        st.seg_start = start;
        if (start > cfg.end)  // (the matcher is about to report the end)
            span = 0;
        else if (start + span > cfg.end + 1)
            span = (cfg.end + 1 - start + MRZ_TILE - 1) / MRZ_TILE * MRZ_TILE;
        st.span = span;
        return st;
    }

    // ---- what the driver has done
    // the provider's answer to a stretch: it ends at nx (the empty stretch: at its own start)
    void stretch_ends(int64_t nx) { known_next = nx; }
    // a sequencer launch over the step's pass or stretch has been queued
    void launch_queued(const mrz_plan_step &st) {
        span_of[launched % MRZ_SEG_AHEAD] = st.what == MRZ_PLAN_PASS ? st.span : 0;
        if (st.engine == MRZ_ENGINE_NARROW) n_narrow++;
        if (st.engine == MRZ_ENGINE_DEEP) n_deep++;
        launched++;
    }
    // the list has been encoded up to the last retired launch's matches and emptied
    void drained() { ev_base = known_events; }
};
