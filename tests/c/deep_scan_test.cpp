// tests/c/deep_scan_test.cpp -- TEST: the deep engine's walk of one run by one wave (mrz_deep_scan, mrz_seq_deep.hip),
// as built -- the next group's loads ahead of the fold, quiet groups passed with one ballot -- against the same function
// compiled with -DMRZ_DEEP_SCAN_NO_AHEAD -DMRZ_DEEP_SCAN_NO_QUIET (every group loaded when its turn has come, every block
// folded), on hand-built tables.  A plain program with its own main; the engine source is compiled against tests/emu.
//
// Two translation units from this one file (tests/test_deep_scan_walk.py builds and runs it, with MRZ_DEEP_GROUP 2 and 8):
//   g++ $F -DDST_OLD -DMRZ_DEEP_SCAN_NO_AHEAD -DMRZ_DEEP_SCAN_NO_QUIET -c deep_scan_test.cpp -o old.o
//   g++ $F -c deep_scan_test.cpp -o new.o && g++ $F old.o new.o -o deep_scan_test
//   F = -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/emu -Imodern-rzip_amd/csrc -DMRZ_DEEP_GROUP=2 + DST_EMU_FLAGS
//
// What a case is: a table of 4096-16384 slots with a background of filled and empty stretches, and in it ONE run built for
// a tag t: `len` occupied slots from t's home slot (1 to 40 groups of it; over the table's end where the home slot lies
// late), then the first empty slot -- at every position of a block, in the first and the last block of a group -- and
// sometimes a second one behind it.  The run's entries are passed by t's walk (not due, not lower-ranked, another tag)
// except the ones placed: tag-equal entries (none, a few, more than MRZ_SMAX, exactly max_chain, max_chain - 1; anywhere,
// or all of them in the run's last groups, so that the chain limit is reached late), a first due or lower-ranked entry
// (in group 0, in a late group, nowhere), a second stop behind a due one (the search for the alternative stop ends in a
// later group), lower-ranked occupants whose own walk starts anywhere in the table (displacement), all-ones tags.  Every
// case is scanned from the start, then taken up again as a CONTINUATION (from > 0) at the slot it wanted, at its first
// empty slot or anywhere in the run -- inside groups that the full scan passed --, with that slot rewritten or not.
// After each call every field of the lane's record is compared between the two builds.
//
// The emulator's scheduler (emu_runtime.cpp) takes two context switches with a signal-mask system call each per lane and
// collective: far too slow for 20,000 walks.  This program brings its own: one wave, the lanes hand the processor on in
// lane order at every collective (64 switches, a few nanoseconds each on x86-64; swapcontext elsewhere).
#include <hip/hip_runtime.h>
#include <stdio.h>

#ifdef DST_OLD
#define mrz_seq_deep_kernel dst_old_seq_deep_kernel
#define mrz_launch_sequencer_deep dst_old_launch_sequencer_deep
#define mrz_seq_deep_shared_size dst_old_seq_deep_shared_size
#endif
#include "mrz_seq_deep.hip"

struct dst_call {
    const mrz_cfg *C;
    void *S;
    int i, xw_n, from;
    int64_t better, tag_mask, clean_ptr;
};

#ifdef DST_OLD
void dst_scan_old(const dst_call *c) {
    mrz_deep_scan(*c->C, (mrz_deep_lds *)c->S, c->i, c->better, c->tag_mask, c->clean_ptr, c->xw_n, (int)threadIdx.x & 63, c->from);
}
#else
void dst_scan_old(const dst_call *c);
static void dst_scan_new(const dst_call *c) {
    mrz_deep_scan(*c->C, (mrz_deep_lds *)c->S, c->i, c->better, c->tag_mask, c->clean_ptr, c->xw_n, (int)threadIdx.x & 63, c->from);
}

// ---- one wave of 64 lanes ------------------------------------------------------------------------------------------------
// Lane k runs to its next collective, leaves its contribution and hands on to lane k + 1; lane 63 hands on to lane 0,
// which finds the collective complete.  Results are double-buffered by the parity of the lane's own collective count: a
// lane reads collective c when it is resumed, and lane 0 can only reach collective c + 2 (same parity) after every lane
// has left its contribution to c + 1, that is after every lane has read c.
#if defined(__x86_64__)
extern "C" void dst_switch(void **save_sp, void *to_sp);
asm(".text\n.globl dst_switch\n.type dst_switch,@function\ndst_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n  movq %rsi, %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n  ret\n"
    ".size dst_switch, .-dst_switch\n");
typedef void *dst_ctx;
static void dst_ctx_switch(dst_ctx *from, dst_ctx *to) { dst_switch(from, *to); }
static void dst_ctx_make(dst_ctx *c, char *stack, size_t size, void (*entry)()) {
    void **top = (void **)(((uintptr_t)stack + size) & ~(uintptr_t)15);
    *--top = nullptr;         // (the entry never returns)
    *--top = (void *)entry;   // dst_switch's `ret` lands here: at a 16-byte boundary, as at any call
    for (int k = 0; k < 6; k++) *--top = nullptr;
    *c = (void *)top;
}
#else
typedef ucontext_t dst_ctx;
static void dst_ctx_switch(dst_ctx *from, dst_ctx *to) { swapcontext(from, to); }
static void dst_ctx_make(dst_ctx *c, char *stack, size_t size, void (*entry)()) {
    getcontext(c);
    c->uc_stack.ss_sp = stack;
    c->uc_stack.ss_size = size;
    c->uc_link = nullptr;
    makecontext(c, entry, 0);
}
#endif

static dst_ctx g_main, g_lane[64];
static int g_cur;  // the lane that runs
static uint64_t g_count[64];
static unsigned long long g_bal[2];
static int g_slot[2][64];
static void (*g_body)(const dst_call *);
static const dst_call *g_arg;

static void dst_hand_on() {
    const int me = g_cur, nx = (me + 1) & 63;
    g_cur = nx;
    emu::cur_tid.x = (unsigned)nx;
    dst_ctx_switch(&g_lane[me], &g_lane[nx]);
}
static void dst_lane_main() {
    for (;;) {
        g_body(g_arg);
        const int me = g_cur;
        if (me == 63) {
            dst_ctx_switch(&g_lane[63], &g_main);
        } else
            dst_hand_on();  // (resumed when the next walk begins)
    }
}
static void dst_run_wave(void (*body)(const dst_call *), const dst_call *arg) {
    g_body = body;
    g_arg = arg;
    g_cur = 0;
    emu::cur_tid.x = 0;
    dst_ctx_switch(&g_main, &g_lane[0]);
    for (int k = 1; k < 64; k++)
        if (g_count[k] != g_count[0]) {
            fprintf(stderr, "deep_scan_test: the lanes took different numbers of collectives\n");
            exit(1);
        }
}

namespace emu {
Fiber *cur = nullptr;
Idx cur_tid = {0, 0, 0}, cur_bid = {0, 0, 0}, cur_bdim = {64, 1, 1}, cur_gdim = {1, 1, 1};
unsigned long long ballot(int pred) {
    const int par = (int)(g_count[g_cur]++ & 1);
    if (g_cur == 0) g_bal[par] = 0;
    if (pred) g_bal[par] |= 1ull << g_cur;
    dst_hand_on();
    return g_bal[par];
}
int shfl(int v, int src) {
    const int par = (int)(g_count[g_cur]++ & 1);
    g_slot[par][g_cur] = v;
    dst_hand_on();
    return g_slot[par][src & 63];
}
int shfl_xor(int v, int mask) {
    const int me = g_cur;
    return shfl(v, me ^ mask);
}
int first_live_lane() { return 0; }
static void not_here(const char *what) {
    fprintf(stderr, "deep_scan_test: %s is not part of a walk\n", what);
    abort();
}
void syncthreads() { not_here("__syncthreads"); }
void yield() { not_here("a spin-wait"); }
void request_coresident() {}
void launch(dim3, dim3, const std::function<void()> &) { not_here("a kernel launch"); }
}  // namespace emu

// ---- cases -----------------------------------------------------------------------------------------------------------------
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }  // [lo, hi]
static bool one_in(int n) { return rnd() % (uint64_t)n == 0; }
static uint64_t ones(int k) { return k >= 64 ? ~0ull : ((1ull << k) - 1ull); }
// a tag with exactly `r` trailing ones (r < 64)
static int64_t tag_with(int r) { return (int64_t)(((rnd() << 1) << r) | ones(r)); }

#define DST_BUF (1 << 16)
static uint8_t g_buf[DST_BUF + 64];
static mrz_slot *g_tab, *g_base[3];
static mrz_deep_lds *g_S[2];  // [0] the build under test, [1] the plain loop
static char g_what[512];

#define FAIL(...)                                   \
    do {                                            \
        fprintf(stderr, "deep_scan_test: ");        \
        fprintf(stderr, __VA_ARGS__);               \
        fprintf(stderr, "\n  in %s\n", g_what);     \
        exit(1);                                    \
    } while (0)

static void compare_records(int i, const char *when) {
    const mrz_deep_recs &a = g_S[0]->R, &b = g_S[1]->R;
#define SAME(f)                                                                                                         \
    if (a.f[i] != b.f[i]) FAIL("%s: %s differs: %lld (as built) != %lld (plain loop)", when, #f, (long long)a.f[i], (long long)b.f[i])
    SAME(h); SAME(fe); SAME(w); SAME(kind); SAME(h2); SAME(w2); SAME(kind2); SAME(occ_t); SAME(occ_off); SAME(old_t);
    SAME(old_t2); SAME(alt_w); SAME(alt_kind); SAME(alt_old_t); SAME(nsame); SAME(flags); SAME(cp_scan); SAME(xw_seen);
#undef SAME
    for (int k = 0; k < (int)a.nsame[i]; k++) {
        if (a.same_slot[i][k] != b.same_slot[i][k] || a.same_off[i][k] != b.same_off[i][k] || a.raw[i][k] != b.raw[i][k])
            FAIL("%s: tag-equal entry %d differs: slot %d off %lld raw %u != slot %d off %lld raw %u", when, k, a.same_slot[i][k],
                 (long long)a.same_off[i][k], a.raw[i][k], b.same_slot[i][k], (long long)b.same_off[i][k], b.raw[i][k]);
    }
}

struct dst_cover {
    long cases, conts, groups_max, long_runs, wraps, evict_late, many_same, displaced, displaced_walked, alt_later, over, empty,
        none, cplx, cont_kept, cont_inside, fe_pos[64], fe_first_block, fe_last_block, all_ones;
};
static dst_cover g_cov;

static void both(const dst_call &c0, const char *when) {
    dst_call c = c0;
    c.S = g_S[0];
    dst_run_wave(dst_scan_new, &c);
    c.S = g_S[1];
    dst_run_wave(dst_scan_old, &c);
    compare_records(c.i, when);
}

static void one_case(long no) {
    const int GS = 64 * MRZ_DEEP_GROUP;
    const int tsel = rnd_in(0, 2);
    const int hash_bits = 12 + tsel, nslots = 1 << hash_bits, smask = nslots - 1;
    g_tab = g_base[tsel];
    // masks: tag_mask = kb ones, better = kb .. kb + 2 ones
    const int kb = rnd_in(2, 8), nbetter = kb + rnd_in(0, 2);
    const int64_t tag_mask = (int64_t)ones(kb), better = (int64_t)ones(nbetter);
    // the tag: an inserter mostly, ranked so that lower-ranked entries exist
    // (one in 50 with more than 32 trailing ones: the bits that rank an entry below t reach into the tag's high word)
    int r_t = one_in(8) ? rnd_in(0, kb - 1) : one_in(50) ? rnd_in(33, 40) : rnd_in(kb, nbetter + 6);
    const bool late_home = one_in(6);  // the home slot lies just before the table's end: the run goes over it
    int64_t t;
    if (one_in(400)) {
        t = -1;
        r_t = 64;
        g_cov.all_ones++;
    } else {
        t = tag_with(r_t);
        if (late_home && r_t + 1 < hash_bits) {  // home slot = low hash_bits of t: the bits above the trailing ones set, but a few
            const uint64_t hi = ((uint64_t)smask & ~ones(r_t + 1)) & ~((uint64_t)rnd_in(0, 15) << (r_t + 1));
            t = (int64_t)(((uint64_t)t & ~(uint64_t)smask) | hi | ones(r_t));
        }
    }
    const int h = (int)(t & smask);
    // the run: 1 .. 40 groups (as many as the table holds), the first empty slot anywhere in its last block
    const int gmax = (nslots - 2 * GS) / GS < 40 ? (nslots - 2 * GS) / GS : 40;
    int ngroups = one_in(8) ? rnd_in(1, gmax) : one_in(2) ? rnd_in(1, 3) : rnd_in(2, 6 < gmax ? 6 : gmax);
    const int last_block = one_in(3) ? 0 : one_in(2) ? MRZ_DEEP_GROUP - 1 : rnd_in(0, MRZ_DEEP_GROUP - 1);
    const int fe_in_block = (int)(no % 64);  // every position in turn
    const int len = (ngroups - 1) * GS + last_block * 64 + fe_in_block;  // occupied slots before the first empty one
    const bool fe2 = one_in(3);
    const int64_t q = rnd_in(64, DST_BUF - 1);
    const int max_chain_tab[8] = {1, 2, 3, 4, 6, 16, 32, 128};
    const int max_chain = max_chain_tab[rnd_in(0, 7)];
    // save what the run overwrites (and a little behind it, for the continuation's store)
    const int region = len + 4;
    static mrz_slot saved[40 * 64 * 8 + 64 * 8 + 8];
    for (int p = 0; p < region; p++) saved[p] = g_tab[(h + p) & smask];
    // an entry t's walk passes: every bit of `better`, at least t's trailing ones (nothing ranks below all ones), another tag
    const int pass_ones = r_t >= 62 ? nbetter : r_t > nbetter ? r_t : nbetter;
    auto passive = [&]() {
        mrz_slot e;
        do e.t = tag_with(rnd_in(pass_ones, pass_ones + 3));
        while (e.t == t);
        e.off = (int64_t)rnd_in(0, DST_BUF - 1);
        return e;
    };
    for (int p = 0; p < len; p++) g_tab[(h + p) & smask] = passive();
    mrz_slot none;
    none.off = 0;
    none.t = 0;
    g_tab[(h + len) & smask] = none;
    if (fe2) g_tab[(h + len + 1) & smask] = none;
    // where a placed entry goes: 0 anywhere, 1 group 0, 2 the last groups
    auto place = [&](int mode) {
        if (len == 0) return -1;
        if (mode == 1) return rnd_in(0, (len < GS ? len : GS) - 1);
        if (mode == 2) return rnd_in(len > 2 * GS ? len - 2 * GS : 0, len - 1);
        return rnd_in(0, len - 1);
    };
    auto put = [&](int p, int64_t tag) {
        if (p < 0) return;
        mrz_slot e;
        e.t = tag;
        e.off = (int64_t)rnd_in(0, DST_BUF - 1);
        if ((e.off | e.t) == 0) e.off = 1;
        g_tab[(h + p) & smask] = e;
    };
    // tag-equal entries
    {
        const int pick = rnd_in(0, 9);
        int n = pick < 3 ? 0 : pick == 3 ? 1 : pick == 4 ? rnd_in(2, 5) : pick == 5 ? MRZ_SMAX + rnd_in(1, 4) : pick == 6 ? max_chain
                : pick == 7 ? max_chain - 1 : pick == 8 ? rnd_in(1, 40) : max_chain + 1;
        if (n > len) n = len;
        const int mode = rnd_in(0, 2);
        for (int k = 0; k < n; k++) put(place(mode == 1 ? 0 : mode), t);
        if (n > MRZ_SMAX) g_cov.many_same++;
    }
    // stops of the insert's walk: due entries (lack a bit of `better`) and lower-ranked ones (fewer trailing ones than t)
    auto due_tag = [&]() { return nbetter > 0 ? tag_with(rnd_in(0, nbetter - 1)) : tag_with(0); };
    auto low_tag = [&]() { return r_t > nbetter ? tag_with(rnd_in(nbetter, (r_t > 63 ? 63 : r_t) - 1)) : due_tag(); };
    {
        const int first = rnd_in(0, 5);  // 0, 1: nowhere; 2: group 0; 3, 4: late; 5: anywhere
        if (first >= 2) {
            const int p1 = place(first == 2 ? 1 : first == 5 ? 0 : 2);
            const bool due = one_in(2);
            put(p1, due ? due_tag() : low_tag());
            if (p1 >= 0 && one_in(2) && p1 + 1 < len) {  // a second stop behind the first: in the same block, or groups later
                const int hi = one_in(3) && p1 + 63 < len - 1 ? p1 + 63 : len - 1;
                put(rnd_in(p1 + 1, hi), one_in(2) ? due_tag() : low_tag());
            }
        }
        if (one_in(10))
            for (int k = rnd_in(1, 6); k > 0; k--) put(place(0), one_in(2) ? due_tag() : low_tag());
        if (one_in(50)) put(place(0), -1);
    }
    mrz_cfg C;
    memset(&C, 0, sizeof(C));
    C.buf = g_buf;
    C.tab = g_tab;
    C.end = DST_BUF;
    C.max_chain = max_chain;
    C.slot_mask = smask;
    C.nslots = nslots;
    C.limit = nslots / 3 * 2;
    dst_call c;
    c.C = &C;
    c.S = nullptr;
    c.i = rnd_in(0, MRZ_DEEP_LANES - 1);
    c.xw_n = rnd_in(0, MRZ_DEEP_XW);
    c.from = 0;
    c.better = better;
    c.tag_mask = tag_mask;
    c.clean_ptr = (int64_t)rnd_in(0, smask);
    snprintf(g_what, sizeof(g_what),
             "case %ld: MRZ_DEEP_GROUP %d, %d slots, t %#llx (home %d, %d trailing ones), tag_mask %d bits, better %d bits, max_chain %d, "
             "%d occupied slots (%d groups)%s, lane %d",
             no, MRZ_DEEP_GROUP, nslots, (unsigned long long)t, h, r_t, kb, nbetter, max_chain, len, ngroups, fe2 ? " + 2 empty" : "", c.i);
    // both builds start from the same (arbitrary) state of the records
    for (size_t k = 0; k < sizeof(mrz_deep_recs) / 8; k++) ((uint64_t *)&g_S[0]->R)[k] = rnd();
    g_S[0]->R.q[c.i] = q;
    g_S[0]->R.t[c.i] = t;
    memcpy(&g_S[1]->R, &g_S[0]->R, sizeof(mrz_deep_recs));
    both(c, "full scan");
    // what the case turned out to be
    const mrz_deep_recs &R = g_S[0]->R;
    const int kind = R.kind[c.i], fepos = (R.fe[c.i] - h) & smask, wpos = R.w[c.i] >= 0 ? (R.w[c.i] - h) & smask : -1;
    g_cov.cases++;
    if (ngroups > g_cov.groups_max) g_cov.groups_max = ngroups;
    if (ngroups >= 20) g_cov.long_runs++;
    if (h + len >= nslots) g_cov.wraps++;
    if (fepos == len) {
        g_cov.fe_pos[fe_in_block]++;
        if (last_block == 0) g_cov.fe_first_block++;
        if (last_block == MRZ_DEEP_GROUP - 1) g_cov.fe_last_block++;
    }
    if (R.flags[c.i] & MRZ_DF_CPLX) g_cov.cplx++;
    if (kind == MRZ_DK_EVICT && R.nsame[c.i] > 0 && ((R.same_slot[c.i][0] - h) & smask) >= 2 * GS) g_cov.evict_late++;
    if (kind == MRZ_DK_DISPLACE) {
        g_cov.displaced++;
        if (R.w2[c.i] >= 0 && ((R.w2[c.i] - R.h2[c.i]) & smask) >= 64) g_cov.displaced_walked++;
    }
    if (kind == MRZ_DK_OVER) {
        g_cov.over++;
        if (R.alt_w[c.i] >= 0 && ((R.alt_w[c.i] - h) & smask) / GS > wpos / GS) g_cov.alt_later++;
    }
    if (kind == MRZ_DK_EMPTY) g_cov.empty++;
    if (kind == MRZ_DK_NONE) g_cov.none++;
    // the continuation: taken up at the slot the insert wanted, at the first empty slot, or anywhere before it
    for (int rep = 0; rep < 2; rep++) {
        const int pick = rnd_in(0, 3);
        int from = pick == 0 && wpos > 0 ? wpos : pick == 1 && fepos > 0 ? fepos : fepos > 0 ? rnd_in(1, fepos) : 0;
        if (from <= 0) break;
        // what an earlier lane of the batch may have done there: taken the slot with a tag this walk passes
        if (one_in(2)) g_tab[(h + from) & smask] = passive();
        c.from = from;
        c.xw_n = rnd_in(0, MRZ_DEEP_XW);
        c.clean_ptr = (int64_t)rnd_in(0, smask);
        const int k0 = g_S[0]->R.kind[c.i], f0 = g_S[0]->R.flags[c.i];
        const bool taken_up = !(f0 & MRZ_DF_CPLX) && k0 != MRZ_DK_EVICT && k0 != MRZ_DK_DISPLACE && from <= ((g_S[0]->R.fe[c.i] - h) & smask);
        char when[64];
        snprintf(when, sizeof(when), "continuation %d from %d", rep, from);
        both(c, when);
        g_cov.conts++;
        if (taken_up) {
            if (wpos >= 0 && wpos < from) g_cov.cont_kept++;
            if (from >= GS && from % GS != 0) g_cov.cont_inside++;
        }
        const mrz_deep_recs &R2 = g_S[0]->R;
        if (R2.flags[c.i] & MRZ_DF_CPLX) break;
    }
    // the table as it was
    for (int p = 0; p < region; p++) g_tab[(h + p) & smask] = saved[p];
}

int main(int argc, char **argv) {
    long cases = 20000;
    for (int a = 1; a + 1 < argc; a += 2) {
        if (!strcmp(argv[a], "--cases")) cases = atol(argv[a + 1]);
        if (!strcmp(argv[a], "--seed")) g_rng ^= (uint64_t)atoll(argv[a + 1]) * 0x9e3779b97f4a7c15ull;
    }
    static char stacks[64][64 * 1024] __attribute__((aligned(64)));
    for (int k = 0; k < 64; k++) dst_ctx_make(&g_lane[k], stacks[k], sizeof(stacks[k]), dst_lane_main);
    for (int k = 0; k < DST_BUF + 64; k++) g_buf[k] = (uint8_t)("abab\0c"[rnd() % 6]);  // (few symbols: the 64-byte probes find something)
    for (int s = 0; s < 2; s++) g_S[s] = (mrz_deep_lds *)calloc(1, sizeof(mrz_deep_lds));
    // the tables' background: filled stretches of 1 .. 300 slots with arbitrary tags, empty stretches of 1 .. 20
    for (int ts = 0; ts < 3; ts++) {
        const int n = 4096 << ts;
        g_base[ts] = (mrz_slot *)calloc((size_t)n, sizeof(mrz_slot));
        for (int s = 0; s < n;) {
            for (int k = rnd_in(1, 300); k > 0 && s < n; k--, s++) {
                g_base[ts][s].t = tag_with(rnd_in(0, 20));
                g_base[ts][s].off = (int64_t)rnd_in(1, DST_BUF - 1);
            }
            s += rnd_in(1, 20);
        }
    }
    for (long no = 0; no < cases; no++) one_case(no);
    const dst_cover &v = g_cov;
    printf("deep_scan_test: MRZ_DEEP_GROUP %d: %ld cases + %ld continuations (%ld with the insert's place kept, %ld taken up inside a later "
           "group); up to %ld groups, %ld runs of 20 or more; %ld over the table's end; %ld evictions whose first tag-equal entry lies "
           "behind group 1; %ld with more than MRZ_SMAX tag-equal entries; %ld displacements (%ld with an occupant's walk of more than a "
           "block); %ld due stops (%ld with the alternative stop in a later group); %ld empty; %ld look-ups only; %ld complex; first empty "
           "slot in a group's first / last block %ld / %ld; %ld all-ones tags\n",
           MRZ_DEEP_GROUP, v.cases, v.conts, v.cont_kept, v.cont_inside, v.groups_max, v.long_runs, v.wraps, v.evict_late, v.many_same, v.displaced,
           v.displaced_walked, v.over, v.alt_later, v.empty, v.none, v.cplx, v.fe_first_block, v.fe_last_block, v.all_ones);
    if (cases >= 5000) {  // the generator reaches what it is meant to reach
        bool ok = v.groups_max >= (MRZ_DEEP_GROUP <= 2 ? 40 : 20) && v.long_runs && v.wraps && v.evict_late && v.many_same && v.displaced &&
                  v.displaced_walked && v.over && v.alt_later && v.empty && v.none && v.cont_kept && v.cont_inside && v.fe_first_block &&
                  v.fe_last_block;
        for (int k = 0; k < 64; k++) ok = ok && v.fe_pos[k] > 0;
        if (!ok) {
            fprintf(stderr, "deep_scan_test: a kind of case was never generated\n");
            return 1;
        }
    }
    printf("deep_scan_test ok\n");
    return 0;
}
#endif  // !DST_OLD
