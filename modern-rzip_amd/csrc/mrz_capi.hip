// mrz_capi.hip -- the C-ABI layer of libmrzgpu.so (include/mrzgpu.h): context
// and device-buffer management, chunk orchestration (HIP stream of launches),
// nothing else.  Host code only; the kernels live in the other .hip files.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mrzgpu.h"
#include "mrz_chunk_plan.h"
#include "mrz_ctx.h"
#include "mrz_seq_stats.h"



// levels[] rows {mb_used, initial_freq, max_chain_len}, src/rzip.c:65-73
static const unsigned k_levels[10][3] = { { 1, 4, 1 },  { 2, 4, 2 },  { 4, 4, 2 },   { 8, 4, 2 },   { 16, 4, 3 },
                                          { 32, 4, 4 }, { 32, 2, 6 }, { 64, 1, 16 }, { 64, 1, 32 }, { 64, 1, 128 } };

// init_hash_indexes (src/rzip.c:669-673): (random() << 16) ^ random() from
// glibc's TYPE_3 additive-feedback generator at its default seed 1, computed
// here so the table does not depend on what else the host process did with
// random().
static void mrz_make_hash_index(int64_t H[256]) {
    int32_t r[31];
    int32_t word = 1;
    r[0] = 1;
    for (int i = 1; i < 31; i++) {
        const long hi = word / 127773, lo = word % 127773;
        long w = 16807 * lo - 2836 * hi;
        if (w < 0) w += 2147483647;
        r[i] = word = (int32_t)w;
    }
    int f = 3, b = 0;
    uint32_t draw[512];
    for (int k = -310; k < 512; k++) {
        const uint32_t s = (uint32_t)r[f] + (uint32_t)r[b];
        r[f] = (int32_t)s;
        if (++f == 31) f = 0;
        if (++b == 31) b = 0;
        if (k >= 0) draw[k] = s >> 1;
    }
    for (int i = 0; i < 256; i++) H[i] = ((int64_t)draw[2 * i] << 16) ^ (int64_t)draw[2 * i + 1];
}

extern "C" int mrz_abi_version(void) { return MRZ_ABI_VERSION; }

// Room for the emitted matches of a chunk of n bytes (24 B each).  Matches are >= 31 bytes and disjoint, so n / 31 + 2
// always suffices -- 53 GB for a 64 GiB chunk, more than the chunk for a 256 GiB window.  Beyond MRZ_EVENT_CAP entries
// (6.4 GB: one match per 256 bytes of a 64 GiB chunk; text emits one per ~400 bytes, the tar mix one per 500 KB) the
// list is bounded instead, and mrz_rzip_chunk encodes it in pieces whenever it runs short of room (the room rule
// there).  mrz_set_event_capacity / MRZ_EVENT_CAPACITY set the bound by hand (MRZ_EVENT_MIN at least).
#define MRZ_EVENT_CAP (1ll << 28)
#define MRZ_EVENT_MIN 1024ll
#define MRZ_EVENT_MAX (1ll << 31)
static int64_t mrz_event_room(const mrz_ctx *ctx, int64_t n) {
    if (ctx->event_cap_set > 0) return ctx->event_cap_set;
    const int64_t worst = n / MRZ_MIN_MATCH + 2;
    return worst < MRZ_EVENT_CAP ? worst : MRZ_EVENT_CAP;
}

extern "C" const char *mrz_strerror(int code) {
    switch (code) {
        case MRZ_OK: return "ok";
        case MRZ_E_ARG: return "bad argument";
        case MRZ_E_NODEVICE: return "no usable HIP device (libmrzgpu has no CPU fallback)";
        case MRZ_E_NOMEM: return "out of memory";
        case MRZ_E_HIP: return "HIP runtime error";
        case MRZ_E_OVERFLOW: return "internal capacity exceeded";
        case MRZ_E_STATE: return "call order violated";
        case MRZ_E_CORRUPT: return "corrupt record stream or archive";
        case MRZ_E_UNSUPPORTED: return "block type not handled on this path (back-end codecs are host code)";
        default: return "unknown error";
    }
}

extern "C" int mrz_last_hip_error(const mrz_ctx *ctx, const char **text) {
    if (!ctx) return 0;
    if (text) *text = hipGetErrorString(ctx->last_err);
    return (int)ctx->last_err;
}

extern "C" int mrz_chunk_bytes(int64_t chunk_size) {
    int bits = 8;
    while (chunk_size >> bits > 0) bits++;
    return bits / 8 + (bits % 8 ? 1 : 0);
}

extern "C" void mrz_close(mrz_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    hipFree(ctx->d_index);
    hipFree(ctx->d_tab);
    hipFree(ctx->d_state);
    if (ctx->h_ring) hipHostFree(ctx->h_ring);
    hipFree(ctx->d_fe_hdr);
    hipFree(ctx->d_bitmap);
    hipFree(ctx->d_tile_cnt);
    hipFree(ctx->d_tile_off);
    hipFree(ctx->d_grp_cnt);
    hipFree(ctx->d_cand);
    hipFree(ctx->d_events);
    hipFree(ctx->d_block_s0);
    hipFree(ctx->d_block_s1);
    hipFree(ctx->d_lit_off);
    hipFree(ctx->d_totals);
    hipFree(ctx->d_s0);
    hipFree(ctx->d_s1);
    hipFree(ctx->d_in);
    hipFree(ctx->d_crc_tables);
    hipFree(ctx->d_crc_parts);
    hipFree(ctx->d_crc_out);
    if (ctx->d_gmailbox) hipFree(ctx->d_gmailbox);
    if (ctx->d_seq_shared) hipFree(ctx->d_seq_shared);
    if (ctx->d_deep_shared) hipFree(ctx->d_deep_shared);
    if (ctx->d_wlog) hipFree(ctx->d_wlog);
    if (ctx->rz_scratch) hipFree(ctx->rz_scratch);
    if (ctx->d_rz_out) hipFree(ctx->d_rz_out);
    if (ctx->d_rz_done) hipFree(ctx->d_rz_done);
    if (ctx->seg_tab) hipFree(ctx->seg_tab);
    if (ctx->d_rs_tables) hipFree(ctx->d_rs_tables);
    if (ctx->d_rs_out) hipFree(ctx->d_rs_out);
    if (ctx->d_rs_dec) hipFree(ctx->d_rs_dec);
    if (ctx->d_rs_lost) hipFree(ctx->d_rs_lost);
    if (ctx->lz4_scratch) hipFree(ctx->lz4_scratch);
    if (ctx->b2_scratch) hipFree(ctx->b2_scratch);
    if (ctx->side_stream) hipStreamDestroy(ctx->side_stream);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    free(ctx);
}

extern "C" int mrz_open(mrz_ctx **out, int device, int level, int64_t max_chunk) {
    if (!out || level < 1 || level > 9 || max_chunk < 0) return MRZ_E_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        fprintf(stderr, "libmrzgpu: hipGetDeviceCount -> %d (%s), %d device(s), asked for %d\n", (int)e0,
                hipGetErrorString(e0), ndev, device);
        return MRZ_E_NODEVICE;
    }
    e0 = hipSetDevice(device);
    if (e0 != hipSuccess) {
        fprintf(stderr, "libmrzgpu: hipSetDevice(%d) -> %d (%s)\n", device, (int)e0, hipGetErrorString(e0));
        return MRZ_E_NODEVICE;
    }
    mrz_ctx *ctx = (mrz_ctx *)calloc(1, sizeof(mrz_ctx));
    if (!ctx) return MRZ_E_NOMEM;
    ctx->farm_helpers = -1;
    ctx->seg_positions = MRZ_SEG_POSITIONS;
    ctx->cand_cap = MRZ_CAND_CAP;
    // diagnostics / test knobs, read once per ctx: never per chunk
    {
        const char *e = getenv("MRZ_SEQ_ENGINE");
        if (e && !strcmp(e, "wide")) ctx->engine_pin = 1;
        if (e && !strcmp(e, "narrow")) ctx->engine_pin = 2;
        if (e && !strcmp(e, "deep")) ctx->engine_pin = 3;
        ctx->deep_min_bits = 6;
        if (const char *d = getenv("MRZ_DEEP_MIN_BITS")) ctx->deep_min_bits = atoi(d);
        // (at deep masks the narrow engine's one-wave table walks cost 70 us per candidate: stride-64G 20.2 s with it,
        // 8.1 s when those segments go to the deep engine too; rep64k-10G, whose mask stays below, is unchanged)
        ctx->narrow_max_bits = ctx->deep_min_bits;
        if (const char *d = getenv("MRZ_NARROW_MAX_BITS")) ctx->narrow_max_bits = atoi(d);
        e = getenv("MRZ_PRINT_PROF");
        if (e) ctx->print_prof = !strcmp(e, "narrow") ? 2 : 1;
        if (const char *c = getenv("MRZ_EVENT_CAPACITY")) {  // (as mrz_set_event_capacity; out of range: the default)
            const long long v = atoll(c);
            if (v >= MRZ_EVENT_MIN && v <= MRZ_EVENT_MAX)
                ctx->event_cap_set = v;
            else if (v > 0)
                fprintf(stderr, "libmrzgpu: MRZ_EVENT_CAPACITY=%s ignored (%lld .. %lld entries)\n", c, MRZ_EVENT_MIN,
                        MRZ_EVENT_MAX);
        }
        if (const char *r = getenv("MRZ_RETIRE_SCHEDULE")) {  // (as mrz_set_retire_schedule; malformed: the default)
            const int hold = r[0] - '0';
            const bool one = r[0] && !strcmp(r + 1, ":one"), all = r[0] && !strcmp(r + 1, ":all");
            if (hold >= 1 && hold <= MRZ_SEG_AHEAD && (one || all))
                ctx->retire_hold = hold, ctx->retire_all = all ? 1 : 0;
            else
                fprintf(stderr, "libmrzgpu: MRZ_RETIRE_SCHEDULE=%s ignored (<1..%d>:one or <1..%d>:all)\n", r, MRZ_SEG_AHEAD,
                        MRZ_SEG_AHEAD);
        }
    }
    ctx->farm_default = mrz_sequencer_default_helpers(device);
    ctx->device = device;
    ctx->level = level;
    ctx->mb_used = k_levels[level][0];
    ctx->initial_freq = k_levels[level][1];
    ctx->max_chain = k_levels[level][2];
    // table geometry, src/rzip.c:521-530
    const int64_t want = (int64_t)ctx->mb_used * (1048576 / 16);
    for (ctx->hash_bits = 0; (1ll << ctx->hash_bits) < want; ctx->hash_bits++) {
    }
    ctx->nslots = 1ll << ctx->hash_bits;
    mrz_make_hash_index(ctx->h_index);

    int rc = MRZ_OK;
    e0 = hipStreamCreate(&ctx->stream);
    if (e0 != hipSuccess) {
        fprintf(stderr, "libmrzgpu: hipStreamCreate -> %d (%s)\n", (int)e0, hipGetErrorString(e0));
        rc = MRZ_E_NODEVICE;
    }
    int64_t cap;
    if (!rc) { cap = 0; rc = mrz_grow(ctx, &ctx->d_index, &cap, 256); }
    if (!rc) { cap = 0; rc = mrz_grow(ctx, &ctx->d_tab, &cap, ctx->nslots); }
    if (!rc) { cap = 0; rc = mrz_grow(ctx, &ctx->d_state, &cap, 1); }
    if (!rc && hipHostMalloc((void **)&ctx->h_ring, MRZ_SEG_AHEAD * sizeof(mrz_seq_state)) != hipSuccess) rc = MRZ_E_NOMEM;
    if (!rc) { cap = 0; rc = mrz_grow(ctx, &ctx->d_fe_hdr, &cap, 1); }
    if (!rc) { cap = 0; rc = mrz_grow(ctx, &ctx->d_totals, &cap, 1); }
    if (!rc) { cap = 0; rc = mrz_grow(ctx, &ctx->d_crc_out, &cap, 4); }
    if (!rc) {
        void *p = nullptr;
        if (hipMalloc(&p, mrz_crc_tables_size()) != hipSuccess)
            rc = MRZ_E_NOMEM;
        else
            ctx->d_crc_tables = (mrz_crc_tables *)p;
    }
    if (!rc) {
        mrz_crc_tables *tb = (mrz_crc_tables *)malloc(mrz_crc_tables_size());
        if (!tb)
            rc = MRZ_E_NOMEM;
        else {
            mrz_crc_build_tables(tb);
            if (hipMemcpy(ctx->d_crc_tables, tb, mrz_crc_tables_size(), hipMemcpyHostToDevice) != hipSuccess)
                rc = MRZ_E_HIP;
            free(tb);
        }
    }
    if (!rc && hipMemcpy(ctx->d_index, ctx->h_index, sizeof(ctx->h_index), hipMemcpyHostToDevice) != hipSuccess)
        rc = MRZ_E_HIP;
    const size_t mbox = mrz_sequencer_mailbox_size() > mrz_seq_narrow_mailbox_size() ? mrz_sequencer_mailbox_size()
                                                                                     : mrz_seq_narrow_mailbox_size();
    if (!rc && mbox && !getenv("MRZ_NO_HELPER_WGS")) {
        void *p = nullptr;
        if (hipMalloc(&p, mbox) != hipSuccess)
            rc = MRZ_E_NOMEM;
        else
            ctx->d_gmailbox = p;
    }
    if (!rc) {
        if (hipMalloc(&ctx->d_seq_shared, mrz_sequencer_shared_size()) != hipSuccess ||
            hipMalloc((void **)&ctx->d_wlog, mrz_sequencer_wlog_size(ctx->nslots)) != hipSuccess)
            rc = MRZ_E_NOMEM;
        ctx->seq_wgs = 3;
        if (const char *e = getenv("MRZ_SEQ_WGS")) ctx->seq_wgs = atoi(e);
        if (hipMalloc(&ctx->d_deep_shared, mrz_seq_deep_shared_size()) != hipSuccess) rc = MRZ_E_NOMEM;
        ctx->deep_scanners = 63;
        if (const char *e = getenv("MRZ_DEEP_SCANNERS")) ctx->deep_scanners = atoi(e);
    }
    if (!rc && max_chunk > 0) {
        rc = mrz_grow(ctx, &ctx->d_events, &ctx->event_cap, mrz_event_room(ctx, max_chunk));
        if (!rc) rc = mrz_grow(ctx, &ctx->d_crc_parts, &ctx->crc_parts_cap, mrz_crc32_parts_needed(max_chunk));
        if (!rc) rc = mrz_fe_reserve(ctx, max_chunk / MRZ_TILE + 2, max_chunk);
    }
    if (rc) {
        mrz_close(ctx);
        return rc;
    }
    *out = ctx;
    return MRZ_OK;
}

extern "C" void *mrz_stream(const mrz_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int mrz_synchronize(mrz_ctx *ctx) {
    if (!ctx) return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MRZ_OK;
}

extern "C" int mrz_set_profiling(mrz_ctx *ctx, int enable) {
    if (!ctx) return MRZ_E_ARG;
    ctx->profiling = enable ? 1 : 0;
    return MRZ_OK;
}

extern "C" int mrz_set_progress(mrz_ctx *ctx, mrz_progress_fn fn, void *user) {
    if (!ctx) return MRZ_E_ARG;
    ctx->progress_fn = fn;
    ctx->progress_user = user;
    return MRZ_OK;
}

extern "C" int mrz_fetch_events(mrz_ctx *ctx, int64_t first, int64_t count, mrz_match *host_dst) {
    if (!ctx || first < 0 || count < 0 || (count > 0 && !host_dst)) return MRZ_E_ARG;
    if (first + count > ctx->events_final) return MRZ_E_STATE;
    if (first < ctx->ev_base) return MRZ_E_STATE;  // encoded and dropped from the list (the progress hook saw them)
    if (!count) return MRZ_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    static_assert(sizeof(mrz_match) == sizeof(mrz_event), "mrz_match mirrors mrz_event");
    HIPCHK(ctx, hipMemcpyAsync(host_dst, ctx->d_events + (first - ctx->ev_base), (size_t)count * sizeof(mrz_event), hipMemcpyDeviceToHost,
                               ctx->copy_stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    return MRZ_OK;
}

extern "C" int mrz_set_cand_provider(mrz_ctx *ctx, mrz_cand_provider_fn fn, void *user) {
    if (!ctx) return MRZ_E_ARG;
    ctx->cand_fn = fn;
    ctx->cand_user = user;
    return MRZ_OK;
}

extern "C" int mrz_copy_to_device(mrz_ctx *ctx, void *dst_device, const void *src_host, int64_t n) {
    if (!ctx || n < 0 || (n > 0 && (!dst_device || !src_host))) return MRZ_E_ARG;
    if (!n) return MRZ_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(dst_device, src_host, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the source may be reused on return
    return MRZ_OK;
}

extern "C" int mrz_copy_device(mrz_ctx *ctx, void *dst_device, const void *src_device, int64_t n) {
    if (!ctx || n < 0 || (n > 0 && (!dst_device || !src_device))) return MRZ_E_ARG;
    if (!n) return MRZ_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(dst_device, src_device, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MRZ_OK;
}

extern "C" int mrz_set_segment_positions(mrz_ctx *ctx, int64_t positions) {
    if (!ctx || positions < MRZ_TILE || positions > MRZ_SEG_POSITIONS || positions % MRZ_TILE) return MRZ_E_ARG;
    ctx->seg_positions = positions;
    return MRZ_OK;
}

extern "C" int mrz_set_candidate_capacity(mrz_ctx *ctx, int64_t entries) {
    if (!ctx || entries < MRZ_TILE || entries > (1ll << 30)) return MRZ_E_ARG;
    ctx->cand_cap = entries;
    return MRZ_OK;
}

extern "C" int mrz_set_event_capacity(mrz_ctx *ctx, int64_t entries) {
    if (!ctx || (entries > 0 && entries < MRZ_EVENT_MIN) || entries > MRZ_EVENT_MAX) return MRZ_E_ARG;
    ctx->event_cap_set = entries > 0 ? entries : 0;
    return MRZ_OK;
}

extern "C" int mrz_set_retire_schedule(mrz_ctx *ctx, int hold, int all) {
    if (!ctx || hold > MRZ_SEG_AHEAD || (hold > 0 && all != 0 && all != 1)) return MRZ_E_ARG;
    ctx->retire_hold = hold > 0 ? hold : 0;
    ctx->retire_all = hold > 0 ? all : 0;
    return MRZ_OK;
}

extern "C" int mrz_schedule_info(const mrz_ctx *ctx, int64_t out[4]) {
    if (!ctx || !out) return MRZ_E_ARG;
    memcpy(out, ctx->sched_info, sizeof(ctx->sched_info));
    return MRZ_OK;
}

extern "C" int mrz_set_xcd(mrz_ctx *ctx, int xcd) {
    if (!ctx || xcd < 0 || xcd > 7) return MRZ_E_ARG;
    ctx->xcd = xcd;
    return MRZ_OK;
}

// the front end's buffers: passes of up to `tiles` tiles, lists of up to `entries` candidates
int mrz_fe_reserve(mrz_ctx *ctx, int64_t tiles, int64_t entries) {
    const int64_t max_tiles = ctx->seg_positions / MRZ_TILE;
    if (tiles > max_tiles) tiles = max_tiles;
    if (tiles < 1) tiles = 1;
    if (entries > ctx->cand_cap) entries = ctx->cand_cap;
    if (entries < MRZ_TILE) entries = MRZ_TILE;
    if (tiles > ctx->fe_tiles_cap) {
        int64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        if (ctx->d_bitmap) hipFree(ctx->d_bitmap), ctx->d_bitmap = nullptr;
        if (ctx->d_tile_cnt) hipFree(ctx->d_tile_cnt), ctx->d_tile_cnt = nullptr;
        if (ctx->d_tile_off) hipFree(ctx->d_tile_off), ctx->d_tile_off = nullptr;
        if (ctx->d_grp_cnt) hipFree(ctx->d_grp_cnt), ctx->d_grp_cnt = nullptr;
        ctx->fe_tiles_cap = 0;
        int rc = mrz_grow(ctx, &ctx->d_bitmap, &c0, tiles * (MRZ_TILE / 16) + 64);
        if (!rc) rc = mrz_grow(ctx, &ctx->d_tile_cnt, &c1, tiles + 1);
        if (!rc) rc = mrz_grow(ctx, &ctx->d_tile_off, &c2, tiles + 2);
        if (!rc) rc = mrz_grow(ctx, &ctx->d_grp_cnt, &c3, tiles / MRZ_FE_GROUP + 2);
        if (rc) return rc;
        ctx->fe_tiles_cap = tiles;
    }
    return mrz_grow(ctx, &ctx->d_cand, &ctx->cand_alloc, entries);
}

extern "C" int mrz_window_scan(mrz_ctx *ctx, const void *range_bytes, int64_t range_len, int where, int64_t range_start,
                               int64_t chunk_n, int64_t seg_start, int64_t max_span, int64_t min_mask, int64_t p_done,
                               int64_t cap, mrz_candidate *cand_out, int32_t *tile_off_out, void *bitmap_out, int out_where,
                               int64_t *scan_next, int64_t *n_cand) {
    if (!ctx || !range_bytes || !cand_out || !tile_off_out || !bitmap_out || !scan_next || !n_cand) return MRZ_E_ARG;
    if (range_len <= 0 || range_start < 0 || chunk_n <= 0 || cap < MRZ_TILE) return MRZ_E_ARG;
    if (max_span <= 0 || max_span > ctx->seg_positions || max_span % MRZ_TILE || seg_start % MRZ_TILE || seg_start < range_start)
        return MRZ_E_ARG;
    if (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    // the last position's 31-byte window must lie in the rank's bytes (or the chunk ends first); the kernels stage whole
    // 16-byte pieces: 48 bytes of halo keep every load inside the rank's bytes
    const int64_t end = chunk_n - MRZ_MIN_MATCH;
    int64_t last_pos = seg_start + max_span - 1;
    if (last_pos > end) last_pos = end;
    const int64_t need_end = last_pos + 48 < chunk_n ? last_pos + 48 : chunk_n;
    if (last_pos >= seg_start && need_end > range_start + range_len) return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t *d_range = nullptr;
    int rc = mrz_stage_input(ctx, range_bytes, range_len, where, &d_range);
    if (rc) return rc;
    const int64_t tiles = max_span / MRZ_TILE;
    const int64_t save_cap = ctx->cand_cap;
    if (cap > ctx->cand_cap) ctx->cand_cap = cap;
    rc = mrz_fe_reserve(ctx, tiles, cap);
    ctx->cand_cap = save_cap;
    if (rc) return rc;
    mrz_seq_state hs;
    memset(&hs, 0, sizeof(hs));
    hs.n = chunk_n;
    hs.end = end;
    // (a matcher position inside or beyond the stretch's first tile would move the pass's first tile: the outputs are
    // laid out from seg_start, so such a position is not used as a filter -- the list is a superset then)
    hs.p = p_done + 1 < seg_start + MRZ_TILE ? p_done : seg_start - 1;
    hs.min_mask = min_mask;
    hs.scan_next = seg_start;
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_state, &hs, sizeof(hs), hipMemcpyHostToDevice, s));
    // the kernels index the chunk by absolute position: give them the pointer position 0 would have.  They stay
    // inside [range_start, need_end + 16) of it; the staging buffer is padded by 64 bytes.
    HIPCHK(ctx, mrz_launch_frontend(s, d_range - range_start, chunk_n, ctx->d_index, ctx->d_state, (int)tiles, cap,
                                    ctx->d_fe_hdr, ctx->d_bitmap, ctx->d_tile_cnt, ctx->d_tile_off, ctx->d_grp_cnt, ctx->d_cand));
    HIPCHK(ctx, hipMemcpyAsync(&hs, ctx->d_state, sizeof(hs), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    int64_t T = (hs.scan_next - seg_start) / MRZ_TILE;  // tiles the pass covered (none: the matcher is past the stretch)
    if (hs.seg_start != seg_start || T < 0 || T > tiles) {
        // (p_done lies beyond the stretch: the pass began further on; report the stretch as empty)
        T = 0;
        hs.n_cand = 0;
        hs.scan_next = hs.scan_next > seg_start ? hs.scan_next : seg_start;
    }
    const hipMemcpyKind k = out_where == MRZ_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (hs.n_cand > 0) HIPCHK(ctx, hipMemcpyAsync(cand_out, ctx->d_cand, (size_t)hs.n_cand * sizeof(mrz_cand), k, s));
    if (T > 0) {
        HIPCHK(ctx, hipMemcpyAsync(tile_off_out, ctx->d_tile_off, (size_t)(T + 1) * sizeof(int), k, s));
        HIPCHK(ctx, hipMemcpyAsync(bitmap_out, ctx->d_bitmap, (size_t)T * (MRZ_TILE / 8), k, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    *scan_next = hs.scan_next;
    *n_cand = hs.n_cand;
    return MRZ_OK;
}

extern "C" int mrz_set_farm_helpers(mrz_ctx *ctx, int n) {
    if (!ctx) return MRZ_E_ARG;
    ctx->farm_helpers = n < 0 ? -1 : n;
    return MRZ_OK;
}

extern "C" int mrz_get_timings(const mrz_ctx *ctx, mrz_timings *out) {
    if (!ctx || !out) return MRZ_E_ARG;
    *out = ctx->timings;
    return MRZ_OK;
}

extern "C" int64_t mrz_table_slots(const mrz_ctx *ctx) { return ctx ? ctx->nslots : 0; }

extern "C" int mrz_fetch_table(mrz_ctx *ctx, void *host_dst) {
    if (!ctx || !host_dst) return MRZ_E_ARG;
    if (!ctx->have_chunk) return MRZ_E_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpy(host_dst, ctx->d_tab, (size_t)ctx->nslots * sizeof(mrz_slot), hipMemcpyDeviceToHost));
    return MRZ_OK;
}

// resolves a caller buffer to a device pointer (staging host memory)
int mrz_stage_input(mrz_ctx *ctx, const void *buf, int64_t n, int where, const uint8_t **dev) {
    if (where == MRZ_MEM_DEVICE) {
        *dev = (const uint8_t *)buf;
        return MRZ_OK;
    }
    if (where != MRZ_MEM_HOST) return MRZ_E_ARG;
    int rc = mrz_grow(ctx, &ctx->d_in, &ctx->in_cap, n + 64);
    if (rc) return rc;
    if (n > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->d_in, buf, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    *dev = ctx->d_in;
    return MRZ_OK;
}

extern "C" int mrz_crc32(mrz_ctx *ctx, const void *buf, int64_t n, int where, uint32_t *crc_out) {
    if (!ctx || !crc_out || n < 0 || (n > 0 && !buf)) return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t *d = nullptr;
    int rc = mrz_stage_input(ctx, buf, n, where, &d);
    if (rc) return rc;
    rc = mrz_grow(ctx, &ctx->d_crc_parts, &ctx->crc_parts_cap, mrz_crc32_parts_needed(n));
    if (rc) return rc;
    HIPCHK(ctx, mrz_launch_crc32(ctx->stream, d, n, ctx->d_crc_tables, ctx->d_crc_parts, ctx->d_crc_out));
    HIPCHK(ctx, hipMemcpyAsync(crc_out, ctx->d_crc_out, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MRZ_OK;
}

// HIP event pairs around the stages of a chunk (mrz_set_profiling).  Owns its events: whatever path the call leaves by,
// they are destroyed.
struct mrz_prof_spans {
    struct pair {
        hipEvent_t a, b;
        int kind;  // 0 front end, 1 sequencer, 2 encode, 3 crc
    };
    const bool on;
    const hipStream_t s;
    pair *v = nullptr;
    int n = 0, cap = 0;
    bool open = false;  // v[n] has been begun
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;

    mrz_prof_spans(bool enabled, hipStream_t stream) : on(enabled), s(stream) {
        if (!on) return;
        hipEventCreate(&ev_begin);
        hipEventCreate(&ev_end);
        hipEventRecord(ev_begin, s);
    }
    mrz_prof_spans(const mrz_prof_spans &) = delete;
    ~mrz_prof_spans() {
        for (int i = 0; i < n + (open ? 1 : 0); i++) {
            hipEventDestroy(v[i].a);
            hipEventDestroy(v[i].b);
        }
        free(v);
        if (ev_begin) hipEventDestroy(ev_begin);
        if (ev_end) hipEventDestroy(ev_end);
    }
    void begin(int kind) {
        if (!on) return;
        if (n == cap) {
            const int ncap = cap ? cap * 2 : 64;
            pair *nv = (pair *)realloc(v, (size_t)ncap * sizeof(pair));
            if (nv) v = nv, cap = ncap;
        }
        if (n < cap) {
            v[n].kind = kind;
            hipEventCreate(&v[n].a);
            hipEventCreate(&v[n].b);
            hipEventRecord(v[n].a, s);
            open = true;
        }
    }
    void end() {
        if (!open) return;
        hipEventRecord(v[n].b, s);
        open = false;
        n++;
    }
    void end_total() {
        if (on) hipEventRecord(ev_end, s);
    }
    void collect(mrz_timings *t) {
        if (!on) return;
        hipStreamSynchronize(s);
        for (int i = 0; i < n; i++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, v[i].a, v[i].b) != hipSuccess) continue;
            if (v[i].kind == 0) t->tagscan_ms += ms;
            if (v[i].kind == 1) t->sequencer_ms += ms;
            if (v[i].kind == 2) t->encode_ms += ms;
            if (v[i].kind == 3) t->crc_ms += ms;
        }
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev_begin, ev_end) == hipSuccess) t->total_ms = ms;
    }
};

// one mrz_rzip_chunk call: what its steps share besides the plan
struct mrz_chunk_call {
    mrz_ctx *ctx;
    hipStream_t s;
    const uint8_t *d_buf;
    int64_t n;
    int chunk_bytes;
    hipError_t herr = hipSuccess;  // the first HIP error: sticks, and ends the call with MRZ_E_HIP
    int rc = MRZ_OK;               // ... and the first refusal of any other kind
    mrz_enc_totals tot;
    uint32_t crc = 0;
    int64_t base0 = 0, base1 = 0, lit_from = 0, n_flushes = 0;  // stream bytes so far; first literal of the next piece
    hipEvent_t seg_ev[MRZ_SEG_AHEAD];  // one per ring slot: the launch's snapshot has arrived
    int n_seg_ev = 0;
    mrz_prof_spans prof;

    mrz_chunk_call(mrz_ctx *c, const uint8_t *buf, int64_t bytes, int cb)
        : ctx(c), s(c->stream), d_buf(buf), n(bytes), chunk_bytes(cb), prof(c->profiling != 0, c->stream) {
        memset(&tot, 0, sizeof(tot));
    }
    bool ok() const { return herr == hipSuccess && !rc; }
};
// a HIP call of the chunk in flight: not made once one has failed
#define MRZ_STEP(c, expr)                                  \
    do {                                                   \
        if ((c).herr == hipSuccess) (c).herr = (expr);     \
    } while (0)

// hash_search prologue (src/rzip.c:518-546): zero the table, reset state; the CRC of the chunk; the launches' events
static void mrz_chunk_begin(mrz_chunk_call &c, mrz_seq_state *hs, int64_t victim_round, int64_t ev_cap) {
    mrz_ctx *ctx = c.ctx;
    memset(hs, 0, sizeof(*hs));
    hs->n = c.n;
    hs->end = c.n - MRZ_MIN_MATCH;
    hs->min_mask = hs->tag_mask = (1ll << ctx->initial_freq) - 1;
    hs->limit = ctx->nslots / 3 * 2;
    hs->victim_round = victim_round;
    hs->max_chain = ctx->max_chain;
    hs->slot_mask = ctx->nslots - 1;
    hs->event_cap = ev_cap;
    hs->finished = hs->end > 0 ? 0 : 1;
    MRZ_STEP(c, hipMemsetAsync(ctx->d_tab, 0, (size_t)ctx->nslots * sizeof(mrz_slot), c.s));
    MRZ_STEP(c, hipMemcpyAsync(ctx->d_state, hs, sizeof(*hs), hipMemcpyHostToDevice, c.s));
    MRZ_STEP(c, hipMemsetAsync(ctx->d_totals, 0, sizeof(mrz_enc_totals), c.s));
    c.prof.begin(3);
    MRZ_STEP(c, mrz_launch_crc32(c.s, c.d_buf, c.n, ctx->d_crc_tables, ctx->d_crc_parts, ctx->d_crc_out));
    c.prof.end();
    ctx->events_final = 0;
    ctx->ev_base = 0;
    for (int k = 0; k < MRZ_SEG_AHEAD && c.herr == hipSuccess; k++) {
        MRZ_STEP(c, hipEventCreateWithFlags(&c.seg_ev[k], hipEventDisableTiming));
        if (c.herr == hipSuccess) c.n_seg_ev++;
    }
    memset(ctx->sched_info, 0, sizeof(ctx->sched_info));
}

// ---- pieces: the matches [ctx->ev_base, upto) are encoded into the streams behind what is there and leave the list
// (nothing is in flight: the stream holds only finished launches, and the progress hook has been shown all of them)
static int mrz_encode_piece(mrz_chunk_call &c, int64_t upto, int final_piece) {
    mrz_ctx *ctx = c.ctx;
    const int64_t Ep = upto - ctx->ev_base;
    const int64_t nblocks = (Ep + 1 + 255) / 256;
    int r = mrz_grow(ctx, &ctx->d_block_s0, &ctx->block_cap, nblocks);
    if (!r) r = mrz_grow(ctx, &ctx->d_block_s1, &ctx->block1_cap, nblocks);
    if (!r) r = mrz_grow(ctx, &ctx->d_lit_off, &ctx->lit_off_cap, Ep + 2);
    if (r) return r;
    c.prof.begin(2);
    MRZ_STEP(c, mrz_launch_enc_size(c.s, ctx->d_events, Ep, final_piece, c.lit_from, c.n, c.chunk_bytes, ctx->d_block_s0,
                                    ctx->d_block_s1, c.base0, c.base1, ctx->d_totals));
    MRZ_STEP(c, hipMemcpyAsync(&c.tot, ctx->d_totals, sizeof(c.tot), hipMemcpyDeviceToHost, c.s));
    MRZ_STEP(c, hipStreamSynchronize(c.s));
    if (c.herr == hipSuccess) {
        // (a chunk without drains: the streams of the last chunk are not kept)
        if (!c.base0) r = mrz_grow(ctx, &ctx->d_s0, &ctx->s0_cap, c.tot.s0_len + 7 + 16);
        else r = mrz_grow_keep(ctx, &ctx->d_s0, &ctx->s0_cap, c.base0 + c.tot.s0_len + 7 + 16, c.base0);
        if (!r && !c.base1) r = mrz_grow(ctx, &ctx->d_s1, &ctx->s1_cap, c.tot.s1_len + 16);
        else if (!r) r = mrz_grow_keep(ctx, &ctx->d_s1, &ctx->s1_cap, c.base1 + c.tot.s1_len + 16, c.base1);
    }
    if (c.herr == hipSuccess && !r) {
        MRZ_STEP(c, mrz_launch_enc_write(c.s, c.d_buf, ctx->d_events, Ep, final_piece, c.lit_from, c.n, c.chunk_bytes,
                                         ctx->d_block_s0, ctx->d_block_s1, ctx->d_s0, ctx->d_s1, c.base1, c.tot.s1_len,
                                         ctx->d_lit_off, ctx->d_totals, c.crc));
        MRZ_STEP(c, hipMemcpyAsync(&c.tot, ctx->d_totals, sizeof(c.tot), hipMemcpyDeviceToHost, c.s));
    }
    c.prof.end();
    return r;
}

// nothing in flight: encode what the list holds and empty it
static int mrz_drain(mrz_chunk_call &c, mrz_chunk_plan &plan) {
    mrz_ctx *ctx = c.ctx;
    const int r = mrz_encode_piece(c, plan.known_events, 0);
    if (r || c.herr != hipSuccess) return r;
    plan.drained();
    ctx->ev_base = plan.ev_base;
    MRZ_STEP(c, hipMemcpyAsync(&ctx->d_state->ev_base, &ctx->ev_base, sizeof(int64_t), hipMemcpyHostToDevice, c.s));
    MRZ_STEP(c, hipStreamSynchronize(c.s));
    c.base0 += c.tot.s0_len;
    c.base1 += c.tot.s1_len;
    c.lit_from = plan.known_last;  // (the end of the piece's last match)
    c.n_flushes++;
    return 0;
}

// the oldest launch's event has completed: the plan takes its snapshot, the progress hook hears of it
static void mrz_retire(mrz_chunk_call &c, mrz_chunk_plan &plan) {
    mrz_ctx *ctx = c.ctx;
    const mrz_plan_news news = plan.retire(ctx->h_ring[plan.retired % MRZ_SEG_AHEAD]);
    if (ctx->progress_fn) {
        ctx->events_final = news.n_events;
        if (ctx->progress_fn(ctx->progress_user, news.n_events, news.last_match, 0)) c.rc = MRZ_E_STATE;
    }
}

static void mrz_wait_oldest(mrz_chunk_call &c, mrz_chunk_plan &plan) {
    MRZ_STEP(c, hipEventSynchronize(c.seg_ev[plan.retired % MRZ_SEG_AHEAD]));
    if (c.herr == hipSuccess) mrz_retire(c, plan);
}

// whatever has completed meanwhile (the engine choice and the span want the matcher's latest news) -- or, under a
// schedule, what the schedule says
static void mrz_retire_completed(mrz_chunk_call &c, mrz_chunk_plan &plan) {
    const int64_t retired0 = plan.retired;
    if (!plan.cfg.hold)
        while (plan.retired < plan.launched && !plan.finished && !c.rc &&
               hipEventQuery(c.seg_ev[plan.retired % MRZ_SEG_AHEAD]) == hipSuccess)
            mrz_retire(c, plan);
    for (const int64_t upto = plan.retired + plan.due(); plan.retired < upto && !plan.finished && c.ok();) mrz_wait_oldest(c, plan);
    if (c.herr == hipSuccess) plan.polled(plan.retired - retired0);
}

// the candidates of the step's stretch: a front-end pass, or (window sharding) the stretch's owner scans it (with the
// mask this rank has last heard of) and the geometry goes to the sequencer through the matcher state.  False: refused.
static bool mrz_launch_frontend_step(mrz_chunk_call &c, mrz_chunk_plan &plan, const mrz_plan_step &st) {
    mrz_ctx *ctx = c.ctx;
    const int64_t end = plan.cfg.end;
    c.prof.begin(0);
    if (st.what == MRZ_PLAN_PASS) {
        MRZ_STEP(c, mrz_launch_frontend(c.s, c.d_buf, c.n, ctx->d_index, ctx->d_state, (int)st.max_tiles, ctx->cand_cap,
                                        ctx->d_fe_hdr, ctx->d_bitmap, ctx->d_tile_cnt, ctx->d_tile_off, ctx->d_grp_cnt,
                                        ctx->d_cand));
    } else if (!st.span) {
        plan.stretch_ends(st.seg_start);
    } else {
        int64_t geo[5] = { st.seg_start, 0, 0, 0, plan.known_mask };  // seg_start, seg_end, n_cand, scan_next, list_mask
        int64_t nx = st.seg_start, nc = 0;
        const bool refused = c.herr == hipSuccess &&
                             ctx->cand_fn(ctx->cand_user, st.seg_start, st.span, plan.known_mask, plan.known_p, ctx->cand_cap,
                                          (mrz_candidate *)ctx->d_cand, ctx->d_tile_off, ctx->d_bitmap, &nx, &nc, (void *)c.s);
        if (refused || nx <= st.seg_start || nx > st.seg_start + st.span || nx % MRZ_TILE || nc < 0 || nc > ctx->cand_cap) {
            hipStreamSynchronize(c.s);
            c.rc = MRZ_E_STATE;
            return false;
        }
        geo[1] = nx < end + 1 ? nx : end + 1;
        geo[2] = nc;
        geo[3] = nx;
        MRZ_STEP(c, hipMemcpyAsync(&ctx->d_state->seg_start, geo, sizeof(geo), hipMemcpyHostToDevice, c.s));
        MRZ_STEP(c, hipStreamSynchronize(c.s));  // (geo lives on this stack frame)
        plan.stretch_ends(nx);
    }
    c.prof.end();
    return true;
}

// the step's engine over the list, then the launch's snapshot and event
static void mrz_launch_sequencer_step(mrz_chunk_call &c, mrz_chunk_plan &plan, const mrz_plan_step &st) {
    mrz_ctx *ctx = c.ctx;
    const int helpers = ctx->farm_helpers >= 0 && ctx->farm_helpers < ctx->farm_default ? ctx->farm_helpers : ctx->farm_default;
    const mrz_u64 *bitmap = (const mrz_u64 *)ctx->d_bitmap;
    c.prof.begin(1);
    if (st.engine == MRZ_ENGINE_NARROW)
        MRZ_STEP(c, mrz_launch_sequencer_narrow(c.s, c.d_buf, ctx->d_tab, ctx->d_cand, ctx->d_tile_off, bitmap, ctx->d_events,
                                                ctx->d_state, ctx->d_gmailbox, helpers, ctx->xcd));
    else if (st.engine == MRZ_ENGINE_DEEP)
        MRZ_STEP(c, mrz_launch_sequencer_deep(c.s, c.d_buf, ctx->d_tab, ctx->d_cand, ctx->d_tile_off, bitmap, ctx->d_events,
                                              ctx->d_state, ctx->d_gmailbox, helpers, ctx->xcd, ctx->d_deep_shared,
                                              ctx->deep_scanners));
    else
        MRZ_STEP(c, mrz_launch_sequencer(c.s, c.d_buf, ctx->d_tab, ctx->d_cand, ctx->d_tile_off, bitmap, ctx->d_events,
                                         ctx->d_state, ctx->d_gmailbox, helpers, ctx->d_seq_shared, ctx->d_wlog, ctx->nslots,
                                         ctx->seq_wgs, ctx->xcd, ctx->engine_pin ? 0 : ctx->deep_min_bits));
    c.prof.end();
    const int slot = (int)(plan.launched % MRZ_SEG_AHEAD);
    MRZ_STEP(c, hipMemcpyAsync(&ctx->h_ring[slot], ctx->d_state, offsetof(mrz_seq_state, prof), hipMemcpyDeviceToHost, c.s));
    MRZ_STEP(c, hipEventRecord(c.seg_ev[slot], c.s));
    plan.launch_queued(st);
    // (the first two launches are waited for: the engine hint arrives early)
    if (plan.launched <= 2 && !ctx->engine_pin && !ctx->cand_fn) MRZ_STEP(c, hipStreamSynchronize(c.s));
}

// the queued launches run out; the final matcher state, the last piece, and what the ctx reports of the chunk
static void mrz_chunk_finish(mrz_chunk_call &c, const mrz_chunk_plan &plan, mrz_seq_state *hs) {
    mrz_ctx *ctx = c.ctx;
    hipStreamSynchronize(c.s);  // (also after a refusal of the progress hook: the queued launches run out)
    for (int k = 0; k < c.n_seg_ev; k++) hipEventDestroy(c.seg_ev[k]);
    MRZ_STEP(c, hipMemcpyAsync(hs, ctx->d_state, sizeof(*hs), hipMemcpyDeviceToHost, c.s));
    MRZ_STEP(c, hipMemcpyAsync(&c.crc, ctx->d_crc_out, 4, hipMemcpyDeviceToHost, c.s));
    MRZ_STEP(c, hipStreamSynchronize(c.s));
    if (c.herr == hipSuccess) {
        if (!c.rc && (hs->error || !hs->finished)) {
            fprintf(stderr,
                    "libmrzgpu: sequencer stopped abnormally: error=%d finished=%d p=%lld end=%lld events=%lld/%lld "
                    "count=%lld min_mask=%lld scan_next=%lld launches=%lld\n",
                    hs->error, hs->finished, (long long)hs->p, (long long)hs->end, (long long)hs->n_events,
                    (long long)hs->event_cap, (long long)hs->count, (long long)hs->min_mask, (long long)hs->scan_next,
                    (long long)plan.launched);
            c.rc = MRZ_E_OVERFLOW;
        }
        if (!c.rc && ctx->progress_fn) {
            ctx->events_final = hs->n_events;
            if (ctx->progress_fn(ctx->progress_user, hs->n_events, hs->last_match, 1)) c.rc = MRZ_E_STATE;
        }
    }
    // record encoding: the last piece (the whole chunk unless the list has been drained)
    if (c.ok()) {
        c.rc = mrz_encode_piece(c, hs->n_events, 1);
        c.prof.end_total();
        MRZ_STEP(c, hipStreamSynchronize(c.s));
    }
    ctx->timings.n_segments = (int32_t)plan.launched;
    ctx->timings.n_narrow = (int32_t)plan.n_narrow;
    ctx->timings.n_deep = (int32_t)plan.n_deep;
    ctx->timings.n_event_flushes = (int32_t)c.n_flushes;
    ctx->sched_info[0] = plan.retired;
    ctx->sched_info[1] = plan.max_burst;
    ctx->sched_info[2] = plan.max_lag;
    ctx->sched_info[3] = plan.n_idle;
    c.prof.collect(&ctx->timings);
}

// (one list for both engines and for the indices the kernels count under: mrz_seq_stats.h)
#define MRZ_ST_NAME(id, name) name,
static const char *const k_stat_names[MRZ_ST_N] = { MRZ_SEQ_STATS_LIST(MRZ_ST_NAME) };
#undef MRZ_ST_NAME

static void mrz_chunk_fill_result(const mrz_chunk_call &c, const mrz_seq_state &hs, mrz_chunk_result *res) {
    mrz_ctx *ctx = c.ctx;
    ctx->s0_len = c.base0 + c.tot.s0_len + 7;
    ctx->s1_len = c.base1 + c.tot.s1_len;
    ctx->have_chunk = 1;
    res->s0_len = ctx->s0_len;
    res->s1_len = ctx->s1_len;
    res->crc32 = c.crc;
    res->d_s0 = ctx->d_s0;
    res->d_s1 = ctx->d_s1;
    res->stats.inserts = hs.inserts;
    res->stats.tag_hits = hs.tag_hits;
    res->stats.tag_misses = hs.tag_misses;
    res->stats.literals = c.tot.literals + 1;  // the zero-length terminator counts (src/rzip.c:219,664)
    res->stats.literal_bytes = c.tot.literal_bytes;
    res->stats.matches = c.tot.matches;
    res->stats.match_bytes = c.tot.match_bytes;
    res->min_mask = hs.min_mask;
    res->hash_count = hs.count;
    res->n_events = hs.n_events;
    if (ctx->print_prof)
        for (int k = 0; k < MRZ_ST_N; k++)
            if (hs.prof[k]) fprintf(stderr, "seqstat %-12s %lld\n", k_stat_names[k], (long long)hs.prof[k]);
}

extern "C" int mrz_rzip_chunk(mrz_ctx *ctx, const void *chunk, int64_t n, int where, int chunk_bytes,
                              int64_t *victim_round, mrz_chunk_result *res) {
    if (!ctx || !res || !victim_round || n < 0 || (n > 0 && !chunk) || chunk_bytes < 1 || chunk_bytes > 8)
        return MRZ_E_ARG;
    if (*victim_round < 0 || *victim_round >= (int64_t)ctx->max_chain) return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    memset(res, 0, sizeof(*res));
    memset(&ctx->timings, 0, sizeof(ctx->timings));
    ctx->have_chunk = 0;

    const uint8_t *d_buf = nullptr;
    int rc = mrz_stage_input(ctx, chunk, n, where, &d_buf);
    if (rc) return rc;
    rc = mrz_grow(ctx, &ctx->d_events, &ctx->event_cap, mrz_event_room(ctx, n));
    if (rc) return rc;
    rc = mrz_grow(ctx, &ctx->d_crc_parts, &ctx->crc_parts_cap, mrz_crc32_parts_needed(n));
    if (rc) return rc;
    const int64_t end = n - MRZ_MIN_MATCH;  // last position that is looked up (src/rzip.c:544)
    if (end > 0) {
        rc = mrz_fe_reserve(ctx, end / MRZ_TILE + 2, end + 1);
        if (rc) return rc;
    }

    mrz_plan_config cfg;
    cfg.end = end;
    // entries the sequencers may fill (by default all the list holds); `bounded`: fewer than the chunk could emit, so the
    // list is drained in pieces (the room rule of the plan)
    cfg.ev_cap = ctx->event_cap_set > 0 ? ctx->event_cap_set : ctx->event_cap;
    cfg.bounded = cfg.ev_cap < n / MRZ_MIN_MATCH + 2;
    cfg.pass_cap = mrz_plan_pass_cap(cfg.ev_cap);
    cfg.cand_cap = ctx->cand_cap;
    cfg.seg_positions = ctx->seg_positions;
    cfg.fe_tiles_cap = ctx->fe_tiles_cap;
    cfg.provider = ctx->cand_fn != nullptr;
    cfg.engine_pin = ctx->engine_pin;
    cfg.deep_min_bits = ctx->deep_min_bits;
    cfg.narrow_max_bits = ctx->narrow_max_bits;
    cfg.hold = ctx->retire_hold;
    cfg.hold_all = ctx->retire_all;

    mrz_chunk_call c(ctx, d_buf, n, chunk_bytes);
    mrz_seq_state hs;  // the matcher state the chunk begins with, then the one it ends with
    mrz_chunk_begin(c, &hs, *victim_round, cfg.ev_cap);
    mrz_chunk_plan plan;
    plan.init(cfg, hs.min_mask);
    while (!plan.finished && c.ok()) {
        mrz_retire_completed(c, plan);
        if (plan.finished || !c.ok()) break;
        const mrz_plan_step st = plan.next();
        switch (st.what) {
            case MRZ_PLAN_WAIT: mrz_wait_oldest(c, plan); break;
            case MRZ_PLAN_DRAIN: c.rc = mrz_drain(c, plan); break;
            case MRZ_PLAN_FAIL: c.rc = MRZ_E_OVERFLOW; break;
            case MRZ_PLAN_PASS:
            case MRZ_PLAN_STRETCH:
                if (mrz_launch_frontend_step(c, plan, st)) mrz_launch_sequencer_step(c, plan, st);
                break;
        }
    }
    mrz_chunk_finish(c, plan, &hs);
    if (c.herr != hipSuccess) {
        ctx->last_err = c.herr;
        return MRZ_E_HIP;
    }
    if (c.rc) return c.rc;
    *victim_round = hs.victim_round;
    mrz_chunk_fill_result(c, hs, res);
    return MRZ_OK;
}

extern "C" int mrz_fetch_streams(mrz_ctx *ctx, uint8_t *s0_host, uint8_t *s1_host) {
    if (!ctx) return MRZ_E_ARG;
    if (!ctx->have_chunk) return MRZ_E_STATE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (s0_host && ctx->s0_len > 0)
        HIPCHK(ctx, hipMemcpyAsync(s0_host, ctx->d_s0, (size_t)ctx->s0_len, hipMemcpyDeviceToHost, ctx->stream));
    if (s1_host && ctx->s1_len > 0)
        HIPCHK(ctx, hipMemcpyAsync(s1_host, ctx->d_s1, (size_t)ctx->s1_len, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MRZ_OK;
}
