// mrz_unarchive.hip -- the decompress side of the host driver (include/mrzgpu_host.h): `mrzip -d` of a -n / -l
// archive held in memory (runzip_fd, src/runzip.c:332-437), whole or a byte range of it.  Host code: each entry point
// is one loop over the chunk cursor of mrz_archive.h, which reads every archive byte, plus its own data path; what
// lives on the device is owned by scope.
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <new>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../include/mrzgpu_host.h"
#include "mrz_archive.h"
#include "mrz_ctx.h"
#include "mrz_md5.h"

namespace {

struct DeviceBuf {
    uint8_t *p = nullptr;
    ~DeviceBuf() {
        if (p) hipFree(p);
    }
};

// Streams of a chunk that holds LZ4 blocks, put together in device memory: CTYPE_NONE payloads are copied into place,
// LZ4 payloads are uploaded as they are and decoded into place by mrz_lz4_decompress_batch, all blocks of all streams
// in one launch.  What the blocks decode to never exists in host memory.
struct DeviceStreams {
    DeviceBuf base;
    uint8_t *s0 = nullptr, *s1 = nullptr;
};

// the first `nstreams` streams of the chunk (1: stream 0 alone)
int build_device_streams(mrz_ctx *ctx, const mrz_arc_chunk &c, int nstreams, DeviceStreams &ds) {
    int64_t packed = 0;
    for (int s = 0; s < nstreams; s++)
        for (const mrz_arc_block &b : c.blocks[s])
            if (b.ctype == MRZ_CTYPE_LZ4) packed += (b.c_len + 31) & ~15ll;
    const int64_t len1 = nstreams > 1 ? c.stream_len[1] : 0;
    const int64_t at1 = (c.stream_len[0] + 64 + 255) & ~255ll, at_packed = at1 + ((len1 + 64 + 255) & ~255ll);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (hipMalloc((void **)&ds.base.p, (size_t)(at_packed + packed + 64)) != hipSuccess) return MRZ_E_NOMEM;
    ds.s0 = ds.base.p;
    ds.s1 = ds.base.p + at1;
    std::vector<const void *> src;
    std::vector<void *> dst;
    std::vector<int64_t> c_lens, u_lens;
    int64_t pk = at_packed;
    for (int s = 0; s < nstreams; s++) {
        uint8_t *w = s ? ds.s1 : ds.s0;
        for (const mrz_arc_block &b : c.blocks[s]) {
            if (b.ctype == MRZ_CTYPE_LZ4) {
                if (b.c_len)
                    HIPCHK(ctx, hipMemcpyAsync(ds.base.p + pk, b.p, (size_t)b.c_len, hipMemcpyHostToDevice, ctx->stream));
                src.push_back(ds.base.p + pk);
                dst.push_back(w);
                c_lens.push_back(b.c_len);
                u_lens.push_back(b.u_len);
                pk += (b.c_len + 31) & ~15ll;
            } else if (b.c_len)
                HIPCHK(ctx, hipMemcpyAsync(w, b.p, (size_t)b.c_len, hipMemcpyHostToDevice, ctx->stream));
            w += b.u_len;
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> status(src.size());
    const int rc = mrz_lz4_decompress_batch(ctx, src.data(), c_lens.data(), (int)src.size(), MRZ_MEM_DEVICE, dst.data(),
                                            u_lens.data(), MRZ_MEM_DEVICE, status.data());
    if (rc) return rc;
    for (int32_t st : status)
        if (st) return MRZ_E_CORRUPT;
    return MRZ_OK;
}

int runzip_buffer_impl(int device, const void *mrz_v, int64_t n, void **out, int64_t *out_len) {
    if (!mrz_v || !out || !out_len) return MRZ_E_ARG;
    const uint8_t *mrz = (const uint8_t *)mrz_v;
    mrz_arc_header h;
    int rc = mrz_arc_read_header(mrz, n, &h);
    if (rc) return rc;
    // an archive written to STDOUT in several chunks carries no size (src/mrzip.c:137-140): grow chunk by chunk
    const bool size_known = h.size_known();
    int64_t cap = size_known ? h.expected : 0;
    std::unique_ptr<uint8_t, void (*)(void *)> res((uint8_t *)malloc((size_t)(cap > 0 ? cap : 1)), free);  // mrz_free's
    if (!res) return MRZ_E_NOMEM;
    mrz_arc_cursor cur{ mrz, n, h.first_chunk, MRZ_ARC_NONE_LZ4 };
    int64_t total = 0;
    {  // the context lives as long as the chunk loop
        CtxGuard g;
        rc = mrz_open(&g.ctx, device, 7, 0);
        if (rc) return rc;
        mrz_arc_chunk c;
        std::vector<uint8_t> s0, s1;
        do {  // runzip_chunk, src/runzip.c:226-330
            rc = cur.next(c);
            if (rc) return rc;
            const bool packed = c.has_lz4(0) || c.has_lz4(1);
            DeviceStreams ds;
            if (packed) {
                if (c.blocks[0].size() + c.blocks[1].size() > 0x7fffffffu) return MRZ_E_UNSUPPORTED;
                rc = build_device_streams(g.ctx, c, 2, ds);
                if (rc) return rc;
                if (!size_known) {  // the one case in which stream 0 (the records, not the literals) comes back: its
                                    // records say how much room the chunk needs
                    s0.resize((size_t)c.stream_len[0]);
                    if (c.stream_len[0] &&
                        hipMemcpy(s0.data(), ds.s0, (size_t)c.stream_len[0], hipMemcpyDeviceToHost) != hipSuccess)
                        return MRZ_E_HIP;
                }
            } else {
                c.gather(0, s0);
                c.gather(1, s1);
            }
            if (!size_known) {
                int64_t need = 0;
                if (!mrz_arc_records_out_len(s0.data(), (int64_t)s0.size(), c.cb, &need)) return MRZ_E_CORRUPT;
                if (total + need > cap) {
                    uint8_t *r2 = (uint8_t *)realloc(res.get(), (size_t)(total + need > 0 ? total + need : 1));
                    if (!r2) return MRZ_E_NOMEM;
                    res.release();  // realloc has dealt with it
                    res.reset(r2);
                    cap = total + need;
                }
            }
            int64_t got = 0;
            uint32_t crc_calc = 0, crc_stored = 0;
            rc = mrz_runzip_chunk(g.ctx, packed ? ds.s0 : s0.data(), c.stream_len[0], packed ? ds.s1 : s1.data(),
                                  c.stream_len[1], packed ? MRZ_MEM_DEVICE : MRZ_MEM_HOST, c.cb, res.get() + total,
                                  MRZ_MEM_HOST, cap - total, &got, &crc_calc, &crc_stored);
            if (rc == MRZ_E_ARG) rc = MRZ_E_CORRUPT;  // more output than the header promised
            if (rc) return rc;
            // "Bad checksum", src/runzip.c:317-320 (only without a hash)
            if (!h.hash_code && crc_calc != crc_stored) return MRZ_E_CORRUPT;
            total += got;
        } while (!c.eof);
    }
    if (size_known && total != h.expected) return MRZ_E_CORRUPT;
    if (h.hash_code == 1) {  // src/runzip.c:384-412, behind the last chunk
        uint8_t d[16];
        Md5 md5;
        md5.update(res.get(), (size_t)total);
        md5.finish(d);
        if (cur.at + 16 > n || memcmp(d, mrz + cur.at, 16)) return MRZ_E_CORRUPT;
    }
    *out = res.release();
    *out_len = total;
    return MRZ_OK;
}

// ---- a byte range of the file a -n archive decodes to --------------------------------------------------------------
// Both range calls: mrz_arc_range judges the arguments against the header, clips every chunk and gives the closing
// verdict.  They differ in when a NULL output with count > 0 is refused: mrz_runzip_buffer_range after the walk (it
// validates what it walks first), mrz_runzip_buffer_range_ex before it where the header carries the size, and without
// one it walks for the length but does no work for the range.

struct RangePart {  // a chunk that intersects the range
    int cb;
    std::vector<uint8_t> s0;
    mrz_arc_table s1;  // the literal stream stays in the archive
    int64_t s1_len;
    int64_t lo, count;  // bytes [lo, lo + count) of the chunk ...
    int64_t out_at;     // ... go to out_host + out_at
};

// CTYPE_NONE blocks only: the origins come to the host and runs of them are copied out of the archive's blocks
int runzip_buffer_range_impl(int device, const void *mrz_v, int64_t n, int64_t first, int64_t count, void *out_host,
                             int64_t *file_len) {
    if (!mrz_v) return MRZ_E_ARG;
    const uint8_t *mrz = (const uint8_t *)mrz_v;
    mrz_arc_header h;
    int rc = mrz_arc_read_header(mrz, n, &h);
    if (rc) return rc;
    mrz_arc_range rg;
    rc = rg.begin(h, first, count, file_len);
    if (rc || (rg.size_known && !count)) return rc;
    // the chunks: header, stream 0 gathered, stream 1 as a table, decoded length from the records
    std::vector<RangePart> parts;
    mrz_arc_cursor cur{ mrz, n, h.first_chunk, MRZ_ARC_NONE_ONLY };
    mrz_arc_chunk c;
    do {
        rc = cur.next(c);
        if (rc) return rc;
        RangePart part;
        c.gather(0, part.s0);
        int64_t chunk_len = 0;
        if (!mrz_arc_records_out_len(part.s0.data(), (int64_t)part.s0.size(), c.cb, &chunk_len)) return MRZ_E_CORRUPT;
        if (rg.clip(chunk_len, &part.lo, &part.count, &part.out_at)) {
            part.cb = c.cb;
            part.s1.set(std::move(c.blocks[1]));
            part.s1_len = c.stream_len[1];
            parts.push_back(std::move(part));
        }
        rg.total += chunk_len;
    } while (!rg.covered() && !c.eof);
    rc = rg.finish(file_len);
    if (rc || !count) return rc;
    if (!out_host) return MRZ_E_ARG;
    CtxGuard g;
    rc = mrz_open(&g.ctx, device, 7, 0);
    std::vector<int64_t> origins;
    for (size_t k = 0; !rc && k < parts.size(); k++) {
        const RangePart &pt = parts[k];
        origins.resize((size_t)pt.count);
        mrz_range_info info;
        rc = mrz_runzip_origins(g.ctx, pt.s0.data(), (int64_t)pt.s0.size(), pt.s1_len, MRZ_MEM_HOST, pt.cb, pt.lo, pt.count,
                                origins.data(), MRZ_MEM_HOST, &info);
        if (rc == MRZ_E_ARG) rc = MRZ_E_CORRUPT;  // the device's reading of the records differs from the host walk's
        if (rc) break;
        uint8_t *dst = (uint8_t *)out_host + pt.out_at;
        for (int64_t i = 0; i < pt.count;) {  // runs of consecutive origins
            int64_t j = i + 1;
            while (j < pt.count && origins[(size_t)j] == origins[(size_t)j - 1] + 1) j++;
            pt.s1.copy(origins[(size_t)i], j - i, dst + i);
            i = j;
        }
    }
    return rc;
}

// ---- ... and of a -l archive: stream 1 stays in its blocks, the touched ones are decoded as far as they are needed -----
// One entry of the stream-1 table the device sees: a block, or a piece of at most kLz4MaxInput bytes of a longer
// CTYPE_NONE block, so that offsets inside an entry fit the 32 bits of mrz_uz_span.
struct S1Piece {
    size_t block;  // index into the chunk's stream-1 blocks
    int64_t at;    // where the piece begins in its block
};

// `cnt` bytes of one chunk into d_out (device memory): origins, spans, the touched blocks' prefixes, gather.  Which
// bytes they are is the resolver's business: resolve(d_org, &ri) leaves their cnt origins, in the order of d_out, in
// device memory at d_org -- one range (mrz_runzip_origins) or the packed parts of many (mrz_runzip_origins_multi).
template <class Resolve>
int chunk_blocks(mrz_ctx *ctx, int cus, const mrz_arc_table &s1, int64_t cnt, Resolve &&resolve, uint8_t *d_out,
                 mrz_archive_range_info &acc) {
    std::vector<int64_t> starts;
    std::vector<S1Piece> pieces;
    for (size_t k = 0; k < s1.blocks.size(); k++) {
        int64_t off = 0;
        do {
            starts.push_back(s1.starts[k] + off);
            pieces.push_back(S1Piece{ k, off });
            off += kLz4MaxInput;
        } while (off < s1.blocks[k].u_len);
    }
    const int64_t nt = (int64_t)starts.size();
    auto al = [](int64_t v) { return (v + 255) & ~255ll; };
    const int64_t o_starts = al(cnt * 8), o_span = o_starts + al(nt * 8), o_base = o_span + al(nt * 8);
    DeviceBuf tab;
    if (hipMalloc((void **)&tab.p, (size_t)(o_base + al(nt * 8))) != hipSuccess) return MRZ_E_NOMEM;
    int64_t *d_org = (int64_t *)tab.p, *d_starts = (int64_t *)(tab.p + o_starts), *d_base = (int64_t *)(tab.p + o_base);
    mrz_uz_span *d_span = (mrz_uz_span *)(tab.p + o_span);

    mrz_range_info ri;
    int rc = resolve(d_org, &ri);
    if (rc == MRZ_E_ARG) rc = MRZ_E_CORRUPT;  // the device's reading of the records differs from the length walk's
    if (rc) return rc;
    acc.chunks_in_range++;
    acc.total_hops += ri.total_hops;
    if (ri.max_hops > acc.max_hops) acc.max_hops = ri.max_hops;

    std::vector<mrz_uz_span> span((size_t)nt, mrz_uz_span{ 0xffffffffu, 0u });
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(d_starts, starts.data(), (size_t)nt * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(d_span, span.data(), (size_t)nt * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, mrz_launch_block_span(s, cus, d_org, cnt, d_starts, nt, d_span));
    HIPCHK(ctx, hipMemcpyAsync(span.data(), d_span, (size_t)nt * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));

    // what the touched entries need: LZ4 payloads in front, then per entry the bytes from its lowest offset on
    int64_t packed = 0, staged = 0;
    for (int64_t t = 0; t < nt; t++) {
        if (span[(size_t)t].lo > span[(size_t)t].hi) continue;
        const mrz_arc_block &b = s1.blocks[pieces[(size_t)t].block];
        const int64_t hi = span[(size_t)t].hi, low = span[(size_t)t].lo;
        if (pieces[(size_t)t].at + hi >= b.u_len) return MRZ_E_STATE;  // (an origin lies below s1_len: cannot happen)
        if (b.ctype == MRZ_CTYPE_LZ4) {
            packed += (b.c_len + 31) & ~15ll;
            staged += (hi + 1 + 31) & ~15ll;
        } else
            staged += (hi - low + 1 + 31) & ~15ll;
    }
    DeviceBuf stage;
    if (hipMalloc((void **)&stage.p, (size_t)(packed + staged + 64)) != hipSuccess) return MRZ_E_NOMEM;
    std::vector<int64_t> base((size_t)nt, 0);
    std::vector<const void *> src;
    std::vector<void *> dst;
    std::vector<int64_t> c_lens, u_lens, wants;
    int64_t pk = 0, st = packed;
    size_t last_block = (size_t)-1;
    for (int64_t t = 0; t < nt; t++) {
        if (span[(size_t)t].lo > span[(size_t)t].hi) continue;
        const S1Piece &pc = pieces[(size_t)t];
        const mrz_arc_block &b = s1.blocks[pc.block];
        const int64_t hi = span[(size_t)t].hi, low = span[(size_t)t].lo;
        if (pc.block != last_block) acc.s1_blocks_touched++;
        last_block = pc.block;
        if (b.ctype == MRZ_CTYPE_LZ4) {  // the prefix [0, hi]: a decode cannot begin anywhere else
            if (b.c_len) HIPCHK(ctx, hipMemcpyAsync(stage.p + pk, b.p, (size_t)b.c_len, hipMemcpyHostToDevice, s));
            src.push_back(stage.p + pk);
            dst.push_back(stage.p + st);
            c_lens.push_back(b.c_len);
            u_lens.push_back(b.u_len);
            wants.push_back(hi + 1);
            base[(size_t)t] = st + low;
            pk += (b.c_len + 31) & ~15ll;
            st += (hi + 1 + 31) & ~15ll;
            acc.s1_lz4_bytes += hi + 1;
            acc.s1_bytes_uploaded += b.c_len;
        } else {  // bytes [low, hi] of the piece
            HIPCHK(ctx, hipMemcpyAsync(stage.p + st, b.p + pc.at + low, (size_t)(hi - low + 1), hipMemcpyHostToDevice, s));
            base[(size_t)t] = st;
            st += (hi - low + 1 + 31) & ~15ll;
            acc.s1_bytes_uploaded += hi - low + 1;
        }
    }
    if (src.size() > 0x7fffffffu) return MRZ_E_UNSUPPORTED;
    HIPCHK(ctx, hipMemcpyAsync(d_base, base.data(), (size_t)nt * 8, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (!src.empty()) {
        std::vector<int32_t> status(src.size());
        rc = mrz_lz4_decompress_prefix_batch(ctx, src.data(), c_lens.data(), (int)src.size(), MRZ_MEM_DEVICE, dst.data(),
                                             u_lens.data(), wants.data(), MRZ_MEM_DEVICE, status.data());
        if (rc) return rc;
        for (int32_t v : status)
            if (v) return MRZ_E_CORRUPT;
    }
    HIPCHK(ctx, mrz_launch_block_gather(s, cus, d_org, cnt, d_starts, nt, d_span, d_base, stage.p, d_out));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return MRZ_OK;
}

// bytes [lo, lo + cnt) of one chunk
int range_chunk_blocks(mrz_ctx *ctx, int cus, const void *s0, int64_t s0_len, int where0, const mrz_arc_table &s1,
                       int64_t s1_len, int cb, int64_t lo, int64_t cnt, uint8_t *d_out, mrz_archive_range_info &acc) {
    return chunk_blocks(
        ctx, cus, s1, cnt,
        [&](int64_t *d_org, mrz_range_info *ri) {
            return mrz_runzip_origins(ctx, s0, s0_len, s1_len, where0, cb, lo, cnt, d_org, MRZ_MEM_DEVICE, ri);
        },
        d_out, acc);
}

// The parts of one chunk that a list of ranges asks for, to d_out + part.out_at each (device memory): the parts are
// resolved flat, in list order, by ONE mrz_runzip_origins_multi (one parse of stream 0), gathered flat by the same span
// and gather kernels, and -- unless they follow each other in the output anyway, where they are gathered in place --
// moved to their places by one mrz_copy_device_batch.
int ranges_chunk_blocks(mrz_ctx *ctx, int cus, const void *s0, int64_t s0_len, int where0, const mrz_arc_table &s1,
                        int64_t s1_len, int cb, const std::vector<mrz_arc_part> &parts, uint8_t *d_out,
                        mrz_archive_range_info &acc) {
    std::vector<mrz_byte_range> rl(parts.size());
    int64_t cnt = 0;
    for (size_t k = 0; k < parts.size(); k++) {
        rl[k] = mrz_byte_range{ parts[k].lo, parts[k].cnt };
        cnt += parts[k].cnt;
    }
    const bool in_place = mrz_arc_ranges::contiguous(parts);
    DeviceBuf flat;
    if (!in_place && hipMalloc((void **)&flat.p, (size_t)cnt) != hipSuccess) return MRZ_E_NOMEM;
    int rc = chunk_blocks(
        ctx, cus, s1, cnt,
        [&](int64_t *d_org, mrz_range_info *ri) {
            return mrz_runzip_origins_multi(ctx, s0, s0_len, s1_len, where0, cb, rl.data(), (int64_t)rl.size(), d_org,
                                            MRZ_MEM_DEVICE, ri);
        },
        in_place ? d_out + parts[0].out_at : flat.p, acc);
    if (rc || in_place) return rc;
    std::vector<const void *> src(parts.size());
    std::vector<void *> dst(parts.size());
    std::vector<int64_t> lens(parts.size());
    int64_t at = 0;
    for (size_t k = 0; k < parts.size(); k++) {
        src[k] = flat.p + at;
        dst[k] = d_out + parts[k].out_at;
        lens[k] = parts[k].cnt;
        at += parts[k].cnt;
    }
    return mrz_copy_device_batch(ctx, src.data(), dst.data(), lens.data(), (int64_t)parts.size());
}

// mrz_runzip_buffer_ranges: runzip_buffer_range_ex_impl with mrz_arc_ranges in place of mrz_arc_range.  `shared`: a
// context of the caller's to work on (mrz_ar_extract_mrz makes three calls on one); NULL: one is opened on first need.
int runzip_buffer_ranges_impl(mrz_ctx *shared, int device, const void *mrz_v, int64_t n, const mrz_byte_range *ranges,
                              int64_t n_ranges, void *out, int out_where, int64_t *file_len,
                              mrz_archive_range_info &acc) {
    if (!mrz_v || n_ranges < 0 || (n_ranges > 0 && !ranges) || (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE))
        return MRZ_E_ARG;
    const uint8_t *mrz = (const uint8_t *)mrz_v;
    mrz_arc_header h;
    int rc = mrz_arc_read_header(mrz, n, &h);
    if (rc) return rc;
    mrz_arc_ranges rg;
    rc = rg.begin(h, ranges, n_ranges, file_len);
    if (rc || (rg.size_known && !rg.sum)) return rc;
    if (!out && rg.sum > 0) {
        if (rg.size_known) return MRZ_E_ARG;
        rg.bad = true;
    }
    CtxGuard g;
    mrz_ctx *ctx = shared;
    int cus = 0;
    auto open_ctx = [&]() {  // on first need: an archive may be walked without any device work
        if (!cus) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        if (ctx) return (int)MRZ_OK;
        const int r = mrz_open(&g.ctx, device, 7, 0);
        ctx = g.ctx;
        return r;
    };
    DeviceBuf scratch;  // the packed ranges, when `out` is host memory
    uint8_t *d_out = out_where == MRZ_MEM_DEVICE ? (uint8_t *)out : nullptr;
    mrz_arc_cursor cur{ mrz, n, h.first_chunk, MRZ_ARC_NONE_LZ4 };
    mrz_arc_chunk c;
    std::vector<uint8_t> s0;
    std::vector<mrz_arc_part> parts;
    do {
        rc = cur.next(c);
        if (rc) return rc;
        // stream 0 and the chunk's length: as runzip_buffer_range_ex_impl has them
        int64_t s0_lz4 = 0;
        for (const mrz_arc_block &b : c.blocks[0])
            if (b.ctype == MRZ_CTYPE_LZ4) s0_lz4 += b.u_len;
        const bool s0_on_device = s0_lz4 > 0;
        DeviceStreams ds;
        int64_t chunk_len = 0;
        if (s0_on_device) {
            if (c.blocks[0].size() > 0x7fffffffu) return MRZ_E_UNSUPPORTED;
            rc = open_ctx();
            if (rc) return rc;
            rc = build_device_streams(ctx, c, 1, ds);
            if (rc) return rc;
            acc.s0_lz4_bytes += s0_lz4;
            mrz_range_info ri;
            rc = mrz_runzip_origins(ctx, ds.s0, c.stream_len[0], c.stream_len[1], MRZ_MEM_DEVICE, c.cb, 0, 0, nullptr,
                                    MRZ_MEM_DEVICE, &ri);
            if (rc == MRZ_E_ARG) rc = MRZ_E_CORRUPT;  // too short to hold a terminator
            if (rc) return rc;
            chunk_len = ri.chunk_len;
        } else {
            c.gather(0, s0);
            if (!mrz_arc_records_out_len(s0.data(), (int64_t)s0.size(), c.cb, &chunk_len)) return MRZ_E_CORRUPT;
        }
        if (rg.clip(chunk_len, parts)) {
            rc = open_ctx();
            if (rc) return rc;
            if (!d_out) {
                if (hipMalloc((void **)&scratch.p, (size_t)rg.sum) != hipSuccess) return MRZ_E_NOMEM;
                d_out = scratch.p;
            }
            mrz_arc_table s1;
            s1.set(std::move(c.blocks[1]));
            rc = ranges_chunk_blocks(ctx, cus, s0_on_device ? (const void *)ds.s0 : (const void *)s0.data(),
                                     s0_on_device ? c.stream_len[0] : (int64_t)s0.size(),
                                     s0_on_device ? MRZ_MEM_DEVICE : MRZ_MEM_HOST, s1, c.stream_len[1], c.cb, parts, d_out,
                                     acc);
            if (rc) return rc;
        }
        rg.total += chunk_len;
    } while (!rg.covered() && !c.eof);
    rc = rg.finish(file_len);
    if (rc || !rg.sum) return rc;
    if (!out) return MRZ_E_ARG;
    if (scratch.p && hipMemcpy(out, scratch.p, (size_t)rg.sum, hipMemcpyDeviceToHost) != hipSuccess) return MRZ_E_HIP;
    return MRZ_OK;
}

int runzip_buffer_range_ex_impl(int device, const void *mrz_v, int64_t n, int64_t first, int64_t count, void *out,
                                int out_where, int64_t *file_len, mrz_archive_range_info &acc) {
    if (!mrz_v || (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE)) return MRZ_E_ARG;
    const uint8_t *mrz = (const uint8_t *)mrz_v;
    mrz_arc_header h;
    int rc = mrz_arc_read_header(mrz, n, &h);
    if (rc) return rc;
    mrz_arc_range rg;
    rc = rg.begin(h, first, count, file_len);
    if (rc || (rg.size_known && !count)) return rc;
    if (!out && count > 0) {
        if (rg.size_known) return MRZ_E_ARG;
        rg.bad = true;
    }
    CtxGuard g;
    int cus = 0;
    auto open_ctx = [&]() {  // on first need: an archive may be walked without any device work
        if (g.ctx) return (int)MRZ_OK;
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        return mrz_open(&g.ctx, device, 7, 0);
    };
    DeviceBuf scratch;  // the range, when `out` is host memory
    uint8_t *d_out = out_where == MRZ_MEM_DEVICE ? (uint8_t *)out : nullptr;
    mrz_arc_cursor cur{ mrz, n, h.first_chunk, MRZ_ARC_NONE_LZ4 };
    mrz_arc_chunk c;
    std::vector<uint8_t> s0;
    do {
        rc = cur.next(c);
        if (rc) return rc;
        // stream 0 and the chunk's length: on the device where an LZ4 block of it decodes to anything (decoded whole: the
        // parse needs every record), otherwise gathered and walked on the host as mrz_runzip_buffer_range does -- the
        // payloads of LZ4 blocks that claim u_len 0 included, where mrz_runzip_buffer says MRZ_E_CORRUPT: a known gap
        int64_t s0_lz4 = 0;
        for (const mrz_arc_block &b : c.blocks[0])
            if (b.ctype == MRZ_CTYPE_LZ4) s0_lz4 += b.u_len;
        const bool s0_on_device = s0_lz4 > 0;
        DeviceStreams ds;
        int64_t chunk_len = 0;
        if (s0_on_device) {
            if (c.blocks[0].size() > 0x7fffffffu) return MRZ_E_UNSUPPORTED;
            rc = open_ctx();
            if (rc) return rc;
            rc = build_device_streams(g.ctx, c, 1, ds);
            if (rc) return rc;
            acc.s0_lz4_bytes += s0_lz4;
            mrz_range_info ri;
            rc = mrz_runzip_origins(g.ctx, ds.s0, c.stream_len[0], c.stream_len[1], MRZ_MEM_DEVICE, c.cb, 0, 0, nullptr,
                                    MRZ_MEM_DEVICE, &ri);
            if (rc == MRZ_E_ARG) rc = MRZ_E_CORRUPT;  // too short to hold a terminator
            if (rc) return rc;
            chunk_len = ri.chunk_len;
        } else {
            c.gather(0, s0);
            if (!mrz_arc_records_out_len(s0.data(), (int64_t)s0.size(), c.cb, &chunk_len)) return MRZ_E_CORRUPT;
        }
        int64_t lo, cnt, out_at;
        if (rg.clip(chunk_len, &lo, &cnt, &out_at)) {
            rc = open_ctx();
            if (rc) return rc;
            if (!d_out) {
                if (hipMalloc((void **)&scratch.p, (size_t)count) != hipSuccess) return MRZ_E_NOMEM;
                d_out = scratch.p;
            }
            mrz_arc_table s1;
            s1.set(std::move(c.blocks[1]));
            rc = range_chunk_blocks(g.ctx, cus, s0_on_device ? (const void *)ds.s0 : (const void *)s0.data(),
                                    s0_on_device ? c.stream_len[0] : (int64_t)s0.size(),
                                    s0_on_device ? MRZ_MEM_DEVICE : MRZ_MEM_HOST, s1, c.stream_len[1], c.cb, lo, cnt,
                                    d_out + out_at, acc);
            if (rc) return rc;
        }
        rg.total += chunk_len;
    } while (!rg.covered() && !c.eof);
    rc = rg.finish(file_len);
    if (rc || !count) return rc;
    if (!out) return MRZ_E_ARG;
    if (scratch.p && hipMemcpy(out, scratch.p, (size_t)count, hipMemcpyDeviceToHost) != hipSuccess) return MRZ_E_HIP;
    return MRZ_OK;
}

// the header promises that the library never takes the host process down: what the standard containers throw ends here
template <class F>
int no_throw(F &&call) {
    try {
        return call();
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    } catch (const std::length_error &) {
        return MRZ_E_CORRUPT;
    }
}

}  // namespace

extern "C" int mrz_runzip_buffer(int device, const void *mrz, int64_t n, void **out, int64_t *out_len) {
    return no_throw([&] { return runzip_buffer_impl(device, mrz, n, out, out_len); });
}

extern "C" int mrz_runzip_buffer_range(int device, const void *mrz, int64_t n, int64_t first, int64_t count,
                                       void *out_host, int64_t *file_len) {
    return no_throw([&] { return runzip_buffer_range_impl(device, mrz, n, first, count, out_host, file_len); });
}

int mrz_runzip_buffer_ranges_on(mrz_ctx *ctx, int device, const void *mrz, int64_t n, const mrz_byte_range *ranges,
                                int64_t n_ranges, void *out, int out_where, int64_t *file_len,
                                mrz_archive_range_info *info) {
    mrz_archive_range_info acc;
    memset(&acc, 0, sizeof(acc));
    const int rc = no_throw([&] {
        return runzip_buffer_ranges_impl(ctx, device, mrz, n, ranges, n_ranges, out, out_where, file_len, acc);
    });
    if (info) *info = acc;
    return rc;
}

extern "C" int mrz_runzip_buffer_ranges(int device, const void *mrz, int64_t n, const mrz_byte_range *ranges,
                                        int64_t n_ranges, void *out, int out_where, int64_t *file_len,
                                        mrz_archive_range_info *info) {
    return mrz_runzip_buffer_ranges_on(nullptr, device, mrz, n, ranges, n_ranges, out, out_where, file_len, info);
}

extern "C" int mrz_runzip_buffer_range_ex(int device, const void *mrz, int64_t n, int64_t first, int64_t count, void *out,
                                          int out_where, int64_t *file_len, mrz_archive_range_info *info) {
    mrz_archive_range_info acc;
    memset(&acc, 0, sizeof(acc));
    const int rc = no_throw(
        [&] { return runzip_buffer_range_ex_impl(device, mrz, n, first, count, out, out_where, file_len, acc); });
    if (info) *info = acc;
    return rc;
}
