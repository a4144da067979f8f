// mrz_ar.hip -- the drivers of the ARZIP entry points: create() of ar-mrzip over members in memory (checksums and
// digests on the device, the order on the device, the collapse and the framing on the host: mrz_ar_index.h), the
// parser's ABI face and the verifier.  Everything that knows the archive's bytes is in mrz_ar_index.h; everything that
// computes is in mrz_blake2b.hip and mrz_tlsh.hip.  This file owns the data paths.
#include <string.h>

#include <map>
#include <new>
#include <utility>
#include <vector>

#include "../../include/mrzgpu_host.h"
#include "mrz_ar_index.h"
#include "mrz_ctx.h"
#include "mrz_tlsh_tables.h"

namespace {
struct ArDevBuf {
    void *p = nullptr;
    ~ArDevBuf() {
        if (p) hipFree(p);
    }
};
}  // namespace

static_assert(MRZ_AR_DIGEST == MRZ_TLSH_STORED, "the archive keeps 137 bytes of a digest");

extern "C" int mrz_ar_create(mrz_ctx *ctx, const mrz_ar_member *members, int64_t n, int where, void *out, int out_where,
                             int64_t out_cap, int64_t *out_len, mrz_ar_info *info) {
    if (!ctx || n < 0 || n > 0x7fffffffll || (n && !members) || !out_len ||
        (where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) ||
        (out && out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE) || (out && out_cap < 0))
        return MRZ_E_ARG;
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) {
        const mrz_ar_member &m = members[i];
        if (m.size < 0 || (m.size && !m.data) || (m.name_len && !m.name)) return MRZ_E_ARG;
        if (m.size > MRZ_TLSH_MAX_LEN) return MRZ_E_UNSUPPORTED;  // before any byte is touched
        total += (m.size + 15) & ~15ll;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the members on the device
    ArDevBuf stage;
    std::vector<const void *> d_ptrs((size_t)n);
    std::vector<int64_t> lens((size_t)n);
    if (where == MRZ_MEM_HOST && total) {
        if (hipMalloc(&stage.p, (size_t)total) != hipSuccess) {
            stage.p = nullptr;
            return MRZ_E_NOMEM;
        }
    }
    int64_t off = 0;
    for (int64_t i = 0; i < n; i++) {
        lens[i] = members[i].size;
        if (where == MRZ_MEM_HOST) {
            d_ptrs[i] = lens[i] ? (const uint8_t *)stage.p + off : nullptr;
            if (lens[i])
                HIPCHK(ctx, hipMemcpyAsync((uint8_t *)stage.p + off, members[i].data, (size_t)lens[i],
                                           hipMemcpyHostToDevice, ctx->stream));
            off += (lens[i] + 15) & ~15ll;
        } else
            d_ptrs[i] = members[i].data;
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the checksum kernel runs on the side stream
    std::vector<mrz_ar_rec> recs((size_t)n);
    std::vector<uint8_t> sums((size_t)n * MRZ_AR_SUM);
    int rc = n ? mrz_blake2b_batch(ctx, d_ptrs.data(), lens.data(), (int)n, MRZ_MEM_DEVICE, MRZ_AR_SUM, sums.data())
               : MRZ_OK;
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++) {
        mrz_ar_rec &r = recs[i];
        r.mtime = members[i].mtime;
        r.size = lens[i];
        r.offset = 0;
        memcpy(r.sum, &sums[(size_t)i * MRZ_AR_SUM], MRZ_AR_SUM);
        memset(r.digest, 0, MRZ_AR_DIGEST);
        r.name = (const uint8_t *)members[i].name;
        r.name_len = members[i].name_len;
        r.index = i;
        r.record_at = 0;
    }
    int64_t unique = 0, dup = 0;
    if (!out) {  // sizing: what the collapse keeps does not depend on the order
        mrz_ar_collapse(recs, &unique, &dup);
        *out_len = MRZ_AR_HEAD + mrz_ar_metadata_size(recs) + unique;
        if (info) *info = mrz_ar_info{ unique, dup, 0, mrz_ar_metadata_size(recs) };
        return MRZ_OK;
    }
    // digests of the members above 500 bytes (compute_checksums: the others keep 137 zero bytes)
    std::vector<const uint8_t *> t_ptrs;
    std::vector<int64_t> t_lens, t_who;
    for (int64_t i = 0; i < n; i++)
        if (lens[i] > 500) {
            t_ptrs.push_back((const uint8_t *)d_ptrs[i]);
            t_lens.push_back(lens[i]);
            t_who.push_back(i);
        }
    if (!t_who.empty()) {
        std::vector<char> hex(t_who.size() * (MRZ_TLSH_HEX + 1));
        rc = mrz_tlsh_device_batch(ctx, t_ptrs.data(), t_lens.data(), (int)t_who.size(), nullptr, hex.data(), nullptr);
        if (rc) return rc;
        for (size_t k = 0; k < t_who.size(); k++)  // no digest: the string is empty and the 137 bytes stay zero
            if (hex[k * (MRZ_TLSH_HEX + 1)])
                memcpy(recs[t_who[k]].digest, &hex[k * (MRZ_TLSH_HEX + 1)], MRZ_AR_DIGEST);
    }
    std::vector<uint8_t> digs((size_t)n * MRZ_AR_DIGEST);
    for (int64_t i = 0; i < n; i++) memcpy(&digs[(size_t)i * MRZ_AR_DIGEST], recs[i].digest, MRZ_AR_DIGEST);
    std::vector<int32_t> perm((size_t)n);
    rc = mrz_ar_order(ctx, digs.data(), n, perm.data());
    if (rc) return rc;
    std::vector<mrz_ar_rec> ordered((size_t)n);
    for (int64_t k = 0; k < n; k++) ordered[k] = recs[perm[k]];
    mrz_ar_collapse(ordered, &unique, &dup);
    const int64_t meta = mrz_ar_metadata_size(ordered), need = MRZ_AR_HEAD + meta + unique;
    *out_len = need;
    if (info) *info = mrz_ar_info{ unique, dup, (int64_t)t_who.size(), meta };
    if (out_cap < need) return MRZ_E_ARG;
    std::vector<uint8_t> head((size_t)(MRZ_AR_HEAD + meta));
    mrz_ar_write_metadata(ordered, head.data());
    uint8_t *o = (uint8_t *)out;
    hipStream_t st = ctx->stream;
    if (out_where == MRZ_MEM_HOST)
        memcpy(o, head.data(), head.size());
    else
        HIPCHK(ctx, hipMemcpyAsync(o, head.data(), head.size(), hipMemcpyHostToDevice, st));
    int64_t at = MRZ_AR_HEAD + meta;
    for (size_t k : mrz_ar_payload_plan(ordered)) {
        const mrz_ar_rec &r = ordered[k];
        if (!r.size) continue;
        if (out_where == MRZ_MEM_DEVICE)
            HIPCHK(ctx, hipMemcpyAsync(o + at, d_ptrs[r.index], (size_t)r.size, hipMemcpyDeviceToDevice, st));
        else if (where == MRZ_MEM_HOST)
            memcpy(o + at, members[r.index].data, (size_t)r.size);
        else
            HIPCHK(ctx, hipMemcpyAsync(o + at, d_ptrs[r.index], (size_t)r.size, hipMemcpyDeviceToHost, st));
        at += r.size;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return at == need ? MRZ_OK : MRZ_E_OVERFLOW;
}

extern "C" int mrz_ar_parse(const void *ar, int64_t n, mrz_ar_entry *entries, int64_t cap, int64_t *count,
                            int64_t *payload_at) {
    if (!ar || n < 0 || !count || (entries && cap < 0)) return MRZ_E_ARG;
    std::vector<mrz_ar_rec> recs;
    int64_t pay = 0;
    int rc = mrz_ar_read((const uint8_t *)ar, n, n, recs, &pay);
    if (rc) return rc;
    *count = (int64_t)recs.size();
    if (payload_at) *payload_at = pay;
    if (!entries) return MRZ_OK;
    if ((int64_t)recs.size() > cap) return MRZ_E_ARG;
    for (size_t i = 0; i < recs.size(); i++) {
        const mrz_ar_rec &r = recs[i];
        entries[i] = mrz_ar_entry{ r.mtime, r.size, r.offset, r.record_at, r.record_at + MRZ_AR_FIXED, r.name_len, 0 };
    }
    return MRZ_OK;
}

extern "C" int mrz_ar_verify(mrz_ctx *ctx, const void *ar, int64_t n, int where, int64_t *first_bad, int64_t *n_bad) {
    if (!ctx || !ar || n < 0 || !first_bad || !n_bad || (where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE))
        return MRZ_E_ARG;
    *first_bad = -1;
    *n_bad = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the metadata on the host
    std::vector<uint8_t> copy;
    const uint8_t *meta = (const uint8_t *)ar;
    int64_t have = n;
    if (where == MRZ_MEM_DEVICE) {
        if (n < MRZ_AR_HEAD) return MRZ_E_CORRUPT;
        copy.resize(MRZ_AR_HEAD);
        HIPCHK(ctx, hipMemcpy(copy.data(), ar, MRZ_AR_HEAD, hipMemcpyDeviceToHost));
        int64_t m = 0;
        int rc = mrz_ar_read_head(copy.data(), n, &m);
        if (rc) return rc;
        copy.resize((size_t)(MRZ_AR_HEAD + m));
        if (m) HIPCHK(ctx, hipMemcpy(copy.data() + MRZ_AR_HEAD, (const uint8_t *)ar + MRZ_AR_HEAD, (size_t)m,
                                     hipMemcpyDeviceToHost));
        meta = copy.data();
        have = MRZ_AR_HEAD + m;
    }
    std::vector<mrz_ar_rec> recs;
    int64_t pay = 0;
    int rc = mrz_ar_read(meta, have, n, recs, &pay);
    if (rc) return rc;
    if (recs.empty()) return MRZ_OK;
    // one hash per distinct (offset, size)
    std::map<std::pair<int64_t, int64_t>, int> slot;
    std::vector<const void *> ptrs;
    std::vector<int64_t> lens;
    std::vector<int> of((size_t)recs.size());
    for (size_t i = 0; i < recs.size(); i++) {
        auto ins = slot.emplace(std::make_pair(recs[i].offset, recs[i].size), (int)ptrs.size());
        if (ins.second) {
            ptrs.push_back(recs[i].size ? (const uint8_t *)ar + pay + recs[i].offset : nullptr);
            lens.push_back(recs[i].size);
        }
        of[i] = ins.first->second;
    }
    std::vector<uint8_t> sums(ptrs.size() * MRZ_AR_SUM);
    rc = mrz_blake2b_batch(ctx, ptrs.data(), lens.data(), (int)ptrs.size(), where, MRZ_AR_SUM, sums.data());
    if (rc) return rc;
    for (size_t i = 0; i < recs.size(); i++)
        if (memcmp(recs[i].sum, &sums[(size_t)of[i] * MRZ_AR_SUM], MRZ_AR_SUM)) {
            if (*first_bad < 0) *first_bad = (int64_t)i;
            ++*n_bad;
        }
    return MRZ_OK;
}

// ---- extract: members out of an archive in memory, or straight out of the .mrz that holds it ------------------------

// mrz_runzip_buffer_ranges on a context of the caller's (mrz_unarchive.hip)
int mrz_runzip_buffer_ranges_on(mrz_ctx *ctx, int device, const void *mrz, int64_t n, const mrz_byte_range *ranges,
                                int64_t n_ranges, void *out, int out_where, int64_t *file_len,
                                mrz_archive_range_info *info);

namespace {
// what a selection asks for: the records in selection order, where each goes, and the distinct payloads behind them
struct ArSelection {
    std::vector<int64_t> rec;                            // record index of every selection entry
    std::vector<int64_t> at;                             // output offset of every entry, and the total
    std::vector<std::pair<int64_t, int64_t>> distinct;   // (offset, size), ascending by offset
    std::vector<size_t> slot;                            // per entry: its place in `distinct`
};

int ar_select(const std::vector<mrz_ar_rec> &recs, const int64_t *which, int64_t n_which, ArSelection &sel) {
    const int64_t n = which ? n_which : (int64_t)recs.size();
    if (n < 0) return MRZ_E_ARG;
    sel.rec.resize((size_t)n);
    sel.at.assign((size_t)n + 1, 0);
    std::map<std::pair<int64_t, int64_t>, size_t> seen;
    for (int64_t k = 0; k < n; k++) {
        const int64_t r = which ? which[k] : k;
        if (r < 0 || r >= (int64_t)recs.size()) return MRZ_E_ARG;
        sel.rec[(size_t)k] = r;
        if (recs[(size_t)r].size > INT64_MAX - sel.at[(size_t)k]) return MRZ_E_ARG;
        sel.at[(size_t)k + 1] = sel.at[(size_t)k] + recs[(size_t)r].size;
        seen.emplace(std::make_pair(recs[(size_t)r].offset, recs[(size_t)r].size), 0);
    }
    sel.distinct.clear();
    for (auto &kv : seen) {  // the map's order: ascending by offset
        kv.second = sel.distinct.size();
        sel.distinct.push_back(kv.first);
    }
    sel.slot.resize((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        const mrz_ar_rec &r = recs[(size_t)sel.rec[(size_t)k]];
        sel.slot[(size_t)k] = seen[std::make_pair(r.offset, r.size)];
    }
    return MRZ_OK;
}

// offsets and the sizing half of info; MRZ_E_ARG when `out` is there and too small
int ar_report(const ArSelection &sel, void *out, int64_t out_cap, int64_t *out_offsets, mrz_ar_extract_info *info) {
    memcpy(out_offsets, sel.at.data(), sel.at.size() * sizeof(int64_t));
    if (info)
        *info = mrz_ar_extract_info{ (int64_t)sel.rec.size(), (int64_t)sel.distinct.size(), sel.at.back(), 0, -1 };
    return out && out_cap < sel.at.back() ? MRZ_E_ARG : MRZ_OK;
}

// every distinct payload (at d_ptrs, in `where`) hashed once and held against the records of the selection
int ar_check(mrz_ctx *ctx, const std::vector<mrz_ar_rec> &recs, const ArSelection &sel,
             const std::vector<const void *> &ptrs, int where, mrz_ar_extract_info *info) {
    if (sel.distinct.empty() || sel.distinct.size() > 0x7fffffffu) return sel.distinct.empty() ? MRZ_OK : MRZ_E_UNSUPPORTED;
    std::vector<int64_t> lens(sel.distinct.size());
    for (size_t d = 0; d < lens.size(); d++) lens[d] = sel.distinct[d].second;
    std::vector<uint8_t> sums(lens.size() * MRZ_AR_SUM);
    const int rc = mrz_blake2b_batch(ctx, ptrs.data(), lens.data(), (int)lens.size(), where, MRZ_AR_SUM, sums.data());
    if (rc || !info) return rc;
    for (size_t k = 0; k < sel.rec.size(); k++)
        if (memcmp(recs[(size_t)sel.rec[k]].sum, &sums[sel.slot[k] * MRZ_AR_SUM], MRZ_AR_SUM)) {
            if (info->first_bad < 0) info->first_bad = (int64_t)k;
            info->n_bad++;
        }
    return MRZ_OK;
}

int ar_extract_impl(mrz_ctx *ctx, const void *ar, int64_t n, int where, const int64_t *which, int64_t n_which, void *out,
                    int out_where, int64_t out_cap, int64_t *out_offsets, int flags, mrz_ar_extract_info *info) {
    if (!ctx || !ar || n < 0 || !out_offsets || (flags & ~MRZ_AR_VERIFY) || (which && n_which < 0) ||
        (where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) ||
        (out && out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE) || (out && out_cap < 0))
        return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the metadata on the host, as mrz_ar_verify fetches it
    std::vector<uint8_t> copy;
    const uint8_t *meta = (const uint8_t *)ar;
    int64_t have = n;
    if (where == MRZ_MEM_DEVICE) {
        if (n < MRZ_AR_HEAD) return MRZ_E_CORRUPT;
        copy.resize(MRZ_AR_HEAD);
        HIPCHK(ctx, hipMemcpy(copy.data(), ar, MRZ_AR_HEAD, hipMemcpyDeviceToHost));
        int64_t m = 0;
        int rc = mrz_ar_read_head(copy.data(), n, &m);
        if (rc) return rc;
        copy.resize((size_t)(MRZ_AR_HEAD + m));
        if (m) HIPCHK(ctx, hipMemcpy(copy.data() + MRZ_AR_HEAD, (const uint8_t *)ar + MRZ_AR_HEAD, (size_t)m,
                                     hipMemcpyDeviceToHost));
        meta = copy.data();
        have = MRZ_AR_HEAD + m;
    }
    std::vector<mrz_ar_rec> recs;
    int64_t pay = 0;
    int rc = mrz_ar_read_prefix(meta, have, n, recs, &pay);
    if (rc) return rc;
    ArSelection sel;
    rc = ar_select(recs, which, n_which, sel);
    if (rc) return rc;
    rc = ar_report(sel, out, out_cap, out_offsets, info);
    if (rc || !out) return rc;
    const uint8_t *payload = (const uint8_t *)ar + pay;
    uint8_t *o = (uint8_t *)out;
    hipStream_t st = ctx->stream;
    const size_t ns = sel.rec.size();
    if (where == MRZ_MEM_DEVICE && out_where == MRZ_MEM_DEVICE) {  // one launch for all of them
        std::vector<const void *> src(ns);
        std::vector<void *> dst(ns);
        std::vector<int64_t> lens(ns);
        for (size_t k = 0; k < ns; k++) {
            const mrz_ar_rec &r = recs[(size_t)sel.rec[k]];
            src[k] = payload + r.offset;
            dst[k] = o + sel.at[k];
            lens[k] = r.size;
        }
        rc = mrz_copy_device_batch(ctx, src.data(), dst.data(), lens.data(), (int64_t)ns);
        if (rc) return rc;
    } else {
        for (size_t k = 0; k < ns; k++) {
            const mrz_ar_rec &r = recs[(size_t)sel.rec[k]];
            if (!r.size) continue;
            if (where == MRZ_MEM_HOST && out_where == MRZ_MEM_HOST)
                memcpy(o + sel.at[k], payload + r.offset, (size_t)r.size);
            else
                HIPCHK(ctx, hipMemcpyAsync(o + sel.at[k], payload + r.offset, (size_t)r.size,
                                           where == MRZ_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st));
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    if (!(flags & MRZ_AR_VERIFY)) return MRZ_OK;
    std::vector<const void *> ptrs(sel.distinct.size());
    for (size_t d = 0; d < ptrs.size(); d++)
        ptrs[d] = sel.distinct[d].second ? payload + sel.distinct[d].first : nullptr;
    return ar_check(ctx, recs, sel, ptrs, where, info);
}

void ar_add(mrz_archive_range_info *acc, const mrz_archive_range_info &p) {
    if (!acc) return;
    acc->chunks_in_range += p.chunks_in_range;
    acc->total_hops += p.total_hops;
    if (p.max_hops > acc->max_hops) acc->max_hops = p.max_hops;
    acc->s0_lz4_bytes += p.s0_lz4_bytes;
    acc->s1_blocks_touched += p.s1_blocks_touched;
    acc->s1_lz4_bytes += p.s1_lz4_bytes;
    acc->s1_bytes_uploaded += p.s1_bytes_uploaded;
}

// Three range calls on one context: the 13 bytes of the head, the metadata, the distinct payloads.  The parse of
// stream 0 is not kept between them: a chunk that holds the head, the metadata and a payload is parsed three times.
int ar_extract_mrz_impl(int device, const void *mrz, int64_t n, const int64_t *which, int64_t n_which, void *out,
                        int out_where, int64_t out_cap, int64_t *out_offsets, int flags, mrz_ar_extract_info *info,
                        mrz_archive_range_info *range_info) {
    if (range_info) memset(range_info, 0, sizeof(*range_info));
    if (!mrz || n < 0 || !out_offsets || (flags & ~MRZ_AR_VERIFY) || (which && n_which < 0) ||
        (out && out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE) || (out && out_cap < 0))
        return MRZ_E_ARG;
    CtxGuard g;
    int rc = mrz_open(&g.ctx, device, 7, 0);
    if (rc) return rc;
    mrz_ctx *ctx = g.ctx;
    mrz_archive_range_info part;
    int64_t file_len = 0;
    // 1. the head
    std::vector<uint8_t> head(MRZ_AR_HEAD);
    mrz_byte_range want{ 0, MRZ_AR_HEAD };
    rc = mrz_runzip_buffer_ranges_on(ctx, device, mrz, n, &want, 1, head.data(), MRZ_MEM_HOST, &file_len, &part);
    ar_add(range_info, part);
    if (rc == MRZ_E_ARG) rc = MRZ_E_CORRUPT;  // what the .mrz holds is shorter than an ARZIP's head
    if (rc) return rc;
    int64_t meta = 0;
    rc = mrz_ar_read_head(head.data(), file_len, &meta);
    if (rc) return rc;
    // 2. the metadata
    head.resize((size_t)(MRZ_AR_HEAD + meta));
    want = mrz_byte_range{ MRZ_AR_HEAD, meta };
    rc = mrz_runzip_buffer_ranges_on(ctx, device, mrz, n, &want, 1, head.data() + MRZ_AR_HEAD, MRZ_MEM_HOST, &file_len,
                                     &part);
    ar_add(range_info, part);
    if (rc) return rc;
    std::vector<mrz_ar_rec> recs;
    int64_t pay = 0;
    rc = mrz_ar_read_prefix(head.data(), (int64_t)head.size(), file_len, recs, &pay);
    if (rc) return rc;
    ArSelection sel;
    rc = ar_select(recs, which, n_which, sel);
    if (rc) return rc;
    rc = ar_report(sel, out, out_cap, out_offsets, info);
    if (rc || !out) return rc;
    // 3. the distinct payloads, ascending, packed into device memory by one call
    const size_t nd = sel.distinct.size(), ns = sel.rec.size();
    std::vector<mrz_byte_range> ranges(nd);
    std::vector<int64_t> d_at(nd + 1, 0);
    for (size_t d = 0; d < nd; d++) {
        ranges[d] = mrz_byte_range{ pay + sel.distinct[d].first, sel.distinct[d].second };
        d_at[d + 1] = d_at[d] + sel.distinct[d].second;
    }
    ArDevBuf packed;
    if (d_at[nd] && hipMalloc(&packed.p, (size_t)d_at[nd]) != hipSuccess) {
        packed.p = nullptr;
        return MRZ_E_NOMEM;
    }
    rc = mrz_runzip_buffer_ranges_on(ctx, device, mrz, n, ranges.data(), (int64_t)nd, packed.p, MRZ_MEM_DEVICE, &file_len,
                                     &part);
    ar_add(range_info, part);
    if (rc) return rc;
    const uint8_t *dp = (const uint8_t *)packed.p;
    uint8_t *o = (uint8_t *)out;
    if (out_where == MRZ_MEM_DEVICE) {  // duplicates and the selection's order: one launch
        std::vector<const void *> src(ns);
        std::vector<void *> dst(ns);
        std::vector<int64_t> lens(ns);
        for (size_t k = 0; k < ns; k++) {
            src[k] = dp + d_at[sel.slot[k]];
            dst[k] = o + sel.at[k];
            lens[k] = sel.distinct[sel.slot[k]].second;
        }
        rc = mrz_copy_device_batch(ctx, src.data(), dst.data(), lens.data(), (int64_t)ns);
        if (rc) return rc;
    } else if (d_at[nd]) {
        std::vector<uint8_t> host((size_t)d_at[nd]);
        HIPCHK(ctx, hipMemcpy(host.data(), dp, host.size(), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < ns; k++) {
            const int64_t len = sel.distinct[sel.slot[k]].second;
            if (len) memcpy(o + sel.at[k], host.data() + d_at[sel.slot[k]], (size_t)len);
        }
    }
    if (!(flags & MRZ_AR_VERIFY)) return MRZ_OK;
    // 4. the hashes, over the device bytes
    std::vector<const void *> ptrs(nd);
    for (size_t d = 0; d < nd; d++) ptrs[d] = sel.distinct[d].second ? dp + d_at[d] : nullptr;
    return ar_check(ctx, recs, sel, ptrs, MRZ_MEM_DEVICE, info);
}
}  // namespace

extern "C" int mrz_ar_extract(mrz_ctx *ctx, const void *ar, int64_t n, int where, const int64_t *which, int64_t n_which,
                              void *out, int out_where, int64_t out_cap, int64_t *out_offsets, int flags,
                              mrz_ar_extract_info *info) {
    try {
        return ar_extract_impl(ctx, ar, n, where, which, n_which, out, out_where, out_cap, out_offsets, flags, info);
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}

extern "C" int mrz_ar_extract_mrz(int device, const void *mrz, int64_t n, const int64_t *which, int64_t n_which, void *out,
                                  int out_where, int64_t out_cap, int64_t *out_offsets, int flags,
                                  mrz_ar_extract_info *info, mrz_archive_range_info *range_info) {
    try {
        return ar_extract_mrz_impl(device, mrz, n, which, n_which, out, out_where, out_cap, out_offsets, flags, info,
                                   range_info);
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}
