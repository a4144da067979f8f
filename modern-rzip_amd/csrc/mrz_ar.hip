// mrz_ar.hip -- the drivers of the ARZIP entry points: create() of ar-mrzip over members in memory (checksums and
// digests on the device, the order on the device, the collapse and the framing on the host: mrz_ar_index.h), the
// parser's ABI face and the verifier.  Everything that knows the archive's bytes is in mrz_ar_index.h; everything that
// computes is in mrz_blake2b.hip and mrz_tlsh.hip.  This file owns the data paths.
#include <string.h>

#include <vector>

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
