// mrz_ar_index.h -- the "ARZIP" solid archive as ar-mrzip writes and reads it (ar-mrzip/ar-mrzip.cpp:395-401, 440-532,
// 540-580): the collapse of exact duplicates, the size arithmetic, the metadata writer and the parser.  Host code
// without a HIP call or include and without mrz_ctx, so that tests/c/ar_index_test.cpp drives it on its own; the driver
// (mrz_ar.hip) owns the context, the hashes and the payload copies.  Parsed bytes are untrusted: every rule of
// mrz_ar_read below is a verdict of the ABI.
//
//   "ARZIP" | u64be metadata_size | one record per member, in archive order | payload
//   record:  u64be mtime | u64be size | u64be offset | 64 bytes BLAKE2b-512 | 137 bytes TLSH | u32be name_len | name
// metadata_size is the sum of the records' lengths; `offset` counts from the start of the payload.  The payload holds
// every member whose offset is the running write offset, i.e. the first member of every distinct checksum.
#pragma once
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/mrzgpu.h"  // the MRZ_E_* codes

#define MRZ_AR_DIGEST 137
#define MRZ_AR_SUM 64
#define MRZ_AR_HEAD 13                                    // magic + metadata_size
#define MRZ_AR_FIXED (24 + MRZ_AR_SUM + MRZ_AR_DIGEST + 4)  // a record without its name

struct mrz_ar_rec {
    uint64_t mtime;
    int64_t size;
    int64_t offset;
    uint8_t sum[MRZ_AR_SUM];
    uint8_t digest[MRZ_AR_DIGEST];
    const uint8_t *name;
    uint32_t name_len;
    int64_t index;      // writer: the member's place in the caller's list; reader: the record's place in the archive
    int64_t record_at;  // reader: where the record begins in the archive
};

static inline void mrz_ar_put_be(uint8_t *p, uint64_t v, int nbytes) {
    for (int i = 0; i < nbytes; i++) p[i] = (uint8_t)(v >> (8 * (nbytes - 1 - i)));
}

static inline uint64_t mrz_ar_get_be(const uint8_t *p, int nbytes) {
    uint64_t v = 0;
    for (int i = 0; i < nbytes; i++) v = (v << 8) | p[i];
    return v;
}

// Walks the records in order: the first one of a checksum takes the running offset, which then grows by its size; the
// later ones share that offset.  *unique: bytes the payload will hold; *duplicate: bytes it is spared.
static inline void mrz_ar_collapse(std::vector<mrz_ar_rec> &recs, int64_t *unique, int64_t *duplicate) {
    std::map<std::string, int64_t> seen;
    int64_t at = 0, dup = 0;
    for (auto &r : recs) {
        auto ins = seen.emplace(std::string((const char *)r.sum, MRZ_AR_SUM), at);
        r.offset = ins.first->second;
        if (ins.second)
            at += r.size;
        else
            dup += r.size;
    }
    *unique = at;
    *duplicate = dup;
}

static inline int64_t mrz_ar_metadata_size(const std::vector<mrz_ar_rec> &recs) {
    int64_t s = 0;
    for (const auto &r : recs) s += (int64_t)r.name_len + MRZ_AR_FIXED;
    return s;
}

// magic, metadata_size and the records into out[0, MRZ_AR_HEAD + metadata_size); returns that length
static inline int64_t mrz_ar_write_metadata(const std::vector<mrz_ar_rec> &recs, uint8_t *out) {
    memcpy(out, "ARZIP", 5);
    mrz_ar_put_be(out + 5, (uint64_t)mrz_ar_metadata_size(recs), 8);
    uint8_t *p = out + MRZ_AR_HEAD;
    for (const auto &r : recs) {
        mrz_ar_put_be(p, r.mtime, 8);
        mrz_ar_put_be(p + 8, (uint64_t)r.size, 8);
        mrz_ar_put_be(p + 16, (uint64_t)r.offset, 8);
        memcpy(p + 24, r.sum, MRZ_AR_SUM);
        memcpy(p + 24 + MRZ_AR_SUM, r.digest, MRZ_AR_DIGEST);
        mrz_ar_put_be(p + 24 + MRZ_AR_SUM + MRZ_AR_DIGEST, r.name_len, 4);
        if (r.name_len) memcpy(p + MRZ_AR_FIXED, r.name, r.name_len);
        p += MRZ_AR_FIXED + r.name_len;
    }
    return (int64_t)(p - out);
}

// the records that own payload bytes, in payload order: those whose offset is the running write offset
static inline std::vector<size_t> mrz_ar_payload_plan(const std::vector<mrz_ar_rec> &recs) {
    std::vector<size_t> plan;
    int64_t at = 0;
    for (size_t i = 0; i < recs.size(); i++)
        if (recs[i].offset == at) {
            plan.push_back(i);
            at += recs[i].size;
        }
    return plan;
}

// The header alone (the first MRZ_AR_HEAD bytes of an archive of n bytes): the length of the metadata
static inline int mrz_ar_read_head(const uint8_t *ar, int64_t n, int64_t *metadata_size) {
    if (n < MRZ_AR_HEAD || memcmp(ar, "ARZIP", 5)) return MRZ_E_CORRUPT;
    const uint64_t m = mrz_ar_get_be(ar + 5, 8);
    if (m > (uint64_t)(n - MRZ_AR_HEAD)) return MRZ_E_CORRUPT;  // truncated metadata
    *metadata_size = (int64_t)m;
    return MRZ_OK;
}

// Parses ar[0, have) of an archive of n bytes; `have` must cover the metadata.  MRZ_E_CORRUPT unless the magic is
// there, the records consume metadata_size exactly and every offset + size lies inside the payload.  Names point into
// `ar`.
static inline int mrz_ar_read(const uint8_t *ar, int64_t have, int64_t n, std::vector<mrz_ar_rec> &recs,
                              int64_t *payload_at) {
    int64_t meta = 0;
    int rc = mrz_ar_read_head(ar, have < n ? have : n, &meta);
    if (rc) return rc;
    if (meta > n - MRZ_AR_HEAD || meta > have - MRZ_AR_HEAD) return MRZ_E_CORRUPT;
    const int64_t end = MRZ_AR_HEAD + meta, payload = n - end;
    int64_t at = MRZ_AR_HEAD;
    recs.clear();
    while (at < end) {
        if (end - at < MRZ_AR_FIXED) return MRZ_E_CORRUPT;
        mrz_ar_rec r;
        r.mtime = mrz_ar_get_be(ar + at, 8);
        const uint64_t size = mrz_ar_get_be(ar + at + 8, 8), offset = mrz_ar_get_be(ar + at + 16, 8);
        if (size > (uint64_t)payload || offset > (uint64_t)payload - size) return MRZ_E_CORRUPT;
        r.size = (int64_t)size;
        r.offset = (int64_t)offset;
        memcpy(r.sum, ar + at + 24, MRZ_AR_SUM);
        memcpy(r.digest, ar + at + 24 + MRZ_AR_SUM, MRZ_AR_DIGEST);
        r.name_len = (uint32_t)mrz_ar_get_be(ar + at + 24 + MRZ_AR_SUM + MRZ_AR_DIGEST, 4);
        if ((int64_t)r.name_len > end - at - MRZ_AR_FIXED) return MRZ_E_CORRUPT;
        r.name = ar + at + MRZ_AR_FIXED;
        r.index = (int64_t)recs.size();
        r.record_at = at;
        recs.push_back(r);
        at += MRZ_AR_FIXED + r.name_len;
    }
    *payload_at = end;
    return MRZ_OK;
}

// The same verdicts from the head alone: head[0, head_len) is the start of an archive of total_len bytes that the
// caller does not hold (mrz_ar_extract_mrz decodes nothing of it but these bytes).  head_len must be exactly
// MRZ_AR_HEAD + metadata_size, or at least MRZ_AR_HEAD + metadata_size when the caller holds more (a whole archive):
// fewer bytes are MRZ_E_CORRUPT like a truncated archive, and so is a total_len that cannot hold head_len.  No byte at
// or behind head_len is read; the payload's extent, against which every offset + size is judged, comes from total_len.
static inline int mrz_ar_read_prefix(const uint8_t *head, int64_t head_len, int64_t total_len,
                                     std::vector<mrz_ar_rec> &recs, int64_t *payload_at) {
    if (!head || head_len < 0 || total_len < head_len) return MRZ_E_CORRUPT;
    return mrz_ar_read(head, head_len, total_len, recs, payload_at);
}
