// mrz_archive.h -- the framing of a -n / -l archive as the three runzip entry points read it: magic header, chunk
// headers, the block chains of the two streams, the decoded length of a chunk and the arithmetic of a byte range over
// the chunks.  Everything that reads archive bytes is here, and nothing else: host code without a HIP call or include
// and without mrz_ctx, so that tests/c/archive_test.cpp drives it on its own.  The drivers (mrz_unarchive.hip) own the
// context, the device buffers and the data paths.  The bytes are untrusted: every rule below is a verdict of the ABI.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/mrzgpu.h"  // the MRZ_E_* codes

enum { MRZ_CTYPE_NONE = 3, MRZ_CTYPE_LZ4 = 5 };
constexpr int64_t kLz4MaxInput = 0x7E000000ll;

static inline int64_t mrz_arc_le(const uint8_t *p, int nbytes) {
    uint64_t v = 0;
    for (int i = 0; i < nbytes; i++) v |= (uint64_t)p[i] << (8 * i);
    return (int64_t)v;
}

// the magic header (read_magic, src/mrzip.c:225-321): the size it carries (<= 0: none; an archive written to STDOUT in
// several chunks, src/mrzip.c:137-140), the hash in use and where the first chunk begins
struct mrz_arc_header {
    int64_t expected;
    int hash_code;  // 0: per-chunk CRC only, 1: MD5 behind the last chunk
    int64_t first_chunk;
    bool size_known() const { return expected > 0; }
};

static inline int mrz_arc_read_header(const uint8_t *mrz, int64_t n, mrz_arc_header *h) {
    if (n < 20 || memcmp(mrz, "MRZI", 4)) return MRZ_E_CORRUPT;
    if (mrz[15]) return MRZ_E_UNSUPPORTED;  // encrypted
    h->expected = mrz_arc_le(mrz + 6, 8);
    h->hash_code = mrz[14];
    if (h->hash_code != 0 && h->hash_code != 1) return MRZ_E_UNSUPPORTED;  // MD5 (default) or CRC only
    h->first_chunk = 20 + mrz[19];
    return MRZ_OK;
}

// One block of a stream: CTYPE_NONE, or CTYPE_LZ4 as `mrzip -l` writes it (lz4_compress_buf, src/stream.c:278-312)
struct mrz_arc_block {
    int ctype;
    const uint8_t *p;
    int64_t c_len, u_len;
};

// which blocks a caller takes; under NONE_ONLY an LZ4 block is MRZ_E_UNSUPPORTED whatever its lengths say
enum mrz_arc_policy { MRZ_ARC_NONE_ONLY, MRZ_ARC_NONE_LZ4 };

// follows one stream's block chain (fill_buffer, src/stream.c:1412-1571): the chain's blocks in order, *total their
// decoded length, *end_max raised to the end of the last payload byte seen.  The order of the checks is behaviour.
static inline int mrz_arc_walk_chain(const uint8_t *mrz, int64_t n, int64_t initial_pos, int64_t head_at, int cb,
                                     mrz_arc_policy policy, std::vector<mrz_arc_block> &blocks, int64_t *total,
                                     int64_t *end_max) {
    int64_t at = head_at;
    *total = 0;
    for (;;) {
        if (at + 1 + 3 * cb > n) return MRZ_E_CORRUPT;
        const int ctype = mrz[at];
        const int64_t c_len = mrz_arc_le(mrz + at + 1, cb), u_len = mrz_arc_le(mrz + at + 1 + cb, cb);
        const int64_t next = mrz_arc_le(mrz + at + 1 + 2 * cb, cb);
        if (ctype != MRZ_CTYPE_NONE && !(ctype == MRZ_CTYPE_LZ4 && policy == MRZ_ARC_NONE_LZ4)) return MRZ_E_UNSUPPORTED;
        if (c_len < 0 || u_len < 0) return MRZ_E_CORRUPT;
        if (ctype == MRZ_CTYPE_NONE && c_len != u_len) return MRZ_E_CORRUPT;
        const int64_t pay = at + 1 + 3 * cb;
        if (c_len > n - pay) return MRZ_E_CORRUPT;  // (compared without adding: a length field may be 2^63 - 1)
        if (ctype == MRZ_CTYPE_LZ4) {
            if (u_len > kLz4MaxInput) return MRZ_E_UNSUPPORTED;
            // no LZ4 block is longer than LZ4_compressBound of what it holds, and none holds more than 255 bytes per
            // byte of its own (a length byte adds at most 255): whatever claims otherwise is not worth an allocation
            if (c_len > u_len + u_len / 255 + 16 || u_len / 255 > c_len) return MRZ_E_CORRUPT;
        }
        blocks.push_back(mrz_arc_block{ ctype, mrz + pay, c_len, u_len });
        *total += u_len;
        if (pay + c_len > *end_max) *end_max = pay + c_len;
        if (!next) return MRZ_OK;
        if (next < 0 || next > n - initial_pos || initial_pos + next <= at) return MRZ_E_CORRUPT;  // chains only run forward
        at = initial_pos + next;
    }
}

// One chunk as the cursor yields it (runzip_chunk, src/runzip.c:226-330); what it decodes to: mrz_arc_records_out_len
struct mrz_arc_chunk {
    int cb, eof;
    std::vector<mrz_arc_block> blocks[2];
    int64_t stream_len[2];  // what the blocks of each stream decode to
    bool has_lz4(int s) const {
        for (const mrz_arc_block &b : blocks[s])
            if (b.ctype == MRZ_CTYPE_LZ4) return true;
        return false;
    }
    // the payloads of a stream, concatenated: what it decodes to where it holds no LZ4 block
    void gather(int s, std::vector<uint8_t> &dst) const {
        dst.clear();
        for (const mrz_arc_block &b : blocks[s]) dst.insert(dst.end(), b.p, b.p + b.c_len);
    }
};

// Pulls one chunk per next(): header and both chains, nothing behind them.  A caller that stops early has looked at no
// byte from `at` on -- behind a header that carries the size the range calls stop at the chunk that covers the range.
struct mrz_arc_cursor {
    const uint8_t *mrz;
    int64_t n;
    int64_t at;  // where the next chunk begins (at first: the header's first_chunk); behind the last: where the MD5 is
    mrz_arc_policy policy;
    int next(mrz_arc_chunk &c) {
        if (at + 2 > n) return MRZ_E_CORRUPT;
        const int cb = c.cb = mrz[at];
        c.eof = mrz[at + 1];
        if (cb < 1 || cb > 8 || at + 2 + cb > n) return MRZ_E_CORRUPT;
        // chunk_bytes, eof, chunk size (the field is chunk_bytes wide: a chunk below one page does not fit its own
        // size there, src/stream.c:779-780,1224 -- so it is not used for sizing)
        const int64_t initial_pos = at + 2 + cb;
        int64_t end_max = initial_pos + 2 * (1 + 3 * cb);
        c.blocks[0].clear();
        c.blocks[1].clear();
        c.stream_len[0] = c.stream_len[1] = 0;
        for (int s = 0; s < 2; s++) {
            const int rc = mrz_arc_walk_chain(mrz, n, initial_pos, initial_pos + s * (1 + 3 * cb), cb, policy, c.blocks[s],
                                              &c.stream_len[s], &end_max);
            if (rc) return rc;
        }
        at = end_max;
        return MRZ_OK;
    }
};

// bytes a chunk decodes to: the lengths of the records of a gathered stream 0 (3 or 3 + cb bytes each; one with LZ4
// blocks has its length from the device parse instead); false without a terminator
static inline bool mrz_arc_records_out_len(const uint8_t *s0, int64_t n0, int cb, int64_t *out_len) {
    int64_t need = 0, i = 0;
    while (i + 3 <= n0) {
        const int64_t len = s0[i + 1] | (int64_t)s0[i + 2] << 8;
        if (s0[i] == 0) {
            if (len == 0) {
                *out_len = need;
                return true;
            }
            i += 3;
        } else
            i += 3 + cb;
        need += len;
    }
    return false;
}

// Bytes [first, first + count) of the file against the chunks, as both range calls judge them.  The caller walks the
// chunks and adds each one's decoded length to `total`.
struct mrz_arc_range {
    int64_t first, count;
    bool size_known;
    bool bad;       // no file has such a range: the walk goes on (without a size the length is owed), the work does not
    int64_t total;  // decoded bytes of the chunks passed so far

    // against a header that carries the size: *file_len first, then the verdict on the arguments
    int begin(const mrz_arc_header &h, int64_t first_, int64_t count_, int64_t *file_len) {
        *this = mrz_arc_range{ first_, count_, h.size_known(), first_ < 0 || count_ < 0 || count_ > INT64_MAX - first_, 0 };
        if (size_known && file_len) *file_len = h.expected;
        return size_known && (bad || first > h.expected || count > h.expected - first) ? MRZ_E_ARG : MRZ_OK;
    }
    // the part of the next chunk (chunk_len bytes from `total` on) inside the range: bytes [*lo, *lo + *cnt) of the
    // chunk go to the output at *out_at; false: outside
    bool clip(int64_t chunk_len, int64_t *lo, int64_t *cnt, int64_t *out_at) const {
        if (bad || count <= 0 || total >= first + count || total + chunk_len <= first) return false;
        const int64_t a = first > total ? first : total;
        const int64_t b = first + count < total + chunk_len ? first + count : total + chunk_len;
        *lo = a - total;
        *cnt = b - a;
        *out_at = a - first;
        return true;
    }
    bool covered() const { return size_known && total >= first + count; }  // nothing past the range is looked at

    // after the walk: the length where the header had none, and what is left to say about the range
    int finish(int64_t *file_len) const {
        if (!size_known) {
            if (file_len) *file_len = total;
            if (bad || first > total || count > total - first) return MRZ_E_ARG;
        } else if (total < first + count)
            return MRZ_E_CORRUPT;  // fewer bytes than the header promised
        return MRZ_OK;
    }
};

// A list of ranges of the file against the chunks (mrz_runzip_buffer_ranges): mrz_arc_range for many ranges at once.
// The output is packed in list order: range k goes to output offset sum(count_j, j < k).  The caller walks the chunks,
// asks for the parts of each one and adds its decoded length to `total`.
struct mrz_arc_part {
    int64_t lo, cnt;  // bytes [lo, lo + cnt) of the chunk ...
    int64_t out_at;   // ... go to output offset out_at
};

struct mrz_arc_ranges {
    const mrz_byte_range *ranges;
    int64_t n;
    std::vector<int64_t> out_base;  // where each range begins in the output (meaningless when bad)
    bool size_known;
    bool bad;          // no file has such a list: the walk goes on (without a size the length is owed), the work does not
    int64_t sum;       // bytes asked for
    int64_t last_end;  // the end of the last byte any non-empty range asks for: nothing behind it is needed
    int64_t total;     // decoded bytes of the chunks passed so far

    // against a header that carries the size: *file_len first, then the verdict on the list
    int begin(const mrz_arc_header &h, const mrz_byte_range *ranges_, int64_t n_, int64_t *file_len) {
        ranges = ranges_;
        n = n_;
        size_known = h.size_known();
        bad = false;
        sum = last_end = total = 0;
        out_base.assign((size_t)n, 0);
        if (size_known && file_len) *file_len = h.expected;
        bool beyond = false;
        for (int64_t k = 0; k < n && !bad; k++) {
            const int64_t first = ranges[k].first, count = ranges[k].count;
            if (first < 0 || count < 0 || count > INT64_MAX - first || count > INT64_MAX - sum) {
                bad = true;
                break;
            }
            out_base[(size_t)k] = sum;
            sum += count;
            if (count > 0 && first + count > last_end) last_end = first + count;
            if (size_known && (first > h.expected || count > h.expected - first)) beyond = true;
        }
        return size_known && (bad || beyond) ? MRZ_E_ARG : MRZ_OK;
    }
    // the parts of the next chunk (chunk_len bytes from `total` on) that the ranges ask for, in list order; false: none
    bool clip(int64_t chunk_len, std::vector<mrz_arc_part> &parts) const {
        parts.clear();
        if (bad || sum <= 0 || total >= last_end) return false;
        for (int64_t k = 0; k < n; k++) {
            const int64_t first = ranges[k].first, count = ranges[k].count;
            if (count <= 0 || total >= first + count || total + chunk_len <= first) continue;
            const int64_t a = first > total ? first : total;
            const int64_t b = first + count < total + chunk_len ? first + count : total + chunk_len;
            if (b <= a) continue;  // an empty chunk inside the range
            parts.push_back(mrz_arc_part{ a - total, b - a, out_base[(size_t)k] + (a - first) });
        }
        return !parts.empty();
    }
    // the parts follow each other in the output without a gap: they can be written in place
    static bool contiguous(const std::vector<mrz_arc_part> &parts) {
        for (size_t k = 1; k < parts.size(); k++)
            if (parts[k].out_at != parts[k - 1].out_at + parts[k - 1].cnt) return false;
        return true;
    }
    bool covered() const { return size_known && total >= last_end; }  // nothing past the last range is looked at

    // after the walk: the length where the header had none, and what is left to say about the list
    int finish(int64_t *file_len) const {
        if (!size_known) {
            if (file_len) *file_len = total;
            if (bad) return MRZ_E_ARG;
            for (int64_t k = 0; k < n; k++)
                if (ranges[k].first > total || ranges[k].count > total - ranges[k].first) return MRZ_E_ARG;
        } else if (total < last_end)
            return MRZ_E_CORRUPT;  // fewer bytes than the header promised
        return MRZ_OK;
    }
};

// A stream's blocks with the stream offset each one starts at (CTYPE_NONE: the bytes stay in the archive).
struct mrz_arc_table {
    std::vector<mrz_arc_block> blocks;
    std::vector<int64_t> starts;
    void set(std::vector<mrz_arc_block> b) {
        blocks = std::move(b);
        starts.clear();
        int64_t at = 0;
        for (const mrz_arc_block &k : blocks) {
            starts.push_back(at);
            at += k.u_len;
        }
    }
    // n bytes of the stream from offset `at` ([at, at + n) lies inside it); CTYPE_NONE blocks only
    void copy(int64_t at, int64_t n, uint8_t *dst) const {
        // from the last block that starts at or before `at`
        size_t lo = (size_t)(std::upper_bound(starts.begin(), starts.end(), at) - starts.begin()) - 1;
        while (n > 0) {
            const int64_t off = at - starts[lo];
            const mrz_arc_block &b = blocks[lo++];
            const int64_t take = b.c_len - off < n ? b.c_len - off : n;
            if (take > 0) memcpy(dst, b.p + off, (size_t)take);
            dst += take;
            at += take;
            n -= take;
        }
    }
};
