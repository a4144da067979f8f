// tests/c/archive_test.cpp -- TEST: the archive framing of the three runzip entry points (mrz_archive.h) on its own.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imodern-rzip_amd/csrc tests/c/archive_test.cpp -o archive_test
//
// No HIP, no library: archives come from the framing writer below (what Sink::put_block of mrz_host.hip writes: chunk
// header, the two empty head blocks, then blocks in flush order with `next` patched into the previous header of the
// same stream).  Payload bytes are arbitrary except where a stream 0 is walked for its records.  Every parse runs on a
// heap copy of exactly the archive's length, so the address sanitizer sees any read past n.
//
// The expected code of every refusal is what the three entry points of the commit BEFORE this parser existed returned
// for the same bytes (emulator build; `archive_test DIR` writes each case to DIR/<index>.bin and prints the table, a
// few lines of ctypes did the rest): `lz4` is mrz_runzip_buffer and mrz_runzip_buffer_range_ex (CTYPE_NONE and
// CTYPE_LZ4), `none` is mrz_runzip_buffer_range (CTYPE_NONE only).  Where include/mrzgpu_host.h states the case, the
// line is cited.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mrz_archive.h"

#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "archive_test: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                            \
            fprintf(stderr, "\n  in %s\n", g_case.c_str());                          \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)
static std::string g_case;

typedef std::vector<uint8_t> Bytes;

// ---- the framing writer ---------------------------------------------------------------------------------------------
struct ExpBlock {
    int ctype;
    int64_t hdr_at, pay_at, c_len, u_len;
};
struct ExpChunk {
    int cb, eof;
    int64_t at, initial_pos, next_at;
    std::vector<ExpBlock> blocks[2];
    int64_t len(int s) const {
        int64_t v = 0;
        for (const ExpBlock &b : blocks[s]) v += b.u_len;
        return v;
    }
};
struct Writer {
    Bytes out;
    std::vector<bool> framing;  // per byte of `out`: not payload
    std::vector<ExpChunk> chunks;
    int64_t last_next[2];

    void put(int64_t v, int width) {
        for (int i = 0; i < width; i++) out.push_back((uint8_t)((uint64_t)v >> (8 * i)));
        framing.resize(out.size(), true);
    }
    void magic(int64_t size, int hash_code, int extra = 0) {
        out.assign(20 + extra, 0);
        memcpy(out.data(), "MRZI", 4);
        out[5] = 9;
        for (int i = 0; i < 8; i++) out[6 + i] = (uint8_t)((uint64_t)size >> (8 * i));
        out[14] = (uint8_t)hash_code;
        out[19] = (uint8_t)extra;
        framing.assign(out.size(), true);
    }
    void block(int s, int ctype, int64_t c_len, int64_t u_len, const uint8_t *payload = nullptr) {
        ExpChunk &c = chunks.back();
        const int64_t at = (int64_t)out.size();
        if (last_next[s] >= 0)
            for (int i = 0; i < c.cb; i++) out[last_next[s] + i] = (uint8_t)((uint64_t)(at - c.initial_pos) >> (8 * i));
        out.push_back((uint8_t)ctype);
        put(c_len, c.cb);
        put(u_len, c.cb);
        last_next[s] = (int64_t)out.size();
        put(0, c.cb);
        c.blocks[s].push_back(ExpBlock{ ctype, at, (int64_t)out.size(), c_len, u_len });
        for (int64_t i = 0; i < c_len; i++) out.push_back(payload ? payload[i] : (uint8_t)(0xA5 + 7 * i + s));
        framing.resize(out.size(), false);
        c.next_at = (int64_t)out.size();
    }
    void chunk(int cb, int eof) {
        chunks.push_back(ExpChunk());
        ExpChunk &c = chunks.back();
        c.cb = cb;
        c.eof = eof;
        c.at = (int64_t)out.size();
        out.push_back((uint8_t)cb);
        out.push_back((uint8_t)eof);
        put(4096, cb);  // the size field: never used for sizing
        c.initial_pos = (int64_t)out.size();
        last_next[0] = last_next[1] = -1;
        block(0, 3, 0, 0);
        block(1, 3, 0, 0);
    }
    void md5() {
        put(0x5d5d5d5d5d5d5d5dll, 8);
        put(0x5d5d5d5d5d5d5d5dll, 8);
    }
};

void poke(Bytes &b, int64_t at, int width, int64_t v) {
    for (int i = 0; i < width; i++) b[(size_t)(at + i)] = (uint8_t)((uint64_t)v >> (8 * i));
}

// a stream 0 that decodes to `lit` bytes: one literal record, the terminator, four CRC bytes
Bytes records(int lit, bool terminator = true) {
    Bytes r = { 0, (uint8_t)lit, (uint8_t)(lit >> 8) };
    if (terminator) r.insert(r.end(), { 0, 0, 0, 1, 2, 3, 4 });
    return r;
}

// ---- a parse as the range calls' host side does it ------------------------------------------------------------------
struct Exact {  // a heap copy of exactly n bytes
    uint8_t *p;
    int64_t n;
    Exact(const Bytes &b, int64_t n_) : p((uint8_t *)malloc((size_t)n_)), n(n_) {
        if (n) memcpy(p, b.data(), (size_t)n);
    }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
};

struct Parsed {
    mrz_arc_header h;
    std::vector<mrz_arc_chunk> chunks;
    std::vector<int64_t> next_at, chunk_len;  // chunk_len -1: stream 0 holds an LZ4 block
    int64_t total;
};

// header, then up to max_chunks chunks; a stream 0 without LZ4 blocks is gathered and walked, a stream 1 without is
// read whole through its table
int parse(const Exact &a, mrz_arc_policy policy, Parsed &r, size_t max_chunks = 1000) {
    r = Parsed();
    int rc = mrz_arc_read_header(a.p, a.n, &r.h);
    if (rc) return rc;
    mrz_arc_cursor cur{ a.p, a.n, r.h.first_chunk, policy };
    mrz_arc_chunk c;
    Bytes s0;
    while (r.chunks.size() < max_chunks) {
        rc = cur.next(c);
        if (rc) return rc;
        int64_t chunk_len = -1;
        if (!c.has_lz4(0)) {
            c.gather(0, s0);
            CHECK((int64_t)s0.size() == c.stream_len[0], "gathered %zu", s0.size());
            if (!mrz_arc_records_out_len(s0.data(), (int64_t)s0.size(), c.cb, &chunk_len)) return MRZ_E_CORRUPT;
            r.total += chunk_len;
        }
        r.chunks.push_back(c);
        r.next_at.push_back(cur.at);
        r.chunk_len.push_back(chunk_len);
        if (!c.has_lz4(1) && c.stream_len[1] > 0) {
            mrz_arc_table t;
            t.set(c.blocks[1]);
            Bytes all((size_t)c.stream_len[1]), part(all.size());
            t.copy(0, c.stream_len[1], all.data());
            for (int64_t from = 0; from < c.stream_len[1]; from++) {  // ... and from every offset
                t.copy(from, c.stream_len[1] - from, part.data());
                CHECK(!memcmp(part.data(), all.data() + from, (size_t)(c.stream_len[1] - from)), "from %lld", (long long)from);
            }
            c.gather(1, part);
            CHECK(part == all, "table copy differs from gather");
        }
        if (c.eof) break;
    }
    return MRZ_OK;
}

void check_against(const Writer &w, const Exact &a, const Parsed &r, size_t nchunks) {
    CHECK(r.chunks.size() == nchunks, "%zu chunks", r.chunks.size());
    for (size_t k = 0; k < nchunks; k++) {
        const ExpChunk &e = w.chunks[k];
        const mrz_arc_chunk &c = r.chunks[k];
        CHECK(c.cb == e.cb && c.eof == e.eof, "chunk %zu: cb %d eof %d", k, c.cb, c.eof);
        CHECK(r.next_at[k] == e.next_at, "chunk %zu: next at %lld, expected %lld", k, (long long)r.next_at[k], (long long)e.next_at);
        for (int s = 0; s < 2; s++) {
            CHECK(c.blocks[s].size() == e.blocks[s].size(), "chunk %zu stream %d: %zu blocks", k, s, c.blocks[s].size());
            CHECK(c.stream_len[s] == e.len(s), "chunk %zu stream %d: length %lld", k, s, (long long)c.stream_len[s]);
            for (size_t i = 0; i < e.blocks[s].size(); i++) {
                const mrz_arc_block &b = c.blocks[s][i];
                const ExpBlock &x = e.blocks[s][i];
                CHECK(b.p == a.p + x.pay_at && b.c_len == x.c_len && b.u_len == x.u_len && b.ctype == x.ctype,
                      "chunk %zu stream %d block %zu: at %lld c_len %lld u_len %lld ctype %d", k, s, i, (long long)(b.p - a.p),
                      (long long)b.c_len, (long long)b.u_len, b.ctype);
            }
        }
    }
}

// ---- accepted archives ----------------------------------------------------------------------------------------------
// `nchunks` chunks of `cb`; stream 0 is records for `lit` literal bytes cut into three blocks, stream 1 several blocks
// interleaved with them (or none at all); with `lz4`, some blocks of stream 1 -- and of the LAST chunk's stream 0 -- are
// CTYPE_LZ4 with lengths the size rules pass
Writer valid_archive(int cb, int nchunks, bool with_size, int hash_code, bool lz4, bool empty_s1, int extra = 0) {
    Writer w;
    const int lit = 9;
    w.magic(with_size ? (int64_t)lit * nchunks : 0, hash_code, extra);
    for (int k = 0; k < nchunks; k++) {
        const bool last = k == nchunks - 1;
        w.chunk(cb, last);
        const Bytes r = records(lit);
        const bool lz4_s0 = lz4 && last && nchunks > 1;
        if (lz4_s0)
            w.block(0, 5, 7, 10);
        else
            w.block(0, 3, 4, 4, r.data());
        if (!empty_s1) w.block(1, 3, 3, 3);
        if (!empty_s1) w.block(1, lz4 ? 5 : 3, lz4 ? 9 : 2, lz4 ? 30 : 2);
        if (!lz4_s0) w.block(0, 3, 0, 0, r.data() + 4);  // an empty block in the middle of a chain
        if (!lz4_s0) w.block(0, 3, 6, 6, r.data() + 4);
        if (!empty_s1) w.block(1, 3, 4, 4);
    }
    if (hash_code == 1) w.md5();
    return w;
}

void test_accepts() {
    int n_archives = 0;
    for (int cb : { 1, 2, 4, 8 })
        for (int nchunks : { 1, 2 })
            for (int with_size = 0; with_size < 2; with_size++)
                for (int hash_code = 0; hash_code < 2; hash_code++)
                    for (int lz4 = 0; lz4 < 2; lz4++)
                        for (int empty_s1 = 0; empty_s1 < 2; empty_s1++) {
                            char name[160];
                            snprintf(name, sizeof name, "accept cb=%d chunks=%d size=%d hash=%d lz4=%d empty_s1=%d", cb, nchunks,
                                     with_size, hash_code, lz4, empty_s1);
                            g_case = name;
                            const int extra = (cb + nchunks) % 3;  // bytes between magic and first chunk (mrz[19])
                            const Writer w = valid_archive(cb, nchunks, with_size, hash_code, lz4, empty_s1, extra);
                            const Exact a(w.out, (int64_t)w.out.size());
                            Parsed r;
                            int rc = parse(a, MRZ_ARC_NONE_LZ4, r);
                            CHECK(rc == MRZ_OK, "rc %d", rc);
                            check_against(w, a, r, (size_t)nchunks);
                            CHECK(r.h.hash_code == hash_code && r.h.size_known() == (with_size != 0) && r.h.first_chunk == 20 + extra,
                                  "header: hash %d expected %lld first chunk %lld", r.h.hash_code, (long long)r.h.expected,
                                  (long long)r.h.first_chunk);
                            if (with_size) CHECK(r.h.expected == 9 * nchunks, "expected %lld", (long long)r.h.expected);
                            CHECK(r.chunk_len[0] == 9, "chunk length %lld", (long long)r.chunk_len[0]);
                            CHECK(r.next_at.back() + (hash_code == 1 ? 16 : 0) == a.n, "the MD5 is not where the cursor ended");
                            // the NONE-only policy: the same answer without LZ4 blocks, MRZ_E_UNSUPPORTED with them
                            Parsed r2;
                            rc = parse(a, MRZ_ARC_NONE_ONLY, r2);
                            const bool any_lz4 = lz4 && !(empty_s1 && nchunks == 1);
                            CHECK(rc == (any_lz4 ? MRZ_E_UNSUPPORTED : MRZ_OK), "NONE only: rc %d", rc);
                            if (!any_lz4) check_against(w, a, r2, (size_t)nchunks);
                            // lazy: a cursor stopped behind chunk 0 has read nothing behind it -- the archive cut there
                            // gives the same chunk, and only the next step fails
                            if (nchunks == 2) {
                                const Exact cut(w.out, w.chunks[0].next_at);
                                Parsed r3;
                                rc = parse(cut, MRZ_ARC_NONE_LZ4, r3, 1);
                                CHECK(rc == MRZ_OK, "cut behind chunk 0: rc %d", rc);
                                check_against(w, cut, r3, 1);
                                rc = parse(cut, MRZ_ARC_NONE_LZ4, r3);
                                CHECK(rc == MRZ_E_CORRUPT, "cut behind chunk 0, second chunk: rc %d", rc);
                            }
                            n_archives++;
                        }
    CHECK(n_archives == 128, "%d", n_archives);
}

// ---- refusals ------------------------------------------------------------------------------------------------------
struct Refusal {
    std::string name;
    Bytes bytes;
    int lz4, none;  // expected under MRZ_ARC_NONE_LZ4 / MRZ_ARC_NONE_ONLY
};
const int OK = MRZ_OK, COR = MRZ_E_CORRUPT, UNS = MRZ_E_UNSUPPORTED;

// one chunk of `cb`: stream 0 = valid records in two blocks, stream 1 = two blocks; size and MD5 in place
Writer base(int cb) {
    Writer w;
    w.magic(9, 1);
    w.chunk(cb, 1);
    const Bytes r = records(9);
    w.block(0, 3, 4, 4, r.data());
    w.block(1, 3, 5, 5);
    w.block(0, 3, 6, 6, r.data() + 4);
    w.block(1, 3, 4, 4);
    w.md5();
    return w;
}
// the first real block of stream 0 becomes {ctype, c_len, u_len}; `plant`: what stops a walk that accepts it -- 'n': the
// next stream-0 block points at itself (MRZ_E_CORRUPT), 'u': the head of stream 1 is ctype 6 (MRZ_E_UNSUPPORTED).
// payload > 0: the block really has that many bytes (they follow the archive's last block).
Bytes lengths(int cb, int ctype, int64_t c_len, int64_t u_len, char plant = 0, int64_t payload = 0) {
    Writer w = base(cb);
    const ExpChunk &c = w.chunks[0];
    ExpBlock b = c.blocks[0][1];
    if (payload) {  // a block of its own at the end, in place of the small one
        w.out.resize(w.out.size() - 16);
        w.block(0, ctype, payload, payload);
        b = w.chunks[0].blocks[0].back();
        poke(w.out, c.blocks[0][0].hdr_at + 1 + 2 * cb, cb, b.hdr_at - c.initial_pos);  // head -> the new block
    }
    w.out[(size_t)b.hdr_at] = (uint8_t)ctype;
    poke(w.out, b.hdr_at + 1, cb, c_len);
    poke(w.out, b.hdr_at + 1 + cb, cb, u_len);
    if (plant == 'n') poke(w.out, b.hdr_at + 1 + 2 * cb, cb, b.hdr_at - c.initial_pos);
    if (plant == 'u') w.out[(size_t)c.blocks[1][0].hdr_at] = 6;
    return w.out;
}

std::vector<Refusal> refusals() {
    std::vector<Refusal> t;
    const Writer w2 = base(2), w8 = base(8);
    const ExpChunk &c2 = w2.chunks[0];
    auto cut = [](const Bytes &b, int64_t n) { return Bytes(b.begin(), b.begin() + n); };
    auto with = [](Bytes b, int64_t at, int v) {
        b[(size_t)at] = (uint8_t)v;
        return b;
    };
    auto next_is = [&](int64_t v) {  // the `next` of stream 0's second block
        Bytes b = w2.out;
        poke(b, c2.blocks[0][1].hdr_at + 5, 2, v);
        return b;
    };
    const int64_t i63 = INT64_MAX, room = (int64_t)w2.out.size() - c2.blocks[0][1].pay_at;  // behind that block's header
    // ---- the magic header (include/mrzgpu_host.h:120 for encryption)
    t.push_back({ "base archive, cb 2", w2.out, OK, OK });
    t.push_back({ "base archive, cb 8", w8.out, OK, OK });
    t.push_back({ "empty", cut(w2.out, 0), COR, COR });
    t.push_back({ "magic cut at 19", cut(w2.out, 19), COR, COR });
    t.push_back({ "magic only", cut(w2.out, 20), COR, COR });
    t.push_back({ "wrong magic", with(w2.out, 3, 'P'), COR, COR });
    t.push_back({ "encrypted", with(w2.out, 15, 1), UNS, UNS });
    t.push_back({ "hash code 2", with(w2.out, 14, 2), UNS, UNS });
    // ---- the chunk header
    t.push_back({ "cb 0", with(w2.out, c2.at, 0), COR, COR });
    t.push_back({ "cb 9", with(w2.out, c2.at, 9), COR, COR });
    for (int k = 1; k <= 3; k++) t.push_back({ "chunk header cut after byte " + std::to_string(k), cut(w2.out, c2.at + k), COR, COR });
    for (int k = 1; k <= 9; k++)
        t.push_back({ "chunk header cut after byte " + std::to_string(k) + ", cb 8", cut(w8.out, w8.chunks[0].at + k), COR, COR });
    // ---- block headers
    t.push_back({ "no block header", cut(w2.out, c2.initial_pos), COR, COR });
    t.push_back({ "head of stream 0 cut", cut(w2.out, c2.initial_pos + 6), COR, COR });
    t.push_back({ "head of stream 1 missing", cut(w2.out, c2.initial_pos + 7), COR, COR });
    t.push_back({ "head of stream 1 cut", cut(w2.out, c2.initial_pos + 13), COR, COR });
    t.push_back({ "second block header cut", cut(w2.out, c2.blocks[0][1].hdr_at + 6), COR, COR });
    t.push_back({ "payload cut", cut(w2.out, c2.blocks[0][1].pay_at + 3), COR, COR });
    // ---- lengths (include/mrzgpu_host.h:118-120)
    t.push_back({ "c_len one beyond the archive", lengths(2, 3, room + 1, room + 1), COR, COR });
    t.push_back({ "c_len up to the archive's end, stream 1 reached", lengths(2, 3, room, room, 'u'), UNS, UNS });
    t.push_back({ "c_len 2^63 - 1", lengths(8, 3, i63, i63), COR, COR });
    t.push_back({ "c_len -1", lengths(8, 3, -1, 4), COR, COR });
    t.push_back({ "u_len -1", lengths(8, 3, 4, -1), COR, COR });
    t.push_back({ "both -1", lengths(8, 3, -1, -1), COR, COR });
    t.push_back({ "NONE with c_len != u_len", lengths(2, 3, 4, 5), COR, COR });
    t.push_back({ "NONE accepted, stream 1 reached", lengths(2, 3, 4, 4, 'u'), UNS, UNS });
    t.push_back({ "ctype 6", lengths(2, 6, 4, 4), UNS, UNS });
    t.push_back({ "ctype 6 with negative lengths", lengths(8, 6, -1, -1), UNS, UNS });
    // ---- LZ4 blocks: the NONE-only policy refuses the ctype before it looks at a length (include/mrzgpu_host.h:124)
    t.push_back({ "LZ4, valid lengths", lengths(2, 5, 4, 9, 'n'), COR, UNS });
    t.push_back({ "LZ4, valid lengths, stream 1 reached", lengths(2, 5, 4, 9, 'u'), UNS, UNS });
    t.push_back({ "LZ4, negative lengths", lengths(8, 5, -1, -1), COR, UNS });
    t.push_back({ "LZ4, c_len 2^63 - 1", lengths(8, 5, i63, i63), COR, UNS });
    t.push_back({ "LZ4, c_len beyond the archive", lengths(2, 5, room + 1, 300), COR, UNS });
    // c_len > u_len + u_len/255 + 16 (include/mrzgpu_host.h:119)
    t.push_back({ "LZ4, c_len = u_len + u_len/255 + 16", lengths(2, 5, 20, 4, 'u'), UNS, UNS });
    t.push_back({ "LZ4, c_len = u_len + u_len/255 + 17", lengths(2, 5, 21, 4, 'u'), COR, UNS });
    t.push_back({ "LZ4, c_len = u_len + u_len/255 + 16, u_len 255", lengths(4, 5, 272, 255, 'u', 272), UNS, UNS });
    t.push_back({ "LZ4, c_len = u_len + u_len/255 + 17, u_len 255", lengths(4, 5, 273, 255, 'u', 273), COR, UNS });
    // u_len > 255 * c_len (include/mrzgpu_host.h:119)
    t.push_back({ "LZ4, u_len/255 = c_len", lengths(2, 5, 4, 4 * 255 + 254, 'u'), UNS, UNS });
    t.push_back({ "LZ4, u_len/255 = c_len + 1", lengths(2, 5, 4, 5 * 255, 'u'), COR, UNS });
    t.push_back({ "LZ4, c_len 0, u_len 254", lengths(2, 5, 0, 254, 'u'), UNS, UNS });
    t.push_back({ "LZ4, c_len 0, u_len 255", lengths(2, 5, 0, 255, 'u'), COR, UNS });
    // u_len > 0x7E000000 (include/mrzgpu_host.h:119); 0x7E000000 / 255 = 8290237
    t.push_back({ "LZ4, u_len 0x7E000000", lengths(4, 5, 8290237, 0x7E000000, 'n', 8290237), COR, UNS });
    t.push_back({ "LZ4, u_len 0x7E000001", lengths(4, 5, 8290237, 0x7E000001, 'n', 8290237), UNS, UNS });
    t.push_back({ "LZ4, u_len 0x7E000001, too long for its c_len", lengths(4, 5, 4, 0x7E000001), UNS, UNS });
    // ---- next: chains only run forward
    const int64_t b1 = c2.blocks[0][1].hdr_at - c2.initial_pos;
    t.push_back({ "next at itself", next_is(b1), COR, COR });
    t.push_back({ "next backwards, at the head", next_is(7), COR, COR });  // (0 would end the chain)
    t.push_back({ "next one byte forward", next_is(b1 + 1), UNS, UNS });   // lands in the header: ctype 4
    t.push_back({ "next beyond n", next_is((int64_t)w2.out.size() - c2.initial_pos + 1), COR, COR });
    t.push_back({ "next at n", next_is((int64_t)w2.out.size() - c2.initial_pos), COR, COR });
    t.push_back({ "next negative, cb 8", [&] {
                     Bytes b = w8.out;
                     poke(b, w8.chunks[0].blocks[0][1].hdr_at + 17, 8, -40);
                     return b;
                 }(), COR, COR });
    // ---- the records of stream 0
    Writer nt;
    nt.magic(9, 1);
    nt.chunk(2, 1);
    nt.block(0, 3, 3, 3, records(9, false).data());
    nt.block(1, 3, 9, 9);
    nt.md5();
    t.push_back({ "stream 0 without a terminator", nt.out, COR, COR });
    return t;
}

void test_refusals(const char *dump_dir) {
    const std::vector<Refusal> t = refusals();
    for (size_t k = 0; k < t.size(); k++) {
        g_case = t[k].name;
        if (dump_dir) {
            const std::string path = std::string(dump_dir) + "/" + std::to_string(k) + ".bin";
            FILE *f = fopen(path.c_str(), "wb");
            const size_t n = t[k].bytes.size();
            CHECK(f && (!n || fwrite(t[k].bytes.data(), 1, n, f) == n) && !fclose(f), "%s", path.c_str());
            printf("%zu\t%d\t%d\t%s\n", k, t[k].lz4, t[k].none, t[k].name.c_str());
        }
        const Exact a(t[k].bytes, (int64_t)t[k].bytes.size());
        Parsed r;
        int rc = parse(a, MRZ_ARC_NONE_LZ4, r);
        CHECK(rc == t[k].lz4, "NONE + LZ4: rc %d, expected %d", rc, t[k].lz4);
        rc = parse(a, MRZ_ARC_NONE_ONLY, r);
        CHECK(rc == t[k].none, "NONE only: rc %d, expected %d", rc, t[k].none);
    }
    // what the plants hide: the walk of stream 0 alone accepts the block at each limit
    const struct {
        int cb;
        int64_t c_len, u_len, payload;
    } limits[] = { { 2, 20, 4, 0 }, { 4, 272, 255, 272 }, { 2, 4, 4 * 255 + 254, 0 }, { 2, 0, 254, 0 }, { 4, 8290237, 0x7E000000, 8290237 } };
    for (const auto &l : limits) {
        g_case = "limit c_len " + std::to_string(l.c_len) + " u_len " + std::to_string(l.u_len);
        const Bytes b = lengths(l.cb, 5, l.c_len, l.u_len, 0, l.payload);
        const Exact a(b, (int64_t)b.size());
        const int64_t initial_pos = 20 + 2 + l.cb;
        std::vector<mrz_arc_block> blocks;
        int64_t total = 0, end_max = 0;
        const int rc = mrz_arc_walk_chain(a.p, a.n, initial_pos, initial_pos, l.cb, MRZ_ARC_NONE_LZ4, blocks, &total, &end_max);
        CHECK(rc == MRZ_OK && blocks.size() >= 2 && blocks[1].ctype == 5 && blocks[1].c_len == l.c_len && blocks[1].u_len == l.u_len,
              "rc %d, %zu blocks", rc, blocks.size());
        CHECK(total == l.u_len + (l.payload ? 0 : 6) && end_max <= a.n, "total %lld end %lld", (long long)total, (long long)end_max);
    }
}

// ---- sweeps: whatever the bytes, a code and no sanitizer report ------------------------------------------------------
void parse_both(const Bytes &b, int64_t n) {
    const Exact a(b, n);
    Parsed r;
    for (mrz_arc_policy p : { MRZ_ARC_NONE_LZ4, MRZ_ARC_NONE_ONLY }) {
        const int rc = parse(a, p, r);
        CHECK(rc == MRZ_OK || rc == MRZ_E_CORRUPT || rc == MRZ_E_UNSUPPORTED, "rc %d", rc);
    }
}

void test_sweeps() {
    const Writer ws[] = { valid_archive(2, 2, true, 1, false, false), valid_archive(8, 2, false, 1, true, false, 2) };
    for (const Writer &w : ws)
        for (int64_t n = 0; n < (int64_t)w.out.size(); n++) {
            g_case = "truncated to " + std::to_string(n);
            parse_both(w.out, n);
        }
    const Writer &w = ws[1];
    for (size_t at = 0; at < w.out.size(); at++) {
        if (!w.framing[at]) continue;
        for (int m = 0; m < 4; m++) {
            g_case = "byte " + std::to_string(at) + " mutation " + std::to_string(m);
            Bytes b = w.out;
            b[at] = m == 0 ? 0x00 : m == 1 ? 0xFF : m == 2 ? b[at] ^ 0x01 : b[at] ^ 0x80;
            parse_both(b, (int64_t)b.size());
        }
    }
}

// ---- records_out_len -------------------------------------------------------------------------------------------------
void test_records() {
    g_case = "records_out_len";
    for (int cb : { 1, 2, 4, 8 }) {
        Bytes s0 = { 0, 5, 0, 1, 0x34, 0x12 };  // a literal of 5, a match of 0x1234 ...
        s0.insert(s0.end(), (size_t)cb, 0x77);  // ... with its offset
        s0.insert(s0.end(), { 0, 0xff, 0xff });
        const size_t before_term = s0.size();
        s0.insert(s0.end(), { 0, 0, 0, 9, 9, 9, 9 });
        for (size_t n = 0; n <= s0.size(); n++) {
            const Exact a(s0, (int64_t)n);
            int64_t len = -1;
            const bool ok = mrz_arc_records_out_len(a.p, a.n, cb, &len);
            CHECK(ok == (n >= before_term + 3), "cb %d, %zu bytes: %d", cb, n, (int)ok);
            if (ok) CHECK(len == 5 + 0x1234 + 0xffff, "cb %d: %lld", cb, (long long)len);
        }
    }
}

// ---- the range arithmetic --------------------------------------------------------------------------------------------
void test_range() {
    const int64_t lens[3] = { 3, 5, 2 }, total = 10;
    mrz_arc_header h = { 0, 1, 20 };
    for (int with_size = 0; with_size < 2; with_size++) {
        h.expected = with_size ? total : 0;
        for (int64_t first = 0; first <= total; first++)
            for (int64_t count = 0; count <= total - first; count++) {
                g_case = "range first " + std::to_string(first) + " count " + std::to_string(count) + (with_size ? " with size" : "");
                mrz_arc_range rg;
                int64_t file_len = -1;
                int rc = rg.begin(h, first, count, &file_len);
                CHECK(rc == MRZ_OK && file_len == (with_size ? total : -1), "begin: rc %d file_len %lld", rc, (long long)file_len);
                int64_t out[10], want[10];
                for (int i = 0; i < 10; i++) out[i] = want[i] = -1;
                for (int64_t g = 0; g < total; g++)  // byte by byte: file byte g belongs at out[g - first]
                    if (g >= first && g < first + count) want[g - first] = g;
                int walked = 0;
                for (int k = 0; k < 3; k++) {
                    int64_t lo = -1, cnt = -1, out_at = -1;
                    if (rg.clip(lens[k], &lo, &cnt, &out_at)) {
                        CHECK(lo >= 0 && cnt > 0 && lo + cnt <= lens[k] && out_at >= 0 && out_at + cnt <= count, "chunk %d: lo %lld cnt %lld at %lld", k,
                              (long long)lo, (long long)cnt, (long long)out_at);
                        for (int64_t i = 0; i < cnt; i++) {
                            CHECK(out[out_at + i] == -1, "chunk %d writes byte %lld twice", k, (long long)(out_at + i));
                            out[out_at + i] = rg.total + lo + i;
                        }
                    }
                    rg.total += lens[k];
                    walked++;
                    if (rg.covered()) break;
                }
                CHECK(!memcmp(out, want, sizeof out), "the clipped pieces are not the range");
                // behind a size the walk ends with the first chunk that reaches first + count; without, at the end
                int64_t need = 0, upto = 0;
                while (need < 3 && (need == 0 || upto < first + count)) upto += lens[need++];
                CHECK(walked == (with_size ? need : 3), "walked %d chunks", walked);
                rc = rg.finish(&file_len);
                CHECK(rc == MRZ_OK && file_len == (with_size ? total : rg.total), "finish: rc %d file_len %lld", rc, (long long)file_len);
            }
    }
    // the argument verdicts (include/mrzgpu_host.h:128-129): MRZ_E_ARG with *file_len set, before the walk where the
    // header carries the size and after it where not; the parent commit's range calls give the same for each
    const int64_t bad[][2] = { { -1, 1 }, { 0, -1 }, { -1, -1 }, { 4, 7 }, { 11, 0 }, { 1, INT64_MAX }, { INT64_MAX, 1 }, { INT64_MAX, INT64_MAX } };
    for (const auto &fc : bad)
        for (int with_size = 0; with_size < 2; with_size++) {
            g_case = "bad range first " + std::to_string(fc[0]) + " count " + std::to_string(fc[1]) + (with_size ? " with size" : "");
            h.expected = with_size ? total : 0;
            mrz_arc_range rg;
            int64_t file_len = -1;
            int rc = rg.begin(h, fc[0], fc[1], &file_len);
            CHECK(rc == (with_size ? MRZ_E_ARG : MRZ_OK) && file_len == (with_size ? total : -1), "begin: rc %d file_len %lld", rc,
                  (long long)file_len);
            if (with_size) continue;
            for (int k = 0; k < 3; k++) {
                int64_t lo, cnt, out_at;
                const bool in = rg.clip(lens[k], &lo, &cnt, &out_at);
                CHECK(!in || (fc[0] == 4 && fc[1] == 7), "chunk %d is clipped", k);  // (4, 7) is wrong only once the length is known
                rg.total += lens[k];
                CHECK(!rg.covered(), "covered without a size");
            }
            rc = rg.finish(&file_len);
            CHECK(rc == MRZ_E_ARG && file_len == total, "finish: rc %d file_len %lld", rc, (long long)file_len);
        }
    // fewer bytes than the header promised (include/mrzgpu_host.h:128)
    g_case = "short archive";
    h.expected = 12;
    mrz_arc_range rg;
    CHECK(rg.begin(h, 8, 4, nullptr) == MRZ_OK, "begin");
    rg.total = total;
    CHECK(!rg.covered() && rg.finish(nullptr) == MRZ_E_CORRUPT, "finish");
}

int main(int argc, char **argv) {
    test_accepts();
    test_refusals(argc > 1 ? argv[1] : nullptr);
    test_sweeps();
    test_records();
    test_range();
    printf("archive_test ok\n");
    return 0;
}
