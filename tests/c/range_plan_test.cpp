// tests/c/range_plan_test.cpp -- TEST: mrz_arc_ranges (mrz_archive.h), the clipping of a list of ranges against the
// chunks of an archive and the placement of the clipped parts in the packed output, on its own.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imodern-rzip_amd/csrc tests/c/range_plan_test.cpp -o range_plan_test
//
// No HIP, no library.  A model file of chunk lengths is walked the way mrz_runzip_buffer_ranges walks an archive; what
// the parts must be is computed byte by byte: output byte j of the packed list is file byte first_k + (j - base_k), and
// every such pair must be delivered exactly once, by the chunk that holds the file byte.  A list of one range must
// give what mrz_arc_range gives.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mrz_archive.h"

#define CHECK(cond, ...)                                                                \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "range_plan_test: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                               \
            fprintf(stderr, "\n");                                                      \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

typedef std::vector<mrz_byte_range> List;

static mrz_arc_header header(int64_t expected) { return mrz_arc_header{ expected, 1, 24 }; }

// walks `chunks` under the list; returns finish()'s code; src[j] = file byte that lands at output byte j (-1: none)
static int walk(const std::vector<int64_t> &chunks, bool size_known, const List &list, std::vector<int64_t> &src,
                std::vector<int> &touched, int64_t *file_len, int *chunks_seen) {
    int64_t file = 0;
    for (int64_t c : chunks) file += c;
    mrz_arc_ranges rg;
    *file_len = -1;
    const int rc = rg.begin(header(size_known ? file : 0), list.data(), (int64_t)list.size(), file_len);
    touched.clear();
    *chunks_seen = 0;
    if (rc || (rg.size_known && !rg.sum)) return rc;
    src.assign((size_t)(rg.bad ? 0 : rg.sum), -1);
    std::vector<mrz_arc_part> parts;
    size_t k = 0;
    bool eof;
    do {
        const int64_t len = chunks[k];
        eof = k + 1 == chunks.size();
        ++*chunks_seen;
        if (rg.clip(len, parts)) {
            touched.push_back((int)k);
            for (const mrz_arc_part &p : parts) {
                CHECK(p.cnt > 0 && p.lo >= 0 && p.lo + p.cnt <= len, "part [%lld, +%lld) of a chunk of %lld",
                      (long long)p.lo, (long long)p.cnt, (long long)len);
                CHECK(p.out_at >= 0 && p.out_at + p.cnt <= rg.sum, "part placed at %lld", (long long)p.out_at);
                for (int64_t i = 0; i < p.cnt; i++) {
                    CHECK(src[(size_t)(p.out_at + i)] == -1, "output byte %lld delivered twice", (long long)(p.out_at + i));
                    src[(size_t)(p.out_at + i)] = rg.total + p.lo + i;
                }
            }
            // contiguous(): exactly when the flat order is the output order
            bool cont = true;
            for (size_t q = 1; q < parts.size(); q++) cont = cont && parts[q].out_at == parts[q - 1].out_at + parts[q - 1].cnt;
            CHECK(mrz_arc_ranges::contiguous(parts) == cont, "contiguous()");
        } else
            CHECK(parts.empty(), "parts left behind by a chunk outside every range");
        rg.total += len;
        k++;
    } while (!rg.covered() && !eof);
    return rg.finish(file_len);
}

static void expect_ok(const std::vector<int64_t> &chunks, bool size_known, const List &list, const std::vector<int> &want_touched,
                      int want_seen) {
    std::vector<int64_t> src;
    std::vector<int> touched;
    int64_t file_len;
    int seen;
    const int rc = walk(chunks, size_known, list, src, touched, &file_len, &seen);
    CHECK(rc == MRZ_OK, "rc %d", rc);
    int64_t file = 0;
    for (int64_t c : chunks) file += c;
    CHECK(file_len == file, "file_len %lld", (long long)file_len);
    size_t j = 0;
    int64_t sum = 0;
    for (const mrz_byte_range &r : list) sum += r.count;
    if (size_known && !sum) {
        CHECK(seen == 0, "an empty list walked %d chunks", seen);
        return;
    }
    for (const mrz_byte_range &r : list)
        for (int64_t i = 0; i < r.count; i++, j++)
            CHECK(src[j] == r.first + i, "output byte %zu comes from %lld, not %lld", j, (long long)src[j],
                  (long long)(r.first + i));
    CHECK(j == src.size(), "output of %zu bytes, %zu expected", src.size(), j);
    CHECK(touched == want_touched, "touched chunks");
    CHECK(seen == want_seen, "%d chunks walked, %d expected", seen, want_seen);
}

static int code_of(const std::vector<int64_t> &chunks, bool size_known, const List &list, int64_t *file_len, int *seen) {
    std::vector<int64_t> src;
    std::vector<int> touched;
    const int rc = walk(chunks, size_known, list, src, touched, file_len, seen);
    if (rc) CHECK(touched.empty() || !size_known, "work was done for a refused list");
    return rc;
}

int main() {
    const std::vector<int64_t> chunks = { 100, 50, 0, 200, 70 };  // seams at 100, 150, 150, 350; 420 bytes
    for (int known = 0; known < 2; known++) {
        const int all = 5;
        expect_ok(chunks, known, { { 10, 20 } }, { 0 }, known ? 1 : all);
        expect_ok(chunks, known, { { 90, 20 } }, { 0, 1 }, known ? 2 : all);
        expect_ok(chunks, known, { { 0, 420 } }, { 0, 1, 3, 4 }, all);
        expect_ok(chunks, known, { { 360, 5 }, { 419, 1 } }, { 4 }, all);                        // only the last chunk
        expect_ok(chunks, known, { { 400, 20 }, { 0, 0 }, { 5, 70 } }, { 0, 4 }, all);           // the middle untouched
        expect_ok(chunks, known, { { 80, 40 }, { 90, 30 } }, { 0, 1 }, known ? 2 : all);         // interleaved over a seam
        expect_ok(chunks, known, { { 300, 10 }, { 120, 10 }, { 10, 10 } }, { 0, 1, 3 }, known ? 4 : all);  // descending
        expect_ok(chunks, known, { { 149, 2 }, { 149, 2 }, { 140, 100 } }, { 1, 3 }, known ? 4 : all);     // identical, overlapping
        expect_ok(chunks, known, { { 420, 0 }, { 0, 0 } }, {}, known ? 0 : all);
        expect_ok(chunks, known, {}, {}, known ? 0 : all);
        expect_ok(chunks, known, { { 100, 50 } }, { 1 }, known ? 2 : all);                       // exactly one chunk
        // a bad range at each position: MRZ_E_ARG, with the length; against a size before anything is walked
        const List good = { { 0, 4 }, { 200, 4 }, { 7, 0 } };
        const mrz_byte_range bad[] = { { 420, 1 }, { 0, 421 }, { -1, 2 }, { 3, -1 }, { INT64_MAX, 1 }, { 1, INT64_MAX } };
        for (const mrz_byte_range &b : bad)
            for (size_t p = 0; p < good.size(); p++) {
                List l = good;
                l[p] = b;
                int64_t file_len;
                int seen;
                CHECK(code_of(chunks, known, l, &file_len, &seen) == MRZ_E_ARG, "bad range {%lld, %lld} at %zu",
                      (long long)b.first, (long long)b.count, p);
                CHECK(file_len == 420 && seen == (known ? 0 : all), "file_len %lld after %d chunks", (long long)file_len, seen);
            }
    }
    {  // fewer bytes than the header promised: the walk ends at eof, the verdict is MRZ_E_CORRUPT
        mrz_arc_ranges rg;
        int64_t file_len = -1;
        const List l = { { 10, 5 }, { 400, 20 } };
        CHECK(rg.begin(header(420), l.data(), 2, &file_len) == MRZ_OK && file_len == 420, "begin");
        rg.total = 300;
        CHECK(!rg.covered() && rg.finish(&file_len) == MRZ_E_CORRUPT, "a short file");
    }
    {  // one range: the parts and verdicts of mrz_arc_range
        const int64_t firsts[] = { 0, 99, 100, 149, 150, 151, 349, 419 }, counts[] = { 1, 2, 51, 300 };
        for (int64_t first : firsts)
            for (int64_t count : counts) {
                if (first + count > 420) continue;
                const mrz_byte_range r{ first, count };
                mrz_arc_ranges many;
                mrz_arc_range one;
                int64_t fl;
                CHECK(many.begin(header(420), &r, 1, &fl) == one.begin(header(420), first, count, &fl), "begin");
                std::vector<mrz_arc_part> parts;
                for (int64_t len : chunks) {
                    int64_t lo, cnt, out_at;
                    // (an empty chunk inside the range: mrz_arc_range hands out an empty part, the list none)
                    const bool in = one.clip(len, &lo, &cnt, &out_at) && cnt > 0;
                    CHECK(many.clip(len, parts) == in, "clip");
                    if (in)
                        CHECK(parts.size() == 1 && parts[0].lo == lo && parts[0].cnt == cnt && parts[0].out_at == out_at, "part");
                    one.total += len;
                    many.total += len;
                    CHECK(one.covered() == many.covered(), "covered");
                }
                CHECK(one.finish(&fl) == many.finish(&fl), "finish");
            }
    }
    printf("range_plan_test ok\n");
    return 0;
}
