// tests/c/ar_head_test.cpp -- TEST: mrz_ar_read_prefix (mrz_ar_index.h), the ARZIP parser for a caller that holds the
// head of an archive and knows its total length, but not the payload (mrz_ar_extract_mrz).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imodern-rzip_amd/csrc tests/c/ar_head_test.cpp -o ar_head_test
//
// No HIP, no library.  Every parse runs on a heap copy of exactly head_len bytes, so the address sanitizer sees a read
// at or behind head_len.  The records and verdicts must be those of mrz_ar_read on the whole archive.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "mrz_ar_index.h"

#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "ar_head_test: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                            \
            fprintf(stderr, "\n");                                                   \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

typedef std::vector<uint8_t> Bytes;

// the parse of a heap copy of ar[0, head_len) under a claimed total length
static int parse_head(const Bytes &ar, int64_t head_len, int64_t total, std::vector<mrz_ar_rec> &recs, int64_t *pay) {
    uint8_t *copy = (uint8_t *)malloc((size_t)(head_len > 0 ? head_len : 1));
    if (head_len > 0) memcpy(copy, ar.data(), (size_t)head_len);
    std::vector<mrz_ar_rec> got;
    const int rc = mrz_ar_read_prefix(copy, head_len, total, got, pay);
    recs = got;
    for (mrz_ar_rec &r : recs) r.name = ar.data() + (r.name - copy);  // the copy goes away
    free(copy);
    return rc;
}

static bool same(const mrz_ar_rec &a, const mrz_ar_rec &b) {
    return a.mtime == b.mtime && a.size == b.size && a.offset == b.offset && !memcmp(a.sum, b.sum, MRZ_AR_SUM) &&
           !memcmp(a.digest, b.digest, MRZ_AR_DIGEST) && a.name_len == b.name_len && a.index == b.index &&
           a.record_at == b.record_at && !memcmp(a.name, b.name, a.name_len);
}

int main() {
    // an archive of five members: an empty one, a duplicate, names of 0 and 300 bytes
    const std::string long_name(300, 'n');
    const char *names[] = { "a", "", long_name.c_str(), "dup-of-a", "empty" };
    const int64_t sizes[] = { 700, 1, 5000, 700, 0 };
    std::vector<mrz_ar_rec> recs(5);
    for (int i = 0; i < 5; i++) {
        mrz_ar_rec &r = recs[i];
        r.mtime = 1700000000u + i;
        r.size = sizes[i];
        r.offset = 0;
        memset(r.sum, i == 3 ? 0x10 : 0x10 + i, MRZ_AR_SUM);  // member 3 shares member 0's checksum
        memset(r.digest, 'A' + i, MRZ_AR_DIGEST);
        r.name = (const uint8_t *)names[i];
        r.name_len = (uint32_t)strlen(names[i]);
        r.index = i;
        r.record_at = 0;
    }
    int64_t unique = 0, dup = 0;
    mrz_ar_collapse(recs, &unique, &dup);
    CHECK(unique == 5701 && dup == 700, "collapse: %lld unique, %lld duplicate", (long long)unique, (long long)dup);
    const int64_t meta = mrz_ar_metadata_size(recs), head_len = MRZ_AR_HEAD + meta, total = head_len + unique;
    Bytes ar((size_t)total, 0x5a);
    CHECK(mrz_ar_write_metadata(recs, ar.data()) == head_len, "writer");

    // the head alone gives what the whole archive gives
    std::vector<mrz_ar_rec> whole, head;
    int64_t pay_w = 0, pay_h = 0;
    CHECK(mrz_ar_read(ar.data(), total, total, whole, &pay_w) == MRZ_OK && whole.size() == 5, "whole archive");
    CHECK(parse_head(ar, head_len, total, head, &pay_h) == MRZ_OK, "the head alone");
    CHECK(pay_h == pay_w && pay_h == head_len && head.size() == whole.size(), "payload at %lld", (long long)pay_h);
    for (size_t i = 0; i < head.size(); i++) CHECK(same(head[i], whole[i]), "record %zu", i);
    CHECK(head[3].offset == head[0].offset && head[4].size == 0, "the duplicate shares its offset");
    // a caller that holds more than the head (the whole archive) gets the same
    CHECK(parse_head(ar, total, total, head, &pay_h) == MRZ_OK && head.size() == 5, "more than the head");

    // every shorter head is a truncated archive; so is a total length that cannot hold the head
    for (int64_t h = 0; h < head_len; h++) {
        int64_t pay = 0;
        CHECK(parse_head(ar, h, total, head, &pay) == MRZ_E_CORRUPT, "head of %lld bytes", (long long)h);
    }
    int64_t pay = 0;
    CHECK(parse_head(ar, head_len, head_len - 1, head, &pay) == MRZ_E_CORRUPT, "total below the head");
    CHECK(mrz_ar_read_prefix(nullptr, 0, 0, head, &pay) == MRZ_E_CORRUPT, "no head at all");
    CHECK(mrz_ar_read_prefix(ar.data(), -1, total, head, &pay) == MRZ_E_CORRUPT, "negative length");

    // the payload's extent comes from the total length: one byte less, and the last payload leaves it
    CHECK(parse_head(ar, head_len, total - 1, head, &pay) == MRZ_E_CORRUPT, "offset + size beyond the payload");
    CHECK(parse_head(ar, head_len, total + 100, head, &pay) == MRZ_OK, "a longer payload is fine");
    // with no payload at all only the empty members fit
    CHECK(parse_head(ar, head_len, head_len, head, &pay) == MRZ_E_CORRUPT, "no payload");

    // a bit flipped in every byte of the head: the verdict is that of the whole-archive parser, nothing is read beyond
    for (int64_t at = 0; at < head_len; at++) {
        Bytes bad = ar;
        bad[(size_t)at] ^= 0x40;
        std::vector<mrz_ar_rec> a, b;
        int64_t pa = 0, pb = 0;
        const int want = mrz_ar_read(bad.data(), total, total, a, &pa);
        CHECK(parse_head(bad, head_len, total, b, &pb) == want, "flip at %lld", (long long)at);
        if (want == MRZ_OK) {
            CHECK(a.size() == b.size() && pa == pb, "flip at %lld: records", (long long)at);
            for (size_t i = 0; i < a.size(); i++) CHECK(same(a[i], b[i]), "flip at %lld: record %zu", (long long)at, i);
        }
    }
    // the empty archive
    Bytes empty(MRZ_AR_HEAD, 0);
    memcpy(empty.data(), "ARZIP", 5);
    CHECK(parse_head(empty, MRZ_AR_HEAD, MRZ_AR_HEAD, head, &pay) == MRZ_OK && head.empty() && pay == MRZ_AR_HEAD, "empty");
    printf("ar_head_test ok\n");
    return 0;
}
