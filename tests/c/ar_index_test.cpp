// ar_index_test.cpp -- the host-only halves of the ar-mrzip index without a device: the ARZIP collapse, size
// arithmetic, metadata writer and parser (mrz_ar_index.h) and the host half of the TLSH digest (mrz_tlsh_tables.h).
// A plain program (its own main, no HIP); tests/test_ar_index_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "mrz_ar_index.h"
#include "mrz_tlsh_tables.h"

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            failures++;                                             \
        }                                                           \
    } while (0)

struct Member {
    std::string name;
    uint64_t mtime;
    std::string data;
    uint8_t sum_byte;  // stands in for the checksum: equal data, equal byte
};

static std::vector<mrz_ar_rec> records(const std::vector<Member> &ms) {
    std::vector<mrz_ar_rec> recs(ms.size());
    for (size_t i = 0; i < ms.size(); i++) {
        mrz_ar_rec &r = recs[i];
        r.mtime = ms[i].mtime;
        r.size = (int64_t)ms[i].data.size();
        r.offset = -1;
        memset(r.sum, 0x77, MRZ_AR_SUM);
        r.sum[MRZ_AR_SUM - 1] = ms[i].sum_byte;  // (all 64 bytes take part in the comparison)
        memset(r.digest, 'A' + (int)(i % 26), MRZ_AR_DIGEST);
        r.name = (const uint8_t *)ms[i].name.data();
        r.name_len = (uint32_t)ms[i].name.size();
        r.index = (int64_t)i;
        r.record_at = 0;
    }
    return recs;
}

static std::vector<uint8_t> archive(const std::vector<Member> &ms, std::vector<mrz_ar_rec> &recs) {
    std::vector<uint8_t> out((size_t)(MRZ_AR_HEAD + mrz_ar_metadata_size(recs)));
    CHECK(mrz_ar_write_metadata(recs, out.data()) == (int64_t)out.size());
    for (size_t k : mrz_ar_payload_plan(recs)) out.insert(out.end(), ms[k].data.begin(), ms[k].data.end());
    return out;
}

static void test_length_code() {
    CHECK(mrz_tlsh_lcode(0) == 0 && mrz_tlsh_lcode(1) == 0 && mrz_tlsh_lcode(2) == 1 && mrz_tlsh_lcode(3) == 2);
    CHECK(mrz_tlsh_lcode(4) == 3 && mrz_tlsh_lcode(5) == 3 && mrz_tlsh_lcode(6) == 4);
    for (int i = 1; i < 170; i++) {
        CHECK(k_tlsh_len_steps[i] > k_tlsh_len_steps[i - 1]);
        CHECK(mrz_tlsh_lcode(k_tlsh_len_steps[i]) == i);
        CHECK(mrz_tlsh_lcode((int64_t)k_tlsh_len_steps[i - 1] + 1) == i);
    }
    CHECK(mrz_tlsh_lcode(MRZ_TLSH_MAX_LEN) == 169);
}

static void test_hex() {
    static const uint8_t perm[256] = { MRZ_TLSH_PEARSON_ROWS };
    int seen[256] = { 0 };
    for (int i = 0; i < 256; i++) seen[perm[i]]++;
    for (int i = 0; i < 256; i++) CHECK(seen[i] == 1);
    CHECK(perm[2] == MRZ_TLSH_SALT_A && perm[3] == MRZ_TLSH_SALT_B && perm[5] == MRZ_TLSH_SALT_C);
    CHECK(perm[7] == MRZ_TLSH_SALT_D && perm[11] == MRZ_TLSH_SALT_E && perm[13] == MRZ_TLSH_SALT_F);
    mrz_tlsh_fin f;
    memset(&f, 0, sizeof(f));
    f.q1 = 3;
    f.q2 = 7;
    f.q3 = 11;  // 300 / 11 = 27 -> 11, 700 / 11 = 63 -> 15
    f.nonzero = 129;
    for (int i = 0; i < MRZ_TLSH_CODE; i++) f.code[i] = (uint8_t)i;
    const uint8_t chain[3] = { 0x12, 0xAB, 0x0F };
    char hex[MRZ_TLSH_HEX + 1];
    mrz_tlsh_hex(f, chain, 600, hex);  // length code of 600 is 15 = 0x0F -> F0
    CHECK(strlen(hex) == MRZ_TLSH_HEX);
    CHECK(!strncmp(hex, "21BAF0F0BF", 10));
    CHECK(!strncmp(hex + 10, "3F3E3D", 6) && !strcmp(hex + MRZ_TLSH_HEX - 4, "0100"));
    CHECK(mrz_tlsh_valid(f, 600) && !mrz_tlsh_valid(f, 49));
    f.nonzero = 128;
    CHECK(!mrz_tlsh_valid(f, 600));
    f.nonzero = 200;
    f.q3 = 0;
    CHECK(!mrz_tlsh_valid(f, 600));
    // the product wraps in 32 bits before the division, as in the reference
    f.q1 = 42949673u;  // * 100 = 2^32 + 4 -> 4
    f.q2 = f.q3 = 50000000u;  // * 100 = 2^32 + 705032704; / 50000000 = 14.1
    mrz_tlsh_hex(f, chain, 600, hex);
    CHECK(hex[8] == '0' && hex[9] == 'E');  // q1 ratio 0, q2 ratio 14 (not 100 % 16 = 4)
}

static void test_archive() {
    const std::vector<Member> ms = {
        { "a", 1, "hello", 1 },          { "empty", 2, "", 2 },       { "a-again", 3, "hello", 1 },
        { "", 4, "world!", 3 },          { "empty-again", 5, "", 2 }, { std::string(300, 'n'), ~0ull, "xyz", 4 },
        { "far-duplicate", 7, "xyz", 4 },
    };
    std::vector<mrz_ar_rec> recs = records(ms);
    int64_t unique = 0, dup = 0;
    mrz_ar_collapse(recs, &unique, &dup);
    CHECK(unique == 5 + 6 + 3 && dup == 5 + 3);
    const int64_t want_off[] = { 0, 5, 0, 5, 5, 11, 11 };
    for (size_t i = 0; i < recs.size(); i++) CHECK(recs[i].offset == want_off[i]);
    int64_t names = 0;
    for (const auto &m : ms) names += (int64_t)m.name.size();
    CHECK(mrz_ar_metadata_size(recs) == names + (int64_t)ms.size() * (88 + 4 + 137));
    // the empty member at the running offset is in the plan (it writes nothing); its duplicate behind "world!" is not
    const std::vector<size_t> plan = mrz_ar_payload_plan(recs);
    CHECK((plan == std::vector<size_t>{ 0, 1, 3, 5 }));
    std::vector<uint8_t> ar = archive(ms, recs);
    CHECK((int64_t)ar.size() == MRZ_AR_HEAD + mrz_ar_metadata_size(recs) + unique);
    CHECK(!memcmp(ar.data(), "ARZIP", 5) && ar[5] == 0 && ar[13] == 0 && ar[13 + 7] == 1);  // big-endian numbers

    std::vector<mrz_ar_rec> back;
    int64_t pay = 0;
    CHECK(mrz_ar_read(ar.data(), (int64_t)ar.size(), (int64_t)ar.size(), back, &pay) == MRZ_OK);
    CHECK(back.size() == ms.size() && pay == MRZ_AR_HEAD + mrz_ar_metadata_size(recs));
    for (size_t i = 0; i < back.size() && i < ms.size(); i++) {
        CHECK(back[i].mtime == ms[i].mtime && back[i].size == (int64_t)ms[i].data.size());
        CHECK(back[i].offset == want_off[i] && back[i].name_len == ms[i].name.size());
        CHECK(!memcmp(back[i].name, ms[i].name.data(), ms[i].name.size()));
        CHECK(!memcmp(back[i].sum, recs[i].sum, MRZ_AR_SUM) && !memcmp(back[i].digest, recs[i].digest, MRZ_AR_DIGEST));
        CHECK(!memcmp(ar.data() + pay + back[i].offset, ms[i].data.data(), ms[i].data.size()));
    }
    // the metadata alone is enough for a parse (the verifier reads a device archive that way)
    CHECK(mrz_ar_read(ar.data(), pay, (int64_t)ar.size(), back, &pay) == MRZ_OK && back.size() == ms.size());
    CHECK(mrz_ar_read(ar.data(), pay - 1, (int64_t)ar.size(), back, &pay) == MRZ_E_CORRUPT);

    // every truncation: refused while metadata is missing, and while a member's bytes are
    for (int64_t n = 0; n < (int64_t)ar.size(); n++) {
        std::vector<uint8_t> cut(ar.begin(), ar.begin() + n);  // (its own allocation: a read beyond it is caught)
        CHECK(mrz_ar_read(cut.data(), n, n, back, &pay) == MRZ_E_CORRUPT);
    }
    // every single-byte mutation of the header and the numbers of a record: accepted or refused, never a wild read
    for (int64_t at = 0; at < pay; at++)
        for (int bit = 0; bit < 8; bit += 7) {
            std::vector<uint8_t> mut(ar);
            mut[(size_t)at] ^= (uint8_t)(1u << bit);
            const int rc = mrz_ar_read(mut.data(), (int64_t)mut.size(), (int64_t)mut.size(), back, &pay);
            CHECK(rc == MRZ_OK || rc == MRZ_E_CORRUPT);
            if (at < 13) CHECK(rc == MRZ_E_CORRUPT);  // magic, or a metadata_size the records do not consume exactly
            if (rc == MRZ_OK)
                for (const auto &r : back) CHECK(r.offset >= 0 && r.size >= 0 && r.offset + r.size <= (int64_t)mut.size() - pay);
        }
    // offset + size at the end of the payload is the limit
    std::vector<uint8_t> edge(ar);
    mrz_ar_put_be(edge.data() + 13 + 16, (uint64_t)(unique - 5), 8);
    CHECK(mrz_ar_read(edge.data(), (int64_t)edge.size(), (int64_t)edge.size(), back, &pay) == MRZ_OK);
    mrz_ar_put_be(edge.data() + 13 + 16, (uint64_t)(unique - 4), 8);
    CHECK(mrz_ar_read(edge.data(), (int64_t)edge.size(), (int64_t)edge.size(), back, &pay) == MRZ_E_CORRUPT);
    mrz_ar_put_be(edge.data() + 13 + 16, ~0ull - 2, 8);  // offset + size wraps
    CHECK(mrz_ar_read(edge.data(), (int64_t)edge.size(), (int64_t)edge.size(), back, &pay) == MRZ_E_CORRUPT);

    // no members at all
    std::vector<mrz_ar_rec> none;
    uint8_t head[MRZ_AR_HEAD];
    CHECK(mrz_ar_write_metadata(none, head) == MRZ_AR_HEAD);
    CHECK(mrz_ar_read(head, MRZ_AR_HEAD, MRZ_AR_HEAD, back, &pay) == MRZ_OK && back.empty() && pay == MRZ_AR_HEAD);
}

int main() {
    test_length_code();
    test_hex();
    test_archive();
    if (failures) {
        printf("ar_index_test: %d failures\n", failures);
        return 1;
    }
    printf("ar_index_test ok\n");
    return 0;
}
