/* tests/c/capi_extract_test.c -- TEST: a plain C99 caller (gcc, no ctypes) of the entry points behind the member
 * extractor: mrz_copy_device_batch, mrz_runzip_ranges / mrz_runzip_origins_multi, mrz_runzip_buffer_ranges and
 * mrz_ar_extract / mrz_ar_extract_mrz, against include/mrzgpu.h and include/mrzgpu_host.h alone.
 *
 *   gcc -std=c99 -Iinclude tests/c/capi_extract_test.c -Lmodern-rzip_amd -lmrzgpu -o capi_extract_test
 *
 * Device memory comes from mrz_window_part_create; what lies there is read back through mrz_ar_extract (device archive,
 * host output) and mrz_crc32. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mrzgpu.h"
#include "mrzgpu_host.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "capi_extract_test: line %d: %s\n", __LINE__, #cond);    \
            return 1;                                                                \
        }                                                                            \
    } while (0)

#define N_MEMBERS 5

int main(void) {
    static uint8_t data[N_MEMBERS][6000];
    const int64_t sizes[N_MEMBERS] = { 6000, 1, 0, 501, 6000 };
    mrz_ar_member mem[N_MEMBERS];
    uint32_t x = 12345;
    int i;
    for (i = 0; i < N_MEMBERS; i++) {
        int64_t k;
        for (k = 0; k < sizes[i]; k++) {
            x = x * 1664525u + 1013904223u;
            data[i][k] = (uint8_t)("the quick brown fox "[(x >> 24) % 20] + (k % 7 == 0));
        }
        mem[i].name = "member";
        mem[i].name_len = 6;
        mem[i].reserved = 0;
        mem[i].mtime = (uint64_t)i;
        mem[i].data = data[i];
        mem[i].size = sizes[i];
    }
    memcpy(data[4], data[0], 6000); /* an exact duplicate */

    mrz_ctx *ctx = NULL;
    CHECK(mrz_abi_version() == 4 && mrz_open(&ctx, 0, 7, 1 << 20) == MRZ_OK);
    int64_t ar_len = 0;
    CHECK(mrz_ar_create(ctx, mem, N_MEMBERS, MRZ_MEM_HOST, NULL, MRZ_MEM_HOST, 0, &ar_len, NULL) == MRZ_OK);
    uint8_t *ar = (uint8_t *)malloc((size_t)ar_len);
    CHECK(ar && mrz_ar_create(ctx, mem, N_MEMBERS, MRZ_MEM_HOST, ar, MRZ_MEM_HOST, ar_len, &ar_len, NULL) == MRZ_OK);
    mrz_ar_entry ent[N_MEMBERS];
    int64_t count = 0, pay = 0;
    CHECK(mrz_ar_parse(ar, ar_len, ent, N_MEMBERS, &count, &pay) == MRZ_OK && count == N_MEMBERS);

    /* mrz_ar_extract, host to host: a selection in reversed order with one member twice */
    const int64_t which[4] = { 4, 3, 0, 3 };
    int64_t offs[5], offs2[5];
    mrz_ar_extract_info info;
    CHECK(mrz_ar_extract(ctx, ar, ar_len, MRZ_MEM_HOST, which, 4, NULL, MRZ_MEM_HOST, 0, offs, 0, &info) == MRZ_OK);
    CHECK(info.members == 4 && info.bytes_out == offs[4] && info.n_bad == 0 && info.first_bad == -1);
    const int64_t total = offs[4];
    uint8_t *want = (uint8_t *)malloc((size_t)total + 1), *got = (uint8_t *)malloc((size_t)total + 1);
    CHECK(want && got);
    for (i = 0; i < 4; i++) {
        CHECK(offs[i + 1] - offs[i] == ent[which[i]].size);
        memcpy(want + offs[i], ar + pay + ent[which[i]].offset, (size_t)ent[which[i]].size);
    }
    CHECK(mrz_ar_extract(ctx, ar, ar_len, MRZ_MEM_HOST, which, 4, got, MRZ_MEM_HOST, total, offs2, MRZ_AR_VERIFY, &info) ==
          MRZ_OK);
    CHECK(!memcmp(got, want, (size_t)total) && !memcmp(offs, offs2, sizeof(offs)) && info.n_bad == 0);
    CHECK(mrz_ar_extract(ctx, ar, ar_len, MRZ_MEM_HOST, which, 4, got, MRZ_MEM_HOST, total - 1, offs2, 0, NULL) == MRZ_E_ARG);

    /* the archive in device memory: mrz_ar_extract from there, and mrz_copy_device_batch inside that memory */
    const int64_t gran = mrz_window_granularity(0);
    CHECK(gran > 0);
    mrz_window_part *part = NULL;
    void *dptr = NULL;
    int fd = -1;
    CHECK(mrz_window_part_create(0, (2 * ar_len + 64 + total + gran - 1) / gran * gran, &part, &dptr, &fd) == MRZ_OK);
    uint8_t *dev = (uint8_t *)dptr;
    CHECK(mrz_copy_to_device(ctx, dev, ar, ar_len) == MRZ_OK);
    memset(got, 0, (size_t)total);
    CHECK(mrz_ar_extract(ctx, dev, ar_len, MRZ_MEM_DEVICE, which, 4, got, MRZ_MEM_HOST, total, offs2, MRZ_AR_VERIFY, &info) ==
          MRZ_OK);
    CHECK(!memcmp(got, want, (size_t)total) && info.n_bad == 0 && info.distinct_payloads <= 3);
    {
        uint8_t *packed = dev + ((ar_len + 63) & ~(int64_t)63); /* the selection's layout, made by one batched copy */
        const void *src[4];
        void *dst[4];
        int64_t lens[4];
        uint32_t crc_dev = 0, crc_host = 1;
        for (i = 0; i < 4; i++) {
            src[i] = dev + pay + ent[which[i]].offset;
            dst[i] = packed + offs[i];
            lens[i] = ent[which[i]].size;
        }
        CHECK(mrz_copy_device_batch(ctx, src, dst, lens, 4) == MRZ_OK);
        CHECK(mrz_crc32(ctx, packed, total, MRZ_MEM_DEVICE, &crc_dev) == MRZ_OK);
        CHECK(mrz_crc32(ctx, want, total, MRZ_MEM_HOST, &crc_host) == MRZ_OK && crc_dev == crc_host);
        lens[1] = -1;
        CHECK(mrz_copy_device_batch(ctx, src, dst, lens, 4) == MRZ_E_ARG);
        CHECK(mrz_copy_device_batch(ctx, NULL, NULL, NULL, 0) == MRZ_OK);
    }

    /* the two streams of the archive as one chunk: many ranges after one parse */
    {
        int64_t victim = 0;
        mrz_chunk_result res;
        const int cb = mrz_chunk_bytes(ar_len);
        CHECK(mrz_rzip_chunk(ctx, ar, ar_len, MRZ_MEM_HOST, cb, &victim, &res) == MRZ_OK);
        uint8_t *s0 = (uint8_t *)malloc((size_t)res.s0_len + 1), *s1 = (uint8_t *)malloc((size_t)res.s1_len + 1);
        CHECK(s0 && s1 && mrz_fetch_streams(ctx, s0, s1) == MRZ_OK);
        const mrz_byte_range ranges[3] = { { ar_len - 100, 100 }, { 0, 13 }, { pay + 10, 20 } };
        uint8_t bytes[133];
        int64_t origins[133];
        mrz_range_info ri;
        CHECK(mrz_runzip_ranges(ctx, s0, res.s0_len, s1, res.s1_len, MRZ_MEM_HOST, cb, ranges, 3, bytes, MRZ_MEM_HOST, &ri) ==
              MRZ_OK);
        CHECK(ri.chunk_len == ar_len && !memcmp(bytes, ar + ar_len - 100, 100) && !memcmp(bytes + 100, ar, 13) &&
              !memcmp(bytes + 113, ar + ranges[2].first, 20));
        CHECK(mrz_runzip_origins_multi(ctx, s0, res.s0_len, res.s1_len, MRZ_MEM_HOST, cb, ranges, 3, origins, MRZ_MEM_HOST,
                                       &ri) == MRZ_OK);
        for (i = 0; i < 133; i++) CHECK(origins[i] >= 0 && origins[i] < res.s1_len && s1[origins[i]] == bytes[i]);
        const mrz_byte_range beyond[2] = { { 0, 1 }, { ar_len, 1 } };
        CHECK(mrz_runzip_ranges(ctx, s0, res.s0_len, s1, res.s1_len, MRZ_MEM_HOST, cb, beyond, 2, bytes, MRZ_MEM_HOST, &ri) ==
              MRZ_E_ARG && ri.chunk_len == ar_len);
        free(s0);
        free(s1);
    }

    /* the archive as a .mrz: ranges of it, and members straight out of it */
    {
        mrz_control ctl;
        memset(&ctl, 0, sizeof(ctl));
        ctl.rzip_compression_level = ctl.compression_level = 7;
        ctl.ramsize = (int64_t)60 << 30;
        ctl.page_size = 4096;
        ctl.hash_code = 1;
        void *mrz = NULL;
        int64_t mrz_len = 0, file_len = 0;
        CHECK(mrz_rzip_buffer(&ctl, ar, ar_len, &mrz, &mrz_len, NULL, NULL) == MRZ_OK);
        const mrz_byte_range ranges[2] = { { pay + ent[3].offset, ent[3].size }, { 0, 13 } };
        uint8_t *bytes = (uint8_t *)malloc((size_t)ent[3].size + 13);
        mrz_archive_range_info ainfo;
        CHECK(bytes && mrz_runzip_buffer_ranges(0, mrz, mrz_len, ranges, 2, bytes, MRZ_MEM_HOST, &file_len, &ainfo) == MRZ_OK);
        CHECK(file_len == ar_len && ainfo.chunks_in_range == 1 &&
              !memcmp(bytes, ar + ranges[0].first, (size_t)ent[3].size) && !memcmp(bytes + ent[3].size, "ARZIP", 5));
        memset(got, 0, (size_t)total);
        CHECK(mrz_ar_extract_mrz(0, mrz, mrz_len, which, 4, got, MRZ_MEM_HOST, total, offs2, MRZ_AR_VERIFY, &info, &ainfo) ==
              MRZ_OK);
        CHECK(!memcmp(got, want, (size_t)total) && !memcmp(offs, offs2, sizeof(offs)) && info.n_bad == 0 &&
              info.distinct_payloads <= 3 && ainfo.chunks_in_range == 3);
        free(bytes);
        mrz_free(mrz);
    }
    mrz_window_part_destroy(part);
    mrz_close(ctx);
    free(ar);
    free(want);
    free(got);
    printf("capi_extract_test ok\n");
    return 0;
}
