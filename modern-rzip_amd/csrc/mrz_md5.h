// mrz_md5.h -- MD5 (RFC 1321; libgcrypt GCRY_MD_MD5 in the reference): the whole-file hash of a -n archive, written by
// mrz_host.hip (through mrz_framing.h's sink) and checked by mrz_unarchive.hip.  Host code.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

struct Md5 {
    uint32_t h[4];
    uint64_t total;
    uint8_t pend[64];
    size_t npend;
    Md5() : total(0), npend(0) {
        h[0] = 0x67452301u;
        h[1] = 0xefcdab89u;
        h[2] = 0x98badcfeu;
        h[3] = 0x10325476u;
    }
    static uint32_t rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }
    void block(const uint8_t *p) {
        static const uint32_t K[64] = {
            0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
            0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
            0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
            0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
            0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
            0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
            0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
            0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391 };
        static const int S[4][4] = { { 7, 12, 17, 22 }, { 5, 9, 14, 20 }, { 4, 11, 16, 23 }, { 6, 10, 15, 21 } };
        uint32_t m[16];
        memcpy(m, p, 64);  // little-endian host
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
        for (int i = 0; i < 64; i++) {
            const int r = i >> 4;
            uint32_t f;
            int g;
            switch (r) {
                case 0: f = d ^ (b & (c ^ d)); g = i; break;
                case 1: f = c ^ (d & (b ^ c)); g = (5 * i + 1) & 15; break;
                case 2: f = b ^ c ^ d; g = (3 * i + 5) & 15; break;
                default: f = c ^ (b | ~d); g = (7 * i) & 15; break;
            }
            const uint32_t nb = b + rol(a + f + K[i] + m[g], S[r][i & 3]);
            a = d;
            d = c;
            c = b;
            b = nb;
        }
        h[0] += a;
        h[1] += b;
        h[2] += c;
        h[3] += d;
    }
    void update(const uint8_t *p, size_t n) {
        total += n;
        if (npend) {
            size_t take = 64 - npend;
            if (take > n) take = n;
            memcpy(pend + npend, p, take);
            npend += take;
            p += take;
            n -= take;
            if (npend < 64) return;
            block(pend);
            npend = 0;
        }
        for (; n >= 64; p += 64, n -= 64) block(p);
        if (n) {
            memcpy(pend, p, n);
            npend = n;
        }
    }
    void finish(uint8_t out[16]) {
        const uint64_t bits = total * 8;
        uint8_t tail[128];
        size_t k = npend;
        memcpy(tail, pend, k);
        tail[k++] = 0x80;
        while (k % 64 != 56) tail[k++] = 0;
        for (int i = 0; i < 8; i++) tail[k++] = (uint8_t)(bits >> (8 * i));
        for (size_t o = 0; o < k; o += 64) block(tail + o);
        memcpy(out, h, 16);
    }
};
