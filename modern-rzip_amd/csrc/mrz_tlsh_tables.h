// mrz_tlsh_tables.h -- the published constants of the TLSH digest (256 buckets, 3 checksum bytes, 5-byte window: the
// configuration ar-mrzip is built with) and the host half of the digest: length code, quartile ratios, validity and the
// hex string.  Host code without a HIP call or include, so that tests/c/ar_index_test.cpp drives it on its own; the
// kernels (mrz_tlsh.hip) take the permutation through MRZ_TLSH_PEARSON_ROWS.
#pragma once
#include <stdint.h>
#include <string.h>

#define MRZ_TLSH_BUCKETS 256
#define MRZ_TLSH_CODE 64          // code bytes: four buckets of two bits each
#define MRZ_TLSH_BIN 69           // 3 checksum bytes, length code, ratio byte, code
#define MRZ_TLSH_HEX 138          // the digest as upper-case hex
#define MRZ_TLSH_STORED 137       // what ar-mrzip keeps of it
#define MRZ_TLSH_MIN_LEN 50       // shorter messages have no digest
#define MRZ_TLSH_MAX_LEN 4224281216ll  // the last length threshold; beyond it the reference's length code is undefined

// Pearson's permutation of 0..255, 32 entries per row
#define MRZ_TLSH_PEARSON_ROWS                                                                                          \
    1, 87, 49, 12, 176, 178, 102, 166, 121, 193, 6, 84, 249, 230, 44, 163, 14, 197, 213, 181, 161, 85, 218, 80, 64,    \
    239, 24, 226, 236, 142, 38, 200,                                                                                   \
    110, 177, 104, 103, 141, 253, 255, 50, 77, 101, 81, 18, 45, 96, 31, 222, 25, 107, 190, 70, 86, 237, 240, 34, 72,   \
    242, 20, 214, 244, 227, 149, 235,                                                                                  \
    97, 234, 57, 22, 60, 250, 82, 175, 208, 5, 127, 199, 111, 62, 135, 248, 174, 169, 211, 58, 66, 154, 106, 195, 245, \
    171, 17, 187, 182, 179, 0, 243,                                                                                    \
    132, 56, 148, 75, 128, 133, 158, 100, 130, 126, 91, 13, 153, 246, 216, 219, 119, 68, 223, 78, 83, 88, 201, 99,     \
    122, 11, 92, 32, 136, 114, 52, 10,                                                                                 \
    138, 30, 48, 183, 156, 35, 61, 26, 143, 74, 251, 94, 129, 162, 63, 152, 170, 7, 115, 167, 241, 206, 3, 150, 55,    \
    59, 151, 220, 90, 53, 23, 131,                                                                                     \
    125, 173, 15, 238, 79, 95, 89, 16, 105, 137, 225, 224, 217, 160, 37, 123, 118, 73, 2, 157, 46, 116, 9, 145, 134,   \
    228, 207, 212, 202, 215, 69, 229,                                                                                  \
    27, 188, 67, 124, 168, 252, 42, 4, 29, 108, 21, 247, 19, 205, 39, 203, 233, 40, 186, 147, 198, 192, 155, 33, 164,  \
    191, 98, 204, 165, 180, 117, 76,                                                                                   \
    140, 36, 210, 172, 41, 54, 159, 8, 185, 232, 113, 196, 231, 47, 146, 120, 51, 65, 28, 144, 254, 221, 93, 189, 194, \
    139, 112, 43, 71, 109, 184, 209

// the salts of the six bucket mappings, already sent through the permutation once (Pearson of 2, 3, 5, 7, 11, 13)
#define MRZ_TLSH_SALT_A 49
#define MRZ_TLSH_SALT_B 12
#define MRZ_TLSH_SALT_C 178
#define MRZ_TLSH_SALT_D 166
#define MRZ_TLSH_SALT_E 84
#define MRZ_TLSH_SALT_F 230

// length code: the number of thresholds below the length (a step function; 170 thresholds, ten per row)
static const uint32_t k_tlsh_len_steps[170] = {
    1u, 2u, 3u, 5u, 7u, 11u, 17u, 25u, 38u, 57u,
    86u, 129u, 194u, 291u, 437u, 656u, 854u, 1110u, 1443u, 1876u,
    2439u, 3171u, 3475u, 3823u, 4205u, 4626u, 5088u, 5597u, 6157u, 6772u,
    7450u, 8195u, 9014u, 9916u, 10907u, 11998u, 13198u, 14518u, 15970u, 17567u,
    19323u, 21256u, 23382u, 25720u, 28292u, 31121u, 34233u, 37656u, 41422u, 45564u,
    50121u, 55133u, 60646u, 66711u, 73382u, 80721u, 88793u, 97672u, 107439u, 118183u,
    130002u, 143002u, 157302u, 173032u, 190335u, 209369u, 230306u, 253337u, 278670u, 306538u,
    337191u, 370911u, 408002u, 448802u, 493682u, 543050u, 597356u, 657091u, 722800u, 795081u,
    874589u, 962048u, 1058252u, 1164078u, 1280486u, 1408534u, 1549388u, 1704327u, 1874759u, 2062236u,
    2268459u, 2495305u, 2744836u, 3019320u, 3321252u, 3653374u, 4018711u, 4420582u, 4862641u, 5348905u,
    5883796u, 6472176u, 7119394u, 7831333u, 8614467u, 9475909u, 10423501u, 11465851u, 12612437u, 13873681u,
    15261050u, 16787154u, 18465870u, 20312458u, 22343706u, 24578077u, 27035886u, 29739474u, 32713425u, 35984770u,
    39583245u, 43541573u, 47895730u, 52685306u, 57953837u, 63749221u, 70124148u, 77136564u, 84850228u, 93335252u,
    102668779u, 112935659u, 124229227u, 136652151u, 150317384u, 165349128u, 181884040u, 200072456u, 220079703u,
    242087671u,
    266296456u, 292926096u, 322218735u, 354440623u, 389884688u, 428873168u, 471760495u, 518936559u, 570830240u,
    627913311u,
    690704607u, 759775136u, 835752671u, 919327967u, 1011260767u, 1112386880u, 1223623232u, 1345985727u, 1480584256u,
    1628642751u,
    1791507135u, 1970657856u, 2167723648u, 2384496256u, 2622945920u, 2885240448u, 3173764736u, 3491141248u, 3840255616u,
    4224281216u
};

// the length code of a message of `len` bytes, 0 <= len <= MRZ_TLSH_MAX_LEN: the first step that reaches the length
static inline int mrz_tlsh_lcode(int64_t len) {
    int lo = 0, hi = 169;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if ((int64_t)k_tlsh_len_steps[mid] >= len)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// what the finish kernel leaves per message, and the three checksum chains
struct mrz_tlsh_fin {
    uint32_t q1, q2, q3;  // the 64th, 128th and 192nd smallest bucket count
    uint32_t nonzero;     // buckets that were hit at all
    uint8_t code[MRZ_TLSH_CODE];
};

static inline uint8_t mrz_tlsh_swap_nibbles(uint8_t b) { return (uint8_t)((b << 4) | (b >> 4)); }

// a digest exists when the message is long enough, the upper quartile is not zero and more than half of the buckets
// were hit
static inline bool mrz_tlsh_valid(const mrz_tlsh_fin &f, int64_t len) {
    return len >= MRZ_TLSH_MIN_LEN && f.q3 != 0 && f.nonzero > MRZ_TLSH_BUCKETS / 2;
}

// the 138 hex characters and a NUL into hex[139].  The ratios are taken as the reference takes them: the product in
// 32 bits (it wraps), the division in float, the remainder of the truncated quotient.
static inline void mrz_tlsh_hex(const mrz_tlsh_fin &f, const uint8_t chain[3], int64_t len, char *hex) {
    uint8_t bin[MRZ_TLSH_BIN];
    for (int k = 0; k < 3; k++) bin[k] = mrz_tlsh_swap_nibbles(chain[k]);
    bin[3] = mrz_tlsh_swap_nibbles((uint8_t)mrz_tlsh_lcode(len));
    const unsigned r1 = (unsigned)((float)(uint32_t)(f.q1 * 100u) / (float)f.q3) % 16u;
    const unsigned r2 = (unsigned)((float)(uint32_t)(f.q2 * 100u) / (float)f.q3) % 16u;
    bin[4] = mrz_tlsh_swap_nibbles((uint8_t)(r1 | (r2 << 4)));
    for (int i = 0; i < MRZ_TLSH_CODE; i++) bin[5 + i] = f.code[MRZ_TLSH_CODE - 1 - i];
    static const char digits[] = "0123456789ABCDEF";
    for (int i = 0; i < MRZ_TLSH_BIN; i++) {
        hex[2 * i] = digits[bin[i] >> 4];
        hex[2 * i + 1] = digits[bin[i] & 15];
    }
    hex[MRZ_TLSH_HEX] = 0;
}
