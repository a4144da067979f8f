// mrz_rs.hip -- rs-mrzip's encoder on the GPU: CCSDS RS(255,223) parity in Berlekamp's dual
// basis for every 223-byte row, and the burst interleave, fused.
//
// Restates rse32 (rs-mrzip/reed-solomon.c:115-141), scatter (:311-321) and the burst loop of
// encode() (rs-mrzip/rs-mrzip.c:119-158).  The reference encodes one row after another on one
// core; the 8176 rows of a burst (and all bursts) are independent, so:
//   * a 128-thread workgroup takes 112 consecutive rows (8176 = 73 x 112): their 24,976 input
//     bytes are loaded coalesced (16 B per lane) into an LDS image with 260-byte rows (4 x 65: a
//     row's bytes can be read a dword at a time, and one column of 64 rows spans all 64 banks);
//   * thread t runs the 32-byte LFSR of row t: per data byte one dual->conventional look-up (four
//     at a time, ahead of the steps that use them) and one 32-byte row of the precomputed
//     "feedback x generator" table (256 x 32 B in LDS, its halves in two arrays so that each
//     ds_read_b128 spreads over all banks) XORed into the shifted register held in 8 dwords --
//     the log/antilog arithmetic of the reference (:122-134) is folded into that table;
//   * the 32 parity bytes go back through the conventional->dual table into columns 223..254 of
//     the LDS image, and the image is written out transposed (column c of row r at
//     c * 8176 + r, :311-321) as 16-byte words: 16 rows per lane, 112 contiguous bytes per column.
// The data columns are written unchanged (taltab o tal1tab = identity, :118,138).
// Tables are generated on the host from the field polynomial, the generator roots and the 8
// dual-basis images; nothing is copied from the reference.
//
// Bound: 223 B read + 255 B written per row (478 B per row) against HBM; measured, the kernel is bound by the LFSR's
// LDS traffic instead (32 B of table per data byte: without the LFSR the same kernel moves 3.1 TB/s, with it 1.3).
#include <string.h>

#include <thread>
#include <vector>

#include "mrz_ctx.h"
#include "mrz_device.h"

#define MRZ_RS_ROWS 8176  // BLK_LEN, rs-mrzip/reed-solomon.h:31
#define MRZ_RS_K 223
#define MRZ_RS_N 255
#define MRZ_RS_TILE 112   // rows per workgroup; 8176 = 73 * 112
#define MRZ_RS_THREADS 128
#define MRZ_RS_PITCH 260  // bytes between the rows of the LDS image: 4 x 65 -- a row's data can be read a dword at a time, and
                          // the dwords (and bytes) of one column of 64 consecutive rows lie on 64 different banks

struct mrz_rs_tables {
    uint8_t fbgen[256][32];  // fbgen[f][j] = f * g_j in GF(256), conventional basis
    uint8_t tal[256];        // conventional -> dual basis
    uint8_t tal1[256];       // dual -> conventional
    uint8_t ex[256];         // alpha^i (index -> polynomial form), ex[255] = 0     (Alpha_to, reed-solomon.c:28)
    uint8_t lg[256];         // log_alpha (polynomial -> index form), lg[0] = 255   (Index_of, :43)
};

static void mrz_rs_build_tables(mrz_rs_tables *T) {
    uint8_t ex[256], lg[256];
    unsigned v = 1;
    for (int i = 0; i < 255; i++) {  // GF(2^8), p(x) = x^8 + x^7 + x^2 + x + 1, alpha = 2
        ex[i] = (uint8_t)v;
        lg[v] = (uint8_t)i;
        v <<= 1;
        if (v & 0x100) v ^= 0x187;
    }
    auto mul = [&](uint8_t a, uint8_t b) -> uint8_t { return (!a || !b) ? 0 : ex[(lg[a] + lg[b]) % 255]; };
    uint8_t g[33] = { 1 };  // g(x) = prod_{j=112..143} (x - alpha^(11 j))
    for (int j = 112, deg = 0; j <= 143; j++, deg++) {
        const uint8_t root = ex[(11 * j) % 255];
        g[deg + 1] = 0;
        for (int k = deg + 1; k > 0; k--) g[k] = g[k - 1] ^ mul(g[k], root);
        g[0] = mul(g[0], root);
    }
    for (int f = 0; f < 256; f++)
        for (int j = 0; j < 32; j++) T->fbgen[f][j] = mul((uint8_t)f, g[j]);
    static const uint8_t basis[8] = { 0x8d, 0xef, 0xec, 0x86, 0xfa, 0x99, 0xaf, 0x7b };
    for (int i = 0; i < 256; i++) {
        uint8_t t = 0;
        for (int k = 0; k < 8; k++)
            if (i & (1 << k)) t ^= basis[7 - k];
        T->tal[i] = t;
    }
    for (int i = 0; i < 256; i++) T->tal1[T->tal[i]] = (uint8_t)i;
    for (int i = 0; i < 255; i++) {
        T->ex[i] = ex[i];
        T->lg[ex[i]] = (uint8_t)i;
    }
    T->ex[255] = 0;
    T->lg[0] = 255;
}

// the tables, built and uploaded on a ctx's first Reed-Solomon call
static int mrz_rs_need_tables(mrz_ctx *ctx) {
    if (ctx->d_rs_tables) return MRZ_OK;
    mrz_rs_tables *T = (mrz_rs_tables *)malloc(sizeof(mrz_rs_tables));
    void *p = nullptr;
    hipError_t e = T ? hipMalloc(&p, sizeof(mrz_rs_tables)) : hipErrorOutOfMemory;
    if (e == hipSuccess) {
        mrz_rs_build_tables(T);
        e = hipMemcpy(p, T, sizeof(mrz_rs_tables), hipMemcpyHostToDevice);
    }
    free(T);
    if (e != hipSuccess) {
        if (p) hipFree(p);
        ctx->last_err = e;
        return MRZ_E_NOMEM;
    }
    ctx->d_rs_tables = p;
    return MRZ_OK;
}

// grid.x = bursts * 73; each workgroup: 112 rows of one burst
__global__ __launch_bounds__(MRZ_RS_THREADS) void mrz_rs_encode_kernel(const uint8_t *__restrict__ in, int64_t n,
                                                                       const mrz_rs_tables *__restrict__ T,
                                                                       uint8_t *__restrict__ out) {
    // (the two halves of a table row in arrays of their own: a 16-byte read of row f then lands on banks 4 (f % 16)..+3,
    // all 64 banks in use -- with 32-byte rows each of the two reads had half of the banks to itself)
    __shared__ __attribute__((aligned(16))) uint8_t s_fb_lo[256][16], s_fb_hi[256][16];
    __shared__ uint8_t s_tal[256], s_tal1[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[MRZ_RS_TILE * MRZ_RS_PITCH + 16];

    const int tid = threadIdx.x;
    for (int i = tid; i < 256 * 32 / 16; i += MRZ_RS_THREADS) {
        const uint4 v = reinterpret_cast<const uint4 *>(&T->fbgen[0][0])[i];
        *reinterpret_cast<uint4 *>((i & 1) ? &s_fb_hi[i >> 1][0] : &s_fb_lo[i >> 1][0]) = v;
    }
    for (int i = tid; i < 256; i += MRZ_RS_THREADS) {
        s_tal[i] = T->tal[i];
        s_tal1[i] = T->tal1[i];
    }
    const int64_t burst = blockIdx.x / (MRZ_RS_ROWS / MRZ_RS_TILE);
    const int tile = blockIdx.x % (MRZ_RS_ROWS / MRZ_RS_TILE);
    const int64_t row0 = burst * MRZ_RS_ROWS + (int64_t)tile * MRZ_RS_TILE;  // global row index
    const int64_t in0 = row0 * MRZ_RS_K;
    // stage 112 x 223 input bytes (zero beyond n, rs-mrzip.c:132-133) into 255-byte LDS rows
    const int tile_bytes = MRZ_RS_TILE * MRZ_RS_K;
    for (int x = tid * 16; x < tile_bytes; x += MRZ_RS_THREADS * 16) {
        uint8_t tmp[16];
        const int64_t gpos = in0 + x;
        if (gpos + 16 <= n) {
            const uint4 v = mrz_ld16(in + gpos);
            __builtin_memcpy(tmp, &v, 16);
        } else {
            for (int k = 0; k < 16; k++) tmp[k] = (gpos + k < n) ? in[gpos + k] : (uint8_t)0;
        }
        int r = x / MRZ_RS_K, c = x % MRZ_RS_K;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            s_img[r * MRZ_RS_PITCH + c] = tmp[k];  // (112 x 223 = 1561 x 16: no piece straddles the tile's end)
            if (++c == MRZ_RS_K) {
                c = 0;
                r++;
            }
        }
    }
    __syncthreads();
#ifndef MRZ_RS_SKIP_LFSR  // (-DMRZ_RS_SKIP_LFSR / -DMRZ_RS_SKIP_SCATTER: ablation builds for tools/probe_rs.py, never shipped)
    if (tid < MRZ_RS_TILE) {
        // rse32: bb[j] = bb[j-1] ^ g_j * feedback, bb[0] = g_0 * feedback  (:120-135)
        uint32_t b[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        // The data bytes come a dword at a time and their dual->conventional look-ups four at a time: none of that
        // waits for the register, so a step's critical path is the one trip to the LDS for its table row.
        const uint32_t *row32 = reinterpret_cast<const uint32_t *>(&s_img[tid * MRZ_RS_PITCH]);
        auto step = [&](uint32_t d) {
            const uint32_t fb = d ^ (b[7] >> 24);
#pragma unroll
            for (int k = 7; k > 0; k--) b[k] = (b[k] << 8) | (b[k - 1] >> 24);
            b[0] <<= 8;
            const uint4 g0 = *reinterpret_cast<const uint4 *>(&s_fb_lo[fb][0]);
            const uint4 g1 = *reinterpret_cast<const uint4 *>(&s_fb_hi[fb][0]);
            b[0] ^= g0.x;
            b[1] ^= g0.y;
            b[2] ^= g0.z;
            b[3] ^= g0.w;
            b[4] ^= g1.x;
            b[5] ^= g1.y;
            b[6] ^= g1.z;
            b[7] ^= g1.w;
        };
        {  // bytes 222, 221, 220 (223 = 4 x 55 + 3; the top byte of this dword is the first parity column)
            const uint32_t w = row32[MRZ_RS_K / 4];
            const uint32_t d2 = s_tal1[(w >> 16) & 0xff], d1 = s_tal1[(w >> 8) & 0xff], d0 = s_tal1[w & 0xff];
            step(d2);
            step(d1);
            step(d0);
        }
#pragma unroll 2
        for (int j = MRZ_RS_K / 4 - 1; j >= 0; j--) {
            const uint32_t w = row32[j];
            const uint32_t d3 = s_tal1[w >> 24], d2 = s_tal1[(w >> 16) & 0xff], d1 = s_tal1[(w >> 8) & 0xff],
                           d0 = s_tal1[w & 0xff];
            step(d3);
            step(d2);
            step(d1);
            step(d0);
        }
        uint8_t *par = &s_img[tid * MRZ_RS_PITCH + MRZ_RS_K];
#pragma unroll
        for (int j = 0; j < 32; j++) par[j] = s_tal[(b[j >> 2] >> (8 * (j & 3))) & 0xff];  // :138
    }
#endif
    __syncthreads();
    // scatter (:311-321): dst[c * 8176 + r] = row r, column c.  A column's 112 bytes of this tile are 7 x 16 B: a lane
    // gathers 16 rows of one column from the image (the odd row pitch keeps the 16 byte reads of neighbouring lanes on
    // different banks) and stores them as one 16-byte word (8176, 112 and the burst size are multiples of 16)
#ifndef MRZ_RS_SKIP_SCATTER
    uint8_t *dst = out + burst * (int64_t)MRZ_RS_N * MRZ_RS_ROWS + (int64_t)tile * MRZ_RS_TILE;
    const int segs = MRZ_RS_TILE / 16;  // 7
    for (int idx = tid; idx < MRZ_RS_N * segs; idx += MRZ_RS_THREADS) {
        const int c = idx / segs, u = idx % segs;
        const uint8_t *p = &s_img[(16 * u) * MRZ_RS_PITCH + c];
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            w[k] = (uint32_t)p[(4 * k) * MRZ_RS_PITCH] | (uint32_t)p[(4 * k + 1) * MRZ_RS_PITCH] << 8 |
                   (uint32_t)p[(4 * k + 2) * MRZ_RS_PITCH] << 16 | (uint32_t)p[(4 * k + 3) * MRZ_RS_PITCH] << 24;
        uint4 v;
        v.x = w[0];
        v.y = w[1];
        v.z = w[2];
        v.w = w[3];
        *reinterpret_cast<uint4 *>(dst + (int64_t)c * MRZ_RS_ROWS + 16 * u) = v;
    }
#endif
}

// ---- BLAKE2b-512 on the host (the trailer hash of rs-mrzip.c:138,148 is one serial chain over
// the whole padded stream; it runs on a host thread while the GPU encodes) ---------------------
namespace {
struct HostB2 {
    uint64_t h[8], t0 = 0, t1 = 0;
    uint8_t buf[128];
    size_t buflen = 0;
    static uint64_t ror(uint64_t x, int c) { return (x >> c) | (x << (64 - c)); }
    HostB2() {
        static const uint64_t iv[8] = { 0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                                        0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                                        0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL };
        for (int i = 0; i < 8; i++) h[i] = iv[i];
        h[0] ^= 0x01010000ULL ^ 64;
    }
    void compress(const uint8_t *blk, bool last) {
        static const uint64_t iv[8] = { 0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                                        0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                                        0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL };
        static const uint8_t sg[10][16] = {
            { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 }, { 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3 },
            { 11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4 }, { 7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8 },
            { 9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13 }, { 2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9 },
            { 12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11 }, { 13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10 },
            { 6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5 }, { 10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0 }
        };
        uint64_t m[16], v[16];
        memcpy(m, blk, 128);
        for (int i = 0; i < 8; i++) {
            v[i] = h[i];
            v[i + 8] = iv[i];
        }
        v[12] ^= t0;
        v[13] ^= t1;
        if (last) v[14] = ~v[14];
        static const int q[8][4] = { { 0, 4, 8, 12 }, { 1, 5, 9, 13 }, { 2, 6, 10, 14 }, { 3, 7, 11, 15 },
                                     { 0, 5, 10, 15 }, { 1, 6, 11, 12 }, { 2, 7, 8, 13 }, { 3, 4, 9, 14 } };
        for (int r = 0; r < 12; r++) {
            const uint8_t *s = sg[r % 10];
            for (int g = 0; g < 8; g++) {
                uint64_t &a = v[q[g][0]], &b = v[q[g][1]], &c = v[q[g][2]], &d = v[q[g][3]];
                a += b + m[s[2 * g]];
                d = ror(d ^ a, 32);
                c += d;
                b = ror(b ^ c, 24);
                a += b + m[s[2 * g + 1]];
                d = ror(d ^ a, 16);
                c += d;
                b = ror(b ^ c, 63);
            }
        }
        for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
    }
    void count(uint64_t inc) {
        t0 += inc;
        if (t0 < inc) t1++;
    }
    void update(const uint8_t *p, size_t n) {
        while (n) {
            if (buflen == 128) {
                count(128);
                compress(buf, false);
                buflen = 0;
            }
            size_t take = 128 - buflen;
            if (take > n) take = n;
            memcpy(buf + buflen, p, take);
            buflen += take;
            p += take;
            n -= take;
        }
    }
    void zeros(uint64_t n) {
        static const uint8_t z[4096] = { 0 };
        while (n) {
            const size_t take = n > sizeof(z) ? sizeof(z) : (size_t)n;
            update(z, take);
            n -= take;
        }
    }
    void final(uint8_t out[64]) {
        count(buflen);
        memset(buf + buflen, 0, 128 - buflen);
        compress(buf, true);
        memcpy(out, h, 64);
    }
};
}  // namespace

extern "C" int64_t mrz_rs_encoded_size(int64_t n) {
    if (n < 0) return MRZ_E_ARG;
    const int64_t burst_in = (int64_t)MRZ_RS_K * MRZ_RS_ROWS;
    return (n / burst_in + 1) * (int64_t)MRZ_RS_N * MRZ_RS_ROWS + 64 + 4;  // feof() needs a short read (rs-mrzip.c:125)
}

extern "C" int mrz_rs_encode(mrz_ctx *ctx, const void *in, int64_t n, int where, void *out, int out_where,
                             int64_t out_cap) {
    if (!ctx || n < 0 || (n > 0 && !in) || !out) return MRZ_E_ARG;
    const int64_t total = mrz_rs_encoded_size(n);
    if (out_cap < total) return MRZ_E_ARG;
    if (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t burst_in = (int64_t)MRZ_RS_K * MRZ_RS_ROWS, burst_out = (int64_t)MRZ_RS_N * MRZ_RS_ROWS;
    const int64_t nbursts = n / burst_in + 1;

    // the serial trailer hash runs on a host thread (host input) or after a device->host copy
    std::vector<uint8_t> host_copy;
    const uint8_t *h_in = (const uint8_t *)in;
    const uint8_t *d_in = nullptr;
    int rc = mrz_stage_input(ctx, in, n, where, &d_in);
    if (rc) return rc;
    if (where == MRZ_MEM_DEVICE) {
        host_copy.resize((size_t)n);
        if (n) HIPCHK(ctx, hipMemcpy(host_copy.data(), in, (size_t)n, hipMemcpyDeviceToHost));
        h_in = host_copy.data();
    }
    uint8_t digest[64];
    std::thread hasher([&]() {
        HostB2 b;
        b.update(h_in, (size_t)n);
        b.zeros((uint64_t)(nbursts * burst_in - n));  // the padded rows are hashed too (rs-mrzip.c:132-138)
        b.final(digest);
    });

    rc = mrz_rs_need_tables(ctx);
    if (rc) {
        hasher.join();
        return rc;
    }
    uint8_t *d_out = (uint8_t *)out;
    if (out_where == MRZ_MEM_HOST) {
        rc = mrz_grow(ctx, &ctx->d_rs_out, &ctx->rs_out_cap, nbursts * burst_out);
        if (rc) {
            hasher.join();
            return rc;
        }
        d_out = ctx->d_rs_out;
    }
    hipError_t e = hipSuccess;
    hipEvent_t ea = nullptr, eb = nullptr;
    if (ctx->profiling) {
        hipEventCreate(&ea);
        hipEventCreate(&eb);
        hipEventRecord(ea, ctx->stream);
    }
    hipLaunchKernelGGL(mrz_rs_encode_kernel, dim3((unsigned)(nbursts * (MRZ_RS_ROWS / MRZ_RS_TILE))), dim3(MRZ_RS_THREADS),
                       0, ctx->stream, d_in, n, (const mrz_rs_tables *)ctx->d_rs_tables, d_out);
    e = hipGetLastError();
    if (ctx->profiling) hipEventRecord(eb, ctx->stream);
    if (e == hipSuccess && out_where == MRZ_MEM_HOST)
        e = hipMemcpyAsync(out, d_out, (size_t)(nbursts * burst_out), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (ctx->profiling) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ea, eb) == hipSuccess) ctx->timings.encode_ms = ms;  // reported via mrz_get_timings
        hipEventDestroy(ea);
        hipEventDestroy(eb);
    }
    hasher.join();
    if (e != hipSuccess) {
        ctx->last_err = e;
        return MRZ_E_HIP;
    }
    // trailer: BLAKE2b-512 + k_i, k_j (first short row and its length, rs-mrzip.c:128-136,148-157)
    const int64_t rem = n - (nbursts - 1) * burst_in;
    const unsigned k_i = (unsigned)(rem / MRZ_RS_K), k_j = (unsigned)(rem % MRZ_RS_K);
    uint8_t tail[68];
    memcpy(tail, digest, 64);
    tail[64] = (uint8_t)(k_i & 0xff);
    tail[65] = (uint8_t)(k_i >> 8);
    tail[66] = (uint8_t)(k_j & 0xff);
    tail[67] = (uint8_t)(k_j >> 8);
    if (out_where == MRZ_MEM_HOST)
        memcpy((uint8_t *)out + nbursts * burst_out, tail, 68);
    else
        HIPCHK(ctx, hipMemcpy((uint8_t *)out + nbursts * burst_out, tail, 68, hipMemcpyHostToDevice));
    return MRZ_OK;
}


// ---- rs-mrzip decoder (rs-mrzip/rs-mrzip.c:37-117 decode(), reed-solomon.c:143-309 rsd32, :323-333 gather) ------
// Two kernels on one stream, no host read-back between them.
//
// mrz_rs_decode_kernel, one lane per codeword: the 8176 rows of a burst are independent.  A workgroup takes 128 rows:
// the interleaved input is read column by column (byte c of row r at c * 8176 + r: coalesced across the lanes), kept
// in an LDS image, and the 32 syndromes s[i] = row(alpha^(11 (111 + i))) of its dual->conventional image are
// accumulated on the way.  The 223 data bytes of every row go out as they came, row-major (taltab o tal1tab =
// identity).  Rows whose syndromes vanish -- all of them on undamaged input -- get status 0 and are done; every other
// row is appended to a device list as {row, 32 syndromes in index form}: one agent-scope atomic per wave reserves the
// slots of all its damaged rows.
//
// mrz_rs_repair_kernel, one WAVE per codeword: a fixed grid whose waves stride over that list.  Repair needs the
// syndromes only.  The error locator, its roots and the error values are those of rsd32 -- same field, same syndromes,
// Berlekamp-Massey over 32 steps without erasures, Chien points i = 1..255 with location 139 i mod 255, Forney with
// alpha^(111 i) -- so corrected bytes, counts and "uncorrectable" verdicts (miscorrections included) agree with it;
// the work is laid across the lanes instead of arrays:
//   * lane i (0..32) holds lambda_i and b_i; the discrepancy of step r is the XOR of the terms lambda_i s[r-i], which
//     the lanes put side by side in LDS and every lane folds for itself; the shift of b goes the same way;
//   * the 255 Chien points are 4 passes of 64, one point per lane and pass, evaluated together (lambda_j is
//     one broadcast read per j); ballots count the roots.  The sum over the odd j is kept apart: the derivative
//     rsd32 divides by, sum_{j odd} lambda_j x^(j-1), is that sum times x^-1;
//   * lane i (0..31) forms omega_i = sum_j s[i+1-j] lambda_j, and every lane evaluates omega at its four points the
//     same way; the lanes whose point is a root then hold numerator and denominator of their error value.
// The value e of column loc is XORed into the output where kernel 1 left the row: taltab is GF(2)-linear (built by
// XOR of basis images), so tal[a ^ e] = tal[a] ^ tal[e] and the conventional-basis row image is not needed.  Columns
// 223..254 are parity: counted, not part of the output.  A locator with deg distinct roots is separable, so its
// derivative cannot vanish at one of them (rsd32's `den == 0` exit is dead code once the root count matches); a guard
// reports -1 all the same.  Roots are distinct columns, so the order they are applied in does not matter.
//
// Known-lost ranges (mrz_rs_decode_lost, mrz_rs_repair_kernel<true>): rsd32(data, eras_pos, no_eras), :183-193,198-221,
// which the reference's decode() always calls with no_eras = 0.  The caller's sorted byte ranges of the encoded input
// are copied to device scratch on the ctx stream; mrz_rs_decode_kernel does not look at them (clean input pays
// nothing), and the repair kernel without them, <false>, is the kernel above.  Per listed codeword <true> adds:
//   * every lane searches the ranges for the byte offsets of the columns of its four Chien points (binary search);
//     four ballots give the erased columns in the Chien layout, no_eras is their popcount;
//   * lambda starts as the erasure locator prod (1 + alpha^(11 c) x): no_eras wave-uniform steps
//     lam_i ^= alpha^u lam_(i-1) through the two slots of b in turn, then b_i = log lam_i;
//   * Berlekamp-Massey runs from r = no_eras + 1 with el = no_eras, the branch test 2 el <= r + no_eras - 1 and the
//     update el = r + no_eras - el: 32 - no_eras steps.  Chien, omega and Forney are unchanged; deg may reach 32.
// Three rules fix the status: zero syndromes give 0 whatever is marked (the row is never listed; rsd32 returns before
// it looks at eras_pos); more than 32 erased columns in a listed row give -1 and the row stays as it came (this
// project's definition: rsd32's locator loop would write lambda[33]); otherwise the status is rsd32's, the number of
// roots of the errata locator, in which erased columns count even where the byte was right.
#define MRZ_RSD_ROWS 128
#define MRZ_RSD_STRIDE 260  // bytes per LDS row (65 words: lanes of a wave hit different banks)
#define MRZ_RSR_THREADS 256  // repair kernel: 4 waves per workgroup
#define MRZ_RSR_WGS_PER_CU 8

struct mrz_rsd_entry {
    int row;        // global codeword index: burst * 8176 + row of the burst
    uint32_t s[8];  // s[1..32] in index form (255 = zero), s[i] in byte i - 1
};
struct mrz_rsd_head {
    unsigned long long corrected;      // sum of the positive statuses
    unsigned long long uncorrectable;  // number of -1 statuses
    unsigned n_listed;                 // entries of the list
    unsigned pad;
};

__global__ __launch_bounds__(MRZ_RSD_ROWS) void mrz_rs_decode_kernel(const uint8_t *__restrict__ in,
                                                                     const mrz_rs_tables *__restrict__ T,
                                                                     uint8_t *__restrict__ out, int *__restrict__ counts,
                                                                     mrz_rsd_head *__restrict__ head,
                                                                     mrz_rsd_entry *__restrict__ list) {
    __shared__ uint8_t s_ex[256], s_lg[256], s_tal1[256];
    __shared__ __attribute__((aligned(4))) uint8_t s_img[MRZ_RSD_ROWS * MRZ_RSD_STRIDE];
    const int tid = threadIdx.x;
    for (int i = tid; i < 256; i += MRZ_RSD_ROWS) {
        s_ex[i] = T->ex[i];
        s_lg[i] = T->lg[i];
        s_tal1[i] = T->tal1[i];
    }
    __syncthreads();
    const int tiles = (MRZ_RS_ROWS + MRZ_RSD_ROWS - 1) / MRZ_RSD_ROWS;  // 64: the last one holds 112 rows
    const int64_t burst = blockIdx.x / tiles;
    const int row0 = (int)(blockIdx.x % tiles) * MRZ_RSD_ROWS;
    const int nrows = MRZ_RS_ROWS - row0 < MRZ_RSD_ROWS ? MRZ_RS_ROWS - row0 : MRZ_RSD_ROWS;
    const uint8_t *src = in + burst * (int64_t)MRZ_RS_N * MRZ_RS_ROWS + row0;
    uint8_t *row = &s_img[tid * MRZ_RSD_STRIDE];
    int syn_error = 0;
    uint32_t sw[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };  // the syndromes in index form, four to a dword
    if (tid < nrows) {
        // gather + dual -> conventional + syndromes: s[i] = sum_j data[j] alpha^((111 + i) 11 j), :156-166
        int s[33], pw[33];
#pragma unroll
        for (int i = 1; i <= 32; i++) {
            s[i] = 0;
            pw[i] = 0;
        }
        for (int c = 0; c < MRZ_RS_N; c++) {
            const uint8_t raw = src[(int64_t)c * MRZ_RS_ROWS + tid];
            row[c] = raw;
            const int d = s_tal1[raw];
            if (d != 0) {
                const int lgd = s_lg[d];
#pragma unroll
                for (int i = 1; i <= 32; i++) {
                    int e = lgd + pw[i];
                    e = e >= 255 ? e - 255 : e;
                    s[i] ^= s_ex[e];
                }
            }
#pragma unroll
            for (int i = 1; i <= 32; i++) {  // exponent of column c + 1
                int e = pw[i] + ((111 + i) * 11) % 255;
                pw[i] = e >= 255 ? e - 255 : e;
            }
        }
#pragma unroll
        for (int i = 1; i <= 32; i++) {
            syn_error |= s[i];
            sw[(i - 1) >> 2] |= (uint32_t)s_lg[s[i]] << (8 * ((i - 1) & 3));
        }
        if (!syn_error) counts[burst * MRZ_RS_ROWS + row0 + tid] = 0;
    }
    // damaged rows go to the list: the wave's first damaged lane reserves the slots of all of them
    const unsigned long long damaged = __ballot(syn_error != 0);
    if (damaged) {
        const int lane = tid & 63;
        const int leader = __ffsll((long long)damaged) - 1;
        int base = 0;
        if (lane == leader)
            base = (int)__hip_atomic_fetch_add(&head->n_listed, (unsigned)__popcll(damaged), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
        base = __shfl(base, leader);
        if (syn_error) {
            mrz_rsd_entry *e = &list[base + __popcll(damaged & ((1ull << lane) - 1))];
            e->row = (int)(burst * MRZ_RS_ROWS + row0 + tid);
#pragma unroll
            for (int k = 0; k < 8; k++) e->s[k] = sw[k];
        }
    }
    __syncthreads();
    // the data bytes of the rows, row-major
    uint8_t *dst = out + (burst * MRZ_RS_ROWS + row0) * (int64_t)MRZ_RS_K;
    for (int idx = tid; idx < nrows * MRZ_RS_K; idx += MRZ_RSD_ROWS) {
        const int r = idx / MRZ_RS_K, c = idx % MRZ_RS_K;
        dst[idx] = s_img[r * MRZ_RSD_STRIDE + c];
    }
}

// grid: any; the waves stride over the list.  The lanes of a wave hand values to each other through a piece of LDS
// that belongs to the wave: a wave's LDS operations execute in program order, so what every lane stored before a
// ballot is there for all of them after it (the accesses are volatile: the compiler keeps their order too).  The
// ballot itself is the point where the lanes meet when the wave is emulated by fibers, which is also why a value that
// is rewritten every Berlekamp-Massey step has two slots, used in turn.  All 64 lanes run every ballot: the loop
// bounds and branches around them are wave-uniform.
struct mrz_rsr_wave {
    uint8_t syn[64];      // [i] = s[i], index form, for i = 1..32; 255 elsewhere
    uint8_t term[2][32];  // the terms lambda_i s[r-i] of a step's discrepancy
    uint8_t b[2][40];     // [i + 1] = b_i of a step; [0] = 255, what is shifted in
    uint8_t lam[36];      // lambda in index form
    uint8_t om[32];       // omega in index form
};

// is byte `pos` of the encoded input inside one of the n sorted, disjoint ranges?  (the last range that starts at or
// before pos is the only one that can hold it)
__device__ static inline bool mrz_rs_in_ranges(const mrz_rs_range *__restrict__ rg, int64_t n, int64_t pos) {
    int64_t lo = 0, hi = n;  // -> the first range that starts beyond pos
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rg[mid].offset <= pos)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo > 0 && pos < rg[lo - 1].offset + rg[lo - 1].len;
}

// ERAS = false is the decoder without erasures (mrz_rs_decode_ex; rg / n_rg are not looked at); ERAS = true takes the
// caller's lost ranges (mrz_rs_decode_lost).
template <bool ERAS>
__global__ __launch_bounds__(MRZ_RSR_THREADS) void mrz_rs_repair_kernel(const mrz_rs_tables *__restrict__ T,
                                                                        const mrz_rsd_entry *__restrict__ list,
                                                                        mrz_rsd_head *__restrict__ head,
                                                                        uint8_t *__restrict__ out, int *__restrict__ counts,
                                                                        const mrz_rs_range *__restrict__ rg, int64_t n_rg) {
    __shared__ uint8_t s_ex[512];  // alpha^i for i = 0..509: the sum of two index forms needs no reduction mod 255
    __shared__ uint8_t s_lg[256], s_tal[256];
    __shared__ __attribute__((aligned(16))) mrz_rsr_wave s_wave[MRZ_RSR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 512; i += MRZ_RSR_THREADS) s_ex[i] = i < 510 ? T->ex[i < 255 ? i : i - 255] : (uint8_t)0;
    for (int i = tid; i < 256; i += MRZ_RSR_THREADS) {
        s_lg[i] = T->lg[i];
        s_tal[i] = T->tal[i];
    }
    volatile mrz_rsr_wave *W = &s_wave[tid / 64];
    if (lane < 2) W->b[lane][0] = 255;
    __syncthreads();
    const unsigned n_listed = head->n_listed;  // complete: the kernel that wrote it ran before this one
    const unsigned n_waves = gridDim.x * (MRZ_RSR_THREADS / 64);
    unsigned long long corrected = 0, lost = 0;  // of this wave's codewords (wave-uniform)
    // the four Chien points of this lane, i = lane + 1 + 64 p, and i mod 255 (point 256 does not exist)
    int pt[4], step[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        pt[p] = lane + 1 + 64 * p;
        step[p] = pt[p] >= 255 ? pt[p] - 255 : pt[p];
    }
    for (unsigned k = blockIdx.x * (MRZ_RSR_THREADS / 64) + tid / 64; k < n_listed; k += n_waves) {
        const mrz_rsd_entry *ent = &list[k];
        const int row = ent->row;
        // the erased columns, in the layout of the Chien points: bit l of eras[p] = column 139 pt mod 255 of point
        // pt = l + 1 + 64 p lies in a lost range (column c of row r of burst b is byte b * 2084880 + c * 8176 + r)
        unsigned long long eras[4] = { 0, 0, 0, 0 };
        int no_eras = 0;
        if (ERAS) {
            const int64_t at = (int64_t)(row / MRZ_RS_ROWS) * ((int64_t)MRZ_RS_N * MRZ_RS_ROWS) + row % MRZ_RS_ROWS;
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int col = (139 * pt[p]) % 255;
                eras[p] = __ballot(pt[p] <= 255 && mrz_rs_in_ranges(rg, n_rg, at + (int64_t)col * MRZ_RS_ROWS));
                no_eras += __popcll(eras[p]);
            }
            if (no_eras > 32) {  // beyond the code's reach (and rsd32's lambda[33]): uncorrectable, the row stays as it came
                if (lane == 0) counts[row] = -1;
                lost++;
                continue;
            }
        }
        W->syn[lane] = lane >= 1 && lane <= 32 ? reinterpret_cast<const uint8_t *>(ent->s)[lane - 1] : (uint8_t)255;

        // Berlekamp-Massey: lambda in polynomial form, b in index form, coefficient i on lane i (0..32)
        int lam = lane == 0 ? 1 : 0, b = lane == 0 ? 0 : 255, el = 0;
        (void)__ballot(1);  // syn is there
        if (ERAS && no_eras) {
            // lambda starts as the erasure locator prod (1 + alpha^(11 c) x) over the erased columns c (:183-193): one
            // wave-uniform step lam_i ^= alpha^u lam_(i-1) per column, the coefficient below handed down through the
            // slots of b (b[.][0] = 255 is the zero that lane 0 takes).  The product does not depend on the order.
            int k = 0;
#pragma unroll 1
            for (int p = 0; p < 4; p++) {
#pragma unroll 1
                for (unsigned long long m = eras[p]; m; m &= m - 1) {
                    const int c = (139 * (__ffsll((long long)m) + 64 * p)) % 255, u = (11 * c) % 255;
                    const int slot = ++k & 1;
                    if (lane <= 32) W->b[slot][lane + 1] = s_lg[lam];
                    (void)__ballot(1);
                    const int down = lane <= 32 ? (int)W->b[slot][lane] : 255;
                    if (down != 255) lam ^= s_ex[u + down];
                }
            }
            b = s_lg[lam];
            el = no_eras;
        }
#pragma unroll 1
        for (int r = no_eras + 1; r <= 32; r++) {
            const int slot = r & 1;
            if (lane < 32) {
                int t = 0;
                if (lane < r && lam != 0) {
                    const int sv = W->syn[r - lane];
                    if (sv != 255) t = s_ex[s_lg[lam] + sv];
                }
                W->term[slot][lane] = (uint8_t)t;
            }
            if (lane <= 32) W->b[slot][lane + 1] = (uint8_t)b;
            (void)__ballot(1);
            const volatile uint32_t *tw = reinterpret_cast<const volatile uint32_t *>(&W->term[slot][0]);
            uint32_t x = tw[0] ^ tw[1] ^ tw[2] ^ tw[3] ^ tw[4] ^ tw[5] ^ tw[6] ^ tw[7];
            x ^= x >> 16;
            x ^= x >> 8;
            const int d = s_lg[x & 0xff];                    // the discrepancy, index form
            const int bdown = lane <= 32 ? (int)W->b[slot][lane] : 255;  // b of the coefficient below
            if (d == 255) {
                b = bdown;
            } else {
                const int t = bdown != 255 ? lam ^ (int)s_ex[d + bdown] : lam;
                if (2 * el <= r + no_eras - 1) {
                    el = r + no_eras - el;
                    const int q = (int)s_lg[lam] - d + 255;
                    b = lam == 0 ? 255 : (q >= 255 ? q - 255 : q);
                } else
                    b = bdown;
                lam = t;
            }
        }
        const int lidx = s_lg[lam];  // index form; lanes above 32 hold zero
        if (lane <= 32) W->lam[lane] = (uint8_t)lidx;
        unsigned long long nz = __ballot(lidx != 255);  // bit 0 is set: lambda_0 = 1
        nz |= nz >> 1;
        nz |= nz >> 2;
        nz |= nz >> 4;
        nz |= nz >> 8;
        nz |= nz >> 16;
        nz |= nz >> 32;
        const int deg = __popcll(nz) - 1;

        // Chien search: lambda(alpha^i) at the four points of the lane; the terms of odd j also on their own
        int ev[4] = { 1, 1, 1, 1 }, odd[4] = { 0, 0, 0, 0 }, e[4] = { 0, 0, 0, 0 };
#pragma unroll 1
        for (int j = 1; j <= deg; j++) {
            const int lj = W->lam[j];
#pragma unroll
            for (int p = 0; p < 4; p++) {  // i j mod 255
                const int x = e[p] + step[p];
                e[p] = x >= 255 ? x - 255 : x;
            }
            if (lj != 255) {
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int v = s_ex[lj + e[p]];
                    ev[p] ^= v;
                    if (j & 1) odd[p] ^= v;
                }
            }
        }
        int nroots = 0, no_den = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int is_root = pt[p] <= 255 && ev[p] == 0;
            nroots += __popcll(__ballot(is_root));
            no_den |= is_root && odd[p] == 0;
        }
        int status = deg;
        if (nroots != deg || __ballot(no_den)) {
            status = -1;  // uncorrectable: the row stays as it came
        } else {
            // omega(x) = s(x) lambda(x) mod x^32, coefficient i on lane i, index form
            if (lane < 32) {
                int om = 0;
                const int top = deg < lane ? deg : lane;
#pragma unroll 1
                for (int j = 0; j <= top; j++) {
                    const int lj = W->lam[j], sv = W->syn[lane + 1 - j];
                    if (lj != 255 && sv != 255) om ^= s_ex[lj + sv];
                }
                W->om[lane] = s_lg[om];
            }
            (void)__ballot(1);
            int num[4] = { 0, 0, 0, 0 };
#pragma unroll
            for (int p = 0; p < 4; p++) e[p] = 0;
#pragma unroll 1
            for (int c = 0; c < 32; c++) {  // omega(alpha^i)
                const int oc = W->om[c];
                if (oc != 255) {
#pragma unroll
                    for (int p = 0; p < 4; p++) num[p] ^= s_ex[oc + e[p]];
                }
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int x = e[p] + step[p];
                    e[p] = x >= 255 ? x - 255 : x;
                }
            }
            // Forney: value = omega(x) x^111 / lambda'(x) at x = alpha^i, and lambda'(x) = x^-1 * (odd terms)
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (pt[p] <= 255 && ev[p] == 0 && num[p] != 0) {
                    const int loc = (139 * pt[p]) % 255;
                    const int x = ((int)s_lg[num[p]] + (112 * step[p]) % 255 + 255 - (int)s_lg[odd[p]]) % 255;
                    if (loc < MRZ_RS_K) out[(int64_t)row * MRZ_RS_K + loc] ^= s_tal[s_ex[x]];
                }
            }
        }
        if (lane == 0) counts[row] = status;
        if (status > 0) corrected += (unsigned long long)status;
        if (status < 0) lost++;
    }
    if (lane == 0) {
        if (corrected) atomicAdd(&head->corrected, corrected);
        if (lost) atomicAdd(&head->uncorrectable, lost);
    }
}

extern "C" int64_t mrz_rs_codewords(int64_t n) {
    return n < 0 ? 0 : n / ((int64_t)MRZ_RS_N * MRZ_RS_ROWS) * MRZ_RS_ROWS;
}

// mrz_rs_decode_ex (n_lost = 0) and mrz_rs_decode_lost: `lost` is host memory, checked by the caller
static int mrz_rs_decode_impl(mrz_ctx *ctx, const void *in, int64_t n, int where, void *out, int out_where,
                              int64_t out_cap, int64_t *out_len, const mrz_rs_range *lost, int64_t n_lost,
                              int32_t *row_status, int status_where, int flags, mrz_rs_report *rep) {
    if (!ctx || !in || !out || !out_len || n < 0) return MRZ_E_ARG;
    if (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    if (row_status && status_where != MRZ_MEM_HOST && status_where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    const int64_t burst_in = (int64_t)MRZ_RS_K * MRZ_RS_ROWS, burst_out = (int64_t)MRZ_RS_N * MRZ_RS_ROWS;
    const int64_t nbursts = n / burst_out;
    const int64_t tail = n - nbursts * burst_out;
    if (nbursts < 1) return MRZ_E_CORRUPT;
    if (out_cap < nbursts * burst_in) return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t *d_in = nullptr;
    int rc = mrz_stage_input(ctx, in, n, where, &d_in);
    if (rc) return rc;
    rc = mrz_rs_need_tables(ctx);
    if (rc) return rc;
    const int64_t rows = nbursts * MRZ_RS_ROWS, produced_all = rows * MRZ_RS_K;
    uint8_t *d_out = (uint8_t *)out;
    if (out_where == MRZ_MEM_HOST) {
        rc = mrz_grow(ctx, &ctx->d_rs_out, &ctx->rs_out_cap, produced_all);
        if (rc) return rc;
        d_out = ctx->d_rs_out;
    }
    // scratch: totals and list length, one status per row (unless the caller's array is device memory), the list
    const int64_t head_bytes = 64;
    rc = mrz_grow(ctx, &ctx->d_rs_dec, &ctx->rs_dec_cap, head_bytes + rows * 4 + rows * (int64_t)sizeof(mrz_rsd_entry));
    if (rc) return rc;
    mrz_rsd_head *d_head = (mrz_rsd_head *)ctx->d_rs_dec;
    int *d_counts = (int *)(ctx->d_rs_dec + head_bytes);
    mrz_rsd_entry *d_list = (mrz_rsd_entry *)(ctx->d_rs_dec + head_bytes + rows * 4);
    if (row_status && status_where == MRZ_MEM_DEVICE) d_counts = row_status;
    if (n_lost > 0) {  // the sorted ranges, for the repair kernel's search
        rc = mrz_grow(ctx, &ctx->d_rs_lost, &ctx->rs_lost_cap, n_lost);
        if (rc) return rc;
    }
    int cus = 0;
    HIPCHK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    if (cus < 1) cus = 1;

    const bool has_trailer = tail == 64 + 4, hash = has_trailer && !(flags & MRZ_RS_SKIP_CHECKSUM);
    uint8_t trailer[68];
    mrz_rsd_head h_head;
    std::vector<uint8_t> hash_copy;  // device output: the rows come to the host to be hashed
    if (hash && out_where == MRZ_MEM_DEVICE) hash_copy.resize((size_t)produced_all);
    hipError_t e = hipMemsetAsync(d_head, 0, sizeof(mrz_rsd_head), ctx->stream);
    if (e == hipSuccess && n_lost > 0)
        e = hipMemcpyAsync(ctx->d_rs_lost, lost, (size_t)n_lost * sizeof(mrz_rs_range), hipMemcpyHostToDevice, ctx->stream);
    hipEvent_t ea = nullptr, eb = nullptr;
    if (ctx->profiling) {
        hipEventCreate(&ea);
        hipEventCreate(&eb);
        hipEventRecord(ea, ctx->stream);
    }
    if (e == hipSuccess) {
        const int tiles = (MRZ_RS_ROWS + MRZ_RSD_ROWS - 1) / MRZ_RSD_ROWS;
        hipLaunchKernelGGL(mrz_rs_decode_kernel, dim3((unsigned)(nbursts * tiles)), dim3(MRZ_RSD_ROWS), 0, ctx->stream, d_in,
                           (const mrz_rs_tables *)ctx->d_rs_tables, d_out, d_counts, d_head, d_list);
        if (n_lost > 0)
            hipLaunchKernelGGL(mrz_rs_repair_kernel<true>, dim3((unsigned)(cus * MRZ_RSR_WGS_PER_CU)), dim3(MRZ_RSR_THREADS),
                               0, ctx->stream, (const mrz_rs_tables *)ctx->d_rs_tables, (const mrz_rsd_entry *)d_list, d_head,
                               d_out, d_counts, (const mrz_rs_range *)ctx->d_rs_lost, n_lost);
        else
            hipLaunchKernelGGL(mrz_rs_repair_kernel<false>, dim3((unsigned)(cus * MRZ_RSR_WGS_PER_CU)), dim3(MRZ_RSR_THREADS),
                               0, ctx->stream, (const mrz_rs_tables *)ctx->d_rs_tables, (const mrz_rsd_entry *)d_list, d_head,
                               d_out, d_counts, (const mrz_rs_range *)nullptr, (int64_t)0);
        e = hipGetLastError();
    }
    if (ctx->profiling) hipEventRecord(eb, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_head, d_head, sizeof(h_head), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && out_where == MRZ_MEM_HOST)
        e = hipMemcpyAsync(out, d_out, (size_t)produced_all, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && hash && out_where == MRZ_MEM_DEVICE)
        e = hipMemcpyAsync(hash_copy.data(), d_out, (size_t)produced_all, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && row_status && status_where == MRZ_MEM_HOST)
        e = hipMemcpyAsync(row_status, d_counts, (size_t)rows * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && has_trailer) {
        if (where == MRZ_MEM_HOST)
            memcpy(trailer, (const uint8_t *)in + nbursts * burst_out, 68);
        else
            e = hipMemcpyAsync(trailer, (const uint8_t *)in + nbursts * burst_out, 68, hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t e_sync = hipStreamSynchronize(ctx->stream);  // the call's one wait
    if (e == hipSuccess) e = e_sync;
    if (ctx->profiling) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ea, eb) == hipSuccess) ctx->timings.encode_ms = ms;  // reported via mrz_get_timings
        hipEventDestroy(ea);
        hipEventDestroy(eb);
    }
    if (e != hipSuccess) {
        ctx->last_err = e;
        return MRZ_E_HIP;
    }
    mrz_rs_report r;
    memset(&r, 0, sizeof(r));
    r.corrected = (int64_t)h_head.corrected;  // rs-mrzip.c:103-108
    r.uncorrectable = (int64_t)h_head.uncorrectable;
    int64_t produced = produced_all;
    if (has_trailer) {
        // trailer: BLAKE2b-512 of every 223-byte row as decoded, then the first short row and its length (:70-95)
        if (hash) {
            uint8_t digest[64];
            HostB2 b;
            b.update(out_where == MRZ_MEM_HOST ? (const uint8_t *)out : hash_copy.data(), (size_t)produced_all);
            b.final(digest);
            r.checksum_ok = memcmp(digest, trailer, 64) == 0;
        }
        const int64_t k_i = trailer[64] | trailer[65] << 8, k_j = trailer[66] | trailer[67] << 8;
        if (k_i < MRZ_RS_ROWS) {
            const int64_t cut = (nbursts - 1) * burst_in + k_i * MRZ_RS_K + (k_j < MRZ_RS_K ? k_j : MRZ_RS_K);
            if (cut < produced) produced = cut;
        }
    } else
        r.truncated = 1;  // "file truncated. can't validate the checksum or remove superfluous 0x00 padding" (:58-68)
    if (flags & MRZ_RS_SKIP_CHECKSUM) r.checksum_ok = -1;
    *out_len = produced;
    if (rep) *rep = r;
    return MRZ_OK;
}

extern "C" int mrz_rs_decode_ex(mrz_ctx *ctx, const void *in, int64_t n, int where, void *out, int out_where,
                                int64_t out_cap, int64_t *out_len, int32_t *row_status, int status_where, int flags,
                                mrz_rs_report *rep) {
    return mrz_rs_decode_impl(ctx, in, n, where, out, out_where, out_cap, out_len, nullptr, 0, row_status, status_where,
                              flags, rep);
}

extern "C" int mrz_rs_decode_lost(mrz_ctx *ctx, const void *in, int64_t n, int where, void *out, int out_where,
                                  int64_t out_cap, int64_t *out_len, const mrz_rs_range *lost, int64_t n_lost,
                                  int32_t *row_status, int status_where, int flags, mrz_rs_report *rep) {
    if (n_lost < 0 || (n_lost > 0 && !lost) || n < 0) return MRZ_E_ARG;
    int64_t end = 0;  // of the range before: ascending and disjoint (adjacent is allowed)
    for (int64_t i = 0; i < n_lost; i++) {
        if (lost[i].len <= 0 || lost[i].offset < end || lost[i].len > n - lost[i].offset) return MRZ_E_ARG;
        end = lost[i].offset + lost[i].len;
    }
    return mrz_rs_decode_impl(ctx, in, n, where, out, out_where, out_cap, out_len, lost, n_lost, row_status, status_where,
                              flags, rep);
}

extern "C" int mrz_rs_decode(mrz_ctx *ctx, const void *in, int64_t n, int where, void *out_host, int64_t out_cap,
                             int64_t *out_len, mrz_rs_report *rep) {
    return mrz_rs_decode_ex(ctx, in, n, where, out_host, MRZ_MEM_HOST, out_cap, out_len, nullptr, MRZ_MEM_HOST, 0, rep);
}
