// mrz_synth.hip -- the reproducible workload streams of include/mrzgpu_synth.h (noise, Zipf text, the S3 tar mix), built
// in HBM at any size and for any byte range.  The definition is in that header; the host reference is
// modern_rzip_amd/workloads.py (synth_*), with which every byte must agree.  Set-up code, not timed path: it exists so
// that inputs of tens of GiB have bytes a test can pin.
//
// Kernels
//   mrz_synth_fill_kernel      noise and zero padding.  One workgroup per work item (a piece of at most 1 MiB of one
//                              member); a lane writes one 16-byte aligned group per store (64 lanes = 1 KiB per wave
//                              instruction), the groups that straddle the piece's ends byte by byte.  16 output bytes
//                              are two draws of rnd (three where the piece's stream offset is not a multiple of 8).
//                              Bound: HBM writes.
//   mrz_synth_text_len_kernel  pass 1 of text.  A text member is cut into tiles of MRZ_SYN_TILE_WORDS words; a tile's
//                              byte length is not known before its words are drawn.  The cumulative Zipf table and the
//                              word lengths (25 KB) sit in LDS; a lane draws 4 words (a 13-step binary search each),
//                              the workgroup reduces the lengths.  Persistent grid over the tiles of all members.
//   mrz_synth_text_scan_kernel exclusive scan of the tile lengths of one member per workgroup: a tile's byte offset.
//   mrz_synth_text_put_kernel  pass 2.  Redraws the ranks (cheaper than storing them), scans the lengths inside the
//                              workgroup, assembles the tile's bytes in an LDS stage (the word table, 50 KB, is in LDS
//                              too) and writes the stage out in aligned 16-byte stores.  The stage is shifted by the
//                              low 4 bits of the tile's first global address, so an aligned LDS group is an aligned
//                              global group.  Tiles that begin beyond the member's (clipped) end are skipped: the number
//                              of tiles is bounded by size / 3 words (the shortest word and its separator).
// A member that begins before the requested range has its tile lengths computed from its own beginning; only its bytes
// are clipped.  Duplicates are ordinary members (regenerated), so there is no device-to-device copy pass.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/mrzgpu_synth.h"
#include "mrz_ctx.h"
#include "mrz_device.h"

#define MRZ_SYN_G 0x9E3779B97F4A7C15ull
#define MRZ_SYN_M1 0xBF58476D1CE4E5B9ull
#define MRZ_SYN_M2 0x94D049BB133111EBull
enum { MRZ_SYN_NOISE = 0, MRZ_SYN_WORD = 1, MRZ_SYN_VLEN = 2, MRZ_SYN_VCHAR = 3 };

#define MRZ_SYN_VOCAB 5000
#define MRZ_SYN_ZIPF_TOTAL 2441286195u  // cum[4999]; a constant, so the draw's modulo is a multiply
#define MRZ_SYN_NEWLINE 20000
#define MRZ_SYN_MAX_WORD 10

#define MRZ_SYN_FILL_THREADS 256
#define MRZ_SYN_PIECE (1ll << 20)  // bytes per fill work item at most

#define MRZ_SYN_THREADS 512
#define MRZ_SYN_WPT 4  // words per lane and tile
#define MRZ_SYN_TILE_WORDS (MRZ_SYN_THREADS * MRZ_SYN_WPT)
#define MRZ_SYN_STAGE (MRZ_SYN_TILE_WORDS * (MRZ_SYN_MAX_WORD + 1) + 16)
#define MRZ_SYN_SCAN_THREADS 256

__host__ __device__ static inline uint64_t mrz_syn_mix(uint64_t z) {
    z ^= z >> 30;
    z *= MRZ_SYN_M1;
    z ^= z >> 27;
    z *= MRZ_SYN_M2;
    return z ^ (z >> 31);
}
__host__ __device__ static inline uint64_t mrz_syn_key(uint64_t seed, unsigned stream) {
    return mrz_syn_mix(seed + MRZ_SYN_G * (uint64_t)(stream + 1));
}
// rnd(seed, stream, i) with key = mrz_syn_key(seed, stream)
__host__ __device__ static inline uint64_t mrz_syn_draw(uint64_t key, uint64_t i) {
    return mrz_syn_mix(key + MRZ_SYN_G * (i + 1));
}

// ---- noise and zeros ---------------------------------------------------------------------------------------------------

struct mrz_syn_fill_item {
    int64_t dst;   // offset in the output buffer
    int64_t j0;    // offset of the piece in its noise stream
    int64_t n;     // bytes (1 .. MRZ_SYN_PIECE)
    uint64_t key;  // key(seed, NOISE)
    int64_t zero;  // != 0: the piece is zeros
};

__device__ __forceinline__ uint8_t mrz_syn_noise_byte(uint64_t key, int64_t j) {
    return (uint8_t)(mrz_syn_draw(key, (uint64_t)j >> 3) >> (8 * (int)(j & 7)));
}

__global__ __launch_bounds__(MRZ_SYN_FILL_THREADS) void mrz_synth_fill_kernel(uint8_t *__restrict__ out,
                                                                              const mrz_syn_fill_item *__restrict__ items) {
    const mrz_syn_fill_item it = items[blockIdx.x];
    uint8_t *p = out + it.dst;
    // 16-byte groups by global address: group g covers piece bytes [16 g - shift, 16 g - shift + 16)
    const int shift = (int)((uintptr_t)p & 15);
    const int64_t groups = (it.n + shift + 15) >> 4;
    const int sh = 8 * (int)((it.j0 - shift) & 7);  // the same for every group: they are 16 bytes apart
    for (int64_t g = threadIdx.x; g < groups; g += MRZ_SYN_FILL_THREADS) {
        const int64_t b = g * 16 - shift;  // piece offset of the group's first byte (< 0 in the first group if shifted)
        if (b >= 0 && b + 16 <= it.n) {
            uint64_t lo = 0, hi = 0;
            if (!it.zero) {
                const uint64_t w = (uint64_t)(it.j0 + b) >> 3;
                const uint64_t w0 = mrz_syn_draw(it.key, w), w1 = mrz_syn_draw(it.key, w + 1);
                if (sh) {
                    const uint64_t w2 = mrz_syn_draw(it.key, w + 2);
                    lo = (w0 >> sh) | (w1 << (64 - sh));
                    hi = (w1 >> sh) | (w2 << (64 - sh));
                } else {
                    lo = w0;
                    hi = w1;
                }
            }
            *(uint4 *)(p + b) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        } else {
            const int64_t b0 = b < 0 ? 0 : b, b1 = b + 16 < it.n ? b + 16 : it.n;
            for (int64_t k = b0; k < b1; k++) p[k] = it.zero ? (uint8_t)0 : mrz_syn_noise_byte(it.key, it.j0 + k);
        }
    }
}

// ---- text --------------------------------------------------------------------------------------------------------------

struct alignas(16) mrz_syn_ranks {
    uint32_t cum[MRZ_SYN_VOCAB];
    uint8_t wlen[MRZ_SYN_VOCAB + 8];  // (+8: the struct stays a multiple of 16 bytes)
};
struct alignas(16) mrz_syn_tables {
    mrz_syn_ranks r;
    uint8_t words[MRZ_SYN_VOCAB * MRZ_SYN_MAX_WORD];  // word w at 10 w
};
static_assert(sizeof(mrz_syn_ranks) % 16 == 0 && sizeof(mrz_syn_tables) % 16 == 0, "copied as 16-byte pieces");

struct mrz_syn_text_member {
    int64_t dst;    // offset of the member's byte 0 in the output buffer (negative if it begins before the range)
    int64_t lo, hi; // the member's bytes [lo, hi) are wanted
    uint64_t key;   // key(seed, WORD)
    int64_t tile0;  // index of its first tile in the tile arrays (ascending; one sentinel entry closes the list)
};

__device__ __forceinline__ void mrz_syn_load_lds(void *lds, const void *glob, int bytes) {
    for (int i = threadIdx.x; i < bytes / 16; i += blockDim.x) ((uint4 *)lds)[i] = ((const uint4 *)glob)[i];
}

// rank of word k: the first r with cum[r] > rnd % cum[4999]
__device__ __forceinline__ int mrz_syn_rank(const uint32_t *cum, uint64_t key, int64_t k) {
    const uint32_t u = (uint32_t)(mrz_syn_draw(key, (uint64_t)k) % MRZ_SYN_ZIPF_TOTAL);
    int lo = 0, hi = MRZ_SYN_VOCAB - 1;
#pragma unroll
    for (int s = 0; s < 13; s++) {  // 2^13 > 5000; once lo == hi the step changes nothing
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > u) hi = mid; else lo = mid + 1;
    }
    return hi;
}

// the member that owns tile `item`: the last m with mem[m].tile0 <= item (workgroup-uniform)
__device__ __forceinline__ int mrz_syn_find_member(const mrz_syn_text_member *mem, int n_mem, int64_t item) {
    int lo = 0, hi = n_mem - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mem[mid].tile0 <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// exclusive prefix of v over the workgroup (blockDim.x / 64 waves, wsum has one entry per wave) and the total.
// Ends with every lane past its reads of wsum only after the caller's next __syncthreads.
__device__ __forceinline__ int mrz_syn_block_excl(int v, int *wsum, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int incl = mrz_wave_incl_sum(v, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < nw; w++) {
        const int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + incl - v;
}

__global__ __launch_bounds__(MRZ_SYN_THREADS) void mrz_synth_text_len_kernel(const mrz_syn_tables *__restrict__ tb,
                                                                             const mrz_syn_text_member *__restrict__ mem,
                                                                             int n_mem, int64_t n_items,
                                                                             int *__restrict__ tile_len) {
    __shared__ mrz_syn_ranks R;
    __shared__ int wsum[MRZ_SYN_THREADS / 64];
    mrz_syn_load_lds(&R, &tb->r, (int)sizeof(R));
    __syncthreads();
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int m = mrz_syn_find_member(mem, n_mem, item);
        const uint64_t key = mem[m].key;
        const int64_t k0 = (item - mem[m].tile0) * MRZ_SYN_TILE_WORDS + (int64_t)threadIdx.x * MRZ_SYN_WPT;
        int sum = 0;
#pragma unroll
        for (int i = 0; i < MRZ_SYN_WPT; i++) sum += R.wlen[mrz_syn_rank(R.cum, key, k0 + i)] + 1;
        int total;
        mrz_syn_block_excl(sum, wsum, &total);
        if (threadIdx.x == 0) tile_len[item] = total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(MRZ_SYN_SCAN_THREADS) void mrz_synth_text_scan_kernel(const mrz_syn_text_member *__restrict__ mem,
                                                                                   const int *__restrict__ tile_len,
                                                                                   int64_t *__restrict__ tile_off) {
    __shared__ int wsum[MRZ_SYN_SCAN_THREADS / 64];
    const int64_t t0 = mem[blockIdx.x].tile0, nt = mem[blockIdx.x + 1].tile0 - t0;
    int64_t carry = 0;
    for (int64_t c = 0; c < nt; c += MRZ_SYN_SCAN_THREADS) {
        const int64_t t = c + threadIdx.x;
        const int v = t < nt ? tile_len[t0 + t] : 0;
        int total;
        const int excl = mrz_syn_block_excl(v, wsum, &total);
        if (t < nt) tile_off[t0 + t] = carry + excl;
        carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(MRZ_SYN_THREADS) void mrz_synth_text_put_kernel(uint8_t *__restrict__ out,
                                                                             const mrz_syn_tables *__restrict__ tb,
                                                                             const mrz_syn_text_member *__restrict__ mem,
                                                                             int n_mem, int64_t n_items,
                                                                             const int *__restrict__ tile_len,
                                                                             const int64_t *__restrict__ tile_off) {
    __shared__ mrz_syn_tables T;
    __shared__ __attribute__((aligned(16))) uint8_t stage[MRZ_SYN_STAGE];
    __shared__ int wsum[MRZ_SYN_THREADS / 64];
    mrz_syn_load_lds(&T, tb, (int)sizeof(T));
    __syncthreads();
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int m = mrz_syn_find_member(mem, n_mem, item);
        const int64_t off = tile_off[item];  // of the tile's first byte in the member
        const int tlen = tile_len[item];
        const int64_t mlo = mem[m].lo, mhi = mem[m].hi;
        if (off >= mhi || off + tlen <= mlo) continue;  // (workgroup-uniform)
        const uint64_t key = mem[m].key;
        const int64_t k0 = (item - mem[m].tile0) * MRZ_SYN_TILE_WORDS + (int64_t)threadIdx.x * MRZ_SYN_WPT;
        int rank[MRZ_SYN_WPT], sum = 0;
#pragma unroll
        for (int i = 0; i < MRZ_SYN_WPT; i++) {
            rank[i] = mrz_syn_rank(T.r.cum, key, k0 + i);
            sum += T.r.wlen[rank[i]] + 1;
        }
        int total;
        int at = mrz_syn_block_excl(sum, wsum, &total);
        // stage index = tile byte + shift, so that stage and global address agree in their low 4 bits
        uint8_t *g0 = out + (mem[m].dst + off);  // global address of tile byte 0 (never dereferenced outside [lo, hi))
        const int shift = (int)((uintptr_t)g0 & 15);
        at += shift;
#pragma unroll
        for (int i = 0; i < MRZ_SYN_WPT; i++) {
            const int n = T.r.wlen[rank[i]];
            const uint8_t *w = T.words + rank[i] * MRZ_SYN_MAX_WORD;
            for (int c = 0; c < n; c++) stage[at + c] = w[c];
            stage[at + n] = (k0 + i + 1) % MRZ_SYN_NEWLINE == 0 ? (uint8_t)'\n' : (uint8_t)' ';
            at += n + 1;
        }
        __syncthreads();
        // tile bytes [jlo, jhi) are wanted; stage bytes [s0, s1)
        const int jlo = mlo > off ? (int)(mlo - off) : 0;
        const int jhi = mhi - off < (int64_t)tlen ? (int)(mhi - off) : tlen;
        const int s0 = jlo + shift, s1 = jhi + shift;
        uint8_t *gs = g0 - shift;  // global address of stage byte 0: 16-byte aligned
        for (int s = (s0 & ~15) + 16 * (int)threadIdx.x; s < s1; s += 16 * MRZ_SYN_THREADS) {
            if (s >= s0 && s + 16 <= s1) {
                *(uint4 *)(gs + s) = *(const uint4 *)(stage + s);
            } else {
                const int a = s < s0 ? s0 : s, b = s + 16 < s1 ? s + 16 : s1;
                for (int k = a; k < b; k++) gs[k] = stage[k];
            }
        }
        __syncthreads();
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

static void mrz_syn_build_tables(mrz_syn_tables *tb, uint64_t vocab_seed) {
    memset(tb, 0, sizeof(*tb));
    uint64_t c = 0;
    for (int r = 0; r < MRZ_SYN_VOCAB; r++) tb->r.cum[r] = (uint32_t)(c += (1ull << 28) / (uint64_t)(r + 1));
    const uint64_t kl = mrz_syn_key(vocab_seed, MRZ_SYN_VLEN), kc = mrz_syn_key(vocab_seed, MRZ_SYN_VCHAR);
    for (int w = 0; w < MRZ_SYN_VOCAB; w++) {
        tb->r.wlen[w] = (uint8_t)(2 + mrz_syn_draw(kl, (uint64_t)w) % 9);
        for (int k = 0; k < MRZ_SYN_MAX_WORD; k++)
            tb->words[w * MRZ_SYN_MAX_WORD + k] = (uint8_t)('a' + mrz_syn_draw(kc, (uint64_t)(w * MRZ_SYN_MAX_WORD + k)) % 26);
    }
}

struct mrz_syn_dev {  // device allocations of one call, freed on every way out
    void *p[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    mrz_syn_dev() {}
    mrz_syn_dev(const mrz_syn_dev &) = delete;  // (a launch must name plain pointers, never a member of this)
    ~mrz_syn_dev() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
};

static int mrz_syn_upload(mrz_ctx *ctx, void **d, const void *h, size_t bytes) {
    if (hipMalloc(d, bytes) != hipSuccess) return MRZ_E_NOMEM;
    HIPCHK(ctx, hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return MRZ_OK;
}

static void mrz_syn_add_fill(std::vector<mrz_syn_fill_item> &items, int64_t dst, int64_t j0, int64_t n, uint64_t key,
                             int zero) {
    for (int64_t a = 0; a < n; a += MRZ_SYN_PIECE) {
        const int64_t k = n - a < MRZ_SYN_PIECE ? n - a : MRZ_SYN_PIECE;
        items.push_back({ dst + a, j0 + a, k, key, zero });
    }
}

// launches the fill items and the text members (tile0 not yet set) on the ctx stream and waits for them
static int mrz_syn_run(mrz_ctx *ctx, uint8_t *out, std::vector<mrz_syn_fill_item> &fill,
                       std::vector<mrz_syn_text_member> &text, uint64_t vocab_seed) {
    mrz_syn_dev dev;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!fill.empty()) {
        if (fill.size() > 0x7fffffffull) return MRZ_E_OVERFLOW;
        const int rc = mrz_syn_upload(ctx, &dev.p[0], fill.data(), fill.size() * sizeof(fill[0]));
        if (rc) return rc;
        const mrz_syn_fill_item *d_items = (const mrz_syn_fill_item *)dev.p[0];
        hipLaunchKernelGGL(mrz_synth_fill_kernel, dim3((unsigned)fill.size()), dim3(MRZ_SYN_FILL_THREADS), 0, ctx->stream,
                           out, d_items);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!text.empty()) {
        if (text.size() > 0x7ffffff0ull) return MRZ_E_OVERFLOW;
        int64_t tiles = 0;
        for (auto &t : text) {
            t.tile0 = tiles;
            const int64_t words = (t.hi + 2) / 3;  // words that can begin before byte hi
            tiles += (words + MRZ_SYN_TILE_WORDS - 1) / MRZ_SYN_TILE_WORDS;
        }
        const int n_mem = (int)text.size();
        text.push_back({ 0, 0, 0, 0, tiles });  // sentinel
        mrz_syn_tables *tb = (mrz_syn_tables *)malloc(sizeof(mrz_syn_tables));
        if (!tb) return MRZ_E_NOMEM;
        mrz_syn_build_tables(tb, vocab_seed);
        const bool tables_ok = tb->r.cum[MRZ_SYN_VOCAB - 1] == MRZ_SYN_ZIPF_TOTAL;
        int rc = tables_ok ? mrz_syn_upload(ctx, &dev.p[1], tb, sizeof(*tb)) : MRZ_E_OVERFLOW;
        if (!rc) rc = mrz_syn_upload(ctx, &dev.p[2], text.data(), text.size() * sizeof(text[0]));
        if (!rc) rc = mrz_synchronize(ctx);  // (tb is read by the copy until here)
        free(tb);
        if (rc) return rc;
        if (hipMalloc(&dev.p[3], (size_t)tiles * sizeof(int)) != hipSuccess) return MRZ_E_NOMEM;
        if (hipMalloc(&dev.p[4], (size_t)tiles * sizeof(int64_t)) != hipSuccess) return MRZ_E_NOMEM;
        int cus = 0;
        HIPCHK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        if (cus < 1) cus = 1;
        const mrz_syn_tables *d_tb = (const mrz_syn_tables *)dev.p[1];
        const mrz_syn_text_member *d_mem = (const mrz_syn_text_member *)dev.p[2];
        int *d_len = (int *)dev.p[3];
        int64_t *d_off = (int64_t *)dev.p[4];
        // pass 1 holds 25 KB of LDS (4 workgroups of 8 waves fill a CU), pass 2 about 97 KB (one per CU)
        const int64_t g1 = tiles < 4ll * cus ? tiles : 4ll * cus, g2 = tiles < cus ? tiles : cus;
        hipLaunchKernelGGL(mrz_synth_text_len_kernel, dim3((unsigned)g1), dim3(MRZ_SYN_THREADS), 0, ctx->stream, d_tb, d_mem,
                           n_mem, tiles, d_len);
        hipLaunchKernelGGL(mrz_synth_text_scan_kernel, dim3((unsigned)n_mem), dim3(MRZ_SYN_SCAN_THREADS), 0, ctx->stream,
                           d_mem, (const int *)d_len, d_off);
        hipLaunchKernelGGL(mrz_synth_text_put_kernel, dim3((unsigned)g2), dim3(MRZ_SYN_THREADS), 0, ctx->stream, out, d_tb,
                           d_mem, n_mem, tiles, (const int *)d_len, (const int64_t *)d_off);
        HIPCHK(ctx, hipGetLastError());
    }
    return mrz_synchronize(ctx);
}

extern "C" int mrz_synth_noise(mrz_ctx *ctx, void *d_out, int64_t start, int64_t len, uint64_t seed) {
    if (!ctx || start < 0 || len < 0 || start > INT64_MAX - len || (len > 0 && !d_out)) return MRZ_E_ARG;
    if (!len) return MRZ_OK;
    std::vector<mrz_syn_fill_item> fill;
    std::vector<mrz_syn_text_member> text;
    mrz_syn_add_fill(fill, 0, start, len, mrz_syn_key(seed, MRZ_SYN_NOISE), 0);
    return mrz_syn_run(ctx, (uint8_t *)d_out, fill, text, 0);
}

extern "C" int mrz_synth_text(mrz_ctx *ctx, void *d_out, int64_t len, uint64_t seed, uint64_t vocab_seed) {
    if (!ctx || len < 0 || (len > 0 && !d_out)) return MRZ_E_ARG;
    if (!len) return MRZ_OK;
    std::vector<mrz_syn_fill_item> fill;
    std::vector<mrz_syn_text_member> text;
    text.push_back({ 0, 0, len, mrz_syn_key(seed, MRZ_SYN_WORD), 0 });
    return mrz_syn_run(ctx, (uint8_t *)d_out, fill, text, vocab_seed);
}

extern "C" int mrz_synth_tar(mrz_ctx *ctx, void *d_out, int64_t start, int64_t len, const mrz_synth_member *plan,
                             int64_t n_members, uint64_t vocab_seed) {
    if (!ctx || start < 0 || len < 0 || start > INT64_MAX - len || n_members < 0 || (len > 0 && (!d_out || !plan)))
        return MRZ_E_ARG;
    if (!len) return MRZ_OK;
    const int64_t end = start + len;
    int64_t prev_end = 0;
    for (int64_t i = 0; i < n_members; i++) {
        const mrz_synth_member &d = plan[i];
        if (d.dst < prev_end || d.size <= 0 || d.dst > INT64_MAX - d.size - 512) return MRZ_E_ARG;
        if (d.kind != MRZ_SYNTH_TEXT && d.kind != MRZ_SYNTH_NOISE) return MRZ_E_ARG;
        prev_end = d.dst + d.size;
    }
    if (!n_members || end > ((prev_end + 511) & ~511ll)) return MRZ_E_ARG;
    std::vector<mrz_syn_fill_item> fill;
    std::vector<mrz_syn_text_member> text;
    int64_t at = start;  // bytes before `at` are accounted for
    for (int64_t i = 0; i < n_members && at < end; i++) {
        const mrz_synth_member &d = plan[i];
        if (d.dst + d.size <= start) continue;
        if (d.dst >= end) break;
        if (d.dst > at) mrz_syn_add_fill(fill, at - start, 0, d.dst - at, 0, 1);  // padding in front of the member
        const int64_t lo = start > d.dst ? start - d.dst : 0;                    // the member's bytes [lo, hi)
        const int64_t hi = end - d.dst < d.size ? end - d.dst : d.size;
        if (d.kind == MRZ_SYNTH_NOISE)
            mrz_syn_add_fill(fill, d.dst + lo - start, lo, hi - lo, mrz_syn_key(d.seed, MRZ_SYN_NOISE), 0);
        else
            text.push_back({ d.dst - start, lo, hi, mrz_syn_key(d.seed, MRZ_SYN_WORD), 0 });
        at = d.dst + hi;
    }
    if (at < end) mrz_syn_add_fill(fill, at - start, 0, end - at, 0, 1);
    return mrz_syn_run(ctx, (uint8_t *)d_out, fill, text, vocab_seed);
}
