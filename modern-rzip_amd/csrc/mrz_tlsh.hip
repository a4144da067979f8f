// mrz_tlsh.hip -- the index half of ar-mrzip on the device: the TLSH digest of every member (compute_checksums,
// ar-mrzip/ar-mrzip.cpp:137-172, with vendor/tlsh built for 256 buckets and 3 checksum bytes) and the greedy
// similarity order (:408-437).  DESIGN.md section 4.10.
//
// A digest has two parts with different shapes:
//   * the bucket counts: every byte i >= 4 of a message makes six increments, each a function of bytes i-4..i alone.
//     Order does not matter, so the grid runs over (member, segment): a workgroup counts its segment in an LDS
//     histogram and adds it to the member's 256 counters with global atomics.  The window reads its 4 bytes of halo
//     straight from the previous segment.
//   * three checksum bytes, each a chain of dependent table look-ups over the whole message, chain k salted with the
//     new value of chain k-1.  Once chain k-1 is known at every byte, chain k is a 256-state automaton whose step
//     depends on the data only; a wave carries all 256 states through its segment (4 per lane) and leaves the segment's
//     map 256 -> 256.  A small kernel composes the maps of a member in order, which gives chain k at every segment
//     start; the pass for chain k+1 walks chain k from there as a wave-uniform value.  Three passes, sequenced by
//     launches on the ctx stream; no workgroup waits for another.
// The finish kernel (one wave per member) takes the three quartiles by rank counting and packs the code bytes; the
// length code, the ratios (float operations of the host, as in the reference) and the hex string are host work
// (mrz_tlsh_tables.h).
// Bound: LDS look-ups -- 18 per byte for the counts (random bytes of a 256-byte table: bank conflicts between the 32
// lanes of a group are the norm), 4 per byte and lane plus up to 8 dependent wave-uniform ones for a chain pass.
#include <string.h>

#include <vector>

#include "mrz_ctx.h"
#include "mrz_device.h"
#include "mrz_tlsh_tables.h"

__device__ static const uint8_t k_tlsh_pearson[256] = { MRZ_TLSH_PEARSON_ROWS };

// the member that owns segment `seg`: the last one whose first segment is not behind it (members without segments
// share their successor's first segment and are never chosen)
__device__ static int mrz_tlsh_member(const int64_t *__restrict__ seg_first, int count, int64_t seg) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_first[mid] <= seg)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// ---- bucket counts -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mrz_tlsh_hist_kernel(const uint8_t *const *__restrict__ msgs,
                                                            const int64_t *__restrict__ lens,
                                                            const int64_t *__restrict__ seg_first, int count, int64_t S,
                                                            unsigned *__restrict__ counts) {
    __shared__ uint8_t v[256];
    __shared__ unsigned hist[256];
    const int t = threadIdx.x;
    v[t] = k_tlsh_pearson[t];
    hist[t] = 0;
    __syncthreads();
    const int64_t seg = blockIdx.x;
    const int m = mrz_tlsh_member(seg_first, count, seg);
    const uint8_t *__restrict__ d = msgs[m];
    const int64_t lo = (seg - seg_first[m]) * S;
    const int64_t hi = lo + S < lens[m] ? lo + S : lens[m];
    for (int64_t p = lo + t; p < hi; p += 256) {
        if (p < 4) continue;
        const unsigned b0 = d[p], b1 = d[p - 1], b2 = d[p - 2], b3 = d[p - 3], b4 = d[p - 4];
        atomicAdd(&hist[v[v[v[MRZ_TLSH_SALT_A ^ b0] ^ b1] ^ b2]], 1u);
        atomicAdd(&hist[v[v[v[MRZ_TLSH_SALT_B ^ b0] ^ b1] ^ b3]], 1u);
        atomicAdd(&hist[v[v[v[MRZ_TLSH_SALT_C ^ b0] ^ b2] ^ b3]], 1u);
        atomicAdd(&hist[v[v[v[MRZ_TLSH_SALT_D ^ b0] ^ b2] ^ b4]], 1u);
        atomicAdd(&hist[v[v[v[MRZ_TLSH_SALT_E ^ b0] ^ b1] ^ b4]], 1u);
        atomicAdd(&hist[v[v[v[MRZ_TLSH_SALT_F ^ b0] ^ b3] ^ b4]], 1u);
    }
    __syncthreads();
    if (hist[t]) atomicAdd(&counts[(int64_t)m * 256 + t], hist[t]);
}

// ---- checksum chains ---------------------------------------------------------------------------------------------
// Pass K: the map of chain K over one segment.  starts[seg * 4 + j]: chain j < K at the segment's first byte.
template <int K>
__global__ __launch_bounds__(64) void mrz_tlsh_chain_kernel(const uint8_t *const *__restrict__ msgs,
                                                            const int64_t *__restrict__ lens,
                                                            const int64_t *__restrict__ seg_first, int count, int64_t S,
                                                            const uint8_t *__restrict__ starts,
                                                            uint32_t *__restrict__ maps) {
    __shared__ uint8_t v[256];
    __shared__ uint32_t stage[256];  // per byte of a 256-byte piece: chain 0's data term | d[i] << 8 | d[i-1] << 16
    const int lane = threadIdx.x;
    for (int j = 0; j < 4; j++) v[4 * lane + j] = k_tlsh_pearson[4 * lane + j];
    __syncthreads();
    const int64_t seg = blockIdx.x;
    const int m = mrz_tlsh_member(seg_first, count, seg);
    const uint8_t *__restrict__ d = msgs[m];
    const int64_t lo = (seg - seg_first[m]) * S;
    const int64_t hi = lo + S < lens[m] ? lo + S : lens[m];
    unsigned c0 = K >= 1 ? starts[seg * 4 + 0] : 0u;
    unsigned c1 = K >= 2 ? starts[seg * 4 + 1] : 0u;
    unsigned x0 = 4 * lane, x1 = 4 * lane + 1, x2 = 4 * lane + 2, x3 = 4 * lane + 3;
    for (int64_t base = lo; base < hi; base += 256) {
        for (int r = 0; r < 4; r++) {
            const int64_t p = base + 64 * r + lane;
            uint32_t pk = 0;
            if (p >= 4 && p < hi) {
                const unsigned di = d[p], dj = d[p - 1];
                pk = v[v[1u ^ di] ^ dj] | (di << 8) | (dj << 16);
            }
            stage[64 * r + lane] = pk;
        }
        __syncthreads();
        const int n = hi - base < 256 ? (int)(hi - base) : 256;
        for (int j = base < 4 ? (int)(4 - base) : 0; j < n; j++) {
            const uint32_t pk = stage[j];
            unsigned a = pk & 255u;
            if (K >= 1) {
                const unsigned di = (pk >> 8) & 255u, dj = (pk >> 16) & 255u;
                c0 = v[a ^ c0];
                a = v[v[v[c0] ^ di] ^ dj];
                if (K >= 2) {
                    c1 = v[a ^ c1];
                    a = v[v[v[c1] ^ di] ^ dj];
                }
            }
            x0 = v[a ^ x0];
            x1 = v[a ^ x1];
            x2 = v[a ^ x2];
            x3 = v[a ^ x3];
        }
        __syncthreads();
    }
    maps[seg * 64 + lane] = x0 | (x1 << 8) | (x2 << 16) | (x3 << 24);
}

// One wave per member composes the maps of pass k in segment order: starts[seg * 4 + k] = chain k at the segment's
// first byte, finals[m * 4 + k] = the chain at the end.  The rows (256 bytes, one dword per lane) are loaded eight ahead
// of the walk, so the dependent part of a step is a lane read, not a memory access.
__global__ __launch_bounds__(64) void mrz_tlsh_compose_kernel(const int64_t *__restrict__ seg_first, int k,
                                                              const uint32_t *__restrict__ maps,
                                                              uint8_t *__restrict__ starts,
                                                              uint8_t *__restrict__ finals) {
    const int m = blockIdx.x, lane = threadIdx.x;
    const int64_t end = seg_first[m + 1];
    int c = 0;
    for (int64_t s = seg_first[m]; s < end; s += 8) {
        uint32_t row[8];
#pragma unroll
        for (int r = 0; r < 8; r++) row[r] = s + r < end ? maps[(s + r) * 64 + lane] : 0u;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (s + r < end) {
                if (lane == 0) starts[(s + r) * 4 + k] = (uint8_t)c;
                const uint32_t w = (uint32_t)__shfl((int)row[r], c >> 2, MRZ_WAVE);
                c = (int)((w >> (8 * (c & 3))) & 255u);
            }
        }
    }
    if (lane == 0) finals[(int64_t)m * 4 + k] = (uint8_t)c;
}

// ---- finish: quartiles by rank counting, buckets hit, code bytes; one wave per member ---------------------------
__global__ __launch_bounds__(64) void mrz_tlsh_finish_kernel(const unsigned *__restrict__ counts,
                                                             mrz_tlsh_fin *__restrict__ fins) {
    __shared__ unsigned s[256];
    const int m = blockIdx.x, lane = threadIdx.x;
    unsigned own[4];
    for (int j = 0; j < 4; j++) {
        own[j] = counts[(int64_t)m * 256 + 4 * lane + j];
        s[4 * lane + j] = own[j];
    }
    __syncthreads();
    int less[4] = { 0, 0, 0, 0 }, leq[4] = { 0, 0, 0, 0 };
    for (int i = 0; i < 256; i++) {
        const unsigned u = s[i];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            less[j] += u < own[j];
            leq[j] += u <= own[j];
        }
    }
    // the value at sorted index r is the count with  #smaller <= r < #smaller-or-equal
    unsigned q[3];
    for (int k = 0; k < 3; k++) {
        const int r = 64 * (k + 1) - 1;
        int hit = -1;
        for (int j = 0; j < 4; j++)
            if (less[j] <= r && r < leq[j]) hit = j;
        const unsigned long long who = __ballot(hit >= 0);
        const int src = __ffsll((long long)who) - 1;  // some count sits at every index: `who` is never empty
        q[k] = (unsigned)__shfl((int)(hit >= 0 ? own[hit] : 0u), src, MRZ_WAVE);
    }
    int nz = (own[0] != 0) + (own[1] != 0) + (own[2] != 0) + (own[3] != 0);
    for (int dlt = 1; dlt < 64; dlt <<= 1) nz += __shfl_xor(nz, dlt, MRZ_WAVE);
    unsigned h = 0;
    for (int j = 0; j < 4; j++) h |= (own[j] > q[2] ? 3u : own[j] > q[1] ? 2u : own[j] > q[0] ? 1u : 0u) << (2 * j);
    mrz_tlsh_fin *f = fins + m;
    f->code[lane] = (uint8_t)h;
    if (lane == 0) {
        f->q1 = q[0];
        f->q2 = q[1];
        f->q3 = q[2];
        f->nonzero = (unsigned)nz;
    }
}

// ---- the greedy order ----------------------------------------------------------------------------------------------
// Step c of the loop at ar-mrzip.cpp:408-437: every remaining position is scored against the head (position c) and the
// step's winner goes to keys[c], smallest key wins:
//     score > 130            position                                   (the first such position)
//     0 < score <= 130       1 << 40 | (255 - score) << 32 | position   (the best score, then the first position)
//     score == 0             no key; keys[c] stays all ones and the step swaps with position 0
// The swap of step c - 1 (positions c and keys[c - 1]'s) is applied on the way: the launch reads perm_in through it and
// writes the whole permutation to perm_out, so no launch writes what another workgroup of the same launch reads.
#define MRZ_AR_ROW 144  // a 137-byte digest padded with zeros to nine 16-byte loads
#define MRZ_AR_NONE (~0ull)

__device__ __forceinline__ int mrz_zero_bytes(uint32_t x) {
    uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    t = ~(t | x | 0x7f7f7f7fu);
    return __popc(t);
}

__device__ __forceinline__ int64_t mrz_ar_next_of(unsigned long long key) {
    return key == MRZ_AR_NONE ? 0 : (int64_t)(key & 0xffffffffull);
}

__global__ __launch_bounds__(256) void mrz_ar_order_step_kernel(const uint8_t *__restrict__ dig,
                                                                const int *__restrict__ perm_in,
                                                                int *__restrict__ perm_out, int n, int c,
                                                                unsigned long long *keys) {
    __shared__ unsigned long long part[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t sa = c, sb = c > 0 ? mrz_ar_next_of(keys[c - 1]) : 0;  // c == 0: nothing pending (sa == sb)
    const int head = perm_in[sb];                                         // what stands at position c after the swap
    unsigned long long key = MRZ_AR_NONE;
    if (i < n) {
        const int e = i == sa ? head : i == sb ? perm_in[sa] : perm_in[i];
        perm_out[i] = e;
        if (i > c) {
            const uint8_t *a = dig + (int64_t)head * MRZ_AR_ROW, *b = dig + (int64_t)e * MRZ_AR_ROW;
            int score = -(MRZ_AR_ROW - MRZ_TLSH_STORED);  // the padding always matches
#pragma unroll
            for (int k = 0; k < MRZ_AR_ROW / 16; k++) {
                const uint4 x = mrz_ld16(a + 16 * k), y = mrz_ld16(b + 16 * k);
                score += mrz_zero_bytes(x.x ^ y.x) + mrz_zero_bytes(x.y ^ y.y) + mrz_zero_bytes(x.z ^ y.z) +
                         mrz_zero_bytes(x.w ^ y.w);
            }
            if (score > 130)
                key = (unsigned long long)i;
            else if (score > 0)
                key = (1ull << 40) | ((unsigned long long)(255 - score) << 32) | (unsigned long long)i;
        }
    }
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const unsigned long long o = (unsigned long long)mrz_shfl_xor64((int64_t)key, dlt);
        if (o < key) key = o;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (part[w] < key) key = part[w];
        if (key != MRZ_AR_NONE) atomicMin(&keys[c], key);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) hipFree(p);
    }
    int alloc(mrz_ctx *ctx, int64_t bytes) {
        hipError_t e = hipMalloc(&p, (size_t)(bytes > 0 ? bytes : 16));
        if (e != hipSuccess) {
            p = nullptr;
            ctx->last_err = e;
            return MRZ_E_NOMEM;
        }
        return MRZ_OK;
    }
};

inline int64_t up16(int64_t v) { return (v + 15) & ~15ll; }
}  // namespace

extern "C" int mrz_tlsh_length_code(int64_t len) {
    if (len < 0) return MRZ_E_ARG;
    if (len > MRZ_TLSH_MAX_LEN) return MRZ_E_UNSUPPORTED;
    return mrz_tlsh_lcode(len);
}

// segment length of a call: the caller's, or one that gives a batch of `total` bytes some 8192 segments
static int mrz_tlsh_segment_len(const mrz_tlsh_opts *opts, int64_t total, int64_t *S) {
    if (opts && opts->segment_len) {
        if (opts->segment_len < MRZ_TLSH_SEGMENT_MIN || opts->segment_len > MRZ_TLSH_SEGMENT_MAX) return MRZ_E_ARG;
        *S = opts->segment_len;
        return MRZ_OK;
    }
    int64_t s = 16384;
    while (s < 262144 && s * 8192 < total) s *= 2;
    *S = s;
    return MRZ_OK;
}

// the messages are in device memory (d_msgs: their device addresses, a host array)
int mrz_tlsh_device_batch(mrz_ctx *ctx, const uint8_t *const *d_msgs, const int64_t *lens, int count,
                          const mrz_tlsh_opts *opts, char *out_host, uint8_t *valid) {
    int64_t total = 0;
    for (int i = 0; i < count; i++) total += lens[i];
    int64_t S = 0;
    int rc = mrz_tlsh_segment_len(opts, total, &S);
    if (rc) return rc;
    std::vector<int64_t> seg_first((size_t)count + 1);
    int64_t nseg = 0;
    for (int i = 0; i < count; i++) {
        seg_first[i] = nseg;
        nseg += (lens[i] + S - 1) / S;
    }
    seg_first[count] = nseg;
    if (nseg > 0x7fffffffll) return MRZ_E_UNSUPPORTED;
    // ptrs | lens | seg_first | counts | fins | finals | starts | maps
    const int64_t o_ptrs = 0, o_lens = o_ptrs + up16((int64_t)count * 8), o_first = o_lens + up16((int64_t)count * 8),
                  o_counts = o_first + up16(((int64_t)count + 1) * 8), o_fins = o_counts + (int64_t)count * 1024,
                  o_finals = o_fins + up16((int64_t)count * (int64_t)sizeof(mrz_tlsh_fin)),
                  o_starts = o_finals + up16((int64_t)count * 4), o_maps = o_starts + up16(nseg * 4),
                  need = o_maps + nseg * 256;
    DevBuf buf;
    rc = buf.alloc(ctx, need);
    if (rc) return rc;
    uint8_t *base = (uint8_t *)buf.p;
    hipStream_t st = ctx->stream;
    const uint8_t *const *p_ptrs = (const uint8_t *const *)(base + o_ptrs);
    const int64_t *p_lens = (const int64_t *)(base + o_lens), *p_first = (const int64_t *)(base + o_first);
    unsigned *p_counts = (unsigned *)(base + o_counts);
    mrz_tlsh_fin *p_fins = (mrz_tlsh_fin *)(base + o_fins);
    uint8_t *p_finals = base + o_finals, *p_starts = base + o_starts;
    uint32_t *p_maps = (uint32_t *)(base + o_maps);
    HIPCHK(ctx, hipMemcpyAsync(base + o_ptrs, d_msgs, (size_t)count * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(base + o_lens, lens, (size_t)count * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(base + o_first, seg_first.data(), ((size_t)count + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(p_counts, 0, (size_t)count * 1024, st));
    HIPCHK(ctx, hipMemsetAsync(p_starts, 0, (size_t)up16(nseg * 4), st));
    const dim3 segs((unsigned)nseg), members((unsigned)count);
    if (nseg) {
        hipLaunchKernelGGL(mrz_tlsh_hist_kernel, segs, dim3(256), 0, st, p_ptrs, p_lens, p_first, count, S, p_counts);
        hipLaunchKernelGGL(mrz_tlsh_chain_kernel<0>, segs, dim3(64), 0, st, p_ptrs, p_lens, p_first, count, S,
                           (const uint8_t *)p_starts, p_maps);
    }
    hipLaunchKernelGGL(mrz_tlsh_compose_kernel, members, dim3(64), 0, st, p_first, 0, (const uint32_t *)p_maps, p_starts,
                       p_finals);
    if (nseg)
        hipLaunchKernelGGL(mrz_tlsh_chain_kernel<1>, segs, dim3(64), 0, st, p_ptrs, p_lens, p_first, count, S,
                           (const uint8_t *)p_starts, p_maps);
    hipLaunchKernelGGL(mrz_tlsh_compose_kernel, members, dim3(64), 0, st, p_first, 1, (const uint32_t *)p_maps, p_starts,
                       p_finals);
    if (nseg)
        hipLaunchKernelGGL(mrz_tlsh_chain_kernel<2>, segs, dim3(64), 0, st, p_ptrs, p_lens, p_first, count, S,
                           (const uint8_t *)p_starts, p_maps);
    hipLaunchKernelGGL(mrz_tlsh_compose_kernel, members, dim3(64), 0, st, p_first, 2, (const uint32_t *)p_maps, p_starts,
                       p_finals);
    hipLaunchKernelGGL(mrz_tlsh_finish_kernel, members, dim3(64), 0, st, (const unsigned *)p_counts, p_fins);
    HIPCHK(ctx, hipGetLastError());
    std::vector<mrz_tlsh_fin> fins((size_t)count);
    std::vector<uint8_t> finals((size_t)count * 4);
    HIPCHK(ctx, hipMemcpyAsync(fins.data(), p_fins, (size_t)count * sizeof(mrz_tlsh_fin), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(finals.data(), p_finals, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < count; i++) {
        char *hex = out_host + (size_t)i * (MRZ_TLSH_HEX + 1);
        const bool ok = mrz_tlsh_valid(fins[i], lens[i]);
        if (ok)
            mrz_tlsh_hex(fins[i], &finals[(size_t)i * 4], lens[i], hex);
        else
            memset(hex, 0, MRZ_TLSH_HEX + 1);
        if (valid) valid[i] = ok ? 1 : 0;
    }
    return MRZ_OK;
}

extern "C" int mrz_tlsh_batch(mrz_ctx *ctx, const void *const *msgs, const int64_t *lens, int count, int where,
                              const mrz_tlsh_opts *opts, char *out_host, uint8_t *valid) {
    if (!ctx || count < 0 || (where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) ||
        (count && (!msgs || !lens || !out_host)))
        return MRZ_E_ARG;
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        if (lens[i] < 0 || (lens[i] && !msgs[i])) return MRZ_E_ARG;
        if (lens[i] > MRZ_TLSH_MAX_LEN) return MRZ_E_UNSUPPORTED;  // before any byte is touched
        total += up16(lens[i]);
    }
    int64_t S = 0;
    int rc = mrz_tlsh_segment_len(opts, total, &S);
    if (rc) return rc;
    if (!count) return MRZ_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (where == MRZ_MEM_DEVICE) return mrz_tlsh_device_batch(ctx, (const uint8_t *const *)msgs, lens, count, opts,
                                                              out_host, valid);
    DevBuf data;
    rc = data.alloc(ctx, total);
    if (rc) return rc;
    std::vector<const uint8_t *> ptrs((size_t)count);
    int64_t off = 0;
    for (int i = 0; i < count; i++) {
        ptrs[i] = (const uint8_t *)data.p + off;
        if (lens[i])
            HIPCHK(ctx, hipMemcpyAsync((uint8_t *)data.p + off, msgs[i], (size_t)lens[i], hipMemcpyHostToDevice,
                                       ctx->stream));
        off += up16(lens[i]);
    }
    return mrz_tlsh_device_batch(ctx, ptrs.data(), lens, count, opts, out_host, valid);
}

extern "C" int mrz_ar_order(mrz_ctx *ctx, const uint8_t *digests137, int64_t n, int32_t *perm_out) {
    if (!ctx || n < 0 || n > 0x7fffffffll || (n && (!digests137 || !perm_out))) return MRZ_E_ARG;
    for (int64_t i = 0; i < n; i++) perm_out[i] = (int32_t)i;
    if (n < 2) return MRZ_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> rows((size_t)n * MRZ_AR_ROW, 0);
    for (int64_t i = 0; i < n; i++)
        memcpy(&rows[(size_t)i * MRZ_AR_ROW], digests137 + (size_t)i * MRZ_TLSH_STORED, MRZ_TLSH_STORED);
    // rows | perm A | perm B | keys
    const int64_t o_perm = up16(n * MRZ_AR_ROW), o_keys = o_perm + 2 * up16(n * 4), need = o_keys + n * 8;
    DevBuf buf;
    int rc = buf.alloc(ctx, need);
    if (rc) return rc;
    uint8_t *base = (uint8_t *)buf.p;
    int *perm[2] = { (int *)(base + o_perm), (int *)(base + o_perm + up16(n * 4)) };
    unsigned long long *keys = (unsigned long long *)(base + o_keys);
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(base, rows.data(), rows.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(perm[0], perm_out, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(keys, 0xff, (size_t)n * 8, st));
    const dim3 grid((unsigned)((n + 255) / 256));
    int cur = 0;
    for (int64_t c = 0; c + 1 < n; c++, cur ^= 1)
        hipLaunchKernelGGL(mrz_ar_order_step_kernel, grid, dim3(256), 0, st, (const uint8_t *)base,
                           (const int *)perm[cur], perm[cur ^ 1], (int)n, (int)c, keys);
    HIPCHK(ctx, hipGetLastError());
    // the last step's swap (positions n - 1 and its winner's) is still pending
    unsigned long long last = 0;
    HIPCHK(ctx, hipMemcpyAsync(perm_out, perm[cur], (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&last, keys + (n - 2), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int64_t nx = last == MRZ_AR_NONE ? 0 : (int64_t)(last & 0xffffffffull);
    const int32_t t = perm_out[n - 1];
    perm_out[n - 1] = perm_out[nx];
    perm_out[nx] = t;
    return MRZ_OK;
}
