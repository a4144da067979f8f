// mrz_segcopy.hip -- many device-to-device copies in one launch (mrz_copy_device_batch, include/mrzgpu.h).
//
// An archive member is a (source, destination, length) triple; 10^5 small ones placed by one hipMemcpyAsync each are
// bound by the launches, not by the bytes.  Here the host cuts every non-empty segment into tiles of MRZ_SEG_TILE bytes
// and uploads one table {src, dst, len, index of the segment's first tile}; a workgroup takes a tile, finds its segment
// by a binary search over the tile indices (the tile index comes from blockIdx: the search runs on scalar loads) and
// copies the tile's bytes.  Where source and destination agree modulo 16 a lane moves 16 bytes per step between a
// byte-wise head (up to the destination's next 16-byte boundary) and a byte-wise tail; where they agree modulo 4 only,
// 4 bytes per step in the same way; otherwise single bytes.  A tile begins a multiple of MRZ_SEG_TILE (itself a
// multiple of 16) behind its segment's start, so all tiles of a segment take the same path.  Nothing outside
// [dst, dst + len) is written; no LDS, nothing shared between workgroups, no wait.
// Bound: HBM read + write for long segments on the 16-byte path (2 x len bytes moved); a segment shorter than a few
// hundred bytes is bound by the search (log2(segments) dependent scalar loads) and by its head and tail, which keep
// most of the workgroup idle.
#include <vector>

#include "mrz_ctx.h"
#include "mrz_device.h"

#ifndef MRZ_SEG_TILE
#define MRZ_SEG_TILE 16384
#endif
#define MRZ_SEG_THREADS 256
static_assert(MRZ_SEG_TILE % 16 == 0, "tiles keep the alignment of their segment");

struct mrz_seg {
    const uint8_t *src;
    uint8_t *dst;
    int64_t len;    // > 0
    int64_t tile0;  // index of the segment's first tile: ascends strictly, seg[0].tile0 == 0
};

// n bytes from s to d, s and d congruent modulo sizeof(V): V-wide between a byte-wise head and tail
template <typename V>
__device__ __forceinline__ void mrz_seg_copy_wide(uint8_t *__restrict__ d, const uint8_t *__restrict__ s, int64_t n) {
    const int tid = (int)threadIdx.x;
    int64_t head = (int64_t)((sizeof(V) - ((uintptr_t)d & (sizeof(V) - 1))) & (sizeof(V) - 1));
    if (head > n) head = n;
    const int64_t body = (n - head) / (int64_t)sizeof(V);
    const int64_t tail_at = head + body * (int64_t)sizeof(V);
    if (tid < head) d[tid] = s[tid];
    const V *sv = (const V *)(s + head);
    V *dv = (V *)(d + head);
    for (int64_t v = tid; v < body; v += MRZ_SEG_THREADS) dv[v] = sv[v];
    if (tail_at + tid < n) d[tail_at + tid] = s[tail_at + tid];
}

__global__ __launch_bounds__(MRZ_SEG_THREADS) void mrz_seg_copy_kernel(const mrz_seg *__restrict__ seg, int64_t nseg,
                                                                       int64_t ntiles) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        // the segment that holds tile t: the last g with seg[g].tile0 <= t (the same in every lane)
        int64_t lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (seg[mid].tile0 <= t)
                lo = mid;
            else
                hi = mid - 1;
        }
        const mrz_seg g = seg[lo];
        const int64_t off = (t - g.tile0) * MRZ_SEG_TILE;
        int64_t n = g.len - off;
        if (n > MRZ_SEG_TILE) n = MRZ_SEG_TILE;
        const uint8_t *s = g.src + off;
        uint8_t *d = g.dst + off;
        const unsigned diff = (unsigned)(((uintptr_t)s ^ (uintptr_t)d) & 15);
        if (!diff)
            mrz_seg_copy_wide<uint4>(d, s, n);
        else if (!(diff & 3))
            mrz_seg_copy_wide<uint32_t>(d, s, n);
        else
            for (int64_t k = threadIdx.x; k < n; k += MRZ_SEG_THREADS) d[k] = s[k];
    }
}

extern "C" int mrz_copy_device_batch(mrz_ctx *ctx, const void *const *src, void *const *dst, const int64_t *lens,
                                     int64_t n) {
    if (!ctx || n < 0 || (n > 0 && (!src || !dst || !lens))) return MRZ_E_ARG;
    for (int64_t i = 0; i < n; i++)
        if (lens[i] < 0 || (lens[i] > 0 && (!src[i] || !dst[i]))) return MRZ_E_ARG;
    try {
        std::vector<mrz_seg> tab;
        int64_t ntiles = 0;
        for (int64_t i = 0; i < n; i++) {
            if (!lens[i]) continue;
            tab.push_back(mrz_seg{ (const uint8_t *)src[i], (uint8_t *)dst[i], lens[i], ntiles });
            ntiles += (lens[i] + MRZ_SEG_TILE - 1) / MRZ_SEG_TILE;
        }
        if (tab.empty()) return MRZ_OK;
        HIPCHK(ctx, hipSetDevice(ctx->device));
        int rc = mrz_grow(ctx, (uint8_t **)&ctx->seg_tab, &ctx->seg_tab_cap, (int64_t)(tab.size() * sizeof(mrz_seg)));
        if (rc) return rc;
        hipStream_t s = ctx->stream;
        HIPCHK(ctx, hipMemcpyAsync(ctx->seg_tab, tab.data(), tab.size() * sizeof(mrz_seg), hipMemcpyHostToDevice, s));
        int cus = 0;
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        int64_t grid = (int64_t)(cus > 0 ? cus : 64) * 8;  // 8 workgroups of 4 waves per CU: full occupancy
        if (grid > ntiles) grid = ntiles;
        hipLaunchKernelGGL(mrz_seg_copy_kernel, dim3((unsigned)grid), dim3(MRZ_SEG_THREADS), 0, s,
                           (const mrz_seg *)ctx->seg_tab, (int64_t)tab.size(), ntiles);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(s));  // the table (and the caller's arrays) may be reused on return
        return MRZ_OK;
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}
