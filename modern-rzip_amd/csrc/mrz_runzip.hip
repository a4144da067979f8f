// mrz_runzip.hip -- the decoder of the two rzip streams of a chunk.
//
// Restates the record loop of runzip_chunk (src/runzip.c:277-308) with unzip_literal (:120-157)
// and unzip_match (:159-207): stream 0 is a sequence of records {head:u8, len:u16le} (+ a
// chunk_bytes-wide distance when head != 0), ended by a zero-length literal and the stored
// CRC-32 (most significant byte first, src/rzip.c:662-665); a literal copies `len` bytes of
// stream 1, a match copies `len` bytes of history starting `dist` back, the first
// min(len, dist) history bytes repeated when len > dist (:182-199).
//
// Four passes on the GPU:
//   1. parse, speculative: stream 0 is cut into 1 KiB tiles; records are 3 or 3 + chunk_bytes
//      bytes, so a tile can only be entered at offsets 0 .. 2 + chunk_bytes.  One thread per
//      (tile, entry offset) walks the tile and notes where it leaves it and what it saw
//      (records, output bytes, literal bytes);
//   2. scan: one workgroup composes the per-tile entry->exit tables (associative), which
//      gives every tile its true entry offset and the running record / output / literal
//      counts in front of it;
//   3. parse, for real: one thread per tile writes its records {out_pos, literal offset or
//      distance} and validates them;
//   4. decode: the output is cut into tiles (8-128 KiB, by record density) claimed in order by persistent workgroups.
//      A match needs its history: bytes of earlier tiles are awaited through per-tile done
//      flags (release / acquire at agent scope -- tiles are written on different XCDs), bytes
//      of the same tile are ordered by workgroup barriers.  A workgroup only ever waits for
//      tiles claimed before its own, i.e. by workgroups that are already running.
// Then the CRC-32 kernel runs over the output.  Bound: HBM for literal-heavy input; on highly
// repetitive input the copy chain (tile k needs tile k-1) is latency-bound.
//
// Range decode (mrz_runzip_range / mrz_runzip_origins) replaces pass 4 by mrz_uz_resolve_kernel: every byte of
// [first, first + count) follows its match records backwards to the one stream-1 byte it comes from.  Independent per
// byte: no output scratch, no ordering between workgroups, no literal read that is not delivered.  Its cost follows
// the number of match records followed (hops), not the size of the chunk.
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "mrz_ctx.h"
#include "mrz_device.h"

#define MRZ_UZ_PT 1024        // stream-0 parse tile
#define MRZ_UZ_PHMAX 11       // entry offsets: record size <= 3 + 8
#define MRZ_UZ_END 255        // parse state: terminator seen
#define MRZ_UZ_ERR 254        // parse state: record runs past the end of stream 0
#define MRZ_UZ_TSHIFT_MIN 13  // output tile of the decode pass: 8 KiB (many short records) .. 128 KiB (few long ones)
#define MRZ_UZ_TSHIFT_MAX 17
#ifndef MRZ_UZ_DEC_THREADS
#define MRZ_UZ_DEC_THREADS 512
#endif
#define MRZ_UZ_THREADS 256
#define MRZ_UZ_SCAN_THREADS 128  // run tables of the scan live in LDS: 128 x 12 x 25 B
#define MRZ_UZ_MATCH (1ull << 63)
#define MRZ_UZ_SPIN_LIMIT (1ll << 30)

struct mrz_urec {
    int64_t out_pos;          // first output byte of the record
    unsigned long long src;   // literal: offset in stream 1; match: MRZ_UZ_MATCH | distance
};

struct mrz_uz_hdr {
    int64_t nrec, out_total, lit_total, term_pos;
    int final_state;
    int error;                // 1 = invalid record (distance 0 / beyond history, empty match), 2 = a wait gave up
    unsigned long long next_tile;   // decode pass: tile claim counter
    unsigned long long prefix_done; // decode pass: every tile below this index is complete
    unsigned long long total_hops;  // range resolve: match records followed, summed over the bytes of the range
    unsigned long long max_hops;    // ... and the most for one byte
};

struct mrz_uz_tile {          // per parse tile and entry offset
    unsigned char exit_state[MRZ_UZ_PHMAX + 1];
    unsigned nrec[MRZ_UZ_PHMAX + 1];
    int64_t outb[MRZ_UZ_PHMAX + 1];
    int64_t litb[MRZ_UZ_PHMAX + 1];
};

struct mrz_uz_base {          // per parse tile, after the scan
    int64_t rec_base, out_base, lit_base;
    int entry;                // true entry offset, or MRZ_UZ_END / MRZ_UZ_ERR
};

// walk one parse tile from `pos`; sink(kind, len, dist_pos) is called per record when WRITE
template <bool WRITE>
__device__ __forceinline__ int mrz_uz_walk(const uint8_t *__restrict__ s0, int64_t s0_len, int cb, int64_t pos,
                                           int64_t tile_end, unsigned *nrec_out, int64_t *outb_out, int64_t *litb_out,
                                           mrz_urec *__restrict__ rec, int64_t rec_at, int64_t out_at, int64_t lit_at,
                                           mrz_uz_hdr *hdr) {
    unsigned nrec = 0;
    int64_t outb = 0, litb = 0;
    int state = -1;
    while (pos < tile_end) {
        if (pos + 3 > s0_len) {
            state = MRZ_UZ_ERR;
            break;
        }
        const int head = s0[pos];
        const int64_t len = (int64_t)s0[pos + 1] | ((int64_t)s0[pos + 2] << 8);
        if (!head && !len) {  // terminator; the stored CRC follows
            state = pos + 7 <= s0_len ? MRZ_UZ_END : MRZ_UZ_ERR;
            if (WRITE && state == MRZ_UZ_END) {
                hdr->term_pos = pos;
                rec[rec_at + nrec].out_pos = out_at + outb;
                rec[rec_at + nrec].src = 0;
            }
            break;
        }
        if (!head) {
            if (WRITE) {
                rec[rec_at + nrec].out_pos = out_at + outb;
                rec[rec_at + nrec].src = (unsigned long long)(lit_at + litb);
            }
            litb += len;
            pos += 3;
        } else {
            if (pos + 3 + cb > s0_len) {
                state = MRZ_UZ_ERR;
                break;
            }
            if (WRITE) {
                unsigned long long dist = 0;
                for (int k = 0; k < cb; k++) dist |= (unsigned long long)s0[pos + 3 + k] << (8 * k);
                // unzip_match: n = MIN(len, offset) < 1 is "corrupt archive" (:176-177); history starts at 0
                if (dist < 1 || dist > (unsigned long long)(out_at + outb) || len < 1) hdr->error = 1;
                rec[rec_at + nrec].out_pos = out_at + outb;
                rec[rec_at + nrec].src = MRZ_UZ_MATCH | dist;
            }
            pos += 3 + cb;
        }
        outb += len;
        nrec++;
    }
    *nrec_out = nrec;
    *outb_out = outb;
    *litb_out = litb;
    return state >= 0 ? state : (int)(pos - tile_end);
}

__global__ __launch_bounds__(MRZ_UZ_THREADS) void mrz_uz_parse1_kernel(const uint8_t *__restrict__ s0, int64_t s0_len,
                                                                       int cb, int64_t ntiles,
                                                                       mrz_uz_tile *__restrict__ tiles) {
    const int ph = 3 + cb;
    const int64_t id = (int64_t)blockIdx.x * MRZ_UZ_THREADS + threadIdx.x;
    const int64_t t = id / ph;
    const int c = (int)(id % ph);
    if (t >= ntiles) return;
    unsigned nrec;
    int64_t outb, litb;
    int64_t tile_end = (t + 1) * MRZ_UZ_PT;
    if (tile_end > s0_len) tile_end = s0_len;
    int st;
    st = mrz_uz_walk<false>(s0, s0_len, cb, t * MRZ_UZ_PT + c, tile_end, &nrec, &outb, &litb, nullptr, 0, 0, 0, nullptr);
    // a walk that reaches the end of stream 0 without a terminator is an error
    if (st < MRZ_UZ_ERR && tile_end == s0_len) st = MRZ_UZ_ERR;
    tiles[t].exit_state[c] = (unsigned char)st;
    tiles[t].nrec[c] = nrec;
    tiles[t].outb[c] = outb;
    tiles[t].litb[c] = litb;
}

// one workgroup: thread i composes the tables of tiles [i*per, (i+1)*per) for every entry state, thread 0 chains the
// runs, then every thread replays its run from its true entry state and writes the per-tile bases
__global__ __launch_bounds__(MRZ_UZ_SCAN_THREADS) void mrz_uz_scan_kernel(const mrz_uz_tile *__restrict__ tiles,
                                                                     int64_t ntiles, int cb,
                                                                     mrz_uz_base *__restrict__ bases,
                                                                     mrz_uz_hdr *__restrict__ hdr) {
    __shared__ unsigned char r_exit[MRZ_UZ_SCAN_THREADS][MRZ_UZ_PHMAX + 1];
    __shared__ int64_t r_nrec[MRZ_UZ_SCAN_THREADS][MRZ_UZ_PHMAX + 1];
    __shared__ int64_t r_outb[MRZ_UZ_SCAN_THREADS][MRZ_UZ_PHMAX + 1];
    __shared__ int64_t r_litb[MRZ_UZ_SCAN_THREADS][MRZ_UZ_PHMAX + 1];
    __shared__ int s_entry[MRZ_UZ_SCAN_THREADS];
    __shared__ int64_t s_rec[MRZ_UZ_SCAN_THREADS], s_out[MRZ_UZ_SCAN_THREADS], s_lit[MRZ_UZ_SCAN_THREADS];
    const int ph = 3 + cb;
    const int i = threadIdx.x;
    const int64_t per = (ntiles + MRZ_UZ_SCAN_THREADS - 1) / MRZ_UZ_SCAN_THREADS;
    const int64_t t0 = (int64_t)i * per;
    int64_t t1 = t0 + per;
    if (t1 > ntiles) t1 = ntiles;
    for (int c = 0; c < ph; c++) {
        int st = c;
        int64_t nr = 0, ob = 0, lb = 0;
        for (int64_t t = t0; t < t1 && st < MRZ_UZ_ERR; t++) {
            nr += tiles[t].nrec[st];
            ob += tiles[t].outb[st];
            lb += tiles[t].litb[st];
            st = tiles[t].exit_state[st];
        }
        r_exit[i][c] = (unsigned char)st;
        r_nrec[i][c] = nr;
        r_outb[i][c] = ob;
        r_litb[i][c] = lb;
    }
    __syncthreads();
    if (i == 0) {
        int st = 0;
        int64_t nr = 0, ob = 0, lb = 0;
        for (int k = 0; k < MRZ_UZ_SCAN_THREADS; k++) {
            s_entry[k] = st;
            s_rec[k] = nr;
            s_out[k] = ob;
            s_lit[k] = lb;
            if (st < MRZ_UZ_ERR && (int64_t)k * per < ntiles) {
                nr += r_nrec[k][st];
                ob += r_outb[k][st];
                lb += r_litb[k][st];
                st = r_exit[k][st];
            }
        }
        hdr->nrec = nr;
        hdr->out_total = ob;
        hdr->lit_total = lb;
        hdr->final_state = ntiles ? st : MRZ_UZ_ERR;
    }
    __syncthreads();
    int st = s_entry[i];
    int64_t nr = s_rec[i], ob = s_out[i], lb = s_lit[i];
    for (int64_t t = t0; t < t1; t++) {
        bases[t].entry = st;
        bases[t].rec_base = nr;
        bases[t].out_base = ob;
        bases[t].lit_base = lb;
        if (st < MRZ_UZ_ERR) {
            nr += tiles[t].nrec[st];
            ob += tiles[t].outb[st];
            lb += tiles[t].litb[st];
            st = tiles[t].exit_state[st];
        }
    }
}

__global__ __launch_bounds__(MRZ_UZ_THREADS) void mrz_uz_parse2_kernel(const uint8_t *__restrict__ s0, int64_t s0_len,
                                                                       int cb, int64_t ntiles,
                                                                       const mrz_uz_base *__restrict__ bases,
                                                                       mrz_urec *__restrict__ rec,
                                                                       mrz_uz_hdr *__restrict__ hdr) {
    const int64_t t = (int64_t)blockIdx.x * MRZ_UZ_THREADS + threadIdx.x;
    if (t >= ntiles) return;
    const mrz_uz_base b = bases[t];
    if (b.entry >= MRZ_UZ_ERR) return;
    int64_t tile_end = (t + 1) * MRZ_UZ_PT;
    if (tile_end > s0_len) tile_end = s0_len;
    unsigned nrec;
    int64_t outb, litb;
    mrz_uz_walk<true>(s0, s0_len, cb, t * MRZ_UZ_PT + b.entry, tile_end, &nrec, &outb, &litb, rec, b.rec_base, b.out_base,
                      b.lit_base, hdr);
}

// workgroup-wide copy of n bytes (both sides arbitrarily aligned): 16 B per thread and step
__device__ __forceinline__ void mrz_uz_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int64_t n) {
    for (int64_t o = (int64_t)threadIdx.x * 16; o < n; o += (int64_t)MRZ_UZ_DEC_THREADS * 16) {
        if (o + 16 <= n) {
            const uint4 v = mrz_ld16(src + o);
            __builtin_memcpy(dst + o, &v, 16);
        } else
            for (int64_t k = o; k < n; k++) dst[k] = src[k];
    }
}

__device__ __forceinline__ void mrz_uz_acquire() {
#ifdef __HIP_DEVICE_COMPILE__
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
}
__device__ __forceinline__ void mrz_uz_release() {
#ifdef __HIP_DEVICE_COMPILE__
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#endif
}

__global__ __launch_bounds__(MRZ_UZ_DEC_THREADS) void mrz_uz_decode_kernel(const mrz_urec *__restrict__ rec, int64_t nrec,
                                                                       const uint8_t *__restrict__ s1,
                                                                       uint8_t *__restrict__ out, int64_t out_total,
                                                                       int64_t ntiles, int tshift,
                                                                       unsigned *__restrict__ done,
                                                                       mrz_uz_hdr *__restrict__ hdr) {
    const int64_t TO = (int64_t)1 << tshift;
    __shared__ long long s_tile, s_first, s_prefix;
    __shared__ int s_fail;
    long long known = 0;  // every tile below this index is known to be complete (and acquired)
    unsigned long long vmask = 0;  // bit i: tile known + i has been seen complete and acquired as well
    while (true) {
        if (threadIdx.x == 0) {
            const long long t = (long long)__hip_atomic_fetch_add(&hdr->next_tile, 1ull, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_AGENT);
            s_tile = t;
            s_fail = 0;
            if (t < ntiles) {
                // last record that starts at or before the tile's first byte
                const int64_t T0 = (t << tshift);
                int64_t lo = 0, hi = nrec - 1;
                while (lo < hi) {
                    const int64_t mid = (lo + hi + 1) >> 1;
                    if (rec[mid].out_pos <= T0)
                        lo = mid;
                    else
                        hi = mid - 1;
                }
                s_first = lo;
            }
        }
        __syncthreads();
        const long long t = s_tile;
        if (t >= ntiles) return;
        const int64_t T0 = (t << tshift);
        const int64_t T1 = T0 + TO < out_total ? T0 + TO : out_total;
        int64_t written_to = T0;  // bytes of this tile below this are written (maybe not yet ordered)
        bool unordered = false;   // stores since the last barrier
        for (int64_t r = s_first; r < nrec; r++) {
            const int64_t o = rec[r].out_pos;
            if (o >= T1) break;
            const int64_t o_end = rec[r + 1].out_pos;
            const unsigned long long src = rec[r].src;
            const int64_t x0 = o > T0 ? o : T0, x1 = o_end < T1 ? o_end : T1;
            if (x1 <= x0) continue;
            if (!(src & MRZ_UZ_MATCH)) {
                mrz_uz_copy(out + x0, s1 + (int64_t)src + (x0 - o), x1 - x0);
            } else {
                const int64_t dist = (int64_t)(src & ~MRZ_UZ_MATCH);
                const int64_t len = o_end - o, span = len < dist ? len : dist, from = o - dist;
                // history needed by this piece
                const int64_t h0 = span == len ? from + (x0 - o) : from;
                const int64_t h1 = span == len ? from + (x1 - o) : from + span;
                if (h0 < T0) {
                    const long long need_hi = (long long)(((h1 < T0 ? h1 : T0) - 1) >> tshift);
                    const long long need_lo = (long long)(h0 >> tshift) > known ? (long long)(h0 >> tshift) : known;
                    bool seen = need_hi < known;
                    if (!seen && need_hi - known < 64) {
                        const unsigned long long hi_bits = need_hi - known == 63 ? ~0ull : ((1ull << (need_hi - known + 1)) - 1ull);
                        const unsigned long long needmask = hi_bits & ~((1ull << (need_lo - known)) - 1ull);
                        seen = (vmask & needmask) == needmask;
                    }
                    if (!seen) {
                        if (threadIdx.x == 0) {
                            long long spins = 0;
                            // relaxed polls (an acquire load would invalidate the L2 on every iteration); one acquire
                            // fence by every thread follows the barrier below
                            long long p = (long long)__hip_atomic_load(&hdr->prefix_done, __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT);
                            for (long long q = (long long)(h0 >> tshift) > p ? (long long)(h0 >> tshift) : p;
                                 q <= need_hi; q++) {
                                while (!__hip_atomic_load(&done[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                                    if (spins++ > MRZ_UZ_SPIN_LIMIT) {
                                        s_fail = 1;
                                        break;
                                    }
                                    __builtin_amdgcn_s_sleep(1);
                                }
                                if (s_fail) break;
                            }
                            s_prefix = p;
                        }
                        __syncthreads();
                        mrz_uz_acquire();
                        if (s_fail) {
                            if (threadIdx.x == 0) hdr->error = 2;
                            return;
                        }
                        // remember the prefix and, in a 64-tile window above it, the single tiles just seen
                        const long long p = s_prefix > known ? s_prefix : known;
                        vmask = p - known >= 64 ? 0ull : vmask >> (p - known);
                        known = p;
                        for (long long qq = need_lo > known ? need_lo : known; qq <= need_hi && qq - known < 64; qq++)
                            vmask |= 1ull << (qq - known);
                        unordered = false;
                    }
                }
                if (h1 > T0 && unordered) {  // history inside this tile: order the earlier stores
                    __syncthreads();
                    unordered = false;
                }
                if (span == len)
                    mrz_uz_copy(out + x0, out + from + (x0 - o), x1 - x0);
                else  // the first `dist` history bytes repeat (src/runzip.c:182-199)
                    for (int64_t x = x0 + threadIdx.x; x < x1; x += MRZ_UZ_DEC_THREADS) out[x] = out[from + (x - o) % span];
            }
            written_to = x1;
            unordered = true;
        }
        (void)written_to;
        __syncthreads();
        if (threadIdx.x == 0) {
            mrz_uz_release();
            __hip_atomic_store(&done[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // after the release fence
            // push the completed prefix forward as far as the flags allow
            unsigned long long p = __hip_atomic_load(&hdr->prefix_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while ((long long)p < ntiles && __hip_atomic_load(&done[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                unsigned long long expect = p;
                if (__hip_atomic_compare_exchange_strong(&hdr->prefix_done, &expect, p + 1, __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    p = p + 1;
                else
                    p = expect;
            }
        }
        __syncthreads();
    }
}

// ---- range decode: the origin of single output bytes --------------------------------------------------------------

// the record that holds output byte x: the last r in [0, hi] with rec[r].out_pos <= x (out_pos ascends strictly over
// the records in front of the terminator, and rec[0].out_pos == 0)
__device__ __forceinline__ int64_t mrz_uz_find(const mrz_urec *__restrict__ rec, int64_t x, int64_t hi) {
    int64_t lo = 0;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (rec[mid].out_pos <= x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// a value that is the same in every lane of the wave, said so to the compiler: searches on it use scalar loads.  (The
// emulator has nothing to gain from it, and a collective per pass there costs more than the pass.)
__device__ __forceinline__ int64_t mrz_uz_uniform64(int64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    return mrz_uni64(v);
#else
    return v;
#endif
}

// Every output byte has exactly one origin in stream 1: a literal record gives it directly, a match record sends
// position x to out_pos - dist + (x - out_pos) % min(len, dist) (unzip_match's "first min(len, dist) history bytes
// repeat", src/runzip.c:182-199), which lies in front of the record -- one hop; x falls strictly, so the walk ends.
// A lane owns one byte per pass and a wave 64 consecutive ones, so the stores coalesce.  The wave searches once for
// the record of its first byte, with wave-uniform operands; where the 64 positions fall into that record -- the common
// case -- nobody searches again, and a lane whose byte lies elsewhere searches for itself.  That test is the divergent
// branch itself: the wave skips it when no lane takes it, and no collective is needed to say so.  From then on every
// lane walks alone (lanes that stay in one record make the same loads in step); the record a hop leaves bounds the
// next search from above.  No LDS, nothing shared between workgroups, no wait on memory.
// ORIGINS: dst[i] = stream-1 offset of output byte first + i (int64); otherwise dst[i] = s1[that offset].
// nrec counts the records in front of the terminator, which is rec[nrec].  A walk of more than nrec hops cannot
// happen on validated records; it ends with hdr->error = 2 instead of running on.
template <bool ORIGINS>
__global__ __launch_bounds__(MRZ_UZ_THREADS) void mrz_uz_resolve_kernel(const mrz_urec *__restrict__ rec, int64_t nrec,
                                                                        const uint8_t *__restrict__ s1, int64_t first,
                                                                        int64_t count, void *__restrict__ dst,
                                                                        mrz_uz_hdr *__restrict__ hdr) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * MRZ_UZ_THREADS;
    int64_t sum_hops = 0, top_hops = 0;
    // `base` is the wave's first byte of the pass (the same in all its lanes)
    const int64_t base0 = mrz_uz_uniform64((int64_t)blockIdx.x * MRZ_UZ_THREADS + (threadIdx.x - lane));
    if (base0 >= count) return;  // the whole wave: nothing to resolve, nothing to report
    for (int64_t base = base0; base < count; base += stride) {
        int64_t r = mrz_uz_find(rec, first + base, nrec - 1);  // once per wave
        int64_t o = rec[r].out_pos, o_end = rec[r + 1].out_pos;
        const int64_t i = base + lane;
        int64_t hops = 0, origin = 0;
        if (i < count) {
            int64_t x = first + i, hi = nrec - 1;
            if (x >= o_end) {  // (x >= o holds: x >= first + base) not the wave's record
                r = mrz_uz_find(rec, x, hi);
                o = rec[r].out_pos;
                o_end = rec[r + 1].out_pos;
            }
            while (true) {
                const unsigned long long src = rec[r].src;
                if (!(src & MRZ_UZ_MATCH)) {
                    origin = (int64_t)src + (x - o);
                    break;
                }
                if (hops >= nrec) {
                    hdr->error = 2;
                    break;
                }
                const int64_t dist = (int64_t)(src & ~MRZ_UZ_MATCH), len = o_end - o;
                const int64_t span = len < dist ? len : dist;
                const int64_t k = x - o;
                x = o - dist + (k < span ? k : k % span);
                hops++;
                hi = r;
                r = mrz_uz_find(rec, x, hi);
                o = rec[r].out_pos;
                o_end = rec[r + 1].out_pos;
            }
        }
        if (i < count) {
            if (ORIGINS)
                ((int64_t *)dst)[i] = origin;
            else
                ((uint8_t *)dst)[i] = s1[origin];
        }
        sum_hops += hops;
        top_hops = hops > top_hops ? hops : top_hops;
    }
    // statistics: reduce over the wave, then one atomic each per wave
    for (int d = 32; d; d >>= 1) {
        sum_hops += mrz_shfl_xor64(sum_hops, d);
        const int64_t t = mrz_shfl_xor64(top_hops, d);
        top_hops = t > top_hops ? t : top_hops;
    }
    if (lane == 0 && sum_hops) {
        atomicAdd(&hdr->total_hops, (unsigned long long)sum_hops);
        unsigned long long seen = __hip_atomic_load(&hdr->max_hops, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while ((unsigned long long)top_hops > seen) {
            const unsigned long long was = atomicCAS(&hdr->max_hops, seen, (unsigned long long)top_hops);
            if (was == seen) break;
            seen = was;
        }
    }
}

// ---- many ranges of a chunk in one launch (mrz_runzip_ranges / mrz_runzip_origins_multi) --------------------------
// The ranges come as a table of n + 1 entries of 16 bytes: first[r], and prefix[r] = the sum of the counts in front of
// range r (entry n holds the total).  Flat index i of the packed output belongs to the last r with prefix[r] <= i --
// empty ranges share their prefix with their successor and are never found.
struct mrz_uz_rng {
    int64_t first, prefix;
};

__device__ __forceinline__ int64_t mrz_uz_find_rng(const mrz_uz_rng *__restrict__ rng, int64_t i, int64_t hi) {
    int64_t lo = 0;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (rng[mid].prefix <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// mrz_uz_resolve_kernel over the packed output of nrng ranges.  A wave owns 64 consecutive flat indices; it searches
// once, with wave-uniform operands, for the range of its first index and for the record of that range's byte there; a
// lane whose index lies beyond that range searches the table for itself, and one whose byte lies outside that record
// (in front of it too: the ranges come in any order) searches the records for itself.  The walk, its hop limit, the
// hdr->error = 2 exit and the statistics are those of mrz_uz_resolve_kernel, restated here so that kernel's code stays
// what it is.  No LDS, nothing shared between workgroups, no wait on memory.
template <bool ORIGINS>
__global__ __launch_bounds__(MRZ_UZ_THREADS) void mrz_uz_resolve_multi_kernel(const mrz_urec *__restrict__ rec, int64_t nrec,
                                                                              const uint8_t *__restrict__ s1,
                                                                              const mrz_uz_rng *__restrict__ rng,
                                                                              int64_t nrng, int64_t count,
                                                                              void *__restrict__ dst,
                                                                              mrz_uz_hdr *__restrict__ hdr) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * MRZ_UZ_THREADS;
    int64_t sum_hops = 0, top_hops = 0;
    const int64_t base0 = mrz_uz_uniform64((int64_t)blockIdx.x * MRZ_UZ_THREADS + (threadIdx.x - lane));
    if (base0 >= count) return;  // the whole wave
    for (int64_t base = base0; base < count; base += stride) {
        // once per wave: the range of the first index, and the record of its byte
        const int64_t g = mrz_uz_find_rng(rng, base, nrng - 1);
        int64_t g_first = rng[g].first, g_at = rng[g].prefix;
        const int64_t g_end = rng[g + 1].prefix;
        int64_t r = mrz_uz_find(rec, g_first + (base - g_at), nrec - 1);
        int64_t o = rec[r].out_pos, o_end = rec[r + 1].out_pos;
        const int64_t i = base + lane;
        int64_t hops = 0, origin = 0;
        if (i < count) {
            if (i >= g_end) {  // not the wave's range
                const int64_t g2 = mrz_uz_find_rng(rng, i, nrng - 1);
                g_first = rng[g2].first;
                g_at = rng[g2].prefix;
            }
            int64_t x = g_first + (i - g_at), hi = nrec - 1;
            if (x < o || x >= o_end) {  // not the wave's record
                r = mrz_uz_find(rec, x, hi);
                o = rec[r].out_pos;
                o_end = rec[r + 1].out_pos;
            }
            while (true) {
                const unsigned long long src = rec[r].src;
                if (!(src & MRZ_UZ_MATCH)) {
                    origin = (int64_t)src + (x - o);
                    break;
                }
                if (hops >= nrec) {
                    hdr->error = 2;
                    break;
                }
                const int64_t dist = (int64_t)(src & ~MRZ_UZ_MATCH), len = o_end - o;
                const int64_t span = len < dist ? len : dist;
                const int64_t k = x - o;
                x = o - dist + (k < span ? k : k % span);
                hops++;
                hi = r;
                r = mrz_uz_find(rec, x, hi);
                o = rec[r].out_pos;
                o_end = rec[r + 1].out_pos;
            }
            if (ORIGINS)
                ((int64_t *)dst)[i] = origin;
            else
                ((uint8_t *)dst)[i] = s1[origin];
        }
        sum_hops += hops;
        top_hops = hops > top_hops ? hops : top_hops;
    }
    for (int d = 32; d; d >>= 1) {
        sum_hops += mrz_shfl_xor64(sum_hops, d);
        const int64_t t = mrz_shfl_xor64(top_hops, d);
        top_hops = t > top_hops ? t : top_hops;
    }
    if (lane == 0 && sum_hops) {
        atomicAdd(&hdr->total_hops, (unsigned long long)sum_hops);
        unsigned long long seen = __hip_atomic_load(&hdr->max_hops, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while ((unsigned long long)top_hops > seen) {
            const unsigned long long was = atomicCAS(&hdr->max_hops, seen, (unsigned long long)top_hops);
            if (was == seen) break;
            seen = was;
        }
    }
}

// ---- range decode over a stream 1 that stays in its blocks (mrz_runzip_buffer_range_ex) ---------------------------
// The origins of a range stay on the device; `starts` is the table of the chunk's stream-1 blocks as ascending offsets
// in stream 1, starts[0] == 0 (an empty block shares its start with its successor and is never found).

// the block that holds stream-1 offset x: the last b with starts[b] <= x
__device__ __forceinline__ int64_t mrz_uz_block_of(const int64_t *__restrict__ starts, int64_t nblocks, int64_t x) {
    int64_t lo = 0, hi = nblocks - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= x)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// span[b] = the lowest and highest in-block offset that any origin asks of block b (the host presets lo = ~0, hi = 0:
// an untouched block keeps lo > hi; no block is longer than 2^32).  Consecutive output bytes mostly have consecutive
// origins, so the 64 origins of a wave fall into one or two blocks: the wave reduces per distinct block (one round of
// shuffles each) and its leader issues the two atomics.
__global__ __launch_bounds__(MRZ_UZ_THREADS) void mrz_uz_block_span_kernel(const int64_t *__restrict__ origins,
                                                                           int64_t count,
                                                                           const int64_t *__restrict__ starts,
                                                                           int64_t nblocks,
                                                                           mrz_uz_span *__restrict__ span) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t stride = (int64_t)gridDim.x * MRZ_UZ_THREADS;
    const int64_t base0 = mrz_uz_uniform64((int64_t)blockIdx.x * MRZ_UZ_THREADS + (threadIdx.x - lane));
    for (int64_t base = base0; base < count; base += stride) {
        const int64_t i = base + lane;
        int64_t b = -1;
        uint32_t off = 0;
        if (i < count) {
            const int64_t x = origins[i];
            b = mrz_uz_block_of(starts, nblocks, x);
            off = (uint32_t)(x - starts[b]);
        }
        mrz_u64 todo = __ballot(i < count);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int64_t bl = mrz_bcast64(b, leader);
            const bool mine = b == bl;
            uint32_t lo = mine ? off : 0xffffffffu, hi = mine ? off : 0u;
            for (int d = 32; d; d >>= 1) {
                const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, d, MRZ_WAVE), h2 = (uint32_t)__shfl_xor((int)hi, d, MRZ_WAVE);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if (lane == leader) {
                atomicMin(&span[bl].lo, lo);
                atomicMax(&span[bl].hi, hi);
            }
            todo &= ~__ballot(mine);
        }
    }
}

// out[i] = staged[base[b] + (in-block offset of origin i) - span[b].lo], b the origin's block: `staged` holds, for every
// touched block, its bytes from in-block offset span[b].lo on at staged + base[b]
__global__ __launch_bounds__(MRZ_UZ_THREADS) void mrz_uz_block_gather_kernel(const int64_t *__restrict__ origins,
                                                                             int64_t count,
                                                                             const int64_t *__restrict__ starts,
                                                                             int64_t nblocks,
                                                                             const mrz_uz_span *__restrict__ span,
                                                                             const int64_t *__restrict__ base,
                                                                             const uint8_t *__restrict__ staged,
                                                                             uint8_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * MRZ_UZ_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MRZ_UZ_THREADS + threadIdx.x; i < count; i += stride) {
        const int64_t x = origins[i];
        const int64_t b = mrz_uz_block_of(starts, nblocks, x);
        out[i] = staged[base[b] + (x - starts[b]) - (int64_t)span[b].lo];
    }
}

static unsigned uz_block_grid(int cus, int64_t count) {
    int64_t grid = (int64_t)(cus > 0 ? cus : 64) * 8;
    const int64_t blocks = (count + MRZ_UZ_THREADS - 1) / MRZ_UZ_THREADS;
    return (unsigned)(grid > blocks ? blocks : grid);
}

extern "C" hipError_t mrz_launch_block_span(hipStream_t stream, int cus, const int64_t *origins, int64_t count,
                                            const int64_t *starts, int64_t nblocks, mrz_uz_span *span) {
    hipLaunchKernelGGL(mrz_uz_block_span_kernel, dim3(uz_block_grid(cus, count)), dim3(MRZ_UZ_THREADS), 0, stream, origins,
                       count, starts, nblocks, span);
    return hipGetLastError();
}

extern "C" hipError_t mrz_launch_block_gather(hipStream_t stream, int cus, const int64_t *origins, int64_t count,
                                              const int64_t *starts, int64_t nblocks, const mrz_uz_span *span,
                                              const int64_t *base, const uint8_t *staged, uint8_t *out) {
    hipLaunchKernelGGL(mrz_uz_block_gather_kernel, dim3(uz_block_grid(cus, count)), dim3(MRZ_UZ_THREADS), 0, stream,
                       origins, count, starts, nblocks, span, base, staged, out);
    return hipGetLastError();
}

static int uz_grow(mrz_ctx *ctx, int64_t want) {
    return mrz_grow(ctx, (uint8_t **)&ctx->rz_scratch, &ctx->rz_scratch_cap, want);
}

// what the three parse launches leave behind
struct uz_parsed {
    mrz_uz_hdr h;           // as of the end of the parse
    mrz_uz_hdr *d_hdr;
    mrz_urec *d_rec;        // h.nrec records and the terminator's
    const uint8_t *d_s0;
    uint8_t *d_extra;       // `extra` bytes of scratch behind everything else (the staged stream 1 of a host call)
};

// Uploads stream 0 when it is host memory -- and `up_len` bytes of `up` to d_extra along with it --, runs the two parse
// passes and the scan, and waits for the header.  The verdict on the stream (p->h) is the caller's to read.
static int uz_parse(mrz_ctx *ctx, const void *s0, int64_t s0_len, int where, int chunk_bytes, int64_t extra,
                    const void *up, int64_t up_len, uz_parsed *p) {
    hipStream_t s = ctx->stream;
    const int64_t ntiles = (s0_len + MRZ_UZ_PT - 1) / MRZ_UZ_PT;
    const int64_t max_rec = s0_len / 3 + 2;

    // scratch layout (256-B aligned pieces)
    auto al = [](int64_t v) { return (v + 255) / 256 * 256; };
    const int64_t o_hdr = 0;
    const int64_t o_tiles = o_hdr + al(sizeof(mrz_uz_hdr));
    const int64_t o_bases = o_tiles + al(ntiles * (int64_t)sizeof(mrz_uz_tile));
    const int64_t o_rec = o_bases + al(ntiles * (int64_t)sizeof(mrz_uz_base));
    const int64_t o_s0 = o_rec + al(max_rec * (int64_t)sizeof(mrz_urec));
    const int64_t o_extra = o_s0 + (where == MRZ_MEM_HOST ? al(s0_len + 64) : 0);
    const int64_t o_end = o_extra + al(extra);
    int rc = uz_grow(ctx, o_end);
    if (rc) return rc;
    uint8_t *base = (uint8_t *)ctx->rz_scratch;
    mrz_uz_hdr *d_hdr = (mrz_uz_hdr *)(base + o_hdr);
    mrz_uz_tile *d_tiles = (mrz_uz_tile *)(base + o_tiles);
    mrz_uz_base *d_bases = (mrz_uz_base *)(base + o_bases);
    mrz_urec *d_rec = (mrz_urec *)(base + o_rec);
    const uint8_t *d_s0 = (const uint8_t *)s0;
    if (where == MRZ_MEM_HOST) {
        HIPCHK(ctx, hipMemcpyAsync(base + o_s0, s0, (size_t)s0_len, hipMemcpyHostToDevice, s));
        if (up_len) HIPCHK(ctx, hipMemcpyAsync(base + o_extra, up, (size_t)up_len, hipMemcpyHostToDevice, s));
        d_s0 = base + o_s0;
    }
    HIPCHK(ctx, hipMemsetAsync(d_hdr, 0, sizeof(mrz_uz_hdr), s));
    const int ph = 3 + chunk_bytes;
    {
        const int64_t threads = ntiles * ph;
        hipLaunchKernelGGL(mrz_uz_parse1_kernel, dim3((unsigned)((threads + MRZ_UZ_THREADS - 1) / MRZ_UZ_THREADS)),
                           dim3(MRZ_UZ_THREADS), 0, s, d_s0, s0_len, chunk_bytes, ntiles, d_tiles);
        hipLaunchKernelGGL(mrz_uz_scan_kernel, dim3(1), dim3(MRZ_UZ_SCAN_THREADS), 0, s, d_tiles, ntiles, chunk_bytes, d_bases,
                           d_hdr);
        hipLaunchKernelGGL(mrz_uz_parse2_kernel, dim3((unsigned)((ntiles + MRZ_UZ_THREADS - 1) / MRZ_UZ_THREADS)),
                           dim3(MRZ_UZ_THREADS), 0, s, d_s0, s0_len, chunk_bytes, ntiles, d_bases, d_rec, d_hdr);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(&p->h, d_hdr, sizeof(p->h), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    p->d_hdr = d_hdr;
    p->d_rec = d_rec;
    p->d_s0 = d_s0;
    p->d_extra = base + o_extra;
    return MRZ_OK;
}

extern "C" int mrz_runzip_chunk(mrz_ctx *ctx, const void *s0, int64_t s0_len, const void *s1, int64_t s1_len, int where,
                                int chunk_bytes, void *out, int out_where, int64_t out_cap, int64_t *out_len,
                                uint32_t *crc_calc, uint32_t *crc_stored) {
    if (!ctx || !s0 || s0_len < 7 || s1_len < 0 || (s1_len > 0 && !s1) || chunk_bytes < 1 || chunk_bytes > 8 || !out_len)
        return MRZ_E_ARG;
    if ((where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) || (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE))
        return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    uz_parsed ps;
    int rc = uz_parse(ctx, s0, s0_len, where, chunk_bytes, where == MRZ_MEM_HOST ? s1_len + 64 : 0, s1, s1_len, &ps);
    if (rc) return rc;
    mrz_uz_hdr h = ps.h;
    mrz_uz_hdr *d_hdr = ps.d_hdr;
    mrz_urec *d_rec = ps.d_rec;
    const uint8_t *d_s0 = ps.d_s0, *d_s1 = where == MRZ_MEM_HOST ? ps.d_extra : (const uint8_t *)s1;
    if (h.final_state != MRZ_UZ_END || h.error || h.lit_total > s1_len) return MRZ_E_CORRUPT;
    *out_len = h.out_total;
    if (h.out_total > out_cap || (h.out_total > 0 && !out)) return MRZ_E_ARG;

    uint8_t *d_out = (uint8_t *)out;
    if (out_where == MRZ_MEM_HOST) {
        rc = mrz_grow(ctx, &ctx->d_rz_out, &ctx->rz_out_cap, h.out_total + 64);
        if (rc) return rc;
        d_out = ctx->d_rz_out;
    }
    // tile size from the record density: about 32 records per tile, 8 KiB .. 128 KiB
    int tshift = MRZ_UZ_TSHIFT_MIN;
    {
        const int64_t target = h.out_total / (h.nrec > 0 ? h.nrec : 1) * 32;
        while (tshift < MRZ_UZ_TSHIFT_MAX && ((int64_t)1 << tshift) < target) tshift++;
    }
    const int64_t otiles = (h.out_total + ((int64_t)1 << tshift) - 1) >> tshift;
    if (otiles) {
        rc = mrz_grow(ctx, &ctx->d_rz_done, &ctx->rz_done_cap, otiles);
        if (rc) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->d_rz_done, 0, (size_t)otiles * sizeof(unsigned), s));
        int cus = 0;
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        int64_t grid = (int64_t)(cus > 0 ? cus : 64) * 2;
        if (grid > otiles) grid = otiles;
        hipLaunchKernelGGL(mrz_uz_decode_kernel, dim3((unsigned)grid), dim3(MRZ_UZ_DEC_THREADS), 0, s, d_rec, h.nrec + 1,
                           d_s1, d_out, h.out_total, otiles, tshift, ctx->d_rz_done, d_hdr);
        HIPCHK(ctx, hipGetLastError());
    }
    // CRC-32 of the output (gcry_md_read at src/runzip.c:310) and the stored one behind the terminator
    rc = mrz_grow(ctx, &ctx->d_crc_parts, &ctx->crc_parts_cap, mrz_crc32_parts_needed(h.out_total));
    if (rc) return rc;
    HIPCHK(ctx, mrz_launch_crc32(s, d_out, h.out_total, ctx->d_crc_tables, ctx->d_crc_parts, ctx->d_crc_out));
    uint32_t crc = 0;
    uint8_t stored[4];
    HIPCHK(ctx, hipMemcpyAsync(&crc, ctx->d_crc_out, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(stored, d_s0 + h.term_pos + 3, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(&h, d_hdr, sizeof(h), hipMemcpyDeviceToHost, s));
    if (out_where == MRZ_MEM_HOST && h.out_total)
        HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)h.out_total, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (h.error) return h.error == 2 ? MRZ_E_STATE : MRZ_E_CORRUPT;
    if (crc_calc) *crc_calc = crc;
    if (crc_stored)
        *crc_stored = (uint32_t)stored[0] << 24 | (uint32_t)stored[1] << 16 | (uint32_t)stored[2] << 8 | stored[3];
    return MRZ_OK;
}

// bytes or origins of [first, first + count): see include/mrzgpu.h
static int uz_range(mrz_ctx *ctx, bool want_origins, const void *s0, int64_t s0_len, const void *s1, int64_t s1_len,
                    int where, int chunk_bytes, int64_t first, int64_t count, void *out, int out_where,
                    mrz_range_info *info) {
    if (!ctx || !s0 || s0_len < 7 || s1_len < 0 || chunk_bytes < 1 || chunk_bytes > 8) return MRZ_E_ARG;
    if (!want_origins && s1_len > 0 && !s1) return MRZ_E_ARG;
    if ((where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) || (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE))
        return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    uz_parsed ps;
    int rc = uz_parse(ctx, s0, s0_len, where, chunk_bytes, 0, nullptr, 0, &ps);
    if (rc) return rc;
    const mrz_uz_hdr &h = ps.h;
    if (h.final_state != MRZ_UZ_END || h.error || h.lit_total > s1_len) return MRZ_E_CORRUPT;
    if (info) {
        info->chunk_len = h.out_total;
        info->total_hops = info->max_hops = 0;
    }
    if (first < 0 || count < 0 || first > h.out_total || count > h.out_total - first) return MRZ_E_ARG;
    if (!count) return MRZ_OK;
    if (!out) return MRZ_E_ARG;

    // a host-resident stream 1 stays where it is: its origins are resolved here and the bytes gathered on the host
    const bool origins = want_origins || where == MRZ_MEM_HOST;
    const bool direct = out_where == MRZ_MEM_DEVICE && origins == want_origins;  // the kernel writes `out` itself
    if (direct && want_origins && ((uintptr_t)out & 7)) return MRZ_E_ARG;
    const int64_t item = origins ? 8 : 1;
    void *d_dst = out;
    if (!direct) {
        rc = mrz_grow(ctx, &ctx->d_rz_out, &ctx->rz_out_cap, count * item);
        if (rc) return rc;
        d_dst = ctx->d_rz_out;
    }
    int cus = 0;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    int64_t grid = (int64_t)(cus > 0 ? cus : 64) * 8;  // 32 waves per CU in flight: the walk is a chain of dependent loads
    const int64_t blocks = (count + MRZ_UZ_THREADS - 1) / MRZ_UZ_THREADS;
    if (grid > blocks) grid = blocks;
    if (origins)
        hipLaunchKernelGGL(mrz_uz_resolve_kernel<true>, dim3((unsigned)grid), dim3(MRZ_UZ_THREADS), 0, s, ps.d_rec, h.nrec,
                           (const uint8_t *)nullptr, first, count, d_dst, ps.d_hdr);
    else
        hipLaunchKernelGGL(mrz_uz_resolve_kernel<false>, dim3((unsigned)grid), dim3(MRZ_UZ_THREADS), 0, s, ps.d_rec, h.nrec,
                           (const uint8_t *)s1, first, count, d_dst, ps.d_hdr);
    HIPCHK(ctx, hipGetLastError());
    mrz_uz_hdr after;
    HIPCHK(ctx, hipMemcpyAsync(&after, ps.d_hdr, sizeof(after), hipMemcpyDeviceToHost, s));
    std::vector<int64_t> h_org;
    if (!direct && origins && !want_origins) {  // bytes asked for, stream 1 on the host
        h_org.resize((size_t)count);
        HIPCHK(ctx, hipMemcpyAsync(h_org.data(), d_dst, (size_t)count * 8, hipMemcpyDeviceToHost, s));
    } else if (!direct)
        HIPCHK(ctx, hipMemcpyAsync(out, d_dst, (size_t)(count * item), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (after.error) return after.error == 2 ? MRZ_E_STATE : MRZ_E_CORRUPT;
    if (info) {
        info->total_hops = (int64_t)after.total_hops;
        info->max_hops = (int64_t)after.max_hops;
    }
    if (!h_org.empty()) {
        // consecutive bytes mostly have consecutive origins: copy runs
        std::vector<uint8_t> staged;
        uint8_t *dst = (uint8_t *)out;
        if (out_where == MRZ_MEM_DEVICE) {
            staged.resize((size_t)count);
            dst = staged.data();
        }
        const uint8_t *lit = (const uint8_t *)s1;
        for (int64_t i = 0; i < count;) {
            int64_t j = i + 1;
            while (j < count && h_org[(size_t)j] == h_org[(size_t)j - 1] + 1) j++;
            memcpy(dst + i, lit + h_org[(size_t)i], (size_t)(j - i));
            i = j;
        }
        if (out_where == MRZ_MEM_DEVICE) {
            HIPCHK(ctx, hipMemcpyAsync(out, dst, (size_t)count, hipMemcpyHostToDevice, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
        }
    }
    return MRZ_OK;
}

extern "C" int mrz_runzip_range(mrz_ctx *ctx, const void *s0, int64_t s0_len, const void *s1, int64_t s1_len, int where,
                                int chunk_bytes, int64_t first, int64_t count, void *out, int out_where,
                                mrz_range_info *info) {
    try {
        return uz_range(ctx, false, s0, s0_len, s1, s1_len, where, chunk_bytes, first, count, out, out_where, info);
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}

extern "C" int mrz_runzip_origins(mrz_ctx *ctx, const void *s0, int64_t s0_len, int64_t s1_len, int where, int chunk_bytes,
                                  int64_t first, int64_t count, int64_t *origins, int out_where, mrz_range_info *info) {
    try {
        return uz_range(ctx, true, s0, s0_len, nullptr, s1_len, where, chunk_bytes, first, count, origins, out_where, info);
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}

// bytes or origins of many ranges, packed in list order: see include/mrzgpu.h.  uz_range with a table in place of
// (first, count): one parse, one table upload, one launch.
static int uz_ranges(mrz_ctx *ctx, bool want_origins, const void *s0, int64_t s0_len, const void *s1, int64_t s1_len,
                     int where, int chunk_bytes, const mrz_byte_range *ranges, int64_t n_ranges, void *out, int out_where,
                     mrz_range_info *info) {
    if (!ctx || !s0 || s0_len < 7 || s1_len < 0 || chunk_bytes < 1 || chunk_bytes > 8) return MRZ_E_ARG;
    if (n_ranges < 0 || (n_ranges > 0 && !ranges)) return MRZ_E_ARG;
    if (!want_origins && s1_len > 0 && !s1) return MRZ_E_ARG;
    if ((where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) || (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE))
        return MRZ_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    uz_parsed ps;
    int rc = uz_parse(ctx, s0, s0_len, where, chunk_bytes, (n_ranges + 1) * (int64_t)sizeof(mrz_uz_rng), nullptr, 0, &ps);
    if (rc) return rc;
    const mrz_uz_hdr &h = ps.h;
    if (h.final_state != MRZ_UZ_END || h.error || h.lit_total > s1_len) return MRZ_E_CORRUPT;
    if (info) {
        info->chunk_len = h.out_total;
        info->total_hops = info->max_hops = 0;
    }
    std::vector<mrz_uz_rng> tab((size_t)n_ranges + 1);
    int64_t count = 0;
    for (int64_t k = 0; k < n_ranges; k++) {
        const mrz_byte_range &g = ranges[k];
        if (g.first < 0 || g.count < 0 || g.first > h.out_total || g.count > h.out_total - g.first) return MRZ_E_ARG;
        if (g.count > INT64_MAX / 8 - count) return MRZ_E_ARG;  // more than any buffer holds
        tab[(size_t)k] = mrz_uz_rng{ g.first, count };
        count += g.count;
    }
    tab[(size_t)n_ranges] = mrz_uz_rng{ 0, count };
    if (!count) return MRZ_OK;
    if (!out) return MRZ_E_ARG;

    // as in uz_range: a host-resident stream 1 stays where it is
    const bool origins = want_origins || where == MRZ_MEM_HOST;
    const bool direct = out_where == MRZ_MEM_DEVICE && origins == want_origins;
    if (direct && want_origins && ((uintptr_t)out & 7)) return MRZ_E_ARG;
    const int64_t item = origins ? 8 : 1;
    void *d_dst = out;
    if (!direct) {
        rc = mrz_grow(ctx, &ctx->d_rz_out, &ctx->rz_out_cap, count * item);
        if (rc) return rc;
        d_dst = ctx->d_rz_out;
    }
    const mrz_uz_rng *d_rng = (const mrz_uz_rng *)ps.d_extra;
    HIPCHK(ctx, hipMemcpyAsync(ps.d_extra, tab.data(), tab.size() * sizeof(mrz_uz_rng), hipMemcpyHostToDevice, s));
    int cus = 0;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    int64_t grid = (int64_t)(cus > 0 ? cus : 64) * 8;
    const int64_t blocks = (count + MRZ_UZ_THREADS - 1) / MRZ_UZ_THREADS;
    if (grid > blocks) grid = blocks;
    if (origins)
        hipLaunchKernelGGL(mrz_uz_resolve_multi_kernel<true>, dim3((unsigned)grid), dim3(MRZ_UZ_THREADS), 0, s, ps.d_rec,
                           h.nrec, (const uint8_t *)nullptr, d_rng, n_ranges, count, d_dst, ps.d_hdr);
    else
        hipLaunchKernelGGL(mrz_uz_resolve_multi_kernel<false>, dim3((unsigned)grid), dim3(MRZ_UZ_THREADS), 0, s, ps.d_rec,
                           h.nrec, (const uint8_t *)s1, d_rng, n_ranges, count, d_dst, ps.d_hdr);
    HIPCHK(ctx, hipGetLastError());
    mrz_uz_hdr after;
    HIPCHK(ctx, hipMemcpyAsync(&after, ps.d_hdr, sizeof(after), hipMemcpyDeviceToHost, s));
    std::vector<int64_t> h_org;
    if (!direct && origins && !want_origins) {  // bytes asked for, stream 1 on the host
        h_org.resize((size_t)count);
        HIPCHK(ctx, hipMemcpyAsync(h_org.data(), d_dst, (size_t)count * 8, hipMemcpyDeviceToHost, s));
    } else if (!direct)
        HIPCHK(ctx, hipMemcpyAsync(out, d_dst, (size_t)(count * item), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (after.error) return after.error == 2 ? MRZ_E_STATE : MRZ_E_CORRUPT;
    if (info) {
        info->total_hops = (int64_t)after.total_hops;
        info->max_hops = (int64_t)after.max_hops;
    }
    if (!h_org.empty()) {
        std::vector<uint8_t> staged;
        uint8_t *dst = (uint8_t *)out;
        if (out_where == MRZ_MEM_DEVICE) {
            staged.resize((size_t)count);
            dst = staged.data();
        }
        const uint8_t *lit = (const uint8_t *)s1;
        for (int64_t i = 0; i < count;) {  // runs of consecutive origins
            int64_t j = i + 1;
            while (j < count && h_org[(size_t)j] == h_org[(size_t)j - 1] + 1) j++;
            memcpy(dst + i, lit + h_org[(size_t)i], (size_t)(j - i));
            i = j;
        }
        if (out_where == MRZ_MEM_DEVICE) {
            HIPCHK(ctx, hipMemcpyAsync(out, dst, (size_t)count, hipMemcpyHostToDevice, s));
            HIPCHK(ctx, hipStreamSynchronize(s));
        }
    }
    return MRZ_OK;
}

extern "C" int mrz_runzip_ranges(mrz_ctx *ctx, const void *s0, int64_t s0_len, const void *s1, int64_t s1_len, int where,
                                 int chunk_bytes, const mrz_byte_range *ranges, int64_t n_ranges, void *out, int out_where,
                                 mrz_range_info *info) {
    try {
        return uz_ranges(ctx, false, s0, s0_len, s1, s1_len, where, chunk_bytes, ranges, n_ranges, out, out_where, info);
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}

extern "C" int mrz_runzip_origins_multi(mrz_ctx *ctx, const void *s0, int64_t s0_len, int64_t s1_len, int where,
                                        int chunk_bytes, const mrz_byte_range *ranges, int64_t n_ranges, int64_t *origins,
                                        int out_where, mrz_range_info *info) {
    try {
        return uz_ranges(ctx, true, s0, s0_len, nullptr, s1_len, where, chunk_bytes, ranges, n_ranges, origins, out_where,
                         info);
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}
