// mrz_lz4.hip -- the per-block LZ4 compressibility gate, and the LZ4 block codec (the -l back-end) further down:
// the same compressor with its bytes written out, and LZ4_decompress_safe as one wave per block.
//
// Replaces lz4_compresses (src/stream.c:1685-1733), which asks "what would
// LZ4_compress_default(buf, tmp, in_len, in_len + 1) return?" for a growing
// prefix of each stream block and never looks at the compressed bytes.  Only
// the SIZE matters, so the kernel runs the LZ4 fast-compressor state machine
// (liblz4 1.9.3 LZ4_compress_fast, acceleration 1: single-probe hash table,
// skip-strength 6, one-position look-back, immediate re-test after a match)
// and counts output bytes without producing them.
//
// One wavefront per block, hash table (8192 x u32) in LDS.  The state machine
// is sequential, the steps are wave-wide:
//   * search: 64 consecutive probes at once (positions from the skip schedule by
//     a wave prefix sum); "what did the table hold when probe i ran" is the old
//     LDS value unless an earlier probe of the batch hashed to the same cell
//     (forwarded in registers); ballot picks the first hit / end-of-input; only
//     the probes that really ran commit their table writes (last writer per cell);
//   * catch-up and match extension: 64 lanes x 1 B backwards, 64 lanes x 16 B
//     forwards with ballot + ffs;
// many blocks run concurrently (one per wave; the gate sees every block of a
// chunk's two streams).  Bit-exact with liblz4 1.9.3 sizes.
//
// Bound: latency of dependent L2 reads per match; HBM traffic = bytes tested.
#include <string.h>

#include <new>
#include <vector>

#include "mrz_ctx.h"
#include "mrz_device.h"

#define MRZ_LZ_MFLIMIT 12
#define MRZ_LZ_LASTLITERALS 5
#define MRZ_LZ_MINLEN 13
#define MRZ_LZ_MAXDIST 65535
#define MRZ_LZ_64K_LIMIT (65536 + 11)
#define MRZ_LZ_STREAM_MIN (10 * 1048576)
#ifndef MRZ_LZ_FIRST_WIDTH
#define MRZ_LZ_FIRST_WIDTH 16  // probes in the first batch of a search
#endif

__device__ __forceinline__ uint32_t mrz_lz_hash(const uint8_t *p, bool small) {
    if (small) return (mrz_ld4(p) * 2654435761u) >> (32 - 13);
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return (uint32_t)(((v << 24) * 889523592379ULL) >> (64 - 12));
}

// number of equal bytes of a[0..) and b[0..) with a limited to [.., alimit)
__device__ static int64_t mrz_lz_count(const uint8_t *src, int64_t a, int64_t b, int64_t alimit, int lane) {
    const int64_t maxf = alimit - a;
    if (maxf <= 0) return 0;
    for (int64_t base = 0;; base += 1024) {
        const int64_t off = base + lane * 16;
        int lane_len = 0;
        bool full = false;
        if (off < maxf) {
            const int64_t rem = maxf - off;
            const int lim = rem < 16 ? (int)rem : 16;
            int d;
            if (rem >= 16)
                d = mrz_first_diff16(mrz_ld16(src + a + off), mrz_ld16(src + b + off));
            else {
                d = 0;
                while (d < lim && src[a + off + d] == src[b + off + d]) d++;
            }
            lane_len = d < lim ? d : lim;
            full = lane_len == 16;
        }
        const mrz_u64 stop = __ballot(!full);
        if (stop) {
            const int fl = __ffsll((long long)stop) - 1;
            return base + (int64_t)fl * 16 + mrz_lane_read(lane_len, fl);
        }
    }
}

__device__ __forceinline__ void mrz_st16(uint8_t *p, uint4 v) { __builtin_memcpy(p, &v, 16); }

// dst[0, len) = src[0, len), the ranges apart: 64 lanes x 16 B, then the last len % 16 bytes one per lane
__device__ static void mrz_lz_copy(uint8_t *dst, const uint8_t *src, int64_t len, int lane) {
    for (int64_t off = (int64_t)lane * 16; off + 16 <= len; off += 1024) mrz_st16(dst + off, mrz_ld16(src + off));
    const int64_t t = (len & ~15ll) + lane;
    if (t < len) dst[t] = src[t];
}

// the bytes that follow a 15 in a token nibble: (rest / 255) times 255, then rest % 255
__device__ static void mrz_lz_put_len(uint8_t *dst, int64_t rest, int lane) {
    const int64_t full = rest / 255;
    for (int64_t j = lane; j < full; j += 64) dst[j] = 255;
    if (lane == 0) dst[full] = (uint8_t)(rest - full * 255);
}

// what LZ4_compress_default(src, dst, n, cap) returns (0 = does not fit).  EMIT = false only counts (the gate and
// mrz_lz4_sizes: `dst` is not touched); EMIT = true also writes liblz4 1.9.3's bytes, every store below dst + cap
// (each follows the `limited` check that liblz4 itself relies on to stay inside the buffer).
template <bool EMIT>
__device__ static int mrz_lz4_wave(const uint8_t *__restrict__ src, int n, int cap, uint32_t *tab, int lane,
                                   uint8_t *__restrict__ dst) {
    if (n <= 0) {
        if (n < 0 || cap <= 0) return 0;
        if constexpr (EMIT)
            if (lane == 0) dst[0] = 0;
        return 1;
    }
    const bool limited = cap < n + n / 255 + 16;
    const bool small = n < MRZ_LZ_64K_LIMIT;
    for (int i = lane; i < 8192; i += 64) tab[i] = 0;
    const int64_t mfl1 = (int64_t)n - MRZ_LZ_MFLIMIT + 1;
    const int64_t mlimit = (int64_t)n - MRZ_LZ_LASTLITERALS;
    const int64_t olimit = cap;
    int64_t ip = 0, anchor = 0, op = 0;
    int64_t tok = 0;  // EMIT: where the current sequence's token goes, and its literal nibble
    int tok_lit = 0;
    bool to_tail = n < MRZ_LZ_MINLEN;

    if (!to_tail) {
        if (lane == 0) tab[mrz_lz_hash(src, small)] = 0;
        ip = 1;
    }
    while (!to_tail) {
        // ---- search: probes k = 0,1,2,.. at positions given by the skip schedule
        int64_t pos0 = ip;
        int k0 = 0;
        int64_t match = 0;
        bool found = false;
        // compressible data finds its match within a few probes: the first batch of a search is 16 probes wide
        // (the all-pairs forwarding below costs `width` shuffle rounds), later ones 64
        int width = MRZ_LZ_FIRST_WIDTH;
        while (true) {
            const int k = k0 + lane;
            const bool active = lane < width;
            const int my_step = !active ? 0 : (k == 0 ? 1 : (63 + k) >> 6);
            const int incl = mrz_wave_incl_sum(my_step, lane);
            const int64_t pos = pos0 + (incl - my_step);
            const int64_t nxt = pos + my_step;
            const bool runs = active && nxt <= mfl1;  // this probe gets past `if (fwd > mflimitPlusOne) goto _last_literals`
            uint32_t h = 0xffffffffu;  // inactive lanes never equal a real cell index
            if (runs) h = mrz_lz_hash(src + pos, small);
            // table value seen by this probe: old cell unless an earlier probe of the batch wrote it
            uint32_t mi = runs ? tab[h] : 0;
            int next_same = 64;
            for (int j = 0; j < width; j++) {
                const uint32_t hj = (uint32_t)__shfl((int)h, j, MRZ_WAVE);
                const uint32_t pj = (uint32_t)__shfl((int)(uint32_t)pos, j, MRZ_WAVE);
                if (hj == h) {
                    if (j < lane) mi = pj;
                    if (j > lane && next_same == 64) next_same = j;
                }
            }
            bool hit = false;
            if (runs) {
                const bool near = small || ((int64_t)mi + MRZ_LZ_MAXDIST >= pos);
                hit = near && mrz_ld4(src + mi) == mrz_ld4(src + pos);
            }
            const mrz_u64 m_end = __ballot(active && !runs);
            const mrz_u64 m_hit = __ballot(hit);
            const int first_end = m_end ? __ffsll((long long)m_end) - 1 : width;
            const int first_hit = m_hit ? __ffsll((long long)m_hit) - 1 : 64;
            // probes [0, last_run] executed their table update
            int last_run;
            if (first_hit < first_end)
                last_run = first_hit;
            else
                last_run = first_end - 1;
            if (lane <= last_run && next_same > last_run) tab[h] = (uint32_t)pos;
            if (first_hit < first_end) {
                ip = mrz_bcast64(pos, first_hit);
                match = (int64_t)(uint32_t)mrz_lane_read((int)mi, first_hit);
                found = true;
                break;
            }
            if (first_end < width) break;  // ran out of input: last literals
            pos0 = mrz_bcast64(nxt, width - 1);
            k0 += width;
            width = 64;
        }
        if (!found) {
            to_tail = true;
            break;
        }
        // ---- catch up (look back over equal bytes) -------------------------
        {
            int64_t room = ip - anchor;
            if (match < room) room = match;  // match > lowLimit(=0)
            int64_t back = 0;
            while (back < room) {
                const int64_t j = back + lane;
                const bool eq = j < room && src[ip - 1 - j] == src[match - 1 - j];
                const mrz_u64 ne = __ballot(!eq);
                if (ne) {
                    back += __ffsll((long long)ne) - 1;
                    break;
                }
                back += 64;
            }
            ip -= back;
            match -= back;
        }
        // ---- literal run accounting ---------------------------------------
        {
            const int64_t lit = ip - anchor;
            tok = op;
            op += 1;  // token
            if (limited && op + lit + (2 + 1 + MRZ_LZ_LASTLITERALS) + lit / 255 > olimit) return 0;
            if constexpr (EMIT) {
                tok_lit = lit < 15 ? (int)lit : 15;
                if (lit >= 15) mrz_lz_put_len(dst + op, lit - 15, lane);
            }
            if (lit >= 15) op += (lit - 15) / 255 + 1;
            if constexpr (EMIT) mrz_lz_copy(dst + op, src + anchor, lit, lane);
            op += lit;
        }
        // ---- match(es): _next_match loop ------------------------------------
        while (true) {
            if constexpr (EMIT)
                if (lane == 0) {
                    dst[op] = (uint8_t)(ip - match);
                    dst[op + 1] = (uint8_t)((ip - match) >> 8);
                }
            op += 2;  // offset
            int64_t mc = mrz_lz_count(src, ip + 4, match + 4, mlimit, lane);
            ip += mc + 4;
            if (limited && op + (1 + MRZ_LZ_LASTLITERALS) + (mc + 240) / 255 > olimit) return 0;
            if constexpr (EMIT) {
                if (lane == 0) dst[tok] = (uint8_t)(tok_lit << 4 | (mc < 15 ? (int)mc : 15));
                if (mc >= 15) mrz_lz_put_len(dst + op, mc - 15, lane);
            }
            if (mc >= 15) {
                mc -= 15;
                op += mc / 255 + 1;
            }
            anchor = ip;
            if (ip >= mfl1) {
                to_tail = true;
                break;
            }
            // fill table with ip-2, then test ip immediately
            const uint32_t h2 = mrz_lz_hash(src + ip - 2, small);
            const uint32_t h = mrz_lz_hash(src + ip, small);
            uint32_t mi = 0;
            if (lane == 0) {
                tab[h2] = (uint32_t)(ip - 2);
                mi = tab[h];
                tab[h] = (uint32_t)ip;
            }
            mi = (uint32_t)mrz_lane_read((int)mi, 0);
            if ((small || (int64_t)mi + MRZ_LZ_MAXDIST >= ip) && mrz_ld4(src + mi) == mrz_ld4(src + ip)) {
                tok = op;
                tok_lit = 0;
                op += 1;  // token of a zero-literal sequence
                match = mi;
                continue;
            }
            ip++;
            break;
        }
    }
    // ---- last literals ------------------------------------------------------
    const int64_t last = (int64_t)n - anchor;
    if (limited && op + last + 1 + (last + 255 - 15) / 255 > olimit) return 0;
    if constexpr (EMIT) {
        if (lane == 0) dst[op] = (uint8_t)((last < 15 ? (int)last : 15) << 4);
        if (last >= 15) mrz_lz_put_len(dst + op + 1, last - 15, lane);
    }
    op += 1;
    if (last >= 15) op += (last - 15) / 255 + 1;
    if constexpr (EMIT) mrz_lz_copy(dst + op, src + anchor, last, lane);
    op += last;
    return (int)op;
}

__device__ __forceinline__ int mrz_lz4_size_wave(const uint8_t *__restrict__ src, int n, int cap, uint32_t *tab,
                                                 int lane) {
    return mrz_lz4_wave<false>(src, n, cap, tab, lane, nullptr);
}

// sizes[i] = LZ4_compress_default size of block i with dst capacity lens[i] + 1
__global__ __launch_bounds__(64) void mrz_lz4_sizes_kernel(const uint8_t *const *__restrict__ bufs,
                                                           const int *__restrict__ lens, int count,
                                                           int *__restrict__ sizes) {
    __shared__ uint32_t tab[8192];
    const int i = blockIdx.x;
    if (i >= count) return;
    const int r = mrz_lz4_size_wave(bufs[i], lens[i], lens[i] + 1, tab, threadIdx.x);
    if (threadIdx.x == 0) sizes[i] = r;
}

// lz4_compresses (src/stream.c:1685-1733) for block blockIdx.x
__global__ __launch_bounds__(64) void mrz_lz4_gate_kernel(const uint8_t *const *__restrict__ bufs,
                                                          const int64_t *__restrict__ lens, int count, int threshold,
                                                          int *__restrict__ results) {
    __shared__ uint32_t tab[8192];
    const int i = blockIdx.x;
    if (i >= count) return;
    const uint8_t *s_buf = bufs[i];
    int test_len = (int)lens[i];
    int in_len = test_len < MRZ_LZ_STREAM_MIN ? test_len : MRZ_LZ_STREAM_MIN;
    int buftest = in_len;
    double pct = 101;
    while (test_len > 0) {
        const int r = mrz_lz4_size_wave(s_buf, in_len, in_len + 1, tab, threadIdx.x);
        if (r > 0) {
            pct = 100 * ((double)r / (double)in_len);
            if (r < in_len * ((double)threshold / 100)) break;
        }
        test_len -= in_len;
        if (test_len > 0) {
            buftest += in_len;
            if (buftest < MRZ_LZ_STREAM_MIN) buftest <<= 1;
            in_len = test_len < buftest ? test_len : buftest;
        }
    }
    if (threadIdx.x == 0) results[i] = (int)(pct > threshold ? 0 : pct < 1 ? pct + 1 : pct);
}

// outs[i][0, out_lens[i]) = LZ4_compress_default(bufs[i], lens[i]) into caps[i] bytes; out_lens[i] = 0: does not fit
__global__ __launch_bounds__(64) void mrz_lz4_compress_kernel(const uint8_t *const *__restrict__ bufs,
                                                              const int64_t *__restrict__ lens,
                                                              uint8_t *const *__restrict__ outs,
                                                              const int64_t *__restrict__ caps, int count,
                                                              int64_t *__restrict__ out_lens) {
    __shared__ uint32_t tab[8192];
    const int i = blockIdx.x;
    if (i >= count) return;
    const int n = (int)lens[i];
    const int64_t bound = (int64_t)n + n / 255 + 16;  // a larger capacity changes nothing
    const int cap = (int)(caps[i] < bound ? caps[i] : bound);
    const int r = mrz_lz4_wave<true>(bufs[i], n, cap, tab, threadIdx.x, outs[i]);
    if (threadIdx.x == 0) out_lens[i] = r;
}

// ---- decoder ---------------------------------------------------------------------
// LZ4_decompress_safe(src, dst, c_len, u_len) of liblz4 1.9.3 as one wave: the sequences are walked one after the
// other (every value that steers the walk is wave-uniform), the copies are wave-wide.  Returns 0 iff liblz4 would
// return u_len, with one deliberate difference: an offset of 0 is a reject (liblz4 copies bytes it has not written).
// The accept rules are those of liblz4's loop, line by line, its `shortcut` included -- it is the one place where a
// match may end inside the last 5 bytes.  Independently of them no load leaves [src, src + c_len) and no store leaves
// [dst, dst + u_len): every length is compared with what is left of both buffers before it is used.
//
// A match reads bytes that this wave stored for earlier sequences, possibly the previous instruction's.  The stores
// of one wave are ordered before its later loads by the workgroup barrier (vmcnt(0) + s_barrier; the block is this one
// wave), as in mrz_uz_decode_kernel; `synced` skips the barrier when the source lies in bytes that are ordered already.
//
// PREFIX: the first `want` bytes only (0 <= want <= u_len; the whole-block instantiation ignores `want`).  The walk and
// its accept rules are the same, against the block's real c_len and u_len.  The copy -- a literal run or a match --
// with which the produced count reaches `want` is validated as the full decoder validates it before it copies (lengths
// against both buffers, the last-sequence rule and, for that last sequence, that it ends at u_len; for a match the
// offset, the u_len - 5 rule or the shortcut's conditions); then it is cut at `want` and the wave returns 0.  Exactly
// `want` bytes are stored, nothing at or beyond dst + want, and no load leaves [src, src + c_len).  want == u_len is
// the full decoder: it walks on to the end of the input.  want == 0 < u_len touches nothing and returns 0.
// THE CONTRACT: a reject that the full walk meets only behind that copy is not seen.  (Range decode makes the same
// trade for the CRC.)
template <bool PREFIX>
__device__ static int mrz_lz4_decode_wave(const uint8_t *__restrict__ src, int64_t c_len, uint8_t *dst, int64_t u_len,
                                          int64_t want, int lane) {
    if constexpr (PREFIX)
        if (want == 0 && u_len > 0) return 0;
    // where the walk ends: a whole block is walked to the end of its input, as the full decoder walks it
    const int64_t cut = PREFIX && want < u_len ? want : u_len + 1;
    (void)cut;
    if (c_len <= 0 || u_len < 0) return 1;
    if (u_len == 0) return c_len == 1 && src[0] == 0 ? 0 : 1;
    int64_t ip = 0, op = 0, synced = 0;
    while (true) {
        if (ip >= c_len) return 1;
        const int token = mrz_uni(src[ip]);
        ip++;
        int64_t lit = token >> 4;
        int64_t ml = token & 15;
        int64_t offset;
        bool checked = false;  // the shortcut: 0..14 literals and a short match far from both ends
        if (lit != 15 && ip < c_len - 16 && op <= u_len - 32) {
            if constexpr (PREFIX)
                if (op + lit >= cut) {
                    for (int64_t j = lane; j < cut - op; j += 64) dst[op + j] = src[ip + j];
                    return 0;
                }
            for (int64_t j = lane; j < lit; j += 64) dst[op + j] = src[ip + j];
            ip += lit;
            op += lit;
            offset = mrz_uni((int)src[ip] | (int)src[ip + 1] << 8);
            ip += 2;
            checked = ml != 15 && offset >= 8 && offset <= op;
        } else {
            if (lit == 15) {  // 255 255 .. x; liblz4 stops reading 15 bytes before the end without calling it an error
                const int64_t stop_at = c_len - 15;
                if (ip >= stop_at) return 1;
                while (true) {
                    const int64_t pos = ip + lane;
                    const bool valid = pos < stop_at;
                    const int b = valid ? src[pos] : 0;
                    const mrz_u64 stop = __ballot(b != 255);
                    if (!stop) {
                        lit += 255 * 64;
                        ip += 64;
                        continue;
                    }
                    const int f = __ffsll((long long)stop) - 1;
                    lit += 255 * f;
                    ip += f;
                    if (ip < stop_at) {
                        lit += mrz_lane_read(b, f);
                        ip++;
                    }
                    break;
                }
            }
            if (lit > c_len - ip || lit > u_len - op) return 1;
            if (op + lit > u_len - 12 || ip + lit > c_len - 8) {  // must be the last sequence
                if (ip + lit != c_len) return 1;
                if constexpr (PREFIX)
                    if (op + lit >= cut) {
                        if (op + lit != u_len) return 1;
                        mrz_lz_copy(dst + op, src + ip, cut - op, lane);
                        return 0;
                    }
                mrz_lz_copy(dst + op, src + ip, lit, lane);
                return op + lit == u_len ? 0 : 1;
            }
            if constexpr (PREFIX)
                if (op + lit >= cut) {
                    mrz_lz_copy(dst + op, src + ip, cut - op, lane);
                    return 0;
                }
            mrz_lz_copy(dst + op, src + ip, lit, lane);
            ip += lit;
            op += lit;
            offset = mrz_uni((int)src[ip] | (int)src[ip + 1] << 8);
            ip += 2;
        }
        if (ml == 15) {  // liblz4 refuses a length byte among the last 5 bytes, the closing one included
            const int64_t stop_at = c_len - 5;
            while (true) {
                const int64_t pos = ip + lane;
                const bool valid = pos < stop_at;
                const int b = valid ? src[pos] : 0;
                const mrz_u64 stop = __ballot(b != 255);
                if (!stop) {
                    ml += 255 * 64;
                    ip += 64;
                    continue;
                }
                const int f = __ffsll((long long)stop) - 1;
                if (ip + f >= stop_at) return 1;
                ml += 255 * f + mrz_lane_read(b, f);
                ip += f + 1;
                break;
            }
        }
        ml += 4;
        if (offset == 0 || offset > op) return 1;
        if (ml > u_len - op) return 1;
        if (!checked && op + ml > u_len - 5) return 1;
        const int64_t from = op - offset;
        if constexpr (PREFIX)
            if (ml > cut - op) ml = cut - op;  // validated whole, copied as far as `want`
        if ((offset < ml ? op : from + ml) > synced) {
            __syncthreads();
            synced = op;
        }
        if (offset >= ml)
            mrz_lz_copy(dst + op, dst + from, ml, lane);
        else {  // periodic: every byte comes from the first period, which is stored and ordered
            const int period = (int)offset, step = 64 % period;
            int idx = lane % period;
            for (int64_t j = lane; j < ml; j += 64) {
                dst[op + j] = dst[from + idx];
                idx += step;
                if (idx >= period) idx -= period;
            }
        }
        op += ml;
        if constexpr (PREFIX)
            if (op >= cut) return 0;
    }
}

__global__ __launch_bounds__(64) void mrz_lz4_decode_kernel(const uint8_t *const *__restrict__ bufs,
                                                            const int64_t *__restrict__ c_lens,
                                                            uint8_t *const *__restrict__ outs,
                                                            const int64_t *__restrict__ u_lens, int count,
                                                            int *__restrict__ status) {
    const int i = blockIdx.x;
    if (i >= count) return;
    const int r = mrz_lz4_decode_wave<false>(bufs[i], c_lens[i], outs[i], u_lens[i], u_lens[i], threadIdx.x);
    if (threadIdx.x == 0) status[i] = r ? MRZ_E_CORRUPT : 0;
}

// the first wants[i] bytes of every block
__global__ __launch_bounds__(64) void mrz_lz4_decode_prefix_kernel(const uint8_t *const *__restrict__ bufs,
                                                                   const int64_t *__restrict__ c_lens,
                                                                   uint8_t *const *__restrict__ outs,
                                                                   const int64_t *__restrict__ u_lens,
                                                                   const int64_t *__restrict__ wants, int count,
                                                                   int *__restrict__ status) {
    const int i = blockIdx.x;
    if (i >= count) return;
    const int r = mrz_lz4_decode_wave<true>(bufs[i], c_lens[i], outs[i], u_lens[i], wants[i], threadIdx.x);
    if (threadIdx.x == 0) status[i] = r ? MRZ_E_CORRUPT : 0;
}

// ---- host side -----------------------------------------------------------------
// scratch layout: ptrs[count] (8 B) | lens[count] (8 B) | results[count] (4 B, padded) | staged block bytes
static int mrz_lz4_prepare(mrz_ctx *ctx, const void *const *bufs, const int64_t *lens, int count, int where,
                           const uint8_t ***d_ptrs, int64_t **d_lens, int **d_res) {
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        if (lens[i] < 0 || lens[i] > 0x7E000000ll || (lens[i] && !bufs[i])) return MRZ_E_ARG;
        total += (lens[i] + 31) & ~15ll;
    }
    const int64_t hdr = (int64_t)count * 16 + (((int64_t)count * 4 + 15) & ~15ll);
    const int64_t need = hdr + (where == MRZ_MEM_HOST ? total : 0) + 64;
    if (need > ctx->lz4_scratch_cap || !ctx->lz4_scratch) {
        if (ctx->lz4_scratch) hipFree(ctx->lz4_scratch);
        ctx->lz4_scratch = nullptr;
        ctx->lz4_scratch_cap = 0;
        void *p = nullptr;
        if (hipMalloc(&p, (size_t)need) != hipSuccess) return MRZ_E_NOMEM;
        ctx->lz4_scratch = p;
        ctx->lz4_scratch_cap = need;
    }
    uint8_t *base = (uint8_t *)ctx->lz4_scratch;
    *d_ptrs = (const uint8_t **)base;
    *d_lens = (int64_t *)(base + (int64_t)count * 8);
    *d_res = (int *)(base + (int64_t)count * 16);
    uint8_t *d_data = base + hdr;
    const uint8_t **h_ptrs = (const uint8_t **)malloc((size_t)count * sizeof(void *));
    if (!h_ptrs) return MRZ_E_NOMEM;
    hipError_t e = hipSuccess;
    int64_t off = 0;
    for (int i = 0; i < count && e == hipSuccess; i++) {
        if (where == MRZ_MEM_HOST) {
            h_ptrs[i] = d_data + off;
            if (lens[i]) e = hipMemcpyAsync(d_data + off, bufs[i], (size_t)lens[i], hipMemcpyHostToDevice, ctx->stream);
            off += (lens[i] + 31) & ~15ll;
        } else
            h_ptrs[i] = (const uint8_t *)bufs[i];
    }
    if (e == hipSuccess) e = hipMemcpyAsync(*d_ptrs, h_ptrs, (size_t)count * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(*d_lens, lens, (size_t)count * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // h_ptrs / lens are host temporaries
    free(h_ptrs);
    if (e != hipSuccess) {
        ctx->last_err = e;
        return MRZ_E_HIP;
    }
    return MRZ_OK;
}

extern "C" int mrz_lz4_compresses_batch(mrz_ctx *ctx, const void *const *bufs, const int64_t *lens, int count,
                                        int where, int threshold, int *results) {
    if (!ctx || count < 0 || (count && (!bufs || !lens || !results))) return MRZ_E_ARG;
    if (where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    if (!count) return MRZ_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint8_t **d_ptrs;
    int64_t *d_lens;
    int *d_res;
    int rc = mrz_lz4_prepare(ctx, bufs, lens, count, where, &d_ptrs, &d_lens, &d_res);
    if (rc) return rc;
    hipLaunchKernelGGL(mrz_lz4_gate_kernel, dim3((unsigned)count), dim3(64), 0, ctx->stream,
                       (const uint8_t *const *)d_ptrs, (const int64_t *)d_lens, count, threshold, d_res);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(results, d_res, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MRZ_OK;
}

extern "C" int mrz_lz4_compresses(mrz_ctx *ctx, const void *s_buf, int64_t s_len, int where, int threshold,
                                  int *result) {
    const void *bufs[1] = { s_buf };
    return mrz_lz4_compresses_batch(ctx, bufs, &s_len, 1, where, threshold, result);
}

extern "C" int mrz_lz4_sizes(mrz_ctx *ctx, const void *const *bufs, const int *lens, int count, int where,
                             int *sizes) {
    if (!ctx || count < 0 || (count && (!bufs || !lens || !sizes))) return MRZ_E_ARG;
    if (where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    if (!count) return MRZ_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *l64 = (int64_t *)malloc((size_t)count * 8);
    if (!l64) return MRZ_E_NOMEM;
    for (int i = 0; i < count; i++) l64[i] = lens[i];
    const uint8_t **d_ptrs;
    int64_t *d_lens;
    int *d_res;
    int rc = mrz_lz4_prepare(ctx, bufs, l64, count, where, &d_ptrs, &d_lens, &d_res);
    free(l64);
    if (rc) return rc;
    // the sizes kernel wants 32-bit lengths: reuse the results area after a conversion on the host side
    int *h32 = (int *)malloc((size_t)count * sizeof(int));
    if (!h32) return MRZ_E_NOMEM;
    memcpy(h32, lens, (size_t)count * sizeof(int));
    int *d_len32 = (int *)d_lens;  // 8 B per entry reserved, 4 B used
    hipError_t e = hipMemcpyAsync(d_len32, h32, (size_t)count * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    free(h32);
    if (e != hipSuccess) {
        ctx->last_err = e;
        return MRZ_E_HIP;
    }
    hipLaunchKernelGGL(mrz_lz4_sizes_kernel, dim3((unsigned)count), dim3(64), 0, ctx->stream,
                       (const uint8_t *const *)d_ptrs, (const int *)d_len32, count, d_res);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(sizes, d_res, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MRZ_OK;
}

// ---- the block codec ---------------------------------------------------------------
extern "C" int64_t mrz_lz4_bound(int64_t n) {
    if (n < 0 || n > 0x7E000000ll) return -1;
    return n + n / 255 + 16;
}

// scratch of at least `need` bytes (contents are not kept)
static int mrz_lz4_reserve(mrz_ctx *ctx, int64_t need) {
    if (need <= ctx->lz4_scratch_cap && ctx->lz4_scratch) return MRZ_OK;
    if (ctx->lz4_scratch) hipFree(ctx->lz4_scratch);
    ctx->lz4_scratch = nullptr;
    ctx->lz4_scratch_cap = 0;
    void *p = nullptr;
    if (hipMalloc(&p, (size_t)need) != hipSuccess) return MRZ_E_NOMEM;
    ctx->lz4_scratch = p;
    ctx->lz4_scratch_cap = need;
    return MRZ_OK;
}

// Shared by both directions.  scratch layout: in ptrs | in lens | out ptrs | out lens | results | extra (8 B per block
// each) | staged inputs (where == host) | staged outputs (out_where == host), every block on a 16-byte boundary.
// in_lens[i] bytes are read from bufs[i]; out_room[i] bytes may be written at outs[i]; `extra` (may be null) is one
// more column of the caller's (the prefix decode's u_lens).
struct mrz_lz4_job {
    uint8_t *base;
    int64_t in_at, out_at;
    std::vector<const uint8_t *> in_ptr;
    std::vector<uint8_t *> out_ptr;
};

static int mrz_lz4_stage(mrz_ctx *ctx, mrz_lz4_job &job, const void *const *bufs, const int64_t *in_lens, int count,
                         int where, void *const *outs, const int64_t *out_room, int out_where,
                         const int64_t *extra = nullptr) {
    int64_t in_total = 0, out_total = 0;
    for (int i = 0; i < count; i++) {
        in_total += (in_lens[i] + 31) & ~15ll;
        out_total += (out_room[i] + 31) & ~15ll;
    }
    const int64_t hdr = (int64_t)count * 48;
    job.in_at = (hdr + 15) & ~15ll;
    job.out_at = job.in_at + (where == MRZ_MEM_HOST ? in_total : 0);
    const int rc = mrz_lz4_reserve(ctx, job.out_at + (out_where == MRZ_MEM_HOST ? out_total : 0) + 64);
    if (rc) return rc;
    job.base = (uint8_t *)ctx->lz4_scratch;
    job.in_ptr.resize((size_t)count);
    job.out_ptr.resize((size_t)count);
    hipError_t e = hipSuccess;
    int64_t in_off = job.in_at, out_off = job.out_at;
    for (int i = 0; i < count && e == hipSuccess; i++) {
        if (where == MRZ_MEM_HOST) {
            job.in_ptr[(size_t)i] = job.base + in_off;
            if (in_lens[i])
                e = hipMemcpyAsync(job.base + in_off, bufs[i], (size_t)in_lens[i], hipMemcpyHostToDevice, ctx->stream);
            in_off += (in_lens[i] + 31) & ~15ll;
        } else
            job.in_ptr[(size_t)i] = (const uint8_t *)bufs[i];
        if (out_where == MRZ_MEM_HOST) {
            job.out_ptr[(size_t)i] = job.base + out_off;
            out_off += (out_room[i] + 31) & ~15ll;
        } else
            job.out_ptr[(size_t)i] = (uint8_t *)outs[i];
    }
    const size_t col = (size_t)count * 8;
    if (e == hipSuccess) e = hipMemcpyAsync(job.base, job.in_ptr.data(), col, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(job.base + col, in_lens, col, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(job.base + 2 * col, job.out_ptr.data(), col, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(job.base + 3 * col, out_room, col, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && extra) e = hipMemcpyAsync(job.base + 5 * col, extra, col, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the host arrays are the caller's and ours
    if (e != hipSuccess) {
        ctx->last_err = e;
        return MRZ_E_HIP;
    }
    return MRZ_OK;
}

static int mrz_lz4_batch_args(mrz_ctx *ctx, const void *const *bufs, const int64_t *a, int count, int where,
                              void *const *outs, const int64_t *b, int out_where, const void *res) {
    if (!ctx || count < 0 || (count && (!bufs || !a || !outs || !b || !res))) return MRZ_E_ARG;
    if (where != MRZ_MEM_HOST && where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    if (out_where != MRZ_MEM_HOST && out_where != MRZ_MEM_DEVICE) return MRZ_E_ARG;
    return MRZ_OK;
}

extern "C" int mrz_lz4_compress_batch(mrz_ctx *ctx, const void *const *bufs, const int64_t *lens, int count, int where,
                                      void *const *outs, const int64_t *out_caps, int out_where, int64_t *out_lens) {
    int rc = mrz_lz4_batch_args(ctx, bufs, lens, count, where, outs, out_caps, out_where, out_lens);
    if (rc) return rc;
    if (!count) return MRZ_OK;
    try {
        // no block needs more than mrz_lz4_bound(n) bytes: stage (and let the kernel see) no more than that
        std::vector<int64_t> room((size_t)count);
        for (int i = 0; i < count; i++) {
            if (lens[i] < 0 || lens[i] > 0x7E000000ll || (lens[i] && !bufs[i])) return MRZ_E_ARG;
            if (out_caps[i] < 0 || (out_caps[i] && !outs[i])) return MRZ_E_ARG;
            const int64_t bound = mrz_lz4_bound(lens[i]);
            room[(size_t)i] = out_caps[i] < bound ? out_caps[i] : bound;
        }
        HIPCHK(ctx, hipSetDevice(ctx->device));
        mrz_lz4_job job;
        rc = mrz_lz4_stage(ctx, job, bufs, lens, count, where, outs, room.data(), out_where);
        if (rc) return rc;
        const size_t col = (size_t)count * 8;
        int64_t *d_res = (int64_t *)(job.base + 4 * col);
        hipLaunchKernelGGL(mrz_lz4_compress_kernel, dim3((unsigned)count), dim3(64), 0, ctx->stream,
                           (const uint8_t *const *)job.base, (const int64_t *)(job.base + col),
                           (uint8_t *const *)(job.base + 2 * col), (const int64_t *)(job.base + 3 * col), count, d_res);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(out_lens, d_res, col, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (out_where == MRZ_MEM_HOST) {
            for (int i = 0; i < count; i++)
                if (out_lens[i] > 0)
                    HIPCHK(ctx, hipMemcpyAsync(outs[i], job.out_ptr[(size_t)i], (size_t)out_lens[i],
                                               hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
    return MRZ_OK;
}

extern "C" int mrz_lz4_decompress_batch(mrz_ctx *ctx, const void *const *bufs, const int64_t *c_lens, int count,
                                        int where, void *const *outs, const int64_t *u_lens, int out_where,
                                        int32_t *status) {
    int rc = mrz_lz4_batch_args(ctx, bufs, c_lens, count, where, outs, u_lens, out_where, status);
    if (rc) return rc;
    if (!count) return MRZ_OK;
    try {
        for (int i = 0; i < count; i++) {
            if (c_lens[i] < 0 || c_lens[i] > 0x7E000000ll || (c_lens[i] && !bufs[i])) return MRZ_E_ARG;
            if (u_lens[i] < 0 || u_lens[i] > 0x7E000000ll || (u_lens[i] && !outs[i])) return MRZ_E_ARG;
        }
        HIPCHK(ctx, hipSetDevice(ctx->device));
        mrz_lz4_job job;
        rc = mrz_lz4_stage(ctx, job, bufs, c_lens, count, where, outs, u_lens, out_where);
        if (rc) return rc;
        const size_t col = (size_t)count * 8;
        int *d_res = (int *)(job.base + 4 * col);
        hipLaunchKernelGGL(mrz_lz4_decode_kernel, dim3((unsigned)count), dim3(64), 0, ctx->stream,
                           (const uint8_t *const *)job.base, (const int64_t *)(job.base + col),
                           (uint8_t *const *)(job.base + 2 * col), (const int64_t *)(job.base + 3 * col), count, d_res);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(status, d_res, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (out_where == MRZ_MEM_HOST) {  // a rejected block's bytes are unspecified: they stay on the device
            for (int i = 0; i < count; i++)
                if (!status[i] && u_lens[i])
                    HIPCHK(ctx, hipMemcpyAsync(outs[i], job.out_ptr[(size_t)i], (size_t)u_lens[i],
                                               hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
    return MRZ_OK;
}

extern "C" int mrz_lz4_decompress_prefix_batch(mrz_ctx *ctx, const void *const *bufs, const int64_t *c_lens, int count,
                                               int where, void *const *outs, const int64_t *u_lens, const int64_t *wants,
                                               int out_where, int32_t *status) {
    int rc = mrz_lz4_batch_args(ctx, bufs, c_lens, count, where, outs, u_lens, out_where, status);
    if (rc) return rc;
    if (count && !wants) return MRZ_E_ARG;
    if (!count) return MRZ_OK;
    try {
        for (int i = 0; i < count; i++) {
            if (c_lens[i] < 0 || c_lens[i] > 0x7E000000ll || (c_lens[i] && !bufs[i])) return MRZ_E_ARG;
            if (u_lens[i] < 0 || u_lens[i] > 0x7E000000ll) return MRZ_E_ARG;
            if (wants[i] < 0 || wants[i] > u_lens[i] || (wants[i] && !outs[i])) return MRZ_E_ARG;
        }
        HIPCHK(ctx, hipSetDevice(ctx->device));
        mrz_lz4_job job;
        rc = mrz_lz4_stage(ctx, job, bufs, c_lens, count, where, outs, wants, out_where, u_lens);
        if (rc) return rc;
        const size_t col = (size_t)count * 8;
        int *d_res = (int *)(job.base + 4 * col);
        hipLaunchKernelGGL(mrz_lz4_decode_prefix_kernel, dim3((unsigned)count), dim3(64), 0, ctx->stream,
                           (const uint8_t *const *)job.base, (const int64_t *)(job.base + col),
                           (uint8_t *const *)(job.base + 2 * col), (const int64_t *)(job.base + 5 * col),
                           (const int64_t *)(job.base + 3 * col), count, d_res);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(status, d_res, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (out_where == MRZ_MEM_HOST) {  // a rejected block's bytes are unspecified: they stay on the device
            for (int i = 0; i < count; i++)
                if (!status[i] && wants[i])
                    HIPCHK(ctx, hipMemcpyAsync(outs[i], job.out_ptr[(size_t)i], (size_t)wants[i], hipMemcpyDeviceToHost,
                                               ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
    return MRZ_OK;
}
