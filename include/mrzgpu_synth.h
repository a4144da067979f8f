/* mrzgpu_synth.h -- reproducible workload streams built in device memory (libmrzgpu.so).
 *
 * Not an interface of the reference (those are in mrzgpu.h and mrzgpu_host.h): these functions make the inputs that the
 * tests and measurements of this project run on.  Every byte of a stream is a pure function of (seed, position), in
 * integer arithmetic only, so the host reference (modern_rzip_amd.workloads.synth_*) and the kernels
 * (csrc/mrz_synth.hip) agree bit for bit, any byte range can be built without the bytes before it, and a hash of a
 * stream -- or of the matcher's output on it -- can be committed.
 *
 * THE DEFINITION (normative; all arithmetic modulo 2^64 unless a type says otherwise)
 *
 *   G = 0x9E3779B97F4A7C15   M1 = 0xBF58476D1CE4E5B9   M2 = 0x94D049BB133111EB
 *   mix(z):   z ^= z >> 30;  z *= M1;  z ^= z >> 27;  z *= M2;  z ^= z >> 31      (the splitmix64 finaliser)
 *   key(seed, stream)    = mix(seed + G * (stream + 1))
 *   rnd(seed, stream, i) = mix(key(seed, stream) + G * (i + 1))
 *   e.g. rnd(1, 0, 0) = 0x5e41ab087439611e,  rnd(2^64 - 1, 9, 12345678901234) = 0x0626a736abe0a30c
 *
 *   streams: NOISE 0, WORD 1, VLEN 2, VCHAR 3, KIND 4, SIZE_E 5, SIZE_M 6, CSEED 7, DUP 8, VOCAB 9
 *
 *   noise(seed):  byte j is byte j & 7 (little-endian) of rnd(seed, NOISE, j >> 3).
 *
 *   vocabulary(vocab_seed):  5000 words; word w has 2 + rnd(vocab_seed, VLEN, w) % 9 letters (2..10), letter c of it is
 *       'a' + rnd(vocab_seed, VCHAR, 10 * w + c) % 26.
 *   cum[r] = sum over i <= r of floor(2^28 / (i + 1)), r < 5000  (Zipf 1/rank; cum[4999] = 2441286195 < 2^32)
 *   text(seed, vocab_seed):  word k (k = 0, 1, ...) is the vocabulary's word of rank r = the first r with
 *       cum[r] > rnd(seed, WORD, k) % cum[4999], followed by '\n' if (k + 1) % 20000 == 0 and by ' ' otherwise.
 *       The text is the concatenation.
 *
 *   tar(seed):  member m (m = 0, 1, ...) draws kind = rnd(seed, KIND, m) % 100, e = 10 + rnd(seed, SIZE_E, m) % 12 and
 *       size = (1 << e) + rnd(seed, SIZE_M, m) % (1 << e)  (log-uniform, 1 KiB to 4 MiB).
 *         kind < 60 or m == 0:  the first `size` bytes of text(rnd(seed, CSEED, m), rnd(seed, VOCAB, 0));
 *         kind < 85:            the first `size` bytes of noise(rnd(seed, CSEED, m));
 *         otherwise:            an exact duplicate of member rnd(seed, DUP, m) % m (its size and content; a duplicate
 *                               of a duplicate is a duplicate of the original).
 *       Members follow each other, each zero-padded to a multiple of 512 bytes.
 *
 * A stream is endless; callers cut it.  The members of tar(seed) are listed on the host (workloads.synth_tar_plan) as
 * mrz_synth_member descriptors; a duplicate carries its original's kind, size and seed and is REGENERATED, not copied,
 * which is what makes a byte range independent of the bytes before it. */
#ifndef MRZGPU_SYNTH_H
#define MRZGPU_SYNTH_H

#include <stdint.h>

#include "mrzgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MRZ_SYNTH_TEXT = 0, MRZ_SYNTH_NOISE = 1 };

/* one member of a tar stream (32 bytes; numpy: workloads.SYNTH_MEMBER) */
typedef struct mrz_synth_member {
    int64_t dst;    /* offset of the member in the stream */
    int64_t size;   /* bytes of content (> 0); the bytes up to the next member's dst are zero */
    uint64_t seed;  /* content seed: text(seed, vocab_seed) or noise(seed) */
    int32_t kind;   /* MRZ_SYNTH_TEXT / MRZ_SYNTH_NOISE */
    int32_t origin; /* index of the member this one duplicates, -1 if none (informative; not read here) */
} mrz_synth_member;

/* Each call fills DEVICE memory [d_out, d_out + len) with bytes [start, start + len) of its stream, on the ctx's stream,
 * and returns when that is done.  d_out needs no alignment.  Returns MRZ_OK or a negative MRZ_E_ code. */

int mrz_synth_noise(mrz_ctx *ctx, void *d_out, int64_t start, int64_t len, uint64_t seed);

/* the first len bytes of text(seed, vocab_seed) */
int mrz_synth_text(mrz_ctx *ctx, void *d_out, int64_t len, uint64_t seed, uint64_t vocab_seed);

/* plan: n_members descriptors in HOST memory, dst ascending, members disjoint; the range must end at or before the last
 * member's end rounded up to 512 (MRZ_E_ARG otherwise).  Bytes of the range that no member covers are zero. */
int mrz_synth_tar(mrz_ctx *ctx, void *d_out, int64_t start, int64_t len, const mrz_synth_member *plan, int64_t n_members,
                  uint64_t vocab_seed);

#ifdef __cplusplus
}
#endif
#endif
