/*
 * mrzgpu_host.h -- host driver of libmrzgpu.so: the `mrzip -n` file path built
 * on the C ABI of mrzgpu.h.  It mirrors, for the rzip-only (-n) mode,
 *   void rzip_fd(rzip_control *control, int fd_in, int fd_out)   (include/rzip.h:25, src/rzip.c:807-1132)
 * together with what compress_file (src/mrzip.c:1053-1163) and the stream sink
 * (src/stream.c:771-938 open_stream_out, :1574-1590 write_stream, :1307-1349
 * flush_buffer, :1115-1305 compthread block writer, :1623-1648 close_stream_out)
 * and write_magic (src/mrzip.c:127-188) add around it, so that the bytes
 * written are identical to the reference's output file.
 *
 * mrz_control carries exactly the rzip_control fields that path reads
 * (include/mrzip_private.h:419-524); names follow the reference.
 */
#ifndef MRZGPU_HOST_H
#define MRZGPU_HOST_H

#include "mrzgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int rzip_compression_level; /* -R / -L, 1..9 (src/main.c:575) */
    int compression_level;      /* -L; only recorded in magic[18] (src/mrzip.c:171) */
    int64_t window;             /* -w, units of 100 MiB; 0 = unset (src/rzip.c:883-884) */
    int unlimited;              /* FLAG_UNLIMITED, -U (src/rzip.c:881-882) */
    int64_t ramsize;            /* control->ramsize in bytes (-m * 100 MiB or sysconf) */
    int64_t page_size;          /* control->page_size (4096) */
    int hash_code;              /* control->hash_code; only 1 (MD5, the default) is supported */
    int device;                 /* HIP device ordinal */
    int lz4_test;               /* FLAG_THRESHOLD / LZ4_TEST (-T switches it off, src/main.c:499-510): the pipeline
                                 * asks the LZ4 compressibility gate about every block */
    int threshold;              /* control->threshold, per cent (default 100, src/mrzip.c:1376) */
} mrz_control;

/* As `mrzip -n -L<level> [-w|-U] -m<ramsize>` would write it.  fd_in a regular file: the FILE form of the chunk loop
 * (size from fstat, chunks of max_chunk bytes read one at a time, src/rzip.c:864-866,915-1061), fd_out must seek.
 * fd_in anything else (a pipe): the STDIN form, see mrz_rzip_stream; the output counts as STDOUT if it cannot seek.
 * The archive is written chunk by chunk.  stats (may be NULL) receives the totals printed at -vv. */
int mrz_rzip_fd(const mrz_control *control, int fd_in, int fd_out, mrz_stats *stats);

/* The STDIN form of rzip_fd's chunk loop (mmap_stdin, src/rzip.c:700-732; the loop :915-1061 with STDIN set;
 * setup_ram, src/util.c:156-164): the size is unknown, so every chunk is max_mmap = min(page-rounded maxram,
 * max_chunk) bytes, maxram = ramsize / 3 (ramsize / 6 with to_stdout), until read() returns 0; the chunk in which
 * that happens is shrunk and carries the eof flag -- one more, EMPTY chunk when the input length is a multiple of
 * the chunk size; the stream block size is fixed at the first chunk from the bytes read so far (src/stream.c:803-914).
 * to_stdout = 0: the header is written last, with the total size (src/mrzip.c:1132).  to_stdout = 1: the header goes
 * out first (src/stream.c:1202-1205) and holds the size only if the input ended within the first chunk
 * (src/mrzip.c:137-140); nothing is ever sought, so fd_out may be a pipe.  -U (unlimited) is refused: it takes the
 * window from the file size. */
int mrz_rzip_stream(const mrz_control *control, int fd_in, int fd_out, int to_stdout, mrz_stats *stats);
/* the same with `in` standing for what read() would deliver (tests) */
int mrz_rzip_stream_buffer(const mrz_control *control, const void *in, int64_t n, int to_stdout, void **out,
                           int64_t *out_len, mrz_stats *stats, uint8_t *md5_out);

/* memory -> memory variant of the same path.  *out is malloc'd by the library
 * (release with mrz_free); md5_out (may be NULL) gets the 16 trailing bytes. */
int mrz_rzip_buffer(const mrz_control *control, const void *in, int64_t n, void **out, int64_t *out_len,
                    mrz_stats *stats, uint8_t *md5_out);
void mrz_free(void *p);

/* What `mrzip -l -L<compression_level> -p<threads>` writes for a file of n bytes (file -> file): the chunk loop and
 * sink of mrz_rzip_buffer with the LZ4 back-end behind it (compthread + lz4_compress_buf, src/stream.c:1147-1152,
 * 278-312).  Every stream block of at least 64 bytes goes through mrz_lz4_compress_batch -- all blocks of a chunk in
 * one launch -- and is framed {5, c_len, u_len, next} even when it expands (the reference has no size check there);
 * smaller blocks stay CTYPE_NONE.  The block size follows open_stream_out with two buffers per thread:
 * round_up_page(MIN(limit, MAX(limit / threads', STREAM_BUFSIZE))), limit = ramsize / 3 / 2 adjusted by the file and
 * first-chunk size as for -n, threads' = threads + 1 when threads > 1 (src/stream.c:736,797-914).  Not modelled: the
 * reference's fall-back to fewer threads / a smaller limit when its test malloc fails (machine dependent).
 * compression_level 1..2 only: above that the reference calls LZ4_compress_HC -> MRZ_E_UNSUPPORTED.  magic[18] is
 * rzip_compression_level << 4 | compression_level.  Whole-file identity with the reference's -l output is not pinned
 * by a test (the reference binary needs liblz4's sources, which it does not vendor); its pieces are: the block
 * payloads against liblz4 1.9.3, the streams and framing against the -n path. */
int mrz_rzip_buffer_lz4(const mrz_control *control, int threads, const void *in, int64_t n, void **out, int64_t *out_len,
                        mrz_stats *stats, uint8_t *md5_out);

/* chunking / block sizing rules alone (src/rzip.c:875-894, src/util.c:156-176,
 * src/stream.c:797-914 for -n): returns max_chunk, *stream_bufsize optional */
int64_t mrz_plan(const mrz_control *control, int64_t st_size, int64_t *stream_bufsize);

/* ---- back-end hand-off --------------------------------------------
 * What the reference's sink does between rzip and the back-end codecs: every stream buffer that fills
 * (stream_bufsize bytes, src/stream.c:878-914) is handed over as one block the moment it fills, DURING
 * hash_search (write_sbstream src/rzip.c:197-211 -> flush_buffer src/stream.c:1307-1349 -> compthread
 * :1115-1305); the output keeps flush order; a back-end that honours LZ4_TEST first asks lz4_compresses
 * (src/stream.c:1685-1733, called from lzma/zpaq/bzip3_compress_buf :249,167,124) whether the block is worth
 * compressing.  mrz_rzip_pipeline runs the GPU rzip stage over the chunks of `in`; as soon as a segment of a
 * chunk has been sequenced the host encodes the records that have become final (put_match / put_literal,
 * src/rzip.c:179-227) and cuts blocks; a consumer thread runs the LZ4 gate on the device for every block
 * (control->lz4_test) and then calls `fn` -- once per block, in flush order, while the GPU is still working on
 * the rest of the same chunk.  `fn` is where a back-end would compress (and frame) the block.  A non-zero
 * return of `fn` aborts the run and is returned. */
typedef struct {
    int chunk_index;      /* 0, 1, ... */
    int stream;           /* 0 = control records, 1 = literal bytes */
    int chunk_bytes;      /* width of the header fields of this chunk's blocks (src/rzip.c:1006-1008) */
    int eof;              /* this is the file's last chunk (src/rzip.c:1049) */
    int64_t chunk_size;
    int first_of_chunk;   /* first block of the chunk: the chunk header precedes it in the file */
    int lz4_verdict;      /* lz4_compresses' answer for this block: 0 = does not compress (store it), 1..100 = per
                           * cent of its size; -1 = not asked (control->lz4_test == 0, or fewer than 64 bytes:
                           * compthread only compresses blocks of >= 64 bytes, src/stream.c:1147) */
    int64_t input_final;  /* bytes of the chunk that were final (sequenced) when the block was cut */
} mrz_block_info;
typedef int (*mrz_block_fn)(void *user, const mrz_block_info *info, const uint8_t *payload, int64_t len);
int mrz_rzip_pipeline(const mrz_control *control, const void *in, int64_t n, mrz_block_fn fn, void *user,
                      mrz_stats *stats, uint8_t *md5_out);

/* `mrzip -d` of a whole -n archive held in memory: runzip_fd (src/runzip.c:332-437) over
 * runzip_chunk (:226-330), the block chains of the two streams (fill_buffer, src/stream.c:1412-1571) and the final
 * hash check (:384-412; per-chunk CRC instead when the archive carries no hash, :311-321).
 * Blocks are CTYPE_NONE (3) or CTYPE_LZ4 (5, what `mrzip -l` writes), mixed freely.  A chunk that holds LZ4 blocks has
 * their payloads uploaded as they are and decoded on the device (mrz_lz4_decompress_batch, one launch for the chunk)
 * straight into the two contiguous stream buffers, CTYPE_NONE blocks copied in between, and mrz_runzip_chunk runs on
 * that device memory: the decompressed streams do not cross the bus (exception: an archive without a size in its
 * header, written to STDOUT in several chunks, has stream 0 fetched to size the output).  A block the decoder
 * rejects (rules and the offset-0 difference: mrz_lz4_decompress_batch), c_len beyond the archive,
 * c_len > u_len + u_len/255 + 16 or u_len > 255 * c_len give MRZ_E_CORRUPT; u_len > 0x7E000000, any other ctype
 * (zstd, lzma, bzip3, zpaq) and encryption give MRZ_E_UNSUPPORTED.
 * *out is malloc'd by the library (mrz_free).  Record decoding runs on the GPU (mrz_runzip_chunk). */
int mrz_runzip_buffer(int device, const void *mrz, int64_t n, void **out, int64_t *out_len);

/* CTYPE_NONE blocks only: an archive that holds an LZ4 block gets MRZ_E_UNSUPPORTED here (mrz_runzip_buffer decodes it
 * whole).  Ranges of such an archive: mrz_runzip_buffer_range_ex below.
 * Bytes [first, first + count) of the file a -n archive decodes to, written to out_host; *file_len (may be NULL) is the
 * file's length: the header's where it carries one, otherwise the chunks are walked to the end.  Same header rules and
 * refusals as mrz_runzip_buffer (MRZ_E_UNSUPPORTED, MRZ_E_CORRUPT); first < 0, count < 0 or a range beyond the file
 * give MRZ_E_ARG, with *file_len set.  count == 0 takes out_host == NULL.
 * Per chunk, stream 0's blocks are gathered as there and stream 1 only becomes a table of its blocks; a chunk's length
 * comes from a host walk over its records.  Chunks outside the range do no device work and are not validated beyond
 * that walk; a chunk inside it is validated whole and resolved by mrz_runzip_origins, and its bytes are gathered from
 * the archive's blocks.  Behind a header that carries the size nothing past the range is looked at.
 * The MD5 / per-chunk CRC is NOT checked: either needs every byte.  Use mrz_runzip_buffer for a verified decode. */
int mrz_runzip_buffer_range(int device, const void *mrz, int64_t n, int64_t first, int64_t count, void *out_host,
                            int64_t *file_len);

/* The same range over an archive whose blocks are CTYPE_NONE or CTYPE_LZ4, mixed freely (block acceptance and its
 * refusals: mrz_runzip_buffer; header rules, *file_len, MRZ_E_ARG / MRZ_E_CORRUPT cases, the early stop behind a header
 * that carries the size and NO MD5 / CRC check: mrz_runzip_buffer_range).  `out` is host or device memory per
 * out_where; nothing beyond `count` bytes is written.  `info` may be NULL.
 * Per chunk: a stream 0 without an LZ4 block is gathered and walked on the host as above; one with an LZ4 block is put
 * together on the device, its LZ4 blocks decoded WHOLE (the parse needs every record), and the chunk's length comes
 * from that parse.  Chunks outside the range do no more.  Inside the range the origins stay on the device
 * (mrz_runzip_origins), one kernel finds per stream-1 block the lowest and highest offset an origin asks of it, and
 * only that table (8 bytes a block) comes back.  A touched LZ4 block has its payload uploaded and its first
 * `highest + 1` bytes decoded (mrz_lz4_decompress_prefix_batch, all touched blocks of the chunk in one launch); of a
 * touched CTYPE_NONE block bytes [lowest, highest] are uploaded; a second kernel gathers the range from those pieces.
 * A prefix the decoder rejects is MRZ_E_CORRUPT; a defect behind the highest origin of a block, or in a block that
 * holds no origin, is not seen.  Stream 1 never exists whole anywhere: device memory per chunk is bounded by stream 0
 * + the touched payloads + the prefixes + 9 bytes per range byte (+ 24 bytes per block). */
typedef struct {
    int64_t chunks_in_range, total_hops, max_hops;      /* as mrz_range_info, summed / maxed over the chunks */
    int64_t s0_lz4_bytes;        /* bytes of stream 0 that were LZ4-decoded (always whole blocks) */
    int64_t s1_blocks_touched;   /* stream-1 blocks holding at least one origin */
    int64_t s1_lz4_bytes;        /* sum of `want` over the touched LZ4 blocks of stream 1 */
    int64_t s1_bytes_uploaded;   /* payload bytes of stream 1 sent to the device */
} mrz_archive_range_info;
int mrz_runzip_buffer_range_ex(int device, const void *mrz, int64_t n, int64_t first, int64_t count, void *out,
                               int out_where, int64_t *file_len, mrz_archive_range_info *info);

/* Many ranges of the file in one call, over -n and -l archives alike.  `ranges` (host memory) in any order, overlapping
 * or identical ranges and count == 0 allowed; the output is packed in list order and is, byte for byte, the
 * concatenation of mrz_runzip_buffer_range_ex over the ranges.  Header rules, *file_len, MRZ_E_UNSUPPORTED,
 * MRZ_E_CORRUPT and MRZ_E_ARG follow that function: against a header that carries the size one bad range (first < 0,
 * count < 0, an end beyond the file) is MRZ_E_ARG before any device work; without a size the chunks are walked for the
 * length first.  sum(count) == 0 takes out == NULL.  Behind a header that carries the size the walk stops behind the
 * last chunk any range touches; a chunk no range touches does no device work.
 * Per touched chunk: every range is clipped to the chunk, ALL clipped parts are resolved by one
 * mrz_runzip_origins_multi -- stream 0 is parsed once per chunk, whatever the number of ranges --, the span and gather
 * kernels and the prefix decode of mrz_runzip_buffer_range_ex run once over the flat origins, and one
 * mrz_copy_device_batch moves the chunk's bytes to their places (parts that follow each other in the output are
 * gathered in place instead).
 * info: chunks_in_range counts each touched chunk once, s1_blocks_touched each block once per chunk; the hops are
 * summed / maxed over all parts; the byte counts are what was moved.
 * KNOWN COST, kept on purpose: per stream-1 block ONE interval [lowest, highest] is kept.  Two far-apart ranges in one
 * CTYPE_NONE block upload the bytes between them (for an LZ4 block the prefix is needed anyway). */
int mrz_runzip_buffer_ranges(int device, const void *mrz, int64_t n, const mrz_byte_range *ranges, int64_t n_ranges,
                             void *out, int out_where, int64_t *file_len, mrz_archive_range_info *info);

/* mrz_ar_extract (mrzgpu.h: selection, offsets, sizing call, out_cap, MRZ_AR_VERIFY, info) over an ARZIP archive that is
 * what a -n / -l .mrz (host memory) decodes to; nothing of it is decoded that is not asked for:
 *   1. bytes [0, 13) give the magic and metadata_size -- a wrong magic, a .mrz that decodes to fewer than 13 bytes or
 *      metadata beyond the decoded length are MRZ_E_CORRUPT;
 *   2. bytes [13, 13 + metadata_size) come to the host and are parsed (MRZ_E_CORRUPT as in mrz_ar_parse: every
 *      offset + size is held against the decoded length);
 *   3. the distinct selected payloads, ascending by offset, are decoded by ONE mrz_runzip_buffer_ranges call into
 *      device memory, and one mrz_copy_device_batch places duplicates and the selection's order (host output: one copy
 *      to the host, then memcpy);
 *   4. with MRZ_AR_VERIFY the hashes are taken over those device bytes.
 * The three range calls share one context but not the parse: stream 0 of a chunk that holds the head, the metadata and a
 * payload is parsed three times.  range_info (may be NULL) sums the three calls (max_hops: their maximum).  Archive
 * refusals (MRZ_E_UNSUPPORTED, MRZ_E_CORRUPT) are mrz_runzip_buffer_ranges'. */
int mrz_ar_extract_mrz(int device, const void *mrz, int64_t n, const int64_t *which, int64_t n_which, void *out,
                       int out_where, int64_t out_cap, int64_t *out_offsets, int flags, mrz_ar_extract_info *info,
                       mrz_archive_range_info *range_info);

#ifdef __cplusplus
}
#endif
#endif
