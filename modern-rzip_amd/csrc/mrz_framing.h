// mrz_framing.h -- the framing of a -n / -l archive as the compress-side entry points write it: the sizes of chunks and
// stream blocks, the magic header, the cutter that turns two streams into blocks, the chunk writer with its block
// headers and `next` pointers, the record encoders, the two forms of the chunk loop's input and the archive as a whole.
// Everything that writes archive bytes or decides a size is here, and nothing else: host code without a HIP call or
// include and without mrz_ctx, so that tests/c/framing_test.cpp drives it on its own, as mrz_archive.h is for the bytes
// read.  The driver (mrz_host.hip) owns the contexts, the threads and the device work.  What is written must be
// byte-identical to the reference's output file.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <functional>
#include <vector>

#include "../../include/mrzgpu_host.h"  // mrz_control (and the MRZ_E_* codes of mrzgpu.h)
#include "mrz_archive.h"                // MRZ_CTYPE_*, kLz4MaxInput: defined once for both sides

namespace mrz_framing {

// ---- sizes --------------------------------------------------------------------------------------------------------
const int64_t kMiB = 1048576;
const int64_t kStreamMin = 10 * kMiB;   // STREAM_BUFSIZE, include/mrzip_private.h:27
const int64_t kChunkUnit = 100 * kMiB;  // CHUNK_MULTIPLE, src/rzip.c:46

inline int64_t page_of(const mrz_control *ctl) { return ctl->page_size > 0 ? ctl->page_size : 4096; }
inline int64_t page_floor(int64_t v, int64_t page) {  // round_to_page, src/util.c:166-169
    v -= v % page;
    return v ? v : page;
}
inline int64_t page_ceil(int64_t v, int64_t page) {  // round_up_page, src/util.c:171-176
    const int64_t r = v % page;
    return r ? v + page - r : v;
}
inline int64_t at_least_page(int64_t v, int64_t page) { return v < page ? page : v; }  // src/stream.c:779-780

// The stream block size of open_stream_out (src/stream.c:797-914): `limit` starts at the usable ram, is adjusted by
// the file (:803-805) and by the first chunk (chunk_limit, :878-881), and then the last branch of :913-914 divides it
// among the threads.  With one thread that branch leaves `limit` as it is.  Not modelled: the reduction of threads and
// the shrinking of `limit` when a test malloc of limit + overhead * threads fails (:882-897) -- both depend on the
// machine, not on the input.
inline int64_t stream_bufsize(int64_t usable, int64_t st_size, int64_t chunk_limit, int64_t nthreads, int64_t page) {
    int64_t limit = usable;
    if (st_size > 0 && st_size < limit)
        limit = st_size > kStreamMin ? st_size : kStreamMin;
    else if (limit > chunk_limit)
        limit = chunk_limit;
    int64_t per = limit / nthreads;
    if (per < kStreamMin) per = kStreamMin;
    return page_ceil(limit < per ? limit : per, page);
}

// chunk size of a FILE: max_chunk, src/rzip.c:881-888
inline int64_t max_chunk_file(const mrz_control *ctl, int64_t st_size) {
    int64_t max_chunk;
    if (ctl->unlimited)
        max_chunk = st_size;
    else if (ctl->window)
        max_chunk = ctl->window * kChunkUnit;
    else
        max_chunk = ctl->ramsize / 3 * 2;
    return max_chunk < st_size ? page_floor(max_chunk, page_of(ctl)) : max_chunk;
}
// chunk size of STDIN: max_mmap, src/rzip.c:875-894; maxram = ramsize / 3, / 6 to STDOUT (setup_ram, src/util.c:156-164)
inline int64_t max_mmap_stdin(const mrz_control *ctl, int to_stdout) {
    const int64_t max_mmap = page_floor(ctl->ramsize / (to_stdout ? 6 : 3), page_of(ctl));
    const int64_t max_chunk = ctl->window ? ctl->window * kChunkUnit : ctl->ramsize / 3 * 2;
    return max_mmap < max_chunk ? max_mmap : max_chunk;
}

inline int64_t first_chunk_limit(const mrz_control *ctl, int64_t st_size) {
    const int64_t max_chunk = max_chunk_file(ctl, st_size);
    return at_least_page(st_size < max_chunk ? st_size : max_chunk, page_of(ctl));
}
// -n, file -> file: NO_COMPRESS, one thread
inline int64_t bufsize_file(const mrz_control *ctl, int64_t st_size) {
    return stream_bufsize(ctl->ramsize / 3, st_size, first_chunk_limit(ctl, st_size), 1, page_of(ctl));
}
// -l -p<threads>, file -> file: a back-end compresses, so two buffers per thread -- limit = usable_ram / 2 -- over the
// thread count of prepare_streamout_threads (src/stream.c:736: one more than -p when -p > 1)
inline int64_t bufsize_lz4(const mrz_control *ctl, int threads, int64_t st_size) {
    return stream_bufsize(ctl->ramsize / 3 / 2, st_size, first_chunk_limit(ctl, st_size), threads > 1 ? threads + 1 : 1,
                          page_of(ctl));
}
// -n from STDIN: fixed at the first open_stream_out, where control->st_size is what the first chunk read
inline int64_t bufsize_stdin(const mrz_control *ctl, int to_stdout, int64_t first_read) {
    const int64_t page = page_of(ctl);
    return stream_bufsize(ctl->ramsize / (to_stdout ? 6 : 3), first_read, at_least_page(first_read, page), 1, page);
}

inline void fill_magic(uint8_t mg[20], const mrz_control *ctl, int64_t st_size) {  // write_magic, src/mrzip.c:127-188
    memset(mg, 0, 20);
    mg[0] = 'M';
    mg[1] = 'R';
    mg[2] = 'Z';
    mg[3] = 'I';
    mg[4] = 0;  // MRZIP_MAJOR
    mg[5] = 9;  // MRZIP_MINOR
    for (int i = 0; i < 8; i++) mg[6 + i] = (uint8_t)((uint64_t)st_size >> (8 * i));
    mg[14] = 1;  // hash_code: MD5
    mg[18] = (uint8_t)((ctl->rzip_compression_level << 4) + ctl->compression_level);
}

// ---- the stream cutter --------------------------------------------------------------------------------------------
// write_stream / flush_buffer (src/stream.c:1574-1590,1307-1349): two logical streams are cut into blocks whenever a
// stream buffer of `bufsize` bytes fills; close_stream_out (:1623-1648) flushes both, even when empty.  A flush hands
// the buffer to `flush`, which may take the bytes away (swap) or read them.
struct StreamCutter {
    int64_t bufsize = 0;
    std::function<void(int s, std::vector<uint8_t> &block)> flush;
    std::vector<uint8_t> sbuf[2];
    void hand(int s) {
        flush(s, sbuf[s]);
        sbuf[s].clear();
    }
    void write(int s, const uint8_t *p, int64_t n) {
        while (n) {
            const int64_t room = bufsize - (int64_t)sbuf[s].size();
            const int64_t take = room < n ? room : n;
            sbuf[s].insert(sbuf[s].end(), p, p + take);
            p += take;
            n -= take;
            if ((int64_t)sbuf[s].size() == bufsize) hand(s);
        }
    }
    void close() {
        hand(0);
        hand(1);
    }
};

// ---- records onto a cutter ----------------------------------------------------------------------------------------
// Replays a chunk's finished streams so that "buffer full" events of the two streams interleave as in the reference:
// the stream-1 bytes of a literal follow its 3-byte header (put_literal, src/rzip.c:213-227).
inline int replay_records(StreamCutter &w, int cb, const uint8_t *s0, int64_t n0, const uint8_t *s1, int64_t n1) {
    int64_t i = 0, j = 0;
    while (i < n0) {
        if (i + 3 > n0) return MRZ_E_STATE;
        const int head = s0[i];
        const int64_t len = s0[i + 1] | (int64_t)s0[i + 2] << 8;
        if (head == 0) {
            w.write(0, s0 + i, 3);
            i += 3;
            if (len == 0) {
                if (i + 4 != n0) return MRZ_E_STATE;
                w.write(0, s0 + i, 4);
                i += 4;
                break;
            }
            if (j + len > n1) return MRZ_E_STATE;
            w.write(1, s1 + j, len);
            j += len;
        } else {
            if (i + 3 + cb > n0) return MRZ_E_STATE;
            w.write(0, s0 + i, 3 + cb);
            i += 3 + cb;
        }
    }
    return j == n1 ? MRZ_OK : MRZ_E_STATE;
}

// put_literal (src/rzip.c:213-227): per <= 0xFFFF piece a {00, len} header on stream 0, then its bytes on stream 1
inline void put_literal(StreamCutter &w, const uint8_t *buf, int64_t from, int64_t to) {
    do {
        int64_t len = to - from;
        if (len > 0xFFFF) len = 0xFFFF;
        const uint8_t hdr[3] = { 0, (uint8_t)len, (uint8_t)(len >> 8) };
        w.write(0, hdr, 3);
        if (len) w.write(1, buf + from, len);
        from += len;
    } while (to > from);
}

// put_match (src/rzip.c:179-194): {01, len, dist} per <= 0xFFFF piece, dist = p - offset
inline void put_match(StreamCutter &w, int cb, int64_t p, int64_t ofs, int64_t len) {
    const int64_t dist = p - ofs;
    do {
        const int64_t n = len > 0xFFFF ? 0xFFFF : len;
        uint8_t rec[3 + 8] = { 1, (uint8_t)n, (uint8_t)(n >> 8) };
        for (int i = 0; i < cb; i++) rec[3 + i] = (uint8_t)((uint64_t)dist >> (8 * i));
        w.write(0, rec, 3 + cb);
        len -= n;
    } while (len);
}

// hash_search's emit (src/rzip.c:593-595): the literal in front of a match, if there is one, then the match; returns
// where the match ends
inline int64_t put_event(StreamCutter &w, const uint8_t *buf, int cb, int64_t lit_from, const mrz_match &e) {
    if (lit_from < e.p) put_literal(w, buf, lit_from, e.p);
    put_match(w, cb, e.p, e.ofs, e.len);
    return e.p + e.len;
}

// the tail of hash_search (src/rzip.c:619,664-665): trailing literal, terminator, CRC (most significant byte first)
inline void put_tail(StreamCutter &w, const uint8_t *buf, int64_t lit_from, int64_t n, uint32_t crc) {
    if (lit_from < n) put_literal(w, buf, lit_from, n);
    const uint8_t term[7] = { 0, 0, 0, (uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc };
    w.write(0, term, 7);
}

// ---- the chunk writer ---------------------------------------------------------------------------------------------
// Blocks are appended in flush order, each with a {ctype, c_len, u_len, next} header whose `next` field is patched
// when the following block of the same stream lands (compthread, src/stream.c:1199-1293); the first block of a chunk
// brings the chunk header {cb, eof, size_field} and the two empty heads with it.
//
// -l: the chunk's blocks wait as pending and go through the compressor together when the chunk is complete (one wave
// per block on the device: a batch is what keeps it busy); the file keeps flush order all the same.  compthread with
// LZ4_COMPRESS (src/stream.c:1147-1152): every block of at least 64 bytes is framed {CTYPE_LZ4, c_len, u_len, next}
// with what LZ4_compress_default makes of it, also when that is longer than the block (lz4_compress_buf, :278-312,
// compares nothing); its capacity there, round_up_page(n + n/16 + 67), is beyond LZ4_compressBound, so the call cannot
// fail.  Smaller blocks stay CTYPE_NONE.
//
// The compressor: in[i] -> out[i] (which it sizes) for all blocks at once, got[i] the compressed length.
typedef std::function<int(const std::vector<const std::vector<uint8_t> *> &in, std::vector<std::vector<uint8_t>> &out,
                          std::vector<int64_t> &got)>
    BlockCompressor;

struct ChunkWriter {
    std::vector<uint8_t> &out;
    BlockCompressor lz4;  // empty: -n
    int cb = 1, eof = 0, blocks = 0;
    int64_t size_field = 0, initial_pos = 0, cur_pos = 0;
    int64_t last_head[2] = { 0, 0 };
    struct Pending {
        int s;
        std::vector<uint8_t> data;
    };
    std::vector<Pending> pending;

    explicit ChunkWriter(std::vector<uint8_t> &o) : out(o) {}

    void put_val(int64_t v, int width) {
        for (int i = 0; i < width; i++) out.push_back((uint8_t)((uint64_t)v >> (8 * i)));
    }
    void begin(int64_t chunk_size, int chunk_bytes, int is_last, int64_t page) {
        cb = chunk_bytes;
        eof = is_last;
        size_field = at_least_page(chunk_size, page);
        cur_pos = 0;
        blocks = 0;
        pending.clear();
    }
    void put_block(int s, int ctype, const uint8_t *payload, int64_t c_len, int64_t u_len) {
        if (!blocks++) {
            out.push_back((uint8_t)cb);
            out.push_back((uint8_t)eof);
            put_val(size_field, cb);
            initial_pos = (int64_t)out.size();
            for (int j = 0; j < 2; j++) {
                last_head[j] = cur_pos + 1 + 2 * cb;
                out.push_back(MRZ_CTYPE_NONE);
                put_val(0, cb);
                put_val(0, cb);
                put_val(0, cb);
                cur_pos += 1 + 3 * cb;
            }
        }
        for (int i = 0; i < cb; i++)
            out[(size_t)(initial_pos + last_head[s] + i)] = (uint8_t)((uint64_t)cur_pos >> (8 * i));
        last_head[s] = cur_pos + 1 + 2 * cb;
        out.push_back((uint8_t)ctype);
        put_val(c_len, cb);
        put_val(u_len, cb);
        put_val(0, cb);
        cur_pos += 1 + 3 * cb;
        out.insert(out.end(), payload, payload + c_len);
        cur_pos += c_len;
    }
    void add(int s, std::vector<uint8_t> &block) {  // a cutter's flush
        if (lz4) {
            pending.push_back(Pending{ s, std::vector<uint8_t>() });
            pending.back().data.swap(block);
        } else
            put_block(s, MRZ_CTYPE_NONE, block.data(), (int64_t)block.size(), (int64_t)block.size());
    }
    int end() {  // the chunk is complete; the order of the checks is behaviour
        if (!lz4) return MRZ_OK;
        std::vector<const std::vector<uint8_t> *> in;
        for (const Pending &b : pending) {
            if (b.data.size() < 64) continue;
            if ((int64_t)b.data.size() > kLz4MaxInput) return MRZ_E_UNSUPPORTED;  // the reference's call returns 0
            in.push_back(&b.data);
        }
        std::vector<std::vector<uint8_t>> packed(in.size());
        std::vector<int64_t> got(in.size());
        const int rc = lz4(in, packed, got);
        if (rc) return rc;
        size_t k = 0;
        for (const Pending &b : pending) {
            const int64_t len = (int64_t)b.data.size();
            if (len < 64)
                put_block(b.s, MRZ_CTYPE_NONE, b.data.data(), len, len);
            else {
                if (got[k] <= 0) return MRZ_E_STATE;
                put_block(b.s, MRZ_CTYPE_LZ4, packed[k].data(), got[k], len);
                k++;
            }
        }
        pending.clear();
        return MRZ_OK;
    }
};

// ---- where the chunks come from, where the archive goes -----------------------------------------------------------
struct Reader {  // bytes from memory or from a file descriptor
    const uint8_t *mem = nullptr;
    int64_t mem_n = 0, mem_at = 0;
    int fd = -1;
    std::vector<uint8_t> buf;  // what a file descriptor delivered
    Reader(const void *in, int64_t n) : mem((const uint8_t *)in), mem_n(n) {}
    explicit Reader(int fd_) : fd(fd_) {}
    // up to `want` bytes at *p -- fewer only if the input ends first, *hit_end if a read returned 0; < 0 on error.
    // Memory is handed out where it lies.
    int64_t take(int64_t want, const uint8_t **p, bool *hit_end) {
        if (fd < 0) {
            const int64_t k = mem_n - mem_at < want ? mem_n - mem_at : want;
            *p = mem + mem_at;
            mem_at += k;
            *hit_end = k < want;
            return k;
        }
        buf.resize((size_t)want);
        *p = buf.data();
        *hit_end = false;
        int64_t got = 0;
        while (got < want) {
            const int64_t left = want - got;
            const ssize_t r = read(fd, buf.data() + got, (size_t)(left > (1ll << 30) ? (1ll << 30) : left));
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) return -1;
            if (r == 0) {
                *hit_end = true;
                break;
            }
            got += r;
        }
        return got;
    }
};

// The chunk loop of rzip_fd (src/rzip.c:915-1061) in its two forms: a FILE, whose size is known -- chunks of
// max_chunk bytes, the last one carries the eof flag (:1049) -- and STDIN (mmap_stdin :700-732) -- chunks of
// max_mmap bytes until read() returns 0; the chunk in which that happens is shrunk and carries the eof flag,
// which is one more, empty chunk when the input length is a multiple of the chunk size.
struct Source {
    Reader rd;
    explicit Source(const Reader &r) : rd(r) {}
    virtual ~Source() {}
    // the next chunk; *eof: the reference's control->eof for this chunk; returns an MRZ_ code
    virtual int next(const uint8_t **p, int64_t *n, int *eof) = 0;
    virtual bool more() const = 0;  // while (!pass || len > 0 || (STDIN && !stdin_eof))
};

struct FileSource : Source {  // size known up front
    int64_t left, max_chunk;
    int pass = 0;
    FileSource(const Reader &r, int64_t n, int64_t mc) : Source(r), left(n), max_chunk(mc) {}
    bool more() const override { return !pass || left > 0; }
    int next(const uint8_t **p, int64_t *n, int *eof) override {
        const int64_t csz = max_chunk < left ? max_chunk : left;
        bool hit;
        if (rd.take(csz, p, &hit) != csz) return MRZ_E_ARG;  // the file shrank under us
        *n = csz;
        *eof = csz == left;
        left -= csz;
        pass++;
        return MRZ_OK;
    }
};

struct StdinSource : Source {  // size unknown: mmap_stdin
    int64_t max_mmap;
    bool seen_eof = false;
    StdinSource(const Reader &r, int64_t mm) : Source(r), max_mmap(mm) {}
    bool more() const override { return !seen_eof; }
    int next(const uint8_t **p, int64_t *n, int *eof) override {
        *n = rd.take(max_mmap, p, &seen_eof);  // fewer than max_mmap: "Shrinking chunk"
        if (*n < 0) return MRZ_E_ARG;
        *eof = seen_eof ? 1 : 0;
        return MRZ_OK;
    }
};

struct Out {  // the archive: memory, or a file descriptor written chunk by chunk
    std::vector<uint8_t> *vec = nullptr;
    int fd = -1;
    int put(const uint8_t *p, size_t n, bool at0 = false) {  // at0: fdout_seekto(0) + put_fdout, src/mrzip.c:176-178
        if (vec) {
            if (at0)
                memcpy(vec->data(), p, n);
            else
                vec->insert(vec->end(), p, p + n);
            return MRZ_OK;
        }
        size_t off = 0;
        while (off < n) {
            const ssize_t w = at0 ? pwrite(fd, p + off, n - off, (off_t)off) : write(fd, p + off, n - off);
            if (w < 0) {
                if (errno == EINTR) continue;
                return MRZ_E_ARG;
            }
            off += (size_t)w;
        }
        return MRZ_OK;
    }
};

// ---- the archive --------------------------------------------------------------------------------------------------
// compress_file (src/mrzip.c:1053-1163) around the chunks: begin(), then per chunk start_chunk() before and
// end_chunk() after its streams exist, then finish().
struct ArchiveSink {
    enum { FILE_FORM = 0, STDIN_TO_FILE = 1, STDIN_TO_STDOUT = 2 };
    const mrz_control *ctl;
    int mode;
    int64_t st_size_known;  // FILE_FORM
    int lz4_threads;        // 0 = the -n sink; > 0 = the -l back-end with -p<lz4_threads> (FILE_FORM only)
    Out &out;
    std::vector<uint8_t> piece;
    ChunkWriter writer;
    StreamCutter cutter;
    int64_t st_size = 0;
    int nch = 0;

    ArchiveSink(const mrz_control *c, int mode_, int64_t st_size_known_, int lz4_threads_, Out &o, BlockCompressor lz4)
        : ctl(c), mode(mode_), st_size_known(st_size_known_), lz4_threads(lz4_threads_), out(o), writer(piece) {
        writer.lz4 = lz4;
        cutter.flush = [this](int s, std::vector<uint8_t> &block) { writer.add(s, block); };
    }
    int begin() {  // header placeholder (compress_file, src/mrzip.c:1126)
        const uint8_t mg[20] = { 0 };
        return mode == STDIN_TO_STDOUT ? (int)MRZ_OK : out.put(mg, 20);
    }
    int start_chunk(int64_t csz, int cb, int eof) {
        st_size += csz;
        writer.begin(csz, cb, eof, page_of(ctl));
        if (nch++) return MRZ_OK;
        // the block size is fixed at the first open_stream_out
        if (mode != FILE_FORM)
            cutter.bufsize = bufsize_stdin(ctl, mode == STDIN_TO_STDOUT, csz);
        else if (lz4_threads)
            cutter.bufsize = bufsize_lz4(ctl, lz4_threads, st_size_known);
        else
            cutter.bufsize = bufsize_file(ctl, st_size_known);
        if (mode != STDIN_TO_STDOUT) return MRZ_OK;
        // STDOUT: the first block writes the magic header (src/stream.c:1202-1205); the size is only in it if the
        // input has already ended (write_magic, src/mrzip.c:137-140)
        uint8_t mg[20];
        fill_magic(mg, ctl, eof ? st_size : 0);
        return out.put(mg, 20);
    }
    int end_chunk(const uint8_t *s0, int64_t n0, const uint8_t *s1, int64_t n1) {
        piece.clear();
        int rc = replay_records(cutter, writer.cb, s0, n0, s1, n1);
        if (rc) return rc;
        cutter.close();
        rc = writer.end();
        return rc ? rc : out.put(piece.data(), piece.size());
    }
    int finish(const uint8_t md5[16]) {  // the whole-input hash; compress_file writes the header last (src/mrzip.c:1132)
        const int rc = out.put(md5, 16);
        if (rc || mode == STDIN_TO_STDOUT) return rc;
        uint8_t mg[20];
        fill_magic(mg, ctl, st_size);
        return out.put(mg, 20, true);
    }
};

}  // namespace mrz_framing
