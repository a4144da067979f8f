// mrz_host.hip -- host driver (include/mrzgpu_host.h): the `mrzip -n` / `-l` file path around the GPU rzip stage.
// Host code only, and thin: one chunk loop under the six compress-side entry points, the contexts and the device
// calls of a chunk, the whole-file MD5 on a helper thread (the reference also keeps the checksums off the matcher's
// thread, src/rzip.c:488-505; MD5 is a strictly serial hash, it overlaps the GPU work) and the threads of the
// back-end hand-off.  Every byte written and every size decided is mrz_framing.h's.
// The decompress side (`mrzip -d`) is mrz_unarchive.hip over mrz_archive.h.
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mrzgpu_host.h"
#include "mrz_ctx.h"
#include "mrz_framing.h"
#include "mrz_md5.h"

using namespace mrz_framing;

namespace {

// joins a thread when the scope is left, whichever way (an allocation that throws between the thread's start and its
// join would otherwise destroy a joinable std::thread: std::terminate instead of MRZ_E_NOMEM at the C ABI)
struct mrz_join_guard {
    std::thread &t;
    explicit mrz_join_guard(std::thread &th) : t(th) {}
    ~mrz_join_guard() {
        if (t.joinable()) t.join();
    }
};

template <class F>
int no_bad_alloc(F &&call) {
    try {
        return call();
    } catch (const std::bad_alloc &) {
        return MRZ_E_NOMEM;
    }
}

struct Totals {  // what a run owes its caller beside the bytes
    mrz_stats stats;
    uint8_t md5[16];
    void deliver(mrz_stats *stats_out, uint8_t *md5_out) const {
        if (stats_out) *stats_out = stats;
        if (md5_out) memcpy(md5_out, md5, 16);
    }
};

void add_stats(mrz_stats &t, const mrz_stats &s) {
    t.inserts += s.inserts;
    t.literals += s.literals;
    t.literal_bytes += s.literal_bytes;
    t.matches += s.matches;
    t.match_bytes += s.match_bytes;
    t.tag_hits += s.tag_hits;
    t.tag_misses += s.tag_misses;
}

struct ChunkIn {
    const uint8_t *p;
    int64_t n;
    int index, eof, cb;
};

// The chunk loop of rzip_fd (src/rzip.c:915-1061).  body(chunk, &victim_round, result): the device work of one chunk
// and what becomes of its streams.  The whole-input hash (:1069-1090) is fed chunk by chunk beside it.
template <class Body>
int chunk_loop(Source &src, Totals &t, Body &&body) {
    memset(&t.stats, 0, sizeof(t.stats));
    Md5 md5h;
    int64_t victim_round = 0;  // first rzip_fd call of the process
    for (int index = 0; src.more(); index++) {
        ChunkIn c;
        int rc = src.next(&c.p, &c.n, &c.eof);
        if (rc) return rc;
        c.index = index;
        c.cb = mrz_chunk_bytes(c.n);
        std::thread hasher([&]() { md5h.update(c.p, (size_t)c.n); });
        mrz_join_guard hasher_guard(hasher);
        mrz_chunk_result res;
        rc = body(c, &victim_round, res);
        if (rc) return rc;
        add_stats(t.stats, res.stats);
    }
    md5h.finish(t.md5);
    return MRZ_OK;
}

// an archive: the streams of every chunk come back from the device and go through the sink
int run_archive(const mrz_control *ctl, Source &src, int mode, int64_t st_size_known, int64_t open_chunk, Out &out,
                mrz_stats *stats, uint8_t *md5_out, int lz4_threads) {
    CtxGuard g;
    int rc = mrz_open(&g.ctx, ctl->device, ctl->rzip_compression_level, open_chunk);
    if (rc) return rc;
    BlockCompressor lz4;
    if (lz4_threads)
        lz4 = [&g](const std::vector<const std::vector<uint8_t> *> &in, std::vector<std::vector<uint8_t>> &packed,
                   std::vector<int64_t> &got) {
            std::vector<const void *> src;
            std::vector<void *> dst;
            std::vector<int64_t> lens, caps;
            for (size_t i = 0; i < in.size(); i++) {
                packed[i].resize((size_t)mrz_lz4_bound((int64_t)in[i]->size()));
                src.push_back(in[i]->data());
                dst.push_back(packed[i].data());
                lens.push_back((int64_t)in[i]->size());
                caps.push_back((int64_t)packed[i].size());
            }
            return mrz_lz4_compress_batch(g.ctx, src.data(), lens.data(), (int)src.size(), MRZ_MEM_HOST, dst.data(),
                                          caps.data(), MRZ_MEM_HOST, got.data());
        };
    ArchiveSink sink(ctl, mode, st_size_known, lz4_threads, out, lz4);
    Totals t;
    std::vector<uint8_t> s0, s1;
    rc = sink.begin();
    if (!rc)
        rc = chunk_loop(src, t, [&](const ChunkIn &c, int64_t *victim_round, mrz_chunk_result &res) {
            int r = sink.start_chunk(c.n, c.cb, c.eof);
            if (!r) r = mrz_rzip_chunk(g.ctx, c.p, c.n, MRZ_MEM_HOST, c.cb, victim_round, &res);
            if (r) return r;
            s0.resize((size_t)res.s0_len);
            s1.resize((size_t)res.s1_len);
            r = mrz_fetch_streams(g.ctx, s0.data(), s1.data());
            return r ? r : sink.end_chunk(s0.data(), res.s0_len, s1.data(), res.s1_len);
        });
    if (!rc) rc = sink.finish(t.md5);
    if (!rc) t.deliver(stats, md5_out);
    return rc;
}

int check_control(const mrz_control *ctl) {
    if (!ctl || ctl->rzip_compression_level < 1 || ctl->rzip_compression_level > 9) return MRZ_E_ARG;
    if (ctl->hash_code != 1 && ctl->hash_code != 0) return MRZ_E_ARG;  // MD5 only (reference default)
    return MRZ_OK;
}

int run_file(const mrz_control *ctl, const Reader &rd, int64_t n, Out &out, mrz_stats *stats, uint8_t *md5_out,
             int lz4_threads = 0) {
    if (check_control(ctl) || n < 0) return MRZ_E_ARG;
    const int64_t max_chunk = max_chunk_file(ctl, n);
    FileSource src(rd, n, max_chunk);
    return run_archive(ctl, src, ArchiveSink::FILE_FORM, n, max_chunk < n ? max_chunk : n, out, stats, md5_out,
                       lz4_threads);
}

int run_stdin(const mrz_control *ctl, const Reader &rd, int to_stdout, Out &out, mrz_stats *stats, uint8_t *md5_out) {
    const int rc = check_control(ctl);
    if (rc) return rc;
    if (ctl->unlimited) return MRZ_E_ARG;  // -U takes the window from the file size, which STDIN does not have
    const int64_t mm = max_mmap_stdin(ctl, to_stdout);
    if (mm <= 0) return MRZ_E_ARG;
    StdinSource src(rd, mm);
    return run_archive(ctl, src, to_stdout ? ArchiveSink::STDIN_TO_STDOUT : ArchiveSink::STDIN_TO_FILE, 0, mm, out, stats,
                       md5_out, 0);
}

// run(Out &) into a vector, then into memory the caller releases with mrz_free
template <class Run>
int to_malloc(void **out, int64_t *out_len, Run &&run) {
    return no_bad_alloc([&] {
        std::vector<uint8_t> buf;
        Out o;
        o.vec = &buf;
        const int rc = run(o);
        if (rc) return rc;
        void *p = malloc(buf.size() ? buf.size() : 1);
        if (!p) return (int)MRZ_E_NOMEM;
        memcpy(p, buf.data(), buf.size());
        *out = p;
        *out_len = (int64_t)buf.size();
        return (int)MRZ_OK;
    });
}

}  // namespace

extern "C" int64_t mrz_plan(const mrz_control *ctl, int64_t st_size, int64_t *stream_bufsize) {
    if (stream_bufsize) *stream_bufsize = bufsize_file(ctl, st_size);
    return max_chunk_file(ctl, st_size);
}

extern "C" void mrz_free(void *p) { free(p); }

extern "C" int mrz_rzip_buffer(const mrz_control *ctl, const void *in, int64_t n, void **out, int64_t *out_len,
                               mrz_stats *stats, uint8_t *md5_out) {
    if (!out || !out_len || (n > 0 && !in)) return MRZ_E_ARG;
    return to_malloc(out, out_len, [&](Out &o) { return run_file(ctl, Reader(in, n), n, o, stats, md5_out); });
}

extern "C" int mrz_rzip_buffer_lz4(const mrz_control *ctl, int threads, const void *in, int64_t n, void **out,
                                   int64_t *out_len, mrz_stats *stats, uint8_t *md5_out) {
    if (!out || !out_len || (n > 0 && !in) || threads < 1) return MRZ_E_ARG;
    if (check_control(ctl)) return MRZ_E_ARG;
    if (ctl->compression_level < 1) return MRZ_E_ARG;
    if (ctl->compression_level > 2) return MRZ_E_UNSUPPORTED;  // LZ4_compress_HC, src/stream.c:297-305
    return to_malloc(out, out_len,
                     [&](Out &o) { return run_file(ctl, Reader(in, n), n, o, stats, md5_out, threads); });
}

extern "C" int mrz_rzip_stream_buffer(const mrz_control *ctl, const void *in, int64_t n, int to_stdout, void **out,
                                      int64_t *out_len, mrz_stats *stats, uint8_t *md5_out) {
    if (!out || !out_len || (n > 0 && !in)) return MRZ_E_ARG;
    return to_malloc(out, out_len,
                     [&](Out &o) { return run_stdin(ctl, Reader(in, n), to_stdout, o, stats, md5_out); });
}

extern "C" int mrz_rzip_stream(const mrz_control *ctl, int fd_in, int fd_out, int to_stdout, mrz_stats *stats) {
    return no_bad_alloc([&] {
        Out o;
        o.fd = fd_out;
        return run_stdin(ctl, Reader(fd_in), to_stdout, o, stats, nullptr);
    });
}

extern "C" int mrz_rzip_fd(const mrz_control *ctl, int fd_in, int fd_out, mrz_stats *stats) {
    // a regular file is compressed as a FILE (size from fstat, src/rzip.c:864-866), anything else -- a pipe, a
    // terminal -- the way the reference compresses STDIN; the output counts as STDOUT when it cannot seek
    struct stat sb;
    if (fstat(fd_in, &sb)) return MRZ_E_ARG;
    const bool out_seeks = lseek(fd_out, 0, SEEK_CUR) != (off_t)-1;
    if (!S_ISREG(sb.st_mode)) return mrz_rzip_stream(ctl, fd_in, fd_out, out_seeks ? 0 : 1, stats);
    if (!out_seeks) return MRZ_E_ARG;  // file -> STDOUT keeps the output in a temporary buffer upstream: not mirrored
    return no_bad_alloc([&] {
        const off_t at = lseek(fd_in, 0, SEEK_CUR);
        const int64_t n = (int64_t)sb.st_size - (at > 0 ? (int64_t)at : 0);
        Out o;
        o.fd = fd_out;
        return run_file(ctl, Reader(fd_in), n < 0 ? 0 : n, o, stats, nullptr);
    });
}

// ---- back-end hand-off pipeline -------------------------------------------------
// The reference hands every full stream buffer to a compthread and keeps the output in flush order
// (flush_buffer src/stream.c:1307-1349, compthread :1115-1305, the output_thread ticket :1199-1201).  Here the
// GPU thread produces the two streams of chunk k+1 while a consumer thread takes the blocks the cutter made of
// chunk k and hands them, in exactly that flush order, to the caller's function -- the place where a back-end
// codec would compress the block.
namespace {

struct Block {
    mrz_block_info info;
    std::vector<uint8_t> payload;
};

struct BlockQueue {  // producer -> consumer
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Block> blocks;
    bool done = false;               // nothing more is coming
    std::atomic<int> abort_rc{ 0 };  // what the consumer's side returned when it failed
    void push(Block &&b) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return blocks.size() < 4 || abort_rc; });  // back-pressure: a few blocks in flight
            blocks.push_back(std::move(b));
        }
        cv.notify_all();
    }
    bool pop(Block &b) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !blocks.empty() || done; });
            if (blocks.empty()) return false;
            b = std::move(blocks.front());
            blocks.pop_front();
        }
        cv.notify_all();
        return true;
    }
    template <class F>
    void tell(F &&change) {  // wakes whoever waits: the consumer for blocks, the producer's back-pressure wait
        {
            std::lock_guard<std::mutex> lk(mu);
            change();
        }
        cv.notify_all();
    }
};

// ends the consumer when the scope is left: it first has to be told that nothing more is coming
struct consumer_guard {
    BlockQueue &q;
    std::thread &t;
    ~consumer_guard() {
        q.tell([&] { q.done = true; });
        if (t.joinable()) t.join();
    }
};

// state of the chunk in flight, driven by mrz_rzip_chunk's progress calls
struct ChunkFeed {
    mrz_ctx *ctx;
    const uint8_t *buf;
    int cb;
    StreamCutter *cut;
    mrz_block_info *info;
    const std::atomic<int> *abort_rc;
    int64_t ev_done, lit_from;  // matches encoded so far; end of the last encoded match
    std::vector<mrz_match> ev;
};

int chunk_progress(void *user, int64_t n_events, int64_t last_match, int) {
    ChunkFeed *f = (ChunkFeed *)user;
    if (*f->abort_rc) return 1;
    if (n_events <= f->ev_done) return 0;
    return no_bad_alloc([&] {
        const int64_t cnt = n_events - f->ev_done;
        f->ev.resize((size_t)cnt);
        if (mrz_fetch_events(f->ctx, f->ev_done, cnt, f->ev.data())) return 1;
        f->info->input_final = last_match;
        for (const mrz_match &e : f->ev) f->lit_from = put_event(*f->cut, f->buf, f->cb, f->lit_from, e);
        f->ev_done = n_events;
        return 0;
    });
}

int rzip_pipeline_impl(const mrz_control *ctl, const uint8_t *in, int64_t n, mrz_block_fn fn, void *user,
                       mrz_stats *stats, uint8_t *md5_out) {
    const int64_t max_chunk = max_chunk_file(ctl, n);
    // the LZ4 gate works on a ctx / stream of its own, opened before the consumer starts
    CtxGuard gate;
    int rc = ctl->lz4_test ? mrz_open(&gate.ctx, ctl->device, ctl->rzip_compression_level, 0) : (int)MRZ_OK;
    if (rc) return rc;
    BlockQueue q;
    Totals t;
    rc = no_bad_alloc([&] {
        // consumer: the gate and the caller's function, block by block, in flush order; after a failure it only drains
        std::thread consumer([&]() {
            for (Block b; q.pop(b);) {
                if (q.abort_rc) continue;
                b.info.lz4_verdict = -1;
                int r = 0;
                if (gate.ctx && (int64_t)b.payload.size() >= 64) {  // compthread: `c_len >= 64`, src/stream.c:1147
                    int verdict = 0;
                    r = mrz_lz4_compresses(gate.ctx, b.payload.data(), (int64_t)b.payload.size(), MRZ_MEM_HOST,
                                           ctl->threshold > 0 ? ctl->threshold : 100, &verdict);
                    b.info.lz4_verdict = verdict;
                }
                if (!r) r = fn(user, &b.info, b.payload.data(), (int64_t)b.payload.size());
                if (r) q.tell([&] { q.abort_rc = r; });
            }
        });
        consumer_guard cg{ q, consumer };
        CtxGuard g;
        int r = mrz_open(&g.ctx, ctl->device, ctl->rzip_compression_level, max_chunk < n ? max_chunk : n);
        if (r) return r;
        // write_stream / flush_buffer without the file: every full stream buffer becomes one Block for the consumer
        mrz_block_info info;
        StreamCutter cut;
        cut.bufsize = bufsize_file(ctl, n);
        cut.flush = [&](int s, std::vector<uint8_t> &bytes) {
            Block b;
            b.info = info;
            b.info.stream = s;
            b.payload.swap(bytes);
            info.first_of_chunk = 0;
            q.push(std::move(b));
        };
        FileSource src(Reader(in, n), n, max_chunk);
        return chunk_loop(src, t, [&](const ChunkIn &c, int64_t *victim_round, mrz_chunk_result &res) {
            memset(&info, 0, sizeof(info));
            info.chunk_index = c.index;
            info.chunk_bytes = c.cb;
            info.eof = c.eof;
            info.chunk_size = c.n;
            info.first_of_chunk = 1;
            info.lz4_verdict = -1;
            ChunkFeed feed{ g.ctx, c.p, c.cb, &cut, &info, &q.abort_rc, 0, 0, {} };
            mrz_set_progress(g.ctx, chunk_progress, &feed);
            const int r2 = mrz_rzip_chunk(g.ctx, c.p, c.n, MRZ_MEM_HOST, c.cb, victim_round, &res);
            mrz_set_progress(g.ctx, nullptr, nullptr);
            if (r2) return r2;
            info.input_final = c.n;
            put_tail(cut, c.p, feed.lit_from, c.n, res.crc32);
            cut.close();  // close_stream_out flushes both streams, even when empty (src/stream.c:1623-1648)
            return (int)MRZ_OK;
        });
    });
    if (q.abort_rc) rc = q.abort_rc;
    if (!rc) t.deliver(stats, md5_out);
    return rc;
}

}  // namespace

extern "C" int mrz_rzip_pipeline(const mrz_control *ctl, const void *in_v, int64_t n, mrz_block_fn fn, void *user,
                                 mrz_stats *stats, uint8_t *md5_out) {
    if (!ctl || !fn || n < 0 || (n > 0 && !in_v)) return MRZ_E_ARG;
    if (ctl->rzip_compression_level < 1 || ctl->rzip_compression_level > 9) return MRZ_E_ARG;
    return no_bad_alloc([&] { return rzip_pipeline_impl(ctl, (const uint8_t *)in_v, n, fn, user, stats, md5_out); });
}
