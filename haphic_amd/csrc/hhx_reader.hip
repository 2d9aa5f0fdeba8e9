// A text file as chunks of whole lines in PINNED host memory (the front of a1: pairs_generator* :1539-1583 read the .pairs file line by line).
// The file is read with pread() by a few threads into one of two pinned buffers while the caller tokenises the other (hhx_pairs_parse copies a
// pinned chunk to the device at PCIe rate; from a memory map of the file the same copy ran at 14 GB/s and unmapping 50 GB cost another second).
// A chunk ends after its last line break; the cut-off tail is carried to the front of the next chunk.  Universal newlines as in hhx_text.hip:
// a chunk may end on '\n' or on a '\r' — a "\r\n" pair split across two chunks would count an empty line more, which the tokeniser skips (:1552).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <condition_variable>
#include <thread>

#include "hhx_bgzf.h"

using namespace hhx;

struct hhx_text_reader {
    int fd = -1;
    i64 size = 0, at = 0;                 // file size, next byte to read
    size_t chunk = 0, cap = 0;
    int n_threads = 4;
    unsigned char *buf[2] = {nullptr, nullptr};
    i64 len[2] = {0, 0};                  // bytes of whole lines ready in buf[k]
    int state[2] = {0, 0};                // 0 free for the reader, 1 filled, 2 held by the caller
    std::vector<unsigned char> tail;      // the bytes after the last line break of the chunk read last: the front of the next chunk
    bool raw = false;                     // hhx_text_reader_open_raw: fixed-size chunks cut anywhere, nothing carried (a consumer that keeps its own state across cuts)
    bool bgzf = false;                    // the file is BGZF: `at` / `size` count COMPRESSED bytes, the buffers hold inflated text
    i64 skip = 0;                         // BGZF range: inflated bytes to drop in front of the first line (the range starts inside a block)
    i64 limit = -1;                       // BGZF range: inflated bytes to hand out in all (-1: to the end of the file)
    std::vector<unsigned char> comp;      // compressed bytes read and not yet inflated (whole blocks + a partial tail)
    std::string emsg;                     // set with err == EBADMSG
    int fill = 0, take = 0;               // next buffer to fill / to hand out
    bool eof = false, stop = false;
    int err = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::thread th;

    void read_range(unsigned char *dst, i64 off, size_t n) {
        const int T = n < ((size_t)8 << 20) ? 1 : n_threads;
        std::vector<std::thread> pool;
        const size_t span = ((n + T - 1) / T + 4095) & ~(size_t)4095;
        auto work = [&](size_t lo, size_t hi) {
            while (lo < hi) {
                const ssize_t k = ::pread(fd, dst + lo, hi - lo, (off_t)(off + (i64)lo));
                if (k <= 0) { std::lock_guard<std::mutex> lk(mu); err = k < 0 ? errno : EIO; return; }
                lo += (size_t)k;
            }
        };
        for (int t = 1; t < T; ++t) { const size_t lo = std::min(n, span * t), hi = std::min(n, span * (t + 1)); if (lo < hi) pool.emplace_back(work, lo, hi); }
        work(0, std::min(n, span));
        for (auto &p : pool) p.join();
    }
    void loop() {
        for (;;) {
            int b;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [this] { return stop || state[fill] == 0; });
                if (stop) return;
                b = fill;
            }
            size_t have = tail.size();
            if (have) memcpy(buf[b], tail.data(), have);             // buf[b] is free: the caller has let go of it
            tail.clear();
            size_t cut = 0;
            bool last = false;
            for (;;) {
                if (bgzf) {
                    // compressed bytes for about a chunk of text (BGZF of text: 3-5 x), whole blocks inflated in place behind what the buffer holds
                    const size_t want_c = (size_t)std::min<i64>((i64)std::max<size_t>(chunk / 3, (size_t)1 << 20), size - at);
                    if (want_c) {
                        const size_t old = comp.size();
                        comp.resize(old + want_c);
                        read_range(comp.data() + old, at, want_c);
                        at += (i64)want_c;
                    }
                    std::vector<Block> blocks;
                    size_t used = 0, inflated = 0;
                    const size_t room = cap - have;
                    if (scan_blocks(comp, room, blocks, used, inflated)) { std::lock_guard<std::mutex> lk(mu); err = EBADMSG; emsg = g_err; eof = true; cv.notify_all(); return; }
                    if (!blocks.empty() && inflated > room) { std::lock_guard<std::mutex> lk(mu); err = EOVERFLOW; eof = true; cv.notify_all(); return; }
                    if (blocks.empty() && at >= size && !comp.empty()) { std::lock_guard<std::mutex> lk(mu); err = EBADMSG; emsg = "truncated BGZF block at the end of the file"; eof = true; cv.notify_all(); return; }
                    if (!blocks.empty()) {
                        if (inflate_blocks(comp.data(), blocks, buf[b] + have, n_threads)) { std::lock_guard<std::mutex> lk(mu); err = EBADMSG; emsg = g_err; eof = true; cv.notify_all(); return; }
                        comp.erase(comp.begin(), comp.begin() + (long)used);
                        if (skip) {                                  // a range: the text in front of its first line belongs to the rank before
                            const size_t d = (size_t)std::min<i64>(skip, (i64)inflated);
                            memmove(buf[b] + have, buf[b] + have + d, inflated - d);
                            inflated -= d;
                            skip -= (i64)d;
                        }
                        if (limit >= 0) {                            // ... and the text behind its last line to the rank after
                            if ((i64)inflated >= limit) { inflated = (size_t)limit; at = size; comp.clear(); }
                            limit -= (i64)inflated;
                        }
                        have += inflated;
                    }
                    last = at >= size && comp.empty();
                    cut = have;
                    if (last) break;
                    if (have < chunk && have + ((size_t)64 << 10) <= cap) continue;      // less than a chunk of text so far
                } else {
                    const size_t want = (size_t)std::min<i64>((i64)chunk, size - at);
                    if (have + want > cap) { std::lock_guard<std::mutex> lk(mu); err = EOVERFLOW; eof = true; cv.notify_all(); return; }      // a line longer than a chunk
                    if (want) read_range(buf[b] + have, at, want);
                    at += (i64)want;
                    have += want;
                    last = at >= size;
                    cut = have;
                    if (last || raw) break;
                }
                while (cut > 0 && buf[b][cut - 1] != '\n' && buf[b][cut - 1] != '\r') --cut;
                if (cut > 0) break;                                  // else: no line break in the whole chunk, keep reading into the same buffer
                if (bgzf && have + ((size_t)64 << 10) > cap) { std::lock_guard<std::mutex> lk(mu); err = EOVERFLOW; eof = true; cv.notify_all(); return; }
            }
            if (!last) tail.assign(buf[b] + cut, buf[b] + have);
            {
                std::lock_guard<std::mutex> lk(mu);
                len[b] = (i64)cut;
                state[b] = 1;
                fill = b ^ 1;
                if (last) eof = true;
            }
            cv.notify_all();
            if (last) return;
        }
    }
};

// The byte-range rule of a rank's share of a file (haphic_amd/ranks.py owned_range): a range [begin, end) owns the lines whose first byte lies in it.
// A line starts at 0 and after every '\n'; a boundary x inside a line moves forward to the start of the next line (or the end of the text), so
// the ranges of consecutive boundaries cover every line exactly once, in order.  Lines are cut on '\n' only: a "\r\n" stays whole.
namespace {

struct BgzfIndex {                        // every BGZF block of the file: compressed offset, compressed size, inflated size (its ISIZE trailer)
    std::vector<i64> off, bsize, isize, text;                // text[k] = inflated bytes in front of block k (text.size() == n + 1)
};

int bgzf_index(int fd, i64 size, BgzfIndex &ix) {
    ix = BgzfIndex();
    ix.text.push_back(0);
    unsigned char h[12 + 256], t[4];
    for (i64 at = 0; at < size;) {
        // the block header: gzip magic, FEXTRA, then the BC subfield (BSIZE) wherever it stands among the extra subfields (as scan_blocks reads it)
        const ssize_t k = ::pread(fd, h, sizeof h, at);
        if (k < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return fail("not a BGZF block at compressed offset %lld", (long long)at);
        const i64 xlen = (i64)(h[10] | (h[11] << 8));
        i64 bs = 0;
        for (i64 x = 0; x + 4 <= xlen && 12 + x + 6 <= (i64)k;) {
            const unsigned char *f = h + 12 + x;
            const i64 slen = (i64)(f[2] | (f[3] << 8));
            if (f[0] == 'B' && f[1] == 'C' && slen == 2) { bs = (i64)(f[4] | (f[5] << 8)) + 1; break; }
            x += 4 + slen;
        }
        if (!bs) return fail("not a BGZF block at compressed offset %lld: no BC subfield", (long long)at);
        if (bs < 12 + xlen + 8 || at + bs > size || ::pread(fd, t, 4, at + bs - 4) != 4) return fail("truncated BGZF block at compressed offset %lld", (long long)at);
        ix.off.push_back(at); ix.bsize.push_back(bs); ix.isize.push_back((i64)bgzf_rd32(t));
        ix.text.push_back(ix.text.back() + ix.isize.back());
        at += bs;
    }
    return 0;
}

int bgzf_inflate_block(int fd, const BgzfIndex &ix, size_t k, std::vector<unsigned char> &out) {
    std::vector<unsigned char> comp((size_t)ix.bsize[k]);
    if (::pread(fd, comp.data(), comp.size(), ix.off[k]) != (ssize_t)comp.size()) return fail("cannot read a BGZF block: %s", strerror(errno));
    std::vector<Block> blocks;
    size_t used = 0, inflated = 0;
    if (scan_blocks(comp, (size_t)1 << 20, blocks, used, inflated) || blocks.size() != 1) return fail("not a BGZF block at compressed offset %lld", (long long)ix.off[k]);
    out.assign(inflated, 0);
    return inflated ? inflate_blocks(comp.data(), blocks, out.data(), 1) : 0;
}

// the text offset of the first line start at or after text offset x (x itself when a line starts there)
int bgzf_line_start(int fd, const BgzfIndex &ix, i64 x, i64 &start) {
    const i64 total = ix.text.back();
    start = x;
    if (x <= 0 || x >= total) return 0;
    size_t k = (size_t)(std::upper_bound(ix.text.begin(), ix.text.end(), x - 1) - ix.text.begin()) - 1;     // the block holding byte x - 1
    std::vector<unsigned char> t;
    for (i64 from = x - 1; k < ix.off.size(); ++k) {
        if (!ix.isize[k]) continue;
        if (bgzf_inflate_block(fd, ix, k, t)) return -1;
        for (i64 i = std::max<i64>(from, ix.text[k]) - ix.text[k]; i < (i64)t.size(); ++i)
            if (t[(size_t)i] == '\n') { start = ix.text[k] + i + 1; return 0; }
        from = ix.text[k + 1];
    }
    start = total;
    return 0;
}

int plain_line_start(int fd, i64 size, i64 x, i64 &start) {
    start = x;
    if (x <= 0 || x >= size) return 0;
    unsigned char b[1 << 16];
    for (i64 at = x - 1; at < size;) {
        const ssize_t k = ::pread(fd, b, (size_t)std::min<i64>((i64)sizeof b, size - at), at);
        if (k <= 0) return fail("cannot read: %s", strerror(k < 0 ? errno : EIO));
        const void *nl = memchr(b, '\n', (size_t)k);
        if (nl) { start = at + ((const unsigned char *)nl - b) + 1; return 0; }
        at += k;
    }
    start = size;
    return 0;
}

}  // namespace

static int text_reader_open(const char *path, int64_t chunk_bytes, int n_threads, bool bgzf, int64_t begin, int64_t end, hhx_text_reader **out, bool raw = false);
extern "C" int hhx_text_reader_open(const char *path, int64_t chunk_bytes, int n_threads, hhx_text_reader **out) {
    return text_reader_open(path, chunk_bytes, n_threads, false, -1, -1, out);
}
// the same over a BGZF file (bgzip): the chunks are inflated text.  Fails with "not a BGZF file" on anything else (plain gzip included)
extern "C" int hhx_text_reader_open_bgzf(const char *path, int64_t chunk_bytes, int n_threads, hhx_text_reader **out) {
    return text_reader_open(path, chunk_bytes, n_threads, true, -1, -1, out);
}
// one rank's share of the file: the lines whose first byte lies in [begin, end) (BGZF: the blocks that start in [begin, end) of the COMPRESSED file,
// the same line rule on their inflated text)
extern "C" int hhx_text_reader_open_range(const char *path, int64_t begin, int64_t end, int64_t chunk_bytes, int n_threads, int bgzf, hhx_text_reader **out) {
    if (begin < 0 || end < begin) return fail("hhx_text_reader_open_range: bad range [%lld, %lld)", (long long)begin, (long long)end);
    return text_reader_open(path, chunk_bytes, n_threads, bgzf != 0, begin, end, out);
}
// the bytes of the file as they are, chunk_bytes at a time (the last chunk shorter): a line of any length passes, the consumer joins the pieces
extern "C" int hhx_text_reader_open_raw(const char *path, int64_t chunk_bytes, int n_threads, hhx_text_reader **out) {
    return text_reader_open(path, chunk_bytes, n_threads, false, -1, -1, out, true);
}
static int text_reader_open(const char *path, int64_t chunk_bytes, int n_threads, bool bgzf, int64_t begin, int64_t end, hhx_text_reader **out, bool raw) {
    if (!path || !out || chunk_bytes <= 0) return fail("hhx_text_reader_open: bad argument");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail("cannot open %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) { ::close(fd); return fail("cannot stat %s: %s", path, strerror(errno)); }
    if (bgzf) {
        unsigned char h[18];
        const ssize_t k = ::pread(fd, h, sizeof h, 0);
        const bool ok = k == (ssize_t)sizeof h && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C';
        if (!ok && st.st_size != 0) { ::close(fd); return fail("%s is not a BGZF file (bgzip); a plain gzip stream cannot be inflated in parallel", path); }
    }
    const bool ranged = begin >= 0;
    i64 lo = 0, hi = (i64)st.st_size, skip = 0, limit = -1;
    i64 text_bound = -1;                                               // BGZF: inflated bytes the reader can meet, from the ISIZE trailers
    if (ranged) begin = std::min<i64>(begin, st.st_size), end = std::min<i64>(end, st.st_size);
    if (bgzf && (ranged || st.st_size < 2 * chunk_bytes)) {           // (a large whole file needs no index: its buffers are two chunks whatever it inflates to)
        BgzfIndex ix;
        // a malformed block fails a range here.  The whole file goes on: its cap is bounded by the whole blocks in front of the bad one (+ 68 KB of
        // room, more than one block inflates to), and the reader reports the bad block when it gets there, as it did without the index
        if (bgzf_index(fd, (i64)st.st_size, ix) && ranged) { ::close(fd); return -1; }
        if (ranged) {
            // blocks [kb, ke) start in [begin, end); their text [text[kb], text[ke]), moved to line starts
            const size_t kb = (size_t)(std::lower_bound(ix.off.begin(), ix.off.end(), (i64)begin) - ix.off.begin());
            const size_t ke = (size_t)(std::lower_bound(ix.off.begin(), ix.off.end(), (i64)end) - ix.off.begin());
            i64 t0 = 0, t1 = 0;
            if (bgzf_line_start(fd, ix, ix.text[kb], t0) || bgzf_line_start(fd, ix, ix.text[ke], t1)) { ::close(fd); return -1; }
            if (t0 < t1) {
                const size_t k0 = (size_t)(std::upper_bound(ix.text.begin(), ix.text.end(), t0) - ix.text.begin()) - 1;       // the block holding text byte t0
                const size_t k1 = (size_t)(std::upper_bound(ix.text.begin(), ix.text.end(), t1 - 1) - ix.text.begin()) - 1;   // ... and t1 - 1
                lo = ix.off[k0];
                hi = ix.off[k1] + ix.bsize[k1];
                skip = t0 - ix.text[k0];
                limit = t1 - t0;
                text_bound = ix.text[k1 + 1] - ix.text[k0];
            } else lo = hi = 0;
        } else text_bound = ix.text.back();
    } else if (ranged) {
        if (plain_line_start(fd, (i64)st.st_size, begin, lo) || plain_line_start(fd, (i64)st.st_size, end, hi)) { ::close(fd); return -1; }
        if (hi < lo) hi = lo;
    }
    auto *r = new hhx_text_reader();
    r->fd = fd;
    r->at = lo;
    r->size = hi;
    r->skip = skip;
    r->limit = limit;
    r->chunk = (size_t)chunk_bytes;
    r->cap = 2 * (size_t)chunk_bytes + 4096;                           // a carried tail is shorter than a chunk (or the file has a line longer than one)
    r->bgzf = bgzf;
    r->raw = raw;
    if (!bgzf && (size_t)(hi - lo) + 4096 < r->cap) r->cap = (size_t)(hi - lo) + 4096;     // a small file: no more pinned memory than it has bytes (pinning costs ~0.5 ms per MB)
    if (bgzf && text_bound >= 0 && (size_t)text_bound + ((size_t)68 << 10) < r->cap) r->cap = (size_t)text_bound + ((size_t)68 << 10);   // the ISIZE trailers bound the text (+ one block of room)
    r->n_threads = n_threads > 0 ? std::min(n_threads, 16) : 4;
    for (int k = 0; k < 2; ++k)
        if (hipHostMalloc((void **)&r->buf[k], r->cap, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            for (int q = 0; q < k; ++q) (void)hipHostFree(r->buf[q]);
            const size_t cap = r->cap;
            ::close(fd);
            delete r;
            return fail("hhx_text_reader_open: no pinned memory for two buffers of %zu bytes", cap);
        }
    if (r->size <= r->at) r->eof = true;
    else r->th = std::thread([r] { r->loop(); });
    *out = r;
    return 0;
}

// the next chunk of whole lines: *host stays valid until the next call (the other buffer is being filled meanwhile); *n_bytes == 0: the end of the file
extern "C" int hhx_text_reader_next(hhx_text_reader *r, const uint8_t **host, int64_t *n_bytes) {
    if (!r || !host || !n_bytes) return fail("hhx_text_reader_next: null pointer");
    std::unique_lock<std::mutex> lk(r->mu);
    // the buffer handed out last time goes back to the reader: the caller is done with it (hhx_pairs_parse synchronises its stream after the
    // host -> device copy, before it returns)
    const int prev = r->take ^ 1;
    if (r->state[prev] == 2) { r->state[prev] = 0; r->cv.notify_all(); }
    r->cv.wait(lk, [r] { return r->state[r->take] == 1 || r->err || (r->eof && r->state[r->take] != 1); });
    if (r->err) return fail("reading the text file failed: %s", r->err == EOVERFLOW ? "a line is longer than a chunk" : r->err == EBADMSG ? r->emsg.c_str() : strerror(r->err));
    if (r->state[r->take] != 1) { *host = nullptr; *n_bytes = 0; return 0; }
    *host = r->buf[r->take];
    *n_bytes = r->len[r->take];
    r->state[r->take] = 2;
    r->take ^= 1;
    return 0;
}

extern "C" int hhx_text_reader_close(hhx_text_reader *r) {
    if (!r) return 0;
    { std::lock_guard<std::mutex> lk(r->mu); r->stop = true; }
    r->cv.notify_all();
    if (r->th.joinable()) r->th.join();
    for (int k = 0; k < 2; ++k) if (r->buf[k]) (void)hipHostFree(r->buf[k]);
    if (r->fd >= 0) ::close(r->fd);
    delete r;
    return 0;
}
