// The read set of a handle: the ABI calls that put reads on the device (host arrays, lent device arrays, synthetic reads, the
// FASTA one-shot, the chunked FASTA and FASTQ ingests with the one chunk pipeline they share) and those that reshape the
// resident reads there (split at non-bases, origins, reverse complement), with checksum, copy-back and the gather of a selection.
// A section of the one translation unit dbg_hip.hip, not self-contained: it needs dbg_hip_handle.h (dbg, dev_alloc / dev_free,
// buf_ensure, CHK / HIPCHK, grid_for, Timer), dbg_hip_scan.h (exclusive_scan and its functors, SCAN_TILE, k_startbits, k_synth,
// k_checksum), the kernel headers dbg_fasta.h, dbg_fastq.h, dbg_readsplit.h and dbg_revcomp.h, and free_build, free_reads,
// forget_alphabet and install_reads of dbg_hip.hip in front of it.  What stands behind it needs nothing of it.

static int make_startbits(dbg *h) {
    Timer t(h->stream);
    dev_free(h->d_startbits);
    h->startbits_words = (h->n_bytes + 1 + 31) / 32 + SB_WORDS + 2;
    CHK(dev_alloc(h, &h->d_startbits, h->startbits_words));
    HIPCHK(h, hipMemsetAsync(h->d_startbits, 0, h->startbits_words * 4, h->stream));
    hipLaunchKernelGGL(k_startbits, dim3(grid_for(h->n_reads + 1, 256)), dim3(256), 0, h->stream, h->d_offsets,
                       h->n_reads, h->d_startbits);
    HIPCHK(h, hipGetLastError());
    h->stats.ms_startbits = t.stop();
    return DBG_OK;
}

extern "C" int dbg_set_reads(dbg_t *h, const char *bases, const uint64_t *offsets, uint64_t n_reads) {
    if (!h || !offsets || (n_reads && !bases && offsets[n_reads] != 0)) return DBG_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (offsets[0] != 0) { h->err = "offsets[0] must be 0"; return DBG_E_ARG; }
    for (uint64_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i]) { h->err = "offsets must be non-decreasing"; return DBG_E_ARG; }
    free_build(h);
    free_reads(h);
    const uint64_t nb = offsets[n_reads];
    char *d_b = nullptr;
    uint64_t *d_o = nullptr;
    Timer t(h->stream);
    auto fill = [&]() -> int {
        CHK(dev_alloc(h, &d_b, nb + 64));
        CHK(dev_alloc(h, &d_o, n_reads + 1));
        if (nb) HIPCHK(h, hipMemcpyAsync(d_b, bases, nb, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_o, offsets, (n_reads + 1) * 8, hipMemcpyHostToDevice, h->stream));
        return DBG_OK;
    };
    const int rc = fill();
    if (rc != DBG_OK) { dev_free(d_b); dev_free(d_o); return rc; }
    h->stats.ms_h2d = t.stop();
    return install_reads(h, d_b, nb, d_o, n_reads, true);
}

extern "C" int dbg_set_reads_fasta(dbg_t *h, const char *text, uint64_t n_text) {
    if (!h || (n_text && !text)) return DBG_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    free_build(h);
    free_reads(h);
    char *d_text = nullptr, *bases = nullptr;
    uint32_t *bits = nullptr, *word_rank = nullptr, *len = nullptr;
    uint64_t *line_start = nullptr, *read_idx = nullptr, *byte_off = nullptr, *offsets = nullptr;
    uint8_t *is_read = nullptr;
    auto cleanup = [&]() {
        dev_free(d_text); dev_free(bits); dev_free(word_rank); dev_free(len); dev_free(line_start); dev_free(read_idx);
        dev_free(byte_off); dev_free(is_read);
    };
    int rc = DBG_OK;
    uint64_t n_lines = 0, n_reads = 0, n_bases = 0;
    do {
        Timer t(h->stream);
        if ((rc = dev_alloc(h, &d_text, n_text + 64)) != DBG_OK) break;
        if (n_text && hipMemcpyAsync(d_text, text, n_text, hipMemcpyHostToDevice, h->stream) != hipSuccess) { h->err = "H2D copy failed"; rc = DBG_E_HIP; break; }
        h->stats.ms_h2d = t.stop();
        const uint64_t n_words = (n_text + 31) / 32;
        if ((rc = dev_alloc(h, &bits, n_words)) != DBG_OK) break;
        if ((rc = dev_alloc(h, &word_rank, n_words)) != DBG_OK) break;
        if (n_words) {
            hipLaunchKernelGGL(k_fa_mark, dim3(grid_for(n_words, 256)), dim3(256), 0, h->stream, d_text, n_text, bits);
            if ((rc = exclusive_scan(h, n_words, PopcWords{bits}, word_rank, &n_lines)) != DBG_OK) break;
        }
        if ((rc = dev_alloc(h, &line_start, n_lines)) != DBG_OK) break;
        if ((rc = dev_alloc(h, &is_read, n_lines)) != DBG_OK) break;
        if ((rc = dev_alloc(h, &len, n_lines)) != DBG_OK) break;
        if ((rc = dev_alloc(h, &read_idx, n_lines)) != DBG_OK) break;
        if ((rc = dev_alloc(h, &byte_off, n_lines)) != DBG_OK) break;
        if (n_lines) {
            hipLaunchKernelGGL(k_fa_line_starts, dim3(grid_for(n_words, 256)), dim3(256), 0, h->stream, bits, word_rank, n_words,
                               line_start);
            hipLaunchKernelGGL(k_fa_lines, dim3(grid_for(n_lines, 256)), dim3(256), 0, h->stream, d_text, n_text, line_start,
                               n_lines, is_read, len);
            if ((rc = exclusive_scan(h, n_lines, ByteSet{is_read}, read_idx, &n_reads)) != DBG_OK) break;
            if ((rc = exclusive_scan(h, n_lines, U32At{len}, byte_off, &n_bases)) != DBG_OK) break;
        }
        if ((rc = dev_alloc(h, &bases, n_bases + 64)) != DBG_OK) break;
        if ((rc = dev_alloc(h, &offsets, n_reads + 1)) != DBG_OK) break;
        if (n_lines)
            hipLaunchKernelGGL(k_fa_copy, dim3(grid_for(n_lines * 16, 256)), dim3(256), 0, h->stream, d_text, line_start, n_lines,
                               is_read, len, read_idx, byte_off, bases, offsets);
        if (hipMemcpyAsync(offsets + n_reads, &n_bases, 8, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "FASTA ingest failed on the device"; rc = DBG_E_HIP; break; }
        h->ingest = dbg_ingest_stats_t{};
        h->ingest.bytes_read = n_text;
        h->ingest.chunks = 1;
        h->ingest.chunk_bytes = n_text;
        h->ingest.peak_device_bytes = (n_text + 64) + 8 * std::max<uint64_t>(n_words, 1) + 29 * std::max<uint64_t>(n_lines, 1) +
                                      (n_bases + 64) + 8 * (n_reads + 1);  // everything above is alive here at once
        h->ingest.n_reads = n_reads;
        h->ingest.n_bases = n_bases;
        h->ingest.ms_h2d = h->stats.ms_h2d;
    } while (0);
    cleanup();
    if (rc != DBG_OK) { dev_free(bases); dev_free(offsets); return rc; }
    return install_reads(h, bases, n_bases, offsets, n_reads, true);
}

// ------------------------------------------------------------------------------------------
// The chunk pipeline of the streamed ingests, FASTA and FASTQ.  Two pinned staging buffers: the host reads chunk i+1 while
// chunk i is copied and parsed on the handle's stream, one host wait per chunk and one more for each time a chunk runs
// again.  A format (FastaParse, FastqParse below) supplies its device state, double-buffered so that a chunk can run again
// after a buffer has grown, with a pinned host view of the state after the last chunk, and
//   parse_chunk(cs, n, si)           the chunk's kernels and the copies into the host view, all on the stream
//   reads_held() / reads_parsed()    the reads up to this chunk / after it, by the host view
//   chunk_read(cs, buf, pos, len)    told what the host has read; may end the chunk early (cs.stop, len)
//   before_chunk(cs, n)              room in bases for the chunk
//   after_parse(cs, n, si, done)     the checks on the host view, the retries, and taking the new state
// ------------------------------------------------------------------------------------------
constexpr uint64_t FS_DEFAULT_CHUNK = 16ull << 20;
constexpr uint64_t FS_MAX_CHUNK = 1ull << 30;  // the per-chunk counts of FsPopcPair are 32-bit

namespace {
struct ReadSource {  // a file, or an image in a host buffer (fd < 0)
    int fd = -1;
    const char *mem = nullptr;
    uint64_t size = 0;
    ReadSource() = default;
    ReadSource(const ReadSource &) = delete;
    ~ReadSource() { if (fd >= 0) close(fd); }
    // bytes [off, off + len) into buf: short only at the end of the source; -1 with errno after a failed read
    int64_t read(char *buf, uint64_t len, uint64_t off) const {
        uint64_t got = 0;
        if (fd < 0) {
            got = off < size ? std::min(len, size - off) : 0;
            if (got) memcpy(buf, mem + off, got);
        }
        while (fd >= 0 && got < len) {
            const ssize_t r = pread(fd, buf + got, std::min<uint64_t>(len - got, 1ull << 30), (off_t)(off + got));
            if (r < 0) {
                if (errno == EINTR) continue;
                return -1;
            }
            if (r == 0) break;
            got += (uint64_t)r;
        }
        return (int64_t)got;
    }
};

struct ChunkStream {
    using clock = std::chrono::steady_clock;
    dbg *h;
    const std::string name;  // of the source, in messages
    ReadSource src;
    char *pin[2] = {nullptr, nullptr};
    hipEvent_t ev_copy[2] = {nullptr, nullptr}, ev_t0 = nullptr, ev_done = nullptr;
    char *d_text = nullptr;       // the chunk on the device
    uint64_t *d_flags = nullptr;  // raised by a parse with bases past bases_cap (they were not written)
    char *bases = nullptr;
    uint64_t *offsets = nullptr;
    uint64_t bases_cap = 0, off_cap = 0;  // usable bytes (the allocation has 64 more) / entries
    uint64_t stage = 0, words_cap = 0, nblk_cap = 0;
    uint64_t cur = 0, peak = 0;   // device bytes held by the ingest
    uint64_t stop = UINT64_MAX;   // where the owned bytes end (UINT64_MAX: not seen yet)
    uint64_t closing = 0;         // the last offset, alive until its copy has run
    double range_len = 0;         // the range as known up front, for the projection of offsets_for
    double ms_io = 0, ms_h2d = 0, ms_parse = 0;
    std::vector<void *> dev, host;  // what alloc / pinned gave and release / install have not taken: the destructor's

    ChunkStream(dbg *hh, const char *nm) : h(hh), name(nm) {}
    ChunkStream(const ChunkStream &) = delete;
    ~ChunkStream() {  // every return of an ingest, early or not, comes through here
        (void)hipStreamSynchronize(h->stream);
        for (void *p : host) (void)hipHostFree(p);
        for (auto e : {ev_copy[0], ev_copy[1], ev_t0, ev_done}) if (e) (void)hipEventDestroy(e);
        for (void *p : dev) (void)hipFree(p);
        (void)hipGetLastError();
    }
    int open_file(const char *path) {
        src.fd = open(path, O_RDONLY | O_CLOEXEC);
        if (src.fd < 0) { h->err = name + ": " + strerror(errno); return DBG_E_ARG; }
        struct stat sb;
        if (fstat(src.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { h->err = name + ": not a readable regular file"; return DBG_E_ARG; }
        src.size = (uint64_t)sb.st_size;
        return DBG_OK;
    }
    template <class T>
    int pinned(T **p, uint64_t bytes) {
        HIPCHK(h, hipHostMalloc((void **)p, bytes, hipHostMallocDefault));
        host.push_back(*p);
        return DBG_OK;
    }
    template <class T>
    int alloc(T **p, uint64_t count) {
        CHK(dev_alloc(h, p, count));
        dev.push_back(*p);
        cur += std::max<uint64_t>(count, 1) * sizeof(T);
        peak = std::max(peak, cur);
        return DBG_OK;
    }
    void forget(void *p) {
        const auto it = std::find(dev.begin(), dev.end(), p);
        if (it != dev.end()) dev.erase(it);
    }
    template <class T>
    void release(T *&p, uint64_t count) {
        if (p) cur -= std::max<uint64_t>(count, 1) * sizeof(T);
        forget(p);
        dev_free(p);
    }
    template <class T>
    int grow(T *&p, uint64_t &cap, uint64_t new_cap, uint64_t keep, uint64_t pad) {  // keep: elements to carry over
        T *q = nullptr;
        CHK(alloc(&q, new_cap + pad));
        if (keep) HIPCHK(h, hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
        release(p, cap + pad);
        p = q;
        cap = new_cap;
        return DBG_OK;
    }
    // staging and the parts of the parse state that every format has, for chunks of up to `chunk` bytes of `span` bytes
    int setup(uint64_t chunk, uint64_t span, uint64_t bases_cap0, uint64_t off_cap0) {
        stage = std::max<uint64_t>(std::min(chunk, span), 1);
        words_cap = (stage + 31) / 32;
        nblk_cap = (words_cap + FS_WPB - 1) / FS_WPB;
        for (auto &p : pin) CHK(pinned(&p, stage));
        for (auto *e : {&ev_copy[0], &ev_copy[1], &ev_t0, &ev_done}) HIPCHK(h, hipEventCreate(e));
        CHK(alloc(&d_text, stage + 64));
        CHK(alloc(&d_flags, 1));
        cur += (std::max<uint64_t>((words_cap + SCAN_TILE - 1) / SCAN_TILE, 1) + 1) * 8;  // scan partials (handle arena)
        peak = std::max(peak, cur);
        bases_cap = bases_cap0;
        CHK(alloc(&bases, bases_cap + 64));
        off_cap = off_cap0;  // the offsets start small and grow as reads arrive
        CHK(alloc(&offsets, off_cap));
        HIPCHK(h, hipMemsetAsync(d_flags, 0, 8, h->stream));
        for (auto e : ev_copy) HIPCHK(h, hipEventRecord(e, h->stream));  // "buffer free" holds from the start
        return DBG_OK;
    }
    template <class F>
    int read_chunk(F &f, int b, uint64_t pos, uint64_t &len) {
        const uint64_t limit = stop == UINT64_MAX ? src.size : stop;
        len = pos < limit ? std::min(stage, limit - pos) : 0;
        if (!len) return DBG_OK;
        const auto t0 = clock::now();
        const int64_t got = src.read(pin[b], len, pos);
        ms_io += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
        if (got < 0) { h->err = name + ": read failed: " + strerror(errno); return DBG_E_ARG; }
        len = (uint64_t)got;  // short: the file ended early
        h->ingest.bytes_read += len;
        f.chunk_read(*this, pin[b], pos, len);
        return DBG_OK;
    }
    uint64_t offsets_for(uint64_t n_reads, uint64_t done, uint64_t at_least) const {  // amortised: 1.5x, or the projection
        const double proj = done ? (double)n_reads * std::max(range_len, (double)done) / (double)done * 1.05 + 1024 : 0;
        return std::max<uint64_t>({at_least, off_cap + off_cap / 2, (uint64_t)proj});
    }
    template <class F>
    int timed_parse(F &f, uint64_t n, int si) {  // a chunk again, after a buffer has grown
        HIPCHK(h, hipEventRecord(ev_t0, h->stream));
        CHK(f.parse_chunk(*this, n, si));
        HIPCHK(h, hipEventRecord(ev_done, h->stream));
        HIPCHK(h, hipEventSynchronize(ev_done));
        float c = 0;
        (void)hipEventElapsedTime(&c, ev_t0, ev_done);
        ms_parse += c;
        return DBG_OK;
    }
    template <class F>
    int offsets_retry(F &f, uint64_t n, int si, uint64_t done) {  // more reads than the estimate: grow and parse the chunk again
        const uint64_t held = f.reads_held(), parsed = f.reads_parsed();
        if (parsed + 1 <= off_cap) return DBG_OK;
        CHK(grow(offsets, off_cap, offsets_for(held, done + n, parsed + 1), held, 0));
        return timed_parse(f, n, si);
    }
    template <class F>
    int run(F &f, uint64_t start) {
        uint64_t len[2] = {0, 0}, pos = start;
        CHK(read_chunk(f, 0, pos, len[0]));
        int b = 0, si = 0;
        while (len[b] > 0) {
            const uint64_t n = len[b], done = pos - start, held = f.reads_held();
            CHK(f.before_chunk(*this, n));
            if (done) {  // the offsets this chunk will likely need, at the read density seen so far
                const uint64_t est = held + (uint64_t)((double)held * n / done * 1.25) + 64;
                if (est + 1 > off_cap) CHK(grow(offsets, off_cap, offsets_for(held, done, est + 1), held, 0));
            }
            HIPCHK(h, hipEventRecord(ev_t0, h->stream));
            HIPCHK(h, hipMemcpyAsync(d_text, pin[b], n, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipEventRecord(ev_copy[b], h->stream));
            CHK(f.parse_chunk(*this, n, si));
            HIPCHK(h, hipEventRecord(ev_done, h->stream));
            // the other buffer is free once its copy (chunk i-1) has completed: read chunk i+1 into it meanwhile
            const uint64_t npos = pos + n;
            HIPCHK(h, hipEventSynchronize(ev_copy[b ^ 1]));
            CHK(read_chunk(f, b ^ 1, npos, len[b ^ 1]));
            HIPCHK(h, hipEventSynchronize(ev_done));
            float a = 0, c = 0;
            (void)hipEventElapsedTime(&a, ev_t0, ev_copy[b]);
            (void)hipEventElapsedTime(&c, ev_copy[b], ev_done);
            ms_h2d += a;
            ms_parse += c;
            CHK(f.after_parse(*this, n, si, done));
            si ^= 1;
            b ^= 1;
            pos = npos;
            ++h->ingest.chunks;
        }
        return DBG_OK;
    }
    int close_offsets(uint64_t n_reads, uint64_t n_bases) {
        closing = n_bases;
        HIPCHK(h, hipMemcpyAsync(offsets + n_reads, &closing, 8, hipMemcpyHostToDevice, h->stream));
        return DBG_OK;
    }
    // bases / offsets become the handle's read set, once the stream has run everything queued on them
    int install(uint64_t n_reads, uint64_t n_bases, clock::time_point t_call) {
        forget(bases);
        forget(offsets);
        h->ingest.peak_device_bytes = peak;
        h->ingest.n_reads = n_reads;
        h->ingest.n_bases = n_bases;
        h->ingest.ms_io_wait = ms_io;
        h->ingest.ms_h2d = ms_h2d;
        h->ingest.ms_parse = ms_parse;
        h->stats.ms_h2d = ms_h2d;
        const int rc = install_reads(h, bases, n_bases, offsets, n_reads, true);
        h->ingest.ms_total = std::chrono::duration<double, std::milli>(clock::now() - t_call).count();
        return rc;
    }
};

// ---- FASTA (kernels: dbg_fasta.h): the stream state is the byte cursor, the read count and the line open at the chunk
//      border.  In record mode (dbg_set_reads_fasta_records*) a read is a record and the owned bytes are known up front; in
//      line mode the last owned line ends at the first line start at or past lim, which the host finds as it reads.
struct FastaParse {
    struct HostView {
        FsState st;
        uint64_t flags;
        uint64_t n_seq;  // record mode: sequence line starts of the last chunk
    };
    const bool records;
    const std::string call;  // the ABI call, in messages
    uint64_t lim = 0;        // line starts at or past lim are not owned: they end the last owned line
    uint32_t host_prev = '\n';  // the byte before the next chunk
    HostView *hv = nullptr;  // pinned: the state after the last chunk
    uint32_t *d_wr = nullptr, *d_rs = nullptr;
    uint64_t *d_rank = nullptr, *d_nseq = nullptr;
    uint8_t *d_blk = nullptr;  // two byte arrays of nblk_cap
    FsState *d_state = nullptr;
    FsChunk *d_chunk = nullptr;
    FsState hs{};  // the state after the last chunk taken
    uint64_t n_seq_lines = 0;

    FastaParse(bool rec, const std::string &c) : records(rec), call(c) {}
    int setup(ChunkStream &cs, uint32_t prev) {
        dbg *h = cs.h;
        CHK(cs.pinned(&hv, sizeof(HostView)));
        if (records) CHK(cs.alloc(&d_nseq, 1));
        CHK(cs.alloc(&d_wr, cs.words_cap));
        CHK(cs.alloc(&d_rs, cs.words_cap));
        CHK(cs.alloc(&d_rank, cs.words_cap));
        CHK(cs.alloc(&d_blk, 2 * cs.nblk_cap));
        CHK(cs.alloc(&d_state, 2));
        CHK(cs.alloc(&d_chunk, 1));
        hv->st = hs = FsState{0, 0, 0, prev, 0};  // record mode: the stream begins at a header line start
        hv->n_seq = 0;
        host_prev = prev;
        HIPCHK(h, hipMemcpyAsync(d_state, &hv->st, sizeof(FsState), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return DBG_OK;
    }
    int parse_chunk(ChunkStream &cs, uint64_t n, int si) {
        dbg *h = cs.h;
        const uint64_t words = (n + 31) / 32, nblk = (words + FS_WPB - 1) / FS_WPB;
        const FsState *in = d_state + si;
        uint8_t *blk_f = d_blk, *blk_b = d_blk + cs.nblk_cap;
        hipLaunchKernelGGL(k_fs_blocks, dim3((unsigned)nblk), dim3(256), 0, h->stream, cs.d_text, n, in, blk_f, blk_b);
        hipLaunchKernelGGL(k_fs_carry, dim3(1), dim3(256), 0, h->stream, blk_f, blk_b, nblk, in, d_chunk);
        if (records) {
            HIPCHK(h, hipMemsetAsync(d_nseq, 0, 8, h->stream));
            hipLaunchKernelGGL(k_fs_count<true>, dim3((unsigned)nblk), dim3(256), 0, h->stream, cs.d_text, n, in, (const uint8_t *)blk_f,
                               (const uint8_t *)blk_b, d_wr, d_rs, d_chunk, (unsigned long long *)d_nseq);
        } else {
            hipLaunchKernelGGL(k_fs_count<false>, dim3((unsigned)nblk), dim3(256), 0, h->stream, cs.d_text, n, in, (const uint8_t *)blk_f,
                               (const uint8_t *)blk_b, d_wr, d_rs, d_chunk, (unsigned long long *)nullptr);
        }
        CHK(exclusive_scan(h, words, FsPopcPair{d_wr, d_rs}, d_rank, (uint64_t *)nullptr));
        const uint64_t *total = (const uint64_t *)h->ar_scan.p + std::max<uint64_t>((words + SCAN_TILE - 1) / SCAN_TILE, 1);
        hipLaunchKernelGGL(k_fs_write, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, cs.d_text, n, in, (const FsChunk *)d_chunk,
                           (const uint32_t *)d_wr, (const uint32_t *)d_rs, (const uint64_t *)d_rank, cs.bases, cs.bases_cap,
                           cs.offsets, cs.off_cap, cs.d_flags);
        hipLaunchKernelGGL(k_fs_finish, dim3(1), dim3(64), 0, h->stream, cs.d_text, n, in, (const FsChunk *)d_chunk, total,
                           d_state + (si ^ 1));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(&hv->st, d_state + (si ^ 1), sizeof(FsState), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&hv->flags, cs.d_flags, 8, hipMemcpyDeviceToHost, h->stream));
        if (records) HIPCHK(h, hipMemcpyAsync(&hv->n_seq, d_nseq, 8, hipMemcpyDeviceToHost, h->stream));
        return DBG_OK;
    }
    uint64_t reads_held() const { return hs.n_reads; }
    uint64_t reads_parsed() const { return hv->st.n_reads; }
    void chunk_read(ChunkStream &cs, const char *buf, uint64_t pos, uint64_t &len) {
        if (cs.stop == UINT64_MAX && pos + len > lim) {  // the last owned line ends at the first line start at or past lim
            for (uint64_t p = std::max(lim, pos); p < pos + len; ++p) {
                const uint32_t pv = p == pos ? host_prev : (uint8_t)buf[p - pos - 1], c = (uint8_t)buf[p - pos];
                if (pv == '\n' || (pv == '\r' && c != '\n')) { cs.stop = p; break; }
            }
            if (cs.stop != UINT64_MAX) len = cs.stop - pos;
        }
        if (len) host_prev = (uint8_t)buf[len - 1];
    }
    int before_chunk(ChunkStream &cs, uint64_t n) {
        if (hs.cursor + hs.pend + n > cs.bases_cap)  // only a last line that runs far past `end`
            CHK(cs.grow(cs.bases, cs.bases_cap, std::max(hs.cursor + hs.pend + n, cs.bases_cap + cs.bases_cap / 2),
                        hs.cursor + hs.pend, 64));
        return DBG_OK;
    }
    int after_parse(ChunkStream &cs, uint64_t n, int si, uint64_t done) {
        CHK(cs.offsets_retry(*this, n, si, done));
        if (hv->flags) { cs.h->err = call + ": packed bases overran their buffer (internal error)"; return DBG_E_HIP; }
        hs = hv->st;
        n_seq_lines += hv->n_seq;
        return DBG_OK;
    }
};
}  // namespace

// record mode: the header line start at or after `from` (`size` if none), by windows with the byte in front as prev.
// *first_seq: the first non-space byte in front of it (~0: none); *scanned counts the bytes read.
static int fasta_header_start(const ReadSource &src, uint64_t from, uint64_t *out, uint64_t *first_seq, uint64_t *scanned) {
    const uint64_t size = src.size;
    *out = size;
    *first_seq = ~0ull;
    if (from >= size) return 0;
    std::vector<uint8_t> win(1 << 16);
    uint32_t prev = '\n';  // before the file: byte 0 starts a line
    if (from) {
        if (src.read((char *)win.data(), 1, from - 1) != 1) return -1;
        prev = win[0];
        ++*scanned;
    }
    FaHeaderScan scan(prev);
    for (uint64_t pos = from; pos < size; pos += win.size()) {
        const uint64_t len = std::min<uint64_t>(win.size(), size - pos);
        if (src.read((char *)win.data(), len, pos) != (int64_t)len) return -1;
        *scanned += len;
        const bool hit = scan.feed(win.data(), len, pos);
        *first_seq = scan.first_seq;
        if (hit) { *out = scan.found; return 0; }
    }
    return 0;
}

// the streamed ingest of a file (path) or of an image in a host buffer (mem, mem_size), in line or in record mode
static int fasta_stream_ingest(dbg *h, const char *what, const char *path, const char *mem, uint64_t mem_size, uint64_t begin,
                               uint64_t end, uint64_t chunk_bytes, bool records) {
    const auto t_call = ChunkStream::clock::now();
    const std::string call(what);
    if (!path && !mem && mem_size) { h->err = call + (records ? ": no text" : ": no path"); return DBG_E_ARG; }
    if (begin > end) {
        h->err = call + ": begin " + std::to_string(begin) + " > end " + std::to_string(end);
        return DBG_E_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    ChunkStream cs(h, path ? path : "text");
    cs.src.mem = mem;
    cs.src.size = mem_size;
    if (path) CHK(cs.open_file(path));
    const uint64_t size = cs.src.size;
    uint64_t lim = std::min(end, size);      // line starts at or past lim are not owned: they end the last owned line
    uint64_t start = std::min(begin, size);
    uint32_t prev = '\n';                    // before the file: byte 0 starts a line
    uint64_t scan_bytes = 0;
    if (records) {  // the owned bytes: from the first header at or after begin to the first at or after end
        uint64_t seq0 = ~0ull, seq1 = ~0ull;
        if (fasta_header_start(cs.src, start, &start, &seq0, &scan_bytes) != 0 ||
            fasta_header_start(cs.src, std::max(lim, start), &lim, &seq1, &scan_bytes) != 0) {
            h->err = cs.name + ": read failed: " + strerror(errno);
            return DBG_E_ARG;
        }
        if (begin == 0 && seq0 != ~0ull) {
            free_build(h);
            free_reads(h);
            h->err = call + ": " + cs.name + ": malformed FASTA: sequence before the first header at byte " + std::to_string(seq0);
            return DBG_E_ARG;
        }
    } else if (start > 0 && start < size) {
        char c;
        if (cs.src.read(&c, 1, start - 1) != 1) { h->err = cs.name + ": read failed: " + strerror(errno); return DBG_E_ARG; }
        prev = (uint8_t)c;
    }
    const uint64_t chunk = chunk_bytes ? std::min(chunk_bytes, FS_MAX_CHUNK) : FS_DEFAULT_CHUNK;
    free_build(h);
    free_reads(h);
    h->ingest = dbg_ingest_stats_t{};
    h->ingest.chunk_bytes = chunk;
    h->ingest.bytes_read = records ? scan_bytes : (start > 0 && start < size) ? 1 : 0;
    if (records) {
        h->fasta_rec = dbg_fasta_records_stats_t{};
        h->fasta_rec.first_byte = start;
        h->fasta_rec.end_byte = lim;
        h->fasta_rec.scan_bytes = scan_bytes;
    }

    FastaParse fa(records, call);
    fa.lim = lim;
    const uint64_t range = lim > start ? lim - start : 0;  // the packed bases of a range are at most its length
    cs.range_len = (double)range;
    // first line start at or past lim (UINT64_MAX: not seen yet); record mode knows it: the stream ends at a header
    cs.stop = (records || lim >= size) ? lim : UINT64_MAX;
    CHK(cs.setup(chunk, (records ? lim : size) - start, range, std::min<uint64_t>(1 << 16, range + 2)));
    CHK(fa.setup(cs, prev));
    CHK(cs.run(fa, start));

    const uint64_t n_reads = fa.hs.n_reads, n_bases = fa.hs.cursor;  // the pending white space of the last line is dropped
    CHK(cs.close_offsets(n_reads, n_bases));
    if (records) {
        HIPCHK(h, hipMemsetAsync(fa.d_nseq, 0, 8, h->stream));
        if (n_reads) {
            const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(n_reads, 256), 1024);
            hipLaunchKernelGGL(k_fs_longest, dim3(grid), dim3(256), 0, h->stream, (const uint64_t *)cs.offsets, n_reads,
                               (unsigned long long *)fa.d_nseq);
            HIPCHK(h, hipGetLastError());
        }
        HIPCHK(h, hipMemcpyAsync(&fa.hv->n_seq, fa.d_nseq, 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (records) {
        h->fasta_rec.n_records = n_reads;
        h->fasta_rec.n_sequence_lines = fa.n_seq_lines;
        h->fasta_rec.longest_record = fa.hv->n_seq;
    }
    return cs.install(n_reads, n_bases, t_call);
}


extern "C" int dbg_set_reads_fasta_file(dbg_t *h, const char *path, uint64_t begin, uint64_t end, uint64_t chunk_bytes) {
    if (!h) return DBG_E_ARG;
    if (!path) { h->err = "set_reads_fasta_file: no path"; return DBG_E_ARG; }
    return fasta_stream_ingest(h, "set_reads_fasta_file", path, nullptr, 0, begin, end, chunk_bytes, false);
}

extern "C" int dbg_set_reads_fasta_records_file(dbg_t *h, const char *path, uint64_t begin, uint64_t end, uint64_t chunk_bytes) {
    if (!h) return DBG_E_ARG;
    if (!path) { h->err = "set_reads_fasta_records_file: no path"; return DBG_E_ARG; }
    return fasta_stream_ingest(h, "set_reads_fasta_records_file", path, nullptr, 0, begin, end, chunk_bytes, true);
}

// the whole image in a host buffer: one range through the same stream (the buffer is staged chunk by chunk)
extern "C" int dbg_set_reads_fasta_records(dbg_t *h, const char *text, uint64_t n_text) {
    if (!h || (n_text && !text)) return DBG_E_ARG;
    return fasta_stream_ingest(h, "set_reads_fasta_records", nullptr, text, n_text, 0, UINT64_MAX, 0, true);
}

extern "C" int dbg_fasta_records_stats(dbg_t *h, dbg_fasta_records_stats_t *out) {
    if (!h || !out) return DBG_E_ARG;
    *out = h->fasta_rec;
    return DBG_OK;
}

extern "C" int dbg_fasta_ingest_stats(dbg_t *h, dbg_ingest_stats_t *out) {
    if (!h || !out) return DBG_E_ARG;
    *out = h->ingest;
    return DBG_OK;
}

// ------------------------------------------------------------------------------------------
// chunked FASTQ ingest from a file (kernels and the plain-C++ searches: dbg_fastq.h), through the chunk pipeline above.  The
// stream state is the line count, the sequence and quality cursors and the line open at the chunk border.  The host knows
// the owned bytes [first record start, next range's first record start) before the first chunk, so no chunk looks for its
// end.  With a mask the quality bytes are kept at the places of their bases until k_fq_mask has run.
// ------------------------------------------------------------------------------------------
namespace {
struct FastqParse {
    struct HostView {
        FqState st;
        uint64_t flags, err;
    };
    const std::string path;
    HostView *hv = nullptr;  // pinned: the state after the last chunk
    uint32_t *d_wr = nullptr, *d_wq = nullptr, *d_ls = nullptr, *d_lidx = nullptr, *d_blk_ls = nullptr;
    uint64_t *d_rank = nullptr;
    uint8_t *d_blk = nullptr;
    FqState *d_state = nullptr;
    FqChunk *d_chunk = nullptr;
    uint64_t *d_err = nullptr;  // [0] the least (record, kind) of a malformed file [1] masked bases
    char *qual = nullptr;       // quality bytes at the places of their bases (mask on), bases_cap + 64 bytes
    FqState hs{};               // the state after the last chunk taken

    explicit FastqParse(const char *p) : path(p) {}
    static uint64_t records_of(uint64_t n_lines) { return (n_lines + 2) / 4; }  // sequence lines among the lines so far
    int malformed(dbg *h, uint64_t key) const {
        h->err = "set_reads_fastq_file: " + path + ": malformed FASTQ: record " + std::to_string(key >> 3) + ": " +
                 fq_kind_name((uint32_t)(key & 7));
        return DBG_E_ARG;
    }
    int setup(ChunkStream &cs, bool mask) {
        dbg *h = cs.h;
        CHK(cs.pinned(&hv, sizeof(HostView)));
        CHK(cs.alloc(&d_wr, cs.words_cap));
        CHK(cs.alloc(&d_wq, cs.words_cap));
        CHK(cs.alloc(&d_ls, cs.words_cap));
        CHK(cs.alloc(&d_lidx, cs.words_cap));
        CHK(cs.alloc(&d_rank, cs.words_cap));
        CHK(cs.alloc(&d_blk, cs.nblk_cap));
        CHK(cs.alloc(&d_blk_ls, cs.nblk_cap));
        CHK(cs.alloc(&d_state, 2));
        CHK(cs.alloc(&d_chunk, 1));
        CHK(cs.alloc(&d_err, 2));
        if (mask) CHK(cs.alloc(&qual, cs.bases_cap + 64));
        HIPCHK(h, hipMemsetAsync(d_err, 0xFF, 8, h->stream));
        HIPCHK(h, hipMemsetAsync(d_err + 1, 0, 8, h->stream));
        hv->st = hs = FqState{0, 0, 0, 0, '\n', 0};  // a record start is a line start
        hv->flags = 0;
        hv->err = FQ_NO_ERROR;
        HIPCHK(h, hipMemcpyAsync(d_state, &hv->st, sizeof(FqState), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return DBG_OK;
    }
    int parse_chunk(ChunkStream &cs, uint64_t n, int si) {
        dbg *h = cs.h;
        const uint64_t words = (n + 31) / 32, nblk = (words + FS_WPB - 1) / FS_WPB;
        const FqState *in = d_state + si;
        hipLaunchKernelGGL(k_fq_blocks, dim3((unsigned)nblk), dim3(256), 0, h->stream, cs.d_text, n, in, d_blk_ls, d_blk);
        hipLaunchKernelGGL(k_fq_carry, dim3(1), dim3(256), 0, h->stream, d_blk_ls, d_blk, nblk, in, d_chunk);
        hipLaunchKernelGGL(k_fq_count, dim3((unsigned)nblk), dim3(256), 0, h->stream, cs.d_text, n, in, (const uint32_t *)d_blk_ls,
                           (const uint8_t *)d_blk, d_wr, d_wq, d_ls, d_lidx, d_chunk);
        CHK(exclusive_scan(h, words, FqPopcPair{d_wr, d_wq}, d_rank, (uint64_t *)nullptr));
        const uint64_t *total = (const uint64_t *)h->ar_scan.p + std::max<uint64_t>((words + SCAN_TILE - 1) / SCAN_TILE, 1);
        hipLaunchKernelGGL(k_fq_write, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, cs.d_text, n, in, (const FqChunk *)d_chunk,
                           (const uint32_t *)d_wr, (const uint32_t *)d_wq, (const uint32_t *)d_ls, (const uint32_t *)d_lidx,
                           (const uint64_t *)d_rank, cs.bases, qual, cs.bases_cap, cs.offsets, cs.off_cap, cs.d_flags,
                           (unsigned long long *)d_err);
        hipLaunchKernelGGL(k_fq_finish, dim3(1), dim3(64), 0, h->stream, cs.d_text, n, in, (const FqChunk *)d_chunk, total,
                           d_state + (si ^ 1));
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(&hv->st, d_state + (si ^ 1), sizeof(FqState), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&hv->flags, cs.d_flags, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(&hv->err, d_err, 8, hipMemcpyDeviceToHost, h->stream));
        return DBG_OK;
    }
    uint64_t reads_held() const { return records_of(hs.n_lines); }
    uint64_t reads_parsed() const { return records_of(hv->st.n_lines); }
    void chunk_read(ChunkStream &, const char *, uint64_t, uint64_t &) {}
    int before_chunk(ChunkStream &, uint64_t) { return DBG_OK; }  // a record's sequence is under half its bytes
    int after_parse(ChunkStream &cs, uint64_t n, int si, uint64_t done) {
        dbg *h = cs.h;
        if (hv->err != FQ_NO_ERROR) return malformed(h, hv->err);  // every check in front of it has run: it is the first
        CHK(cs.offsets_retry(*this, n, si, done));
        if (hv->flags) {
            // Kept bytes past half the range: only a file whose quality lines are shorter than its reads, which the next
            // header reports.  Until then the buffers grow and the chunk runs again; nothing was written out of bounds.
            const uint64_t keep = std::min(cs.bases_cap, std::max(hs.cur_s, hs.cur_q) + hs.pend);
            const uint64_t cap = std::max(std::max(hs.cur_s, hs.cur_q) + hs.pend + n, cs.bases_cap + cs.bases_cap / 2);
            uint64_t qcap = cs.bases_cap;
            CHK(cs.grow(cs.bases, cs.bases_cap, cap, keep, 64));
            if (qual) CHK(cs.grow(qual, qcap, cap, keep, 64));
            HIPCHK(h, hipMemsetAsync(cs.d_flags, 0, 8, h->stream));
            CHK(cs.timed_parse(*this, n, si));
            if (hv->flags) { h->err = "set_reads_fastq_file: packed bases overran their buffer (internal error)"; return DBG_E_HIP; }
        }
        hs = hv->st;
        return DBG_OK;
    }
};
}  // namespace

// the file without its trailing white space: *out = position after the last non-space byte (0: there is none)
static int fastq_trimmed_size(const ReadSource &src, uint64_t *out) {
    std::vector<uint8_t> win(1 << 16);
    uint64_t hi = src.size;
    while (hi) {
        const uint64_t lo = hi > win.size() ? hi - win.size() : 0;
        if (src.read((char *)win.data(), hi - lo, lo) != (int64_t)(hi - lo)) return -1;
        const uint64_t keep = fq_trim(win.data(), hi - lo);
        if (keep) { *out = lo + keep; return 0; }
        hi = lo;
    }
    *out = 0;
    return 0;
}

// the record start at or after `from` in the file that ends at `size` (its trailing white space trimmed): `size` if none
static int fastq_record_start(const ReadSource &src, uint64_t from, uint64_t size, uint64_t *out) {
    *out = std::min(from, size);
    if (from == 0 || from >= size) return 0;  // the file begins with a record
    std::vector<uint8_t> win(1 << 16);
    if (src.read((char *)win.data(), 1, from - 1) != 1) return -1;
    FqStartScan scan(win[0]);
    for (uint64_t pos = from; pos < size; pos += win.size()) {
        const uint64_t len = std::min<uint64_t>(win.size(), size - pos);
        if (src.read((char *)win.data(), len, pos) != (int64_t)len) return -1;
        if (scan.feed(win.data(), len, pos)) { *out = scan.found; return 0; }
    }
    *out = size;
    return 0;
}

extern "C" int dbg_set_reads_fastq_file(dbg_t *h, const char *path, uint64_t begin, uint64_t end, uint64_t chunk_bytes,
                                        uint32_t min_quality) {
    if (!h) return DBG_E_ARG;
    const auto t_call = ChunkStream::clock::now();
    if (!path) { h->err = "set_reads_fastq_file: no path"; return DBG_E_ARG; }
    if (begin > end) {
        h->err = "set_reads_fastq_file: begin " + std::to_string(begin) + " > end " + std::to_string(end);
        return DBG_E_ARG;
    }
    if (min_quality > 93) { h->err = "set_reads_fastq_file: min_quality " + std::to_string(min_quality) + " > 93"; return DBG_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    ChunkStream cs(h, path);
    CHK(cs.open_file(path));
    uint64_t size = 0, start = 0, stop = 0;
    if (fastq_trimmed_size(cs.src, &size) != 0 || fastq_record_start(cs.src, begin, size, &start) != 0 ||
        fastq_record_start(cs.src, end, size, &stop) != 0) {
        h->err = cs.name + ": read failed: " + strerror(errno);
        return DBG_E_ARG;
    }
    const uint64_t chunk = chunk_bytes ? std::min(chunk_bytes, FS_MAX_CHUNK) : FS_DEFAULT_CHUNK;
    free_build(h);
    free_reads(h);
    h->ingest = dbg_ingest_stats_t{};
    h->ingest.chunk_bytes = chunk;
    h->fastq = dbg_fastq_stats_t{};
    h->fastq.min_quality = min_quality;
    h->fastq.first_byte = start;
    h->fastq.end_byte = stop;

    FastqParse fq(path);
    const uint64_t range = stop - start;
    cs.range_len = (double)range;
    cs.stop = stop;
    // a record's sequence is under half its bytes, and a record has six bytes or more
    CHK(cs.setup(chunk, range, range / 2, std::min<uint64_t>(1 << 16, range / 6 + 2)));
    CHK(fq.setup(cs, min_quality != 0));
    CHK(cs.run(fq, start));

    // the end of the range: whole records, or a last record of the file with an empty read and no quality line.  The
    // pending white space of the last line is dropped (cur_s, cur_q do not count it).
    const FqState &hs = fq.hs;
    const uint64_t n_reads = fq.reads_held(), n_bases = hs.cur_s;
    if ((hs.n_lines & 3) == 1 || (hs.n_lines & 3) == 2) return fq.malformed(h, (hs.n_lines >> 2) * 8 + FQ_E_TRUNCATED);
    if (hs.cur_s != hs.cur_q) return fq.malformed(h, (n_reads - 1) * 8 + FQ_E_LENGTH);
    CHK(cs.close_offsets(n_reads, n_bases));
    if (fq.qual) {
        HIPCHK(h, hipEventRecord(cs.ev_t0, h->stream));
        if (n_bases) {
            hipLaunchKernelGGL(k_fq_mask, dim3(grid_for((n_bases + 15) / 16, 256)), dim3(256), 0, h->stream, cs.bases,
                               (const char *)fq.qual, n_bases, min_quality, (const uint64_t *)cs.offsets, n_reads,
                               (unsigned long long *)(fq.d_err + 1), (unsigned long long *)fq.d_err);
            HIPCHK(h, hipGetLastError());
        }
        HIPCHK(h, hipEventRecord(cs.ev_done, h->stream));
        uint64_t res[2] = {FQ_NO_ERROR, 0};
        HIPCHK(h, hipMemcpyAsync(res, fq.d_err, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        float c = 0;
        (void)hipEventElapsedTime(&c, cs.ev_t0, cs.ev_done);
        h->fastq.ms_mask = c;
        if (res[0] != FQ_NO_ERROR) return fq.malformed(h, res[0]);
        h->fastq.masked_bases = res[1];
        h->fastq.quality_bytes_held = cs.bases_cap + 64;
        cs.release(fq.qual, cs.bases_cap + 64);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->fastq.n_records = n_reads;
    h->fastq.peak_device_bytes = cs.peak;
    return cs.install(n_reads, n_bases, t_call);
}


extern "C" int dbg_fastq_ingest_stats(dbg_t *h, dbg_fastq_stats_t *out) {
    if (!h || !out) return DBG_E_ARG;
    *out = h->fastq;
    return DBG_OK;
}

extern "C" int dbg_set_reads_device(dbg_t *h, const void *d_bases, uint64_t n_bytes, const void *d_offsets,
                                    uint64_t n_reads) {
    if (!h || !d_offsets || (n_bytes && !d_bases)) return DBG_E_ARG;
    if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_offsets & 7)) { h->err = "device buffers must be 16/8-byte aligned"; return DBG_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    free_build(h);
    free_reads(h);
    return install_reads(h, (char *)d_bases, n_bytes, (uint64_t *)d_offsets, n_reads, false);  // lent: never written, never freed
}

extern "C" int dbg_synth_reads(dbg_t *h, uint64_t seed, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                               uint32_t read_len, uint32_t err_thr24) {
    if (!h || read_len == 0 || genome_len < read_len) return DBG_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    free_build(h);
    free_reads(h);
    const uint64_t nb = n_reads * read_len;
    char *d_b = nullptr;
    uint64_t *d_o = nullptr;
    auto fill = [&]() -> int {
        CHK(dev_alloc(h, &d_b, nb + 64));
        CHK(dev_alloc(h, &d_o, n_reads + 1));
        const uint64_t golden = 0x9E3779B97F4A7C15ull;
        const uint64_t kg = mix64(seed + 1 * golden), ks = mix64(seed + 2 * golden), ke = mix64(seed + 3 * golden);
        const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, (nb + 255) / 256), 1u << 20);
        hipLaunchKernelGGL(k_synth, dim3(grid), dim3(256), 0, h->stream, d_b, d_o, kg, ks, ke, genome_len, first_read, n_reads,
                           read_len, err_thr24);
        HIPCHK(h, hipGetLastError());
        return DBG_OK;
    };
    const int rc = fill();
    if (rc != DBG_OK) { dev_free(d_b); dev_free(d_o); return rc; }
    return install_reads(h, d_b, nb, d_o, n_reads, true);
}

extern "C" int dbg_reads_checksum(dbg_t *h, uint64_t *out) {
    if (!h || !out) return DBG_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->d_scalars + 8, 0, 8, h->stream));
    if (h->n_bytes) {
        const unsigned grid = (unsigned)std::min<uint64_t>((h->n_bytes + 255) / 256, 1u << 16);
        hipLaunchKernelGGL(k_checksum, dim3(grid), dim3(256), 0, h->stream, h->d_bases, h->n_bytes,
                           (unsigned long long *)(h->d_scalars + 8));
    }
    HIPCHK(h, hipMemcpyAsync(out, h->d_scalars + 8, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DBG_OK;
}

extern "C" int dbg_copy_reads(dbg_t *h, char *bases, uint64_t *offsets) {
    if (!h) return DBG_E_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (bases && h->n_bytes) HIPCHK(h, hipMemcpyAsync(bases, h->d_bases, h->n_bytes, hipMemcpyDeviceToHost, h->stream));
    if (offsets && h->d_offsets)
        HIPCHK(h, hipMemcpyAsync(offsets, h->d_offsets, (h->n_reads + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DBG_OK;
}

// ---- the resident reads cut at the bytes that are not bases (kernels: dbg_readsplit.h)
extern "C" int dbg_split_reads(dbg_t *h, uint32_t flags, dbg_split_stats_t *out) {
    if (!h) return DBG_E_ARG;
    if (flags & ~DBG_SPLIT_FOLD_CASE) { h->err = "dbg_split_reads: unknown flag bits"; return DBG_E_ARG; }
    if (!h->d_offsets) { h->err = "no reads set"; return DBG_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    free_build(h);
    dev_free(h->d_org_read); dev_free(h->d_org_pos);
    h->split_done = false;
    h->org_shift = 0;
    const int fold = (flags & DBG_SPLIT_FOLD_CASE) ? 1 : 0;
    const uint64_t n = h->n_bytes, n_reads = h->n_reads;
    const uint64_t n_words = (n + RS_WORD_BYTES - 1) / RS_WORD_BYTES;
    dbg_split_stats_t s{};
    s.n_reads_in = s.n_reads_out = n_reads;
    s.n_bytes_in = s.n_bytes_out = n;
    RsTotals *d_tot = (RsTotals *)(h->d_scalars + 16);
    RsTotals t{};
    HIPCHK(h, hipMemsetAsync(d_tot, 0, sizeof(RsTotals), h->stream));
    if (n_words) {
        const unsigned grid = (unsigned)std::min<uint64_t>((n_words + 255) / 256, 8192);
        hipLaunchKernelGGL(k_rs_count, dim3(grid), dim3(256), 0, h->stream, h->d_bases, n, h->d_startbits, fold, d_tot);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(&t, d_tot, sizeof(RsTotals), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint64_t n_kept = t.kept, n_pieces = t.starts;
    s.n_cut_bytes = n - n_kept;
    s.n_folded_bytes = t.folded;
    if (s.n_cut_bytes == 0 && n_pieces == n_reads && (t.folded == 0 || h->own_bases)) {
        // every read is one piece, whole: the read set stays where it is
        if (t.folded) {
            hipLaunchKernelGGL(k_rs_fold, dim3(grid_for((n + 15) / 16, 256)), dim3(256), 0, h->stream, h->d_bases, n);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipStreamSynchronize(h->stream));
            forget_alphabet(h);
            s.changed = 1;
        }
        h->split_done = true;
        if (out) *out = s;
        return DBG_OK;
    }
    // exact-size outputs next to the old read set
    char *nb = nullptr;
    uint64_t *noff = nullptr, *org_read = nullptr, *org_pos = nullptr;
    auto fail = [&](int rc) { dev_free(nb); dev_free(noff); dev_free(org_read); dev_free(org_pos); return rc; };
    const uint64_t nblk = (n + RS_BLOCK_BYTES - 1) / RS_BLOCK_BYTES;
    int rc = dev_alloc(h, &nb, n_kept + 64);
    if (rc == DBG_OK) rc = dev_alloc(h, &noff, n_pieces + 1);
    if (rc == DBG_OK) rc = dev_alloc(h, &org_read, n_pieces);
    if (rc == DBG_OK) rc = dev_alloc(h, &org_pos, n_pieces);
    if (rc == DBG_OK) rc = buf_ensure(h, h->ar_scan, 2 * nblk * 8);
    if (rc != DBG_OK) return fail(rc);
    s.peak_extra_device_bytes = (n_kept + 64) + (n_pieces + 1) * 8 + std::max<uint64_t>(n_pieces, 1) * 16 + 2 * nblk * 8;
    uint64_t *blk_kept = (uint64_t *)h->ar_scan.p, *blk_starts = blk_kept + nblk;
    hipError_t e = hipMemsetAsync(nb + n_kept, 0, 64, h->stream);
    if (e == hipSuccess && !nblk) e = hipMemsetAsync(noff, 0, 8, h->stream);
    if (e == hipSuccess && nblk) {
        hipLaunchKernelGGL(k_rs_blocks, dim3((unsigned)nblk), dim3(256), 0, h->stream, h->d_bases, n, h->d_startbits, fold,
                           blk_kept, blk_starts);
        hipLaunchKernelGGL(k_rs_carry, dim3(1), dim3(256), 0, h->stream, blk_kept, blk_starts, nblk);
        hipLaunchKernelGGL(k_rs_write, dim3((unsigned)nblk), dim3(256), 0, h->stream, h->d_bases, n, h->d_startbits, fold,
                           h->d_offsets, n_reads, blk_kept, blk_starts, nb, n_kept, noff, org_read, org_pos, n_pieces);
        if (n_pieces)
            hipLaunchKernelGGL(k_rs_read_stats, dim3(grid_for(n_pieces, 256)), dim3(256), 0, h->stream, h->d_offsets, noff,
                               org_read, org_pos, n_pieces, d_tot);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&t, d_tot, sizeof(RsTotals), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("dbg_split_reads: ") + hipGetErrorString(e); return fail(DBG_E_HIP); }
    s.n_reads_out = n_pieces;
    s.n_bytes_out = n_kept;
    s.n_reads_changed = t.nonempty_reads - t.intact;
    s.n_reads_emptied = n_reads - t.with_piece;
    s.changed = 1;
    h->d_org_read = org_read;
    h->d_org_pos = org_pos;
    h->split_done = true;
    if (out) *out = s;
    return install_reads(h, nb, n_kept, noff, n_pieces, true);  // a borrowed buffer is let go unwritten, an owned one is freed
}

extern "C" int dbg_read_origins(dbg_t *h, uint64_t *read_index, uint64_t *pos) {
    if (!h) return DBG_E_ARG;
    if (!h->split_done) { h->err = "dbg_read_origins: dbg_split_reads has not run on the current read set"; return DBG_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->d_org_read) {  // nothing was cut: piece i is read i, and strand j & 1 of it after every dbg_add_revcomp
        for (uint64_t i = 0; i < h->n_reads; ++i) {
            if (read_index) read_index[i] = i >> h->org_shift;
            if (pos) pos[i] = 0;
        }
        return DBG_OK;
    }
    if (read_index && h->n_reads) HIPCHK(h, hipMemcpyAsync(read_index, h->d_org_read, h->n_reads * 8, hipMemcpyDeviceToHost, h->stream));
    if (pos && h->n_reads) HIPCHK(h, hipMemcpyAsync(pos, h->d_org_pos, h->n_reads * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DBG_OK;
}

// ---- both strands of the resident reads: r0, rc(r0), r1, rc(r1), ... (kernels: dbg_revcomp.h)
extern "C" int dbg_add_revcomp(dbg_t *h, uint32_t flags, dbg_revcomp_stats_t *out) {
    if (!h) return DBG_E_ARG;
    if (flags) { h->err = "dbg_add_revcomp: flag bits are reserved"; return DBG_E_ARG; }
    if (!h->d_offsets) { h->err = "no reads set"; return DBG_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    free_build(h);
    const uint64_t n = h->n_bytes, n_reads = h->n_reads, n2 = 2 * n;
    const bool origins = h->split_done && h->d_org_read;
    dbg_revcomp_stats_t s{};
    s.n_reads_in = n_reads;
    s.n_bytes_in = n;
    s.n_reads_out = 2 * n_reads;
    s.n_bytes_out = n2;
    // exact-size outputs next to the old read set, which stays the handle's until everything has run
    char *nb = nullptr;
    uint64_t *noff = nullptr, *org_read = nullptr, *org_pos = nullptr;
    auto fail = [&](int rc) { dev_free(nb); dev_free(noff); dev_free(org_read); dev_free(org_pos); return rc; };
    int rc = dev_alloc(h, &nb, n2 + 64);
    if (rc == DBG_OK) rc = dev_alloc(h, &noff, 2 * n_reads + 1);
    if (rc == DBG_OK && origins) rc = dev_alloc(h, &org_read, 2 * n_reads);
    if (rc == DBG_OK && origins) rc = dev_alloc(h, &org_pos, 2 * n_reads);
    if (rc != DBG_OK) return fail(rc);
    s.peak_extra_device_bytes = (n2 + 64) + 8 * (2 * n_reads + 1) + (origins ? 32 * std::max<uint64_t>(n_reads, 1) : 0);
    RcTotals *d_tot = (RcTotals *)(h->d_scalars + 16);
    RcTotals t{};
    hipError_t e = hipMemsetAsync(d_tot, 0, sizeof(RcTotals), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(nb + n2, 0, 64, h->stream);
    if (e == hipSuccess) {
        Timer tm(h->stream);
        hipLaunchKernelGGL(k_rc_offsets, dim3(grid_for(n_reads + 1, 256)), dim3(256), 0, h->stream, h->d_offsets, n_reads, noff);
        if (n2) {
            const uint64_t n_tiles = (n2 + RC_TILE_BYTES - 1) / RC_TILE_BYTES;
            if (n_tiles > 0x7FFFFFFFull) { h->err = "dbg_add_revcomp: read set too large"; return fail(DBG_E_ARG); }
            // a lent buffer ends at its last base; one the handle owns has 64 bytes more
            hipLaunchKernelGGL(k_rc_tile, dim3((unsigned)n_tiles), dim3(256), 0, h->stream, h->d_bases,
                               n + (h->own_bases ? 64 : 0), h->d_offsets, n_reads, nb, n2, d_tot);
        }
        if (n_reads) {
            const unsigned grid = (unsigned)std::min<uint64_t>((n_reads + 3) / 4, 8192);
            hipLaunchKernelGGL(k_rc_palindromes, dim3(grid), dim3(256), 0, h->stream, h->d_bases, h->d_offsets, n_reads, d_tot);
        }
        if (origins && n_reads)
            hipLaunchKernelGGL(k_rc_origins, dim3(grid_for(n_reads, 256)), dim3(256), 0, h->stream, h->d_org_read, h->d_org_pos,
                               n_reads, org_read, org_pos);
        e = hipGetLastError();
        s.ms_kernel = tm.stop();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&t, d_tot, sizeof(RcTotals), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = std::string("dbg_add_revcomp: ") + hipGetErrorString(e); return fail(DBG_E_HIP); }
    s.n_other_bytes = t.other;
    s.n_palindromes = t.palindromes;
    if (origins) {
        dev_free(h->d_org_read); dev_free(h->d_org_pos);
        h->d_org_read = org_read;
        h->d_org_pos = org_pos;
    } else if (h->split_done) {
        ++h->org_shift;
    }
    if (out) *out = s;
    return install_reads(h, nb, n2, noff, 2 * n_reads, true);  // a borrowed buffer is let go unwritten, an owned one is freed
}

// ---- a selection of the resident reads, gathered on the device (pull_out_read of construct_graph, debruijn.py:274-278:
//      a few per cent of the reads -- the others never leave the GPU)
struct TakeLen {
    const uint64_t *idx, *offsets;
    uint64_t n_reads;
    __device__ uint64_t operator()(uint64_t i) const { const uint64_t r = idx[i]; return r < n_reads ? offsets[r + 1] - offsets[r] : 0; }
};
__global__ __launch_bounds__(256) void k_take_copy(const uint64_t *__restrict__ idx, uint64_t n, const uint64_t *__restrict__ offsets,
                                                   uint64_t n_reads, const char *__restrict__ bases, const uint64_t *__restrict__ out_off,
                                                   char *out) {
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per selected read
    if (i >= n) return;
    const uint64_t r = idx[i];
    if (r >= n_reads) return;
    const uint64_t beg = offsets[r], len = offsets[r + 1] - beg, o = out_off[i];
    for (uint64_t j = threadIdx.x & 63; j < len; j += 64) out[o + j] = bases[beg + j];
}

extern "C" int dbg_take_reads(dbg_t *h, const uint64_t *indices, uint64_t n, uint64_t *out_offsets, char *out_chars,
                              uint64_t capacity, uint64_t *n_chars) {
    if (!h || (n && !indices) || !n_chars) return DBG_E_ARG;
    if (!h->d_offsets) { h->err = "no reads set"; return DBG_E_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    *n_chars = 0;
    if (out_offsets) out_offsets[0] = 0;
    if (!n) return DBG_OK;
    for (uint64_t i = 0; i < n; ++i)
        if (indices[i] >= h->n_reads) { h->err = "read index out of range"; return DBG_E_ARG; }
    uint64_t *d_idx = nullptr, *d_off = nullptr;
    char *d_out = nullptr;
    CHK(dev_alloc(h, &d_idx, n));
    int rc = dev_alloc(h, &d_off, n + 1);
    if (rc != DBG_OK) { dev_free(d_idx); return rc; }
    auto done = [&](int code) { dev_free(d_idx); dev_free(d_off); dev_free(d_out); return code; };
    if (hipMemcpyAsync(d_idx, indices, n * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) { h->err = "dbg_take_reads: copy of the indices failed"; return done(DBG_E_HIP); }
    uint64_t total = 0;
    rc = exclusive_scan(h, n, TakeLen{d_idx, h->d_offsets, h->n_reads}, d_off, &total);
    if (rc != DBG_OK) return done(rc);
    *n_chars = total;
    if (out_offsets) {
        if (hipMemcpyAsync(out_offsets, d_off, n * 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "dbg_take_reads: copy of the offsets failed"; return done(DBG_E_HIP); }
        out_offsets[n] = total;
    }
    if (!out_chars) return done(DBG_OK);  // first call of the two-call pattern: sizes only
    if (capacity < total) { h->err = "dbg_take_reads: capacity below the selected reads' total length"; return done(DBG_E_CAPACITY); }
    if (total) {
        rc = dev_alloc(h, &d_out, total);
        if (rc != DBG_OK) return done(rc);
        hipLaunchKernelGGL(k_take_copy, dim3(grid_for(n, 4)), dim3(256), 0, h->stream, d_idx, n, h->d_offsets, h->n_reads,
                           h->d_bases, d_off, d_out);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out_chars, d_out, total, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "dbg_take_reads: gather failed"; return done(DBG_E_HIP); }
    }
    return done(DBG_OK);
}
