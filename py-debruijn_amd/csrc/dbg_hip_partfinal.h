// Final-mode walk over a graph in parts, host side (kernels and walker: dbg_partfinal.h): dbg_part_final_walk,
// dbg_part_final_export.
// A section of the one translation unit dbg_hip.hip, not self-contained: it needs all of dbg_hip.hip in front of it
// (MultiPass and part_final_free of the multi-pass build, kNoParts, exclusive_scan / reduce_sum, the handle).

// ==========================================================================================
// Final-mode walk over a graph in parts (dbg_partfinal.h): every simple path of the contracted graph the caller built
// from the ranked skeleton and the branch list.  One walker per thread, two passes like walk_impl: count per start,
// scan, write.  The walkers of a wave interleave their stacks and bitmaps (level d of walker w at d * n_walkers + w).
// ==========================================================================================
struct PartFinal {
    uint64_t n_contigs = 0, n_pieces = 0, n_chars = 0;
    bool written = false;  // pass 1 ran: the arrays below hold the index (false: sizes only, the text exceeded max_chars)
    uint32_t *start_ord = nullptr, *seq = nullptr, *piece_row = nullptr;
    uint64_t *length = nullptr, *score = nullptr, *piece_off = nullptr;
};

static void part_final_free(MultiPass *mp) {
    PartFinal *f = mp->fin;
    if (!f) return;
    dev_free(f->start_ord); dev_free(f->seq); dev_free(f->piece_row); dev_free(f->length); dev_free(f->score); dev_free(f->piece_off);
    delete f;
    mp->fin = nullptr;
}

__global__ __launch_bounds__(256) void k_fw_check(FwGraph g, uint64_t n, unsigned long long *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = fw_fault_at(g, i);
    if (f) atomicOr(err, (unsigned long long)f);
}

// Walker w takes the starts w, w + n_walkers, ...; `budget` steps in all.  *status bit 0: a walker ran out of steps.
__global__ __launch_bounds__(64) void k_fw_walk(FwGraph g, int k, int pass, uint64_t n_walkers, FwLevel *lv, uint32_t *bm, uint64_t budget,
                                                uint64_t *per_ctg, uint64_t *per_piece, uint64_t *per_chr, const uint64_t *base_ctg,
                                                const uint64_t *base_piece, FwOut o, unsigned long long *status) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_walkers) return;
    uint64_t steps = budget;
    for (uint64_t i = w; i < g.n_starts; i += n_walkers) {
        FwCount c{0, 0, 0};
        if (!fw_walk_start(g, k, i, lv + w, bm + w, n_walkers, pass, pass ? base_ctg[i] : 0, pass ? base_piece[i] : 0, o, c, steps)) {
            atomicOr(status, 1ull);
            return;
        }
        if (pass == 0) { per_ctg[i] = c.contigs; per_piece[i] = c.pieces; per_chr[i] = c.chars; }
    }
}

static std::string fw_fault_text(uint64_t f) {
    std::string s;
    auto add = [&](uint64_t bit, const char *what) { if (f & bit) s += std::string(s.empty() ? "" : "; ") + what; };
    add(FW_BAD_KIND, "a kind is not one of the five");
    add(FW_BAD_BRANCH, "a row that ends at a branch node names a branch row that is not below n_branch");
    add(FW_BAD_SUCC, "a successor row of the branch table is neither below n_entries nor DBG_NO_NODE");
    add(FW_BAD_START, "a start is not below n_entries");
    return s;
}

extern "C" int dbg_part_final_walk(dbg_t *h, const dbg_final_skeleton_t *s, uint64_t max_chars, uint64_t *n_contigs, uint64_t *n_pieces,
                                   uint64_t *n_chars) {
    if (!h) return DBG_E_ARG;
    if (n_contigs) *n_contigs = 0;
    if (n_pieces) *n_pieces = 0;
    if (n_chars) *n_chars = 0;
    MultiPass *mp = (MultiPass *)h->multipass;
    if (!mp || !h->k) { h->err = kNoParts; return DBG_E_ARG; }
    part_final_free(mp);  // the result of an earlier walk goes, whatever becomes of this one
    if (!s) { h->err = "dbg_part_final_walk: null skeleton"; return DBG_E_ARG; }
    if (!max_chars) max_chars = 1ull << 30;
    PartFinal *res = new PartFinal();
    mp->fin = res;
    if (!s->n_starts || !s->n_entries) { res->written = true; return DBG_OK; }
    if (s->n_entries >= 0xFFFFFFFFull || s->n_branch >= 0xFFFFFFFFull || s->n_starts >= 0xFFFFFFFFull) {
        h->err = "dbg_part_final_walk: more than 2^32 - 2 entries, branch nodes or starts";
        part_final_free(mp);
        return DBG_E_ARG;
    }
    if (!s->d_kind || !s->d_append || !s->d_score || !s->d_branch || !s->d_starts || (s->n_branch && (!s->d_succ_row || !s->d_succ_count))) {
        h->err = "dbg_part_final_walk: null column";
        part_final_free(mp);
        return DBG_E_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const FwGraph g{(const uint8_t *)s->d_kind, (const uint64_t *)s->d_append, (const uint64_t *)s->d_score, (const uint32_t *)s->d_branch,
                    (const uint32_t *)s->d_succ_row, (const uint32_t *)s->d_succ_count, (const uint32_t *)s->d_starts,
                    s->n_entries, s->n_branch, s->n_starts};
    const uint64_t ns = g.n_starts;
    uint64_t *per[3] = {nullptr, nullptr, nullptr}, *base[2] = {nullptr, nullptr};
    unsigned long long *status = nullptr;
    FwLevel *lv = nullptr;
    uint32_t *bm = nullptr;
    auto body = [&]() -> int {
        CHK(dev_alloc(h, &status, 1));
        HIPCHK(h, hipMemsetAsync(status, 0, 8, h->stream));
        // nothing below follows an index before this kernel has passed all of them
        const uint64_t n_check = std::max(std::max(g.n_entries, g.n_branch * FW_FAN), ns);
        hipLaunchKernelGGL(k_fw_check, dim3(grid_for(n_check, 256)), dim3(256), 0, h->stream, g, n_check, status);
        HIPCHK(h, hipGetLastError());
        uint64_t f = 0;
        HIPCHK(h, hipMemcpyAsync(&f, status, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (f) { h->err = "dbg_part_final_walk: " + fw_fault_text(f) + " (no walk ran)"; return DBG_E_ARG; }
        for (auto &p : per) { CHK(dev_alloc(h, &p, ns)); HIPCHK(h, hipMemsetAsync(p, 0, ns * 8, h->stream)); }
        for (auto &p : base) CHK(dev_alloc(h, &p, ns));
        // walkers: the rule of walk_impl -- 4 GiB of stacks, 2^16 walkers at most
        const uint64_t levels = g.n_branch + 1, bm_words = (g.n_branch + 31) / 32;
        const uint64_t per_walker = levels * sizeof(FwLevel) + bm_words * 4;
        uint64_t n_walkers = std::min<uint64_t>(ns, std::max<uint64_t>(1, (4ull << 30) / per_walker));
        n_walkers = std::min<uint64_t>(n_walkers, 1u << 16);
        CHK(dev_alloc(h, &lv, n_walkers * levels));
        CHK(dev_alloc(h, &bm, n_walkers * bm_words));
        HIPCHK(h, hipMemsetAsync(bm, 0, std::max<uint64_t>(n_walkers * bm_words, 1) * 4, h->stream));
        FwOut o{};
        auto launch = [&](int pass) {
            hipLaunchKernelGGL(k_fw_walk, dim3(grid_for(n_walkers, 64)), dim3(64), 0, h->stream, g, h->k, pass, n_walkers, lv, bm,
                               h->part_final_steps, per[0], per[1], per[2], base[0], base[1], o, status);
        };
        launch(0);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(&f, status, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (f) {
            h->err = "dbg_part_final_walk: a walker took more than " + std::to_string(h->part_final_steps) +
                     " steps (option \"part_final_walk_steps\" raises the budget)";
            return DBG_E_CAPACITY;
        }
        uint64_t n_ctg = 0, n_pc = 0, n_chr = 0;
        CHK(exclusive_scan(h, ns, U64At{per[0]}, base[0], &n_ctg));
        CHK(exclusive_scan(h, ns, U64At{per[1]}, base[1], &n_pc));
        CHK(reduce_sum(h, ns, U64At{per[2]}, &n_chr));
        res->n_contigs = n_ctg; res->n_pieces = n_pc; res->n_chars = n_chr;
        if (n_contigs) *n_contigs = n_ctg;
        if (n_pieces) *n_pieces = n_pc;
        if (n_chars) *n_chars = n_chr;
        if (n_ctg >= 0xFFFFFFFFull) { h->err = "dbg_part_final_walk: more than 2^32 - 2 contigs"; return DBG_E_CAPACITY; }
        if (n_chr > max_chars) {
            h->err = "dbg_part_final_walk: contig text exceeds max_chars (sizes are valid, nothing was written)";
            return DBG_E_CAPACITY;
        }
        CHK(dev_alloc(h, &res->start_ord, n_ctg)); CHK(dev_alloc(h, &res->seq, n_ctg)); CHK(dev_alloc(h, &res->length, n_ctg));
        CHK(dev_alloc(h, &res->score, n_ctg)); CHK(dev_alloc(h, &res->piece_off, n_ctg + 1)); CHK(dev_alloc(h, &res->piece_row, n_pc));
        HIPCHK(h, hipMemcpyAsync(res->piece_off + n_ctg, &res->n_pieces, 8, hipMemcpyHostToDevice, h->stream));
        o = FwOut{res->start_ord, res->seq, res->length, res->score, res->piece_off, res->piece_row, n_ctg, n_pc};
        launch(1);  // the same walk: the bitmaps are clean again and the budget holds as it did
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));
        res->written = true;
        return DBG_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(h->stream);
    for (auto &p : per) dev_free(p);
    for (auto &p : base) dev_free(p);
    dev_free(status); dev_free(lv); dev_free(bm);
    // a text above max_chars keeps its sizes (dbg_part_final_export then refuses); every other failure keeps nothing
    if (rc != DBG_OK && !(rc == DBG_E_CAPACITY && res->n_chars > max_chars)) part_final_free(mp);
    return rc;
}

extern "C" int dbg_part_final_export(dbg_t *h, uint32_t *start_ordinal, uint32_t *seq, uint64_t *length, uint64_t *score,
                                     uint64_t *piece_off, uint32_t *piece_row) {
    if (!h) return DBG_E_ARG;
    MultiPass *mp = (MultiPass *)h->multipass;
    if (!mp || !h->k) { h->err = kNoParts; return DBG_E_ARG; }
    const PartFinal *f = mp->fin;
    if (!f) { h->err = "dbg_part_final_export: dbg_part_final_walk must run first on this graph"; return DBG_E_ARG; }
    if (!f->written) { h->err = "dbg_part_final_export: the last final walk kept its sizes only (text larger than max_chars)"; return DBG_E_ARG; }
    const uint64_t n = f->n_contigs;
    if (piece_off && !n) piece_off[0] = 0;
    if (!n) return DBG_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (start_ordinal) HIPCHK(h, hipMemcpyAsync(start_ordinal, f->start_ord, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (seq) HIPCHK(h, hipMemcpyAsync(seq, f->seq, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (length) HIPCHK(h, hipMemcpyAsync(length, f->length, n * 8, hipMemcpyDeviceToHost, h->stream));
    if (score) HIPCHK(h, hipMemcpyAsync(score, f->score, n * 8, hipMemcpyDeviceToHost, h->stream));
    if (piece_off) HIPCHK(h, hipMemcpyAsync(piece_off, f->piece_off, (n + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    if (piece_row && f->n_pieces) HIPCHK(h, hipMemcpyAsync(piece_row, f->piece_row, f->n_pieces * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DBG_OK;
}
