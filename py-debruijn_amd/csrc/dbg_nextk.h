// The driver's step to the next k (II_assembleFromReads.py:56-75) without spelling the contigs: dbg_build_from_walks builds
// the K-graph of (blocks of contigs of earlier non-final walks, in driver order) + (extra reads) straight from the chain
// structure of the graphs those walks ran on; dbg_build_from_walk is its one-block call with K = k + 1.  Included by
// dbg_hip.hip after every helper it uses ("Next k from the walk").
//
// A non-final contig is a chain x0 -> x1 -> ... -> x(n-1) of k-nodes under one per-node continuation nxt() (k_jump_init's
// rule): k + n - 1 characters.  With d = K - k, for the K-graph of the selected contigs of one block:
//   - nodes: z(x) = key(x) followed by the last bases of nxt^1(x) .. nxt^d(x), for every x that has nxt^d(x) and lies on a
//     selected contig of n >= d + 2 nodes (a read makes nodes only if it is longer than K);
//   - count of the edge z(x) -> z(nxt x), where nxt^(d+1)(x) exists: S(x) = number of such contigs through x (a sum over
//     the starts upstream);
//   - first occurrence: the lowest-ranked such contig through x, at hop distance h from its start: (off + h) << 1 | h != 0.
// Both reductions run by doubling over the jump pointers J_j(u) = nxt^(2^j)(u) (NONE past the chain end, never wrapped):
// B_(j+1)(v) = B_j(v) (+) sum over u with J_j(u) = v of B_j(u), one scatter per round.  Upstream sets of distinct u are
// disjoint in a forest, so every start counts once; cycles carry no weight (they emit no contig).  d only enters the start
// weights (hops >= d + 1) and the walk of d pointers that spells z(x).
// The blocks are reduced one after another (the chain scratch of a block is freed before the next one starts) and then
// merged, in block order, into one table keyed by the two words of the K-mer.
#pragma once

constexpr uint32_t NK_NONE = 0xFFFFFFFFu;

// chain successor of every node, NONE where a chain ends (branch node, no kept successor, next node pulled) and on
// pulled nodes
__global__ __launch_bounds__(256) void k_nk_next(uint64_t n, GDna g, uint32_t *nxt) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    uint32_t t = NK_NONE;
    const uint8_t f = g.flags[v];
    if (!(f & (DBG_F_PULLED | DBG_F_BRANCH)) && g.keep_count((uint32_t)v)) {
        const uint32_t s = g.succ_of((uint32_t)v, g.first_kept((uint32_t)v));
        if (!(g.flags[s] & DBG_F_PULLED)) t = s;
    }
    nxt[v] = t;
}

// pull-style pointer jumping: H = hops to the chain end; *open counts the nodes whose jump is still set
__global__ __launch_bounds__(256) void k_nk_rank_step(uint64_t n, const uint32_t *__restrict__ J, const uint32_t *__restrict__ H,
                                                      uint32_t *J2, uint32_t *H2, unsigned long long *open) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t o = 0;
    if (v < n) {
        uint32_t j = J[v], h = H[v];
        if (j != NK_NONE) { h += H[j]; j = J[j]; }
        J2[v] = j;
        H2[v] = h;
        o = j != NK_NONE;
    }
    o = wave_sum_u64(o);
    if ((threadIdx.x & 63) == 0 && o) atomicAdd(open, (unsigned long long)o);
}

__global__ __launch_bounds__(256) void k_nk_hops_init(uint64_t n, const uint32_t *__restrict__ nxt, uint32_t *J, uint32_t *H) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    J[v] = nxt[v];
    H[v] = nxt[v] != NK_NONE;
}

// the starts that emit a contig (k_walk_chain / k_jump_starts: indegree 0, not pulled, chain ends)
__global__ __launch_bounds__(256) void k_nk_emits(uint64_t n, const uint8_t *__restrict__ flags, const uint32_t *__restrict__ J,
                                                  uint8_t *emit) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    emit[v] = !(flags[v] & (DBG_F_INDEG | DBG_F_PULLED)) && J[v] == NK_NONE;
}
struct NkChars {
    const uint8_t *emit;
    const uint32_t *H;
    int k;
    __device__ uint64_t operator()(uint64_t i) const { return emit[i] ? (uint64_t)k + H[i] : 0; }
};

// weights of the starts: contig index c (ascending start id == the walk's index), rank r = rank_of[c] inside the block
// (NONE: the block does not hold the contig)
__global__ __launch_bounds__(256) void k_nk_weights(uint64_t n, int d, const uint8_t *__restrict__ emit, const uint32_t *__restrict__ cidx,
                                                    const uint32_t *__restrict__ H, const uint32_t *__restrict__ rank_of,
                                                    uint32_t *S, unsigned long long *M, uint32_t *start_of_rank) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    uint32_t s = 0;
    unsigned long long m = ~0ull;
    if (emit[v]) {
        const uint32_t r = rank_of[cidx[v]];
        if (r != NK_NONE) {
            start_of_rank[r] = (uint32_t)v;
            if (H[v] >= (uint32_t)d + 1) { s = 1; m = (unsigned long long)r << 32; }  // n >= d + 2 nodes: the contig makes K-nodes
        }
    }
    S[v] = s;
    M[v] = m;
}

// one doubling round of the sum S and of the min M = (rank << 32 | hops from that start); S2 / M2 hold copies of S / M
__global__ __launch_bounds__(256) void k_nk_push(uint64_t n, int j, const uint32_t *__restrict__ J, const uint32_t *__restrict__ S,
                                                 const unsigned long long *__restrict__ M, uint32_t *J2, uint32_t *S2,
                                                 unsigned long long *M2, unsigned long long *open) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t o = 0;
    if (v < n) {
        const uint32_t t = J[v];
        uint32_t t2 = NK_NONE;
        if (t != NK_NONE) {
            const uint32_t s = S[v];
            if (s) {
                atomicAdd(&S2[t], s);
                atomicMin(&M2[t], M[v] + (1ull << j));
                o = 1;
            }
            t2 = J[t];
        }
        J2[v] = t2;
    }
    o = wave_sum_u64(o);
    if ((threadIdx.x & 63) == 0 && o) atomicAdd(open, (unsigned long long)o);
}

// z(x): key(x) shifted by 2d bits across the two key words, the last bases of nxt^1(x) .. nxt^d(x) behind it; t = nxt^d(x).
// false where the chain ends before nxt^d(x).  On a cycle the walk just goes round (d <= 62 steps).
__device__ inline bool nk_zkey(const GDna &g, const uint32_t *__restrict__ nxt, uint32_t x, int d, uint64_t &lo, uint64_t &hi,
                               uint32_t &t) {
    lo = g.keys[x];
    hi = g.keys_hi ? g.keys_hi[x] : 0ull;
    t = x;
    for (int i = 0; i < d; ++i) {
        t = nxt[t];
        if (t == NK_NONE) return false;
        hi = (hi << 2) | (lo >> 62);
        lo = (lo << 2) | g.last_code(t);
    }
    return true;
}

// S(x) != 0 puts x on a chain that ends, where H is the exact hop count to the end: x has nxt^d(x) iff H(x) >= d
struct NkZFlag {
    const uint32_t *S, *H;
    uint32_t d;
    __device__ uint64_t operator()(uint64_t i) const { return S[i] && H[i] >= d; }
};

// the K-nodes of the block's contigs: key, stamp, the one successor code (0xFF: none) and its count
__global__ __launch_bounds__(256) void k_nk_emit(uint64_t n, int d, GDna g, const uint32_t *__restrict__ nxt, const uint32_t *__restrict__ S,
                                                 const uint32_t *__restrict__ H, const unsigned long long *__restrict__ M,
                                                 const uint32_t *__restrict__ zidx, const uint64_t *__restrict__ drv_off,
                                                 uint64_t *ck_lo, uint64_t *ck_hi, uint64_t *cstamp, uint8_t *ccode, uint32_t *ccnt) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n || !S[x] || H[x] < (uint32_t)d) return;
    uint64_t lo, hi;
    uint32_t t;
    if (!nk_zkey(g, nxt, (uint32_t)x, d, lo, hi, t)) return;  // not taken: H(x) >= d
    const uint32_t j = zidx[x], nt = nxt[t];
    ck_lo[j] = lo;
    ck_hi[j] = hi;
    const uint64_t m = M[x], h = m & 0xFFFFFFFFull;
    cstamp[j] = ((drv_off[m >> 32] + h) << 1) | (h != 0);
    ccode[j] = nt != NK_NONE ? (uint8_t)g.last_code(nt) : (uint8_t)0xFF;
    ccnt[j] = nt != NK_NONE ? S[x] : 0u;
}

// ---- node table of the union: open addressing, (lo, hi) -> node id; inserts and lookups are separate launches
struct NkTab {
    uint32_t *id;
    uint64_t *lo, *hi;
    uint64_t mask;
    __device__ uint64_t home(uint64_t l, uint64_t h) const { return k128_hash(K128{h, l}) & mask; }
    __device__ void insert(uint64_t l, uint64_t h, uint32_t v) const {
        uint64_t s = home(l, h);
        for (uint64_t p = 0; p <= mask; ++p) {
            if (atomicCAS(&id[s], NK_NONE, v) == NK_NONE) { lo[s] = l; hi[s] = h; return; }
            s = (s + 1) & mask;
        }
    }
    __device__ uint32_t find(uint64_t l, uint64_t h) const {
        uint64_t s = home(l, h);
        for (uint64_t p = 0; p <= mask; ++p) {
            const uint32_t e = id[s];
            if (e == NK_NONE) return NK_NONE;
            if (lo[s] == l && hi[s] == h) return e;
            s = (s + 1) & mask;
        }
        return NK_NONE;
    }
};

__global__ __launch_bounds__(256) void k_nk_insert(uint64_t n, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                   NkTab tab) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tab.insert(lo[i], hi ? hi[i] : 0ull, (uint32_t)i);
}

// contig node j of a block: the node of the union so far (extra reads, earlier blocks) with its key, or NONE (then it is new)
__global__ __launch_bounds__(256) void k_nk_match(uint64_t n_c, const uint64_t *__restrict__ ck_lo, const uint64_t *__restrict__ ck_hi,
                                                  NkTab tab, uint32_t *cid, uint8_t *isnew) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_c) return;
    const uint32_t e = tab.find(ck_lo[j], ck_hi[j]);
    cid[j] = e;
    isnew[j] = e == NK_NONE;
}

// the new nodes of a block take the ids from new_from on and enter the table (a block holds every key once)
__global__ __launch_bounds__(256) void k_nk_insert_new(uint64_t n_c, uint64_t new_from, const uint8_t *__restrict__ isnew,
                                                       const uint32_t *__restrict__ newidx, const uint64_t *__restrict__ ck_lo,
                                                       const uint64_t *__restrict__ ck_hi, NkTab tab, uint32_t *cid) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_c || !isnew[j]) return;
    const uint32_t id = (uint32_t)(new_from + newidx[j]);
    cid[j] = id;
    tab.insert(ck_lo[j], ck_hi[j], id);
}

// the extra-read graph, stamps moved behind the contig text (+2T); fs = its first-seen successor order
__global__ __launch_bounds__(256) void k_nk_fill_extra(uint64_t n_e, const uint64_t *__restrict__ e_lo, const uint64_t *__restrict__ e_hi,
                                                       const uint64_t *__restrict__ e_st, const uint32_t *__restrict__ e_cnt,
                                                       const uint8_t *__restrict__ e_fs, uint64_t stamp_add, uint64_t *lo,
                                                       uint64_t *hi, uint64_t *st, uint32_t *cnt, uint8_t *fs, uint16_t *bo) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_e) return;
    lo[i] = e_lo[i];
    if (hi) hi[i] = e_hi ? e_hi[i] : 0ull;
    st[i] = e_st[i] + stamp_add;
    reinterpret_cast<uint4 *>(cnt)[i] = reinterpret_cast<const uint4 *>(e_cnt)[i];
    fs[i] = e_fs[i];
    bo[i] = 0;
}

// the nodes of one block, blocks in read order: appended (ids from new_from on are this block's) or merged into the node
// that holds the key already -- counts add, the earliest stamp wins (block bases rise, the extra reads lie behind all
// blocks).  bo: the successor codes in the order of the first block whose chains hold that edge (2 bits each, their
// number in bits 8..10); a block gives a node at most one code.
__global__ __launch_bounds__(256) void k_nk_fill_contig(uint64_t n_c, uint64_t new_from, const uint64_t *__restrict__ ck_lo,
                                                        const uint64_t *__restrict__ ck_hi, const uint64_t *__restrict__ cstamp,
                                                        const uint8_t *__restrict__ ccode, const uint32_t *__restrict__ ccnt,
                                                        const uint32_t *__restrict__ cid, uint64_t *lo, uint64_t *hi, uint64_t *st,
                                                        uint32_t *cnt, uint8_t *fs, uint16_t *bo) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_c) return;
    const uint32_t id = cid[j];
    const uint8_t c = ccode[j];
    uint32_t b = 0;
    if (id >= new_from) {
        lo[id] = ck_lo[j];
        if (hi) hi[id] = ck_hi[j];
        reinterpret_cast<uint4 *>(cnt)[id] = make_uint4(0, 0, 0, 0);
        fs[id] = 0;
        st[id] = cstamp[j];
    } else {
        b = bo[id];
        const uint64_t mine = cstamp[j];
        if (mine < st[id]) st[id] = mine;
    }
    if (c != 0xFF) {
        cnt[(uint64_t)id * 4 + c] += ccnt[j];
        const uint32_t held = b >> 8;
        bool seen = false;
        for (uint32_t r = 0; r < held; ++r) seen |= ((b >> (2 * r)) & 3u) == c;
        if (!seen) b = ((b & 0xFFu) | ((uint32_t)c << (2 * held))) | ((held + 1) << 8);
    }
    bo[id] = (uint16_t)b;
}

// successors by key, degrees, indegree flags and the two rank bytes.  First-seen key of a code: the block successors in
// block order (bo; their first occurrences are below T), then the extra graph's first-seen order; codes without count
// last, in ASCII order (A C G T = codes 0 1 3 2) as every build ranks them.  most_common = (count desc, first seen asc).
__global__ __launch_bounds__(256) void k_nk_succ(uint64_t n, int k1, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                 const uint64_t *__restrict__ st, const uint32_t *__restrict__ cnt,
                                                 const uint8_t *__restrict__ fs, const uint16_t *__restrict__ bo, NkTab tab,
                                                 uint32_t *succ, uint8_t *deg, uint8_t *flags, uint8_t *order, uint8_t *fsorder) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 c4 = reinterpret_cast<const uint4 *>(cnt)[i];
    const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
    const uint64_t l = lo[i], h = hi ? hi[i] : 0ull;
    const uint64_t lo_mask = k1 >= 32 ? ~0ull : ((1ull << (2 * k1)) - 1);
    const uint64_t hi_mask = k1 > 32 ? ((1ull << (2 * k1 - 64)) - 1) : 0ull;
    const uint8_t f = fs[i];
    const uint32_t z = bo[i], held = z >> 8;
    uint32_t s[4], key[4], code[4] = {0, 1, 2, 3};
    const uint32_t ascii_rank[4] = {0, 1, 3, 2};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        s[b] = NK_NONE;
        if (c[b]) {
            s[b] = tab.find(((l << 2) | (uint64_t)b) & lo_mask, ((h << 2) | (l >> 62)) & hi_mask);
            uint32_t pos = 0, blk = 4;
            for (int r = 0; r < 4; ++r)
                if (((f >> (2 * r)) & 3u) == (uint32_t)b) { pos = r; break; }
            for (uint32_t r = 0; r < held; ++r)
                if (((z >> (2 * r)) & 3u) == (uint32_t)b) { blk = r; break; }
            key[b] = blk < 4 ? blk : 4u + pos;
        } else {
            key[b] = 16u + ascii_rank[b];
        }
    }
    reinterpret_cast<uint4 *>(succ)[i] = make_uint4(s[0], s[1], s[2], s[3]);
    deg[i] = (uint8_t)((c[0] != 0) + (c[1] != 0) + (c[2] != 0) + (c[3] != 0));
    flags[i] = (uint8_t)(st[i] & 1);
    // insertion sorts of four codes
    uint32_t a[4] = {0, 1, 2, 3};
#pragma unroll
    for (int x = 1; x < 4; ++x)
#pragma unroll
        for (int y = x; y > 0; --y)
            if (key[a[y]] < key[a[y - 1]]) { const uint32_t t = a[y]; a[y] = a[y - 1]; a[y - 1] = t; }
    fsorder[i] = (uint8_t)(a[0] | (a[1] << 2) | (a[2] << 4) | (a[3] << 6));
#pragma unroll
    for (int x = 0; x < 4; ++x) code[x] = a[x];
#pragma unroll
    for (int x = 1; x < 4; ++x)
#pragma unroll
        for (int y = x; y > 0; --y)
            if (c[code[y]] > c[code[y - 1]]) { const uint32_t t = code[y]; code[y] = code[y - 1]; code[y - 1] = t; }
    order[i] = (uint8_t)(code[0] | (code[1] << 2) | (code[2] << 4) | (code[3] << 6));
}

// z(x) for every node x of a source that has nxt^d(x): the K-node id in the union, or NONE
__global__ __launch_bounds__(256) void k_nk_zmap(uint64_t n, int d, GDna g, const uint32_t *__restrict__ nxt, NkTab tab, uint32_t *z) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    uint64_t lo, hi;
    uint32_t t;
    z[x] = nk_zkey(g, nxt, (uint32_t)x, d, lo, hi, t) ? tab.find(lo, hi) : NK_NONE;
}

// ---- pull-out reads of the contigs: OR over a chain of "x has nxt^d(x) and z(x) is a branch K-node".  z(x) is looked up
// in the union, so a contig of exactly K characters (no node of its own) can still hold a branch node.
__global__ __launch_bounds__(256) void k_nk_or_init(uint64_t n, const uint32_t *__restrict__ y, const uint8_t *__restrict__ flags,
                                                    const uint32_t *__restrict__ nxt, uint32_t *J, uint8_t *P) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const uint32_t t = y[x];
    P[x] = t != NK_NONE && (flags[t] & DBG_F_BRANCH);
    J[x] = nxt[x];
}
__global__ __launch_bounds__(256) void k_nk_or_step(uint64_t n, const uint32_t *__restrict__ J, const uint8_t *__restrict__ P,
                                                    uint32_t *J2, uint8_t *P2, unsigned long long *open) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t o = 0;
    if (v < n) {
        uint32_t j = J[v];
        uint8_t p = P[v];
        if (j != NK_NONE) { p |= P[j]; j = J[j]; }
        J2[v] = j;
        P2[v] = p;
        o = j != NK_NONE;
    }
    o = wave_sum_u64(o);
    if ((threadIdx.x & 63) == 0 && o) atomicAdd(open, (unsigned long long)o);
}
__global__ __launch_bounds__(256) void k_nk_or_gather(uint64_t n_r, const uint32_t *__restrict__ start, const uint8_t *__restrict__ P,
                                                      uint8_t *out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_r) out[r] = P[start[r]];
}

// pointer jumping until the count of open jumps stops falling: then every node whose chain ends has J == NONE (a chain
// still open at level j holds a node exactly 2^j hops before its end, which closes in that round); cycles stay open
// (until_zero: until no jump is open at all -- the doubling sums, whose open jumps all lie on chains that end)
template <class Step>
static int nk_jump_until_closed(dbg *h, uint64_t n, Step step, bool until_zero = false) {
    unsigned long long *open = (unsigned long long *)(h->d_scalars + 40);
    uint64_t prev = ~0ull;
    for (int round = 0; round < 64; ++round) {
        HIPCHK(h, hipMemsetAsync(open, 0, 8, h->stream));
        step(round, open);
        HIPCHK(h, hipGetLastError());
        uint64_t now = 0;
        HIPCHK(h, hipMemcpyAsync(&now, open, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (now == 0 || (!until_zero && now == prev)) return round + 1;
        prev = now;
    }
    h->err = "internal: pointer jumping did not converge";
    return -1;
}

// called by dbg_mark_pull_reads on a graph from dbg_build_from_walk(s): flags of the virtual contig reads, block by block
static int nk_mark_contigs(dbg *h) {
    dev_free(h->d_nk_read_flags);
    CHK(dev_alloc(h, &h->d_nk_read_flags, h->nk_reads));
    HIPCHK(h, hipMemsetAsync(h->d_nk_read_flags, 0, h->nk_reads ? h->nk_reads : 1, h->stream));
    if (!h->nk_reads || !h->n_branch) return DBG_OK;
    uint64_t first_read = 0;
    for (const dbg::NkBlock &b : h->nk_blocks) {
        const uint64_t n = b.n_src;
        if (!b.n_reads || !n) { first_read += b.n_reads; continue; }
        uint32_t *J[2] = {nullptr, nullptr};
        uint8_t *P[2] = {nullptr, nullptr};
        int rc = DBG_OK;
        do {
            if ((rc = dev_alloc(h, &J[0], n)) != DBG_OK || (rc = dev_alloc(h, &J[1], n)) != DBG_OK ||
                (rc = dev_alloc(h, &P[0], n)) != DBG_OK || (rc = dev_alloc(h, &P[1], n)) != DBG_OK) break;
            const dim3 grid(grid_for(n, 256));
            hipLaunchKernelGGL(k_nk_or_init, grid, dim3(256), 0, h->stream, n, b.z, h->d_flags, b.next, J[0], P[0]);
            int cur = 0;
            const int rounds = nk_jump_until_closed(h, n, [&](int, unsigned long long *open) {
                hipLaunchKernelGGL(k_nk_or_step, grid, dim3(256), 0, h->stream, n, J[cur], P[cur], J[cur ^ 1], P[cur ^ 1], open);
                cur ^= 1;
            });
            if (rounds < 0) { rc = DBG_E_HIP; break; }
            hipLaunchKernelGGL(k_nk_or_gather, dim3(grid_for(b.n_reads, 256)), dim3(256), 0, h->stream, b.n_reads, b.start, P[cur],
                               h->d_nk_read_flags + first_read);
            if (hipGetLastError() != hipSuccess) { h->err = "pull-out contigs: launch failed"; rc = DBG_E_HIP; break; }
            hipError_t e = hipStreamSynchronize(h->stream);  // the scratch goes back before the next block
            if (e != hipSuccess) { h->err = std::string("pull-out contigs: ") + hipGetErrorString(e); rc = DBG_E_HIP; }
        } while (0);
        dev_free(J[0]); dev_free(J[1]); dev_free(P[0]); dev_free(P[1]);
        if (rc != DBG_OK) return rc;
        first_read += b.n_reads;
    }
    uint64_t total = 0;
    CHK(reduce_sum(h, h->nk_reads, ByteAt{h->d_nk_read_flags}, &total));
    h->n_pull_reads += total;
    return DBG_OK;
}

// why src cannot be a source of a K-graph on dst, or nullptr.  several: the checks of dbg_build_from_walks (a graph in
// parts is named as such even before it has a walk, and the node limit belongs to the list); otherwise the checks of
// dbg_build_from_walk in the order it has always made them (it tests the node limit behind its own arguments)
static const char *nk_refuse_source(const dbg *dst, const dbg *src, bool several) {
    const char *parts = "src holds a graph in parts: build from a single-table graph";
    if (dst == src) return "dst and src must be different handles";
    if (dst->device != src->device) return "dst and src must be on the same device";
    if (several && (src->multipass || src->partial_graph)) return parts;
    if (!src->k || !src->walk_indexed) return "src has no walk of its current graph";
    if (src->multipass || src->partial_graph) return parts;
    if (src->D != 4 || !src->is_dna) return "src is not an ACGT graph (generic alphabets take the text path)";
    if (src->walk_final) return "the last walk of src was a final-mode walk (all simple paths, not chains)";
    if (several && src->n_nodes >= 0xFFFFFFF0ull) return "src has too many nodes";
    return nullptr;
}

// a HIP call inside a do { } while (0) body that owns device memory: on an error set rc and leave through the frees
#define NK_HIP(h, call)                                                        \
    if (hipError_t e_ = (call); e_ != hipSuccess) {                            \
        (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);          \
        rc = e_ == hipErrorOutOfMemory ? DBG_E_NOMEM : DBG_E_HIP;              \
        break;                                                                 \
    } else (void)0

// the K-nodes of one block, kept until the union
struct NkNodes {
    uint64_t n_c = 0;
    uint64_t *lo = nullptr, *hi = nullptr, *stamp = nullptr;
    uint8_t *code = nullptr;
    uint32_t *cnt = nullptr, *cid = nullptr;
    void release() { dev_free(lo); dev_free(hi); dev_free(stamp); dev_free(code); dev_free(cnt); dev_free(cid); }
};

// The chain phase of one block: continuation pointers of src, the two doubling reductions with the block's start weights,
// and the block's K-nodes.  rank_of[c]: position of contig c inside the block or NONE; drv_off[r]: offset of the block's
// r-th contig in the virtual text (block base included).  Everything but `out` and `kept` is freed on return.
static int nk_chain_block(dbg *dst, dbg *src, int d, const std::vector<uint32_t> &rank_of, const std::vector<uint64_t> &drv_off,
                          NkNodes &out, dbg::NkBlock &kept) {
    const uint64_t n = src->n_nodes, n_sel = drv_off.size() - 1;
    kept.n_src = n;
    kept.n_reads = n_sel;
    if (!n_sel || !n) { kept.n_src = 0; return DBG_OK; }
    const GDna g = dna_view(src);
    const dim3 grid(grid_for(n, 256));
    uint32_t *nxt = nullptr, *J[2] = {nullptr, nullptr}, *H[2] = {nullptr, nullptr}, *cidx = nullptr, *d_rank = nullptr,
             *S[2] = {nullptr, nullptr}, *zidx = nullptr, *start_of_rank = nullptr;
    unsigned long long *M[2] = {nullptr, nullptr};
    uint64_t *d_drv = nullptr;
    uint8_t *emit = nullptr;
    int rc = DBG_OK;
    do {
        // 1. continuation pointers and hops to the chain end
        if ((rc = dev_alloc(dst, &nxt, n)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &J[0], n)) != DBG_OK || (rc = dev_alloc(dst, &J[1], n)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &H[0], n)) != DBG_OK || (rc = dev_alloc(dst, &H[1], n)) != DBG_OK) break;
        hipLaunchKernelGGL(k_nk_next, grid, dim3(256), 0, dst->stream, n, g, nxt);
        hipLaunchKernelGGL(k_nk_hops_init, grid, dim3(256), 0, dst->stream, n, nxt, J[0], H[0]);
        int cur = 0;
        if (nk_jump_until_closed(dst, n, [&](int, unsigned long long *open) {
                hipLaunchKernelGGL(k_nk_rank_step, grid, dim3(256), 0, dst->stream, n, J[cur], H[cur], J[cur ^ 1], H[cur ^ 1], open);
                cur ^= 1;
            }) < 0) { rc = DBG_E_HIP; break; }
        uint32_t *Jend = J[cur], *Hops = H[cur];
        // 2. emitting starts == the walk's contig index (checked against it)
        if ((rc = dev_alloc(dst, &emit, n)) != DBG_OK || (rc = dev_alloc(dst, &cidx, n)) != DBG_OK) break;
        hipLaunchKernelGGL(k_nk_emits, grid, dim3(256), 0, dst->stream, n, g.flags, Jend, emit);
        uint64_t n_ctg = 0, n_chr = 0;
        if ((rc = exclusive_scan(dst, n, ByteAt{emit}, cidx, &n_ctg)) != DBG_OK) break;
        if ((rc = reduce_sum(dst, n, NkChars{emit, Hops, src->k}, &n_chr)) != DBG_OK) break;
        if (n_ctg != src->n_contigs || n_chr != src->contig_chars) {
            dst->err = "internal: chains disagree with the walk's contig index";
            rc = DBG_E_HIP;
            break;
        }
        // 3. start weights, then doubling of (sum, min) over the jump pointers
        if ((rc = dev_alloc(dst, &d_rank, rank_of.size())) != DBG_OK || (rc = dev_alloc(dst, &start_of_rank, n_sel)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &d_drv, n_sel + 1)) != DBG_OK) break;
        NK_HIP(dst, hipMemcpyAsync(d_rank, rank_of.data(), rank_of.size() * 4, hipMemcpyHostToDevice, dst->stream));
        NK_HIP(dst, hipMemcpyAsync(d_drv, drv_off.data(), (n_sel + 1) * 8, hipMemcpyHostToDevice, dst->stream));
        if ((rc = dev_alloc(dst, &S[0], n)) != DBG_OK || (rc = dev_alloc(dst, &S[1], n)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &M[0], n)) != DBG_OK || (rc = dev_alloc(dst, &M[1], n)) != DBG_OK) break;
        dev_free(H[cur ^ 1]);
        hipLaunchKernelGGL(k_nk_weights, grid, dim3(256), 0, dst->stream, n, d, emit, cidx, Hops, d_rank, S[0], M[0], start_of_rank);
        NK_HIP(dst, hipMemcpyAsync(J[0], nxt, n * 4, hipMemcpyDeviceToDevice, dst->stream));
        cur = 0;
        if (nk_jump_until_closed(dst, n, [&](int round, unsigned long long *open) {
                (void)hipMemcpyAsync(S[cur ^ 1], S[cur], n * 4, hipMemcpyDeviceToDevice, dst->stream);
                (void)hipMemcpyAsync(M[cur ^ 1], M[cur], n * 8, hipMemcpyDeviceToDevice, dst->stream);
                hipLaunchKernelGGL(k_nk_push, grid, dim3(256), 0, dst->stream, n, round, J[cur], S[cur], M[cur], J[cur ^ 1], S[cur ^ 1],
                                   M[cur ^ 1], open);
                cur ^= 1;
            }, true) < 0) { rc = DBG_E_HIP; break; }
        const uint32_t *Sum = S[cur];
        const unsigned long long *Min = M[cur];
        // 4. the K-nodes of the block's contigs
        if ((rc = dev_alloc(dst, &zidx, n)) != DBG_OK) break;
        if ((rc = exclusive_scan(dst, n, NkZFlag{Sum, Hops, (uint32_t)d}, zidx, &out.n_c)) != DBG_OK) break;
        const uint64_t n_c = out.n_c;
        if ((rc = dev_alloc(dst, &out.lo, n_c)) != DBG_OK || (rc = dev_alloc(dst, &out.hi, n_c)) != DBG_OK ||
            (rc = dev_alloc(dst, &out.stamp, n_c)) != DBG_OK || (rc = dev_alloc(dst, &out.code, n_c)) != DBG_OK ||
            (rc = dev_alloc(dst, &out.cnt, n_c)) != DBG_OK || (rc = dev_alloc(dst, &out.cid, n_c)) != DBG_OK) break;
        hipLaunchKernelGGL(k_nk_emit, grid, dim3(256), 0, dst->stream, n, d, g, nxt, Sum, Hops, Min, zidx, d_drv, out.lo, out.hi,
                           out.stamp, out.code, out.cnt);
        if (hipGetLastError() != hipSuccess) { dst->err = "build_from_walks: launch failed"; rc = DBG_E_HIP; break; }
        hipError_t e = hipStreamSynchronize(dst->stream);  // the scratch goes back before the next block starts
        if (e != hipSuccess) { dst->err = std::string("build_from_walks: ") + hipGetErrorString(e); rc = DBG_E_HIP; break; }
        kept.next = nxt; nxt = nullptr;
        kept.start = start_of_rank; start_of_rank = nullptr;
    } while (0);
    dev_free(nxt); dev_free(J[0]); dev_free(J[1]); dev_free(H[0]); dev_free(H[1]); dev_free(cidx); dev_free(d_rank);
    dev_free(S[0]); dev_free(S[1]); dev_free(zidx); dev_free(start_of_rank); dev_free(M[0]); dev_free(M[1]); dev_free(d_drv);
    dev_free(emit);
    return rc;
}

// one block after its checks: its source, the level difference, the rank of every contig of the source inside the block
// and the offsets of the block's contigs in the virtual text
struct NkPlan {
    dbg *src = nullptr;
    int d = 0;
    std::vector<uint32_t> rank_of;
    std::vector<uint64_t> drv_off;
};

static int nk_build(dbg *dst, int k1, std::vector<NkPlan> &plan, uint64_t T, uint64_t n_kmer_virtual, const char *extra_bases,
                    const uint64_t *extra_offsets, uint64_t n_extra) {
    // the extra reads become dst's reads (dbg_set_reads frees dst's graph); their k1-graph is built on a helper handle
    CHK(dbg_set_reads(dst, extra_bases, extra_offsets, n_extra));
    CHK(compute_alphabet(dst));
    if (!dst->is_dna) { dst->err = "extra reads must be made of A, C, G and T"; return DBG_E_ALPHABET; }
    Timer t_all(dst->stream);
    dbg *ex = nullptr;
    uint64_t n_e = 0;
    if (dst->n_bytes) {
        CHK(dbg_create(dst->device, &ex));
        int rc = dbg_set_reads_device(ex, dst->d_bases, dst->n_bytes, dst->d_offsets, dst->n_reads);
        if (rc == DBG_OK) rc = dbg_build(ex, k1, 0);
        if (rc == DBG_OK) rc = dbg_refine_edge_order(ex);
        if (rc == DBG_OK) rc = ensure_dense(ex);
        if (rc != DBG_OK) { dst->err = std::string("extra reads: ") + ex->err; dbg_destroy(ex); return rc; }
        n_e = ex->n_nodes;
    }
    const bool wide = k1 > 31;
    const uint64_t n_blocks = plan.size();
    std::vector<NkNodes> nodes(n_blocks);
    std::vector<dbg::NkBlock> kept(n_blocks);
    uint32_t *newidx = nullptr, *tab_id = nullptr;
    uint64_t *tab_lo = nullptr, *tab_hi = nullptr;
    uint8_t *isnew = nullptr, *fs = nullptr;
    uint16_t *bo = nullptr;
    auto cleanup = [&]() {
        for (auto &b : nodes) b.release();
        for (auto &b : kept) { dev_free(b.next); dev_free(b.z); dev_free(b.start); }
        dev_free(newidx); dev_free(tab_id); dev_free(tab_lo); dev_free(tab_hi); dev_free(isnew); dev_free(fs); dev_free(bo);
        if (ex) { dbg_destroy(ex); ex = nullptr; }
    };
    int rc = DBG_OK;
    do {
        // 1.-4. block by block: the chain reductions and the block's K-nodes
        uint64_t n_c_all = 0;
        for (uint64_t b = 0; b < n_blocks && rc == DBG_OK; ++b) {
            rc = nk_chain_block(dst, plan[b].src, plan[b].d, plan[b].rank_of, plan[b].drv_off, nodes[b], kept[b]);
            std::vector<uint32_t>().swap(plan[b].rank_of);
            std::vector<uint64_t>().swap(plan[b].drv_off);
            n_c_all += nodes[b].n_c;
        }
        if (rc != DBG_OK) break;
        if (n_e + n_c_all >= 0xFFFFFFF0ull) { dst->err = "more than 2^32-16 nodes"; rc = DBG_E_CAPACITY; break; }
        // 5. union by key: the extra reads' graph first (ids 0 .. n_e-1), then the new nodes of every block in block order
        uint64_t cap = 1024;
        while (cap < 2 * (n_e + n_c_all)) cap <<= 1;
        if ((rc = dev_alloc(dst, &tab_id, cap)) != DBG_OK || (rc = dev_alloc(dst, &tab_lo, cap)) != DBG_OK ||
            (rc = dev_alloc(dst, &tab_hi, cap)) != DBG_OK) break;
        NK_HIP(dst, hipMemsetAsync(tab_id, 0xFF, cap * 4, dst->stream));
        const NkTab tab{tab_id, tab_lo, tab_hi, cap - 1};
        if (n_e) hipLaunchKernelGGL(k_nk_insert, dim3(grid_for(n_e, 256)), dim3(256), 0, dst->stream, n_e, ex->d_keys, ex->d_keys_hi, tab);
        std::vector<uint64_t> new_from(n_blocks + 1, n_e);
        for (uint64_t b = 0; b < n_blocks && rc == DBG_OK; ++b) {
            const NkNodes &nb = nodes[b];
            uint64_t n_new = 0;
            if (nb.n_c) {
                const dim3 cgrid(grid_for(nb.n_c, 256));
                if ((rc = dev_alloc(dst, &isnew, nb.n_c)) != DBG_OK || (rc = dev_alloc(dst, &newidx, nb.n_c)) != DBG_OK) break;
                hipLaunchKernelGGL(k_nk_match, cgrid, dim3(256), 0, dst->stream, nb.n_c, nb.lo, nb.hi, tab, nb.cid, isnew);
                if ((rc = exclusive_scan(dst, nb.n_c, ByteAt{isnew}, newidx, &n_new)) != DBG_OK) break;
                hipLaunchKernelGGL(k_nk_insert_new, cgrid, dim3(256), 0, dst->stream, nb.n_c, new_from[b], isnew, newidx, nb.lo, nb.hi,
                                   tab, nb.cid);
                NK_HIP(dst, hipStreamSynchronize(dst->stream));
                dev_free(isnew); dev_free(newidx);
            }
            new_from[b + 1] = new_from[b] + n_new;
        }
        if (rc != DBG_OK) break;
        const uint64_t nn = new_from[n_blocks];
        // dst's node arrays (owned: free_build releases them)
        dst->k = k1;
        if ((rc = dev_alloc(dst, &dst->d_keys, nn)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_stamps, nn)) != DBG_OK ||
            (rc = dev_alloc(dst, &dst->d_cnt, nn * 4)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_succ, nn * 4)) != DBG_OK ||
            (rc = dev_alloc(dst, &dst->d_flags, nn)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_order, nn)) != DBG_OK ||
            (rc = dev_alloc(dst, &dst->d_fsorder, nn)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_deg, nn)) != DBG_OK) break;
        if (wide && (rc = dev_alloc(dst, &dst->d_keys_hi, nn)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &fs, nn)) != DBG_OK || (rc = dev_alloc(dst, &bo, nn)) != DBG_OK) break;
        dst->n_nodes = nn;
        if (n_e)
            hipLaunchKernelGGL(k_nk_fill_extra, dim3(grid_for(n_e, 256)), dim3(256), 0, dst->stream, n_e, ex->d_keys, ex->d_keys_hi,
                               ex->d_stamps, ex->d_cnt, ex->d_fsorder, 2 * T, dst->d_keys, dst->d_keys_hi, dst->d_stamps, dst->d_cnt,
                               fs, bo);
        for (uint64_t b = 0; b < n_blocks; ++b) {
            const NkNodes &nb = nodes[b];
            if (nb.n_c)
                hipLaunchKernelGGL(k_nk_fill_contig, dim3(grid_for(nb.n_c, 256)), dim3(256), 0, dst->stream, nb.n_c, new_from[b], nb.lo,
                                   nb.hi, nb.stamp, nb.code, nb.cnt, nb.cid, dst->d_keys, dst->d_keys_hi, dst->d_stamps, dst->d_cnt,
                                   fs, bo);
        }
        if (nn)
            hipLaunchKernelGGL(k_nk_succ, dim3(grid_for(nn, 256)), dim3(256), 0, dst->stream, nn, k1, dst->d_keys, dst->d_keys_hi,
                               dst->d_stamps, dst->d_cnt, fs, bo, tab, dst->d_succ, dst->d_deg, dst->d_flags, dst->d_order,
                               dst->d_fsorder);
        // 6. what dbg_mark_pull_reads needs later, per block: chain successors, z(x), the start of every virtual read
        for (uint64_t b = 0; b < n_blocks; ++b) {
            const uint64_t n = kept[b].n_src;
            if (!n) continue;
            if ((rc = dev_alloc(dst, &kept[b].z, n)) != DBG_OK) break;
            hipLaunchKernelGGL(k_nk_zmap, dim3(grid_for(n, 256)), dim3(256), 0, dst->stream, n, plan[b].d, dna_view(plan[b].src),
                               kept[b].next, tab, kept[b].z);
        }
        if (rc != DBG_OK) break;
        if (hipGetLastError() != hipSuccess) { dst->err = "build_from_walks: launch failed"; rc = DBG_E_HIP; break; }
        uint64_t edges = 0;
        if ((rc = reduce_sum(dst, nn * 4, CountSum{dst->d_cnt}, &edges)) != DBG_OK) break;
        dst->n_edge_inst = edges;
        dst->n_kmer_inst = n_kmer_virtual + (ex ? ex->n_kmer_inst : 0);
        if ((rc = finish_graph(dst)) != DBG_OK) break;
        dst->order_exact = true;
        dst->nk_graph = true;
        dst->nk_bytes = T;
        dst->nk_reads = 0;
        for (const auto &b : kept) dst->nk_reads += b.n_reads;
        dst->nk_blocks.swap(kept);
        kept.clear();
        hipError_t e = hipStreamSynchronize(dst->stream);
        if (e != hipSuccess) { dst->err = std::string("build_from_walks: ") + hipGetErrorString(e); rc = DBG_E_HIP; break; }
    } while (0);
    cleanup();
    if (rc != DBG_OK) { const std::string keep = dst->err; free_build(dst); dst->err = keep; return rc; }
    dst->stats = dbg_stats_t{};
    dst->stats.ms_build_total = t_all.stop();
    return DBG_OK;
}

// contig lengths of src's walk -> the block's offsets in the virtual text, from `base` on; adds the block's K-mer windows
static int nk_plan_block(dbg *dst, dbg *src, int k1, const uint64_t *contigs, uint64_t n_sel, uint64_t base, NkPlan &p,
                         uint64_t &n_kmer_virtual) {
    const uint64_t n_ctg = src->n_contigs;
    p.src = src;
    p.d = k1 - src->k;
    p.rank_of.assign(n_ctg, NK_NONE);
    for (uint64_t r = 0; r < n_sel; ++r) {
        if (contigs[r] >= n_ctg) { dst->err = "a block names a contig index out of range"; return DBG_E_ARG; }
        if (p.rank_of[contigs[r]] != NK_NONE) { dst->err = "a block names a contig twice"; return DBG_E_ARG; }
        p.rank_of[contigs[r]] = (uint32_t)r;
    }
    HIPCHK(dst, hipSetDevice(src->device));
    CHK(ensure_dense(src));
    std::vector<uint64_t> off(n_ctg + 1, 0);
    if (n_ctg) HIPCHK(dst, hipMemcpyAsync(off.data(), src->d_ctg_off, (n_ctg + 1) * 8, hipMemcpyDeviceToHost, src->stream));
    HIPCHK(dst, hipStreamSynchronize(src->stream));
    p.drv_off.assign(n_sel + 1, base);
    for (uint64_t r = 0; r < n_sel; ++r) {
        const uint64_t len = off[contigs[r] + 1] - off[contigs[r]];
        p.drv_off[r + 1] = p.drv_off[r] + len;
        if (len > (uint64_t)k1) n_kmer_virtual += len - k1 + 1;  // n_kmer_instances: windows of reads with len > k, as dbg_build counts
    }
    return DBG_OK;
}

extern "C" int dbg_build_from_walks(dbg_t *dst, int k1, const dbg_walk_block_t *blocks, uint64_t n_blocks,
                                    const char *extra_bases, const uint64_t *extra_offsets, uint64_t n_extra) {
    if (!dst || (n_blocks && !blocks)) return DBG_E_ARG;
    auto refuse = [&](const char *msg) { dst->err = msg; return DBG_E_ARG; };
    if (k1 > 63) return refuse("k1 must be at most 63");
    for (uint64_t b = 0; b < n_blocks; ++b) {
        const dbg *src = blocks[b].src;
        if (!src) return refuse("a block has no source");
        if (const char *why = nk_refuse_source(dst, src, true)) return refuse(why);
        if (src->k >= k1) return refuse("k1 must be larger than the k of every source");
        if (blocks[b].n && !blocks[b].contigs) return refuse("a block has no contig indices");
        for (uint64_t a = 0; a < b; ++a)
            if (blocks[a].src == src) return refuse("the same src is named by two blocks");
    }
    if (!extra_offsets || (n_extra && extra_offsets[n_extra] && !extra_bases)) return refuse("extra reads: offsets required");
    std::vector<NkPlan> plan(n_blocks);
    uint64_t T = 0, n_kmer_virtual = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) {
        CHK(nk_plan_block(dst, blocks[b].src, k1, blocks[b].contigs, blocks[b].n, T, plan[b], n_kmer_virtual));
        T = plan[b].drv_off.back();
        if (T >= (1ull << 62)) return refuse("contig text too long for 64-bit stamps");
    }
    return nk_build(dst, k1, plan, T, n_kmer_virtual, extra_bases, extra_offsets, n_extra);
}

extern "C" int dbg_build_from_walk(dbg_t *dst, dbg_t *src, int k1, const uint64_t *order, uint64_t n_order,
                                   const char *extra_bases, const uint64_t *extra_offsets, uint64_t n_extra) {
    if (!dst || !src) return DBG_E_ARG;
    auto refuse = [&](const char *msg) { dst->err = msg; return DBG_E_ARG; };
    if (const char *why = nk_refuse_source(dst, src, false)) return refuse(why);
    if (k1 > 63) return refuse("k1 must be at most 63");
    if (k1 != src->k + 1) return refuse("k1 must be the k of src plus one");
    if (n_order != src->n_contigs || (n_order && !order)) return refuse("order must be a permutation of the contig index");
    if (src->n_nodes >= 0xFFFFFFF0ull) return refuse("src has too many nodes");
    std::vector<uint8_t> seen(n_order, 0);
    for (uint64_t r = 0; r < n_order; ++r) {
        if (order[r] >= n_order || seen[order[r]]) return refuse("order must be a permutation of the contig index");
        seen[order[r]] = 1;
    }
    const dbg_walk_block_t block{src, order, n_order};
    return dbg_build_from_walks(dst, k1, &block, 1, extra_bases, extra_offsets, n_extra);
}
