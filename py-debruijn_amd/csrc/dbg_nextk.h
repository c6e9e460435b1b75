// The driver's k -> k+1 step (II_assembleFromReads.py:56-75) without spelling the contigs: dbg_build_from_walk builds the
// (k+1)-graph of (contigs of the last non-final walk, in driver order) + (extra reads) straight from the chain structure
// of the k-graph.  Included by dbg_hip.hip after every helper it uses ("Next k from the walk").
//
// A non-final contig is a chain x0 -> x1 -> ... -> x(n-1) under one per-node continuation nxt() (k_jump_init's rule), so
// for the (k+1)-graph of the contigs:
//   - nodes: y(x) = key(x) * 4 + last base of nxt(x), for every x on a contig of n >= 3 nodes that has nxt(x);
//   - count of the edge y(x) -> y(nxt x): S(x) = number of such contigs through x (a sum over the starts upstream);
//   - first occurrence: the lowest-ranked such contig through x, at hop distance d from its start: (off + d) << 1 | d != 0.
// Both reductions run by doubling over the jump pointers J_j(u) = nxt^(2^j)(u) (NONE past the chain end, never wrapped):
// B_(j+1)(v) = B_j(v) (+) sum over u with J_j(u) = v of B_j(u), one scatter per round.  Upstream sets of distinct u are
// disjoint in a forest, so every start counts once; cycles carry no weight (they emit no contig).
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

// weights of the starts: contig index c (ascending start id == the walk's index), driver rank r = rank_of[c]
__global__ __launch_bounds__(256) void k_nk_weights(uint64_t n, const uint8_t *__restrict__ emit, const uint32_t *__restrict__ cidx,
                                                    const uint32_t *__restrict__ H, const uint32_t *__restrict__ rank_of,
                                                    uint32_t *S, unsigned long long *M, uint32_t *start_of_rank) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    uint32_t s = 0;
    unsigned long long m = ~0ull;
    if (emit[v]) {
        const uint32_t r = rank_of[cidx[v]];
        start_of_rank[r] = (uint32_t)v;
        if (H[v] >= 2) { s = 1; m = (unsigned long long)r << 32; }  // n >= 3 nodes: the contig makes (k+1)-nodes
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

__device__ inline void nk_ykey(const GDna &g, uint32_t x, uint32_t c, uint64_t &lo, uint64_t &hi) {
    const uint64_t l = g.keys[x], h = g.keys_hi ? g.keys_hi[x] : 0ull;
    lo = (l << 2) | c;
    hi = (h << 2) | (l >> 62);
}

struct NkYFlag {
    const uint32_t *S, *nxt;
    __device__ uint64_t operator()(uint64_t i) const { return S[i] && nxt[i] != NK_NONE; }
};

// the (k+1)-nodes of the contigs: key, stamp, the one successor code (0xFF: none) and its count
__global__ __launch_bounds__(256) void k_nk_emit(uint64_t n, GDna g, const uint32_t *__restrict__ nxt, const uint32_t *__restrict__ S,
                                                 const unsigned long long *__restrict__ M, const uint32_t *__restrict__ yidx,
                                                 const uint64_t *__restrict__ drv_off, uint64_t *ck_lo, uint64_t *ck_hi,
                                                 uint64_t *cstamp, uint8_t *ccode, uint32_t *ccnt) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n || !S[x] || nxt[x] == NK_NONE) return;
    const uint32_t j = yidx[x], nx = nxt[x], nnx = nxt[nx];
    uint64_t lo, hi;
    nk_ykey(g, (uint32_t)x, g.last_code(nx), lo, hi);
    ck_lo[j] = lo;
    ck_hi[j] = hi;
    const uint64_t m = M[x], d = m & 0xFFFFFFFFull;
    cstamp[j] = ((drv_off[m >> 32] + d) << 1) | (d != 0);
    ccode[j] = nnx != NK_NONE ? (uint8_t)g.last_code(nnx) : (uint8_t)0xFF;
    ccnt[j] = nnx != NK_NONE ? S[x] : 0u;
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

// contig node j: the extra-read node with its key, or NONE (then it is new)
__global__ __launch_bounds__(256) void k_nk_match(uint64_t n_c, const uint64_t *__restrict__ ck_lo, const uint64_t *__restrict__ ck_hi,
                                                  NkTab tab, uint32_t *hit, uint8_t *isnew) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_c) return;
    const uint32_t e = tab.find(ck_lo[j], ck_hi[j]);
    hit[j] = e;
    isnew[j] = e == NK_NONE;
}

// the extra-read graph, stamps moved behind the contig text (+2T); fs = its first-seen successor order
__global__ __launch_bounds__(256) void k_nk_fill_extra(uint64_t n_e, const uint64_t *__restrict__ e_lo, const uint64_t *__restrict__ e_hi,
                                                       const uint64_t *__restrict__ e_st, const uint32_t *__restrict__ e_cnt,
                                                       const uint8_t *__restrict__ e_fs, uint64_t stamp_add, uint64_t *lo,
                                                       uint64_t *hi, uint64_t *st, uint32_t *cnt, uint8_t *fs, uint8_t *c0) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_e) return;
    lo[i] = e_lo[i];
    if (hi) hi[i] = e_hi ? e_hi[i] : 0ull;
    st[i] = e_st[i] + stamp_add;
    reinterpret_cast<uint4 *>(cnt)[i] = reinterpret_cast<const uint4 *>(e_cnt)[i];
    fs[i] = e_fs[i];
    c0[i] = 0xFF;
}

// contig nodes: merged into their extra-read twin (counts add, the contig's earlier stamp wins) or appended
__global__ __launch_bounds__(256) void k_nk_fill_contig(uint64_t n_c, uint64_t n_e, const uint64_t *__restrict__ ck_lo,
                                                        const uint64_t *__restrict__ ck_hi, const uint64_t *__restrict__ cstamp,
                                                        const uint8_t *__restrict__ ccode, const uint32_t *__restrict__ ccnt,
                                                        const uint32_t *__restrict__ hit, const uint32_t *__restrict__ newidx,
                                                        uint64_t *lo, uint64_t *hi, uint64_t *st, uint32_t *cnt, uint8_t *fs,
                                                        uint8_t *c0, uint32_t *cid) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_c) return;
    uint32_t id = hit[j];
    const uint8_t c = ccode[j];
    if (id == NK_NONE) {
        id = (uint32_t)(n_e + newidx[j]);
        lo[id] = ck_lo[j];
        if (hi) hi[id] = ck_hi[j];
        reinterpret_cast<uint4 *>(cnt)[id] = make_uint4(0, 0, 0, 0);
        fs[id] = 0;
    }
    st[id] = cstamp[j];  // below T: earlier than any extra read
    if (c != 0xFF) cnt[(uint64_t)id * 4 + c] += ccnt[j];
    c0[id] = c;
    cid[j] = id;
}

__global__ __launch_bounds__(256) void k_nk_insert_new(uint64_t n_c, const uint8_t *__restrict__ isnew, const uint32_t *__restrict__ cid,
                                                       const uint64_t *__restrict__ ck_lo, const uint64_t *__restrict__ ck_hi, NkTab tab) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_c && isnew[j]) tab.insert(ck_lo[j], ck_hi[j], cid[j]);
}

// successors by key, degrees, indegree flags and the two rank bytes.  First-seen key of a code: the contig successor c0
// first (its first occurrence is below T), then the extra graph's first-seen order; codes without count last, in ASCII
// order (A C G T = codes 0 1 3 2) as every build ranks them.  most_common = (count desc, first seen asc).
__global__ __launch_bounds__(256) void k_nk_succ(uint64_t n, int k1, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                 const uint64_t *__restrict__ st, const uint32_t *__restrict__ cnt,
                                                 const uint8_t *__restrict__ fs, const uint8_t *__restrict__ c0, NkTab tab,
                                                 uint32_t *succ, uint8_t *deg, uint8_t *flags, uint8_t *order, uint8_t *fsorder) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 c4 = reinterpret_cast<const uint4 *>(cnt)[i];
    const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
    const uint64_t l = lo[i], h = hi ? hi[i] : 0ull;
    const uint64_t lo_mask = k1 >= 32 ? ~0ull : ((1ull << (2 * k1)) - 1);
    const uint64_t hi_mask = k1 > 32 ? ((1ull << (2 * k1 - 64)) - 1) : 0ull;
    const uint8_t f = fs[i], z = c0[i];
    uint32_t s[4], key[4], code[4] = {0, 1, 2, 3};
    const uint32_t ascii_rank[4] = {0, 1, 3, 2};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        s[b] = NK_NONE;
        if (c[b]) {
            s[b] = tab.find(((l << 2) | (uint64_t)b) & lo_mask, ((h << 2) | (l >> 62)) & hi_mask);
            uint32_t pos = 0;
            for (int r = 0; r < 4; ++r)
                if (((f >> (2 * r)) & 3u) == (uint32_t)b) { pos = r; break; }
            key[b] = (b == z) ? 0u : 1u + pos;
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

// y(x) for every k-node x with a chain successor: the (k+1)-node id in the union, or NONE
__global__ __launch_bounds__(256) void k_nk_ymap(uint64_t n, GDna g, const uint32_t *__restrict__ nxt, NkTab tab, int k1, uint32_t *y) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const uint32_t nx = nxt[x];
    uint32_t r = NK_NONE;
    if (nx != NK_NONE) {
        uint64_t lo, hi;
        nk_ykey(g, (uint32_t)x, g.last_code(nx), lo, hi);
        (void)k1;
        r = tab.find(lo, hi);
    }
    y[x] = r;
}

// ---- pull-out reads of the contigs: OR over a chain (last node excluded) of "y(x) is a branch (k+1)-node"
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

// called by dbg_mark_pull_reads on a graph from dbg_build_from_walk: flags of the virtual contig reads
static int nk_mark_contigs(dbg *h) {
    dev_free(h->d_nk_read_flags);
    CHK(dev_alloc(h, &h->d_nk_read_flags, h->nk_reads));
    HIPCHK(h, hipMemsetAsync(h->d_nk_read_flags, 0, h->nk_reads ? h->nk_reads : 1, h->stream));
    if (!h->nk_reads || !h->n_branch) return DBG_OK;
    const uint64_t n = h->nk_src_nodes;
    uint32_t *J[2] = {nullptr, nullptr};
    uint8_t *P[2] = {nullptr, nullptr};
    int rc = DBG_OK;
    do {
        if ((rc = dev_alloc(h, &J[0], n)) != DBG_OK || (rc = dev_alloc(h, &J[1], n)) != DBG_OK ||
            (rc = dev_alloc(h, &P[0], n)) != DBG_OK || (rc = dev_alloc(h, &P[1], n)) != DBG_OK) break;
        const dim3 grid(grid_for(n, 256));
        if (n) hipLaunchKernelGGL(k_nk_or_init, grid, dim3(256), 0, h->stream, n, h->d_nk_y, h->d_flags, h->d_nk_next, J[0], P[0]);
        int cur = 0;
        const int rounds = n ? nk_jump_until_closed(h, n, [&](int, unsigned long long *open) {
            hipLaunchKernelGGL(k_nk_or_step, grid, dim3(256), 0, h->stream, n, J[cur], P[cur], J[cur ^ 1], P[cur ^ 1], open);
            cur ^= 1;
        }) : 0;
        if (rounds < 0) { rc = DBG_E_HIP; break; }
        hipLaunchKernelGGL(k_nk_or_gather, dim3(grid_for(h->nk_reads, 256)), dim3(256), 0, h->stream, h->nk_reads, h->d_nk_start,
                           P[cur], h->d_nk_read_flags);
        if (hipGetLastError() != hipSuccess) { h->err = "pull-out contigs: launch failed"; rc = DBG_E_HIP; break; }
        uint64_t total = 0;
        if ((rc = reduce_sum(h, h->nk_reads, ByteAt{h->d_nk_read_flags}, &total)) != DBG_OK) break;
        h->n_pull_reads += total;
    } while (0);
    dev_free(J[0]); dev_free(J[1]); dev_free(P[0]); dev_free(P[1]);
    return rc;
}

extern "C" int dbg_build_from_walk(dbg_t *dst, dbg_t *src, int k1, const uint64_t *order, uint64_t n_order,
                                   const char *extra_bases, const uint64_t *extra_offsets, uint64_t n_extra) {
    if (!dst || !src) return DBG_E_ARG;
    if (dst == src) { dst->err = "dst and src must be different handles"; return DBG_E_ARG; }
    if (dst->device != src->device) { dst->err = "dst and src must be on the same device"; return DBG_E_ARG; }
    auto refuse = [&](const char *msg) { dst->err = msg; return DBG_E_ARG; };
    if (!src->k || !src->walk_indexed) return refuse("src has no walk of its current graph");
    if (src->multipass || src->partial_graph) return refuse("src holds a graph in parts: build from a single-table graph");
    if (src->D != 4 || !src->is_dna) return refuse("src is not an ACGT graph (generic alphabets take the text path)");
    if (src->walk_final) return refuse("the last walk of src was a final-mode walk (all simple paths, not chains)");
    if (k1 > 63) return refuse("k1 must be at most 63");
    if (k1 != src->k + 1) return refuse("k1 must be the k of src plus one");
    if (n_order != src->n_contigs || (n_order && !order)) return refuse("order must be a permutation of the contig index");
    if (src->n_nodes >= 0xFFFFFFF0ull) return refuse("src has too many nodes");
    std::vector<uint32_t> rank_of(n_order, NK_NONE);
    for (uint64_t r = 0; r < n_order; ++r) {
        if (order[r] >= n_order || rank_of[order[r]] != NK_NONE) return refuse("order must be a permutation of the contig index");
        rank_of[order[r]] = (uint32_t)r;
    }
    if (!extra_offsets || (n_extra && extra_offsets[n_extra] && !extra_bases)) return refuse("extra reads: offsets required");
    HIPCHK(src, hipSetDevice(src->device));
    CHK(ensure_dense(src));
    // contig lengths in driver order -> offsets of the virtual reads
    std::vector<uint64_t> off(n_order + 1, 0), drv_off(n_order + 1, 0);
    if (n_order) {
        HIPCHK(src, hipMemcpyAsync(off.data(), src->d_ctg_off, (n_order + 1) * 8, hipMemcpyDeviceToHost, src->stream));
        HIPCHK(src, hipStreamSynchronize(src->stream));
    }
    uint64_t n_kmer_virtual = 0;
    for (uint64_t r = 0; r < n_order; ++r) {
        const uint64_t len = off[order[r] + 1] - off[order[r]];
        drv_off[r + 1] = drv_off[r] + len;
        if (len >= (uint64_t)k1) n_kmer_virtual += len - k1 + 1;  // KmerInstances: windows of reads with len >= k
    }
    const uint64_t T = drv_off[n_order];
    if (T >= (1ull << 62)) return refuse("contig text too long for 64-bit stamps");

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
    const GDna g = dna_view(src);
    const uint64_t n = src->n_nodes;
    const dim3 grid(grid_for(n, 256));
    const bool wide = k1 > 31;
    // scratch of the chain phase (freed at the end) and the arrays dst keeps for its pull-out test
    uint32_t *nxt = nullptr, *J[2] = {nullptr, nullptr}, *H[2] = {nullptr, nullptr}, *cidx = nullptr, *d_rank = nullptr,
             *S[2] = {nullptr, nullptr}, *yidx = nullptr, *start_of_rank = nullptr, *ccnt = nullptr, *hit = nullptr,
             *newidx = nullptr, *cid = nullptr, *ynode = nullptr, *tab_id = nullptr;
    unsigned long long *M[2] = {nullptr, nullptr};
    uint64_t *d_drv = nullptr, *ck_lo = nullptr, *ck_hi = nullptr, *cstamp = nullptr, *tab_lo = nullptr, *tab_hi = nullptr;
    uint8_t *emit = nullptr, *ccode = nullptr, *isnew = nullptr, *fs = nullptr, *c0 = nullptr;
    auto cleanup = [&]() {
        dev_free(nxt); dev_free(J[0]); dev_free(J[1]); dev_free(H[0]); dev_free(H[1]); dev_free(cidx); dev_free(d_rank);
        dev_free(S[0]); dev_free(S[1]); dev_free(yidx); dev_free(start_of_rank); dev_free(ccnt); dev_free(hit); dev_free(newidx);
        dev_free(cid); dev_free(ynode); dev_free(tab_id); dev_free(M[0]); dev_free(M[1]); dev_free(d_drv); dev_free(ck_lo);
        dev_free(ck_hi); dev_free(cstamp); dev_free(tab_lo); dev_free(tab_hi); dev_free(emit); dev_free(ccode); dev_free(isnew);
        dev_free(fs); dev_free(c0);
        if (ex) { dbg_destroy(ex); ex = nullptr; }
    };
    int rc = DBG_OK;
    do {
        // 1. continuation pointers and hops to the chain end
        if ((rc = dev_alloc(dst, &nxt, n)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &J[0], n)) != DBG_OK || (rc = dev_alloc(dst, &J[1], n)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &H[0], n)) != DBG_OK || (rc = dev_alloc(dst, &H[1], n)) != DBG_OK) break;
        if (n) {
            hipLaunchKernelGGL(k_nk_next, grid, dim3(256), 0, dst->stream, n, g, nxt);
            hipLaunchKernelGGL(k_nk_hops_init, grid, dim3(256), 0, dst->stream, n, nxt, J[0], H[0]);
        }
        int cur = 0;
        if (n && nk_jump_until_closed(dst, n, [&](int, unsigned long long *open) {
                hipLaunchKernelGGL(k_nk_rank_step, grid, dim3(256), 0, dst->stream, n, J[cur], H[cur], J[cur ^ 1], H[cur ^ 1], open);
                cur ^= 1;
            }) < 0) { rc = DBG_E_HIP; break; }
        uint32_t *Jend = J[cur], *Hops = H[cur];
        // 2. emitting starts == the walk's contig index (checked against it)
        if ((rc = dev_alloc(dst, &emit, n)) != DBG_OK || (rc = dev_alloc(dst, &cidx, n)) != DBG_OK) break;
        if (n) hipLaunchKernelGGL(k_nk_emits, grid, dim3(256), 0, dst->stream, n, g.flags, Jend, emit);
        uint64_t n_ctg = 0, n_chr = 0;
        if ((rc = exclusive_scan(dst, n, ByteAt{emit}, cidx, &n_ctg)) != DBG_OK) break;
        if ((rc = reduce_sum(dst, n, NkChars{emit, Hops, src->k}, &n_chr)) != DBG_OK) break;
        if (n_ctg != src->n_contigs || n_chr != src->contig_chars) {
            dst->err = "internal: chains disagree with the walk's contig index";
            rc = DBG_E_HIP;
            break;
        }
        // 3. start weights, then doubling of (sum, min) over the jump pointers
        if ((rc = dev_alloc(dst, &d_rank, n_order)) != DBG_OK || (rc = dev_alloc(dst, &start_of_rank, n_order)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &d_drv, n_order + 1)) != DBG_OK) break;
        if (n_order) {
            HIPCHK(dst, hipMemcpyAsync(d_rank, rank_of.data(), n_order * 4, hipMemcpyHostToDevice, dst->stream));
            HIPCHK(dst, hipMemcpyAsync(d_drv, drv_off.data(), (n_order + 1) * 8, hipMemcpyHostToDevice, dst->stream));
        }
        if ((rc = dev_alloc(dst, &S[0], n)) != DBG_OK || (rc = dev_alloc(dst, &S[1], n)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &M[0], n)) != DBG_OK || (rc = dev_alloc(dst, &M[1], n)) != DBG_OK) break;
        dev_free(H[cur ^ 1]);
        if (n) {
            hipLaunchKernelGGL(k_nk_weights, grid, dim3(256), 0, dst->stream, n, emit, cidx, Hops, d_rank, S[0], M[0], start_of_rank);
            HIPCHK(dst, hipMemcpyAsync(J[0], nxt, n * 4, hipMemcpyDeviceToDevice, dst->stream));
        }
        cur = 0;
        if (n && nk_jump_until_closed(dst, n, [&](int round, unsigned long long *open) {
                (void)hipMemcpyAsync(S[cur ^ 1], S[cur], n * 4, hipMemcpyDeviceToDevice, dst->stream);
                (void)hipMemcpyAsync(M[cur ^ 1], M[cur], n * 8, hipMemcpyDeviceToDevice, dst->stream);
                hipLaunchKernelGGL(k_nk_push, grid, dim3(256), 0, dst->stream, n, round, J[cur], S[cur], M[cur], J[cur ^ 1], S[cur ^ 1],
                                   M[cur ^ 1], open);
                cur ^= 1;
            }, true) < 0) { rc = DBG_E_HIP; break; }
        const uint32_t *Sum = S[cur];
        const unsigned long long *Min = M[cur];
        // 4. the (k+1)-nodes of the contigs
        uint64_t n_c = 0;
        if ((rc = dev_alloc(dst, &yidx, n)) != DBG_OK) break;
        if ((rc = exclusive_scan(dst, n, NkYFlag{Sum, nxt}, yidx, &n_c)) != DBG_OK) break;
        if (n_e + n_c >= 0xFFFFFFF0ull) { dst->err = "more than 2^32-16 nodes"; rc = DBG_E_CAPACITY; break; }
        if ((rc = dev_alloc(dst, &ck_lo, n_c)) != DBG_OK || (rc = dev_alloc(dst, &ck_hi, n_c)) != DBG_OK ||
            (rc = dev_alloc(dst, &cstamp, n_c)) != DBG_OK || (rc = dev_alloc(dst, &ccode, n_c)) != DBG_OK ||
            (rc = dev_alloc(dst, &ccnt, n_c)) != DBG_OK) break;
        if (n) hipLaunchKernelGGL(k_nk_emit, grid, dim3(256), 0, dst->stream, n, g, nxt, Sum, Min, yidx, d_drv, ck_lo, ck_hi, cstamp,
                                  ccode, ccnt);
        // 5. union with the extra reads' graph by key
        uint64_t cap = 1024;
        while (cap < 2 * (n_e + n_c)) cap <<= 1;
        if ((rc = dev_alloc(dst, &tab_id, cap)) != DBG_OK || (rc = dev_alloc(dst, &tab_lo, cap)) != DBG_OK ||
            (rc = dev_alloc(dst, &tab_hi, cap)) != DBG_OK) break;
        HIPCHK(dst, hipMemsetAsync(tab_id, 0xFF, cap * 4, dst->stream));
        const NkTab tab{tab_id, tab_lo, tab_hi, cap - 1};
        if (n_e) hipLaunchKernelGGL(k_nk_insert, dim3(grid_for(n_e, 256)), dim3(256), 0, dst->stream, n_e, ex->d_keys, ex->d_keys_hi, tab);
        if ((rc = dev_alloc(dst, &hit, n_c)) != DBG_OK || (rc = dev_alloc(dst, &isnew, n_c)) != DBG_OK ||
            (rc = dev_alloc(dst, &newidx, n_c)) != DBG_OK || (rc = dev_alloc(dst, &cid, n_c)) != DBG_OK) break;
        const dim3 cgrid(grid_for(n_c, 256));
        if (n_c) hipLaunchKernelGGL(k_nk_match, cgrid, dim3(256), 0, dst->stream, n_c, ck_lo, ck_hi, tab, hit, isnew);
        uint64_t n_new = 0;
        if ((rc = exclusive_scan(dst, n_c, ByteAt{isnew}, newidx, &n_new)) != DBG_OK) break;
        const uint64_t nn = n_e + n_new;
        // dst's node arrays (owned: free_build releases them)
        dst->k = k1;
        if ((rc = dev_alloc(dst, &dst->d_keys, nn)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_stamps, nn)) != DBG_OK ||
            (rc = dev_alloc(dst, &dst->d_cnt, nn * 4)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_succ, nn * 4)) != DBG_OK ||
            (rc = dev_alloc(dst, &dst->d_flags, nn)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_order, nn)) != DBG_OK ||
            (rc = dev_alloc(dst, &dst->d_fsorder, nn)) != DBG_OK || (rc = dev_alloc(dst, &dst->d_deg, nn)) != DBG_OK) break;
        if (wide && (rc = dev_alloc(dst, &dst->d_keys_hi, nn)) != DBG_OK) break;
        if ((rc = dev_alloc(dst, &fs, nn)) != DBG_OK || (rc = dev_alloc(dst, &c0, nn)) != DBG_OK) break;
        dst->n_nodes = nn;
        if (n_e)
            hipLaunchKernelGGL(k_nk_fill_extra, dim3(grid_for(n_e, 256)), dim3(256), 0, dst->stream, n_e, ex->d_keys, ex->d_keys_hi,
                               ex->d_stamps, ex->d_cnt, ex->d_fsorder, 2 * T, dst->d_keys, dst->d_keys_hi, dst->d_stamps, dst->d_cnt,
                               fs, c0);
        if (n_c) {
            hipLaunchKernelGGL(k_nk_fill_contig, cgrid, dim3(256), 0, dst->stream, n_c, n_e, ck_lo, ck_hi, cstamp, ccode, ccnt, hit,
                               newidx, dst->d_keys, dst->d_keys_hi, dst->d_stamps, dst->d_cnt, fs, c0, cid);
            hipLaunchKernelGGL(k_nk_insert_new, cgrid, dim3(256), 0, dst->stream, n_c, isnew, cid, ck_lo, ck_hi, tab);
        }
        if (nn)
            hipLaunchKernelGGL(k_nk_succ, dim3(grid_for(nn, 256)), dim3(256), 0, dst->stream, nn, k1, dst->d_keys, dst->d_keys_hi,
                               dst->d_stamps, dst->d_cnt, fs, c0, tab, dst->d_succ, dst->d_deg, dst->d_flags, dst->d_order,
                               dst->d_fsorder);
        // 6. what dbg_mark_pull_reads needs later: chain successors, y(x), the start of every virtual read
        if ((rc = dev_alloc(dst, &ynode, n)) != DBG_OK) break;
        if (n) hipLaunchKernelGGL(k_nk_ymap, grid, dim3(256), 0, dst->stream, n, g, nxt, tab, k1, ynode);
        if (hipGetLastError() != hipSuccess) { dst->err = "build_from_walk: launch failed"; rc = DBG_E_HIP; break; }
        uint64_t edges = 0;
        if ((rc = reduce_sum(dst, nn * 4, CountSum{dst->d_cnt}, &edges)) != DBG_OK) break;
        dst->n_edge_inst = edges;
        dst->n_kmer_inst = n_kmer_virtual + (ex ? ex->n_kmer_inst : 0);
        if ((rc = finish_graph(dst)) != DBG_OK) break;
        dst->order_exact = true;
        dst->nk_graph = true;
        dst->nk_reads = n_order;
        dst->nk_bytes = T;
        dst->nk_src_nodes = n;
        dst->d_nk_next = nxt; nxt = nullptr;
        dst->d_nk_y = ynode; ynode = nullptr;
        dst->d_nk_start = start_of_rank; start_of_rank = nullptr;
        hipError_t e = hipStreamSynchronize(dst->stream);
        if (e != hipSuccess) { dst->err = std::string("build_from_walk: ") + hipGetErrorString(e); rc = DBG_E_HIP; break; }
    } while (0);
    cleanup();
    if (rc != DBG_OK) { const std::string keep = dst->err; free_build(dst); dst->err = keep; return rc; }
    dst->stats = dbg_stats_t{};
    dst->stats.ms_build_total = t_all.stop();
    return DBG_OK;
}
