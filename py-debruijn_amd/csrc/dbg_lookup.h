// Query side of a built graph: which node is this k-mer (dbg_lookup_nodes), a few rows of the node table
// (dbg_gather_nodes), getScore of sequences that did not come out of the walk (dbg_score_sequences).
//
// Two ways to find a node, same answers:
//   directory     the builds of the LDS engines leave (SkDirEnt, SkRange) behind; dir_find / wdir_find in their comparing
//                 form replay the table's probing: bucket hash, one directory entry, one run of keys
//   sorted index  every other graph: (keys_hi, keys, id) sorted once on the device, then a lower bound per query
// A graph in parts (multi-pass, a rank of a sharded build, ranks x passes) has a directory per part: LkPartsFinder names the
// part that owns a key from the key's minimizer hash and asks that part's directory (dbg_part_lookup_nodes,
// dbg_part_score_sequences).
//
// The first part of this file -- the lower-bound search, the rolling window encoder, the owner rule and the CSR count of the
// part queries -- is plain C++: a host compiler can include this file alone (tests/test_lookup_host.py and
// tests/test_part_lookup_host.py do).  The kernels follow under __HIPCC__.
#pragma once
#include <stdint.h>

#ifndef DBG_LK_HD
#if defined(__HIPCC__)
#define DBG_LK_HD __host__ __device__
#else
#define DBG_LK_HD
#endif
#endif

namespace dbgk {

// First index i in [0, n] with (hi[i], lo[i]) >= (qhi, qlo); the pairs are sorted ascending by hi, then lo.
// hi == nullptr: every upper word is zero (one-word k-mers) and qhi is compared against zero.
DBG_LK_HD inline uint64_t lk_lower_bound(const uint64_t *hi, const uint64_t *lo, uint64_t n, uint64_t qhi, uint64_t qlo) {
    uint64_t a = 0, b = n;
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        const uint64_t mh = hi ? hi[mid] : 0ull;
        const bool less = mh < qhi || (mh == qhi && lo[mid] < qlo);
        if (less) a = mid + 1;
        else b = mid;
    }
    return a;
}

// Position of (qhi, qlo) in the sorted pairs, or n if it is not there.
DBG_LK_HD inline uint64_t lk_find_sorted(const uint64_t *hi, const uint64_t *lo, uint64_t n, uint64_t qhi, uint64_t qlo) {
    const uint64_t i = lk_lower_bound(hi, lo, n, qhi, qlo);
    if (i < n && lo[i] == qlo && (hi ? hi[i] : 0ull) == qhi) return i;
    return n;
}

// ---- rolling window encoder ----------------------------------------------------------------------------------------------
// A k-mer is the (bits * k)-bit number sum(code[i] << bits * (k - 1 - i)), first character in the top bits, in two words
// (hi * 2^64 + lo); bits = 2 (ACGT) or 5 (generic alphabet), bits * k <= 126.  `run` counts the characters since the last
// one outside the alphabet (saturating), so the window that ends at the last pushed character is a k-mer iff run >= k.
constexpr uint8_t LK_BAD_CODE = 0xFF;

struct LkWindow {
    uint64_t hi, lo;
    uint32_t run;
};

struct LkMask {
    uint64_t hi, lo;
};

DBG_LK_HD inline LkMask lk_mask(int bits, int k) {
    const int nb = bits * k;
    LkMask m;
    m.lo = nb >= 64 ? ~0ull : ((1ull << nb) - 1ull);
    m.hi = nb <= 64 ? 0ull : (nb >= 128 ? ~0ull : ((1ull << (nb - 64)) - 1ull));
    return m;
}

DBG_LK_HD inline LkWindow lk_empty() {
    LkWindow w;
    w.hi = w.lo = 0;
    w.run = 0;
    return w;
}

// Appends one character (its code, LK_BAD_CODE for a character outside the alphabet) and drops the one k back.
DBG_LK_HD inline void lk_push(LkWindow &w, uint8_t code, int bits, LkMask m) {
    const bool bad = code == LK_BAD_CODE;
    w.hi = ((w.hi << bits) | (w.lo >> (64 - bits))) & m.hi;
    w.lo = ((w.lo << bits) | (bad ? 0ull : (uint64_t)code)) & m.lo;
    w.run = bad ? 0u : (w.run == 0xFFFFFFFFu ? w.run : w.run + 1u);
}

// The window of the k characters at s, from scratch.  lut: byte -> code (256 entries, LK_BAD_CODE outside the alphabet).
DBG_LK_HD inline LkWindow lk_encode(const uint8_t *lut, const char *s, int k, int bits) {
    const LkMask m = lk_mask(bits, k);
    LkWindow w = lk_empty();
    for (int i = 0; i < k; ++i) lk_push(w, lut[(uint8_t)s[i]], bits, m);
    return w;
}

// A key handed in by a caller names a k-mer only if no bit above bits * k is set.
DBG_LK_HD inline bool lk_key_in_range(uint64_t hi, uint64_t lo, LkMask m) { return !(hi & ~m.hi) && !(lo & ~m.lo); }

// ---- graphs in parts -------------------------------------------------------------------------------------------------------
// The virtual shard (part of a multi-pass build, rank of a sharded one, rank x pass) that owns a k-mer: the top shard_bits
// of the 22-bit bucket hash of its minimizer -- the rule the builds split their records by (SkGeom::shard_bits).
constexpr int LK_BUCKET_BITS = 22;

DBG_LK_HD inline uint32_t lk_owner_of(uint32_t bucket_hash22, int shard_bits) {
    return shard_bits ? bucket_hash22 >> (LK_BUCKET_BITS - shard_bits) : 0u;
}

// Count of out-edge `code` of `node` in a part's CSR.  A row holds one column per set successor bit ((flags >> 1) & 15),
// in ascending code order (k_part_gather reads them that way): the column of `code` is the row's start plus the number of
// successor bits below it; 0 where the node has no such edge.
DBG_LK_HD inline uint32_t lk_csr_count(const uint8_t *flags, const uint32_t *row_ptr32, const uint32_t *ecnt, uint64_t node,
                                       uint32_t code) {
    const uint32_t pres = ((uint32_t)flags[node] >> 1) & 15u;
    if (!((pres >> code) & 1u)) return 0u;
    return ecnt[row_ptr32[node] + (uint32_t)__builtin_popcount(pres & ((1u << code) - 1u))];
}

}  // namespace dbgk

#if defined(__HIPCC__)
#include "dbg_sk.h"
#include "dbg_wsk.h"

namespace dbgk {

// ---- the three finders: node id of the k-mer (hi, lo), NO_NODE if it is no node --------------------------------------------
struct LkIndexFinder {  // sorted index: hi_s may be null (one-word keys)
    const uint64_t *hi_s, *lo_s;
    const uint32_t *id_s;
    uint64_t n;
    __device__ inline uint32_t find(uint64_t hi, uint64_t lo) const {
        const uint64_t i = lk_find_sorted(hi_s, lo_s, n, hi, lo);
        return i < n ? id_s[i] : NO_NODE;
    }
};

// The range chain of a bucket that was counted in hash sub-ranges: the range whose (mask, val) takes sub-hash `sh`.
__device__ inline bool lk_range_of(const SkRange *__restrict__ ranges, uint64_t bucket, uint64_t n_ranges, uint32_t sh, uint64_t *ri) {
    uint32_t r = ranges[bucket].next;
    for (int guard = 0; r && r < n_ranges && guard < (1 << 20); ++guard) {
        const SkRange rg = ranges[r];
        if (rg.node_cnt && (sh & rg.mask) == rg.val) { *ri = r; return true; }
        r = rg.next;
    }
    return false;
}

// Directory of a one-word build (k_succ_resolve's path; never the DIRECT form: a query need not exist).
template <int CAP>
struct LkDirFinder {
    SkGeom g;
    const SkRange *ranges;
    uint64_t n_buckets, n_ranges;
    const SkDirEnt *dirs;
    const uint64_t *keys;
    uint64_t n_nodes;
    __device__ inline uint32_t find(uint64_t hi, uint64_t lo) const {
        if (hi) return NO_NODE;
        const uint64_t bucket = sk_bucket_of(kmer_bucket22(lo, g.k, g.m), g);
        if (bucket < g.own_lo || bucket >= g.own_lo + g.own_cnt) return NO_NODE;
        bool whole = true;
        uint32_t id = dir_find<CAP>(dirs, bucket - g.own_lo, keys, n_nodes, lo, &whole);
        uint64_t ri = 0;
        if (!whole && lk_range_of(ranges, bucket, n_ranges, sub_hash(lo), &ri))
            id = dir_find<CAP>(dirs, g.own_cnt + (ri - n_buckets), keys, n_nodes, lo);
        return id;
    }
};

struct LkWDirFinder {  // two-word build (k_wsucc_resolve's path)
    SkGeom g;
    const SkRange *ranges;
    uint64_t n_buckets, n_ranges;
    const SkDirEnt *dirs;
    const uint64_t *keys, *keys_hi;
    uint64_t n_nodes;
    __device__ inline uint32_t find(uint64_t hi, uint64_t lo) const {
        const K128 key{hi, lo};
        const uint64_t bucket = sk_bucket_of(wkmer_bucket22(key, g.k, g.m), g);
        if (bucket < g.own_lo || bucket >= g.own_lo + g.own_cnt) return NO_NODE;
        bool whole = true;
        uint32_t id = wdir_find(dirs, bucket - g.own_lo, keys, keys_hi, n_nodes, key, &whole);
        uint64_t ri = 0;
        if (!whole && lk_range_of(ranges, bucket, n_ranges, wsub_hash(key), &ri))
            id = wdir_find(dirs, g.own_cnt + (ri - n_buckets), keys, keys_hi, n_nodes, key);
        return id;
    }
};

// ids[i] = node of (keys_hi[i], keys[i]); one thread per query.  An absent key sets nothing anywhere else.
template <class F>
__global__ __launch_bounds__(256) void k_lookup_nodes(F f, const uint64_t *__restrict__ keys, const uint64_t *__restrict__ keys_hi,
                                                      uint64_t n, LkMask m, uint32_t *ids) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t lo = keys[i], hi = keys_hi ? keys_hi[i] : 0ull;
    ids[i] = lk_key_in_range(hi, lo, m) ? f.find(hi, lo) : NO_NODE;
}

// ---- rows of a few nodes ---------------------------------------------------------------------------------------------------
struct LkGatherArgs {
    const uint64_t *keys, *keys_hi, *stamps;  // sources; keys_hi null: zeros
    const uint32_t *cnt;
    const uint8_t *flags;
    const uint32_t *keepmask;                 // generic layout; DNA: from the flags
    const uint8_t *order, *fsorder;           // DNA: one byte per node; generic: 32 per node
    uint64_t *o_keys, *o_keys_hi, *o_stamps;  // outputs, any may be null
    uint32_t *o_cnt;
    uint8_t *o_flags;
    uint32_t *o_keepmask;
    uint8_t *o_order, *o_fsorder;
    uint64_t n_nodes;
    int D;
};

__global__ __launch_bounds__(256) void k_gather_nodes(LkGatherArgs a, const uint32_t *__restrict__ ids, uint64_t n,
                                                      unsigned long long *bad /* += ids out of range */) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = ids[i];
    if (r >= a.n_nodes) { atomicAdd(bad, 1ull); return; }
    if (a.o_keys) a.o_keys[i] = a.keys[r];
    if (a.o_keys_hi) a.o_keys_hi[i] = a.keys_hi ? a.keys_hi[r] : 0ull;
    if (a.o_stamps) a.o_stamps[i] = a.stamps[r];
    if (a.o_cnt)
        for (int c = 0; c < a.D; ++c) a.o_cnt[i * a.D + c] = a.cnt[r * a.D + c];
    if (a.o_flags) a.o_flags[i] = a.flags[r];
    if (a.o_keepmask) a.o_keepmask[i] = a.keepmask ? a.keepmask[r] : (uint32_t)(a.flags[r] & DBG_F_KEEP_MASK) >> DBG_F_KEEP_SHIFT;
    const int ob = a.D == 4 ? 1 : a.D;  // bytes of the order arrays per node
    if (a.o_order)
        for (int c = 0; c < ob; ++c) a.o_order[i * ob + c] = a.order[r * ob + c];
    if (a.o_fsorder)
        for (int c = 0; c < ob; ++c) a.o_fsorder[i * ob + c] = a.fsorder[r * ob + c];
}

// ---- getScore of many sequences --------------------------------------------------------------------------------------------
// The work is balanced over the windows of the concatenated text, not over the sequences: a workgroup takes LK_TILE
// consecutive text positions, a thread LK_RUN of them.  Position p of sequence s (offsets[s] <= p < offsets[s + 1]) is a
// window iff p + k < offsets[s + 1]: the k-mer chars[p .. p + k) and the character behind it.  The k-mer of position
// p + 1 follows from that of p by one push (lk_push); the text is contiguous, so the rolling never restarts at a sequence
// border -- a window that would straddle one is no window.  A thread adds up the windows of the sequence it is in and
// hands the sum over when the sequence changes; what is left at the end of its run is combined in LDS with the neighbours
// that ended in the same sequence: one atomic per (workgroup, sequence) for those, so a 10^5-character sequence costs each
// of its tiles one add.  Sums are exact 64-bit integers: the order of addition is free.
constexpr int LK_RUN = 16;
constexpr int LK_NT = 256;
constexpr int LK_TILE = LK_RUN * LK_NT;

__device__ inline void lk_flush(uint64_t s, unsigned long long sum, unsigned long long miss, unsigned long long *scores,
                                unsigned long long *first_missing) {
    if (sum) atomicAdd(&scores[s], sum);
    if (miss != ~0ull) atomicMin(&first_missing[s], miss);
}

template <class F>
__global__ __launch_bounds__(LK_NT) void k_score_sequences(F f, const char *__restrict__ chars, uint64_t n_chars,
                                                           const uint64_t *__restrict__ offsets, uint64_t n_seq,
                                                           const uint8_t *__restrict__ lut, int k, int bits, int D,
                                                           const uint32_t *__restrict__ cnt, unsigned long long *scores,
                                                           unsigned long long *first_missing) {
    __shared__ uint64_t s_seq[LK_NT];
    __shared__ unsigned long long s_sum[LK_NT], s_miss[LK_NT];
    const uint64_t p0 = ((uint64_t)blockIdx.x * LK_NT + threadIdx.x) * LK_RUN;
    uint64_t seq = ~0ull;
    unsigned long long sum = 0, miss = ~0ull;
    if (p0 + (uint64_t)k < n_chars) {  // else no position from p0 on has a character behind its k-mer
        // sequence of p0: the last s with offsets[s] <= p0 (empty sequences in front of it are skipped by taking the last)
        uint64_t a = 0, b = n_seq;  // invariant: offsets[a] <= p0 < offsets[b]
        while (b - a > 1) {
            const uint64_t mid = a + ((b - a) >> 1);
            if (offsets[mid] <= p0) a = mid;
            else b = mid;
        }
        seq = a;
        uint64_t seq_beg = offsets[seq], seq_end = offsets[seq + 1];
        const LkMask m = lk_mask(bits, k);
        LkWindow w = lk_empty();
        for (int i = 0; i < k; ++i) lk_push(w, lut[(uint8_t)chars[p0 + i]], bits, m);
        const uint64_t p_lim = n_chars - (uint64_t)k, p_end = p0 + (uint64_t)LK_RUN < p_lim ? p0 + (uint64_t)LK_RUN : p_lim;
        for (uint64_t p = p0; p < p_end; ++p) {
            if (p >= seq_end) {  // the next sequence that is not empty
                lk_flush(seq, sum, miss, scores, first_missing);
                sum = 0;
                miss = ~0ull;
                do { ++seq; seq_beg = offsets[seq]; seq_end = offsets[seq + 1]; } while (p >= seq_end);
            }
            const uint8_t code = lut[(uint8_t)chars[p + k]];
            if (p + (uint64_t)k < seq_end) {
                uint32_t c = 0;
                if (w.run >= (uint32_t)k && code != LK_BAD_CODE && (int)code < D) {
                    const uint32_t node = f.find(w.hi, w.lo);
                    if (node != NO_NODE) c = cnt[(uint64_t)node * D + code];
                }
                if (c) sum += c;
                else if (miss == ~0ull) miss = p - seq_beg;  // positions ascend: the first one is the smallest
            }
            lk_push(w, code, bits, m);
        }
    }
    s_seq[threadIdx.x] = seq;
    s_sum[threadIdx.x] = sum;
    s_miss[threadIdx.x] = miss;
    __syncthreads();
    if (seq != ~0ull && (threadIdx.x == 0 || s_seq[threadIdx.x - 1] != seq)) {  // first thread of a group that ended in `seq`
        for (int t = threadIdx.x + 1; t < LK_NT && s_seq[t] == seq; ++t) {
            sum += s_sum[t];
            if (s_miss[t] < miss) miss = s_miss[t];
        }
        lk_flush(seq, sum, miss, scores, first_missing);
    }
}

// ---- graphs in parts: the finder routes to the part inside the kernel --------------------------------------------------------
static_assert(LK_BUCKET_BITS == SK_BUCKET_BITS, "lk_owner_of splits the bucket hash the builds carry");

// Everything a query needs of one part.  An empty part has no arrays: n_nodes == 0 and every pointer null.
struct LkPart {
    SkGeom g;
    const SkRange *ranges;
    uint64_t n_buckets, n_ranges;
    const SkDirEnt *dirs;
    const uint64_t *keys, *keys_hi;  // keys_hi null for k <= 31
    uint64_t n_nodes;
    const uint8_t *flags;
    const uint32_t *row_ptr32, *ecnt;
    uint64_t pad_;
};
static_assert(sizeof(LkPart) % 16 == 0, "the table is copied in 16-byte pieces");
constexpr int LK_MAX_PARTS = 64;

struct LkFound {
    uint32_t owner;  // virtual shard of the k-mer
    uint32_t part;   // its part on this handle, LK_MAX_PARTS or more: another rank's
    uint32_t local;  // node id in that part, NO_NODE: no node (or not this handle's)
};

// The descriptor table (device memory, n_passes entries) is copied into LDS once per workgroup: load() by every thread of
// the workgroup, then find().  Parts are built with 4096-slot tables only, so the directory has 64 entries per range.
template <bool WIDE>
struct LkPartsFinder {
    const LkPart *table;  // device memory
    int n_passes, v_first, shard_bits, k, m;

    __device__ inline void load(uint4 *s_tab) const {
        const uint4 *src = reinterpret_cast<const uint4 *>(table);
        const int n16 = n_passes * (int)(sizeof(LkPart) / 16);
        for (int i = threadIdx.x; i < n16; i += blockDim.x) s_tab[i] = src[i];
        __syncthreads();
    }

    __device__ inline LkFound find(const uint4 *s_tab, uint64_t hi, uint64_t lo) const {
        const K128 key{hi, lo};
        const uint32_t bh = WIDE ? wkmer_bucket22(key, k, m) : kmer_bucket22(lo, k, m);
        const uint32_t v = lk_owner_of(bh, shard_bits);
        const uint32_t p = v - (uint32_t)v_first;  // wraps for v < v_first
        LkFound r{v, p, NO_NODE};
        if (p >= (uint32_t)n_passes) { r.part = LK_MAX_PARTS; return r; }
        const LkPart *pt = reinterpret_cast<const LkPart *>(s_tab) + p;
        const uint64_t n_nodes = pt->n_nodes;
        if (!n_nodes) return r;
        const SkGeom g = pt->g;
        const uint64_t bucket = sk_bucket_of(bh, g);
        if (bucket < g.own_lo || bucket >= g.own_lo + g.own_cnt) return r;
        const SkDirEnt *dirs = pt->dirs;
        const uint64_t *keys = pt->keys;
        bool whole = true;
        uint64_t ri = 0;
        if (WIDE) {
            const uint64_t *keys_hi = pt->keys_hi;
            r.local = wdir_find(dirs, bucket - g.own_lo, keys, keys_hi, n_nodes, key, &whole);
            if (!whole && lk_range_of(pt->ranges, bucket, pt->n_ranges, wsub_hash(key), &ri))
                r.local = wdir_find(dirs, g.own_cnt + (ri - pt->n_buckets), keys, keys_hi, n_nodes, key);
        } else {
            r.local = dir_find<4096>(dirs, bucket - g.own_lo, keys, n_nodes, lo, &whole);
            if (!whole && lk_range_of(pt->ranges, bucket, pt->n_ranges, sub_hash(lo), &ri))
                r.local = dir_find<4096>(dirs, g.own_cnt + (ri - pt->n_buckets), keys, n_nodes, lo);
        }
        return r;
    }
};

constexpr int LK_TAB16 = LK_MAX_PARTS * (int)(sizeof(LkPart) / 16);

// owner[i] / local[i] of (keys_hi[i], keys[i]); one thread per query.  An absent key sets nothing anywhere else.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_part_lookup(LkPartsFinder<WIDE> f, const uint64_t *__restrict__ keys,
                                                     const uint64_t *__restrict__ keys_hi, uint64_t n, LkMask m, uint8_t *owner,
                                                     uint32_t *local) {
    __shared__ uint4 s_tab[LK_TAB16];
    f.load(s_tab);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t lo = keys[i], hi = keys_hi ? keys_hi[i] : 0ull;
    if (!lk_key_in_range(hi, lo, m)) { owner[i] = 0xFF; local[i] = NO_NODE; return; }
    const LkFound r = f.find(s_tab, hi, lo);
    owner[i] = (uint8_t)r.owner;
    local[i] = r.local;
}

// k_score_sequences over the windows whose k-mer this handle's parts own (ACGT only: a graph in parts has no other
// alphabet).  The body is the one above with two differences: the count comes from the found part's CSR, and a window of
// another rank's k-mer adds nothing and is not missing.  A window that holds a character outside ACGT has no owner: every
// handle records it as missing (the minimum over ranks does not care how many did).  Kept as a kernel of its own: the
// finder's extra state (the LDS table, the part of a found node) would change the code of k_score_sequences.
template <bool WIDE>
__global__ __launch_bounds__(LK_NT) void k_part_score_sequences(LkPartsFinder<WIDE> f, const char *__restrict__ chars,
                                                                uint64_t n_chars, const uint64_t *__restrict__ offsets,
                                                                uint64_t n_seq, const uint8_t *__restrict__ lut,
                                                                unsigned long long *scores, unsigned long long *first_missing) {
    __shared__ uint4 s_tab[LK_TAB16];
    __shared__ uint64_t s_seq[LK_NT];
    __shared__ unsigned long long s_sum[LK_NT], s_miss[LK_NT];
    f.load(s_tab);
    const int k = f.k;
    const uint64_t p0 = ((uint64_t)blockIdx.x * LK_NT + threadIdx.x) * LK_RUN;
    uint64_t seq = ~0ull;
    unsigned long long sum = 0, miss = ~0ull;
    if (p0 + (uint64_t)k < n_chars) {
        uint64_t a = 0, b = n_seq;  // invariant: offsets[a] <= p0 < offsets[b]
        while (b - a > 1) {
            const uint64_t mid = a + ((b - a) >> 1);
            if (offsets[mid] <= p0) a = mid;
            else b = mid;
        }
        seq = a;
        uint64_t seq_beg = offsets[seq], seq_end = offsets[seq + 1];
        const LkMask m = lk_mask(2, k);
        LkWindow w = lk_empty();
        for (int i = 0; i < k; ++i) lk_push(w, lut[(uint8_t)chars[p0 + i]], 2, m);
        const uint64_t p_lim = n_chars - (uint64_t)k, p_end = p0 + (uint64_t)LK_RUN < p_lim ? p0 + (uint64_t)LK_RUN : p_lim;
        for (uint64_t p = p0; p < p_end; ++p) {
            if (p >= seq_end) {  // the next sequence that is not empty
                lk_flush(seq, sum, miss, scores, first_missing);
                sum = 0;
                miss = ~0ull;
                do { ++seq; seq_beg = offsets[seq]; seq_end = offsets[seq + 1]; } while (p >= seq_end);
            }
            const uint8_t code = lut[(uint8_t)chars[p + k]];
            if (p + (uint64_t)k < seq_end) {
                uint32_t c = 0;
                bool mine = true;  // a window with a character outside ACGT is everybody's, and missing
                if (w.run >= (uint32_t)k && code != LK_BAD_CODE) {
                    const LkFound r = f.find(s_tab, w.hi, w.lo);
                    mine = r.part < (uint32_t)LK_MAX_PARTS;
                    if (r.local != NO_NODE) {
                        const LkPart *pt = reinterpret_cast<const LkPart *>(s_tab) + r.part;
                        c = lk_csr_count(pt->flags, pt->row_ptr32, pt->ecnt, r.local, code);
                    }
                }
                if (c) sum += c;
                else if (mine && miss == ~0ull) miss = p - seq_beg;  // positions ascend: the first one is the smallest
            }
            lk_push(w, code, 2, m);
        }
    }
    s_seq[threadIdx.x] = seq;
    s_sum[threadIdx.x] = sum;
    s_miss[threadIdx.x] = miss;
    __syncthreads();
    if (seq != ~0ull && (threadIdx.x == 0 || s_seq[threadIdx.x - 1] != seq)) {  // first thread of a group that ended in `seq`
        for (int t = threadIdx.x + 1; t < LK_NT && s_seq[t] == seq; ++t) {
            sum += s_sum[t];
            if (s_miss[t] < miss) miss = s_miss[t];
        }
        lk_flush(seq, sum, miss, scores, first_missing);
    }
}

}  // namespace dbgk
#endif  // __HIPCC__
