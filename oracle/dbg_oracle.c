/*
 * CPU oracle, C restatement of the graph-construction half of the hot path.
 * TEST INFRASTRUCTURE ONLY: used by tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg; the product never links or loads it.
 *
 * Restates, for the DNA alphabet, what debruijn.py:98-147 (get_graph_from_reads) and
 * debruijn.py:213-222 (edge_count_table) compute:
 *   - for every read with len > k (debruijn.py:126), every window pos in [0, len-k]
 *     is a vertex occurrence; every pos < len-k is an occurrence of the edge
 *     (k-mer, next base);
 *   - per distinct k-mer: the 4 successor counts (the edge_count_table entries
 *     k-mer + base) and the first occurrence, kept as
 *     stamp = (byte offset << 1) | (pos != 0)   [indegree, debruijn.py:134,141-142].
 * Output order is first-occurrence order == the reference's dict order.
 * orc_traverse (below) restates the rest of construct_graph and output_contigs on such a build: pruningEdges, the
 * branch list, tip removal, pull_out_read, the walk in both modes and getScore.
 *
 * Parity status: pinned -- tests/test_oracle_c.py checks it against
 * oracle/dbg_oracle.py, which is itself pinned by the reference's vectors.
 *
 * Base code = (ascii >> 1) & 3 (A=0 C=1 T=2 G=3), same packing as include/dbg.h.
 * Single-threaded, plain C, open-addressing table; k <= 31 in one 64-bit word, 32..63 in unsigned __int128.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef unsigned __int128 orc_u128; /* k in 32..63: a k-mer is up to 126 bits */

typedef struct {
    uint64_t key;
    uint64_t stamp;
    uint32_t cnt[4];
} orc_slot;

typedef struct __attribute__((packed)) { /* 40 bytes, not 48: the largest tables are of this kind */
    orc_u128 key;
    uint64_t stamp;
    uint32_t cnt[4];
} orc_wslot;

/* Bits 63..56 of a table slot's stamp hold the node's successor codes in first-appearance order, 2 bits each (the
 * order of Counter's keys, debruijn.py:159-165 and :215-216); exported stamps are masked to bits 55..0. */
#define ORC_FS_SHIFT 56
#define ORC_STAMP_MASK ((1ULL << ORC_FS_SHIFT) - 1)

typedef struct orc_trav orc_trav; /* traversal state, below */

typedef struct {
    orc_slot *tab;   /* k <= 31 */
    orc_wslot *wtab; /* k >= 32 */
    uint64_t cap, n_nodes, n_kmer_inst, n_edge_inst;
    int k;
    uint32_t *node_slot; /* [n_nodes] table slot of the node in dict order (built by the first orc_traverse) */
    uint32_t *slot_node; /* [cap] dict index of the node in a slot */
    orc_trav *tv;        /* the last orc_traverse */
} orc_t;

static uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}
static uint64_t hash_narrow(uint64_t key) { return mix64(key); }
static uint64_t hash_wide(orc_u128 key) { return mix64((uint64_t)key ^ mix64((uint64_t)(key >> 64) + 0x9E3779B97F4A7C15ULL)); }

static void trav_free(orc_trav *t);

void orc_free(orc_t *o) {
    if (!o) return;
    trav_free(o->tv);
    free(o->node_slot);
    free(o->slot_node);
    free(o->tab);
    free(o->wtab);
    free(o);
}

/* The scan of debruijn.py:126-143 over one key width.  Returns 0, or -1 on a byte outside ACGT. */
#define ORC_DEFINE_SCAN(NAME, KEY_T, SLOT_T, TAB, HASH)                                                     \
    static int NAME(orc_t *o, const char *bases, const uint64_t *offsets, uint64_t n_reads) {               \
        const int k = o->k;                                                                                  \
        const uint64_t mask = o->cap - 1;                                                                    \
        const KEY_T empty = ~(KEY_T)0, kmask = (((KEY_T)1) << (2 * k)) - 1;                                  \
        SLOT_T *tab = o->TAB;                                                                                \
        for (uint64_t r = 0; r < n_reads; ++r) {                                                             \
            const uint64_t beg = offsets[r], len = offsets[r + 1] - beg;                                     \
            if (len <= (uint64_t)k) continue; /* debruijn.py:126 */                                          \
            const unsigned char *s = (const unsigned char *)bases + beg;                                     \
            KEY_T key = 0;                                                                                   \
            for (uint64_t i = 0; i <= len; ++i) {                                                            \
                const unsigned char c = i < len ? s[i] : 0;                                                  \
                if (i < len && c != 'A' && c != 'C' && c != 'G' && c != 'T') return -1;                      \
                if (i >= (uint64_t)k) {                                                                      \
                    /* window [i-k, i) is complete in `key`; s[i] is its successor base (none at i == len) */\
                    const uint64_t pos = i - k;                                                              \
                    uint64_t h = HASH(key) & mask;                                                           \
                    while (tab[h].key != empty && tab[h].key != key) h = (h + 1) & mask;                     \
                    SLOT_T *e = &tab[h];                                                                     \
                    if (e->key == empty) {                                                                   \
                        e->key = key;                                                                        \
                        e->stamp = ((beg + pos) << 1) | (pos != 0);                                          \
                        e->cnt[0] = e->cnt[1] = e->cnt[2] = e->cnt[3] = 0;                                   \
                        o->n_nodes++;                                                                        \
                    }                                                                                        \
                    o->n_kmer_inst++;                                                                        \
                    if (i < len) {                                                                           \
                        const int b = (c >> 1) & 3;                                                          \
                        if (!e->cnt[b]) { /* first appearance of this successor: append its code */          \
                            const int nd = (e->cnt[0] != 0) + (e->cnt[1] != 0) + (e->cnt[2] != 0) + (e->cnt[3] != 0); \
                            e->stamp |= (uint64_t)b << (ORC_FS_SHIFT + 2 * nd);                              \
                        }                                                                                    \
                        e->cnt[b]++; o->n_edge_inst++;                                                       \
                    }                                                                                        \
                }                                                                                            \
                key = ((key << 2) | ((c >> 1) & 3)) & kmask;                                                 \
            }                                                                                                \
        }                                                                                                    \
        return 0;                                                                                            \
    }

ORC_DEFINE_SCAN(scan_narrow, uint64_t, orc_slot, tab, hash_narrow)
ORC_DEFINE_SCAN(scan_wide, orc_u128, orc_wslot, wtab, hash_wide)

/* returns NULL on bad input (k outside 1..63, byte outside ACGT, allocation failure) */
orc_t *orc_build(const char *bases, const uint64_t *offsets, uint64_t n_reads, int k) {
    if (k < 1 || k > 63) return NULL;
    if (n_reads && (offsets[n_reads] >> (ORC_FS_SHIFT - 2))) return NULL; /* stamps must stay below bit 56 */
    uint64_t windows = 0;
    for (uint64_t r = 0; r < n_reads; ++r) {
        uint64_t len = offsets[r + 1] - offsets[r];
        if (len > (uint64_t)k) windows += len - k + 1;
    }
    orc_t *o = (orc_t *)calloc(1, sizeof(orc_t));
    if (!o) return NULL;
    o->k = k;
    o->cap = 1024;   /* load factor at most 0.8 (nodes <= windows); 2x windows would double some tables past 16 GB */
    while (o->cap < windows + windows / 4) o->cap <<= 1;
    int rc;
    if (k <= 31) {
        o->tab = (orc_slot *)malloc(o->cap * sizeof(orc_slot));
        if (!o->tab) { free(o); return NULL; }
        memset(o->tab, 0xFF, o->cap * sizeof(orc_slot));
        rc = scan_narrow(o, bases, offsets, n_reads);
    } else {
        o->wtab = (orc_wslot *)malloc(o->cap * sizeof(orc_wslot));
        if (!o->wtab) { free(o); return NULL; }
        memset(o->wtab, 0xFF, o->cap * sizeof(orc_wslot));
        rc = scan_wide(o, bases, offsets, n_reads);
    }
    if (rc) { orc_free(o); return NULL; }
    return o;
}

uint64_t orc_n_nodes(const orc_t *o) { return o->n_nodes; }
uint64_t orc_n_kmer_instances(const orc_t *o) { return o->n_kmer_inst; }
uint64_t orc_n_edge_instances(const orc_t *o) { return o->n_edge_inst; }

static int cmp_stamp(const void *a, const void *b) {
    const uint64_t x = ((const orc_wslot *)a)->stamp & ORC_STAMP_MASK, y = ((const orc_wslot *)b)->stamp & ORC_STAMP_MASK;
    return x < y ? -1 : x > y;
}

/* nodes in first-occurrence (dict) order; arrays sized orc_n_nodes (counts: n*4, by base code).
 * keys: low 64 bits of the k-mer; keys_hi (may be NULL): bits 64.. (zero for k <= 32). */
int orc_export2(const orc_t *o, uint64_t *keys, uint64_t *keys_hi, uint64_t *stamps, uint32_t *counts) {
    orc_wslot *tmp = (orc_wslot *)malloc((o->n_nodes ? o->n_nodes : 1) * sizeof(orc_wslot));
    if (!tmp) return -1;
    uint64_t n = 0;
    for (uint64_t i = 0; i < o->cap; ++i) {
        if (o->tab && o->tab[i].key != ~0ULL) {
            tmp[n].key = o->tab[i].key;
            tmp[n].stamp = o->tab[i].stamp;
            memcpy(tmp[n].cnt, o->tab[i].cnt, 16);
            ++n;
        } else if (o->wtab && o->wtab[i].key != ~(orc_u128)0) {
            tmp[n++] = o->wtab[i];
        }
    }
    qsort(tmp, n, sizeof(orc_wslot), cmp_stamp);
    for (uint64_t i = 0; i < n; ++i) {
        if (keys) keys[i] = (uint64_t)tmp[i].key;
        if (keys_hi) keys_hi[i] = (uint64_t)(tmp[i].key >> 64);
        if (stamps) stamps[i] = tmp[i].stamp & ORC_STAMP_MASK;
        if (counts) memcpy(counts + 4 * i, tmp[i].cnt, 16);
    }
    free(tmp);
    return 0;
}

int orc_export(const orc_t *o, uint64_t *keys, uint64_t *stamps, uint32_t *counts) {
    return orc_export2(o, keys, NULL, stamps, counts);
}

/* ------------------------------------------------------------------------------------------------------------
 * Traversal: the rest of construct_graph (debruijn.py:150-186, :224-285) and output_contigs (:288-347) on top of
 * an orc_build, single-threaded and iterative.  orc_traverse may be called any number of times on one build (each
 * call replaces the last one's results).  Nodes are numbered in dict order (ascending stamp).
 * ------------------------------------------------------------------------------------------------------------ */
#define ORC_NONE 0xFFFFFFFFu
#define ORC_F_BRANCH 1
#define ORC_F_PULLED 2
#define ORC_TIP_DEPTH 5 /* debruijn.py:246 */

struct orc_trav {
    uint8_t *order;     /* [n_nodes] successor codes by rank, 2 bits each, rank 0 in bits 1:0 */
    uint8_t *keep;      /* [n_nodes] bit b: the successor with code b survives pruningEdges */
    uint8_t *flags;     /* [n_nodes] ORC_F_BRANCH | ORC_F_PULLED */
    uint32_t *branch;   /* branch_kmer, dict order */
    uint32_t *pulled;   /* already_pull_out, append order */
    uint8_t *read_flags;
    uint64_t n_branch, n_pulled, n_reads, n_pull_reads;
    uint32_t *c_start, *c_seq; /* per contig: start node, emission index within the start */
    uint64_t *c_nodes, *c_score, *c_path_off;
    uint32_t *c_path;          /* final mode: the nodes of every contig (c_path_off[i] .. c_path_off[i+1]) */
    uint64_t n_contigs, contig_chars, n_path, cap_contigs, cap_path;
    int final;
};

static void trav_free(orc_trav *t) {
    if (!t) return;
    free(t->order); free(t->keep); free(t->flags); free(t->branch); free(t->pulled); free(t->read_flags);
    free(t->c_start); free(t->c_seq); free(t->c_nodes); free(t->c_score); free(t->c_path_off); free(t->c_path);
    free(t);
}

static orc_u128 node_key(const orc_t *o, uint32_t i) {
    const uint64_t s = o->node_slot[i];
    return o->tab ? (orc_u128)o->tab[s].key : o->wtab[s].key;
}
static uint64_t node_stamp(const orc_t *o, uint32_t i) {
    const uint64_t s = o->node_slot[i];
    return o->tab ? o->tab[s].stamp : o->wtab[s].stamp;
}
static const uint32_t *node_cnt(const orc_t *o, uint32_t i) {
    const uint64_t s = o->node_slot[i];
    /* cnt sits at byte 24 of a packed 40-byte slot: 4-byte aligned, as a uint32_t pointer needs */
    return o->tab ? o->tab[s].cnt : (const uint32_t *)((const char *)(o->wtab + s) + offsetof(orc_wslot, cnt));
}
/* vertices[v].outdegree: distinct successors before pruning (debruijn.py:130-131,135) */
static int node_outdeg(const orc_t *o, uint32_t i) {
    const uint32_t *c = node_cnt(o, i);
    return (c[0] != 0) + (c[1] != 0) + (c[2] != 0) + (c[3] != 0);
}
static uint32_t lookup(const orc_t *o, orc_u128 key) {
    const uint64_t mask = o->cap - 1;
    if (o->tab) {
        const uint64_t kk = (uint64_t)key;
        for (uint64_t h = hash_narrow(kk) & mask; o->tab[h].key != ~0ULL; h = (h + 1) & mask)
            if (o->tab[h].key == kk) return o->slot_node[h];
    } else {
        for (uint64_t h = hash_wide(key) & mask; o->wtab[h].key != ~(orc_u128)0; h = (h + 1) & mask)
            if (o->wtab[h].key == key) return o->slot_node[h];
    }
    return ORC_NONE;
}
static orc_u128 kmask_of(int k) { return (((orc_u128)1) << (2 * k)) - 1; }
static uint32_t succ_of(const orc_t *o, uint32_t i, int b) {
    return lookup(o, ((node_key(o, i) << 2) | (orc_u128)b) & kmask_of(o->k));
}

/* dict order: LSD radix sort of (stamp, slot) pairs, 11 bits a pass */
static int index_nodes(orc_t *o) {
    if (o->node_slot) return 0;
    if (o->cap > 0xFFFFFFFFull) return -1;
    const uint64_t n = o->n_nodes;
    uint64_t *ka = (uint64_t *)malloc((n ? n : 1) * 8), *kb = (uint64_t *)malloc((n ? n : 1) * 8);
    uint32_t *va = (uint32_t *)malloc((n ? n : 1) * 4), *vb = (uint32_t *)malloc((n ? n : 1) * 4);
    o->slot_node = (uint32_t *)malloc(o->cap * 4);
    if (!ka || !kb || !va || !vb || !o->slot_node) { free(ka); free(kb); free(va); free(vb); return -1; }
    uint64_t m = 0, mx = 0;
    for (uint64_t s = 0; s < o->cap; ++s) {
        o->slot_node[s] = ORC_NONE;
        const int used = o->tab ? o->tab[s].key != ~0ULL : o->wtab[s].key != ~(orc_u128)0;
        if (!used) continue;
        ka[m] = (o->tab ? o->tab[s].stamp : o->wtab[s].stamp) & ORC_STAMP_MASK;
        va[m] = (uint32_t)s;
        if (ka[m] > mx) mx = ka[m];
        ++m;
    }
    for (int sh = 0; sh < 64 && (mx >> sh); sh += 11) {
        uint64_t cnt[2048] = {0};
        for (uint64_t i = 0; i < m; ++i) cnt[(ka[i] >> sh) & 2047]++;
        for (uint64_t d = 0, acc = 0; d < 2048; ++d) { const uint64_t c = cnt[d]; cnt[d] = acc; acc += c; }
        for (uint64_t i = 0; i < m; ++i) { const uint64_t j = cnt[(ka[i] >> sh) & 2047]++; kb[j] = ka[i]; vb[j] = va[i]; }
        uint64_t *tk = ka; ka = kb; kb = tk;
        uint32_t *tv = va; va = vb; vb = tv;
    }
    for (uint64_t i = 0; i < m; ++i) o->slot_node[va[i]] = (uint32_t)i;
    free(ka); free(kb); free(vb);
    o->node_slot = va;
    return 0;
}

/* pruningEdges (debruijn.py:150-166): successors ranked by count descending, ties by first appearance
 * (Counter.most_common is a stable sort of Counter's first-seen key order); the first-ranked one always survives,
 * every other one iff count >= max_count / threshold in true (double) division.  Branch list: :230-236. */
static void trav_prune(const orc_t *o, orc_trav *t, double threshold) {
    for (uint64_t i = 0; i < o->n_nodes; ++i) {
        const uint32_t *c = node_cnt(o, (uint32_t)i);
        const uint32_t fs = (uint32_t)(node_stamp(o, (uint32_t)i) >> ORC_FS_SHIFT);
        const int nd = node_outdeg(o, (uint32_t)i);
        int r[4];
        for (int j = 0; j < nd; ++j) {   /* insertion sort, stable: first appearance breaks ties */
            const int b = (fs >> (2 * j)) & 3;
            int p = j;
            while (p > 0 && c[r[p - 1]] < c[b]) { r[p] = r[p - 1]; --p; }
            r[p] = b;
        }
        uint8_t ord = 0, keep = 0;
        for (int j = 0; j < nd; ++j) {
            ord |= (uint8_t)(r[j] << (2 * j));
            if (j == 0 || (double)c[r[j]] >= (double)c[r[0]] / threshold) keep |= (uint8_t)(1u << r[j]);
        }
        t->order[i] = ord;
        t->keep[i] = keep;
        if (__builtin_popcount(keep) > 1) { t->flags[i] |= ORC_F_BRANCH; t->branch[t->n_branch++] = (uint32_t)i; }
    }
}

/* The kept successors of node i, in rank order (the list edges[v] after pruningEdges): rank j -> code, or -1. */
static int kept_code(const orc_t *o, const orc_trav *t, uint32_t i, int j) {
    if (j >= node_outdeg(o, i)) return -1;
    const int b = (t->order[i] >> (2 * j)) & 3;
    return (t->keep[i] >> b) & 1 ? b : -2;
}

/* Tip removal: pruningErrorContigFromBranch (debruijn.py:169-186) driven by :241-254.  Per branch node in dict
 * order, a DFS of depth 5 over the kept successors that are not yet pulled collects every path whose last node has
 * PRE-pruning outdegree 0 (no check for nodes already on the path, as in the reference); then the nodes of those
 * paths, path by path, are appended to already_pull_out unless pulled already or a branch node. */
static int trav_tips(const orc_t *o, orc_trav *t) {
    uint32_t *paths = NULL; /* collected paths, ORC_TIP_DEPTH + 1 words each: length, nodes */
    uint64_t np = 0, capp = 0;
    for (uint64_t bi = 0; bi < t->n_branch; ++bi) {
        const uint32_t root = t->branch[bi];
        if (t->flags[root] & ORC_F_PULLED) continue; /* :245, never true */
        np = 0;
        uint32_t node[ORC_TIP_DEPTH];
        int rank[ORC_TIP_DEPTH], depth = 1;
        node[0] = root; rank[0] = 0;
        /* the root is a branch node: outdegree >= 2, so [root] itself is never a path (:172) */
        while (depth > 0) {
            const uint32_t v = node[depth - 1];
            int b = -1;
            while (rank[depth - 1] < 4) {
                b = kept_code(o, t, v, rank[depth - 1]++);
                if (b != -2) break;
            }
            if (b < 0) { --depth; continue; }
            const uint32_t s = succ_of(o, v, b);
            if (s == ORC_NONE) { free(paths); return -4; }
            if (t->flags[s] & ORC_F_PULLED) continue;  /* :184 */
            if (depth >= ORC_TIP_DEPTH) continue;      /* the call with depth == 0 returns at once (:170) */
            if (node_outdeg(o, s) == 0) {              /* :172-176 */
                if (np == capp) {
                    capp = capp ? capp * 2 : 64;
                    uint32_t *q = (uint32_t *)realloc(paths, capp * (ORC_TIP_DEPTH + 1) * 4);
                    if (!q) { free(paths); return -1; }
                    paths = q;
                }
                uint32_t *p = paths + np++ * (ORC_TIP_DEPTH + 1);
                p[0] = (uint32_t)depth + 1;
                for (int d = 0; d < depth; ++d) p[1 + d] = node[d];
                p[1 + depth] = s;
                continue;
            }
            node[depth] = s; rank[depth] = 0; ++depth;
        }
        /* every path is distinct (successor lists hold no duplicates), so `vec not in output` (:173) drops nothing */
        for (uint64_t q = 0; q < np; ++q) {
            const uint32_t *p = paths + q * (ORC_TIP_DEPTH + 1);
            for (uint32_t d = 0; d < p[0]; ++d) {
                const uint32_t x = p[1 + d];
                if (t->flags[x] & (ORC_F_PULLED | ORC_F_BRANCH)) continue; /* :250-251 */
                t->flags[x] |= ORC_F_PULLED;
                t->pulled[t->n_pulled++] = x;
            }
        }
    }
    free(paths);
    return 0;
}

/* pull_out_read (debruijn.py:274-278): a read is pulled out iff one of its k-length windows is a branch k-mer --
 * a read of length exactly k has one window, a shorter one none. */
static void trav_pull_reads(const orc_t *o, orc_trav *t, const char *bases, const uint64_t *offsets) {
    const int k = o->k;
    const orc_u128 km = kmask_of(k);
    for (uint64_t r = 0; r < t->n_reads; ++r) {
        const uint64_t beg = offsets[r], len = offsets[r + 1] - beg;
        const unsigned char *s = (const unsigned char *)bases + beg;
        orc_u128 key = 0;
        uint8_t hit = 0;
        for (uint64_t i = 0; i < len && !hit; ++i) {
            key = ((key << 2) | ((s[i] >> 1) & 3)) & km;
            if (i + 1 >= (uint64_t)k && t->n_branch) {
                const uint32_t v = lookup(o, key);
                hit = v != ORC_NONE && (t->flags[v] & ORC_F_BRANCH);
            }
        }
        t->read_flags[r] = hit;
        t->n_pull_reads += hit;
    }
}

static int push_contig(const orc_t *o, orc_trav *t, uint32_t start, uint32_t seq, uint64_t nodes, uint64_t score) {
    if (t->n_contigs == t->cap_contigs) {
        const uint64_t nc = t->cap_contigs ? t->cap_contigs * 2 : 1024;
        uint32_t *a = (uint32_t *)realloc(t->c_start, nc * 4);
        if (a) t->c_start = a;
        uint32_t *b = (uint32_t *)realloc(t->c_seq, nc * 4);
        if (b) t->c_seq = b;
        uint64_t *c = (uint64_t *)realloc(t->c_nodes, nc * 8);
        if (c) t->c_nodes = c;
        uint64_t *d = (uint64_t *)realloc(t->c_score, nc * 8);
        if (d) t->c_score = d;
        uint64_t *e = (uint64_t *)realloc(t->c_path_off, (nc + 1) * 8);
        if (e) t->c_path_off = e;
        if (!a || !b || !c || !d || !e) return -1;
        if (!t->n_contigs) t->c_path_off[0] = 0;
        t->cap_contigs = nc;
    }
    const uint64_t i = t->n_contigs++;
    t->c_start[i] = start; t->c_seq[i] = seq; t->c_nodes[i] = nodes; t->c_score[i] = score;
    t->c_path_off[i + 1] = t->n_path;
    t->contig_chars += (uint64_t)o->k + nodes - 1;
    return 0;
}

/* Non-final output_contigs (debruijn.py:288-347 with branch_kmer): outside branch and pulled nodes every node keeps
 * at most one successor, so the DFS from a start is one chain.  It ends at a branch node or a node without kept
 * successors (emitted with it, :304-313), just before a pulled node (:292-303; nothing if the start is pulled), or at
 * a node already on the chain (:289; no contig).  Each node's chain end, node count and score (getScore,
 * II_assembleFromReads.py:14-18: the edge_count_table entries of the path's edges) is resolved once and memoised. */
static int trav_walk_chains(const orc_t *o, orc_trav *t) {
    const uint64_t n = o->n_nodes;
    uint8_t *st = (uint8_t *)calloc(n ? n : 1, 1);       /* 0 open, 1 on the stack, 2 ends, 3 runs into a cycle */
    uint64_t *len = (uint64_t *)malloc((n ? n : 1) * 8), *sc = (uint64_t *)malloc((n ? n : 1) * 8);
    uint32_t *stk = NULL;
    uint64_t cap = 0;
    if (!st || !len || !sc) { free(st); free(len); free(sc); return -1; }
    int rc = 0;
    for (uint32_t s = 0; s < n && !rc; ++s) {
        if (node_stamp(o, s) & 1) continue;              /* starts: indegree 0 (:330-334) */
        if (t->flags[s] & ORC_F_PULLED) continue;
        uint64_t sp = 0;
        uint32_t v = s;
        uint8_t end = 0;
        for (;;) {
            if (st[v] >= 2) { end = st[v]; break; }
            if (st[v] == 1) { end = 3; break; }          /* v is on this chain: a cycle */
            if (sp == cap) {
                cap = cap ? cap * 2 : 4096;
                uint32_t *q = (uint32_t *)realloc(stk, cap * 4);
                if (!q) { rc = -1; break; }
                stk = q;
            }
            stk[sp++] = v;
            st[v] = 1;
            const int b = (t->flags[v] & ORC_F_BRANCH) ? -1 : kept_code(o, t, v, 0);
            const uint32_t nx = b < 0 ? ORC_NONE : succ_of(o, v, b);
            if (b >= 0 && nx == ORC_NONE) { rc = -4; break; }
            if (b < 0 || (t->flags[nx] & ORC_F_PULLED)) { /* the chain ends at v */
                st[v] = 2; len[v] = 1; sc[v] = 0; --sp; end = 2; break;
            }
            v = nx;
        }
        if (rc) break;
        while (sp) {                                     /* unwind: each node takes its successor's result */
            const uint32_t u = stk[--sp];
            st[u] = end;
            if (end == 2) {
                const int b = kept_code(o, t, u, 0);
                const uint32_t nx = succ_of(o, u, b);
                len[u] = len[nx] + 1;
                sc[u] = sc[nx] + node_cnt(o, u)[b];
            }
        }
        if (st[s] == 2) rc = push_contig(o, t, s, 0, len[s], sc[s]);
    }
    free(st); free(len); free(sc); free(stk);
    return rc;
}

static int push_path(orc_trav *t, const uint32_t *path, uint64_t np) {
    if (t->n_path + np > t->cap_path) {
        uint64_t nc = t->cap_path ? t->cap_path : 4096;
        while (nc < t->n_path + np) nc *= 2;
        uint32_t *q = (uint32_t *)realloc(t->c_path, nc * 4);
        if (!q) return -1;
        t->c_path = q; t->cap_path = nc;
    }
    memcpy(t->c_path + t->n_path, path, np * 4);
    t->n_path += np;
    return 0;
}

/* Final output_contigs (branch_kmer == [], debruijn.py:281-283): DFS (:288-316) from every start over the kept
 * successors in rank order, emitting every simple path that ends at a node without kept successors or just before a
 * pulled node.  `vec not in output` (:297,:305) only ever drops the second emission of one path, which happens when a
 * node has several pulled successors: one flag per stack frame.  Returns -2 once more than max_paths paths were
 * emitted, -5 once more than 64 * max_paths + 2^20 DFS steps were taken (simple paths that emit nothing). */
static int trav_walk_final(const orc_t *o, orc_trav *t, uint64_t max_paths) {
    const uint64_t n = o->n_nodes;
    uint8_t *onp = (uint8_t *)calloc(n ? n : 1, 1);
    uint32_t *path = NULL;
    int *rank = NULL;
    uint8_t *emitted = NULL;
    uint64_t cap = 0, steps = 0, max_steps = 64 * max_paths + (1u << 20);
    if (!onp) return -1;
    int rc = 0;
    for (uint32_t s = 0; s < n && !rc; ++s) {
        if (node_stamp(o, s) & 1) continue;
        if (t->flags[s] & ORC_F_PULLED) continue;   /* :292-295, len(vec) == 1 */
        uint32_t seq = 0;
        uint64_t depth = 0;
        uint32_t x = s;
        for (;;) {                                   /* enter x (a child of path[depth-1], or the start) */
            if (++steps > max_steps) { rc = -5; break; }
            if (onp[x]) {
                /* :289 */
            } else if (t->flags[x] & ORC_F_PULLED) {
                if (!emitted[depth - 1]) {
                    emitted[depth - 1] = 1;
                    uint64_t score = 0;
                    for (uint64_t d = 0; d + 1 < depth; ++d)
                        score += node_cnt(o, path[d])[(uint32_t)(node_key(o, path[d + 1]) & 3)];
                    if (t->n_contigs >= max_paths) { rc = -2; break; }
                    if ((rc = push_path(t, path, depth)) || (rc = push_contig(o, t, s, seq++, depth, score))) break;
                }
            } else {
                if (depth == cap) {
                    cap = cap ? cap * 2 : 1024;
                    uint32_t *p = (uint32_t *)realloc(path, cap * 4);
                    if (p) path = p;
                    int *r = (int *)realloc(rank, cap * sizeof(int));
                    if (r) rank = r;
                    uint8_t *e = (uint8_t *)realloc(emitted, cap);
                    if (e) emitted = e;
                    if (!p || !r || !e) { rc = -1; break; }
                }
                path[depth] = x; rank[depth] = 0; emitted[depth] = 0; ++depth;
                if (kept_code(o, t, x, 0) < 0) {        /* len(E[current]) == 0 (:304-313) */
                    uint64_t score = 0;
                    for (uint64_t d = 0; d + 1 < depth; ++d)
                        score += node_cnt(o, path[d])[(uint32_t)(node_key(o, path[d + 1]) & 3)];
                    if (t->n_contigs >= max_paths) { rc = -2; break; }
                    if ((rc = push_path(t, path, depth)) || (rc = push_contig(o, t, s, seq++, depth, score))) break;
                    --depth;
                } else {
                    onp[x] = 1;                         /* descend: its successors are tried next */
                }
            }
            /* next child of the deepest open frame, popping exhausted frames */
            int found = 0;
            while (depth > 0) {
                const uint32_t v = path[depth - 1];
                int b = -1;
                while (rank[depth - 1] < 4) {
                    b = kept_code(o, t, v, rank[depth - 1]++);
                    if (b != -2) break;
                }
                if (b >= 0) {
                    x = succ_of(o, v, b);
                    if (x == ORC_NONE) { rc = -4; break; }
                    found = 1;
                    break;
                }
                onp[v] = 0;
                --depth;
            }
            if (rc || !found) break;
        }
    }
    free(onp); free(path); free(rank); free(emitted);
    return rc;
}

/* Runs prune, branch list, tip removal, pull-out reads and the walk of one build.  bases / offsets: the reads the
 * build was made from.  out6 (may be NULL): n_branch, n_pulled, n_pull_reads, n_contigs, contig_chars, n_nodes.
 * 0, or -1 allocation failure, -2 the final walk's path cap was passed, -3 bad argument, -4 inconsistent build,
 * -5 the final walk's step cap (64 * max_paths + 2^20) was passed. */
int orc_traverse(orc_t *o, const char *bases, const uint64_t *offsets, uint64_t n_reads, double threshold, int final,
                 uint64_t max_paths, uint64_t *out6) {
    if (!o || !(threshold > 0)) return -3;
    trav_free(o->tv);
    o->tv = NULL;
    if (index_nodes(o)) return -1;
    orc_trav *t = (orc_trav *)calloc(1, sizeof(orc_trav));
    if (!t) return -1;
    o->tv = t;
    const uint64_t n = o->n_nodes ? o->n_nodes : 1;
    t->final = final;
    t->n_reads = n_reads;
    t->order = (uint8_t *)calloc(n, 1);
    t->keep = (uint8_t *)calloc(n, 1);
    t->flags = (uint8_t *)calloc(n, 1);
    t->branch = (uint32_t *)malloc(n * 4);
    t->pulled = (uint32_t *)malloc(n * 4);
    t->read_flags = (uint8_t *)malloc(n_reads ? n_reads : 1);
    if (!t->order || !t->keep || !t->flags || !t->branch || !t->pulled || !t->read_flags) return -1;
    trav_prune(o, t, threshold);
    int rc = trav_tips(o, t);
    if (rc) return rc;
    trav_pull_reads(o, t, bases, offsets);
    rc = final ? trav_walk_final(o, t, max_paths) : trav_walk_chains(o, t);
    if (rc) return rc;
    if (out6) {
        out6[0] = t->n_branch; out6[1] = t->n_pulled; out6[2] = t->n_pull_reads;
        out6[3] = t->n_contigs; out6[4] = t->contig_chars; out6[5] = o->n_nodes;
    }
    return 0;
}

/* Numbers the nodes in dict order (done by orc_traverse too); 0 or -1. */
int orc_index(orc_t *o) { return index_nodes(o); }

/* nodes [lo, hi) in dict order, as orc_export2 exports them, without its temporary copy of the table (after orc_index) */
int orc_export_range(const orc_t *o, uint64_t lo, uint64_t hi, uint64_t *keys, uint64_t *keys_hi, uint64_t *stamps,
                     uint32_t *counts) {
    if (!o->node_slot || lo > hi || hi > o->n_nodes) return -3;
    for (uint64_t i = lo; i < hi; ++i) {
        const orc_u128 key = node_key(o, (uint32_t)i);
        if (keys) keys[i - lo] = (uint64_t)key;
        if (keys_hi) keys_hi[i - lo] = (uint64_t)(key >> 64);
        if (stamps) stamps[i - lo] = node_stamp(o, (uint32_t)i) & ORC_STAMP_MASK;
        if (counts) memcpy(counts + 4 * (i - lo), node_cnt(o, (uint32_t)i), 16);
    }
    return 0;
}

/* per node in dict order (NULL skipped): rank order byte, keep mask, flags (1 branch, 2 pulled) */
int orc_trav_nodes(const orc_t *o, uint8_t *order, uint8_t *keep, uint8_t *flags) {
    const orc_trav *t = o->tv;
    if (!t) return -3;
    if (order) memcpy(order, t->order, o->n_nodes);
    if (keep) memcpy(keep, t->keep, o->n_nodes);
    if (flags) memcpy(flags, t->flags, o->n_nodes);
    return 0;
}

/* branch[n_branch] (dict order), pulled[n_pulled] (append order): dict indices; read_flags[n_reads] */
int orc_trav_lists(const orc_t *o, uint32_t *branch, uint32_t *pulled, uint8_t *read_flags) {
    const orc_trav *t = o->tv;
    if (!t) return -3;
    if (branch) memcpy(branch, t->branch, t->n_branch * 4);
    if (pulled) memcpy(pulled, t->pulled, t->n_pulled * 4);
    if (read_flags) memcpy(read_flags, t->read_flags, t->n_reads);
    return 0;
}

/* per contig in emission order: start node's stamp, emission index within the start, characters, score */
int orc_trav_contigs(const orc_t *o, uint64_t *start_stamp, uint32_t *seq, uint64_t *chars, uint64_t *score) {
    const orc_trav *t = o->tv;
    if (!t) return -3;
    for (uint64_t i = 0; i < t->n_contigs; ++i) {
        if (start_stamp) start_stamp[i] = node_stamp(o, t->c_start[i]) & ORC_STAMP_MASK;
        if (seq) seq[i] = t->c_seq[i];
        if (chars) chars[i] = (uint64_t)o->k + t->c_nodes[i] - 1;
        if (score) score[i] = t->c_score[i];
    }
    return 0;
}

static const char ORC_CODE_CHAR[4] = {'A', 'C', 'T', 'G'};

/* Spells contigs idx[0..n) one after another into buf (the text of contig idx[j] starts at off[j], off[n] = total;
 * off is filled in; buf == NULL: off only).  The first node's k-mer, then the last base of every further node. */
int orc_trav_spell(const orc_t *o, const uint64_t *idx, uint64_t n, char *buf, uint64_t *off) {
    const orc_trav *t = o->tv;
    if (!t) return -3;
    const int k = o->k;
    uint64_t pos = 0;
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t i = idx[j];
        if (i >= t->n_contigs) return -3;
        off[j] = pos;
        const uint64_t chars = (uint64_t)k + t->c_nodes[i] - 1;
        if (buf) {
            uint32_t v = t->c_start[i];
            const orc_u128 key = node_key(o, v);
            for (int p = 0; p < k; ++p) buf[pos + p] = ORC_CODE_CHAR[(int)(key >> (2 * (k - 1 - p))) & 3];
            for (uint64_t d = 1; d < t->c_nodes[i]; ++d) {
                if (t->final) {
                    v = t->c_path[t->c_path_off[i] + d];
                } else {
                    const int b = kept_code(o, t, v, 0);
                    v = succ_of(o, v, b);
                }
                buf[pos + k - 1 + d] = ORC_CODE_CHAR[(int)(node_key(o, v) & 3)];
            }
        }
        pos += chars;
    }
    off[n] = pos;
    return 0;
}

/* ------------------------------------------------------------------------------------------------------------
 * Multi-threaded variant of the same scan (k <= 31): the CPU baseline of bench.py on ALL host cores.
 * Hash-partitioned: thread t owns the k-mers whose hash falls into its slice, scans every read, rolls every window
 * (a shift and an or) and inserts only its own -- no locks, no atomics, nothing shared but the read-only input; each
 * thread's table grows by doubling.  Same per-node results as orc_build (tests/test_oracle_c.py compares the digest).
 * out[0] nodes, out[1] distinct edges, out[2] k-mer instances, out[3] edge instances,
 * out[4] digest = sum over nodes of mix64(key ^ mix64(stamp) ^ mix64(cnt0 + 3 cnt1 + 5 cnt2 + 7 cnt3 + 1)).
 * ------------------------------------------------------------------------------------------------------------ */
#include <pthread.h>

typedef struct {
    const char *bases;
    const uint64_t *offsets;
    uint64_t n_reads;
    int k, t, n_threads, rc;
    uint64_t out[5];
} orc_mt_job;

static uint64_t orc_node_digest(uint64_t key, uint64_t stamp, const uint32_t *cnt) {
    return mix64(key ^ mix64(stamp) ^ mix64((uint64_t)cnt[0] + 3ull * cnt[1] + 5ull * cnt[2] + 7ull * cnt[3] + 1));
}

static orc_slot *mt_find(orc_slot **ptab, uint64_t *pcap, uint64_t *pn, uint64_t key, uint64_t h) {
    if ((*pn + 1) * 2 > *pcap) { /* grow: rehash into twice the slots */
        const uint64_t ncap = *pcap * 2;
        orc_slot *nt = (orc_slot *)malloc(ncap * sizeof(orc_slot));
        if (!nt) return NULL;
        memset(nt, 0xFF, ncap * sizeof(orc_slot));
        for (uint64_t i = 0; i < *pcap; ++i) {
            if ((*ptab)[i].key == ~0ULL) continue;
            uint64_t j = hash_narrow((*ptab)[i].key) & (ncap - 1);
            while (nt[j].key != ~0ULL) j = (j + 1) & (ncap - 1);
            nt[j] = (*ptab)[i];
        }
        free(*ptab);
        *ptab = nt;
        *pcap = ncap;
    }
    const uint64_t mask = *pcap - 1;
    uint64_t j = h & mask;
    while ((*ptab)[j].key != ~0ULL && (*ptab)[j].key != key) j = (j + 1) & mask;
    return &(*ptab)[j];
}

static void *mt_worker(void *arg) {
    orc_mt_job *jb = (orc_mt_job *)arg;
    const int k = jb->k;
    const uint64_t kmask = (k == 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
    uint64_t cap = 1 << 16, n = 0, n_inst = 0, n_einst = 0;
    orc_slot *tab = (orc_slot *)malloc(cap * sizeof(orc_slot));
    if (!tab) { jb->rc = -2; return NULL; }
    memset(tab, 0xFF, cap * sizeof(orc_slot));
    const uint64_t T = (uint64_t)jb->n_threads, me = (uint64_t)jb->t;
    for (uint64_t r = 0; r < jb->n_reads; ++r) {
        const uint64_t beg = jb->offsets[r], len = jb->offsets[r + 1] - beg;
        if (len <= (uint64_t)k) continue; /* debruijn.py:126 */
        const unsigned char *s = (const unsigned char *)jb->bases + beg;
        uint64_t key = 0;
        for (uint64_t i = 0; i <= len; ++i) {
            const unsigned char c = i < len ? s[i] : 0;
            if (i < len && c != 'A' && c != 'C' && c != 'G' && c != 'T') { jb->rc = -1; free(tab); return NULL; }
            if (i >= (uint64_t)k) {
                const uint64_t h = hash_narrow(key);
                if ((((h >> 32) * T) >> 32) == me) { /* this thread's slice of the key space */
                    const uint64_t pos = i - k;
                    orc_slot *e = mt_find(&tab, &cap, &n, key, h);
                    if (!e) { jb->rc = -2; free(tab); return NULL; }
                    if (e->key == ~0ULL) {
                        e->key = key;
                        e->stamp = ((beg + pos) << 1) | (pos != 0);
                        e->cnt[0] = e->cnt[1] = e->cnt[2] = e->cnt[3] = 0;
                        ++n;
                    }
                    ++n_inst;
                    if (i < len) { e->cnt[(c >> 1) & 3]++; ++n_einst; }
                }
            }
            key = ((key << 2) | ((c >> 1) & 3)) & kmask;
        }
    }
    uint64_t edges = 0, dig = 0;
    for (uint64_t i = 0; i < cap; ++i) {
        if (tab[i].key == ~0ULL) continue;
        for (int b = 0; b < 4; ++b) edges += tab[i].cnt[b] != 0;
        dig += orc_node_digest(tab[i].key, tab[i].stamp, tab[i].cnt);
    }
    free(tab);
    jb->out[0] = n; jb->out[1] = edges; jb->out[2] = n_inst; jb->out[3] = n_einst; jb->out[4] = dig;
    return NULL;
}

/* 0 on success, -1 byte outside ACGT, -2 allocation or thread failure, -3 bad argument */
int orc_build_mt(const char *bases, const uint64_t *offsets, uint64_t n_reads, int k, int n_threads, uint64_t *out5) {
    if (k < 1 || k > 31 || n_threads < 1 || n_threads > 4096 || !out5) return -3;
    orc_mt_job *jobs = (orc_mt_job *)calloc((size_t)n_threads, sizeof(orc_mt_job));
    pthread_t *th = (pthread_t *)calloc((size_t)n_threads, sizeof(pthread_t));
    if (!jobs || !th) { free(jobs); free(th); return -2; }
    int rc = 0, started = 0;
    for (int t = 0; t < n_threads; ++t) {
        jobs[t].bases = bases; jobs[t].offsets = offsets; jobs[t].n_reads = n_reads;
        jobs[t].k = k; jobs[t].t = t; jobs[t].n_threads = n_threads;
        if (pthread_create(&th[t], NULL, mt_worker, &jobs[t])) { rc = -2; break; }
        ++started;
    }
    for (int t = 0; t < started; ++t) pthread_join(th[t], NULL);
    for (int i = 0; i < 5; ++i) out5[i] = 0;
    for (int t = 0; t < started; ++t) {
        if (jobs[t].rc && !rc) rc = jobs[t].rc;
        for (int i = 0; i < 5; ++i) out5[i] += jobs[t].out[i];
    }
    free(jobs);
    free(th);
    return rc;
}

/* ------------------------------------------------------------------------------------------------------------
 * The same multi-threaded build with the k-mers partitioned ONCE (what a tuned CPU builder does; orc_build_mt above
 * lets every thread roll and hash every window and keep 1/T of them).  Phase 1: thread t scans ITS share of the reads
 * and appends every window as (key, stamp | next base) to the list of the thread that owns the key's hash slice.
 * Phase 2: thread d builds its table from the T lists addressed to it, in reader order (ascending positions: the first
 * instance inserts the first-occurrence stamp).  Same slices, same per-node results, same digest as orc_build_mt.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct { uint64_t key, meta; } orc_tuple;   /* meta: stamp | (next base code + 1) << 61, 0 in the top bits = no successor */
typedef struct { orc_tuple *p; uint64_t n, cap; } orc_vec;
typedef struct {
    const char *bases;
    const uint64_t *offsets;
    uint64_t r_beg, r_end;
    int k, t, n_threads, rc;
    orc_vec *lists;   /* [n_threads][n_threads]: lists[t * T + d] = what reader t found for owner d */
    uint64_t out[5];
} orc_p_job;

static int vec_push(orc_vec *v, uint64_t key, uint64_t meta) {
    if (v->n == v->cap) {
        const uint64_t nc = v->cap ? v->cap * 2 : 4096;
        orc_tuple *np = (orc_tuple *)realloc(v->p, nc * sizeof(orc_tuple));
        if (!np) return -1;
        v->p = np; v->cap = nc;
    }
    v->p[v->n].key = key; v->p[v->n].meta = meta; ++v->n;
    return 0;
}

static void *p_scan(void *arg) {
    orc_p_job *jb = (orc_p_job *)arg;
    const int k = jb->k;
    const uint64_t kmask = (k == 32) ? ~0ULL : ((1ULL << (2 * k)) - 1), T = (uint64_t)jb->n_threads;
    orc_vec *mine = jb->lists + (uint64_t)jb->t * T;
    for (uint64_t r = jb->r_beg; r < jb->r_end; ++r) {
        const uint64_t beg = jb->offsets[r], len = jb->offsets[r + 1] - beg;
        if (len <= (uint64_t)k) continue; /* debruijn.py:126 */
        const unsigned char *s = (const unsigned char *)jb->bases + beg;
        uint64_t key = 0;
        for (uint64_t i = 0; i <= len; ++i) {
            const unsigned char c = i < len ? s[i] : 0;
            if (i < len && c != 'A' && c != 'C' && c != 'G' && c != 'T') { jb->rc = -1; return NULL; }
            if (i >= (uint64_t)k) {
                const uint64_t h = hash_narrow(key), pos = i - k;
                const uint64_t d = ((h >> 32) * T) >> 32;
                const uint64_t stamp = ((beg + pos) << 1) | (pos != 0);
                if (stamp >> 61) { jb->rc = -3; return NULL; }
                if (vec_push(&mine[d], key, stamp | (i < len ? (uint64_t)(((c >> 1) & 3) + 1) << 61 : 0))) { jb->rc = -2; return NULL; }
            }
            key = ((key << 2) | ((c >> 1) & 3)) & kmask;
        }
    }
    return NULL;
}

static void *p_build(void *arg) {
    orc_p_job *jb = (orc_p_job *)arg;
    const uint64_t T = (uint64_t)jb->n_threads, me = (uint64_t)jb->t;
    uint64_t cap = 1 << 16, n = 0, n_inst = 0, n_einst = 0;
    orc_slot *tab = (orc_slot *)malloc(cap * sizeof(orc_slot));
    if (!tab) { jb->rc = -2; return NULL; }
    memset(tab, 0xFF, cap * sizeof(orc_slot));
    for (uint64_t t = 0; t < T; ++t) {
        orc_vec *v = jb->lists + t * T + me;
        for (uint64_t q = 0; q < v->n; ++q) {
            const uint64_t key = v->p[q].key, meta = v->p[q].meta;
            orc_slot *e = mt_find(&tab, &cap, &n, key, hash_narrow(key));
            if (!e) { jb->rc = -2; free(tab); return NULL; }
            if (e->key == ~0ULL) {
                e->key = key;
                e->stamp = meta & ((1ULL << 61) - 1);
                e->cnt[0] = e->cnt[1] = e->cnt[2] = e->cnt[3] = 0;
                ++n;
            }
            ++n_inst;
            if (meta >> 61) { e->cnt[(meta >> 61) - 1]++; ++n_einst; }
        }
        free(v->p); v->p = NULL; v->n = v->cap = 0;   /* consumed: only this thread reads list (t, me) */
    }
    uint64_t edges = 0, dig = 0;
    for (uint64_t i = 0; i < cap; ++i) {
        if (tab[i].key == ~0ULL) continue;
        for (int b = 0; b < 4; ++b) edges += tab[i].cnt[b] != 0;
        dig += orc_node_digest(tab[i].key, tab[i].stamp, tab[i].cnt);
    }
    free(tab);
    jb->out[0] = n; jb->out[1] = edges; jb->out[2] = n_inst; jb->out[3] = n_einst; jb->out[4] = dig;
    return NULL;
}

/* as orc_build_mt; 16 bytes of list per k-mer instance are held between the phases */
int orc_build_mt_partitioned(const char *bases, const uint64_t *offsets, uint64_t n_reads, int k, int n_threads, uint64_t *out5) {
    if (k < 1 || k > 31 || n_threads < 1 || n_threads > 1024 || !out5) return -3;
    const uint64_t T = (uint64_t)n_threads;
    orc_p_job *jobs = (orc_p_job *)calloc(T, sizeof(orc_p_job));
    pthread_t *th = (pthread_t *)calloc(T, sizeof(pthread_t));
    orc_vec *lists = (orc_vec *)calloc(T * T, sizeof(orc_vec));
    int rc = 0;
    if (!jobs || !th || !lists) rc = -2;
    for (int phase = 0; phase < 2 && !rc; ++phase) {
        int started = 0;
        for (uint64_t t = 0; t < T; ++t) {
            jobs[t].bases = bases; jobs[t].offsets = offsets; jobs[t].k = k; jobs[t].t = (int)t; jobs[t].n_threads = n_threads;
            jobs[t].r_beg = n_reads * t / T; jobs[t].r_end = n_reads * (t + 1) / T; jobs[t].lists = lists;
            if (pthread_create(&th[t], NULL, phase ? p_build : p_scan, &jobs[t])) { rc = -2; break; }
            ++started;
        }
        for (int t = 0; t < started; ++t) pthread_join(th[t], NULL);
        for (uint64_t t = 0; t < T && !rc; ++t) rc = jobs[t].rc;
    }
    for (int i = 0; i < 5; ++i) out5[i] = 0;
    if (!rc) for (uint64_t t = 0; t < T; ++t) for (int i = 0; i < 5; ++i) out5[i] += jobs[t].out[i];
    if (lists) for (uint64_t i = 0; i < T * T; ++i) free(lists[i].p);
    free(lists); free(jobs); free(th);
    return rc;
}
