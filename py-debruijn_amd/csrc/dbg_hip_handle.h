// The handle and its arena: the slot enums, the DBG_* build defaults, struct dbg, ShardState, buf_ensure / buf_free /
// pool_trim, HIPCHK / CHK, dev_alloc / dev_free, grid_for, Timer.
// A section of the one translation unit dbg_hip.hip, not self-contained: it needs the system includes, include/dbg.h, every
// kernel header (Slot, SkGeom, FW_DEFAULT_STEPS, DBG_EXW_WAVES) and `using namespace dbgk` in front of it.

// Slots of the arena h->ar_misc: one meaning each, in every build path of the super-k-mer engines
enum MiscSlot {
    MISC_SEGMENTS,      // segment table: what the extraction wrote, or the (bucket, sender) segments a shard received
    MISC_L1_CHILDREN,   // children of multisplit level 1 (start, count)
    MISC_MS_SCPRE,      // multisplit_level's scratch: super-chunk prefix,
    MISC_MS_CMAT,       // ... count matrix (a pre-split extraction writes level 1's itself),
    MISC_MS_OFFS,       // ... scanned offsets
    MISC_BUCKETS,       // final buckets (start, count)
    MISC_RANGES,        // SkRange per bucket and per hash sub-range
    MISC_QUERY_SEGS,    // segments of the cross-bucket queries' owner / target split
    MISC_ESTIMATE_SET,  // hash set of the distinct-k-mer estimate
    MISC_SLOTS
};

// The other arenas of the handle, named the same way.  An enumerator written `B = A` is a second meaning of slot A; its
// comment says why the two are never live together.  Aliases go AFTER the *_SLOTS / *_COLS counter: a real slot added
// behind an alias would continue from the alias' value and leave the count wrong.

// h->ar_node: the node arrays of every engine but the small-k global table, which allocates its own (nodes_in_arena)
enum NodeSlot {
    NODE_KEYS,      // k-mer of every node, low word for k > 31 (d_keys): every engine that builds into the arena
    NODE_STAMPS64,  // 64-bit first-occurrence stamps (d_stamps): written by a build that stamps in 64 bits, else by ensure_dense
    NODE_CNT,       // successor counters, 4 x 32 bits per node (d_cnt): the global wide engine (one GPU or a shard), ensure_dense
    NODE_FLAGS,     // one flag byte per node (d_flags): every engine
    NODE_ORDER,     // successor codes by rank, one byte per node (d_order): as NODE_CNT, and dbg_import_graph
    NODE_SUCC,      // successor ids, 4 per node (d_succ): as NODE_CNT, and dbg_import_graph for k > 31
    NODE_DEG,       // distinct successors per node (d_deg): the global wide engine (one GPU or a shard), dbg_import_graph
    NODE_STAMPS32,  // 32-bit stamps of an LDS-engine build of reads below 2 GiB (d_stamps_st); ensure_dense widens them into NODE_STAMPS64
    NODE_SLOTS
};

// h->ar_csr: the CSR over distinct edges
enum CsrSlot {
    CSR_ROWPTR64,  // 64-bit row pointers (d_rowptr): finish_graph, ensure_dense
    CSR_COL,       // successor node of every edge (d_col): finish_graph or the LDS engines' count kernel
    CSR_ECNT,      // count of every edge (d_ecnt): as CSR_COL
    CSR_ROWPTR32,  // 32-bit row pointers the LDS engines write in the build (d_rowptr32)
    CSR_SLOTS
};

// h->ar_rec[set][column], h->ar_q[set][column]: the two sets a multisplit level reads from and writes to in turn
enum PingPong {
    SET_PING,  // records: what the extraction wrote (or a receiver copied in) and what level 2 writes; queries: as the count kernel wrote them
    SET_PONG,  // records: what levels 1 and 3 write -- the level-1 split of a multi-pass build stays parked here for its passes; queries: grouped by owner shard or by target
    PINGPONG_SETS
};
constexpr int SHARD_EXTRACT_PARTS = 4;  // most parts dbg_shard_extract_part cuts a rank's records into: one set of h->ar_part buffers each
// column of h->ar_rec[set] and of h->ar_part[part]: super-k-mer records as three parallel arrays
enum RecCol {
    REC_W0,              // record word 0: sk_extract / wsk_extract and every multisplit level (shard_extract_wide: low key word of an instance tuple)
    REC_W1,              // record word 1, the meta word of a two-word record (shard_extract_wide: high key word)
    REC_ST,              // stamp of the record, 4 or 8 bytes
    REC_COLS,
    REC_BASES = REC_W0,  // ar_part of shard_extract_wsk only: the bases of the records by value, 32 bytes each, in place of word 0.  A handle extracts its parts with one engine, so a part's buffer never holds both
};
// column of h->ar_q[set]: the successors a bucket could not resolve itself; moved like records by multisplit_level
enum QueryCol {
    Q_KEY,   // the successor's k-mer (low word for k > 31)
    Q_AUX,   // one-word engine: bucket hash of the key, the split's sort key (sharded builds and "resolve_sorted" only); two-word engine: high word, in SET_PONG the meta word
    Q_COL,   // position in d_col that waits for the answer
    Q_COLS
};

// h->ar_wide: the two-word (k > 31) engines
enum WideSlot {
    WIDE_PACKED,      // the reads packed to 2 bits a base: build_wide_once, wsk_extract
    WIDE_TABLE,       // WSlot hash table of the global wide engine: build_wide_once, shard_build_wide; dbg_import_graph's successor pass
    WIDE_TCNT,        // 32-bit successor counters next to the table (its unpacked variant): build_wide_once, shard_build_wide
    WIDE_OCC,         // occupancy byte per table slot: build_wide_once, shard_build_wide
    WIDE_WORD_RANK,   // scan of the occupancy, per 32 slots: build_wide_once, shard_build_wide
    WIDE_KEYS_HI,     // high key word of every node (d_keys_hi): every k > 31 engine; lives as long as the node arrays
    WIDE_SLOTS,
    WIDE_REC_BASES = WIDE_TCNT,  // LDS engine: the records' bases by value, 32 bytes each (wsk_count; shard_extract_wsk hands them to the exchange).  The counters live inside one call of the global engine, which starts from the reads and frees the build first; the bases are dead once wsk_count returns or the exchange has sent them
};

// h->ar_shard: what a sharded or multi-pass build parks for the exchange of successors
enum ShardSlot {
    SHARD_Q_KEYS,        // keys of the successors other shards own, grouped by owner; (lo, hi) pairs for k > 31: sk_count_from_segments / wsk_count park, dbg_shard_answer's caller reads
    SHARD_UNUSED_1,      // unused
    SHARD_RECV_COL,      // a column the receiver adds to the records it was sent: their positions (k > 31, k_wsk_iota128) or rebased 64-bit stamps (dbg_shard_build without sender_bucket_counts); dead when the count returns
    SHARD_Q_COL,         // d_col positions of SHARD_Q_KEYS' queries: dbg_shard_apply / dbg_part_apply write the answers there
    SHARD_WQ_META,       // wsk_count, sharded: meta word per query (k_wq_bucket), the owner split's sort key
    SHARD_UNUSED_5,      // unused
    SHARD_SLOTS,
    SHARD_PART_ANSWERS = SHARD_RECV_COL,  // parent of a multi-pass build: answers of one part to another's queries (multipass_parts).  Ensured after every part's count has been queued on the one stream, which is when the received column is dead
};

// h->ar_walk: the pointer-jumping non-final walk (walk_impl)
enum WalkSlot {
    WALK_JUMP,       // one-step table, one Jump per node
    WALK_DENSE,      // two Jump tables that are dense over the splitters, then the rank of every start
    WALK_SPLITTERS,  // list of the splitter nodes (k_jump_walk)
    WALK_SLOTS
};
// h->ar_refine: dbg_refine_edge_order's pass over the reads
enum RefineSlot {
    REFINE_SET_KEYS,  // member set: keys of the nodes with more than one successor
    REFINE_SET_NODE,  // ... their node ids
    REFINE_ESTAMP,    // first-seen stamp of each of their four edges
    REFINE_FILTER,    // one bit per top hash value of a member
    REFINE_SLOTS
};
// h->ar_tips: dbg_remove_tips
enum TipsSlot {
    TIPS_PULL_RANK,  // rank of every pulled node (d_pull_rank): outlives the call, read by the walk
    TIPS_PEND_A,     // pending branch nodes, ...
    TIPS_PEND_B,     // ... double-buffered
    TIPS_OWNER,      // reservation word per node
    TIPS_SLOTS
};
// h->ar_lookup: the sorted index of the current graph (query side, lookup_index_ensure)
enum LookupSlot {
    LOOKUP_KEYS,     // keys, sorted (low words)
    LOOKUP_IDS,      // node id of every sorted key
    LOOKUP_KEYS_HI,  // high words, two-word keys only
    LOOKUP_SLOTS
};

#ifndef DBG_L1_WIDE_FROM
#define DBG_L1_WIDE_FROM 20  // total bucket bits from which level 1 of the multisplit takes 10 bits instead of 9 (11..20)
#endif
#ifndef DBG_PS_WG_PER_CU
#define DBG_PS_WG_PER_CU DBG_EXW_WAVES  // extraction workgroups per CU of a pre-split extraction
#endif
#ifndef DBG_EXTRACT_PRESPLIT
#define DBG_EXTRACT_PRESPLIT 4  // default of option "extract_presplit" 
#endif

// ------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------
struct dbg {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // reads
    char *d_bases = nullptr;
    bool own_bases = false;
    uint64_t n_bytes = 0;
    uint64_t *d_offsets = nullptr;
    bool own_offsets = false;
    uint64_t n_reads = 0;
    uint32_t *d_startbits = nullptr;  // bit p set: a read starts at byte p (bit n_bytes = sentinel)
    uint64_t startbits_words = 0;
    // dbg_split_reads ran on the current read set; the origins of its pieces (both null: the identity, nothing was cut)
    bool split_done = false;
    uint64_t *d_org_read = nullptr, *d_org_pos = nullptr;
    uint32_t org_shift = 0;  // dbg_add_revcomp calls since then: the identity origins are (j >> org_shift, 0)

    // build
    int k = 0;
    Slot *d_tab = nullptr;
    uint64_t cap = 0;
    int cap_log2 = 0;
    uint32_t *d_occ = nullptr;  // occupancy bitmap over slots
    uint64_t *d_scalars = nullptr;  // [0] error flags [1] N_k [2] N_e [3..63] scratch [64..127] kernel descriptors
    uint64_t n_kmer_inst = 0, n_edge_inst = 0;
    uint64_t n_nodes = 0, n_edges = 0;
    uint64_t *d_keys = nullptr, *d_stamps = nullptr;
    uint64_t *d_keys_hi = nullptr;  // k > 31 only: bits 2k-1..64 of every node's k-mer (dbg_wide.h)
    uint32_t *d_cnt = nullptr;
    uint8_t *d_flags = nullptr;
    uint8_t *d_order = nullptr;  // successor codes ranked by (count desc, ascii asc), 2 bits each
    uint8_t *d_deg = nullptr;    // distinct successors (pre-pruning outdegree) -- feeds the CSR row scan
    uint8_t *d_fsorder = nullptr; // successor codes in first-seen order (dbg_refine_edge_order)
    bool order_exact = false;
    uint32_t *d_succ = nullptr;
    bool nodes_in_arena = false;  // node arrays borrowed from ar_node (super-k-mer engine)
    bool csr_built = false;       // rowptr/col/ecnt already written by k_sk_count
    uint64_t *d_rowptr = nullptr;
    uint32_t *d_col = nullptr, *d_ecnt = nullptr;
    // engine 0 writes ONE representation in the build: keys, stamps (32-bit while the reads stay below 2 GiB), one byte
    // per node (indegree | present bases << 1) and the CSR with 32-bit row pointers.  The dense per-base views above
    // (d_cnt, d_succ, d_order, 64-bit d_stamps / d_rowptr, plain d_flags) are derived by ensure_dense() on first use.
    bool dense_pending = false;
    uint32_t *d_rowptr32 = nullptr;
    void *d_stamps_st = nullptr;
    int stamps_st_bytes = 0;

    // prune / tips
    bool pruned = false, tipped = false;
    uint64_t n_branch = 0, n_pulled = 0, tip_rounds = 0;
    uint64_t *d_pull_rank = nullptr;

    // pull reads
    uint8_t *d_read_flags = nullptr;
    uint64_t n_pull_reads = 0;
    bool pull_reads_done = false;

    // walk
    uint64_t n_starts = 0, n_contigs = 0, contig_chars = 0;
    bool starts_known = false;    // n_starts counted for the current graph
    // engine 0, single GPU: the bucketed super-k-mer records of the last build (arena-owned, valid until the next build /
    // extraction): dbg_refine_edge_order re-reads them bucket by bucket instead of streaming the reads against a global set
    struct { const uint64_t *w0 = nullptr, *w1 = nullptr; const void *st = nullptr; int st_bytes = 0;
             const uint64_t *b_start = nullptr, *b_cnt = nullptr; bool valid = false; } sk_src;
    uint64_t *d_ctg_off = nullptr;
    char *d_ctg_chars = nullptr;
    uint64_t *d_ctg_score = nullptr, *d_ctg_stamp = nullptr;
    uint32_t *d_ctg_seq = nullptr;
    uint32_t *d_ctg_start = nullptr;  // list-ranking walk: start node of every contig (text on demand, dbg_export_contig_text)
    uint32_t *d_lift = nullptr;       // binary-lifting tables of the last walk, built on the first text request
    int lift_levels = 0;
    bool walked = false;          // contig text materialised
    bool walk_final = false;      // the last walk was a final-mode one (all simple paths, not chains)
    bool walk_indexed = false;    // contig index (offsets, scores, start stamps) valid
    bool walk_sizes_only = false; // the last walk (final-mode DFS) exceeded max_chars: counts valid, no index, no start nodes
    uint64_t part_final_steps = dbgk::FW_DEFAULT_STEPS;  // option "part_final_walk_steps": steps a walker of dbg_part_final_walk may take in a pass (2^24: 22 s at the 1.3 us a step measured; the enumeration is exponential in the worst case)
    uint64_t walk_jump_min = 1ull << 14;  // non-final walk: list ranking from this many nodes on (below: one thread per start)

    // alphabet / node layout: 2 bits and 4 successors for DNA, 5 bits and 32 for the generic engine
    int D = 4, sym_bits = 2, n_sym = 0;
    bool alpha_known = false, is_dna = true;
    uint8_t alphabet[32] = {0};       // generic: code -> byte (codes are assigned in byte order)
    uint8_t *d_lut = nullptr;         // generic: byte -> code (256 entries)
    char *d_alpha = nullptr;          // generic: code -> byte (32 entries, device)
    uint32_t *d_keepmask = nullptr;   // generic: surviving successors per node
    uint8_t *d_rank_mc = nullptr, *d_rank_fs = nullptr;  // generic: [n][32] successor codes by rank

    // options (dbg_set_option)
    int engine = 0;          // 0 = super-k-mer partitioned build, 1 = single global hash table
    int bucket_bits = 0;     // 0 = auto (super-k-mer engine)
    int lds_slots = 4096;    // LDS table slots per bucket workgroup (2048 or 4096)
    int phase_limit = 0;     // ablation of k_sk_count (timing only; the build then fails on purpose)
    int est_scale_pct = 100; // test hook: scales the distinct-k-mer estimate (a low one exercises the capacity retry)
    int wide_engine = 1;     // k = 32..63: 1 = super-k-mer / LDS engine (dbg_wsk.h), 0 = global reference-keyed table (dbg_wide.h)
    int count_kernel_u64 = 3; // option "count_kernel_u64": the count kernel of 64-bit stamps (shards, reads of 2 GiB and more): 3 = k_sk_count3 (one hint per slot; 12.2 ms on a 10 M-read shard), 1 = k_sk_count (13.4), 2 = k_sk_count2 (15.5: 320 staged records)
    int stamp64 = 0;         // option "stamp64" 1: dbg_build keeps 64-bit stamps even for reads below 2 GiB (what reads of 2 GiB and more get by themselves; tests)
    int resolve_sorted = 0;  // option "resolve_sorted" 1: cross-bucket queries grouped by the 512 level-1 groups of their target before k_succ_resolve.  Measured (tools/resolve_ab.py, 10 M reads): 3.09 ms with the grouping against 2.05 ms in the askers' order -- off
    int resolve_direct = 1;  // option "resolve_direct" 1: the resolver of a single-GPU build takes a successor's node from the directory entry alone where dir_decide (dbg_dir.h) can name it, and reads no key for it; 0: every query reads and compares its key run.  Measured: DESIGN.md 3
    int resolve_count = 0;   // option "resolve_count" 1 (tests): the resolvers' counting instantiation fills resolve_direct_hits / resolve_keyed
    uint64_t resolve_direct_hits = 0, resolve_keyed = 0;  // queries answered without / with a key read, summed over the handle's resolver launches under "resolve_count" (dbg_get_counter)
    int wcount_kernel = 2;   // 32 <= k <= 63, 32-bit stamps: 2 = k_wsk_count2 (one successor hint per slot, deferred lookups), 1 = k_wsk_count
    int count_kernel = 2;    // k <= 31, 4096 slots: 2 = k_sk_count2 (successor hints, 16-bit counters; falls back to 1 on counter overflow), 1 = k_sk_count

    // grow-only device arena of the super-k-mer engine: hipMalloc of tens of GB costs seconds,
    // so buffers survive across dbg_build calls on the same handle
    struct Buf {
        void *p = nullptr;
        uint64_t bytes = 0;
    };
    Buf ar_rec[PINGPONG_SETS][REC_COLS], ar_q[PINGPONG_SETS][Q_COLS], ar_node[NODE_SLOTS], ar_misc[MISC_SLOTS], ar_csr[CSR_SLOTS], ar_dir, ar_l2, ar_scan, ar_shard[SHARD_SLOTS], ar_walk[WALK_SLOTS], ar_wide[WIDE_SLOTS], ar_refine[REFINE_SLOTS], ar_tips[TIPS_SLOTS], ar_part[SHARD_EXTRACT_PARTS][REC_COLS] /* records of dbg_shard_extract_part, per part */;
    int sk_T = 0, sk_l1 = 0, sk_l2 = 0, sk_nb2 = 0 /* scaled second level, 0 = power of two */, sk_cap = 0;
    bool refine_streaming = false;  // option (tests): dbg_refine_edge_order always takes the pass over the reads
    int target_distinct = 0;  // option: mean distinct k-mers per bucket the auto geometry aims at (0 = default)
    int shard_stamp64 = 0;    // option: dbg_shard_extract hands out 64-bit rank-local stamps even below 2 GiB of reads (tests)
    int extract_generic = 0;  // option: 1 = the window-minimum-through-LDS extraction kernels instead of the per-window register ones (A/B, tests)
    int extract_presplit = DBG_EXTRACT_PRESPLIT;  // option: dbg_build's extraction pre-splits its records by this many top bits of the bucket hash (0: off)
    // What the LDS count kernels of the last build did beyond the ordinary pass (dbg_get_counter "count_*"): the event bits
    // (CountEvent, dbg_device.h) OR-ed over the count launches, the sub-range passes of the last launch and the launches that
    // were repeated, by reason.  A multi-pass parent or a shard holds the OR / the sums of its parts.
    struct CountPaths { uint64_t events = 0, extra_ranges = 0, retries_query_cap = 0, retries_node_cap = 0, retries_counter16 = 0; } count_paths;
    uint64_t presplit_rehists = 0;  // builds whose level 1 took another width than the pre-split extraction counted for, so it ran its histogram pass (dbg_get_counter)
    int extract_grid = 0;  // option: workgroups of a pre-split extraction (0: DBG_PS_WG_PER_CU per CU); the sub-segment limit may still ask for more (tests, A/B)
    uint64_t ms_scatter_small = 0, ms_scatter_wide = 0;  // multisplit levels of this handle that ran the small-fan-out / the wide scatter (dbg_get_counter)
    uint64_t presplit_fallbacks = 0;  // builds whose pre-split extraction overflowed a sub-segment and ran again without the split (dbg_get_counter)
    uint64_t refine_crowded = 0, pull_crowded = 0;  // dbg_refine_edge_order / dbg_mark_pull_reads calls whose per-range kernel met a crowded range and fell back to the pass over the reads (dbg_get_counter)
    uint64_t sk_n_ranges = 0, sk_n_buckets = 0;
    SkGeom sk_geom{};            // hash -> bucket mapping of the last partitioned build (k_succ_resolve)
    void *shard_state = nullptr;  // ShardState (multi-GPU builds)
    void *multipass = nullptr;    // MultiPass (dbg_build_multipass): the parts of the graph, parked in HBM
    bool dropping_parts = false;  // dbg_destroy / a build of another kind: nothing is parked
    dbg *spare_part = nullptr;    // the part handle of the last ONE-pass sharded build: its arenas serve the next one (bench loops)
    bool wide_owner = false;      // a part of a multi-pass build: successor ids are (owner byte, 32-bit local id), not tagged
    bool borrowed_stream = false; // sub-handle of a multi-pass build: the stream belongs to the parent
    bool arena_freed = false;     // an arena buffer went back to the memory pool since the last trim
    std::vector<uint64_t> host_seg_cnt;  // sk_extract: records per extraction segment (host copy)
    std::vector<uint64_t> host_scpre;    // multisplit_level: staging that must outlive an asynchronous upload
    uint64_t shard_node_limit = 0;  // option (tests): lowers the 2^29 - 16 node ids a shard may hand out
    bool partial_graph = false;   // the node table is one shard of several: successor ids point into other handles
    bool shard_open = false;      // dbg_shard_build ran and dbg_shard_apply has not yet: the successors other shards own are unresolved
    int spectrum_variant = 3;     // option "spectrum_variant": how k_spectrum relieves its hot bins (dbg_spectrum.h; measured: DESIGN.md 4l)
    // branch k-mer lookup (pull-out reads)
    uint64_t *d_btab = nullptr;
    uint64_t btab_cap = 0;
    // graph of dbg_build_from_walk(s) (dbg_nextk.h): nk_reads contigs of nk_bytes characters are virtual reads in front of
    // the real ones; their pull-out test needs, per block of contigs, the chain successors of the block's source graph,
    // z(x) and the start of every contig
    struct NkBlock {
        uint64_t n_src = 0, n_reads = 0;  // nodes of the source graph, contigs of the block
        uint32_t *next = nullptr, *z = nullptr, *start = nullptr;
    };
    bool nk_graph = false;
    uint64_t nk_reads = 0, nk_bytes = 0;
    std::vector<NkBlock> nk_blocks;
    uint8_t *d_nk_read_flags = nullptr;

    // query side (dbg_lookup.h).  dir_valid: ar_dir, the SkRange array, sk_geom and sk_cap are those of the build that made
    // the CURRENT graph (a single-GPU dbg_build on one of the LDS engines) -- set there, cleared by everything that replaces
    // or reshapes the graph or reuses ar_dir; never inferred from ar_dir.p
    bool dir_valid = false;
    int lookup_index = 0;     // option "lookup_index" 1 (tests): the sorted index even where the directory is valid
    Buf ar_lookup[LOOKUP_SLOTS];       // sorted index of the current graph: keys, ids, keys_hi (two-word keys) -- 12 or 20 B per node
    bool lookup_built = false;
    uint64_t lookup_index_builds = 0, lookup_dir_calls = 0, lookup_index_calls = 0;  // dbg_get_counter
    // a part of a multi-pass build: ar_dir, the SkRange array, sk_geom and the node arrays are those the part finished its
    // count with on the LDS engine (multipass_parts says so; like dir_valid never inferred from a pointer)
    bool part_dir_ok = false;
    uint64_t part_lookup_calls = 0;  // dbg_part_lookup_nodes[_device] / dbg_part_score_sequences calls that ran (dbg_get_counter)

    dbg_stats_t stats{};
    dbg_ingest_stats_t ingest{};  // the last FASTA or FASTQ ingest
    dbg_fastq_stats_t fastq{};    // the last FASTQ ingest (dbg_set_reads_fastq_file)
    dbg_fasta_records_stats_t fasta_rec{};  // the last record-mode FASTA ingest (dbg_set_reads_fasta_records[_file])
    dbg_contig_out_stats_t ctgout{};  // the last streamed contig output (dbg_ctgout.h)
    uint64_t ctgout_chunk = 0;        // option "ctgout_chunk_bytes": window size where a call names none (0: CO_DEFAULT_CHUNK)
};

// What a sharded build leaves behind for the exchange of successors owned by other ranks.
struct ShardState {
    int n_shards = 0, my_shard = 0, shard_bits = 0, k = 0;
    std::vector<uint64_t> q_start, q_cnt;   // remote queries grouped by owner (own group: count 0)
    uint64_t n_remote = 0;
    uint64_t n_kmer_inst_local = 0;          // k-mer instances of the reads this rank extracted
    std::vector<uint64_t> l1_counts;         // records per level-1 bucket (512) of the last dbg_shard_extract
    int rec_words = 1, rec_stamp_bytes = 4;  // what dbg_shard_extract handed out: words per record in d_w0, bytes per stamp
};
static ShardState &shard_of(dbg *h);
static void multipass_free(dbg *h);
static void drop_spare_part(dbg *h);

// Arena buffers come from the device's stream-ordered memory pool (hipMallocAsync on the handle's stream) with the
// pool told to keep what is freed: a hipMalloc / hipFree of several GB costs ~0.1 s each, and a multi-pass build
// allocates, trims and frees a few hundred GB in pieces of similar sizes -- 14 s of allocator calls around 0.4 s of
// kernels before this.  Everything a handle does is on its one stream, so stream order is program order.
static int buf_ensure(dbg *h, dbg::Buf &b, uint64_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return DBG_OK;
    if (b.p) { (void)hipFreeAsync(b.p, h->stream); h->arena_freed = true; }
    b.p = nullptr;
    b.bytes = 0;
    static const bool trace = getenv("DBG_TRACE_ALLOC") != nullptr;  // diagnostic: arena allocations that take longer than 5 ms
    const auto t_alloc = std::chrono::steady_clock::now();
    hipError_t e = hipMallocAsync(&b.p, bytes, h->stream);
    if (trace) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_alloc).count();
        if (ms > 5.0) fprintf(stderr, "[dbg] hipMallocAsync(%.3f GB) took %.1f ms (buffer %p of handle %p)\n", bytes / 1e9, ms, (void *)&b, (void *)h);
    }
    if (e != hipSuccess) {
        // the pool may be holding freed blocks of the wrong sizes: give them back to the device and try once more
        (void)hipGetLastError();
        (void)hipStreamSynchronize(h->stream);
        hipMemPool_t pool;
        if (hipDeviceGetDefaultMemPool(&pool, h->device) == hipSuccess) (void)hipMemPoolTrimTo(pool, 0);
        e = hipMallocAsync(&b.p, bytes, h->stream);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->err = std::string("hipMallocAsync(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
        b.p = nullptr;
        return DBG_E_NOMEM;
    }
    b.bytes = bytes;
    return DBG_OK;
}
static void buf_free(dbg *h, dbg::Buf &b) {
    if (b.p) { (void)hipFreeAsync(b.p, h->stream); h->arena_freed = true; }
    b.p = nullptr;
    b.bytes = 0;
}
// Blocks the pool kept for reuse go back to the device: called when a build is complete, so that what the library
// holds is what it uses (other allocators of the process -- torch -- see the rest) and a later build does not find the
// pool full of blocks of the wrong sizes.
static void pool_trim(dbg *h) {
    if (!h->arena_freed) return;
    (void)hipStreamSynchronize(h->stream);
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, h->device) == hipSuccess) (void)hipMemPoolTrimTo(pool, 0);
    (void)hipGetLastError();
    h->arena_freed = false;
}

#define HIPCHK(h, call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
            return e_ == hipErrorOutOfMemory ? DBG_E_NOMEM : DBG_E_HIP;                      \
        }                                                                                    \
    } while (0)

#define CHK(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != DBG_OK) return rc_; \
    } while (0)

template <class T>
static int dev_alloc(dbg *h, T **p, uint64_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    HIPCHK(h, hipMalloc((void **)p, count * sizeof(T)));
    return DBG_OK;
}
template <class T>
static void dev_free(T *&p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

static inline unsigned grid_for(uint64_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    explicit Timer(hipStream_t st) : s(st) {
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        (void)hipEventRecord(a, s);
    }
    double stop() {
        (void)hipEventRecord(b, s);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        return ms;
    }
    ~Timer() {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
    }
};
