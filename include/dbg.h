/*
 * dbg.h -- C ABI of the MI355X (gfx950) de Bruijn graph hot path.
 *
 * The reference (Zhijian-Mei/py-debruijn) has no FFI or plugin interface; the
 * boundary it offers is the Python module surface of debruijn.py as consumed by
 * II_assembleFromReads.py:11-12,58,61,63.  This header is the C-ABI a binding
 * for that surface sits on (ctypes stub: INTEGRATION.md; the shipped binding is
 * py-debruijn_amd/_dbg.py).  Each entry point names the reference lines it
 * replaces.  All pointers are plain host pointers unless the name says
 * "device"; every buffer is owned by the caller; the library owns only the
 * opaque handle and the device memory behind it.
 *
 * Conventions
 *   - every function returns 0 (DBG_OK) or a negative DBG_E_* code; the text of
 *     the last failure is dbg_last_error(h).  Nothing throws or aborts.
 *   - a handle is bound to one GPU and is not thread-safe; calls are
 *     stream-synchronous on return.
 *   - k-mers travel as 2-bit packed keys: base code = (ascii >> 1) & 3
 *     (A=0, C=1, T=2, G=3), first base in the most significant used bits,
 *     key = sum(code[i] << 2*(k-1-i)); 1 <= k <= 31 is one 64-bit word, 32 <= k <= 63 two (the upper word:
 *     dbg_export_keys_hi / dbg_device_keys_hi / dbg_part_keys_hi).
 *   - "stamp" of a node = (byte offset of its first occurrence in the
 *     concatenated read buffer << 1) | (1 if that occurrence is NOT at position
 *     0 of its read).  Ascending stamp == the reference's dict insertion order
 *     (debruijn.py:121-147); stamp & 1 == the reference's Node.indegree.
 *   - reads made of upper-case A/C/G/T only take the 2-bit path above (k <= 63).  Any other
 *     alphabet (the reference is alphabet-agnostic; its real inputs are peptides) takes the
 *     generic path: up to 32 distinct bytes, codes in byte order (dbg_get_alphabet), 32 successor
 *     slots per node, k <= 63 (5 bits per character in one word up to k = 11, tables keyed by
 *     reference into the reads above); DBG_E_ALPHABET for more symbols.  k >= 64 is DBG_E_ARG, as on every path.
 *   - that is the default and stays it: 'N' is a character, and k-mers that hold it are nodes.  dbg_split_reads is the
 *     other choice: it replaces the resident reads by their pieces,
 *       pieces(reads, fold) = [m for r in reads for m in re.findall(b"[ACGT]+", fold_acgt(r) if fold else r)]
 *     where fold_acgt maps the four bytes a c g t to A C G T and nothing else.  Every other byte (>= 0x80 included) is
 *     a cut; a read with no base (the empty read too) gives no piece; two reads never merge; no k-mer window spans a
 *     cut.  The graph of the pieces is the reference run on that list, and it takes the 2-bit path.
 */
#ifndef DBG_H
#define DBG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dbg dbg_t;

#define DBG_OK 0
#define DBG_E_ARG (-1)      /* bad argument or call order */
#define DBG_E_HIP (-2)      /* HIP runtime failure (text in dbg_last_error) */
#define DBG_E_ALPHABET (-3) /* the reads hold more than 32 distinct bytes, or a byte outside upper-case "ACGT" in a call that takes such reads only */
#define DBG_E_CAPACITY (-4) /* hash table or an output limit was exceeded */
#define DBG_E_NOMEM (-5)    /* host or device allocation failed */

#define DBG_ABI_VERSION 6 /* not raised for dbg_build_from_walks, nor for the query calls (dbg_lookup_nodes[_device],
                            * dbg_gather_nodes, dbg_score_sequences, dbg_part_lookup_nodes[_device],
                            * dbg_part_score_sequences), nor for dbg_split_reads / dbg_read_origins, nor for dbg_add_revcomp,
                            * nor for dbg_set_reads_fasta_records[_file] / dbg_fasta_records_stats / dbg_write_contigs_fasta_wrapped, nor for dbg_count_spectrum: they only add symbols, every earlier call and struct is
                            * unchanged, and tests/test_fasta_stream.py pins this number; a binding that needs a new
                            * call fails at symbol lookup on an older library */

/* node flag bits (dbg_export_nodes: flags[]) */
#define DBG_F_INDEG 0x01u    /* Node.indegree (0 or 1), debruijn.py:134,141-142 */
#define DBG_F_KEEP_MASK 0x1Eu /* bit (1 + code) set: successor `code` survived pruningEdges */
#define DBG_F_KEEP_SHIFT 1
#define DBG_F_BRANCH 0x20u   /* > 1 surviving successor, debruijn.py:230-235 */
#define DBG_F_PULLED 0x40u   /* in already_pull_out, debruijn.py:249-254 */

#define DBG_NO_NODE 0xFFFFFFFFu

typedef struct dbg_sizes {
    int32_t k;
    int32_t abi_version;
    uint64_t n_reads;
    uint64_t n_bytes;          /* bases in the concatenated read buffer */
    uint64_t n_kmer_instances; /* N_k: k-mer windows of reads with len > k */
    uint64_t n_edge_instances; /* N_e: (k+1)-mer windows */
    uint64_t table_capacity;   /* hash slots */
    uint64_t n_nodes;          /* distinct k-mers == len(vertices) */
    uint64_t n_edges;          /* distinct (k+1)-mers == len(edge_count_table) */
    uint64_t n_branch;
    uint64_t n_pulled;
    uint64_t n_pull_reads;
    uint64_t n_starts;         /* nodes with indegree 0 */
    uint64_t n_contigs;
    uint64_t contig_chars;     /* total characters over all contigs */
    uint64_t tip_rounds;       /* reservation rounds the tip removal needed */
    uint64_t contigs_materialised; /* 1: contig text available (dbg_export_contigs); 0: index only */
    uint64_t max_degree;       /* successor slots per node: 4 (ACGT reads) or 32 (any other alphabet) */
} dbg_sizes_t;

typedef struct dbg_stats {
    /* device time of each phase of the last call, milliseconds (HIP events on the handle's stream) */
    double ms_startbits;  /* read-start bitmap */
    double ms_table_init; /* engine 1: hash table clear */
    double ms_count;      /* encode + hash insert + edge counters (dominant kernel) */
    double ms_compact;    /* engine 1: occupied slots -> node arrays */
    double ms_succ;       /* successor lookup -> 4-way adjacency */
    double ms_csr;        /* degree scan + CSR fill */
    double ms_build_total;
    double ms_prune;
    double ms_tips;
    double ms_pull_reads;
    double ms_walk;
    double ms_h2d;        /* dbg_set_reads copy */
    double ms_extract;    /* engine 0: reads -> super-k-mer records (k_sk_extract) */
    double ms_partition;  /* engine 0: two-level multisplit of the records */
    uint64_t count_launches; /* launches of the dominant kernel in the last dbg_build */
    uint64_t n_records;      /* engine 0: super-k-mer records */
    uint64_t n_buckets;      /* engine 0: final buckets */
    uint64_t n_queries;      /* engine 0: successors resolved across buckets */
} dbg_stats_t;

/* what the last FASTA ingest (dbg_set_reads_fasta_file, or dbg_set_reads_fasta: one chunk) did */
typedef struct dbg_ingest_stats {
    uint64_t bytes_read;        /* file bytes read (the owned lines, the byte before `begin`, the read-ahead of the last chunk) */
    uint64_t chunks;            /* staging chunks copied to the device */
    uint64_t chunk_bytes;       /* size of a staging buffer */
    uint64_t peak_device_bytes; /* most device memory the ingest held at once: text, parse scratch, bases, offsets (the
                                 * read-start bitmap every read set gets is not counted) */
    uint64_t n_reads;
    uint64_t n_bases;
    double ms_total;            /* wall time of the call */
    double ms_io_wait;          /* host time spent in file reads */
    double ms_h2d;              /* device time of the staging copies */
    double ms_parse;            /* device time of the parse kernels */
} dbg_ingest_stats_t;

/* what the last streamed contig output (dbg_write_contigs_fasta, or dbg_export_contig_texts with a text buffer) did */
typedef struct dbg_contig_out_stats {
    uint64_t bytes_written;     /* bytes handed to write() / copied into the caller's buffer */
    uint64_t chunks;            /* windows filled on the device and copied to the host */
    uint64_t chunk_bytes;       /* size of a window */
    uint64_t peak_device_bytes; /* most device memory the call held at once: the two staging buffers and the per-record arrays
                                 * (contig list, record positions: 12 B per record), or, before those, the sorts of the
                                 * driver's order (two key and two id arrays, 24 B per contig, + the sort library's digit
                                 * counters and look-back state, about n / 4 B).  At most
                                 * 2 * chunk_bytes + 24 * (n + 1) + 1 MiB for n records while that last term stays below
                                 * 2 * chunk_bytes + 1 MiB: up to ~4e6 contigs at 4096-byte windows, ~3e7 at the default;
                                 * a caller's list sorts nothing and always keeps it */
    uint64_t lift_bytes;        /* binary-lifting tables of the walk (index-only walks; built once per walk, kept by it) */
    double ms_total;            /* wall time of the call */
    double ms_io_wait;          /* host time in write() / in the copies into the caller's buffer */
    double ms_fill;             /* device time of the fill kernel */
    double ms_d2h;              /* device time of the staging copies */
} dbg_contig_out_stats_t;

/* ---- lifetime ---------------------------------------------------------- */
int dbg_create(int device, dbg_t **out);
void dbg_destroy(dbg_t *h);
const char *dbg_last_error(const dbg_t *h);
int dbg_abi_version(void);
/* Tunables (no reference counterpart): "engine" 0 = partitioned super-k-mer build (default),
 * 1 = single global hash table; "bucket_bits" 0 = auto, else log2 of the bucket count (<= 20);
 * "lds_slots" 2048 or 4096 slots of the per-bucket LDS table; "walk_jump_min_nodes" see dbg_walk;
 * "phase_limit" timing ablation of the count kernel (the build then fails on purpose);
 * "estimate_scale_pct" test hook: scales the distinct-k-mer estimate that sizes the node arrays (a low value
 * makes the first count launch run out of room and exercises the retry; dbg_stats_t.count_launches);
 * "refine_streaming" 1: dbg_refine_edge_order takes its pass over the reads even when the bucketed records of the build
 * are there (test hook: both ways must agree).
 * Count kernels (A/B and tests; the defaults are the measured winners): "count_kernel" k <= 31, 32-bit
 * stamps: 2 = k_sk_count2 (default), 1 = k_sk_count, 3 = k_sk_count3; "count_kernel_u64" k <= 31, 64-bit stamps (shards, reads
 * of 2 GiB and more): 3 = k_sk_count3 (default), 1, 2; "wcount_kernel" k > 31, 32-bit stamps: 2 = k_wsk_count2 (default),
 * 1 = k_wsk_count; "stamp64" 1: dbg_build / dbg_build_multipass keep 64-bit stamps below 2 GiB of reads too (what larger
 * inputs get by themselves); "resolve_sorted" 1 (2: at any size): cross-bucket successor queries grouped by their target
 * before the resolver (measured slower: off); "resolve_direct" 1 (default): the resolver of a single-GPU build takes a
 * cross-bucket successor's node from the directory entry of its home slot alone where that entry names it (the run of
 * occupied slots from the home slot is one slot long and ends inside the 64-slot block) and reads no key for it -- such an
 * answer is not compared, so a single wrong directory entry no longer fails the build by itself; 0: every query reads and
 * compares its key run (the full check); sharded builds and dbg_shard_answer always compare;
 * "resolve_count" 1 (tests): the resolvers run a counting instantiation that fills the resolve_* counters of
 * dbg_get_counter; "wide_engine" 0: k > 31 on the global-table engine of round 1;
 * "extract_generic" 1: the window-minimum-through-LDS extraction kernels; "extract_presplit" f0 in 0..6: dbg_build's
 * extraction (13 <= k <= 31 over ACGT) writes its records pre-split by the top f0 bits of the bucket hash so that level 1 of
 * the multisplit has 2^f0 times fewer children per group (0: one segment per workgroup);
 * "extract_grid" 0..65535: the workgroups of that pre-split extraction (0: four per CU; a whole multiple of it where a
 * sub-segment would otherwise outgrow one super-chunk of the multisplit; tests and A/B); "shard_stamp64" 1: dbg_shard_extract hands out
 * 64-bit rank-local stamps; "target_distinct": mean distinct k-mers per bucket the geometry aims at (0 = default);
 * "lookup_index" 1: the query calls (dbg_lookup_nodes, dbg_score_sequences) find nodes through the sorted index even where
 * the build's directory would answer (test hook: both ways must agree);
 * "ctgout_chunk_bytes": window size of the contig output calls where they are given none (dbg_export_contig_texts;
 * dbg_write_contigs_fasta with chunk_bytes 0) -- a multiple of 4096, 0 = the library default of 4 MiB;
 * "spectrum_variant" 0..3 (A/B and tests; the default is the measured winner): how dbg_count_spectrum's kernel
 * takes the contention off its hot bins -- 0 plain LDS atomics, 1 one sub-histogram per wave, 2 equal bins of a wave combined
 * by ballots until every lane is served, 3 one such round for the first lane's bin and plain atomics for the rest. */
int dbg_set_option(dbg_t *h, const char *name, int64_t value);

/* ---- reads (replaces the `reads` list argument, debruijn.py:206; FASTA
 *      ingest debruijn.py:22-32 stays on the host side of the boundary) ---- */
/* bases: all reads concatenated without separators; offsets[n_reads+1], offsets[0]==0. Copies H2D. */
int dbg_set_reads(dbg_t *h, const char *bases, const uint64_t *offsets, uint64_t n_reads);
/* read_reads (debruijn.py:22-32) on the device: `text` is the raw FASTA file (host buffer); every line that
 * does not start with '>' becomes one read, rstrip'ed (universal newlines, multi-line records are separate
 * reads, blank lines are empty reads).  Sizes afterwards: dbg_get_sizes; the reads: dbg_copy_reads. */
int dbg_set_reads_fasta(dbg_t *h, const char *text, uint64_t n_text);
/* Reads of the lines whose FIRST byte lies in [begin, end) of the file at `path` (end = UINT64_MAX: to EOF), with
 * dbg_set_reads_fasta semantics.  A line that starts inside the range is read to its terminator, even past `end`.
 * Byte p starts a line iff p == 0, t[p-1] == '\n', or t[p-1] == '\r' and t[p] != '\n' (universal newlines), so the
 * reads of [0, b) followed by those of [b, n) are the reads of the whole file for every b.
 * The file streams through two pinned staging buffers of chunk_bytes (0 = library default, 16 MiB); the host reads
 * chunk i+1 while chunk i is copied and parsed on the device.  Neither the host nor the device ever holds the whole
 * image: the device holds the packed bases (sized from the range), the offsets (grown as reads arrive) and ~1.5 chunks
 * of parse state.  DBG_E_ARG (text in dbg_last_error) for a missing or unreadable file or begin > end; a begin at or
 * past the end of the file gives an empty read set. */
int dbg_set_reads_fasta_file(dbg_t *h, const char *path, uint64_t begin, uint64_t end, uint64_t chunk_bytes);
int dbg_fasta_ingest_stats(dbg_t *h, dbg_ingest_stats_t *out);
/* Record mode of the FASTA ingest: read i is RECORD i, not line i.  Lines are those of dbg_set_reads_fasta_file (universal
 * newlines).  A header is a line whose first byte is '>' (a '>' anywhere else is a character; a line that begins with a
 * space and then '>' is a sequence line).  Read i is the concatenation of the sequence lines between header i and the next
 * header or the end of the file, each line rstrip'ed on its own (white space inside a line stays, a blank line adds
 * nothing); a header followed at once by a header or by the end of the file gives an empty read, so n_reads is the number
 * of headers.  Non-header lines in front of the file's first header must be blank after rstrip; anything else is a
 * malformed file: DBG_E_ARG, dbg_last_error names the byte position of the first offending byte, and the handle is left
 * with no reads (and stays usable).  No ';' comment lines, no detection of the format, no check of the alphabet.
 * dbg_set_reads_fasta_records_file reads the records whose header's FIRST byte lies in [begin, end) of the file at `path`
 * (end = UINT64_MAX: to EOF), with the arguments and errors of dbg_set_reads_fasta_file.  A record that starts inside the
 * range is read to its end, even past `end`; bytes between `begin` and the first owned header belong to the previous
 * range's last record; only the range with begin == 0 reports sequence before the first header; a range without a header
 * is an empty read set (DBG_OK).  So the reads of [0, b) followed by those of [b, size) are the reads of the file for every
 * b.  The host finds the first header at or after `begin` and at or after `end` before the first chunk, then the owned
 * bytes stream as in dbg_set_reads_fasta_file; the device holds the packed bases (owned bytes at most), the offsets and
 * ~1.5 chunks of parse state.  dbg_set_reads_fasta_records takes the whole image from a host buffer and runs it as one
 * range through the same stream.  Both fill dbg_ingest_stats_t too (bytes_read counts the host's search as well). */
int dbg_set_reads_fasta_records(dbg_t *h, const char *text, uint64_t n_text);
int dbg_set_reads_fasta_records_file(dbg_t *h, const char *path, uint64_t begin, uint64_t end, uint64_t chunk_bytes);
/* what the last record-mode ingest did, beside dbg_ingest_stats_t */
typedef struct dbg_fasta_records_stats {
    uint64_t n_records;         /* owned headers = reads */
    uint64_t n_sequence_lines;  /* owned non-header lines, blank ones included */
    uint64_t longest_record;    /* bases of the longest read */
    uint64_t first_byte;        /* file position of the first owned header (end_byte if none) */
    uint64_t end_byte;          /* file position of the first header at or past `end`, or the file size */
    uint64_t scan_bytes;        /* bytes the host read to find those two positions */
} dbg_fasta_records_stats_t;
int dbg_fasta_records_stats(dbg_t *h, dbg_fasta_records_stats_t *out);
/* Reads of the FASTQ records whose header line's FIRST byte lies in [begin, end) of the file at `path` (end = UINT64_MAX:
 * to EOF), streamed and parsed like dbg_set_reads_fasta_file (same arguments, same errors, any chunk_bytes from 1 up; it
 * fills dbg_ingest_stats_t too, bytes_read being the bytes of the owned records).  Read i is the sequence line of record i,
 * rstrip'ed; a record that starts inside the range is read to its end, even past `end`.
 * The format is strict four-line FASTQ over universal-newline lines: trailing lines of the file that are empty after rstrip
 * are ignored; the others come in groups of four: a header that begins with '@', the sequence (it must not begin with '@'
 * or '+'; it may be empty), a separator that begins with '+', and a quality line of exactly the sequence's length after
 * rstrip.  Only the file's last record may lack its quality line, and only if its read is empty.  Anything else is a
 * malformed file: DBG_E_ARG, dbg_last_error names the 0-based record within the range and the kind (header, sequence
 * start, separator, length mismatch, truncated record, quality byte), and the handle is left with no reads.
 * The record start at or after a position is the first line start p >= position with t[p] == '@' whose second-next line
 * begins with '+' (0 for position 0); on every file the whole-file parse accepts these are the true header lines, so the
 * reads of [0, b) followed by those of [b, size) are the reads of the file for every b.
 * min_quality q in 0..93 (more: DBG_E_ARG), Phred+33: with q > 0 base j of a read becomes the byte 'N' where
 * qual[j] - 33 < q, whatever it was, and a quality byte outside 33..126 is malformed; lengths do not change, so
 * dbg_split_reads afterwards cuts there and its origins count positions of the unmasked read.  With 0 the mask is off and
 * quality bytes are never stored.  Device memory: the bases (half the owned bytes; twice that while a mask holds the
 * qualities), the offsets and ~1.75 chunks of parse state. */
int dbg_set_reads_fastq_file(dbg_t *h, const char *path, uint64_t begin, uint64_t end, uint64_t chunk_bytes, uint32_t min_quality);
/* what the last dbg_set_reads_fastq_file did, beside dbg_ingest_stats_t */
typedef struct dbg_fastq_stats {
    uint64_t n_records;          /* records owned = reads */
    uint64_t masked_bases;       /* bases the quality mask turned into 'N' (counted whatever the base was) */
    uint64_t quality_bytes_held; /* size of the quality buffer while the mask needed it (0 with the mask off) */
    uint64_t peak_device_bytes;  /* as in dbg_ingest_stats_t, the quality buffer included */
    uint64_t min_quality;
    uint64_t first_byte;         /* file position of the first owned record's header */
    uint64_t end_byte;           /* file position after the last owned record (trailing white space of the file left out) */
    double ms_mask;              /* device time of the mask pass */
} dbg_fastq_stats_t;
int dbg_fastq_ingest_stats(dbg_t *h, dbg_fastq_stats_t *out);
/* Zero-copy: device pointers the caller keeps alive (16-byte aligned bases, u64 offsets[n_reads+1]). */
int dbg_set_reads_device(dbg_t *h, const void *d_bases, uint64_t n_bytes, const void *d_offsets, uint64_t n_reads);
/* Generate reads [first_read, first_read+n_reads) of the synthetic set on the device
 * (bit-identical to py-debruijn_amd/synth.py).  err_thr24 = round(err_rate * 2^24). */
int dbg_synth_reads(dbg_t *h, uint64_t seed, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                    uint32_t read_len, uint32_t err_thr24);
int dbg_reads_checksum(dbg_t *h, uint64_t *out);              /* synth.checksum twin */
int dbg_copy_reads(dbg_t *h, char *bases, uint64_t *offsets); /* D2H of the current read set */
/* [self[i] for i in indices] of the reference's `reads` list without bringing every read to the host (pull_out_read,
 * debruijn.py:274-278, is a few per cent of the reads): the selected reads, concatenated, gathered on the device.
 * out_offsets[n + 1] (may be NULL) and *n_chars are always set; out_chars may be NULL (first call: sizes only),
 * else capacity >= *n_chars. */
int dbg_take_reads(dbg_t *h, const uint64_t *indices, uint64_t n, uint64_t *out_offsets, char *out_chars, uint64_t capacity,
                   uint64_t *n_chars);
/* device pointers of the current read set (bases: n_bytes chars; offsets: u64[n_reads + 1]); valid until the reads change */
int dbg_reads_device(dbg_t *h, const void **d_bases, uint64_t *n_bytes, const void **d_offsets, uint64_t *n_reads);
/* Cuts the resident reads at every byte that is not A/C/G/T (the contract is in the header comment above) in one pass
 * on the device, whichever call set them.  Like dbg_set_reads it drops any graph, walk and parts of the handle.
 * DBG_SPLIT_FOLD_CASE folds a c g t to upper case first; any other flag bit is DBG_E_ARG.
 * A read set with nothing to cut, to fold or to drop stays as it is (changed == 0): the same device pointers, no
 * allocation, one read of the bases.  Folding alone happens in place where the handle owns the bases (changed == 1, the
 * pointers stay).  Otherwise the pieces go to new buffers of exactly their size, the old ones are freed if the handle
 * owns them, and dbg_get_sizes, dbg_copy_reads, dbg_take_reads, dbg_reads_device and dbg_export_pull_reads speak of
 * the pieces from then on.  Buffers lent through dbg_set_reads_device are never written: a lent read set that has to
 * change is replaced by buffers the handle owns. */
#define DBG_SPLIT_FOLD_CASE 1u
typedef struct dbg_split_stats {
    uint64_t n_reads_in, n_bytes_in;
    uint64_t n_reads_out, n_bytes_out; /* the pieces and their bases */
    uint64_t n_cut_bytes;              /* n_bytes_in - n_bytes_out */
    uint64_t n_folded_bytes;           /* kept bytes the fold changed */
    uint64_t n_reads_changed;          /* reads that lose at least one byte */
    uint64_t n_reads_emptied;          /* reads left without a piece (the empty reads among them) */
    uint64_t changed;                  /* 0: the read set is the one that was there */
    uint64_t peak_extra_device_bytes;  /* most device memory the call held beside the read set it found: new bases,
                                        * offsets, origins (8 B + 16 B per piece) and 16 B per 64 KiB block of scan scratch */
} dbg_split_stats_t;
int dbg_split_reads(dbg_t *h, uint32_t flags, dbg_split_stats_t *out /* may be NULL */);
/* Where piece j of the last dbg_split_reads came from: read_index[j] = the read (as numbered before the call), pos[j] =
 * its first byte's position in that read; [n_reads] each, either may be NULL.  After a call that changed nothing: (j, 0).
 * DBG_E_ARG before a dbg_split_reads on the current read set: every dbg_set_reads* forgets the origins. */
int dbg_read_origins(dbg_t *h, uint64_t *read_index, uint64_t *pos);
/* Both strands: replaces the resident reads r0, r1, ... by r0, rc(r0), r1, rc(r1), ... in one streaming pass on the device,
 * whichever call set them.  The graph of both strands is, by definition, the reference run on that list; read j of the
 * new set is strand j & 1 of old read j >> 1.  With n reads, N bytes and offsets o[] (len_i = o[i+1] - o[i]):
 *   - the outputs are buffers of exactly their size that the handle owns: 2N + 64 bytes of bases (64 bytes of zero padding,
 *     aligned as dbg_set_reads aligns them) and 2n + 1 offsets,
 *       out_off[2i] = 2 o[i],  out_off[2i+1] = 2 o[i] + len_i,  out_off[2n] = 2N
 *       out[2 o[i] + j] = in[o[i] + j],  out[2 o[i] + len_i + j] = comp(in[o[i] + len_i - 1 - j])
 *   - comp maps A<->T, C<->G, a<->t, c<->g; every other byte ('N' and bytes >= 0x80 included) maps to itself, so the
 *     alphabet never grows beyond what the input plus these eight bytes allow.  On generic or peptide reads the call
 *     does exactly the same (meaningless there, but defined); n_other_bytes says how many bytes were not complemented.
 *   - an empty read gives two empty reads; n = 0 is DBG_OK with an empty read set; no reads set is DBG_E_ARG; flags are
 *     reserved: any bit set is DBG_E_ARG.
 *   - like dbg_set_reads and dbg_split_reads the call drops any graph, walk and parts of the handle, forgets the cached
 *     alphabet and rebuilds the read-start bitmap.  Buffers lent through dbg_set_reads_device are never written: they are
 *     let go and replaced by owned ones; owned old buffers are freed after the swap.  On any failure the handle keeps
 *     the read set it had.  Calling it twice doubles twice: it is an operation on the list, not a mode.
 *   - dbg_read_origins keeps working: after a dbg_split_reads, entries 2i and 2i+1 both carry piece i's (read_index, pos),
 *     pos being the position of the piece's first byte in forward orientation; identity origins become (j >> 1, 0).  The
 *     strand of read j is j & 1, so no third array exists.  Without a dbg_split_reads it fails as before. */
typedef struct dbg_revcomp_stats {
    uint64_t n_reads_in, n_bytes_in;
    uint64_t n_reads_out, n_bytes_out; /* 2 n_reads_in, 2 n_bytes_in */
    uint64_t n_other_bytes;            /* input bytes comp leaves as they are */
    uint64_t n_palindromes;            /* reads of at least one byte whose reverse complement is the read itself */
    uint64_t peak_extra_device_bytes;  /* the old and the new read set live at once: 2N + 64 + 8 (2n + 1), plus 32 B per
                                        * read for the doubled origins of an earlier split */
    double ms_kernel;                  /* the pass's kernels, by events on the handle's stream */
} dbg_revcomp_stats_t;
int dbg_add_revcomp(dbg_t *h, uint32_t flags, dbg_revcomp_stats_t *out /* may be NULL */);

/* ---- a3 + a4: get_graph_from_reads (debruijn.py:98-147) + edge-count table (:213-222)
 *      -> node table, 4-way successor edges, CSR ------------------------------------ */
/* table_capacity_hint: 0 = size for the worst case (every k-mer instance distinct);
 * otherwise a slot count (rounded up to a power of two); DBG_E_CAPACITY if too small.
 * k: 1..63 for reads over ACGT (k <= 31: one 64-bit word per k-mer, the partitioned engine;
 * 32..63: two words per k-mer, a reference-keyed global table -- BASELINE.json configs[4]);
 * 1..63 for any other alphabet of at most 32 distinct bytes (k <= 11: 5 bits per character in one word;
 * above: tables keyed by reference into the reads -- such nodes have no packed key, dbg_export_nodes returns
 * zeros for keys and the k-mer of node i is the k bytes at offset stamps[i] >> 1 of the reads). */
int dbg_build(dbg_t *h, int k, uint64_t table_capacity_hint);

/* ---- the same graph in several passes (BASELINE.json configs[3]: more nodes than one 32-bit id space, or than one pass
 *      should hold in flight).  The reads are cut into records once and split by the 512 top-9-bit groups of the
 *      bucket hash; pass p builds the groups [p * 512 / n_passes, (p + 1) * 512 / n_passes) into PART p, whose arrays
 *      stay parked in HBM.  A node id is (part, local id < 2^32 - 16): up to 64 x (2^32 - 16) nodes.  n_passes: a power of two
 *      up to 64; k <= 31; ACGT reads.  Afterwards dbg_get_sizes reports the totals; the graph is read part by part
 *      (below); the traversal entry points refuse it (their node ids are 32-bit). */
int dbg_build_multipass(dbg_t *h, int k, int n_passes);
int dbg_part_count(dbg_t *h, int *n_parts);
/* first_node_id: global id of the part's node 0 when the parts are concatenated in order */
int dbg_part_sizes(dbg_t *h, int part, uint64_t *n_nodes, uint64_t *n_edges, uint64_t *first_node_id);
/* keys[n], stamps[n], flags[n] (DBG_F_INDEG | bit (1 + code): base `code` is a successor), CSR row_ptr[n + 1] and per
 * column: col[e] = local id of the successor in part col_part[e], cnt[e] = count of the (k+1)-mer.  The columns of a
 * row follow the base codes set in flags, ascending.  NULL pointers are skipped. */
int dbg_export_part(dbg_t *h, int part, uint64_t *keys, uint64_t *stamps, uint8_t *flags, uint64_t *row_ptr, uint32_t *col,
                    uint8_t *col_part, uint32_t *cnt);
/* the same arrays on the device (valid until the next build): stamps are uint32 or uint64 (*stamp_bytes), row_ptr uint32 */
int dbg_part_device_views(dbg_t *h, int part, const void **d_keys, const void **d_stamps, int *stamp_bytes,
                          const void **d_flags, const void **d_row_ptr32, const void **d_col, const void **d_col_part,
                          const void **d_cnt);
/* upper key words of a part's nodes (k > 31: the k-mer is keys_hi * 2^64 + keys; all zero for k <= 31): keys_hi[n_nodes]
 * on the host and / or the device pointer (NULL for k <= 31); either output may be NULL */
int dbg_part_keys_hi(dbg_t *h, int part, uint64_t *keys_hi, const void **d_keys_hi);
/* ---- ranks x passes (BASELINE.json configs[3] on several GPUs): a rank of a sharded build that builds its shard as
 *      n_passes parts.  Input as for dbg_shard_build with sender_bucket_counts (stamp_bytes 4 or 8); part p of rank r is
 *      VIRTUAL shard r * n_passes + p of n_shards * n_passes (<= 64), and col_part of a column holds the virtual shard
 *      of the successor.  Successors owned by other RANKS are open afterwards:
 *        dbg_part_queries  the successor k-mers of `part`, group of virtual shard v at [q_starts[v], + q_counts[v]) of
 *                          *d_q_keys (uint64, device); arrays of n_shards * n_passes entries, own rank's groups count 0
 *        dbg_part_answer   the owner: node ids (uint32, device; local to `part`) of n k-mers it was asked about
 *        dbg_part_apply    the asker: d_answers (uint32, device) = answers of virtual shard `owner` to that whole group
 *        dbg_multipass_finish  frees the query lists; fails if any successor stayed unresolved
 *      (multi_gpu.sharded_build_multipass runs these around two all-to-alls per pass). */
int dbg_shard_build_multipass(dbg_t *h, int k, int n_shards, int my_shard, int n_passes, const void *d_w0, const void *d_w1,
                              const void *d_st, int stamp_bytes, const uint64_t *recv_counts, const uint64_t *stamp_base,
                              const uint64_t *sender_bucket_counts);
/* The same with n_senders (1..64) messages in the received arrays: recv_counts[n_senders], stamp_base[n_senders],
 * sender_bucket_counts[n_senders][512 / n_shards].  A rank that sends its records in parts (dbg_shard_extract_part, so that
 * the exchange of one part runs while the next is cut) counts as several senders with one stamp base. */
int dbg_shard_build_multipass_from(dbg_t *h, int k, int n_shards, int my_shard, int n_passes, int n_senders, const void *d_w0,
                                   const void *d_w1, const void *d_st, int stamp_bytes, const uint64_t *recv_counts,
                                   const uint64_t *stamp_base, const uint64_t *sender_bucket_counts);
int dbg_part_queries(dbg_t *h, int part, uint64_t *q_starts, uint64_t *q_counts, const void **d_q_keys);
int dbg_part_answer(dbg_t *h, int part, const void *d_q_keys, uint64_t n, void *d_answers);
int dbg_part_apply(dbg_t *h, int part, int owner, const void *d_answers);
int dbg_multipass_finish(dbg_t *h);

/* ---- traversal of a graph in parts (no reference counterpart for the partition; the steps are debruijn.py:150-186, :230-254,
 *      :274-278, :288-347): the per-part primitives of py-debruijn_amd/part_traversal.py, which moves the small id lists and
 *      rows they produce between parts and ranks.  A node is (virtual shard, local id).  Per part a byte of traversal flags
 *      in the DBG_F_* layout (INDEG, keep mask, BRANCH, PULLED) plus DBG_PF_MARK for the caller's marks. */
#define DBG_PF_MARK 0x80u
/* pruningEdges + branch flag on the part's CSR rows; threshold >= 1 */
int dbg_part_prune(dbg_t *h, int part, double threshold, uint64_t *n_branch);
/* local ids (uint32, device, ascending) of the nodes with (flags & mask) == want; d_ids NULL: *n only */
int dbg_part_select(dbg_t *h, int part, uint32_t mask, uint32_t want, void *d_ids, uint64_t capacity, uint64_t *n);
/* rows of n nodes (d_ids uint32, device); outputs are device arrays, any may be NULL: keys, keys_hi, stamps u64[n],
 * counts u32[n][4] by base code, succ_owner u8[n][4] (virtual shard; 0xFF none), succ_local u32[n][4], pflags u8[n] */
int dbg_part_gather(dbg_t *h, int part, const void *d_ids, uint64_t n, void *d_keys, void *d_keys_hi, void *d_stamps,
                    void *d_counts, void *d_succ_owner, void *d_succ_local, void *d_pflags);
/* ---- point queries on a graph in parts (the counterpart of dbg_lookup_nodes / dbg_score_sequences, which refuse such a
 *      graph): after dbg_build_multipass and dbg_shard_build_multipass[_from] (any n_passes, k <= 31 and k > 31), before and
 *      after dbg_multipass_finish, dbg_part_prune, the tip marks and dbg_part_segments.  The owner of a k-mer is a function
 *      of the key alone -- the top log2(n_virtual) bits of its minimizer's bucket hash -- so the kernel routes every query
 *      to its part and asks that part's directory (one table of part descriptors per handle, 144 B a part, built on the
 *      first query of a graph).  Rows of found nodes: dbg_part_gather.  DBG_E_ARG (text in dbg_last_error) for a handle
 *      without a graph in parts, for null pointers, and for a part that finished without a directory of the LDS engine
 *      (the text names the part).  n = 0 / n_seq = 0 return DBG_OK and touch nothing. */
/* owner[i] = virtual shard that owns k-mer i (0xFF: bits above 2k set); local[i] = its local id in that part if this handle
 * holds the part and the k-mer is a node, else DBG_NO_NODE.  keys_hi NULL = zeros. */
int dbg_part_lookup_nodes(dbg_t *h, const uint64_t *keys, const uint64_t *keys_hi, uint64_t n, uint8_t *owner, uint32_t *local);
int dbg_part_lookup_nodes_device(dbg_t *h, const void *d_keys, const void *d_keys_hi, uint64_t n, void *d_owner, void *d_local);
/* dbg_score_sequences over the windows whose k-mer THIS handle's parts own: a single-handle multi-pass graph gives the full
 * scores; on a rank of ranks x passes the sums over ranks are getScore and the minimum over ranks is first_missing.
 * A window whose k-mer another rank owns adds nothing and is not missing; a window that holds a character outside ACGT has
 * no owner and is missing on every handle.  offsets[0] == 0, offsets non-decreasing (DBG_E_ARG otherwise). */
int dbg_part_score_sequences(dbg_t *h, const char *chars, const uint64_t *offsets, uint64_t n_seq, uint64_t *scores, uint64_t *first_missing);
/* sets flag bits on n nodes; d_newly (u8[n], device, may be NULL) = 1 where the bits were not all set before */
int dbg_part_mark(dbg_t *h, int part, const void *d_ids, uint64_t n, uint32_t bits, void *d_newly);
int dbg_part_clear(dbg_t *h, int part, uint32_t bits); /* ... and clears them on every node */
/* kept edges of the part's chain nodes (not branch, not pulled, one kept successor) that leave the part: the targets'
 * local ids grouped by target virtual shard; counts[n_virtual]; d_targets (uint32, device) NULL: counts only */
int dbg_part_cross_targets(dbg_t *h, int part, uint64_t *counts, void *d_targets, uint64_t capacity);
/* one segment of the contig walk per entry node (d_entries uint32, device), inside the part.  kind u8[n]: 0 the path ends
 * at a branch node / a node without kept successor (emitted, that node included), 1 the entry itself is pulled, 2 the chain
 * leaves the part for (next_owner, next_local) -- then `last` holds the count of the leaving edge --, 3 a cycle inside the
 * part, 4 the next node is pulled (emitted up to the current one).  hops u32[n] = edges walked inside the part, score u64[n] =
 * sum of their counts, last u32[n] = node the segment ended at (kind 2: the leaving edge's count). */
int dbg_part_segments(dbg_t *h, int part, const void *d_entries, uint64_t n, void *d_kind, void *d_next_owner, void *d_next_local,
                      void *d_hops, void *d_score, void *d_last);
/* the characters n segments contribute to their contigs: for entry j, at [d_off[j], d_off[j + 1]) of d_chars, the last base of
 * the entry node and of each of the hops[j] nodes the segment appends (d_off[j + 1] - d_off[j] = 1 + hops[j], or 0 to skip);
 * device pointers, d_off uint64[n + 1] */
int dbg_part_segment_text(dbg_t *h, int part, const void *d_entries, uint64_t n, const void *d_off, void *d_chars, uint64_t capacity);
int dbg_part_pflags(dbg_t *h, int part, const void **d_pflags); /* device pointer of the flags, NULL before dbg_part_prune */
/* pull_out_read (debruijn.py:274-278) against an explicit list of k-mers (the branch k-mers of all parts and ranks): host
 * arrays in and out; read_flags[n_reads] = 1 where the read holds one; first_seen[n_keys][4] (may be NULL) = smallest byte
 * offset in this handle's reads of (k-mer, next base by code), UINT64_MAX if absent -- the Counter order of a branch node's
 * successors is count descending, then the minimum of these over all ranks */
int dbg_scan_reads_for_keys(dbg_t *h, int k, const uint64_t *keys, const uint64_t *keys_hi, uint64_t n_keys, uint8_t *read_flags,
                            uint64_t *first_seen);
/* successor ranks (the order bytes of dbg_export_orders) of the current graph, handed in instead of dbg_refine_edge_order */
int dbg_set_orders(dbg_t *h, const uint8_t *order);

/* ---- exact successor order (Counter semantics of debruijn.py:159-165 and :215-216): finds the first
 *      occurrence of every out-edge of the nodes with >= 2 distinct successors (one more pass over the
 *      reads) and rewrites the per-node rank bytes.  Without it equal-count successors are ranked
 *      A<C<G<T; sets, counts and degrees do not depend on it.  Call after dbg_build, before dbg_prune. */
int dbg_refine_edge_order(dbg_t *h);
/* order[n_nodes]: successor base codes, 2 bits each, rank 0 in bits 1:0: count descending, ties by first
 * appearance (== Counter.most_common); fsorder[n_nodes]: by first appearance (== Counter key order). */
int dbg_export_orders(dbg_t *h, uint8_t *order, uint8_t *fsorder);
/* Generic alphabet (max_degree == 32): order / fsorder are [n_nodes][32] bytes, one successor code per
 * rank, 0xFF beyond the out-degree; counts and succ of dbg_export_nodes / dbg_export_succ are [n_nodes][32]. */
/* codes32[code] = the byte a code stands for; bits per symbol 2 (ACGT) or 5 */
int dbg_get_alphabet(dbg_t *h, char *codes32, int *n_symbols, int *bits_per_symbol);
/* surviving successors after dbg_prune, bit `code` per node (both layouts) */
int dbg_export_keepmask(dbg_t *h, uint32_t *keepmask);
/* order[n_nodes]: node ids in the reference's dict order (ascending first-occurrence stamp, debruijn.py:120-133) --
 * the argsort of dbg_export_nodes' stamps, done by a device radix sort. */
int dbg_export_dict_order(dbg_t *h, uint32_t *order);

/* ---- a5 + a6: pruningEdges (debruijn.py:150-166) + branch detection (:230-236) */
int dbg_prune(dbg_t *h, double threshold);
/* ---- a7: tip removal (debruijn.py:169-186 driven by :241-254) */
int dbg_remove_tips(dbg_t *h);
/* ---- a9: reads that contain a branch k-mer (debruijn.py:274-278) */
int dbg_mark_pull_reads(dbg_t *h);
/* ---- a11 + a12: output_contigs / DFS (debruijn.py:288-347); scores are getScore
 *      (II_assembleFromReads.py:14-18).  final_mode != 0 walks with branch_kmer == []
 *      (debruijn.py:281-283).  max_chars bounds the materialised contig text (0 = 1 GiB). */
int dbg_walk(dbg_t *h, int final_mode, uint64_t max_chars);
/* Non-final walks of graphs with >= "walk_jump_min_nodes" nodes (dbg_set_option, default 2^14) resolve every
 * chain by pointer jumping (contigs overlap massively at scale); if the text would exceed max_chars
 * dbg_walk still returns DBG_OK with the contig index only (dbg_get_sizes: contigs_materialised == 0). */

int dbg_get_sizes(dbg_t *h, dbg_sizes_t *out);
int dbg_get_stats(dbg_t *h, dbg_stats_t *out);
/* Named event counters of the handle since dbg_create (they are not reset by a build):
 * "extract_presplit_fallbacks": builds whose pre-split extraction overflowed a sub-segment and ran again without the split.
 * "extract_presplit_rehists": builds whose level 1 took another width than the pre-split extraction had counted its
 *   records for, so that the level ran its histogram pass after all.
 * "ms_scatter_small" / "ms_scatter_wide": multisplit levels that ran the scatter kernel of a small fan-out (up to 64 children
 *   a group) / the wide one.
 * "refine_crowded" / "pull_crowded": dbg_refine_edge_order / dbg_mark_pull_reads calls (k <= 31) whose per-range kernel met a
 *   range with more multi-successor / branch nodes than it has slots for, so that the pass over the reads ran instead.
 * "resolve_direct_hits" / "resolve_keyed": cross-bucket successor queries (dbg_shard_answer's included) answered from the
 *   directory entry alone / after reading keys; counted only while option "resolve_count" is 1.
 * "lookup_dir_calls" / "lookup_index_calls": dbg_lookup_nodes[_device] / dbg_score_sequences calls answered through the
 *   build's directory / through the sorted index; "lookup_index_builds": sorts that built such an index (one per graph).
 * "part_lookup_calls": dbg_part_lookup_nodes[_device] / dbg_part_score_sequences calls that ran a kernel.
 * "count_events" and the other "count_*" counters describe the last build that ran an LDS count kernel (engine 0), not the
 *   handle's life; a multi-pass parent or a shard built in parts reports the OR / the sums over its parts.  "count_events": OR
 *   over the count launches of the rare paths a kernel took: 1 a bucket started in hash sub-ranges, 2 a table overflowed on a
 *   whole bucket and the bucket was split, 4 a table overflowed inside a sub-range, 8 a wave's list of pending edges overflowed
 *   (second-generation kernel, k <= 31), 16 a pass had more cross-range successors than its staging holds, 32 a wave deferred
 *   more successor lookups than its list holds (third-generation kernel, second two-word kernel).
 * "count_extra_ranges": sub-range passes of the last count launch (each adds a range and a directory block behind the buckets').
 * "count_retries_query_cap" / "count_retries_node_cap" / "count_retries_counter16": count launches repeated because the query
 *   list / the node and edge arrays sized from the estimate were too small / a 16-bit successor counter overflowed.
 * DBG_E_ARG for an unknown name. */
int dbg_get_counter(dbg_t *h, const char *name, uint64_t *out);

/* ---- exports: two-call pattern, sizes from dbg_get_sizes; NULL pointers are skipped */
/* keys[n_nodes], stamps[n_nodes], counts[n_nodes*4] (by base code), flags[n_nodes]; table order */
int dbg_export_nodes(dbg_t *h, uint64_t *keys, uint64_t *stamps, uint32_t *counts, uint8_t *flags);
/* k > 31: a k-mer is the 2k-bit number keys_hi[i] * 2^64 + keys[i] (first base in the top bit pair);
 * keys_hi[n_nodes] is all zero for k <= 31. */
int dbg_export_keys_hi(dbg_t *h, uint64_t *keys_hi);
/* succ[n_nodes*4]: node id of successor by base code or DBG_NO_NODE */
int dbg_export_succ(dbg_t *h, uint32_t *succ);
/* CSR over distinct edges: row_ptr[n_nodes+1], col[n_edges], cnt[n_edges] */
int dbg_export_csr(dbg_t *h, uint64_t *row_ptr, uint32_t *col, uint32_t *cnt);
/* ranks[n_nodes]: pull order key of pulled nodes (ascending == append order of
 * already_pull_out, debruijn.py:253), UINT64_MAX for the rest */
int dbg_export_pull_ranks(dbg_t *h, uint64_t *ranks);
/* The two short label lists of construct_graph without anything of size n_nodes leaving the device: the nodes that
 * carry `flag` -- DBG_F_PULLED in pull order (already_pull_out, debruijn.py:253) or DBG_F_BRANCH in dict order
 * (branch_kmer, debruijn.py:230-236) -- as rows[*n_out] (node ids), keys[*n_out], keys_hi[*n_out] (zeros for
 * k <= 32).  *n_out is always set (rows == NULL: count only); DBG_E_CAPACITY if capacity < *n_out. */
int dbg_export_marked(dbg_t *h, uint32_t flag, uint64_t capacity, uint64_t *n_out, uint32_t *rows, uint64_t *keys,
                      uint64_t *keys_hi);
int dbg_export_pull_reads(dbg_t *h, uint8_t *read_flags /* [n_reads] */);
/* contigs in emission order grouped by start: offsets[n_contigs+1] into chars[contig_chars],
 * scores[n_contigs], start_stamp[n_contigs] (stamp of the start node: sort key for dict order),
 * seq_in_start[n_contigs] (emission index within its start) */
int dbg_export_contigs(dbg_t *h, uint64_t *offsets, char *chars, uint64_t *scores, uint64_t *start_stamp,
                       uint32_t *seq_in_start);
/* the same without the text: offsets[n_contigs+1] (contig i has offsets[i+1]-offsets[i] characters) */
int dbg_export_contig_index(dbg_t *h, uint64_t *offsets, uint64_t *scores, uint64_t *start_stamp, uint32_t *seq_in_start);
/* f2: contig sort + FASTA text on the device (II_assembleFromReads.py:64-69).  The contigs of the last materialised walk,
 * sorted by score descending and stable like `sequences.sort(key=getScore, reverse=True)`, as the text the driver
 * writes: ">SEQUENCE_{i}_{k}mer\n{contig}\n" per contig.  *bytes receives the size of the text (call with buf == NULL to
 * ask for it); order_out (may be NULL): [n_contigs] index of the contig at every output position, indices as in
 * dbg_export_contigs.  The same bytes as dbg_write_contigs_fasta with indices NULL writes, but the whole text is held on
 * the device for the one copy; dbg_contig_output_stats is not touched. */
int dbg_export_sorted_fasta(dbg_t *h, uint32_t *order_out, char *buf, uint64_t buf_len, uint64_t *bytes);
/* Text of ONE contig (buf_len >= its length from the index): what a caller uses when dbg_walk kept the index only
 * because the whole text exceeds max_chars (contigs overlap massively at scale).  The first call after a walk builds
 * the binary-lifting tables of the chain successors (n_nodes x ceil(log2(n_nodes + k)) x 4 bytes, shared with
 * dbg_export_contig_texts and dbg_write_contigs_fasta; refused above 64 GiB), later calls are one small kernel each
 * (one thread per character).  After a materialised walk the call is a copy out of the walk's text. */
int dbg_export_contig_text(dbg_t *h, uint64_t index, char *buf, uint64_t buf_len);
/* Contig text in bulk, after any walk that left an index: a materialised one, or an index-only one of the list-ranking
 * path (an index-only final-mode walk has no per-contig start nodes: DBG_E_ARG).  One kernel fills a window of the output
 * at a time (chunk_bytes, a multiple of 4096; 0 = library default, 4 MiB; option "ctgout_chunk_bytes" changes that
 * default) into one of two device staging buffers; the window goes to one of two pinned host buffers, and the host writes
 * window c (or copies it into the caller's buffer) while window c + 1 is filled and copied.  Neither side ever holds the
 * whole text; the device holds 2 * chunk_bytes + 24 * (n + 1) bytes + 1 MiB at most besides the walk's own arrays
 * (dbg_contig_output_stats names the one condition: the sort library's scratch for the driver's order).  An index >= n_contigs is DBG_E_ARG. */
/* texts of n contigs of the last walk (indices into dbg_export_contig_index, any order, repeats allowed), concatenated:
 * two-call pattern of dbg_take_reads -- out_offsets[n + 1] (may be NULL) and *n_chars are always set; out_chars NULL:
 * sizes only, else capacity >= *n_chars (DBG_E_CAPACITY otherwise). */
int dbg_export_contig_texts(dbg_t *h, const uint64_t *indices, uint64_t n, uint64_t *out_offsets, char *out_chars,
                            uint64_t capacity, uint64_t *n_chars);
/* ">SEQUENCE_{first_number + i}_{k_label}mer\n{contig}\n" for i in 0..n-1 written to `path` (append != 0: appended,
 * else truncated).  indices NULL: every contig in the driver's order (score descending, stable over the emission order --
 * the order of dbg_export_sorted_fasta); k_label 0: the graph's k.  DBG_E_ARG (text in dbg_last_error) for a path that
 * cannot be opened for writing and for a chunk_bytes that is no multiple of 4096; n = 0 writes nothing. */
int dbg_write_contigs_fasta(dbg_t *h, const char *path, int append, const uint64_t *indices, uint64_t n,
                            uint64_t first_number, int k_label, uint64_t chunk_bytes, uint64_t *bytes_written);
/* dbg_write_contigs_fasta with the contig of every record in lines of line_width characters, each ended by '\n' (the last
 * line may be shorter).  A contig of 0 characters still gets its one '\n'; a contig whose length is a multiple of
 * line_width gets no extra empty line: the body of a record takes len + max(1, ceil(len / line_width)) bytes.
 * line_width 0: one line per contig, exactly the bytes of dbg_write_contigs_fasta (which is this call with 0). */
int dbg_write_contigs_fasta_wrapped(dbg_t *h, const char *path, int append, const uint64_t *indices, uint64_t n,
                                    uint64_t first_number, int k_label, uint64_t chunk_bytes, uint32_t line_width,
                                    uint64_t *bytes_written);
int dbg_contig_output_stats(dbg_t *h, dbg_contig_out_stats_t *out);
/* ---- the same two outputs for the walk over a graph in parts (csrc/dbg_partout.h).  The caller ranks the skeleton of
 *      segments (one row per entry node, sorted by global id = virtual shard << 32 | local id) and hands it over once:
 *      device pointers, d_gid int64[n], d_next int64[n] (row index of the entry the segment hands over to), d_go_on
 *      uint8[n] (0 / 1), d_hops int64[n], d_rest uint64[n] with rest = hops + go_on * (1 + rest[next]) -- the characters
 *      the chain appends from the entry to its end -- or UINT64_MAX where no contig can start (dead or unresolved).  The
 *      library validates every row in a kernel before anything walks them (gid strictly ascending and inside the build's
 *      virtual shards, next < n, local ids of the parts it holds below their n_nodes, hops within 32 bits, the rest
 *      recurrence; DBG_E_ARG names what failed and nothing is kept), copies the rows (26 B a row), notes for each which of
 *      its parts holds it, and builds the binary-lifting table up[l][i] (4 B a row and level; levels = the smallest count
 *      with 2^levels - 1 >= the jumps of the longest chain).  The copy belongs to the graph: the next build, the next
 *      dbg_part_set_skeleton (also a refused one) and dbg_destroy free it.  More than 2^32 - 1 rows: DBG_E_ARG.
 *      dbg_part_prune must have run on every non-empty part. */
int dbg_part_set_skeleton(dbg_t *h, uint64_t n_entries, const void *d_gid, const void *d_next, const void *d_go_on,
                          const void *d_hops, const void *d_rest);
/* Bytes [b0, b1) of the virtual text of n records -- record i is the contig that starts at skeleton row d_starts[i]
 * (uint64[n], device; k + rest characters), bare (fasta 0: the texts concatenated) or as the FASTA records of
 * dbg_write_contigs_fasta -- into d_out (device, 16-byte aligned, room for b1 - b0 rounded up to 16).  Characters of
 * segments, and of start k-mers, in virtual shards this handle does not hold are the byte 0; headers and newlines are
 * written by every handle: the bytewise maximum over the handles of a build is the text.  *total (may be NULL) receives
 * the size of the whole text; b1 is cut to it; d_out NULL or b0 >= b1: sizes only.  b0 is a multiple of 4096, a window
 * holds 1 GiB at most. */
int dbg_part_contig_window(dbg_t *h, const void *d_starts, uint64_t n, int fasta, uint64_t first_number, int k_label, uint64_t b0,
                           uint64_t b1, void *d_out, uint64_t *total);
/* dbg_export_contig_texts / dbg_write_contigs_fasta with skeleton rows for contig indices (host arrays, the same streaming
 * and dbg_contig_output_stats; peak_device_bytes includes the skeleton's copy and table).  Every chain listed must lie in
 * parts of this handle (DBG_E_ARG otherwise: use dbg_part_contig_window on every rank).  DBG_E_ARG also for: no skeleton
 * set for the current graph, a start >= n_entries or without rest, chunk_bytes no multiple of 4096, a path that cannot be
 * opened.  n = 0 returns DBG_OK and touches nothing (not the file either); a refused call leaves the handle usable. */
int dbg_part_export_contig_texts(dbg_t *h, const uint64_t *starts, uint64_t n, uint64_t *out_offsets, char *out_chars,
                                 uint64_t capacity, uint64_t *n_chars);
int dbg_part_write_contigs_fasta(dbg_t *h, const char *path, int append, const uint64_t *starts, uint64_t n,
                                 uint64_t first_number, int k_label, uint64_t chunk_bytes, uint64_t *bytes_written);
/* ---- final-mode walk (debruijn.py:288-316 with branch_kmer == [], the driver's last k) over a graph in parts
 *      (csrc/dbg_partfinal.h).  The caller contracts the graph: one row per entry node of the ranked skeleton -- the
 *      starts, the targets of chain edges that leave a part and every kept successor of a branch node -- and one row of a
 *      branch table per branch node of the whole graph.  All pointers are device arrays:
 *        d_kind    uint8[n_entries]   0 the chain ends at a node without kept successor (emitted, that node included)
 *                                     1 the entry itself is pulled
 *                                     2 the chain ends in front of a pulled node (emitted up to the node before it)
 *                                     3 dead: the chain closes on itself or never resolved
 *                                     4 the chain ends at the branch node of branch-table row d_branch[i]
 *        d_append  uint64[n_entries]  nodes the chain appends after the entry (the skeleton's rest; kinds 0, 2, 4)
 *        d_score   uint64[n_entries]  sum of the edge counts along them
 *        d_branch  uint32[n_entries]  read where the kind is 4
 *        d_succ_row / d_succ_count    uint32[n_branch * 4]: per branch node the entry rows of its KEPT successors in
 *                                     Counter.most_common order (debruijn.py:159-165) and the counts of the edges to them;
 *                                     DBG_NO_NODE: an empty slot
 *        d_starts  uint32[n_starts]   entry rows of the nodes with indegree 0 in dict order
 *      One kernel validates all of it first (kinds in range, branch rows below n_branch, successor rows below n_entries
 *      or DBG_NO_NODE, starts below n_entries): DBG_E_ARG names what failed and no walk ran.  Then one walker per thread
 *      enumerates every simple path of every start in two passes (count, scan, write).  A walker holds a stack of
 *      n_branch + 1 levels of 24 bytes and n_branch bits -- only branch nodes need an on-path mark -- interleaved with the
 *      other walkers'; their number follows dbg_walk's rule (4 GiB of stacks, 2^16 at most), and walker w takes the
 *      starts w, w + walkers, ...  Every walker counts its steps over all its starts -- a step is one trip of its loop: one
 *      successor slot tried (used or empty) or one level popped, so 5 for every branch level it pushes --: above option "part_final_walk_steps" (dbg_set_option, default 2^24 per walker and pass -- a step measured 1.3 us, a refusal 22 s --, at least 1) the call
 *      stops with DBG_E_CAPACITY, keeps nothing and the handle stays usable.  max_chars (0 = 1 GiB) is checked after the
 *      counting pass like dbg_walk's: DBG_E_CAPACITY with valid sizes, nothing written.
 *      *n_contigs, *n_pieces (rows over all contigs) and *n_chars (sum of the contig lengths) are always set.
 *      n_starts == 0 or n_entries == 0: DBG_OK with zeros.  A handle without a graph in parts: DBG_E_ARG.  The result
 *      belongs to the handle's current graph: the next build, the next final walk and dbg_destroy free it. */
typedef struct dbg_final_skeleton {
    uint64_t n_entries, n_branch, n_starts;
    const void *d_kind, *d_append, *d_score, *d_branch, *d_succ_row, *d_succ_count, *d_starts;
} dbg_final_skeleton_t;
int dbg_part_final_walk(dbg_t *h, const dbg_final_skeleton_t *s, uint64_t max_chars, uint64_t *n_contigs, uint64_t *n_pieces,
                        uint64_t *n_chars);
/* The index of the last final walk to caller-owned host arrays (NULL pointers are skipped): per contig the ordinal of its
 * start in d_starts, its ordinal within that start (contigs come grouped by start, in DFS order), its length
 * k + nodes - 1 and its score (the sum of the edge counts along the path); piece_off[n_contigs + 1] into
 * piece_row[n_pieces], the entry rows the path is made of.  The text of a contig is the text of its first piece followed
 * by every later piece's text without its first k - 1 characters.  DBG_E_ARG without a walk, or after one that kept its
 * sizes only. */
int dbg_part_final_export(dbg_t *h, uint32_t *start_ordinal, uint32_t *seq, uint64_t *length, uint64_t *score,
                          uint64_t *piece_off, uint32_t *piece_row);
/* device-side views for callers that stay on the GPU (valid until the next build/destroy) */
int dbg_device_views(dbg_t *h, const void **d_keys, const void **d_counts, const void **d_stamps,
                     const void **d_flags, const void **d_succ);

/* ---- point queries on the current graph (the reference asks its dicts: `kmer in vertices`, `edges[kmer]`,
 *      `edge_count_table[edge]`, getScore): answered on the device, nothing of size n_nodes moves.
 *      They work on the graph of dbg_build (both engines, ACGT at k = 1..63; any other alphabet at k <= 11),
 *      dbg_build_from_walk(s) and dbg_import_graph, before and after prune, tips and walk.  DBG_E_ARG (text in
 *      dbg_last_error) without a graph, for a graph in parts (dbg_build_multipass: ask dbg_part_lookup_nodes /
 *      dbg_part_score_sequences instead), for one shard of several, and for the
 *      generic alphabet at k >= 12, whose nodes have no packed key.  n = 0 returns DBG_OK and touches nothing.
 *      Two ways to a node, same answers: where the handle still holds the directory of the build that made the graph (a
 *      single-GPU dbg_build on the partitioned engines, k <= 31 and k > 31) a query costs its bucket hash, one directory
 *      entry and one run of keys, and no memory.  Every other graph (engine 1, "wide_engine" 0, generic, from walks,
 *      imported) gets a sorted index on the first lookup: one device radix sort of (keys_hi, keys, id), 12 B per node
 *      (20 B for two-word keys) kept until the next build, import, change of reads or dbg_destroy, plus the same again as
 *      scratch while it is sorted; a query is then a binary search. */
/* node id (row in table order, as in dbg_export_nodes) of n k-mers, DBG_NO_NODE where the k-mer is no node.
 * keys_hi NULL = all zero; for k <= 31 a non-zero keys_hi[i], or key bits above 2k (5k), mean "absent". */
int dbg_lookup_nodes(dbg_t *h, const uint64_t *keys, const uint64_t *keys_hi, uint64_t n, uint32_t *ids);
int dbg_lookup_nodes_device(dbg_t *h, const void *d_keys, const void *d_keys_hi, uint64_t n, void *d_ids);
/* rows of n nodes, any output may be NULL: keys, keys_hi, stamps u64[n]; counts u32[n][D]; flags u8[n];
 * keepmask u32[n]; order / fsorder u8[n] (D == 4) or u8[n][32] (D == 32) -- the same values the whole-graph
 * exports give at those rows (and their preconditions: keepmask after dbg_prune, fsorder of ACGT graphs after
 * dbg_refine_edge_order).  DBG_E_ARG for an id >= n_nodes. */
int dbg_gather_nodes(dbg_t *h, const uint32_t *ids, uint64_t n, uint64_t *keys, uint64_t *keys_hi, uint64_t *stamps,
                     uint32_t *counts, uint8_t *flags, uint32_t *keepmask, uint8_t *order, uint8_t *fsorder);
/* getScore (II_assembleFromReads.py:14-18) of n_seq sequences (chars + offsets[n_seq + 1], host): scores[s] = sum over
 * i in [0, len - k) of count(seq[i : i + k + 1]); first_missing[s] = smallest i whose (k+1)-mer is no edge of the graph
 * (the reference raises KeyError there), UINT64_MAX if none -- then scores[s] is the reference's value.  A sequence of
 * len <= k scores 0.  A character outside the graph's alphabet makes every window that holds it missing.
 * The text goes to the device once; the work is split over the windows of the concatenated text, not over sequences. */
int dbg_score_sequences(dbg_t *h, const char *chars, const uint64_t *offsets, uint64_t n_seq, uint64_t *scores,
                        uint64_t *first_missing);

/* ---- whole-graph statistics on the device (csrc/dbg_spectrum.h): the numbers someone with real reads looks at first, and
 *      how `threshold` is chosen (pruningEdges keeps a successor whose count is at least maxCount / threshold).  One
 *      read-only pass over the counts the graph already holds; nothing of size n_nodes moves or is allocated.  All in the
 *      reference's terms, for the graph construct_graph(reads, k) builds, before pruning:
 *        edge spectrum   E[c] = number of (k+1)-mers e with edge_count_table[e] == c.  A build at k counts (k+1)-mers, so
 *                        this is the exact (k+1)-mer abundance spectrum of the reads: for the 31-mer spectrum build at k = 30.
 *        out-weight      W[c] = number of nodes whose successor counts sum to c (len(edges[v]) before pruningEdges); W[0]
 *                        counts the nodes without a successor.  The sum is the number of windows that START at the k-mer:
 *                        it is NOT the k-mer's multiplicity, because the last k-mer of a read is not counted.
 *        out-degree      D[d] = number of nodes with d distinct successors (Node.outdegree): 0..4 on ACGT graphs, 0..32 on
 *                        generic ones.
 *        kept degree     K[d] = number of nodes with d bits set in the keep mask, over all nodes (pulled ones included):
 *                        valid after dbg_prune (in parts: after dbg_part_prune on every part that has nodes; a part not
 *                        yet pruned adds nothing).  Before that K is all zero and pruned == 0.
 *      Binning: with n_bins = B a count c lands in bin min(c, B - 1): the last bin collects everything at or above B - 1.
 *      edge_hist[0] is always 0.  The bins are zeroed by every call.
 *      The host statement of all this is debruijn.count_spectrum on plain dicts (py-debruijn_amd/debruijn.py). */
typedef struct dbg_spectrum {
    uint64_t n_nodes;          /* nodes looked at */
    uint64_t n_edges;          /* distinct (k+1)-mers = sum of E */
    uint64_t sum_edge_counts;  /* sum of c * E[c] without the clamp; on a whole single graph dbg_sizes_t.n_edge_instances */
    uint64_t max_edge_count;
    uint64_t max_out_weight;
    uint64_t D[33];
    uint64_t K[33];
    uint64_t pruned;           /* 1: K is valid */
    uint64_t n_bins;
    uint64_t peak_extra_device_bytes; /* the one allocation of the call: the bins and the summary, 16 * n_bins + 560 */
    double ms_kernel;          /* the memset of the bins and the kernels, by events on the handle's stream */
} dbg_spectrum_t;
/* part < 0: the handle's whole graph -- the single graph, or the sum over every part it holds (maxima: the maximum);
 * part >= 0: that part of a graph in parts.  edge_hist / node_hist: [n_bins] host arrays, either may be NULL (summary
 * only); out may be NULL.  Works on every graph a handle can hold (dbg_build on every engine and alphabet, dbg_import_graph,
 * dbg_build_from_walk(s), dbg_build_multipass, dbg_shard_build_multipass[_from], a shard after dbg_shard_apply), before and
 * after prune, tips, pull reads and walk, and changes nothing the other calls read.  A graph with 0 nodes: DBG_OK, zeros.
 * DBG_E_ARG (text in dbg_last_error, the handle stays usable) for: no graph; n_bins < 2 or > 2^20; part >= dbg_part_count;
 * part >= 0 on a single graph; a handle on which dbg_shard_build has run and dbg_shard_apply has not run since (for any
 * n_shards: the shard's successors are still open). */
int dbg_count_spectrum(dbg_t *h, int part, uint64_t n_bins, uint64_t *edge_hist, uint64_t *node_hist, dbg_spectrum_t *out);

/* ---- multi-GPU: hash-prefix sharding (no reference counterpart: the reference is one process).
 *      One handle per rank; the caller moves the buffers between ranks (RCCL all-to-all).  Owner
 *      shard of a k-mer = top log2(n_shards) bits of its minimizer bucket hash; n_shards in {1,2,4,8}.
 *      After dbg_shard_apply the handle holds the shard's nodes; successor ids are
 *      (owner shard << 29) | node id on that shard; stamps are global ((byte offset in the
 *      rank-major concatenation of all reads) << 1 | pos != 0). */
/* step 1: this rank's reads -> super-k-mer records grouped by owner (device arrays: w0, w1 uint64,
 * st = rank-local stamps: k <= 31: uint32 while this rank's reads stay below 2 GiB, else uint64 -- dbg_shard_record_layout
 * says which; k > 31 on the LDS engine: always uint32 on the wire, and from 2 GiB of reads on bits 61..32 of the stamp ride
 * in bits 63..34 of the record's meta word (zero below 2 GiB, so the messages are those of a narrow rank); the option
 * "shard_stamp64" 1 forces the wide path at any size.  k > 31 on the global-table engine ("wide_engine" 0): reads below
 * 2 GiB only); send_counts[n_shards] records go to each owner, contiguous and in owner order */
int dbg_shard_extract(dbg_t *h, int k, int n_shards, uint64_t *send_counts, const void **d_w0, const void **d_w1,
                      const void **d_st);
/* dbg_shard_extract for part `part` of n_parts (1..4) slices of this rank's reads (k <= 31: super-k-mer records; k > 31: the
 * records by value of the LDS engine, stamps as for dbg_shard_extract): slices of the position space cut at
 * tile borders -- a k-mer belongs to the slice its first base lies in, so the parts' records together are exactly those of
 * dbg_shard_extract; the stamps are positions in ALL of the rank's reads either way.  The arrays of part p stay valid until
 * part p is extracted again (own buffers per part): multi_gpu.sharded_build_multipass(chunks=...) has part p on the wire
 * while part p + 1 is cut.  dbg_shard_bucket_counts / dbg_shard_record_layout describe the last part extracted. */
int dbg_shard_extract_part(dbg_t *h, int k, int n_shards, int part, int n_parts, uint64_t *send_counts, const void **d_w0,
                           const void **d_w1, const void **d_st);
/* What the last dbg_shard_extract handed out: *w0_words = 64-bit words per record in d_w0 (1: super-k-mer records of
 * k <= 31, or the low key word of the k-mer instances of k > 31 with "wide_engine" 0; 4: the aligned bases of a
 * super-k-mer record of k > 31), *stamp_bytes = bytes per entry of d_st (4; 8 for the instance tuples and for
 * k <= 31 records of a rank that holds 2 GiB of reads or more; the records of k > 31 stay at 4 at any size, their wider
 * stamps continue in the meta word).  The exchange moves counts[d] x words elements of d_w0;
 * all senders of one dbg_shard_build must use ONE stamp width (a rank with 4-byte stamps zero-extends them when another
 * rank has 8: multi_gpu.sharded_build). */
int dbg_shard_record_layout(dbg_t *h, int *w0_words, int *stamp_bytes);
/* records per level-1 bucket (the 512 top-9-bit groups of the bucket hash) of the last dbg_shard_extract (k <= 31, and k > 31 on the LDS engine):
 * owner d holds the buckets [d * 512 / n_shards, (d + 1) * 512 / n_shards), in order, so send_counts[d] is their sum */
int dbg_shard_bucket_counts(dbg_t *h, uint64_t *counts512);
/* step 2: records received from rank r are recv_counts[r] consecutive entries (rank order);
 * stamp_base[r] = bytes of reads held by ranks < r.  Builds the shard's node table.  Successor
 * k-mers owned by other shards: device array *d_q_keys (uint64), group of owner d at
 * [q_starts[d], q_starts[d] + q_counts[d]).
 * sender_bucket_counts: NULL, or [n_shards][512 / n_shards] -- for every sender its dbg_shard_bucket_counts entries of
 * the buckets THIS shard owns.  With it the receiver skips the first multisplit level (the senders did it before the
 * exchange) and rebases the stamps inside the second one.
 * stamp_bytes: width of the entries of d_st32 -- 0 = the layout's default (4; 8 for k-mer instance tuples), 4, or 8
 * (k <= 31 with sender_bucket_counts: senders that hold 2 GiB of reads or more).  The records of k > 31 (LDS engine) come
 * with 4-byte stamps from every sender: the second multisplit level joins the high bits their meta words carry. */
int dbg_shard_build(dbg_t *h, int k, int n_shards, int my_shard, const void *d_w0, const void *d_w1, const void *d_st32,
                    const uint64_t *recv_counts, const uint64_t *stamp_base, uint64_t *q_starts, uint64_t *q_counts,
                    const void **d_q_keys, const uint64_t *sender_bucket_counts, int stamp_bytes);
/* step 3: node ids (uint32, device) of n successor k-mers other ranks asked this shard about */
int dbg_shard_answer(dbg_t *h, const void *d_q_keys, uint64_t n, void *d_answers);
/* step 4: d_answers (uint32, device) laid out like *d_q_keys of step 2; completes successors + CSR */
int dbg_shard_apply(dbg_t *h, const void *d_answers);
/* Traversal after a sharded build ("gather first"): the shards' node arrays, concatenated in shard
 * order on one GPU (device pointers: keys u64[n], stamps u64[n], counts u32[n][4], succ u32[n][4] with ids
 * (owner << 29) | id), become the graph of handle `h`, whose reads must be the rank-major concatenation of all
 * ranks' reads (the global stamps index into it).  Successor ids are rewritten to positions in the concatenation;
 * the arrays are BORROWED, not copied (they are most of the memory of the gathered graph): keep them alive and do
 * not touch them while this handle uses the graph; d_succ is rewritten in place.
 * Afterwards the handle is what dbg_build would have produced on the whole read set (node order aside):
 * dbg_refine_edge_order, dbg_prune, dbg_remove_tips, dbg_mark_pull_reads, dbg_walk and the exports apply. */
int dbg_import_graph(dbg_t *h, int k, int n_shards, const uint64_t *shard_nodes, const void *d_keys,
                     const void *d_keys_hi, const void *d_stamps, const void *d_counts, const void *d_succ);
/* k > 31 (two-word k-mers): d_keys_hi is required and d_succ is ignored -- the shards of such a build carry keys,
 * stamps and counts only (the k-mer INSTANCES travel between ranks, dbg_shard_extract / dbg_shard_build take and
 * return (lo, hi | next base << 62, local stamp | has-successor << 32) u64 triples and there are no successor
 * queries); dbg_import_graph resolves every successor with one table over the gathered nodes.
 * k <= 31: d_keys_hi may be NULL. */
/* device pointer of the upper key words (NULL for k <= 31) */
int dbg_device_keys_hi(dbg_t *h, const void **d_keys_hi);

/* ---- the driver's next k (II_assembleFromReads.py:56-75: build at k, walk, sort the contigs, append the pull-out reads,
 *      build at k+1 from those): the k1 = k + 1 graph of (the contigs of src's last walk, in `order`) followed by the
 *      n_extra reads extra_bases / extra_offsets[n_extra + 1], built into the fresh handle dst from the chain structure of
 *      src's graph -- no contig is ever spelled.  order[n_order]: contig indices (dbg_export_contig_index) in driver order,
 *      a permutation of 0..n_contigs-1.  src is read-only and stays valid; dst must live on the same device.
 *      Afterwards dst is what dbg_build(k1) would have produced on the spelled-out reads: same nodes, keys, counts, stamps
 *      (offsets in that concatenation, T = the contigs' characters, then the extra reads) and flags, node order aside; the
 *      successor ranks are already exact (dbg_refine_edge_order leaves them); dbg_prune, dbg_remove_tips,
 *      dbg_mark_pull_reads, dbg_walk and every export apply.  dbg_export_pull_reads reports n_order + n_extra reads
 *      (contigs first), dbg_get_sizes n_reads = n_order + n_extra and n_bytes = T + the extra bytes.
 *      DBG_E_ARG (text in dbg_last_error) for: no walk of src's current graph, a final-mode walk, a generic alphabet, a graph
 *      in parts, k1 > 63 or k1 != k + 1, an order that is not a permutation of the contig index. */
int dbg_build_from_walk(dbg_t *dst, dbg_t *src, int k1, const uint64_t *order, uint64_t n_order, const char *extra_bases,
                        const uint64_t *extra_offsets, uint64_t n_extra);

/* ---- the same from several walks: from the driver's third k on, its reads are the contigs of the previous walk, then
 *      the pulled contigs of every earlier walk that are still pulled (one block per walk, newest first), then a few real
 *      reads.  Each block names contigs of a graph that is still on the device, so the k1-graph is built from all of them:
 *      the reads of dst are the contigs of block 0, of block 1, ..., then the extra reads; no contig is spelled.
 *      A block may hold any subset of its source's contigs (the empty one included), k1 - k(src) may be any value >= 1,
 *      and the sources need no relation to each other.  Afterwards dst is what dbg_build(k1) would have produced on the
 *      spelled-out concatenation (node order aside, successor ranks exact), everything said for dbg_build_from_walk
 *      applies, and dst may itself be a source of a later call.  dbg_export_pull_reads reports sum(n) + n_extra flags in
 *      read order, dbg_get_sizes the virtual n_reads / n_bytes.  dst keeps 8 B per source node + 4 B per contig of every
 *      block for dbg_mark_pull_reads; the chain scratch of a block (about 57 B per source node) is freed before the next
 *      block starts.
 *      DBG_E_ARG (text in dbg_last_error(dst); every handle stays usable) for: the same src in two blocks or dst among the
 *      sources, a source on another device, without a walk of its current graph, with a final-mode walk, in parts, with
 *      a generic alphabet or with k(src) >= k1, k1 > 63, a contig index out of range or named twice within a block.
 *      DBG_E_ALPHABET for extra reads outside ACGT. */
typedef struct dbg_walk_block {
    dbg_t *src;              /* graph whose last non-final walk holds these contigs; k(src) < k1 */
    const uint64_t *contigs; /* n indices into src's contig index (dbg_export_contig_index), all different; read order */
    uint64_t n;
} dbg_walk_block_t;
int dbg_build_from_walks(dbg_t *dst, int k1, const dbg_walk_block_t *blocks, uint64_t n_blocks, const char *extra_bases,
                         const uint64_t *extra_offsets, uint64_t n_extra);

/* ---- f4: read-support scores of contigs (findSupportReadScore, IV_sortOutputs.py:10-15): out_scores[c] = sum of
 *      read_scores[r] over the reads r (distinct strings: the reference's dict keys) that occur in contig c as a
 *      substring, added in ascending r from 0.0 -- the reference's order, so double sums equal the reference's bit for
 *      bit; an empty read occurs in every contig.  read_is_float (may be NULL = all): 1 where the reference's score
 *      is a Python float; out_float_hits[c] (may be NULL) counts the float-typed reads found in c (0: the reference's
 *      result is an int).  All pointers are host pointers; reads / contigs are concatenated characters + offsets[n + 1].
 *      Uses the handle's device only; its reads and graph are untouched. */
int dbg_support_read_scores(dbg_t *h, const char *read_chars, const uint64_t *read_off, uint64_t n_reads,
                            const double *read_scores, const uint8_t *read_is_float, const char *contig_chars,
                            const uint64_t *contig_off, uint64_t n_contigs, double *out_scores, uint32_t *out_float_hits);

#ifdef __cplusplus
}
#endif
#endif /* DBG_H */
