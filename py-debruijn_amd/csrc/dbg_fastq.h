// Chunked FASTQ ingest (dbg_set_reads_fastq_file): strict four-line records through the chunk pipeline it shares with
// the FASTA stream (dbg_hip_reads.h), with an optional quality mask.
//
// Lines are the project's universal-newline lines.  Line g of the range (counted from its first record) is a header
// (g % 4 == 0), a sequence (1), a separator (2) or a quality line (3): the kind of a byte is a COUNT of line starts, not a
// "nearest event", so a popcount prefix of the line starts runs first (k_fq_blocks per 64 KiB block, k_fq_carry across the
// blocks, the stream state across the chunks).  After that the parse is the per-byte one of the FASTA path, for two line
// kinds and with two cursors: a byte of a sequence or quality line is written iff a non-space byte follows it in its line
// (rstrip), its place is the number of written bytes of its kind before it, and the trailing white space of the line open
// at the chunk end is written speculatively ("pending").  Read index = record index = g / 4: an offset is written at every
// sequence-line start.
//
// Validation sits at the line starts (k_fq_write): a header without '@', a separator without '+', a sequence that starts
// with '@' or '+', and at every header but the first "kept sequence bytes so far != kept quality bytes so far" -- both are
// prefix sums the kernel has.  Every violation goes through one atomicMin on (record, kind); the host looks at it at its
// per-chunk synchronise.  The end of the range (a last record without its quality line, a record cut short) is the host's,
// from the stream state.
//
// With a mask the quality bytes go to a second packed buffer at the same places as the bases, and k_fq_mask turns base j
// into 'N' where qual[j] - 33 < min_quality after the last chunk, 16 bytes a thread.
//
// Per chunk of n bytes the device holds the text (n + 64), three u32 masks, one u32 line count and one u64 rank per 32-byte
// word (0.75 n) and 5 bytes per 64 KiB block: ~1.75 n.
//
// The word helpers, the record-start search and the trailing-white-space trim are plain C++: a host compiler can include
// this file alone (tests/fastq_host.cpp does).
#pragma once
#include <stdint.h>

#ifndef DBG_FQ_HD
#if defined(__HIPCC__)
#define DBG_FQ_HD __host__ __device__
#else
#define DBG_FQ_HD
#endif
#endif

namespace dbgk {

// kinds of a malformed file, in the order a record is checked; an error key is record * 8 + kind
enum : uint32_t { FQ_E_HEADER = 0, FQ_E_SEQ_START = 1, FQ_E_SEPARATOR = 2, FQ_E_LENGTH = 3, FQ_E_TRUNCATED = 4, FQ_E_QUALITY = 5 };
constexpr uint64_t FQ_NO_ERROR = ~0ull;

DBG_FQ_HD inline const char *fq_kind_name(uint32_t kind) {
    switch (kind) {
        case FQ_E_HEADER: return "header";
        case FQ_E_SEQ_START: return "sequence start";
        case FQ_E_SEPARATOR: return "separator";
        case FQ_E_LENGTH: return "length mismatch";
        case FQ_E_TRUNCATED: return "truncated record";
        default: return "quality byte";
    }
}

DBG_FQ_HD inline bool fq_space(uint32_t c) {  // str.isspace() over the ASCII range (fs_space of dbg_fasta.h)
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31);
}

DBG_FQ_HD inline bool fq_line_start(uint32_t prev, uint32_t c) { return prev == '\n' || (prev == '\r' && c != '\n'); }

// masks of a 32-byte word (v: eight little-endian dwords) over its first nb bytes: ls = line starts, ns = non-space bytes.
// prev: the byte before the word.
DBG_FQ_HD inline void fq_masks(const uint32_t (&v)[8], int nb, uint32_t prev, uint32_t &ls, uint32_t &ns) {
    ls = ns = 0;
    for (int i = 0; i < nb; ++i) {
        const uint32_t c = (v[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        ls |= (uint32_t)fq_line_start(prev, c) << i;
        ns |= (uint32_t)!fq_space(c) << i;
        prev = c;
    }
}

// bytes of the word that lie in sequence lines (*seq) and in quality lines (*qual).  lines: line starts in front of the
// word, counted from the first record of the range; byte i lies in line lines + popcount(ls & bits 0..i) - 1.
DBG_FQ_HD inline void fq_kind_masks(uint32_t ls, int nb, uint64_t lines, uint32_t *seq, uint32_t *qual) {
    uint32_t s = 0, q = 0;
    for (int i = 0; i < nb; ++i) {
        lines += (ls >> i) & 1u;
        const uint32_t kind = (uint32_t)((lines - 1) & 3u);
        s |= (uint32_t)(kind == 1u) << i;
        q |= (uint32_t)(kind == 3u) << i;
    }
    *seq = s;
    *qual = q;
}

// the mask on four bases and their four quality bytes, the first nb of them: a base whose quality byte - 33 is below
// min_q becomes 'N'.  *masked counts those bases, *bad is set by a quality byte outside 33..126.
DBG_FQ_HD inline uint32_t fq_mask_dword(uint32_t bases, uint32_t qual, int nb, uint32_t min_q, uint32_t *masked, uint32_t *bad) {
    for (int i = 0; i < nb; ++i) {
        const int32_t c = (int32_t)((qual >> (8 * i)) & 0xFFu);
        if (c < 33 || c > 126) *bad = 1u;
        if (c - 33 < (int32_t)min_q) {
            bases = (bases & ~(0xFFu << (8 * i))) | ((uint32_t)'N' << (8 * i));
            ++*masked;
        }
    }
    return bases;
}

// ---- host side: where the records of a byte range begin and where the file ends --------------------------------------------

// The record start at or after `from`: the first line start p >= from with t[p] == '@' whose second-next line begins with
// '+'.  Fed the bytes from `from` on, window by window.
struct FqStartScan {
    uint64_t found = ~0ull;  // ~0: not seen yet
    uint32_t prev;           // the byte before the next one fed ('\n' in front of the file)
    uint64_t lpos[2] = {0, 0};  // the last two line starts: position and first byte
    uint8_t lc[2] = {0, 0};
    int nl = 0;

    explicit FqStartScan(uint32_t byte_before) : prev(byte_before) {}
    // b: the n bytes at file position pos.  True once the start is known.
    bool feed(const uint8_t *b, uint64_t n, uint64_t pos) {
        for (uint64_t i = 0; i < n && found == ~0ull; ++i) {
            const uint32_t c = b[i];
            if (fq_line_start(prev, c)) {
                if (nl == 2 && lc[0] == '@' && c == '+') found = lpos[0];
                if (nl == 2) { lpos[0] = lpos[1]; lc[0] = lc[1]; nl = 1; }
                lpos[nl] = pos + i;
                lc[nl] = (uint8_t)c;
                ++nl;
            }
            prev = c;
        }
        return found != ~0ull;
    }
};

// bytes of b[0, n) that stay when its trailing white space goes (0: all of it is white space)
inline uint64_t fq_trim(const uint8_t *b, uint64_t n) {
    while (n && fq_space(b[n - 1])) --n;
    return n;
}

#if defined(__HIPCC__)
}  // namespace dbgk
#include "dbg_device.h"
#include "dbg_fasta.h"
#include "dbg_readsplit.h"
namespace dbgk {

struct FqState {       // the stream between two chunks
    uint64_t cur_s;    // packed sequence bytes committed so far
    uint64_t cur_q;    // quality bytes committed so far (counted with the mask off too: the length check needs them)
    uint64_t pend;     // speculative trailing white space of the open line, after the cursor of its kind
    uint64_t n_lines;  // lines started so far: the open line has kind (n_lines - 1) & 3
    uint32_t prev;     // last byte before the chunk
    uint32_t pad;
};

struct FqChunk {              // per-chunk scratch (k_fq_carry)
    uint64_t base_s, base_q;  // destinations of the first sequence / quality byte the chunk writes
    uint32_t first_ev;        // first event of the chunk: 0 none, 1 line start, 2 non-space byte
    uint32_t n_ls;            // line starts in the chunk
    unsigned long long pend;  // pending (speculative) bytes the chunk writes
};

__device__ inline void fq_load_masks(const char *__restrict__ t, uint64_t n, uint64_t w, uint32_t prev0, uint32_t &ls,
                                     uint32_t &ns) {
    const uint64_t p0 = w * 32;
    const uint4 *q = reinterpret_cast<const uint4 *>(t + p0);  // the buffer holds n + 64 bytes: the tail word reads padding
    const uint4 a = q[0], b = q[1];
    const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int nb = n - p0 >= 32 ? 32 : (int)(n - p0);  // and masks by length
    fq_masks(v, nb, p0 ? (uint8_t)t[p0 - 1] : prev0, ls, ns);
}

// per block: its line starts and the first backward code of its words
__global__ __launch_bounds__(256) void k_fq_blocks(const char *__restrict__ t, uint64_t n, const FqState *st, uint32_t *blk_ls,
                                                   uint8_t *blk_b) {
    __shared__ uint32_t sh[256];
    const uint64_t n_words = (n + 31) / 32;
    const uint64_t w0 = (uint64_t)blockIdx.x * FS_WPB + (uint64_t)threadIdx.x * FS_WPT;
    const uint32_t prev0 = st->prev;
    uint32_t cnt = 0, b = 0;
    for (int j = 0; j < FS_WPT; ++j) {
        const uint64_t w = w0 + j;
        if (w >= n_words) break;
        uint32_t ls, ns;
        fq_load_masks(t, n, w, prev0, ls, ns);
        cnt += __popc(ls);
        if (!b) b = fs_bcode(ls, ns);
    }
    uint64_t tot;
    (void)block_exscan_256(cnt, &tot);
    const uint32_t bi = fs_last_nz_256(b, 255 - threadIdx.x, sh);
    if (threadIdx.x == 0) {
        blk_ls[blockIdx.x] = (uint32_t)tot;
        blk_b[blockIdx.x] = (uint8_t)bi;
    }
}

// one block: blk_ls[i] := line starts of the chunk in front of block i; blk_b[i] := first event after block i (0: none
// before the chunk ends).  Chunk-level results to *ck.
__global__ __launch_bounds__(256) void k_fq_carry(uint32_t *blk_ls, uint8_t *blk_b, uint64_t nblk, const FqState *st, FqChunk *ck) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t carry;
    uint64_t lines = 0;  // a chunk is <= 1 GiB: fits 32 bits, summed in 64
    for (uint64_t r = 0; r < nblk; r += 256) {
        const uint64_t i = r + threadIdx.x;
        uint64_t tot;
        const uint64_t ex = block_exscan_256(i < nblk ? blk_ls[i] : 0u, &tot);
        if (i < nblk) blk_ls[i] = (uint32_t)(lines + ex);
        lines += tot;
    }
    if (threadIdx.x == 0) carry = 0u;
    __syncthreads();
    for (uint64_t r = 0; r < nblk; r += 256) {  // backward: lane 0 takes the last block of the round
        const uint64_t top = nblk - 1 - r;
        const bool ok = r + threadIdx.x < nblk;
        const uint64_t i = ok ? top - threadIdx.x : 0;
        const uint32_t v = ok ? blk_b[i] : 0u;
        const uint32_t inc = fs_last_nz_256(v, threadIdx.x, sh);
        const uint32_t exc = threadIdx.x ? sh[threadIdx.x - 1] : 0u;
        const uint32_t c0 = carry;
        __syncthreads();
        if (ok) blk_b[i] = (uint8_t)(exc ? exc : c0);
        if (threadIdx.x == 255 && inc) carry = inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t first = carry;
        const uint32_t kind = (uint32_t)((st->n_lines - 1) & 3u);
        const uint64_t keeps = first == 1u ? 0u : st->pend;  // the open line ends at once: its pending bytes drop
        ck->first_ev = first;
        ck->n_ls = (uint32_t)lines;
        ck->base_s = st->cur_s + (kind == 1u ? keeps : 0u);
        ck->base_q = st->cur_q + (kind == 3u ? keeps : 0u);
        ck->pend = 0;
    }
}

// per word: written sequence bytes (wr_s), written quality bytes (wr_q), line starts (lsm) and the line starts of the chunk
// in front of the word (lidx); pending bytes counted into ck->pend
__global__ __launch_bounds__(256) void k_fq_count(const char *__restrict__ t, uint64_t n, const FqState *st,
                                                  const uint32_t *blk_ls, const uint8_t *blk_b, uint32_t *wr_s, uint32_t *wr_q,
                                                  uint32_t *lsm, uint32_t *lidx, FqChunk *ck) {
    __shared__ uint32_t sh[256];
    const uint64_t n_words = (n + 31) / 32;
    const uint64_t w0 = (uint64_t)blockIdx.x * FS_WPB + (uint64_t)threadIdx.x * FS_WPT;
    const uint32_t prev0 = st->prev;
    uint32_t ls[FS_WPT], ns[FS_WPT];
    uint32_t cnt = 0, b = 0;
#pragma unroll
    for (int j = 0; j < FS_WPT; ++j) {
        ls[j] = ns[j] = 0;
        if (w0 + j < n_words) fq_load_masks(t, n, w0 + j, prev0, ls[j], ns[j]);
        cnt += __popc(ls[j]);
        if (!b) b = fs_bcode(ls[j], ns[j]);
    }
    uint64_t tot;
    uint32_t before = blk_ls[blockIdx.x] + (uint32_t)block_exscan_256(cnt, &tot);  // line starts of the chunk in front of this thread
    const uint32_t lane_b = 255 - threadIdx.x;
    (void)fs_last_nz_256(b, lane_b, sh);
    const uint32_t bx = lane_b ? sh[lane_b - 1] : 0u;
    uint32_t ahead = bx ? bx : blk_b[blockIdx.x];  // 0 open (no event before the chunk ends), 1 line ends, 2 non-space
    uint32_t yes[FS_WPT], open[FS_WPT];
#pragma unroll
    for (int j = FS_WPT - 1; j >= 0; --j) {
        uint32_t y = 0, o = 0;
        for (int i = 31; i >= 0; --i) {
            if ((ns[j] >> i) & 1u) ahead = 2u;
            y |= (uint32_t)(ahead == 2u) << i;
            o |= (uint32_t)(ahead == 0u) << i;
            if ((ls[j] >> i) & 1u) ahead = 1u;
        }
        yes[j] = y;
        open[j] = o;
    }
    const uint64_t lines0 = st->n_lines;
    uint32_t pend = 0;
#pragma unroll
    for (int j = 0; j < FS_WPT; ++j) {
        const uint64_t w = w0 + j;
        if (w >= n_words) break;
        const int nb = n - w * 32 >= 32 ? 32 : (int)(n - w * 32);
        uint32_t seq, qual;
        fq_kind_masks(ls[j], nb, lines0 + before, &seq, &qual);
        wr_s[w] = seq & (yes[j] | open[j]);
        wr_q[w] = qual & (yes[j] | open[j]);
        lsm[w] = ls[j];
        lidx[w] = before;
        pend += __popc((seq | qual) & open[j]);
        before += __popc(ls[j]);
    }
    if (pend) atomicAdd(&ck->pend, (unsigned long long)pend);
}

struct FqPopcPair {  // written sequence bytes in the low half, written quality bytes in the high half (a chunk is <= 1 GiB)
    const uint32_t *wr_s, *wr_q;
    __device__ uint64_t operator()(uint64_t w) const { return (uint64_t)__popc(wr_s[w]) | ((uint64_t)__popc(wr_q[w]) << 32); }
};

// thread per byte: the written bytes to their places, an offset at every sequence-line start, the checks at the line starts.
// qual == nullptr (mask off): quality bytes are counted, never stored.
__global__ __launch_bounds__(256) void k_fq_write(const char *__restrict__ t, uint64_t n, const FqState *st, const FqChunk *ck,
                                                  const uint32_t *wr_s, const uint32_t *wr_q, const uint32_t *lsm,
                                                  const uint32_t *lidx, const uint64_t *rank, char *bases, char *qual,
                                                  uint64_t cap, uint64_t *offsets, uint64_t off_cap, uint64_t *flags,
                                                  unsigned long long *err) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t w = p >> 5;
    const uint32_t bit = (uint32_t)(p & 31), below = (1u << bit) - 1u;
    const uint32_t ms = wr_s[w], mq = wr_q[w], l = lsm[w];
    if (!(((ms | mq | l) >> bit) & 1u)) return;
    const uint64_t rk = rank[w];
    const uint64_t ds = ck->base_s + (rk & 0xFFFFFFFFull) + __popc(ms & below);  // sequence bytes kept in front of p
    const uint64_t dq = ck->base_q + (rk >> 32) + __popc(mq & below);            // quality bytes kept in front of p
    const uint32_t c = (uint8_t)t[p];
    if ((ms >> bit) & 1u) {
        if (ds < cap) bases[ds] = (char)c;
        else atomicOr((unsigned long long *)flags, 1ull);  // the host grows the buffers and runs the chunk again
    }
    if (((mq >> bit) & 1u) && qual) {
        if (dq < cap) qual[dq] = (char)c;
        else atomicOr((unsigned long long *)flags, 1ull);
    }
    if ((l >> bit) & 1u) {
        const uint64_t g = st->n_lines + lidx[w] + __popc(l & below);  // this line, counted from the first record
        const uint64_t rec = g >> 2;
        uint64_t bad = FQ_NO_ERROR;
        switch ((uint32_t)(g & 3u)) {
            case 0:
                if (c != '@') bad = rec * 8 + FQ_E_HEADER;
                if (rec && ds != dq) bad = (rec - 1) * 8 + FQ_E_LENGTH;  // the record that ends here
                break;
            case 1:
                if (c == '@' || c == '+') bad = rec * 8 + FQ_E_SEQ_START;
                if (rec < off_cap) offsets[rec] = ds;  // beyond: the host grows the offsets and runs the chunk again
                break;
            case 2:
                if (c != '+') bad = rec * 8 + FQ_E_SEPARATOR;
                break;
            default: break;
        }
        if (bad != FQ_NO_ERROR) atomicMin(err, (unsigned long long)bad);
    }
}

// the stream state after the chunk; scan_total: the packed totals of FqPopcPair
__global__ void k_fq_finish(const char *__restrict__ t, uint64_t n, const FqState *in, const FqChunk *ck,
                            const uint64_t *scan_total, FqState *out) {
    if (threadIdx.x != 0) return;
    const uint64_t tot = *scan_total;
    const uint64_t pend = ck->pend + (ck->first_ev == 0 ? in->pend : 0);  // no event: the open line goes on
    const uint64_t lines = in->n_lines + ck->n_ls;
    const uint32_t kind = (uint32_t)((lines - 1) & 3u);
    out->cur_s = ck->base_s + (tot & 0xFFFFFFFFull) - (kind == 1u ? pend : 0u);
    out->cur_q = ck->base_q + (tot >> 32) - (kind == 3u ? pend : 0u);
    out->pend = pend;
    out->n_lines = lines;
    out->prev = (uint8_t)t[n - 1];
    out->pad = 0;
}

// the quality mask over the packed bases, 16 bytes a thread: base j becomes 'N' where qual[j] - 33 < min_q.  Both buffers
// are padded by 64 bytes, so the tail thread loads and stores whole vectors and changes its first n - p0 bytes only.
// *masked: one atomic per workgroup.  A quality byte outside 33..126 names its record in *err.
__global__ __launch_bounds__(256) void k_fq_mask(char *bases, const char *__restrict__ qual, uint64_t n, uint32_t min_q,
                                                 const uint64_t *__restrict__ offsets, uint64_t n_reads,
                                                 unsigned long long *masked, unsigned long long *err) {
    __shared__ uint32_t wave_cnt[4];
    const uint64_t p0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    uint32_t cnt = 0;
    if (p0 < n) {
        const int nb = n - p0 >= 16 ? 16 : (int)(n - p0);
        uint4 *bp = reinterpret_cast<uint4 *>(bases + p0);
        const uint4 a = *bp, q = *reinterpret_cast<const uint4 *>(qual + p0);
        const uint32_t qv[4] = {q.x, q.y, q.z, q.w};
        uint32_t v[4] = {a.x, a.y, a.z, a.w};
        uint32_t bad = 0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = nb - 4 * i;
            const uint32_t o = fq_mask_dword(v[i], qv[i], m >= 4 ? 4 : (m > 0 ? m : 0), min_q, &cnt, &bad);
            any |= o != v[i];
            v[i] = o;
        }
        if (any) *bp = make_uint4(v[0], v[1], v[2], v[3]);
        if (bad) {  // rare: the first bad byte of these 16 and its record
            for (int i = 0; i < nb; ++i) {
                const uint32_t c = (uint8_t)qual[p0 + i];
                if (c < 33 || c > 126) {
                    atomicMin(err, (unsigned long long)(rs_read_of(offsets, n_reads, p0 + i) * 8 + FQ_E_QUALITY));
                    break;
                }
            }
        }
    }
    const uint64_t wsum = wave_sum_u64(cnt);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = (uint32_t)wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t s = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (s) atomicAdd(masked, (unsigned long long)s);
    }
}

#endif  // __HIPCC__

}  // namespace dbgk
