// Chunked FASTA ingest (dbg_set_reads_fasta_file): read_reads (debruijn.py:22-32) over a byte stream that reaches the
// device one staging chunk at a time.
//
// The one-shot path (k_fa_* in dbg_hip.hip) lists every line start and then works per line.  A chunk does not hold
// whole lines (a line may be longer than a chunk), and per-line arrays would cost up to 8 bytes per byte of text on a
// file of blank lines, so this path works per byte instead.  A byte of a read line is "written" to the packed bases
// iff a non-space byte follows it (or is it) in the same line -- that is exactly rstrip -- and its place in the
// packed bases is the number of written bytes before it.  Both are prefix problems over the chunk:
//   * line start of byte p:  t[p-1] == '\n', or t[p-1] == '\r' and t[p] != '\n' (universal newlines; the byte before
//     the chunk is carried in the stream state);
//   * is the line of p a read: the first byte of the nearest line start at or before p is not '>' (forward "nearest
//     event" scan, the line open at the chunk start carries its kind in the state);
//   * is p written: the next event (line start or non-space byte) at or after p is a non-space byte (backward
//     "nearest event" scan).  When no event follows before the chunk ends, the line is still open: its trailing white
//     space is written speculatively at the place it would take ("pending") and either becomes part of the read when
//     a later chunk brings a non-space byte, or is overwritten by the next read when the line ends.
// Destinations and read indices are then two popcount prefix sums (one packed u64 scan), and the running byte cursor
// and read count stay on the device from chunk to chunk.
//
// Per chunk of n bytes the device holds the text (n + 64), two u32 masks and one u64 rank per 32-byte word
// (n / 2 bytes) and one byte per 64 KiB block of text: ~1.5 n.
//
// Record mode (dbg_set_reads_fasta_records*): a read is a record, the sequence lines between two header lines joined,
// each rstrip'ed on its own.  What is written and where stays as above -- the bytes of the sequence lines, packed --
// and one thing changes: the read starts are the header line starts, not the sequence line starts, and a read's offset
// is the number of written bytes in front of its header.  The host finds the owned bytes [first header at or after
// begin, first header at or after end) before the first chunk (FaHeaderScan), so the stream begins and ends at a header.
//
// The header search is plain C++: a host compiler can include this file alone (tests/fasta_records_host.cpp does).
#pragma once
#include <stdint.h>

namespace dbgk {

inline bool fa_space(uint32_t c) {  // str.isspace() over the ASCII range (fs_space below)
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31);
}

// The first header line start at or after `from`: the first line start p >= from with t[p] == '>'.  Fed the bytes from
// `from` on, window by window.  first_seq: the first non-space byte fed in front of it (~0: none) -- from 0 on that is
// sequence before the first header.
struct FaHeaderScan {
    uint64_t found = ~0ull;      // ~0: not seen yet
    uint64_t first_seq = ~0ull;
    uint32_t prev;               // the byte before the next one fed ('\n' in front of the file)

    explicit FaHeaderScan(uint32_t byte_before) : prev(byte_before) {}
    // b: the n bytes at file position pos.  True once the start is known.
    bool feed(const uint8_t *b, uint64_t n, uint64_t pos) {
        for (uint64_t i = 0; i < n && found == ~0ull; ++i) {
            const uint32_t c = b[i];
            if (c == '>' && (prev == '\n' || prev == '\r')) found = pos + i;  // after '\r' a '>' is no '\n': a line start
            else if (first_seq == ~0ull && !fa_space(c)) first_seq = pos + i;
            prev = c;
        }
        return found != ~0ull;
    }
};

}  // namespace dbgk

#if defined(__HIPCC__)
#include "dbg_device.h"

namespace dbgk {

constexpr int FS_WPT = 8;                  // 32-byte words per thread
constexpr int FS_WPB = 256 * FS_WPT;       // words per block (64 KiB of text)

struct FsState {         // the stream between two chunks
    uint64_t cursor;     // packed bases committed so far
    uint64_t pend;       // speculative trailing white space of the open read line, at [cursor, cursor + pend)
    uint64_t n_reads;    // read lines started so far
    uint32_t prev;       // last byte before the chunk ('\n' before the file: byte 0 is a line start)
    uint32_t kind;       // the line open at the chunk start: 1 = a read, 0 = a header or a line the range does not own
};

struct FsChunk {                 // per-chunk scratch (k_fs_carry)
    uint64_t base;               // destination of the first byte the chunk writes
    uint32_t first_ev;           // first event of the chunk: 0 none, 1 line start, 2 non-space byte
    uint32_t last_kind;          // kind of the line open at the chunk end
    unsigned long long pend;     // pending (speculative) bytes the chunk writes
};

__device__ inline bool fs_space(uint32_t c) {  // str.isspace() over the ASCII range
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31);
}

// masks of word w: ls = line starts, ns = non-space bytes, rs = line starts of reads (first byte != '>')
__device__ inline void fs_masks(const char *__restrict__ t, uint64_t n, uint64_t w, uint32_t prev0, uint32_t &ls,
                                uint32_t &ns, uint32_t &rs) {
    const uint64_t p0 = w * 32;
    const uint4 *q = reinterpret_cast<const uint4 *>(t + p0);  // the buffer holds n + 64 bytes: the tail word reads padding
    const uint4 a = q[0], b = q[1];
    const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t prev = p0 ? (uint8_t)t[p0 - 1] : prev0;
    const int nb = n - p0 >= 32 ? 32 : (int)(n - p0);
    ls = ns = rs = 0;
    for (int i = 0; i < nb; ++i) {
        const uint32_t c = (v[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        const uint32_t st = prev == '\n' || (prev == '\r' && c != '\n');
        ls |= st << i;
        ns |= (uint32_t)!fs_space(c) << i;
        rs |= (st & (c != '>')) << i;
        prev = c;
    }
}
// forward code: 0 no line start, else 1 + (the last line start of the word begins a read)
__device__ inline uint32_t fs_fcode(uint32_t ls, uint32_t rs) { return ls ? 1u + ((rs >> (31 - __clz(ls))) & 1u) : 0u; }
// backward code: 0 no event, 1 the first event is a line start, 2 it is a non-space byte of the line already open
__device__ inline uint32_t fs_bcode(uint32_t ls, uint32_t ns) {
    const uint32_t ev = ls | ns;
    return ev ? ((ls & (ev & (0u - ev))) ? 1u : 2u) : 0u;
}

// inclusive scan over the 256 lanes in `lane` order, op(earlier, later) = later ? later : earlier
__device__ inline uint32_t fs_last_nz_256(uint32_t v, uint32_t lane, uint32_t *sh) {
    sh[lane] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t o = lane >= d ? sh[lane - d] : 0u;
        __syncthreads();
        if (!v) v = o;
        sh[lane] = v;
        __syncthreads();
    }
    return v;
}

// per block: the last forward code and the first backward code of its words
__global__ __launch_bounds__(256) void k_fs_blocks(const char *__restrict__ t, uint64_t n, const FsState *st, uint8_t *blk_f,
                                                   uint8_t *blk_b) {
    __shared__ uint32_t sh[256];
    const uint64_t n_words = (n + 31) / 32;
    const uint64_t w0 = (uint64_t)blockIdx.x * FS_WPB + (uint64_t)threadIdx.x * FS_WPT;
    const uint32_t prev0 = st->prev;
    uint32_t f = 0, b = 0;
    for (int j = 0; j < FS_WPT; ++j) {
        const uint64_t w = w0 + j;
        if (w >= n_words) break;
        uint32_t ls, ns, rs;
        fs_masks(t, n, w, prev0, ls, ns, rs);
        const uint32_t fc = fs_fcode(ls, rs), bc = fs_bcode(ls, ns);
        if (fc) f = fc;
        if (!b) b = bc;
    }
    const uint32_t fi = fs_last_nz_256(f, threadIdx.x, sh);
    __syncthreads();
    const uint32_t bi = fs_last_nz_256(b, 255 - threadIdx.x, sh);
    if (threadIdx.x == 255) blk_f[blockIdx.x] = (uint8_t)fi;
    if (threadIdx.x == 0) blk_b[blockIdx.x] = (uint8_t)bi;
}

// one block: exclusive carries across the blocks, in place.  blk_f[i] := kind (0/1) of the line open where block i
// starts; blk_b[i] := first event after block i (0: none before the chunk ends).  Chunk-level results to *ck.
__global__ __launch_bounds__(256) void k_fs_carry(uint8_t *blk_f, uint8_t *blk_b, uint64_t nblk, const FsState *st,
                                                  FsChunk *ck) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 1u + st->kind;
    __syncthreads();
    for (uint64_t r = 0; r < nblk; r += 256) {
        const uint64_t i = r + threadIdx.x;
        const uint32_t v = i < nblk ? blk_f[i] : 0u;
        const uint32_t inc = fs_last_nz_256(v, threadIdx.x, sh);
        const uint32_t exc = threadIdx.x ? sh[threadIdx.x - 1] : 0u;
        const uint32_t c0 = carry;
        __syncthreads();
        if (i < nblk) blk_f[i] = (uint8_t)((exc ? exc : c0) - 1u);
        if (threadIdx.x == 255 && inc) carry = inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) ck->last_kind = carry - 1u;
    __syncthreads();
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
        ck->first_ev = carry;
        ck->base = st->cursor + (carry == 1u ? 0u : st->pend);  // the open line ends at once: its pending bytes drop
        ck->pend = 0;
    }
}

// per word: written bytes (wr) and read starts (rs); pending bytes counted into ck->pend.  REC (record mode): the read
// starts are the header line starts (ls & ~rs), and the sequence line starts of the chunk are summed into *n_seq, one
// atomic per workgroup.
template <bool REC>
__global__ __launch_bounds__(256) void k_fs_count(const char *__restrict__ t, uint64_t n, const FsState *st,
                                                  const uint8_t *blk_f, const uint8_t *blk_b, uint32_t *wr_out,
                                                  uint32_t *rs_out, FsChunk *ck, unsigned long long *n_seq) {
    __shared__ uint32_t sh[256];
    const uint64_t n_words = (n + 31) / 32;
    const uint64_t w0 = (uint64_t)blockIdx.x * FS_WPB + (uint64_t)threadIdx.x * FS_WPT;
    const uint32_t prev0 = st->prev;
    uint32_t ls[FS_WPT], ns[FS_WPT], rs[FS_WPT];
    uint32_t f = 0, b = 0;
#pragma unroll
    for (int j = 0; j < FS_WPT; ++j) {
        ls[j] = ns[j] = rs[j] = 0;
        if (w0 + j < n_words) fs_masks(t, n, w0 + j, prev0, ls[j], ns[j], rs[j]);
        const uint32_t fc = fs_fcode(ls[j], rs[j]), bc = fs_bcode(ls[j], ns[j]);
        if (fc) f = fc;
        if (!b) b = bc;
    }
    // entering state of this thread's words from the left (kind) and from the right (next event)
    (void)fs_last_nz_256(f, threadIdx.x, sh);
    const uint32_t fx = threadIdx.x ? sh[threadIdx.x - 1] : 0u;
    __syncthreads();
    const uint32_t lane_b = 255 - threadIdx.x;
    (void)fs_last_nz_256(b, lane_b, sh);
    const uint32_t bx = lane_b ? sh[lane_b - 1] : 0u;
    uint32_t kind = fx ? fx - 1u : blk_f[blockIdx.x];
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
    uint32_t pend = 0;
#pragma unroll
    for (int j = 0; j < FS_WPT; ++j) {
        const uint64_t w = w0 + j;
        if (w >= n_words) break;
        const int nb = n - w * 32 >= 32 ? 32 : (int)(n - w * 32);
        uint32_t inread = 0;
        for (int i = 0; i < nb; ++i) {
            if ((ls[j] >> i) & 1u) kind = (rs[j] >> i) & 1u;
            inread |= kind << i;
        }
        wr_out[w] = inread & (yes[j] | open[j]);
        rs_out[w] = REC ? ls[j] & ~rs[j] : rs[j];
        pend += __popc(inread & open[j]);
    }
    if (pend) atomicAdd(&ck->pend, (unsigned long long)pend);
    if constexpr (REC) {
        uint32_t lines = 0;
#pragma unroll
        for (int j = 0; j < FS_WPT; ++j) lines += __popc(rs[j]);
        __syncthreads();  // the scans above are done with sh
        sh[threadIdx.x] = lines;
        __syncthreads();
        for (uint32_t d = 128; d; d >>= 1) {
            if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
            __syncthreads();
        }
        if (threadIdx.x == 0 && sh[0]) atomicAdd(n_seq, (unsigned long long)sh[0]);
    }
}

struct FsPopcPair {  // written bytes in the low half, read starts in the high half (a chunk is < 4 GiB)
    const uint32_t *wr, *rs;
    __device__ uint64_t operator()(uint64_t w) const { return (uint64_t)__popc(wr[w]) | ((uint64_t)__popc(rs[w]) << 32); }
};

// thread per byte: the written bytes to their place in the packed bases, the read starts to the offsets
__global__ __launch_bounds__(256) void k_fs_write(const char *__restrict__ t, uint64_t n, const FsState *st, const FsChunk *ck,
                                                  const uint32_t *wr, const uint32_t *rsm, const uint64_t *rank,
                                                  char *bases, uint64_t bases_cap, uint64_t *offsets, uint64_t off_cap,
                                                  uint64_t *flags) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint64_t w = p >> 5;
    const uint32_t bit = (uint32_t)(p & 31), below = (1u << bit) - 1u;
    const uint32_t m = wr[w], r = rsm[w];
    if (!(((m | r) >> bit) & 1u)) return;
    const uint64_t rk = rank[w];
    const uint64_t dst = ck->base + (rk & 0xFFFFFFFFull) + __popc(m & below);
    if ((m >> bit) & 1u) {
        if (dst < bases_cap) bases[dst] = t[p];
        else atomicOr((unsigned long long *)flags, 1ull);
    }
    if ((r >> bit) & 1u) {
        const uint64_t idx = st->n_reads + (rk >> 32) + __popc(r & below);
        if (idx < off_cap) offsets[idx] = dst;  // beyond: the host grows the offsets and runs the chunk again
    }
}

// the stream state after the chunk; scan_total: the packed totals of FsPopcPair
__global__ void k_fs_finish(const char *__restrict__ t, uint64_t n, const FsState *in, const FsChunk *ck,
                            const uint64_t *scan_total, FsState *out) {
    if (threadIdx.x != 0) return;
    const uint64_t tot = *scan_total;
    const uint64_t written = tot & 0xFFFFFFFFull, starts = tot >> 32;
    const uint64_t pend = ck->pend + (ck->first_ev == 0 ? in->pend : 0);  // no event: the open line goes on
    out->cursor = ck->base + written - pend;
    out->pend = pend;
    out->n_reads = in->n_reads + starts;
    out->prev = (uint8_t)t[n - 1];
    out->kind = ck->last_kind;
}

// record mode, after the last chunk: the longest read, from the finished offsets (offsets[n_reads] is set)
__global__ __launch_bounds__(256) void k_fs_longest(const uint64_t *__restrict__ offsets, uint64_t n_reads,
                                                    unsigned long long *out) {
    __shared__ unsigned long long sh[256];
    unsigned long long m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * 256) {
        const unsigned long long len = offsets[i + 1] - offsets[i];
        if (len > m) m = len;
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t d = 128; d; d >>= 1) {
        if (threadIdx.x < d && sh[threadIdx.x + d] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0]) atomicMax(out, sh[0]);
}

}  // namespace dbgk
#endif  // __HIPCC__
