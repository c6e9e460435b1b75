// Reads cut at the bytes that are not bases (dbg_split_reads): pieces(reads, fold) = the maximal runs of A/C/G/T of every
// read, in order, after an optional fold of a/c/g/t to upper case.  No piece spans a cut byte or the border of two reads.
//
// The pass works per byte over the resident bases.  With keep(p) = "the byte at p, folded if asked, is one of ACGT" and
// start(p) = keep(p) && (p == 0 || !keep(p - 1) || a read starts at p):
//   * the place of a kept byte in the new bases is the number of kept bytes before it,
//   * the piece that starts at p has the index "number of starts before p".
// Both are prefix sums of popcounts over fixed words of RS_WORD_BYTES bytes: a thread loads a word with 16-byte loads, forms
// its keep mask and its start mask (the previous byte's keep bit is read from the byte itself, the read starts come from the
// start bitmap every read set has) and counts bits.
//   k_rs_count   the first pass: reads the bases once, writes nothing but its totals.  Almost every call ends here.
//   k_rs_fold    folding alone, in place (bases the handle owns).
//   k_rs_blocks / k_rs_carry / k_rs_write   a changing split: per-block sums, their exclusive prefix (one workgroup, RS_ROUND_BLOCKS
//                blocks a round, the carry in a register), then bases, offsets and origins at their places.
// Positions and counts are 64 bits wide everywhere; only sums inside one block are narrower.
//
// The mask helpers are plain C++: a host compiler can include this file alone (tests/readsplit_host.cpp does).
#pragma once
#include <stdint.h>

#ifndef DBG_RS_HD
#if defined(__HIPCC__)
#define DBG_RS_HD __host__ __device__
#else
#define DBG_RS_HD
#endif
#endif

namespace dbgk {

constexpr int RS_WORD_BYTES = 64;                                       // bytes per word: one 64-bit mask, four 16-byte loads
constexpr int RS_WORDS_PER_THREAD = 4;                                  // words a thread of the scan kernels takes (consecutive)
constexpr int RS_BLOCK_BYTES = 256 * RS_WORDS_PER_THREAD * RS_WORD_BYTES;  // bytes per block of 256 threads (64 KiB)
constexpr int RS_ROUND_BLOCKS = 256;                                    // blocks k_rs_carry scans at once
constexpr uint64_t RS_ROUND_BYTES = (uint64_t)RS_ROUND_BLOCKS * RS_BLOCK_BYTES;  // bytes per round of the carry kernel (16 MiB)

// ---- mask helpers (host and device) ------------------------------------------------------------------------------------

// 'A' 'C' 'G' 'T' are 0x41 0x43 0x47 0x54: the bytes 0x40..0x5F whose low five bits are 1, 3, 7 or 20
constexpr uint32_t RS_ACGT_BITS = (1u << 1) | (1u << 3) | (1u << 7) | (1u << 20);

DBG_RS_HD inline bool rs_is_acgt(uint32_t c) { return (c & 0xE0u) == 0x40u && ((RS_ACGT_BITS >> (c & 31u)) & 1u); }
DBG_RS_HD inline bool rs_is_acgt_lower(uint32_t c) { return (c & 0xE0u) == 0x60u && ((RS_ACGT_BITS >> (c & 31u)) & 1u); }

// the fold: a c g t -> A C G T, every other byte (of 256) as it is
DBG_RS_HD inline uint32_t rs_fold(uint32_t c) { return rs_is_acgt_lower(c) ? c ^ 0x20u : c; }

DBG_RS_HD inline bool rs_keep(uint32_t c, bool fold) { return rs_is_acgt(fold ? rs_fold(c) : c); }

// keep mask of a word: bit i = byte i is kept, for the first nb bytes (v: the word as 16 little-endian dwords).
// *folded: bit i = byte i is kept and the fold changed it.
DBG_RS_HD inline uint64_t rs_keep_mask(const uint32_t (&v)[RS_WORD_BYTES / 4], int nb, bool fold, uint64_t *folded) {
    uint64_t keep = 0, low = 0;
    for (int i = 0; i < RS_WORD_BYTES; ++i) {
        const uint32_t c = (v[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        keep |= (uint64_t)rs_is_acgt(c) << i;
        low |= (uint64_t)rs_is_acgt_lower(c) << i;
    }
    const uint64_t valid = nb >= RS_WORD_BYTES ? ~0ull : ((1ull << nb) - 1ull);
    if (!fold) low = 0;
    *folded = low & valid;
    return (keep | low) & valid;
}

// start mask of a word from its keep mask, the keep bit of the byte before the word (0 in front of the buffer) and the
// read-start bits of its positions: a kept byte starts a piece where the byte before it is not kept or a read begins
DBG_RS_HD inline uint64_t rs_start_mask(uint64_t keep, uint32_t prev_keep, uint64_t read_starts) {
    return keep & (~((keep << 1) | (uint64_t)(prev_keep & 1u)) | read_starts);
}

#if defined(__HIPCC__)
}  // namespace dbgk
#include "dbg_device.h"
namespace dbgk {

struct RsTotals {                       // what the first pass counts
    unsigned long long kept;            // bytes that stay
    unsigned long long folded;          // kept bytes the fold changes
    unsigned long long starts;          // piece starts
    unsigned long long nonempty_reads;  // reads of at least one byte (distinct read starts in front of the end)
    unsigned long long with_piece;      // k_rs_write: reads that keep a piece
    unsigned long long intact;          // k_rs_write: reads that are one piece from their first byte to their last
};

struct RsWord {
    uint64_t keep, folded, starts, read_starts;
};

// word w of the bases.  A borrowed buffer ends at n: nothing is read beyond it.
__device__ inline RsWord rs_load_word(const char *__restrict__ bases, uint64_t n, const uint32_t *__restrict__ startbits,
                                      uint64_t w, bool fold) {
    const uint64_t p0 = w * RS_WORD_BYTES;
    uint32_t v[RS_WORD_BYTES / 4];
    int nb = RS_WORD_BYTES;
    if (n - p0 >= (uint64_t)RS_WORD_BYTES) {
        const uint4 *q = reinterpret_cast<const uint4 *>(bases + p0);
#pragma unroll
        for (int i = 0; i < RS_WORD_BYTES / 16; ++i) {
            const uint4 a = q[i];
            v[4 * i] = a.x; v[4 * i + 1] = a.y; v[4 * i + 2] = a.z; v[4 * i + 3] = a.w;
        }
    } else {
        nb = (int)(n - p0);
#pragma unroll
        for (int i = 0; i < RS_WORD_BYTES / 4; ++i) v[i] = 0;
        for (int i = 0; i < nb; ++i) v[i >> 2] |= (uint32_t)(uint8_t)bases[p0 + i] << (8 * (i & 3));
    }
    RsWord r;
    r.keep = rs_keep_mask(v, nb, fold, &r.folded);
    const uint32_t prev = p0 ? (uint32_t)rs_keep((uint8_t)bases[p0 - 1], fold) : 0u;
    const uint64_t valid = nb >= RS_WORD_BYTES ? ~0ull : ((1ull << nb) - 1ull);
    r.read_starts = ((uint64_t)startbits[2 * w] | ((uint64_t)startbits[2 * w + 1] << 32)) & valid;  // the bitmap is padded
    r.starts = rs_start_mask(r.keep, prev, r.read_starts);
    return r;
}

// the first pass: grid-stride over the words, totals by one atomic per wave and counter
__global__ __launch_bounds__(256) void k_rs_count(const char *__restrict__ bases, uint64_t n,
                                                  const uint32_t *__restrict__ startbits, int fold, RsTotals *tot) {
    const uint64_t n_words = (n + RS_WORD_BYTES - 1) / RS_WORD_BYTES;
    uint64_t kept = 0, folded = 0, starts = 0, nonempty = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
        const RsWord r = rs_load_word(bases, n, startbits, w, fold != 0);
        kept += __popcll(r.keep);
        folded += __popcll(r.folded);
        starts += __popcll(r.starts);
        nonempty += __popcll(r.read_starts);
    }
    kept = wave_sum_u64(kept);
    folded = wave_sum_u64(folded);
    starts = wave_sum_u64(starts);
    nonempty = wave_sum_u64(nonempty);
    if ((threadIdx.x & 63) == 0) {
        if (kept) atomicAdd(&tot->kept, (unsigned long long)kept);
        if (folded) atomicAdd(&tot->folded, (unsigned long long)folded);
        if (starts) atomicAdd(&tot->starts, (unsigned long long)starts);
        if (nonempty) atomicAdd(&tot->nonempty_reads, (unsigned long long)nonempty);
    }
}

// folding alone: 16 bytes per thread, in place
__global__ __launch_bounds__(256) void k_rs_fold(char *bases, uint64_t n) {
    const uint64_t p0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (p0 >= n) return;
    if (n - p0 >= 16) {
        uint4 *q = reinterpret_cast<uint4 *>(bases + p0);
        const uint4 a = *q;
        uint32_t v[4] = {a.x, a.y, a.z, a.w};
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t o = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) o |= rs_fold((v[i] >> (8 * b)) & 0xFFu) << (8 * b);
            any |= o != v[i];
            v[i] = o;
        }
        if (any) *q = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        for (uint64_t p = p0; p < n; ++p) bases[p] = (char)rs_fold((uint8_t)bases[p]);
    }
}

// word j of thread t of block b
__device__ inline uint64_t rs_word_of(uint64_t block, uint32_t t, int j) {
    return (block * 256 + t) * RS_WORDS_PER_THREAD + j;
}

// per block: kept bytes and piece starts
__global__ __launch_bounds__(256) void k_rs_blocks(const char *__restrict__ bases, uint64_t n,
                                                   const uint32_t *__restrict__ startbits, int fold, uint64_t *blk_kept,
                                                   uint64_t *blk_starts) {
    const uint64_t n_words = (n + RS_WORD_BYTES - 1) / RS_WORD_BYTES;
    uint64_t kept = 0, starts = 0;
#pragma unroll
    for (int j = 0; j < RS_WORDS_PER_THREAD; ++j) {
        const uint64_t w = rs_word_of(blockIdx.x, threadIdx.x, j);
        if (w >= n_words) break;
        const RsWord r = rs_load_word(bases, n, startbits, w, fold != 0);
        kept += __popcll(r.keep);
        starts += __popcll(r.starts);
    }
    uint64_t tot;
    (void)block_exscan_256(kept | (starts << 32), &tot);  // a block holds 2^16 bytes: both sums fit their halves
    if (threadIdx.x == 0) {
        blk_kept[blockIdx.x] = tot & 0xFFFFFFFFull;
        blk_starts[blockIdx.x] = tot >> 32;
    }
}

// one workgroup: both per-block arrays to their exclusive prefixes, in place, RS_ROUND_BLOCKS blocks a round
__global__ __launch_bounds__(256) void k_rs_carry(uint64_t *blk_kept, uint64_t *blk_starts, uint64_t nblk) {
    uint64_t carry_k = 0, carry_s = 0;
    for (uint64_t base = 0; base < nblk; base += RS_ROUND_BLOCKS) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t a = i < nblk ? blk_kept[i] : 0, b = i < nblk ? blk_starts[i] : 0;
        uint64_t tot;
        const uint64_t ex = block_exscan_256(a | (b << 32), &tot);  // a round holds 2^24 bytes
        if (i < nblk) {
            blk_kept[i] = carry_k + (ex & 0xFFFFFFFFull);
            blk_starts[i] = carry_s + (ex >> 32);
        }
        carry_k += tot & 0xFFFFFFFFull;
        carry_s += tot >> 32;
    }
}

// the read that holds byte p: the last i with offsets[i] <= p (empty reads in front of it share its offset)
__device__ inline uint64_t rs_read_of(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t p) {
    uint64_t lo = 0, hi = n_reads;  // answer in [lo, hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// the kept bytes to their places, a new offset and an origin per piece start.  blk_kept / blk_starts: exclusive prefixes.
__global__ __launch_bounds__(256) void k_rs_write(const char *__restrict__ bases, uint64_t n,
                                                  const uint32_t *__restrict__ startbits, int fold,
                                                  const uint64_t *__restrict__ offsets, uint64_t n_reads,
                                                  const uint64_t *__restrict__ blk_kept,
                                                  const uint64_t *__restrict__ blk_starts, char *out_bases, uint64_t n_kept,
                                                  uint64_t *out_offsets, uint64_t *org_read, uint64_t *org_pos,
                                                  uint64_t n_pieces) {
    const uint64_t n_words = (n + RS_WORD_BYTES - 1) / RS_WORD_BYTES;
    RsWord r[RS_WORDS_PER_THREAD];
    uint64_t kept = 0, starts = 0;
#pragma unroll
    for (int j = 0; j < RS_WORDS_PER_THREAD; ++j) {
        const uint64_t w = rs_word_of(blockIdx.x, threadIdx.x, j);
        r[j] = RsWord{0, 0, 0, 0};
        if (w < n_words) r[j] = rs_load_word(bases, n, startbits, w, fold != 0);
        kept += __popcll(r[j].keep);
        starts += __popcll(r[j].starts);
    }
    uint64_t tot;
    const uint64_t ex = block_exscan_256(kept | (starts << 32), &tot);
    uint64_t dst = blk_kept[blockIdx.x] + (ex & 0xFFFFFFFFull), piece = blk_starts[blockIdx.x] + (ex >> 32);
#pragma unroll
    for (int j = 0; j < RS_WORDS_PER_THREAD; ++j) {
        const uint64_t p0 = rs_word_of(blockIdx.x, threadIdx.x, j) * RS_WORD_BYTES;
        const uint64_t keep = r[j].keep;
        if (keep == ~0ull && !(dst & 15) && dst + RS_WORD_BYTES <= n_kept && !(fold && r[j].folded)) {  // a whole word moves as it is
            const uint4 *q = reinterpret_cast<const uint4 *>(bases + p0);
            uint4 *o = reinterpret_cast<uint4 *>(out_bases + dst);
#pragma unroll
            for (int i = 0; i < RS_WORD_BYTES / 16; ++i) o[i] = q[i];
        } else {
            uint64_t m = keep, d = dst;
            while (m) {
                const int i = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const uint32_t c = (uint8_t)bases[p0 + i];
                if (d < n_kept) out_bases[d] = (char)(fold ? rs_fold(c) : c);
                ++d;
            }
        }
        uint64_t s = r[j].starts;
        while (s) {
            const int i = __ffsll((unsigned long long)s) - 1;
            s &= s - 1;
            const uint64_t p = p0 + i;
            const uint64_t rd = rs_read_of(offsets, n_reads, p);
            if (piece < n_pieces) {
                out_offsets[piece] = dst + __popcll(keep & ((1ull << i) - 1ull));
                org_read[piece] = rd;
                org_pos[piece] = p - offsets[rd];
            }
            ++piece;
        }
        dst += __popcll(keep);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out_offsets[n_pieces] = n_kept;
}

// per piece: is it the first piece of its read, and is it the whole read?
__global__ __launch_bounds__(256) void k_rs_read_stats(const uint64_t *__restrict__ offsets, const uint64_t *__restrict__ out_offsets,
                                                       const uint64_t *__restrict__ org_read, const uint64_t *__restrict__ org_pos,
                                                       uint64_t n_pieces, RsTotals *tot) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t first = 0, whole = 0;
    if (j < n_pieces) {
        const uint64_t rd = org_read[j];
        first = j == 0 || org_read[j - 1] != rd;
        whole = org_pos[j] == 0 && out_offsets[j + 1] - out_offsets[j] == offsets[rd + 1] - offsets[rd];
    }
    first = wave_sum_u64(first);
    whole = wave_sum_u64(whole);
    if ((threadIdx.x & 63) == 0) {
        if (first) atomicAdd(&tot->with_piece, (unsigned long long)first);
        if (whole) atomicAdd(&tot->intact, (unsigned long long)whole);
    }
}

#endif  // __HIPCC__

}  // namespace dbgk
