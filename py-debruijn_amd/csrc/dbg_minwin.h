// Per-lane arithmetic of the register extraction (k_sk_extract_w, dbg_sk.h): the m-mer hash with its index tag, the
// sliding-window minimum over the lane's packed values and the record-start mask on packed index bytes.
// Plain C++: a host compiler can include this file alone (tests/minwin_host.cpp does).
#pragma once
#include <stdint.h>

#ifndef DBG_MW_HD
#if defined(__HIPCC__)
#define DBG_MW_HD __host__ __device__
#else
#define DBG_MW_HD
#endif
#endif

#if defined(__clang__)
#define DBG_MW_UNROLL _Pragma("unroll")
#else
#define DBG_MW_UNROLL
#endif

namespace dbgk {

// m <= 13: an m-mer is at most 26 bits.  Minimizer order = 16-bit hash, ties to the leftmost.
// one multiply: the minimizer order only has to look random, and this hash runs once per base
DBG_MW_HD inline uint32_t mmer_hash16(uint32_t mmer) { return ((mmer ^ (mmer >> 9) ^ 0x3C6EF372u) * 0x9E3779B1u) >> 16; }

// A lane owns 32 positions and looks at the NV = 32 + W - 1 m-mers its windows reach: index 0 .. 31 start at its own
// positions, 32 .. NV - 1 at the first W - 1 positions of the next lane.  packed = hash16 << 16 | index: the unsigned
// minimum of packed values is the smallest hash, the leftmost of equal ones.  (The hash stays where the multiply left it:
// one and-or per value.  The index is the low byte.)
DBG_MW_HD inline uint32_t mmer_packed(uint32_t mmer, uint32_t idx) { return (mmer_hash16(mmer) << 16) | idx; }

DBG_MW_HD inline uint32_t mw_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// mn[q] = min(pv[q .. q + W - 1]) for the 32 positions, by the van Herk / Gil-Werman block scheme: prefix minima P and
// suffix minima S inside blocks of W, window = min(S[q], P[q + W - 1]) -- about 3 min ops per position whatever W.
template <int W>
DBG_MW_HD inline void window_min32(const uint32_t (&pv)[32 + W - 1], uint32_t (&mn)[32]) {
    constexpr int NV = 32 + W - 1;
    uint32_t P[NV];
DBG_MW_UNROLL
    for (int i = 0; i < NV; ++i) P[i] = (i % W == 0) ? pv[i] : mw_min(P[i - 1], pv[i]);
    uint32_t S = 0xFFFFFFFFu;
DBG_MW_UNROLL
    for (int i = NV - 1; i >= 0; --i) {
        S = (i % W == W - 1 || i == NV - 1) ? pv[i] : mw_min(S, pv[i]);
        if (i < 32) mn[i] = (i % W == 0) ? P[i + W - 1] : mw_min(S, P[i + W - 1]);
    }
}

// ---- record starts ---------------------------------------------------------------------------------------------------
// The index byte of a position: the low byte of its window minimum (index of the minimizer in the lane's array, < 64),
// with MW_NO_KMER set where the position holds no k-mer.  Two neighbouring k-mers share a minimizer occurrence iff their
// index bytes are equal, so a record starts at q iff q holds a k-mer and byte[q - 1] != byte[q].  The 32 bytes are packed
// with a stride of 8: byte b of D[g] belongs to position 8 b + g.  That way the predecessors of D[g] are D[g - 1] as it
// stands, and the per-byte "differs" bits (bit 7 of every byte) shifted down by 7 - g fall on the positions' own bits.
constexpr uint32_t MW_NO_KMER = 0x40u;
constexpr uint32_t MW_NONE = 0x7Fu;  // a predecessor byte that equals no index

DBG_MW_HD inline void pack_index_bytes(const uint32_t (&mn)[32], uint32_t vmask, uint32_t (&D)[8]) {
DBG_MW_UNROLL
    for (int g = 0; g < 8; ++g) {
        const uint32_t d = (mn[g] & 0xFFu) | ((mn[g + 8] & 0xFFu) << 8) | ((mn[g + 16] & 0xFFu) << 16) | (mn[g + 24] << 24);
        const uint32_t nv = ~vmask;  // bits g, g + 8, g + 16, g + 24 -> MW_NO_KMER of bytes 0 .. 3
        D[g] = d | ((g <= 6 ? nv << (6 - g) : nv >> (g - 6)) & (MW_NO_KMER * 0x01010101u));
    }
}

// index byte of position j (0 .. 31) of a lane inside its 32 packed bytes
DBG_MW_HD inline int index_byte_at(int j) { return ((j & 7) << 2) | (j >> 3); }

// What the next lane takes as the predecessor of its position 0: this lane's last index byte in the next lane's terms
// (index - 32).  A minimizer that starts at this lane's position 31: MW_NONE.  No k-mer there: some byte from 0x3F up, which
// equals no index of the next lane's position 0 (at most W - 1) either.
DBG_MW_HD inline uint32_t edge_index_byte(const uint32_t (&D)[8]) { return mw_min((D[7] >> 24) - 32u, MW_NONE); }

// bit q = a record starts at position q.  prev_byte: edge_index_byte of the previous lane (MW_NONE: there is none).
DBG_MW_HD inline uint32_t record_starts(const uint32_t (&D)[8], uint32_t prev_byte, uint32_t vmask) {
    uint32_t prev = (D[7] << 8) | prev_byte;  // positions -1, 7, 15, 23
    uint32_t sm = 0;
DBG_MW_UNROLL
    for (int g = 0; g < 8; ++g) {
        const uint32_t x = D[g] ^ prev;         // every byte is below 0x80 on both sides
        const uint32_t y = x + 0x7F7F7F7Fu;     // bit 7 of a byte: the byte of x is not zero (no carry leaves a byte)
        sm |= (y >> (7 - g)) & (0x01010101u << g);
        prev = D[g];
    }
    return sm & vmask;
}

}  // namespace dbgk
