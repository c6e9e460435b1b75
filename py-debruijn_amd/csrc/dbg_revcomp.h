// Both strands of the resident reads (dbg_add_revcomp): the reads r0, r1, ... become r0, rc(r0), r1, rc(r1), ...
// With n reads, N bytes and offsets o[] (len_i = o[i+1] - o[i]):
//   out_off[2i] = 2 o[i],  out_off[2i+1] = 2 o[i] + len_i,  out_off[2n] = 2N           (closed form: no scan)
//   out[2 o[i] + j]         = in[o[i] + j]                                              (strand 0, the read as it is)
//   out[2 o[i] + len_i + j] = comp(in[o[i] + len_i - 1 - j])                            (strand 1, j & 1 of the new index)
// comp swaps A<->T, C<->G, a<->t, c<->g and leaves every other byte (of 256) as it is.
//
// The pass is a stream: N bytes read, 2N written.  k_rc_tile works by tiles of RC_TILE_BYTES bytes of the OUTPUT:
//   * one upper-bound search in the input offsets (doubled on the fly; 256 probes a round) finds the read that holds the
//     tile's first byte,
//   * the next RC_SLICE_READS + 1 offsets go to LDS, and the searches of the chunks end at the last read that begins in
//     the tile; a tile that holds more reads than the slice (long runs of empty reads) searches the global offsets per
//     thread instead,
//   * a thread makes 16 aligned output bytes at a time, strand by strand: for a strand with bytes in the chunk it loads the
//     16 source bytes that would fill the whole chunk with one or two aligned 16-byte loads, shifts them into place, for
//     strand 1 reverses them in registers (byte-reverse every dword, swap the dword order) and complements them four
//     bytes at a time, and keeps the strand's bytes under a mask; one 16-byte store.  Only a source window that begins
//     in front of the buffer, or whose second load would end behind a buffer without padding, is read byte by byte.
//   * bytes that comp leaves alone are counted on strand 1, where comp runs anyway (every input byte is there once),
//     summed through LDS, one atomic per workgroup.
// k_rc_offsets writes the offsets, k_rc_origins doubles the origins of an earlier split, k_rc_palindromes (one wave per
// read, a second small kernel: fusing it would make k_rc_tile keep state across tiles) counts the reads that equal their
// reverse complement.  All positions are 64 bits wide.
//
// The word helpers are plain C++: a host compiler can include this file alone (tests/revcomp_host.cpp does).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef DBG_RC_HD
#if defined(__HIPCC__)
#define DBG_RC_HD __host__ __device__
#else
#define DBG_RC_HD
#endif
#endif

namespace dbgk {

constexpr int RC_CHUNK_BYTES = 16;                                               // output bytes a thread makes at a time
constexpr int RC_CHUNKS_PER_THREAD = 8;                                          // chunks of a thread, 256 chunks apart
constexpr int RC_TILE_BYTES = 256 * RC_CHUNKS_PER_THREAD * RC_CHUNK_BYTES;       // output bytes per workgroup (32 KiB)
constexpr int RC_SLICE_READS = 1024;                                             // reads whose offsets a tile keeps in LDS

// ---- word helpers (host and device) --------------------------------------------------------------------------------------

// the complement of one byte
DBG_RC_HD inline uint32_t rc_comp1(uint32_t c) {
    const uint32_t u = c | 0x20u;
    if (u == 'a' || u == 't') return c ^ 0x15u;  // 'A' ^ 'T'
    if (u == 'c' || u == 'g') return c ^ 0x04u;  // 'C' ^ 'G'
    return c;
}

// 0x80 in every byte of x that is zero, 0 in the others (exact: no carry crosses a byte)
DBG_RC_HD inline uint32_t rc_zero_bytes(uint32_t x) {
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// the complement of four packed bytes.  *moved gets 0x80 in every byte that changed.
DBG_RC_HD inline uint32_t rc_comp4(uint32_t v, uint32_t *moved) {
    // v | 0x20 is 'a' exactly for 'A' and 'a' (the two differ in that bit alone); y: a -> 0x00, c -> 0x02, g -> 0x06, t -> 0x15
    const uint32_t y = (v | 0x20202020u) ^ 0x61616161u;
    const uint32_t at = rc_zero_bytes(y) | rc_zero_bytes(y ^ 0x15151515u);
    const uint32_t cg = rc_zero_bytes((y & 0xFBFBFBFBu) ^ 0x02020202u);  // 0x02 and 0x06 differ in bit 2 alone
    *moved = at | cg;
    return v ^ ((at >> 7) * 0x15u) ^ ((cg >> 7) * 0x04u);
}
DBG_RC_HD inline uint64_t rc_comp8(uint64_t v) {
    uint32_t m;
    return (uint64_t)rc_comp4((uint32_t)v, &m) | ((uint64_t)rc_comp4((uint32_t)(v >> 32), &m) << 32);
}
// sixteen bytes as four little-endian dwords, in place -> how many of them comp leaves as they are
DBG_RC_HD inline int rc_comp16(uint32_t (&v)[4]) {
    int other = 16;
    for (int i = 0; i < 4; ++i) {
        uint32_t m;
        v[i] = rc_comp4(v[i], &m);
        other -= __builtin_popcount(m);
    }
    return other;
}
// how many of sixteen bytes comp leaves as they are
DBG_RC_HD inline int rc_other16(const uint32_t (&v)[4]) {
    uint32_t t[4] = {v[0], v[1], v[2], v[3]};
    return rc_comp16(t);
}

// sixteen bytes in reverse order: every dword byte-reversed, the dwords swapped
DBG_RC_HD inline void rc_reverse16(uint32_t (&v)[4]) {
    const uint32_t a = __builtin_bswap32(v[3]), b = __builtin_bswap32(v[2]);
    v[3] = __builtin_bswap32(v[0]);
    v[2] = __builtin_bswap32(v[1]);
    v[0] = a;
    v[1] = b;
}

// bytes s .. s+15 (0 <= s <= 15) of the 32 bytes w (eight little-endian dwords; with s == 0 the upper four are not looked at)
DBG_RC_HD inline void rc_extract16(const uint32_t (&w)[8], uint32_t s, uint32_t (&out)[4]) {
    uint64_t a = w[0] | ((uint64_t)w[1] << 32), b = w[2] | ((uint64_t)w[3] << 32);
    uint64_t c = w[4] | ((uint64_t)w[5] << 32);
    const uint64_t d = w[6] | ((uint64_t)w[7] << 32);
    if (s & 8u) { a = b; b = c; c = d; }
    const uint32_t r = 8u * (s & 7u);
    if (r) {
        a = (a >> r) | (b << (64u - r));
        b = (b >> r) | (c << (64u - r));
    }
    out[0] = (uint32_t)a; out[1] = (uint32_t)(a >> 32);
    out[2] = (uint32_t)b; out[3] = (uint32_t)(b >> 32);
}

struct RcPlace {
    uint64_t read;    // index into the offsets that were searched
    uint64_t src;     // position of the source byte in the input bases
    uint64_t seg_end; // output position behind the last byte of this strand of this read
    uint32_t strand;  // 0: the read as it is, 1: its reverse complement
};

// Where output byte q comes from.  off: input offsets, of which entries [lo, hi] are looked at; the caller guarantees
// 2 off[lo] <= q < 2 off[hi].  The read is the last i in [lo, hi) with 2 off[i] <= q: the empty reads in front of it share
// its offset and hold nothing.
DBG_RC_HD inline RcPlace rc_locate(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t q) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (2 * off[mid] <= q) lo = mid; else hi = mid;
    }
    const uint64_t o = off[lo], len = off[lo + 1] - o, j = q - 2 * o;
    RcPlace p;
    p.read = lo;
    p.strand = j >= len ? 1u : 0u;
    p.src = p.strand ? o + (2 * len - 1 - j) : o + j;
    p.seg_end = 2 * o + len + (p.strand ? len : 0);
    return p;
}
// the strand that follows p's in the output (hi as in rc_locate; the caller knows that one follows in front of 2 off[hi]):
// strand 1 of the same read, which starts at the read's last byte, or strand 0 of the next read that is not empty
DBG_RC_HD inline RcPlace rc_next_strand(const uint64_t *off, uint64_t hi, RcPlace p) {
    if (!p.strand) {
        const uint64_t len = off[p.read + 1] - off[p.read];
        p.strand = 1;
        p.src = off[p.read + 1] - 1;
        p.seg_end += len;
        return p;
    }
    uint64_t i = p.read + 1;
    while (i + 1 < hi && off[i + 1] == off[i]) ++i;
    p.read = i;
    p.strand = 0;
    p.src = off[i];
    p.seg_end = 2 * off[i] + (off[i + 1] - off[i]);
    return p;
}

// 0xFF in bytes [lo, hi) of a 64-bit word (lo, hi <= 8; hi <= lo: none)
DBG_RC_HD inline uint64_t rc_mask64(uint32_t lo, uint32_t hi) {
    const uint64_t below_hi = hi >= 8 ? ~0ull : (1ull << (8 * hi)) - 1ull;
    const uint64_t below_lo = lo >= 8 ? ~0ull : (1ull << (8 * lo)) - 1ull;
    return below_hi & ~below_lo;
}

// sixteen bytes at p (16-byte aligned) as four little-endian dwords
DBG_RC_HD inline void rc_load16(const char *p, uint32_t *w) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 x = *reinterpret_cast<const uint4 *>(p);
    w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
#else
    memcpy(w, p, 16);
#endif
}

// The sixteen bytes at position first of the input -> w.  Any alignment: one aligned 16-byte load, or two and a shift.
// A window that begins in front of the buffer, or whose loads would end behind the n_in_safe bytes that may be read (N,
// plus the padding where the handle owns the buffer), is read byte by byte, and its bytes outside [0, n) come out as 0.
DBG_RC_HD inline void rc_window16(const char *in, uint64_t n, uint64_t n_in_safe, int64_t first, uint32_t (&v)[4]) {
    if (first >= 0) {
        const uint64_t a = (uint64_t)first & ~(uint64_t)15;
        const uint32_t s = (uint32_t)first & 15u;
        if (a + (s ? 32 : 16) <= n_in_safe) {
            uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            rc_load16(in + a, w);
            if (s) rc_load16(in + a + 16, w + 4);
            rc_extract16(w, s, v);
            return;
        }
    }
    v[0] = v[1] = v[2] = v[3] = 0;
    for (int b = 0; b < RC_CHUNK_BYTES; ++b) {
        const int64_t pos = first + b;
        if (pos >= 0 && (uint64_t)pos < n) v[b >> 2] |= (uint32_t)(uint8_t)in[pos] << (8 * (b & 3));
    }
}

// 16 output bytes at q (a multiple of 16, q < n2 = 2N) -> v; returns the strand-1 bytes among them that comp leaves alone.
// off / lo / hi: as in rc_locate.  The chunk is put together strand by strand: for each strand that has bytes in it, the
// sixteen source bytes that would fill the whole chunk are loaded as one window (reversed and complemented for strand 1),
// and the bytes that belong to the strand are kept.  Most chunks lie in one strand; few touch more than two.
DBG_RC_HD inline uint32_t rc_make_chunk(const char *in, uint64_t n_in_safe, const uint64_t *off, uint64_t lo,
                                         uint64_t hi, uint64_t q, uint64_t n2, uint32_t (&v)[4]) {
    RcPlace p = rc_locate(off, lo, hi, q);
    const uint64_t end = q + RC_CHUNK_BYTES < n2 ? q + RC_CHUNK_BYTES : n2;  // the padding behind the last read stays zero
    uint64_t out_lo = 0, out_hi = 0, q1 = q;
    uint32_t other = 0;
    for (;;) {
        const uint64_t e = p.seg_end < end ? p.seg_end : end;  // this strand has the bytes [q1, e)
        const uint32_t b0 = (uint32_t)(q1 - q), b1 = (uint32_t)(e - q);
        const uint64_t m_lo = rc_mask64(b0 < 8 ? b0 : 8, b1 < 8 ? b1 : 8);
        const uint64_t m_hi = rc_mask64(b0 > 8 ? b0 - 8 : 0, b1 > 8 ? b1 - 8 : 0);
        uint32_t w[4];
        if (!p.strand) {  // output byte q + b is in[p.src - b0 + b]: a copy
            rc_window16(in, n2 / 2, n_in_safe, (int64_t)p.src - (int64_t)b0, w);
        } else {  // output byte q + b is comp(in[p.src + b0 - b]): the window [p.src + b0 - 15, p.src + b0], backwards
            rc_window16(in, n2 / 2, n_in_safe, (int64_t)p.src + (int64_t)b0 - (RC_CHUNK_BYTES - 1), w);
            rc_reverse16(w);
            uint32_t moved[4];
            for (int i = 0; i < 4; ++i) w[i] = rc_comp4(w[i], &moved[i]);
            other += (b1 - b0) - (uint32_t)(__builtin_popcount(moved[0] & (uint32_t)m_lo) + __builtin_popcount(moved[1] & (uint32_t)(m_lo >> 32)) +
                                            __builtin_popcount(moved[2] & (uint32_t)m_hi) + __builtin_popcount(moved[3] & (uint32_t)(m_hi >> 32)));
        }
        out_lo |= (w[0] | ((uint64_t)w[1] << 32)) & m_lo;
        out_hi |= (w[2] | ((uint64_t)w[3] << 32)) & m_hi;
        if (e >= end) break;
        p = rc_next_strand(off, hi, p);
        q1 = e;
    }
    v[0] = (uint32_t)out_lo; v[1] = (uint32_t)(out_lo >> 32);
    v[2] = (uint32_t)out_hi; v[3] = (uint32_t)(out_hi >> 32);
    return other;
}

#if defined(__HIPCC__)
}  // namespace dbgk
#include "dbg_device.h"
namespace dbgk {

struct RcTotals {
    unsigned long long other;        // input bytes comp leaves as they are
    unsigned long long palindromes;  // reads of at least one byte that equal their reverse complement
};

// one workgroup per tile of RC_TILE_BYTES output bytes.  out has room for n2 rounded up to 16 bytes (its padding).
__global__ __launch_bounds__(256) void k_rc_tile(const char *__restrict__ in, uint64_t n_in_safe,
                                                 const uint64_t *__restrict__ offsets, uint64_t n_reads, char *__restrict__ out,
                                                 uint64_t n2, RcTotals *tot) {
    __shared__ uint64_t s_off[RC_SLICE_READS + 1];
    __shared__ uint32_t s_other[4];
    const uint64_t t0 = (uint64_t)blockIdx.x * RC_TILE_BYTES;
    const uint64_t t1 = t0 + RC_TILE_BYTES < n2 ? t0 + RC_TILE_BYTES : n2;
    // the read that holds the tile's first byte: the last i with 2 offsets[i] <= t0.  256 probes a round, one per thread,
    // so 16 M reads take three dependent loads and not twenty-four
    uint64_t i0 = 0, hi = n_reads;
    while (hi - i0 > 1) {
        const uint64_t step = (hi - i0 + 255) / 256, idx = i0 + threadIdx.x * step;
        const int below = __syncthreads_count(idx < hi && 2 * offsets[idx] <= t0);  // a prefix of the threads; thread 0 always
        i0 += (uint64_t)(below - 1) * step;
        hi = i0 + step < hi ? i0 + step : hi;
    }
    const uint64_t cnt = n_reads - i0 < (uint64_t)RC_SLICE_READS ? n_reads - i0 : (uint64_t)RC_SLICE_READS;
    for (uint64_t i = threadIdx.x; i <= cnt; i += 256) s_off[i] = offsets[i0 + i];
    __syncthreads();
    // reads of the slice that begin in front of the tile's end: the searches of the chunks look no further
    uint32_t n_in = 0;
    for (uint32_t base = 0; base <= (uint32_t)cnt; base += 256) {
        const uint32_t i = base + threadIdx.x;
        n_in += (uint32_t)__syncthreads_count(i <= (uint32_t)cnt && 2 * s_off[i] < t1);
    }
    const bool in_slice = n_in <= (uint32_t)cnt;  // else: more reads in this tile than the slice holds
    uint32_t other = 0;
#pragma unroll 2
    for (int c = 0; c < RC_CHUNKS_PER_THREAD; ++c) {
        const uint64_t q = t0 + ((uint64_t)c * 256 + threadIdx.x) * RC_CHUNK_BYTES;
        if (q >= t1) break;
        uint32_t v[4];
        if (in_slice) other += rc_make_chunk(in, n_in_safe, s_off, 0, n_in, q, n2, v);
        else other += rc_make_chunk(in, n_in_safe, offsets, i0, n_reads, q, n2, v);
        *reinterpret_cast<uint4 *>(out + q) = make_uint4(v[0], v[1], v[2], v[3]);
    }
    const uint64_t wsum = wave_sum_u64(other);
    if ((threadIdx.x & 63) == 0) s_other[threadIdx.x >> 6] = (uint32_t)wsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = (unsigned long long)s_other[0] + s_other[1] + s_other[2] + s_other[3];
        if (sum) atomicAdd(&tot->other, sum);
    }
}

// out_off[2i], out_off[2i+1] for read i < n_reads; out_off[2 n_reads] = 2N
__global__ __launch_bounds__(256) void k_rc_offsets(const uint64_t *__restrict__ offsets, uint64_t n_reads, uint64_t *out_off) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_reads) {
        const uint64_t o = offsets[i], len = offsets[i + 1] - o;
        *reinterpret_cast<ulonglong2 *>(out_off + 2 * i) = make_ulonglong2(2 * o, 2 * o + len);
    } else if (i == n_reads) {
        out_off[2 * i] = 2 * offsets[i];
    }
}

// the origins of the pieces of an earlier split: both strands of piece i carry piece i's
__global__ __launch_bounds__(256) void k_rc_origins(const uint64_t *__restrict__ org_read, const uint64_t *__restrict__ org_pos,
                                                    uint64_t n_reads, uint64_t *out_read, uint64_t *out_pos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const uint64_t r = org_read[i], p = org_pos[i];
    *reinterpret_cast<ulonglong2 *>(out_read + 2 * i) = make_ulonglong2(r, r);
    *reinterpret_cast<ulonglong2 *>(out_pos + 2 * i) = make_ulonglong2(p, p);
}

// one wave per read at a time (grid-stride): in[o + j] == comp(in[o + len - 1 - j]) for every j of the first half, the
// middle byte of an odd length included.  One atomic per workgroup.
__global__ __launch_bounds__(256) void k_rc_palindromes(const char *__restrict__ in, const uint64_t *__restrict__ offsets,
                                                        uint64_t n_reads, RcTotals *tot) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t lane = threadIdx.x & 63;
    uint32_t found = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n_reads; i += (uint64_t)gridDim.x * 4) {
        const uint64_t o = offsets[i], len = offsets[i + 1] - o, half = (len + 1) / 2;
        if (!len) continue;
        bool same = true;
        for (uint64_t j0 = 0; j0 < half && same; j0 += 64) {  // same is uniform in the wave
            const uint64_t j = j0 + lane;
            bool ok = true;
            if (j < half) ok = (uint32_t)(uint8_t)in[o + j] == rc_comp1((uint8_t)in[o + len - 1 - j]);
            same = __all(ok);
        }
        found += same;
    }
    if (lane == 0) s_cnt[threadIdx.x >> 6] = found;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = (unsigned long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (sum) atomicAdd(&tot->palindromes, sum);
    }
}

#endif  // __HIPCC__

}  // namespace dbgk
