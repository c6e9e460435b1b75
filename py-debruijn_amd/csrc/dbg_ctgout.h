// Output side of a walk: the text of a list of contigs, bare (the texts concatenated) or as the FASTA records the driver
// writes (">SEQUENCE_{number}_{k}mer\n{contig}\n"), produced window by window so that neither side holds all of it
// (dbg_export_contig_texts, dbg_write_contigs_fasta).
//
// The output is a virtual text: record i of the list starts at byte pos[i] (prefix sum of the record lengths) and the
// whole has pos[n] = total bytes.  A window is a run [b0, b1) of it, b0 a multiple of CO_TILE.  The work is balanced over
// the output bytes, not over the contigs (the shape of k_score_sequences, dbg_lookup.h): a workgroup takes CO_TILE
// consecutive bytes, a thread CO_RUN of them, which it assembles in registers and writes with one 16-byte store.  Two
// lanes of the workgroup search pos[] for the records of the tile's first and last byte; every thread then finds its own
// record between those two (no step at all where one contig covers the tile).  Inside its run a thread pays one
// binary-lifting descent for the first contig character it meets and follows level 0 of the table from there:
// character j >= k of the contig that starts at s is the last character of s's (j - k + 1)-th chain successor, and the
// characters j < k are those of s's own k-mer.
//
// The first part of this file -- record lengths, the map from a byte of a record to its field, the window planner and
// the run emitter itself -- is plain C++: a host compiler can include this file alone (tests/test_ctgout_host.py does).
// The device text sources and the kernel follow under __HIPCC__.
#pragma once
#include <stdint.h>

#ifndef DBG_CO_HD
#if defined(__HIPCC__)
#define DBG_CO_HD __host__ __device__
#else
#define DBG_CO_HD
#endif
#endif

namespace dbgk {

constexpr int CO_RUN = 16;                    // bytes of a thread: one 16-byte store
constexpr int CO_NT = 256;
constexpr int CO_TILE = CO_RUN * CO_NT;       // bytes of a workgroup
constexpr uint64_t CO_DEFAULT_CHUNK = 4ull << 20;  // measured best of 4 / 16 / 64 MiB: pinning the buffers costs more than larger windows save
constexpr uint64_t CO_MAX_CHUNK = 1ull << 30;

// ---- one record ------------------------------------------------------------------------------------------------------------
enum CoField : int { CO_KEYWORD = 0, CO_NUMBER, CO_USCORE, CO_KDIGITS, CO_MER, CO_TEXT, CO_NEWLINE };

DBG_CO_HD inline uint32_t co_digits(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

// ">SEQUENCE_" + number + "_" + k + "mer\n"
DBG_CO_HD inline uint64_t co_header_len(uint32_t n_digits, uint32_t k_digits) { return 10ull + n_digits + 1ull + k_digits + 4ull; }

// bytes of a record whose contig has `len` characters; bare mode: the contig alone
DBG_CO_HD inline uint64_t co_record_len(bool fasta, uint64_t number, uint32_t k_digits, uint64_t len) {
    return fasta ? co_header_len(co_digits(number), k_digits) + len + 1ull : len;
}

// digit q (0 = leftmost) of the n_digits-digit number v
DBG_CO_HD inline char co_digit_at(uint64_t v, uint32_t n_digits, uint32_t q) {
    for (uint32_t s = n_digits - 1 - q; s; --s) v /= 10;
    return (char)('0' + v % 10);
}

struct CoWhere {
    int field;    // CoField
    uint64_t at;  // offset inside the field
};

// which field byte `rel` of a FASTA record lies in (rel < record length)
DBG_CO_HD inline CoWhere co_field_at(uint64_t rel, uint32_t n_digits, uint32_t k_digits, uint64_t len) {
    if (rel < 10) return CoWhere{CO_KEYWORD, rel};
    rel -= 10;
    if (rel < n_digits) return CoWhere{CO_NUMBER, rel};
    rel -= n_digits;
    if (rel < 1) return CoWhere{CO_USCORE, 0};
    rel -= 1;
    if (rel < k_digits) return CoWhere{CO_KDIGITS, rel};
    rel -= k_digits;
    if (rel < 4) return CoWhere{CO_MER, rel};
    rel -= 4;
    if (rel < len) return CoWhere{CO_TEXT, rel};
    return CoWhere{CO_NEWLINE, rel - len};
}

// the byte of every field but the contig text
DBG_CO_HD inline char co_fixed_char(CoWhere w, uint64_t number, uint32_t n_digits, uint32_t k_label, uint32_t k_digits) {
    switch (w.field) {
    case CO_KEYWORD: return ">SEQUENCE_"[w.at];
    case CO_NUMBER: return co_digit_at(number, n_digits, (uint32_t)w.at);
    case CO_USCORE: return '_';
    case CO_KDIGITS: return co_digit_at(k_label, k_digits, (uint32_t)w.at);
    case CO_MER: return "mer\n"[w.at];
    default: return '\n';
    }
}

// ---- wrapped records (dbg_write_contigs_fasta_wrapped): the contig in lines of line_width characters ------------------------
// bytes of a record's body, the contig and its line ends: every line ends with '\n', the last may be shorter, a contig of
// no characters keeps its one '\n' and a contig of a whole number of lines gets no empty line.  line_width 0: one line.
DBG_CO_HD inline uint64_t co_body_len(uint64_t len, uint32_t line_width) {
    if (!line_width || !len) return len + 1ull;
    return len + (len + line_width - 1ull) / line_width;
}

DBG_CO_HD inline uint64_t co_record_len_wrapped(uint64_t number, uint32_t k_digits, uint64_t len, uint32_t line_width) {
    return co_header_len(co_digits(number), k_digits) + co_body_len(len, line_width);
}

// byte q of a body of `body` bytes: false for a '\n', else true and *j = the contig character it holds
DBG_CO_HD inline bool co_body_char(uint64_t q, uint64_t body, uint32_t line_width, uint64_t *j) {
    if (q + 1 == body) return false;
    if (!line_width) { *j = q; return true; }
    const uint64_t line = q / (line_width + 1ull);
    if (q - line * (line_width + 1ull) == line_width) return false;
    *j = q - line;
    return true;
}

// co_field_at for a wrapped record: CO_TEXT carries the contig character, CO_NEWLINE the byte of the body
DBG_CO_HD inline CoWhere co_field_at_wrapped(uint64_t rel, uint32_t n_digits, uint32_t k_digits, uint64_t len, uint32_t line_width) {
    const uint64_t hdr = co_header_len(n_digits, k_digits);
    if (rel < hdr) return co_field_at(rel, n_digits, k_digits, len);
    uint64_t j = 0;
    if (co_body_char(rel - hdr, co_body_len(len, line_width), line_width, &j)) return CoWhere{CO_TEXT, j};
    return CoWhere{CO_NEWLINE, rel - hdr};
}

// ---- windows ---------------------------------------------------------------------------------------------------------------
struct CoWindow {
    uint64_t b0, b1;  // bytes [b0, b1) of the virtual text
    uint64_t tiles;   // workgroups that fill it
};

DBG_CO_HD inline bool co_chunk_ok(uint64_t chunk) { return chunk % (uint64_t)CO_TILE == 0; }
DBG_CO_HD inline uint64_t co_n_windows(uint64_t total, uint64_t chunk) { return (total + chunk - 1) / chunk; }
DBG_CO_HD inline CoWindow co_window(uint64_t total, uint64_t chunk, uint64_t c) {
    CoWindow w;
    w.b0 = c * chunk;
    w.b1 = total - w.b0 < chunk ? total : w.b0 + chunk;
    w.tiles = (w.b1 - w.b0 + (uint64_t)CO_TILE - 1) / (uint64_t)CO_TILE;
    return w;
}
// bytes of a staging buffer: a window, never more than the text rounded up to whole tiles (every store is a full 16 bytes)
DBG_CO_HD inline uint64_t co_stage_bytes(uint64_t total, uint64_t chunk) {
    const uint64_t whole = (total + (uint64_t)CO_TILE - 1) / (uint64_t)CO_TILE * (uint64_t)CO_TILE;
    return whole < chunk ? whole : chunk;
}

// ---- the virtual text ------------------------------------------------------------------------------------------------------
struct CoText {
    const uint64_t *pos;    // [n] first byte of every record
    const uint32_t *list;   // [n] contig of every record; null: record i is contig i
    const uint64_t *off;    // contig offsets of the walk (contig c has off[c + 1] - off[c] characters)
    uint64_t n, total;      // records, bytes
    uint64_t first_number;  // record i is numbered first_number + i
    uint32_t k_label, k_digits;
    int fasta;              // 0: bare texts
    uint32_t line_width = 0;  // FASTA records: characters of a line of the contig (0: the contig on one line); set last, by those who wrap
};

// Last record i in [lo, hi) with pos[i] <= b; needs pos[lo] <= b.  Taking the last skips records of no bytes.
DBG_CO_HD inline uint64_t co_find_record(const uint64_t *pos, uint64_t lo, uint64_t hi, uint64_t b) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (pos[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The CO_RUN bytes from b on (fewer at the end of the text; the rest stay zero), b inside record `rec`, packed little-endian
// into w[4].  Src spells contigs: first(c, j) is character j of contig c and opens a cursor there, next(j) is the
// character behind the last one asked for (j counts on: the cursor never jumps -- the '\n' bytes of a wrapped contig ask
// nothing).
template <class Src>
DBG_CO_HD inline void co_fill_run(const CoText &t, uint64_t rec, uint64_t b, Src &src, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    uint64_t rel = b - t.pos[rec];
    uint32_t c = t.list ? t.list[rec] : (uint32_t)rec, nd = 0;
    uint64_t len = t.off[c + 1] - t.off[c], number = t.first_number + rec, hdr = 0, rec_len = len;
    const uint32_t lw = t.fasta ? t.line_width : 0u;  // bare texts are never wrapped
    if (t.fasta) { nd = co_digits(number); hdr = co_header_len(nd, t.k_digits); rec_len = hdr + co_body_len(len, lw); }
    bool open = false;
#if defined(__HIPCC__)
#pragma unroll  // w[] is indexed by constants: it stays in registers
#endif
    for (int q = 0; q < CO_RUN; ++q) {
        if (b + (uint64_t)q >= t.total) break;
        while (rel >= rec_len) {  // the next record (b + q < total: there is one)
            rel -= rec_len;
            ++rec;
            c = t.list ? t.list[rec] : (uint32_t)rec;
            len = t.off[c + 1] - t.off[c];
            rec_len = len;
            if (t.fasta) { number = t.first_number + rec; nd = co_digits(number); hdr = co_header_len(nd, t.k_digits); rec_len = hdr + co_body_len(len, lw); }
            open = false;
        }
        char ch;
        uint64_t j = rel - hdr;
        if (lw ? (rel >= hdr && co_body_char(rel - hdr, rec_len - hdr, lw, &j)) : (rel >= hdr && rel < hdr + len)) {
            ch = open ? src.next(j) : src.first(c, j);
            open = true;
        } else {
            ch = co_fixed_char(co_field_at(rel, nd, t.k_digits, len), number, nd, t.k_label, t.k_digits);
        }
        w[q >> 2] |= (uint32_t)(uint8_t)ch << (8 * (q & 3));
        ++rel;
    }
}

}  // namespace dbgk

#if defined(__HIPCC__)
namespace dbgk {

// contigs of a materialised walk
struct CoCharsSrc {
    const char *chars;
    const uint64_t *off;
    const char *p;
    __device__ inline char first(uint32_t c, uint64_t j) { p = chars + off[c]; return p[j]; }
    __device__ inline char next(uint64_t j) const { return p[j]; }
};

// contigs of an index-only walk: start node and the binary-lifting tables of the chain successors (up[l * n_nodes + x] is
// the 2^l-th successor of x)
template <class G>
struct CoLiftSrc {
    G g;
    const uint32_t *start;
    const uint32_t *up;
    uint64_t n_nodes;
    int levels;
    uint32_t s, x;  // cursor: the contig's start node, the node whose last character was spelled last
    __device__ inline char first(uint32_t c, uint64_t j) {
        s = x = start[c];
        if (j < (uint64_t)g.k) return g.char_at(s, (int)j);
        uint64_t d = j - (uint64_t)g.k + 1;
        for (int l = 0; l < levels && d; ++l, d >>= 1)
            if (d & 1) x = up[(uint64_t)l * n_nodes + x];
        return g.sym_char(g.last_code(x));
    }
    __device__ inline char next(uint64_t j) {
        if (j < (uint64_t)g.k) return g.char_at(s, (int)j);
        x = up[x];
        return g.sym_char(g.last_code(x));
    }
};

// out[b - b0] for the bytes b of window [b0, b1): grid = the window's tiles, out 16-byte aligned with room for whole runs
template <class Src>
__global__ __launch_bounds__(CO_NT) void k_ctg_window(CoText t, uint64_t b0, uint64_t b1, Src src, char *__restrict__ out) {
    __shared__ uint64_t s_rec[2];
    const uint64_t tile0 = b0 + (uint64_t)blockIdx.x * CO_TILE;
    if (threadIdx.x == 0 || threadIdx.x == 64) {  // two waves: the searches run side by side
        uint64_t last = tile0 + (uint64_t)CO_TILE - 1;
        if (last >= b1) last = b1 - 1;
        s_rec[threadIdx.x ? 1 : 0] = co_find_record(t.pos, 0, t.n, threadIdx.x ? last : tile0);
    }
    __syncthreads();
    const uint64_t b = tile0 + (uint64_t)threadIdx.x * CO_RUN;
    if (b >= b1) return;
    const uint64_t rec = co_find_record(t.pos, s_rec[0], s_rec[1] + 1, b);
    uint32_t w[4];
    co_fill_run(t, rec, b, src, w);
    *reinterpret_cast<uint4 *>(out + (b - b0)) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace dbgk
#endif  // __HIPCC__
