// Directory of one counted range, and what the resolvers can tell from one entry of it without reading a key.
// Plain C++: a host compiler can include this file alone (tests/test_resolve_direct.py does).
#pragma once
#include <stdint.h>

#ifndef DBG_DIR_HD
#if defined(__HIPCC__)
#define DBG_DIR_HD __host__ __device__
#else
#define DBG_DIR_HD
#endif
#endif

namespace dbgk {

// Per 64-slot block of a range's LDS table: the occupancy mask and the node id of the block's first node.  The nodes of
// a block are written in slot order, so (mask, base) turn a slot into a node id and k_succ_resolve can repeat the
// table's linear probing against the node keys in HBM -- a successor that lives in another bucket costs the asker one
// read of this entry and, unless dir_decide settles it, a second dependent read of the key run, instead of a trip
// through a multisplit of all such queries.
struct SkDirEnt {
    unsigned long long mask;
    uint32_t base;
    uint32_t pad;  // bit 0 (DIR_WHOLE_BUCKET); the other bits are zero
};
static_assert(sizeof(SkDirEnt) == 16, "directory entry");

constexpr uint32_t DIR_WHOLE_BUCKET = 1u;  // the whole bucket is this one range (the resolver need not ask the ranges)

// The node of a k-mer that is KNOWN to be in the table, from the entry of its home slot's block alone.  `bit` is the
// home slot's index inside the block.  Linear probing without deletions keeps a key in the run of occupied slots that
// starts at its home slot, so the key is named without a comparison iff
//   - the home slot is occupied,
//   - that run ends before bit 64 of this block (a run that reaches the block's end may go on in the next block:
//     never decided), and
//   - the run holds exactly one slot.
// Returns true and *node = base + popcount(mask below the slot) then; false means "read the keys".  A k-mer that is
// NOT in the table can be decided too, wrongly: only callers whose queries exist by construction may use this.
DBG_DIR_HD inline bool dir_decide(const SkDirEnt &de, int bit, uint64_t *node) {
    if (bit >= 63) return false;  // a run from bit 63 reaches the block's end
    if (((de.mask >> bit) & 3ull) != 1ull) return false;  // home slot empty, or the run goes on
    const unsigned long long below = de.mask & ((1ull << bit) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
    *node = (uint64_t)de.base + (uint64_t)__popcll(below);
#else
    *node = (uint64_t)de.base + (uint64_t)__builtin_popcountll(below);
#endif
    return true;
}

}  // namespace dbgk
