// Kernels of the global-table build (a3 + a4): table init, encode + hash insert + successor counters, the gather into
// node arrays, successor resolution and the CSR.
// A section of the one translation unit dbg_hip.hip, not self-contained: it needs dbg_device.h (Slot, the hash, the
// tile loader) in front of it.

// ------------------------------------------------------------------------------------------
// a3 + a4: encode, hash insert, successor counters, first-occurrence stamp
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_table_init(Slot *tab, uint64_t cap) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) {
        uint4 *p = reinterpret_cast<uint4 *>(tab + i);
        p[0] = make_uint4(~0u, ~0u, ~0u, ~0u);
        p[1] = make_uint4(0, 0, 0, 0);
    }
}

__global__ __launch_bounds__(256) void k_count(const char *__restrict__ bases, uint64_t n_bytes,
                                               const uint32_t *__restrict__ startbits, int k, Slot *tab,
                                               uint64_t cap_mask, int hash_shift, uint32_t *occ,
                                               unsigned long long *scalars) {
    __shared__ TileLds t;
    const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;
    const uint32_t bad = load_tile(t, bases, n_bytes, startbits, tile0);
    if (bad) atomicOr(&scalars[0], STATUS_BAD_BASE);
    __syncthreads();

    const uint32_t mid_mask = (k >= 2) ? ((1u << (k - 1)) - 1u) : 0u;
    uint64_t n_k = 0, n_e = 0;
    for (int j = threadIdx.x; j < TILE; j += 256) {
        const uint64_t p = tile0 + j;
        if (p >= n_bytes) break;
        const uint32_t sw = startwin32(t, j);
        if ((sw >> 1) & mid_mask) continue;        // a read boundary inside the k-mer
        const uint32_t s0 = sw & 1u;                // k-mer sits at position 0 of its read
        const uint32_t sk = (sw >> k) & 1u;         // position p+k starts another read (or is the end)
        if (sk && s0) continue;                     // read of length exactly k: contributes nothing [:126]
        const uint64_t win = window32(t, j);
        const uint64_t kmer = win >> (64 - 2 * k);
        const uint32_t b = (uint32_t)(win >> (62 - 2 * k)) & 3u;
        const uint64_t stamp = (p << 1) | (s0 ^ 1u);
        n_k += 1;
        n_e += sk ^ 1u;

        uint64_t slot = kmer_hash(kmer) >> hash_shift;
        bool found = false;
        for (uint64_t probe = 0; probe <= cap_mask; ++probe) {
            unsigned long long cur =
                __hip_atomic_load(&tab[slot].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == EMPTY_KEY) {
                cur = atomicCAS(&tab[slot].key, EMPTY_KEY, (unsigned long long)kmer);
                if (cur == EMPTY_KEY) {
                    atomicOr(&occ[slot >> 5], 1u << (slot & 31));
                    cur = kmer;
                }
            }
            if (cur == kmer) { found = true; break; }
            slot = (slot + 1) & cap_mask;
        }
        if (!found) { atomicOr(&scalars[0], STATUS_TABLE_FULL); continue; }  // table full
        if (!sk) atomicAdd(&tab[slot].cnt[b], 1u);
        atomicMin(&tab[slot].stamp, (unsigned long long)stamp);
    }
    // one update per workgroup and counter: these are same-address atomics (serialised chip-wide, ~12 ns each)
    uint64_t tot_k, tot_e;
    (void)block_exscan_256(n_k, &tot_k);
    (void)block_exscan_256(n_e, &tot_e);
    if (threadIdx.x == 0) {
        if (tot_k) atomicAdd(&scalars[1], (unsigned long long)tot_k);
        if (tot_e) atomicAdd(&scalars[2], (unsigned long long)tot_e);
    }
}

// occupied slots -> node arrays (table order); the slot's stamp field is re-used for the node id
__global__ __launch_bounds__(256) void k_gather(Slot *tab, const uint32_t *occ, const uint32_t *word_rank,
                                                uint64_t n_words, uint64_t *keys, uint64_t *stamps, uint32_t *cnt,
                                                uint8_t *flags) {
    uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint32_t bits = occ[w];
    uint32_t node = word_rank[w];
    while (bits) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        Slot *s = tab + (w * 32 + b);
        const uint4 lo = reinterpret_cast<const uint4 *>(s)[0];
        const uint4 hi = reinterpret_cast<const uint4 *>(s)[1];
        keys[node] = ((uint64_t)lo.y << 32) | lo.x;
        const uint64_t st = ((uint64_t)lo.w << 32) | lo.z;
        stamps[node] = st;
        reinterpret_cast<uint4 *>(cnt)[node] = hi;
        flags[node] = (uint8_t)(st & 1);
        s->stamp = node;
        ++node;
    }
}

__device__ inline uint32_t tab_find(const Slot *tab, uint64_t cap_mask, int hash_shift, uint64_t key) {
    uint64_t slot = kmer_hash(key) >> hash_shift;
    for (uint64_t probe = 0; probe <= cap_mask; ++probe) {
        const uint64_t cur = tab[slot].key;
        if (cur == key) return (uint32_t)tab[slot].stamp;
        if (cur == EMPTY_KEY) return NO_NODE;
        slot = (slot + 1) & cap_mask;
    }
    return NO_NODE;
}

// successor ids (4-way) + successor rank order byte
__global__ __launch_bounds__(256) void k_succ(const Slot *tab, uint64_t cap_mask, int hash_shift, int k, uint64_t n_nodes,
                                              const uint64_t *keys, const uint32_t *cnt, uint32_t *succ,
                                              uint8_t *order, uint8_t *deg) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const uint64_t kmask = (k == 32) ? ~0ull : ((1ull << (2 * k)) - 1);
    const uint64_t key = keys[i];
    const uint4 c4 = reinterpret_cast<const uint4 *>(cnt)[i];
    const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
    uint32_t s[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
        s[b] = c[b] ? tab_find(tab, cap_mask, hash_shift, ((key << 2) | (uint64_t)b) & kmask) : NO_NODE;
    reinterpret_cast<uint4 *>(succ)[i] = make_uint4(s[0], s[1], s[2], s[3]);
    deg[i] = (uint8_t)((c[0] != 0) + (c[1] != 0) + (c[2] != 0) + (c[3] != 0));
    // rank codes by (count desc, ascii order asc): insertion sort of 4
    uint32_t code[4] = {0, 1, 3, 2};  // ascii order A, C, G, T as codes
#pragma unroll
    for (int a = 1; a < 4; ++a) {
#pragma unroll
        for (int b = a; b > 0; --b) {
            if (c[code[b]] > c[code[b - 1]]) {
                uint32_t tmp = code[b]; code[b] = code[b - 1]; code[b - 1] = tmp;
            }
        }
    }
    order[i] = (uint8_t)(code[0] | (code[1] << 2) | (code[2] << 4) | (code[3] << 6));
}

__global__ __launch_bounds__(256) void k_csr_fill(uint64_t n_nodes, const uint64_t *rowptr, const uint32_t *cnt,
                                                  const uint32_t *succ, uint32_t *col, uint32_t *ecnt) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const uint4 c4 = reinterpret_cast<const uint4 *>(cnt)[i];
    const uint4 s4 = reinterpret_cast<const uint4 *>(succ)[i];
    const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w}, s[4] = {s4.x, s4.y, s4.z, s4.w};
    uint64_t o = rowptr[i];
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (c[b]) { col[o] = s[b]; ecnt[o] = c[b]; ++o; }
}
