// Generic exclusive scan and reduction over a functor (exclusive_scan, reduce_sum, the functors the sections share), the synthetic
// reads with their checksum, and the read-start bitmap.
// A section of the one translation unit dbg_hip.hip, not self-contained: it needs dbg_hip_handle.h (dbg, the arena's
// ar_scan, CHK / HIPCHK, grid_for) and dbg_device.h in front of it.

// ------------------------------------------------------------------------------------------
// generic exclusive scan: out[i] = sum_{j<i} f(j); 256 threads x 16 items per block
// ------------------------------------------------------------------------------------------
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = 256 * SCAN_ITEMS;

template <class F>
__global__ __launch_bounds__(256) void k_scan_reduce(uint64_t n, F f, uint64_t *partial) {
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) s += f(base + i);
    uint64_t tot;
    (void)block_exscan_256(s, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// single block: partial[] -> exclusive prefix in place, grand total to *total
__global__ __launch_bounds__(256) void k_scan_partials(uint64_t *partial, uint64_t nblk, uint64_t *total) {
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nblk; base += 256) {
        uint64_t i = base + threadIdx.x;
        uint64_t v = i < nblk ? partial[i] : 0;
        uint64_t tot;
        uint64_t ex = block_exscan_256(v, &tot);
        if (i < nblk) partial[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class F, class OutT>
__global__ __launch_bounds__(256) void k_scan_write(uint64_t n, F f, const uint64_t *partial, OutT *out) {
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint64_t v[SCAN_ITEMS];
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = (base + i < n) ? f(base + i) : 0;
        s += v[i];
    }
    uint64_t tot;
    uint64_t run = partial[blockIdx.x] + block_exscan_256(s, &tot);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        if (base + i < n) out[base + i] = (OutT)run;
        run += v[i];
    }
}

// out must hold n entries; *d_total (device) receives the total; returns total on host too
template <class F, class OutT>
static int exclusive_scan(dbg *h, uint64_t n, F f, OutT *out, uint64_t *h_total) {
    uint64_t nblk = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (nblk == 0) nblk = 1;
    CHK(buf_ensure(h, h->ar_scan, (nblk + 1) * 8));
    uint64_t *partial = (uint64_t *)h->ar_scan.p;
    uint64_t *d_total = partial + nblk;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_reduce<F>), dim3((unsigned)nblk), dim3(256), 0, h->stream, n, f, partial);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, h->stream, partial, nblk, d_total);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_write<F, OutT>), dim3((unsigned)nblk), dim3(256), 0, h->stream, n, f,
                       partial, out);
    if (!h_total) return DBG_OK;  // the caller does not need the total on the host: no synchronisation
    hipError_t e = hipMemcpyAsync(h_total, d_total, 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->err = std::string("exclusive_scan: ") + hipGetErrorString(e);
        return DBG_E_HIP;
    }
    return DBG_OK;
}

template <class F>
static int reduce_sum(dbg *h, uint64_t n, F f, uint64_t *h_total) {
    uint64_t nblk = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (nblk == 0) nblk = 1;
    CHK(buf_ensure(h, h->ar_scan, (nblk + 1) * 8));
    uint64_t *partial = (uint64_t *)h->ar_scan.p;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scan_reduce<F>), dim3((unsigned)nblk), dim3(256), 0, h->stream, n, f, partial);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, h->stream, partial, nblk, partial + nblk);
    hipError_t e = hipMemcpyAsync(h_total, partial + nblk, 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->err = std::string("reduce_sum: ") + hipGetErrorString(e);
        return DBG_E_HIP;
    }
    return DBG_OK;
}

struct OccBytes32 {  // occupied slots among 32 one-byte flags (each 0 or 1)
    const uint8_t *occ;
    __device__ uint64_t operator()(uint64_t w) const {
        const uint4 a = reinterpret_cast<const uint4 *>(occ)[2 * w], b = reinterpret_cast<const uint4 *>(occ)[2 * w + 1];
        return __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
    }
};
struct PopcWords {
    const uint32_t *w;
    __device__ uint64_t operator()(uint64_t i) const { return __popc(w[i]); }
};
struct DegOf {
    const uint8_t *deg;
    __device__ uint64_t operator()(uint64_t i) const { return deg[i]; }
};
struct U64At {
    const uint64_t *p;
    __device__ uint64_t operator()(uint64_t i) const { return p[i]; }
};
struct KmerInstances {  // k-mer instances of read i
    const uint64_t *off;
    uint64_t k;
    __device__ uint64_t operator()(uint64_t i) const { const uint64_t len = off[i + 1] - off[i]; return len >= k ? len - k + 1 : 0; }
};
struct WRecLenAt {   // k-mers of wide record i
    const uint64_t *w1;
    __device__ uint64_t operator()(uint64_t i) const { return (uint64_t)wrec_len(w1[i]); }
};
struct WRecSuccAt {  // 1 if the last k-mer of wide record i has a successor
    const uint64_t *w1;
    __device__ uint64_t operator()(uint64_t i) const { return (uint64_t)wrec_has_succ(w1[i]); }
};
struct FlagSet {
    const uint8_t *f;
    uint8_t mask, want;
    __device__ uint64_t operator()(uint64_t i) const { return (f[i] & mask) == want; }
};

// ------------------------------------------------------------------------------------------
// synthetic reads (device twin of py-debruijn_amd/synth.py) + checksum
// ------------------------------------------------------------------------------------------
__device__ inline uint64_t synth_draw(uint64_t key, uint64_t ctr) { return mix64(key ^ (ctr * 0xD6E8FEB86659FD93ull)); }

__global__ __launch_bounds__(256) void k_synth(char *bases, uint64_t *offsets, uint64_t kg, uint64_t ks, uint64_t ke,
                                               uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                                               uint32_t read_len, uint32_t err_thr) {
    const uint64_t total = n_reads * read_len;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / read_len, j = i - r * read_len, gr = first_read + r;
        const uint64_t start = synth_draw(ks, gr) % (genome_len - read_len + 1);
        uint32_t code = (uint32_t)(synth_draw(kg, start + j) & 3);
        if (err_thr) {
            const uint64_t e = synth_draw(ke, gr * read_len + j);
            if ((uint32_t)(e & 0xFFFFFFu) < err_thr) code = (code + 1 + (uint32_t)((e >> 24) % 3)) & 3;
        }
        bases[i] = "ACGT"[code];
        if (j == 0) offsets[r] = i;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_reads] = total;
}

__global__ __launch_bounds__(256) void k_checksum(const char *bases, uint64_t n, unsigned long long *out) {
    uint64_t s = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        s += mix64((uint64_t)(uint8_t)bases[i] + 256ull * i);
    s = wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)s);
}

// ------------------------------------------------------------------------------------------
// read-start bitmap
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_startbits(const uint64_t *offsets, uint64_t n_reads, uint32_t *bits) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_reads) {
        uint64_t p = offsets[i];
        atomicOr(&bits[p >> 5], 1u << (p & 31));
    }
}
