// msm_sort.hip -- the digit sort of an MSM call (msm.hip): signed-digit extraction, counting sort of the (scalar, window) entries by bucket (partitioned; one-pass
// under the option "msm_sort_onepass"), descending-population order of the buckets.  One host entry point: msm_sort_enqueue (czk_internal.h).
#include "czk_internal.h"

namespace czk {

// ------------------------------------------------------------------------------------------------
// digit extraction + counting sort
// ------------------------------------------------------------------------------------------------
// Signed digit of window w of the canonical scalar s: 0 (skip) or |d| | sign<<31, d in (-2^(cw-1), 2^(cw-1)] (a window value of exactly 2^(cw-1) stays positive); `carry` runs from window to window.
__device__ __forceinline__ u32 msm_recode_digit(const Fr& s, unsigned c, unsigned W_hi, unsigned w, u32& carry, uint8_t base_is_inf) {
    const unsigned bit = msm_win_bit(c, W_hi, w), cw = msm_win_width(c, W_hi, w);
    const u32 half = 1u << (cw - 1);
    u32 v = 0;
    if (bit < 256) {
        unsigned limb = bit >> 5, off = bit & 31;
        u64 two = (u64)s.l[limb] | ((limb + 1 < 8) ? ((u64)s.l[limb + 1] << 32) : 0);
        v = (u32)(two >> off) & ((1u << cw) - 1u);
    }
    v += carry;
    u32 code;
    if (v > half) {
        code = ((1u << cw) - v) | 0x80000000u;
        carry = 1;
    } else {
        code = v;
        carry = 0;
    }
    if (base_is_inf) code = 0;   // add_assign_mixed skips infinity (short_weierstrass_jacobian.rs:571-573)
    if ((code & 0x7fffffffu) == 0) code = 0;
    return code;
}

// digits[(lane*W + w)*size + i] = the digit of window w of scalar i
__global__ void k_digits(const u64* scalars, size_t n_scalars, size_t size, int montgomery, unsigned c, unsigned W,
                         const uint8_t* inf, size_t n_bases, u32* digits, u32* ranks, u32* counts, size_t B) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= size) return;
    const unsigned lane = blockIdx.y;
    Fr s = fp_load<FrParams>(scalars + 4 * ((size_t)lane * n_scalars + i));
    if (montgomery) s = fp_into_repr(s);   // ec/src/lib.rs:305-307
    u32 carry = 0;
    const unsigned W_hi = msm_full_windows(c);
    for (unsigned w = 0; w < W; w++) {
        const u32 code = msm_recode_digit(s, c, W_hi, w, carry, inf[(size_t)w * n_bases + i]);
        digits[((size_t)lane * W + w) * size + i] = code;
        // the histogram atomic also hands out the entry's rank inside its bucket, so the scatter needs no second atomic
        if (code) ranks[((size_t)lane * W + w) * size + i] = atomicAdd(&counts[(size_t)lane * B + (code & 0x7fffffffu) - 1], 1u);
    }
}

// exclusive scan of counts[lane][0..B) -> offsets.  Three phases:
// per-tile sums (tile = 2048 entries), scan of the tile sums (one block per lane), per-tile exclusive scan.
__global__ __launch_bounds__(256) void k_scan_tile_sums(const u32* counts, size_t B, u32* tile_sums, size_t n_tiles) {
    __shared__ u32 red[256];
    const size_t tile = blockIdx.x;
    const u32* cnt = counts + (size_t)blockIdx.y * B + tile * SCAN_TILE;
    size_t lim = B - tile * SCAN_TILE < SCAN_TILE ? B - tile * SCAN_TILE : SCAN_TILE;
    u32 s = 0;
    for (unsigned i = threadIdx.x; i < lim; i += 256) s += cnt[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (unsigned d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_sums[(size_t)blockIdx.y * n_tiles + tile] = red[0];
}
__global__ __launch_bounds__(1024) void k_scan_tiles(u32* tile_sums, size_t n_tiles) {
    __shared__ u32 part[1024];
    u32* ts = tile_sums + (size_t)blockIdx.x * n_tiles;
    const unsigned tid = threadIdx.x;
    size_t per = (n_tiles + 1023) / 1024;
    size_t start = tid * per, end = start + per < n_tiles ? start + per : n_tiles;
    u32 sum = 0;
    for (size_t i = start; i < end; i++) sum += ts[i];
    part[tid] = sum;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        u32 v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u32 run = tid ? part[tid - 1] : 0;
    for (size_t i = start; i < end; i++) {
        u32 v = ts[i];
        ts[i] = run;
        run += v;
    }
}
__global__ __launch_bounds__(256) void k_scan_apply(u32* counts, u32* offsets, size_t B, const u32* tile_sums, size_t n_tiles) {
    __shared__ u32 part[256];
    const size_t tile = blockIdx.x;
    u32* cnt = counts + (size_t)blockIdx.y * B + tile * SCAN_TILE;
    u32* off = offsets + (size_t)blockIdx.y * B + tile * SCAN_TILE;
    size_t lim = B - tile * SCAN_TILE < SCAN_TILE ? B - tile * SCAN_TILE : SCAN_TILE;
    const unsigned tid = threadIdx.x;
    constexpr unsigned PER = SCAN_TILE / 256;
    u32 v[PER];
    u32 s = 0;
#pragma unroll
    for (unsigned k = 0; k < PER; k++) {
        unsigned i = tid * PER + k;
        v[k] = i < lim ? cnt[i] : 0;
        s += v[k];
    }
    part[tid] = s;
    __syncthreads();
    for (unsigned d = 1; d < 256; d <<= 1) {
        u32 x = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    u32 run = tile_sums[(size_t)blockIdx.y * n_tiles + tile] + (tid ? part[tid - 1] : 0);
#pragma unroll
    for (unsigned k = 0; k < PER; k++) {
        unsigned i = tid * PER + k;
        if (i < lim) off[i] = run;
        run += v[k];
    }
}

// sorted[lane][offsets[b] + k] = (w * n_bases + i) | sign<<31
__global__ void k_scatter(const u32* digits, const u32* ranks, size_t size, unsigned W, size_t n_bases, const u32* offsets, size_t B,
                          u32* sorted) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)W * size) return;
    const unsigned lane = blockIdx.y;
    u32 code = digits[(size_t)lane * W * size + e];
    if (!code) return;
    size_t w = e / size, i = e - w * size;
    size_t b = (code & 0x7fffffffu) - 1;
    u32 pos = offsets[(size_t)lane * B + b] + ranks[(size_t)lane * W * size + e];
    sorted[(size_t)lane * W * size + pos] = (u32)(w * n_bases + i) | (code & 0x80000000u);
}

// ------------------------------------------------------------------------------------------------
// partitioned counting sort (default).  The one-pass sort above costs one global atomic and one random 4-byte store per
// entry -- 54 M of each per 4-lane 2^20-point MSM -- and those are what slows the accumulate kernels of the neighbouring
// MSMs in the pipeline (measured: every ms of k_scatter overlap inflates an accumulate kernel by ~0.6 ms).  Here the
// buckets are grouped into partitions of 1024 (by the LOW bits of the bucket index, so the few thousand over-full buckets of
// the 13-bit top window spread over all partitions; `sorted` is partition-major, which the accumulate kernel does not care about): (1) digits + per-block LDS histogram of partitions (global atomics: one per
// block and partition); (2) scan of the partition sizes; (3) entries move into their partition's region -- per block, the
// entries of one partition land in one contiguous run; (4) one workgroup per partition counts, scans and places its
// entries with LDS atomics and writes the partition's slice of `sorted`, `offsets` and `counts`.
// ------------------------------------------------------------------------------------------------
// split != 0 (bases without window tables): every window is its own bucket set, i.e. window w of lane l is virtual lane l W + w of
// everything downstream (the `digits` layout is the same either way); partition counts are then kept per window.
__global__ __launch_bounds__(256) void k_digits_part(const u64* scalars, size_t n_scalars, size_t size, int montgomery, unsigned c, unsigned W,
                                                     const uint8_t* inf, size_t n_bases, u32* digits, u32* part_counts, unsigned n_parts, int split) {
    __shared__ u32 h[MAX_PARTS];
    const unsigned n_hist = split ? W * n_parts : n_parts;
    for (unsigned t = threadIdx.x; t < n_hist; t += 256) h[t] = 0;
    __syncthreads();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned lane = blockIdx.y;
    if (i < size) {
        Fr s = fp_load<FrParams>(scalars + 4 * ((size_t)lane * n_scalars + i));
        if (montgomery) s = fp_into_repr(s);   // ec/src/lib.rs:305-307
        u32 carry = 0;
        const unsigned W_hi = msm_full_windows(c);
        for (unsigned w = 0; w < W; w++) {
            const u32 code = msm_recode_digit(s, c, W_hi, w, carry, inf[(split ? 0 : (size_t)w * n_bases) + i]);
            digits[((size_t)lane * W + w) * size + i] = code;
            if (code) atomicAdd(&h[(split ? w * n_parts : 0) + (((code & 0x7fffffffu) - 1) & (n_parts - 1))], 1u);
        }
    }
    __syncthreads();
    for (unsigned t = threadIdx.x; t < n_hist; t += 256)
        if (h[t]) atomicAdd(&part_counts[(size_t)lane * n_hist + t], h[t]);   // split: (lane W + w) n_parts + part
}
// part_base[lane][0 .. n_parts] = exclusive scan of part_counts; cursors cleared.  One block per lane.
__global__ __launch_bounds__(1024) void k_part_scan(const u32* part_counts, u32* part_base, u32* part_cursor, unsigned n_parts) {
    __shared__ u32 part[1024];
    const unsigned lane = blockIdx.x, tid = threadIdx.x;
    const u32* cnt = part_counts + (size_t)lane * n_parts;
    u32* base = part_base + (size_t)lane * (n_parts + 1);
    const unsigned per = (n_parts + 1023) / 1024;
    unsigned start = tid * per, end = start + per < n_parts ? start + per : n_parts;
    u32 sum = 0;
    for (unsigned i = start; i < end; i++) sum += cnt[i];
    part[tid] = sum;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        u32 v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u32 run = tid ? part[tid - 1] : 0;
    for (unsigned i = start; i < end; i++) {
        base[i] = run;
        part_cursor[(size_t)lane * n_parts + i] = 0;
        run += cnt[i];
    }
    if (tid == 1023) base[n_parts] = part[1023];
}
// entries -> partition regions: part_idx[dst] = point code, part_lb[dst] = bucket index inside the partition
// NT threads x PS_TILE entries per tile.  A tile leaves as one run per partition, so a run is tile / n_parts entries long: 256 threads (8-entry
// runs at 512 partitions) for the common case, 1024 threads for calls with 2048 partitions (3 * 2^20-point commitments, 2^22-point queries), whose
// runs would otherwise be 2 entries: partial sectors again (same-box: Marlin 5.67 -> 6.01 proofs/s, Groth16 at 2^22 3.12 -> 3.28; at 1024 partitions --
// the 2^21-point h query, Plonk's 3 * 2^19-point commitments -- and at 512 (2^20 points) 512 threads: the isolated sort of 2^21 x 4 lanes 2.74 -> 1.73 ms,
// of 2^20 x 4 lanes 1.03 -> 0.87 ms, per proof within noise).
template <unsigned NT>
__global__ __launch_bounds__(NT) void k_part_scatter(const u32* digits, size_t size, unsigned W, size_t n_bases, const u32* part_base, u32* part_cursor,
                                                     unsigned n_parts, unsigned part_shift, u32* part_idx, uint16_t* part_lb) {
    // The tile is ordered by partition in LDS first and leaves as runs: consecutive lanes then write consecutive addresses of a partition's region
    // (a store instruction touches ~8 sectors instead of 64 partial ones).
    extern __shared__ u32 pscat_lds[];
    u32 *h = pscat_lds, *base = h + n_parts, *lofs = base + n_parts, *red = lofs + n_parts, *st_idx = red + NT;
    uint16_t *st_lb = (uint16_t*)(st_idx + NT * PS_TILE), *st_pt = st_lb + NT * PS_TILE;
    for (unsigned t = threadIdx.x; t < n_parts; t += NT) h[t] = 0;
    __syncthreads();
    const unsigned lane = blockIdx.y, tid = threadIdx.x;
    const size_t total = (size_t)W * size, tile0 = (size_t)blockIdx.x * NT * PS_TILE;
    u32 code[PS_TILE], rank[PS_TILE];
#pragma unroll
    for (unsigned k = 0; k < PS_TILE; k++) {
        size_t e = tile0 + (size_t)k * NT + tid;
        code[k] = e < total ? digits[(size_t)lane * total + e] : 0u;
        if (code[k]) rank[k] = atomicAdd(&h[((code[k] & 0x7fffffffu) - 1) & (n_parts - 1)], 1u);
    }
    __syncthreads();
    // exclusive scan of h over the partitions (n_parts <= 2048: up to 8 per thread) -> lofs; global bases
    const unsigned per = (n_parts + NT - 1) / NT;
    u32 sum = 0;
    for (unsigned i = tid * per; i < tid * per + per && i < n_parts; i++) sum += h[i];
    red[tid] = sum;
    __syncthreads();
    for (unsigned d = 1; d < NT; d <<= 1) {
        u32 x = tid >= d ? red[tid - d] : 0;
        __syncthreads();
        red[tid] += x;
        __syncthreads();
    }
    u32 run = tid ? red[tid - 1] : 0;
    for (unsigned i = tid * per; i < tid * per + per && i < n_parts; i++) {
        lofs[i] = run;
        run += h[i];
        if (h[i]) base[i] = part_base[(size_t)lane * (n_parts + 1) + i] + atomicAdd(&part_cursor[(size_t)lane * n_parts + i], h[i]);
    }
    const u32 n_tile = red[NT - 1];
    __syncthreads();
#pragma unroll
    for (unsigned k = 0; k < PS_TILE; k++) {
        if (!code[k]) continue;
        size_t e = tile0 + (size_t)k * NT + tid;
        size_t w = e / size, i = e - w * size;
        u32 b = (code[k] & 0x7fffffffu) - 1;
        const u32 pt = b & (n_parts - 1), slot = lofs[pt] + rank[k];
        st_idx[slot] = (u32)(w * n_bases + i) | (code[k] & 0x80000000u);
        st_lb[slot] = (uint16_t)(b >> part_shift);
        st_pt[slot] = (uint16_t)pt;
    }
    __syncthreads();
    for (u32 sl = tid; sl < n_tile; sl += NT) {
        const u32 pt = st_pt[sl];
        const size_t dst = (size_t)lane * total + base[pt] + (sl - lofs[pt]);
        part_idx[dst] = st_idx[sl];
        part_lb[dst] = st_lb[sl];
    }
}
// one workgroup per (partition, lane): bucket counts, offsets and the final placement of the partition's entries.  The placement is staged
// in LDS when the partition fits (`cap` entries of dynamic LDS behind the counters): 4-byte stores to random positions of the partition's
// output cost a sector write each, the staged copy leaves as coalesced 4 KiB rows.  Larger partitions (the 2^21-point `h` query: 53 k
// entries) place directly, as rounds 1 - 3 did for every partition.
__global__ __launch_bounds__(PSORT_THREADS) void k_part_sort(const u32* part_idx, const uint16_t* part_lb, const u32* part_base, unsigned n_parts, unsigned part_shift,
                                                             size_t total, size_t B, u32* sorted, u32* offsets, u32* counts, u32 cap) {
    extern __shared__ u32 psort_lds[];
    u32 *cnt = psort_lds, *cur = psort_lds + PART_BUCKETS, *red = psort_lds + 2 * PART_BUCKETS, *stage = psort_lds + 2 * PART_BUCKETS + PSORT_THREADS;
    const unsigned p = blockIdx.x, lane = blockIdx.y, tid = threadIdx.x;
    const u32 r0 = part_base[(size_t)lane * (n_parts + 1) + p], r1 = part_base[(size_t)lane * (n_parts + 1) + p + 1];
    for (unsigned t = tid; t < PART_BUCKETS; t += PSORT_THREADS) cnt[t] = 0;
    __syncthreads();
    const uint16_t* lb = part_lb + (size_t)lane * total;
    const u32* idx = part_idx + (size_t)lane * total;
    // four entries per thread and iteration, loads issued together
    for (u32 j = r0 + tid; j < r1; j += 4 * PSORT_THREADS) {
        const bool h1 = j + PSORT_THREADS < r1, h2 = j + 2 * PSORT_THREADS < r1, h3 = j + 3 * PSORT_THREADS < r1;
        const uint16_t l0 = lb[j], l1 = h1 ? lb[j + PSORT_THREADS] : (uint16_t)0, l2 = h2 ? lb[j + 2 * PSORT_THREADS] : (uint16_t)0,
                       l3 = h3 ? lb[j + 3 * PSORT_THREADS] : (uint16_t)0;
        atomicAdd(&cnt[l0], 1u);
        if (h1) atomicAdd(&cnt[l1], 1u);
        if (h2) atomicAdd(&cnt[l2], 1u);
        if (h3) atomicAdd(&cnt[l3], 1u);
    }
    __syncthreads();
    // exclusive scan of cnt[0..1024): one entry per thread
    const u32 v = tid < PART_BUCKETS ? cnt[tid] : 0u;
    red[tid] = v;
    __syncthreads();
    for (unsigned d = 1; d < PSORT_THREADS; d <<= 1) {
        u32 x = tid >= d ? red[tid - d] : 0;
        __syncthreads();
        red[tid] += x;
        __syncthreads();
    }
    if (tid < PART_BUCKETS) {
        const u32 run = red[tid] - v;                      // exclusive prefix, relative to the partition
        size_t b = ((size_t)tid << part_shift) | p;          // bucket = (index inside the partition, partition)
        cur[tid] = run;
        if (b < B) {
            offsets[(size_t)lane * B + b] = r0 + run;
            counts[(size_t)lane * B + b] = v;
        }
    }
    __syncthreads();
    u32* out = sorted + (size_t)lane * total;
    const bool staged = r1 - r0 <= cap;
    for (u32 j = r0 + tid; j < r1; j += 4 * PSORT_THREADS) {
        const bool h1 = j + PSORT_THREADS < r1, h2 = j + 2 * PSORT_THREADS < r1, h3 = j + 3 * PSORT_THREADS < r1;
        const uint16_t l0 = lb[j], l1 = h1 ? lb[j + PSORT_THREADS] : (uint16_t)0, l2 = h2 ? lb[j + 2 * PSORT_THREADS] : (uint16_t)0,
                       l3 = h3 ? lb[j + 3 * PSORT_THREADS] : (uint16_t)0;
        const u32 v0 = idx[j], v1 = h1 ? idx[j + PSORT_THREADS] : 0u, v2 = h2 ? idx[j + 2 * PSORT_THREADS] : 0u, v3 = h3 ? idx[j + 3 * PSORT_THREADS] : 0u;
        if (staged) {
            stage[atomicAdd(&cur[l0], 1u)] = v0;
            if (h1) stage[atomicAdd(&cur[l1], 1u)] = v1;
            if (h2) stage[atomicAdd(&cur[l2], 1u)] = v2;
            if (h3) stage[atomicAdd(&cur[l3], 1u)] = v3;
        } else {
            out[r0 + atomicAdd(&cur[l0], 1u)] = v0;
            if (h1) out[r0 + atomicAdd(&cur[l1], 1u)] = v1;
            if (h2) out[r0 + atomicAdd(&cur[l2], 1u)] = v2;
            if (h3) out[r0 + atomicAdd(&cur[l3], 1u)] = v3;
        }
    }
    if (staged) {
        __syncthreads();
        for (u32 k = tid; k < r1 - r0; k += PSORT_THREADS) out[r0 + k] = stage[k];
    }
}

// ------------------------------------------------------------------------------------------------
// load balancing: order the buckets by population (descending) so the 64 lanes of a wave fold the same number
// of points (bucket sizes are ~Poisson: without this a wave waits for its fullest bucket, ~30% of the time)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_count_hist(const u32* counts, size_t B, u32* hist) {
    __shared__ u32 h[CNT_BINS];   // block-private histogram: populations cluster on a few values
    for (unsigned i = threadIdx.x; i < CNT_BINS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        u32 c = counts[(size_t)blockIdx.y * B + b];
        atomicAdd(&h[c < CNT_BINS ? c : CNT_BINS - 1], 1u);
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < CNT_BINS; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[(size_t)blockIdx.y * CNT_BINS + i], h[i]);
}
// start[v] = number of buckets with a larger population; one block of CNT_BINS/2 threads per lane
__global__ __launch_bounds__(1024) void k_count_starts(u32* hist) {
    __shared__ u32 part[CNT_BINS];
    u32* h = hist + (size_t)blockIdx.x * CNT_BINS;
    const unsigned tid = threadIdx.x;
    for (unsigned i = tid; i < CNT_BINS; i += blockDim.x) part[i] = h[CNT_BINS - 1 - i];   // reversed: descending order
    __syncthreads();
    if (tid == 0) {
        u32 run = 0;
        for (unsigned i = 0; i < CNT_BINS; i++) {
            u32 c = part[i];
            part[i] = run;
            run += c;
        }
    }
    __syncthreads();
    for (unsigned i = tid; i < CNT_BINS; i += blockDim.x) h[CNT_BINS - 1 - i] = part[i];
}
__global__ __launch_bounds__(1024) void k_count_scatter(const u32* counts, size_t B, u32* starts, u32* perm) {
    __shared__ u32 h[CNT_BINS], base[CNT_BINS];
    for (unsigned i = threadIdx.x; i < CNT_BINS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32 bin = 0, rank = 0;
    if (b < B) {
        u32 c = counts[(size_t)blockIdx.y * B + b];
        bin = c < CNT_BINS ? c : CNT_BINS - 1;
        rank = atomicAdd(&h[bin], 1u);
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < CNT_BINS; i += blockDim.x)
        if (h[i]) base[i] = atomicAdd(&starts[(size_t)blockIdx.y * CNT_BINS + i], h[i]);
    __syncthreads();
    if (b < B) perm[(size_t)blockIdx.y * B + base[bin] + rank] = (u32)b;
}

// ---- host entry point ----
template <unsigned NT>
static void launch_part_scatter(hipStream_t st, const MsmSortDims& d, const MsmSortBufs& s) {
    hipLaunchKernelGGL(k_part_scatter<NT>, dim3((unsigned)((d.total + NT * PS_TILE - 1) / (NT * PS_TILE)), (unsigned)d.lanes), dim3(NT), part_scatter_lds(NT, d.n_parts), st,
                       s.digits, d.size, d.W, d.nb, s.part_base, s.part_cursor, d.n_parts, d.part_shift, s.ranks, s.part_lb);
}

hipError_t msm_sort_enqueue(hipStream_t st, const MsmSortDims& d, const MsmSortBufs& s) {
    const unsigned lanes = (unsigned)d.lanes;
    const size_t total = d.total, B = d.B;
    hipError_t e;
    if (d.one_pass) {
        if ((e = hipMemsetAsync(s.counts, 0, d.lanes * B * 4, st)) != hipSuccess) return e;
        if (d.size)
            hipLaunchKernelGGL(k_digits, dim3((unsigned)((d.size + 255) / 256), lanes), dim3(256), 0, st, d.scalars, d.n_scalars, d.size, d.form == CZK_SCALAR_MONTGOMERY ? 1 : 0, d.c, d.W,
                               d.tv.inf, d.nb, s.digits, s.ranks, s.counts, B);
        hipLaunchKernelGGL(k_scan_tile_sums, dim3((unsigned)d.n_tiles, lanes), dim3(256), 0, st, s.counts, B, s.tile_sums, d.n_tiles);
        hipLaunchKernelGGL(k_scan_tiles, dim3(lanes), dim3(1024), 0, st, s.tile_sums, d.n_tiles);
        hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)d.n_tiles, lanes), dim3(256), 0, st, s.counts, s.offsets, B, s.tile_sums, d.n_tiles);
        if (d.size)
            hipLaunchKernelGGL(k_scatter, dim3((unsigned)((total + 255) / 256), lanes), dim3(256), 0, st, s.digits, s.ranks, d.size, d.W, d.nb, s.offsets, B, s.sorted);
    } else {
        const unsigned n_parts = d.n_parts;
        if ((e = hipMemsetAsync(s.part_counts, 0, d.lanes * n_parts * 4, st)) != hipSuccess) return e;
        if (d.size)
            hipLaunchKernelGGL(k_digits_part, dim3((unsigned)((d.size + 255) / 256), (unsigned)d.real_lanes), dim3(256), 0, st, d.scalars, d.n_scalars, d.size,
                               d.form == CZK_SCALAR_MONTGOMERY ? 1 : 0, d.c, d.Wd, d.tv.inf, d.nb, s.digits, s.part_counts, n_parts, d.split ? 1 : 0);
        hipLaunchKernelGGL(k_part_scan, dim3(lanes), dim3(1024), 0, st, s.part_counts, s.part_base, s.part_cursor, n_parts);
        if (d.size) {   // (thread counts: see k_part_scatter)
            if (n_parts >= 2048 && part_scatter_lds(1024, n_parts) <= d.lds_per_block) launch_part_scatter<1024>(st, d, s);
            else if ((n_parts == 1024 || n_parts == 512) && part_scatter_lds(512, n_parts) <= d.lds_per_block) launch_part_scatter<512>(st, d, s);
            else launch_part_scatter<256>(st, d, s);
        }
        const size_t lds = part_sort_lds(d);   // (czk_internal.h: the staging area's size)
        const u32 cap = part_sort_cap(d);
        hipLaunchKernelGGL(k_part_sort, dim3(n_parts, lanes), dim3(PSORT_THREADS), lds, st, s.ranks, s.part_lb, s.part_base, n_parts, d.part_shift, total, B, s.sorted,
                           s.offsets, s.counts, cap);
    }
    if ((e = hipMemsetAsync(s.chist, 0, d.lanes * CNT_BINS * 4, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_count_hist, dim3((unsigned)((B + 1023) / 1024), lanes), dim3(1024), 0, st, s.counts, B, s.chist);
    hipLaunchKernelGGL(k_count_starts, dim3(lanes), dim3(1024), 0, st, s.chist);
    hipLaunchKernelGGL(k_count_scatter, dim3((unsigned)((B + 1023) / 1024), lanes), dim3(1024), 0, st, s.counts, B, s.chist, s.perm);
    return hipSuccess;
}

}  // namespace czk
