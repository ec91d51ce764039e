// plonk_layout.hip -- the index side of mpc-plonk's CircuitLayout::from_circuit (mpc-plonk/src/relations/flat.rs:35-137) on the GPU, up to the two
// evaluation vectors, and the gather that lays an assignment out over the wire slots.
//
// czk_plonk_layout: with W = 3 n_gates wire slots (in0, in1, out per gate) and w = get_root_of_unity(W) of the mixed-radix domain,
//     w_evals[i] = w^succ[i]  (i < W)        succ = the wiring permutation as slot indices (:75-80: each slot of a variable names the variable's next slot)
//     s_evals[j] = 0 (j < n_prods), 1 (n_prods <= j < n_gates)                                  (:40-46: products first, then sums)
// One thread per wire slot.  Domain elements come from the per-byte power tables of pow_tables.h, built per call; nothing of size W crosses from the host
// except succ.
//
// czk_fr_gather: out[l][i] = src[l][index[i]], the step p_evals[i] = vals[var] of :91-100 over share lanes (the index array is public, the values are
// shares).  One thread per output element and lane; an element moves as two 16-byte vector accesses.
#include "call.h"
#include "pow_tables.h"

namespace czk {

// Reads nothing outside succ[0..W) and the tables whatever succ holds: an entry >= W is not used as an exponent, its slot gets 0 (no domain element).
__global__ __launch_bounds__(256) void k_plonk_layout(const u32* succ, u32 W, u32 n_gates, u32 n_prods, unsigned nb, const u64* tab, u64* w_evals,
                                                       u64* s_evals) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W) return;
    const u32 e = succ[i];
    fp_store<FrParams>(w_evals + 4 * i, e < W ? marlin_domain_element(tab, e, nb) : Fr::zero());
    if (i < n_gates) fp_store<FrParams>(s_evals + 4 * i, i < n_prods ? Fr::zero() : Fr::one());
}

// Reads nothing outside index[0..n) and src[l][0..src_len): an index >= src_len writes 0.
__global__ __launch_bounds__(256) void k_fr_gather(const u64* src, size_t src_len, size_t src_stride, const u32* index, size_t n, u64* out,
                                                    size_t out_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
    if (i >= n) return;
    const u32 j = index[i];
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (j < src_len) {
        const uint4* p = reinterpret_cast<const uint4*>(src + 4 * (l * src_stride + j));
        lo = p[0];
        hi = p[1];
    }
    uint4* q = reinterpret_cast<uint4*>(out + 4 * (l * out_stride + i));
    q[0] = lo;
    q[1] = hi;
}

}  // namespace czk

using namespace czk;

extern "C" int czk_plonk_layout(czk_ctx* ctx, const uint32_t* succ, size_t n_gates, size_t n_prods, uint64_t* w_evals, uint64_t* s_evals, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (!n_gates || (n_gates & (n_gates - 1))) return set_err(ctx, CZK_ERR_SIZE, "plonk_layout: the number of gates must be a power of two");
    if (n_gates > (((size_t)1 << 32) - 1) / 3) return set_err(ctx, CZK_ERR_SIZE, "plonk_layout: 3 n_gates wire slots exceed the 32-bit slot indices");
    if (n_prods > n_gates) return set_err(ctx, CZK_ERR_SIZE, "plonk_layout: more products than gates");
    if (!succ || !w_evals || !s_evals) return set_err(ctx, CZK_ERR_ARG, "null plonk_layout argument");
    const size_t W = 3 * n_gates;
    unsigned k = 0;
    while (((size_t)1 << k) < n_gates) k++;
    MixedDomain* d = nullptr;
    CZK_TRY(get_mixed_domain(ctx, k, &d));   // CZK_ERR_SIZE when no domain of 3 * 2^k elements exists
    if (mem == CZK_MEM_HOST) {               // a permutation of [0, W): every slot below W and none named twice
        std::vector<uint64_t> seen((W + 63) / 64, 0);
        for (size_t i = 0; i < W; i++) {
            const uint32_t e = succ[i];
            if (e >= W) return set_err(ctx, CZK_ERR_ARG, "plonk_layout: succ names a slot beyond the 3 n_gates wire slots");
            if (seen[e >> 6] >> (e & 63) & 1) return set_err(ctx, CZK_ERR_ARG, "plonk_layout: succ is not a permutation (a slot is named twice)");
            seen[e >> 6] |= (uint64_t)1 << (e & 63);
        }
    }
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    unsigned nb = 1;                         // bytes of the largest exponent W - 1
    while (nb < 4 && ((W - 1) >> (8 * nb))) nb++;
    const MarlinRoots roots = pow_table_roots(d->group_gen);
    Staged ss{ctx}, sw{ctx}, se{ctx}, tab{ctx};
    CZK_TRY(ss.to_device(succ, W * 4, mem));
    CZK_TRY(sw.to_device(mem == CZK_MEM_HOST ? nullptr : w_evals, W * 32, mem));
    CZK_TRY(se.to_device(mem == CZK_MEM_HOST ? nullptr : s_evals, n_gates * 32, mem));
    CZK_TRY(tab.to_device(nullptr, 4 * 256 * 32, CZK_MEM_HOST));   // workspace from the staging pool: given back once the kernels are enqueued
    {
        ProfScope ps(ctx, "plonk_layout");
        hipLaunchKernelGGL(k_marlin_pow_tables, dim3(4), dim3(256), 0, ctx->stream, (u64*)tab.dev, roots);
        hipLaunchKernelGGL(k_plonk_layout, grid_for(W, 256), dim3(256), 0, ctx->stream, (const u32*)ss.dev, (u32)W, (u32)n_gates, (u32)n_prods, nb,
                           (const u64*)tab.dev, (u64*)sw.dev, (u64*)se.dev);
    }
    CZK_HIP(ctx, hipGetLastError());
    if (mem == CZK_MEM_HOST) CZK_HIP(ctx, hipMemcpyAsync(s_evals, se.dev, n_gates * 32, hipMemcpyDeviceToHost, ctx->stream));
    return sw.to_host(w_evals, W * 32);      // (host callers: the one blocking point)
}

extern "C" int czk_fr_gather(czk_ctx* ctx, const uint64_t* src, size_t src_len, size_t src_stride, size_t lanes, const uint32_t* index, size_t n,
                             uint64_t* out, size_t out_stride, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (!n || !lanes) return CZK_OK;
    if (!src || !index || !out) return set_err(ctx, CZK_ERR_ARG, "null fr_gather argument");
    if (src_stride < src_len || out_stride < n) return set_err(ctx, CZK_ERR_SIZE, "fr_gather: a lane stride is shorter than the lane");
    if (!src_len) return set_err(ctx, CZK_ERR_SIZE, "fr_gather: nothing to gather from");
    if (lanes > 65535) return set_err(ctx, CZK_ERR_SIZE, "fr_gather: more than 65535 lanes");
    if (n >= ((size_t)1 << 39)) return set_err(ctx, CZK_ERR_SIZE, "fr_gather: more outputs than one launch holds");
    if (mem == CZK_MEM_HOST)
        for (size_t i = 0; i < n; i++)
            if (index[i] >= src_len) return set_err(ctx, CZK_ERR_ARG, "fr_gather: index beyond the source lane");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    // lanes of `stride` elements of which the last holds `len`: the span a host caller's array must cover
    const size_t src_bytes = ((lanes - 1) * src_stride + src_len) * 32, out_bytes = ((lanes - 1) * out_stride + n) * 32;
    Staged ss{ctx}, si{ctx}, so{ctx};
    CZK_TRY(ss.to_device(src, src_bytes, mem));
    CZK_TRY(si.to_device(index, n * 4, mem));
    // a host caller's padding between lanes (out_stride > n) is not the call's to change: it goes up with the buffer and comes back as it was
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST && out_stride == n ? nullptr : out, out_bytes, mem));
    dim3 grid = grid_for(n, 256);
    grid.y = (unsigned)lanes;
    {
        ProfScope ps(ctx, "fr_gather");
        hipLaunchKernelGGL(k_fr_gather, grid, dim3(256), 0, ctx->stream, (const u64*)ss.dev, src_len, src_stride, (const u32*)si.dev, n, (u64*)so.dev,
                           out_stride);
    }
    CZK_HIP(ctx, hipGetLastError());
    return so.to_host(out, out_bytes);
}
