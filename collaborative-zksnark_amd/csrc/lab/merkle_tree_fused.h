// merkle_tree_fused.h -- the tree of czk_fr_merkle_commit, fused form: one workgroup of 2^S threads hashes a subtree.  Measured against the plain form and
// not shipped: faster below 2^16 leaves, 2.4 x slower at 2^21 (EXPERIMENTS.md section 31).  Lab library only (merkle_probe.hip).
//
// A launch starts at tree level L0 (m = n >> L0 digests per lane).  Thread t of a subtree makes digest sub 2^S + t of that level -- the leaf hash of its
// element (L0 = 0), or the hash of its two children at level L0 - 1, read from the tree -- writes it to the tree and leaves its state words in LDS.  Then up to
// S levels follow through LDS, a barrier each: thread t < c hashes entries 2t and 2t + 1 of the level below into entry t of the other LDS buffer and writes
// the digest to its place in the tree.  So a launch writes S + 1 levels, a tree takes ceil((log2 n + 1) / (S + 1)) launches, and no digest is read back
// from HBM inside a subtree.  LDS: two buffers of 2^S digests, word-major ([word][entry]: thread t's reads of entries 2t, 2t + 1 are a stride of two banks).
// S = 8: 16 KiB of LDS and 256 threads per workgroup, so neither LDS (160 KiB per CU: 10 workgroups) nor the wave slots (8 workgroups of 4 waves) bind
// before the other; a launch's upper levels idle most of a workgroup's lanes, and the other resident workgroups' lower levels fill the SIMDs meanwhile.
#pragma once
#include "../call.h"
#include "../merkle_hash.h"

namespace czk {
namespace {

constexpr unsigned MERKLE_SUBTREE_LOG = 8;   // S

// Reads a[lane][0..n) (LEAF) or level L0 - 1 of the tree; writes levels L0 .. L0 + min(S, log2 m) of tree[lane]: nothing else.
template <unsigned S, bool LEAF>
__global__ void __launch_bounds__(1u << S) k_merkle_subtree(const u64* a, size_t stride, size_t n, unsigned L0, size_t lanes, u32* tree, size_t tree_stride) {
    constexpr unsigned T = 1u << S;
    __shared__ u32 lds[2][8][T];
    const size_t m = n >> L0;                                // digests per lane at level L0
    const unsigned cnt = m < T ? (unsigned)m : T;            // ... and per subtree
    const size_t per_lane = m / cnt, subtrees = lanes * per_lane;
    const unsigned t = threadIdx.x;
    for (size_t s = blockIdx.x; s < subtrees; s += gridDim.x) {   // (uniform per workgroup: the barriers below are reached by all of it)
        const size_t lane = s / per_lane, sub = s - lane * per_lane;
        u32* lt = tree + 8 * lane * tree_stride;
        u32 st[8], w[16];
        if (t < cnt) {
            const size_t i = sub * cnt + t;
            if (LEAF) merkle_leaf_hash(fp_load<FrParams>(a + 4 * (lane * stride + i)), st);
            else {
                const u32* ch = lt + 8 * (merkle_level_offset(n, L0 - 1) + 2 * i);
                merkle_load_digest(ch, w), merkle_load_digest(ch + 8, w + 8);
                merkle_node_hash(w, st);
            }
            merkle_store_digest(lt + 8 * (merkle_level_offset(n, L0) + i), st);
#pragma unroll
            for (int j = 0; j < 8; j++) lds[0][j][t] = st[j];
        }
        unsigned buf = 0, level = L0;
        for (unsigned c = cnt >> 1; c; c >>= 1) {
            __syncthreads();
            level++;
            if (t < c) {
#pragma unroll
                for (int j = 0; j < 8; j++) w[j] = lds[buf][j][2 * t], w[8 + j] = lds[buf][j][2 * t + 1];
                merkle_node_hash(w, st);
                merkle_store_digest(lt + 8 * (merkle_level_offset(n, level) + sub * c + t), st);
#pragma unroll
                for (int j = 0; j < 8; j++) lds[buf ^ 1][j][t] = st[j];
            }
            buf ^= 1;
        }
        __syncthreads();   // the next subtree's first level overwrites buffer 0
    }
}

// Enqueues the whole tree of `lanes` device vectors (n = 2^log_n elements, `stride` apart) on the context's stream.
inline void merkle_tree_fused(czk_ctx* ctx, const u64* a, size_t lanes, size_t n, unsigned log_n, size_t stride, u32* tree, size_t tree_stride) {
    constexpr unsigned S = MERKLE_SUBTREE_LOG;
    const size_t cap = merkle_max_blocks(ctx);
    for (unsigned L0 = 0; L0 <= log_n; L0 += S + 1) {
        const size_t m = n >> L0, subtrees = lanes * (m >> S ? m >> S : 1);
        const dim3 grid((unsigned)(subtrees < cap ? subtrees : cap));
        if (L0 == 0) hipLaunchKernelGGL((k_merkle_subtree<S, true>), grid, dim3(1u << S), 0, ctx->stream, a, stride, n, L0, lanes, tree, tree_stride);
        else hipLaunchKernelGGL((k_merkle_subtree<S, false>), grid, dim3(1u << S), 0, ctx->stream, a, stride, n, L0, lanes, tree, tree_stride);
    }
}

}  // namespace
}  // namespace czk
