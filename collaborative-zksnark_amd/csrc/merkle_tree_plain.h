// merkle_tree_plain.h -- the tree of czk_fr_merkle_commit, plain form: one thread per leaf, then one launch per level (log2 n + 1 launches; every level
// above the leaves reads its children back from the tree).  The shipped form: measured against the fused form of lab/merkle_tree_fused.h in
// EXPERIMENTS.md section 31.
#pragma once
#include "call.h"
#include "merkle_hash.h"

namespace czk {
namespace {

// level 0: digest i of lane l = the leaf hash of a[l][i].  Reads a[l][0..n), writes tree[l][0..n): nothing else.
__global__ void __launch_bounds__(256) k_merkle_leaves(const u64* a, size_t stride, size_t n, size_t lanes, u32* tree, size_t tree_stride) {
    const size_t total = lanes * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t lane = idx / n, i = idx - lane * n;
        u32 st[8];
        merkle_leaf_hash(fp_load<FrParams>(a + 4 * (lane * stride + i)), st);
        merkle_store_digest(tree + 8 * (lane * tree_stride + i), st);
    }
}

// level `level` >= 1 (m = n >> level digests per lane) from the level below.  Writes that level of tree[l]: nothing else.
__global__ void __launch_bounds__(256) k_merkle_level(size_t n, unsigned level, size_t lanes, u32* tree, size_t tree_stride) {
    const size_t m = n >> level, total = lanes * m;
    const size_t below = merkle_level_offset(n, level - 1), here = merkle_level_offset(n, level);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t lane = idx / m, i = idx - lane * m;
        u32* lt = tree + 8 * lane * tree_stride;
        u32 st[8], w[16];
        merkle_load_digest(lt + 8 * (below + 2 * i), w), merkle_load_digest(lt + 8 * (below + 2 * i + 1), w + 8);
        merkle_node_hash(w, st);
        merkle_store_digest(lt + 8 * (here + i), st);
    }
}

inline void merkle_tree_plain(czk_ctx* ctx, const u64* a, size_t lanes, size_t n, unsigned log_n, size_t stride, u32* tree, size_t tree_stride) {
    const size_t cap = merkle_max_blocks(ctx);
    auto grid = [&](size_t items) {
        const size_t blocks = (items + 255) / 256;
        return dim3((unsigned)(blocks < cap ? blocks : cap));
    };
    hipLaunchKernelGGL(k_merkle_leaves, grid(lanes * n), dim3(256), 0, ctx->stream, a, stride, n, lanes, tree, tree_stride);
    for (unsigned level = 1; level <= log_n; level++)
        hipLaunchKernelGGL(k_merkle_level, grid(lanes * (n >> level)), dim3(256), 0, ctx->stream, n, level, lanes, tree, tree_stride);
}

}  // namespace
}  // namespace czk
