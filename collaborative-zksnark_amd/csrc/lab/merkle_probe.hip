// merkle_probe.hip -- lab library only: czk_lab_merkle_commit builds the tree of czk_fr_merkle_commit with the form that was NOT shipped (a workgroup per
// subtree, merkle_tree_fused.h), so that tools/fri_bench.py can time the two forms against each other and tests/test_merkle_fri.py can hold this one to the
// same bytes.  Device memory only; arguments and checks as czk_fr_merkle_commit's; only enqueues.
#include "merkle_tree_fused.h"

using namespace czk;

extern "C" int czk_lab_merkle_commit(czk_ctx* ctx, const uint64_t* a, size_t lanes, size_t n, size_t stride, uint8_t* tree, size_t tree_stride) {
    if (!ctx) return CZK_ERR_ARG;
    if (!n || (n & (n - 1))) return set_err(ctx, CZK_ERR_SIZE, "czk_lab_merkle_commit: n must be a power of two");
    if (stride < n || n > SIZE_MAX / 64 || tree_stride < 2 * n - 1) return set_err(ctx, CZK_ERR_SIZE, "czk_lab_merkle_commit: a lane stride is shorter than the lane");
    if (!lanes) return CZK_OK;
    if (lanes - 1 > (SIZE_MAX / 32 - (2 * n - 1)) / tree_stride || lanes - 1 > (SIZE_MAX / 32 - n) / stride)
        return set_err(ctx, CZK_ERR_SIZE, "czk_lab_merkle_commit: lanes x stride overflows");
    if (!a || !tree) return set_err(ctx, CZK_ERR_ARG, "czk_lab_merkle_commit: null argument");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    unsigned log_n = 0;
    while (((size_t)1 << log_n) < n) log_n++;
    {
        ProfScope ps(ctx, "merkle_commit_fused");
        merkle_tree_fused(ctx, (const u64*)a, lanes, n, log_n, stride, (u32*)tree, tree_stride);
    }
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}
