// commit_tree.hip -- czk_fr_vec_commit: the "czk tree commitment v1" of include/czk.h, a SHA-256 tree over the canonical bytes of Fr vectors, hashed on
// the GPU where the vectors live.  The commit-then-open round of the SPDZ open (net_rounds.hip czk_net_atomic_broadcast_tree) is its user.
//
//   leaf_i = SHA256(TAG_LEAF || bytes of a[i E .. min(n, (i + 1) E)))            k_commit_level<true>:  one thread per (lane, leaf)
//   node_j = SHA256(TAG_NODE || up to F digests of the level below)              k_commit_level<false>: one thread per (lane, node), one launch per level
//   commit = SHA256(TAG_ROOT || u64_le(n) || top || rand32)                      k_commit_root:         one thread per lane
//
// A tag is one SHA-256 block, so its chaining value is a constant (host, once: sha256.h) and every hash starts from it.  Leaves and nodes are the same
// loop: 32-byte items, two per block, then the padding for the true item count.  An element becomes SHA's big-endian words by a byte swap of its
// canonical limbs; a digest is kept as its eight state words, which ARE the big-endian words of its bytes.
// Memory: a thread walks its leaf's 1 KiB front to back while its neighbours are 1 KiB away -- no LDS transpose: each 128-byte line a thread touches
// is consumed by that thread within its next two blocks, and the kernel is bound by its integer instructions (~1700 per compression, ~450 per
// Montgomery conversion), not by the loads: measured, EXPERIMENTS.md section 24.
#include "call.h"
#include "sha256.h"
#include "sha256_dev.h"

using namespace czk;

namespace {
constexpr unsigned E = CZK_COMMIT_LEAF_ELEMS, F = CZK_COMMIT_FANOUT;
static_assert(E >= 8 && (E & (E - 1)) == 0 && F >= 8 && (F & (F - 1)) == 0, "leaf size and fan-out are powers of two >= 8");

struct Sha256State {
    u32 h[8];
};

// item k of a hash's input as eight big-endian words: a leaf's k-th element (Montgomery -> canonical, limbs byte-swapped) or a node's k-th child digest
template <bool LEAF>
__device__ __forceinline__ void load_item(const void* base, size_t k, u32* w) {
    if (LEAF) {
        const Fr v = fp_into_repr(fp_load<FrParams>((const u64*)base + 4 * k));
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(v.l[j]);
    } else {
        const uint4* q = (const uint4*)((const u32*)base + 8 * k);
        const uint4 lo = q[0], hi = q[1];
        w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
    }
}

// One level of the tree.  in: per lane `n_in` items (LEAF: Fr elements at lane stride `in_stride` elements; else digests, lane stride n_in);
// out: per lane n_out = ceil(n_in / PER) digests (n_in = 0: the one hash of the tag alone), PER = E or F.  Item idx = lane * n_out + j reads items
// [j PER, min(n_in, (j + 1) PER)) of its lane and writes digest idx: nothing else.
template <bool LEAF>
__global__ void __launch_bounds__(256) k_commit_level(Sha256State tag, const void* in, size_t in_stride, size_t n_in, size_t n_out, size_t lanes, u32* out) {
    constexpr unsigned PER = LEAF ? E : F;
    const size_t total = lanes * n_out;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t lane = idx / n_out, j = idx - lane * n_out;
        const size_t first = j * PER;
        const unsigned cnt = (unsigned)(n_in - first < PER ? n_in - first : PER);   // first <= n_in: j < n_out
        const char* lane_base = (const char*)in + lane * in_stride * 32;
        u32 st[8], w[16];
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = tag.h[i];
        const u32 bits = 512u + 256u * cnt;   // the tag block + cnt items of 32 bytes
#pragma unroll 1
        for (unsigned k = 0; k < cnt; k += 2) {
            load_item<LEAF>(lane_base, first + k, w);
            if (k + 1 < cnt) load_item<LEAF>(lane_base, first + k + 1, w + 8);
            else {   // an odd count: the padding fits behind the last item
                w[8] = 0x80000000u;
#pragma unroll
                for (int i = 9; i < 15; i++) w[i] = 0;
                w[15] = bits;
            }
            sha256_block(st, w);
        }
        if ((cnt & 1) == 0) {   // an even count (0 included): a block of padding
            w[0] = 0x80000000u;
#pragma unroll
            for (int i = 1; i < 15; i++) w[i] = 0;
            w[15] = bits;
            sha256_block(st, w);
        }
        uint4* o = (uint4*)(out + 8 * idx);
        o[0] = make_uint4(st[0], st[1], st[2], st[3]);
        o[1] = make_uint4(st[4], st[5], st[6], st[7]);
    }
}

// commit = SHA256(TAG_ROOT || u64_le(n) || top || rand32): 72 bytes after the tag block, so two blocks.  top: lanes digests; rand, out: lanes x 32 bytes
__global__ void __launch_bounds__(256) k_commit_root(Sha256State tag, unsigned long long n, const u32* top, const u32* rand, size_t lanes, u32* out) {
    for (size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x; lane < lanes; lane += (size_t)gridDim.x * blockDim.x) {
        u32 st[8], w[16];
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = tag.h[i];
        w[0] = __builtin_bswap32((u32)n), w[1] = __builtin_bswap32((u32)(n >> 32));
#pragma unroll
        for (int i = 0; i < 8; i++) w[2 + i] = top[8 * lane + i];
#pragma unroll
        for (int i = 0; i < 6; i++) w[10 + i] = __builtin_bswap32(rand[8 * lane + i]);
        sha256_block(st, w);
        w[0] = __builtin_bswap32(rand[8 * lane + 6]), w[1] = __builtin_bswap32(rand[8 * lane + 7]);
        w[2] = 0x80000000u;
#pragma unroll
        for (int i = 3; i < 15; i++) w[i] = 0;
        w[15] = (64 + 8 + 32 + 32) * 8;
        sha256_block(st, w);
#pragma unroll
        for (int i = 0; i < 8; i++) out[8 * lane + i] = __builtin_bswap32(st[i]);   // the digest's bytes in memory order
    }
}

// chaining value after the tag's one block
Sha256State tag_state(const char* tag) {
    uint8_t block[64] = {0};
    memcpy(block, tag, strlen(tag));
    Sha256 s;
    s.update(block, 64);
    Sha256State r;
    memcpy(r.h, s.h, sizeof r.h);
    return r;
}

constexpr unsigned BLOCKS_PER_CU = 8;   // grid cap of the three kernels, as the pointwise Fr kernels' (fr_vec.hip fr_grid)
unsigned grid_cap(czk_ctx* ctx, size_t items) {   // blocks of 256 threads for a grid-stride loop over `items`
    const size_t max_blocks = (size_t)ctx->num_cu * BLOCKS_PER_CU;
    if (items >= max_blocks * 256) return (unsigned)max_blocks;
    const unsigned blocks = grid_for(items, 256).x;
    return blocks ? blocks : 1u;
}
}  // namespace

namespace czk {
// a: device.  Enqueues the tree and the root on the context's stream, copies the lanes x 32 commitment bytes to out32 (host) and waits for them.
int commit_tree_device(czk_ctx* ctx, const u64* a, size_t lanes, size_t n, size_t stride, const uint8_t* rand32, uint8_t* out32) {
    static const Sha256State T_LEAF = tag_state("czk-commit-v1/leaf"), T_NODE = tag_state("czk-commit-v1/node"), T_ROOT = tag_state("czk-commit-v1/root");
    // digests of every level, then the randomness and the commitments: one piece of per-call scratch
    size_t per_lane = 0;
    for (size_t m = n;;) {
        m = m ? (m + (per_lane ? F : E) - 1) / (per_lane ? F : E) : 1;
        per_lane += m;
        if (m == 1) break;
    }
    if (lanes > (SIZE_MAX / 64) / (per_lane + 2)) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_vec_commit: lanes x levels overflows");
    DeviceBuf ws;
    CZK_TRY(stage_take(ctx, lanes * (per_lane + 2) * 32, &ws));
    u32* level = (u32*)ws.p;
    u32* rnd = level + 8 * lanes * per_lane;
    u32* out = rnd + 8 * lanes;
    int rc = CZK_OK;
    hipError_t e = hipMemcpyAsync(rnd, rand32, lanes * 32, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "commit_tree");
        size_t m = n ? (n + E - 1) / E : 1;
        hipLaunchKernelGGL(k_commit_level<true>, dim3(grid_cap(ctx, lanes * m)), dim3(256), 0, ctx->stream, T_LEAF, (const void*)a, stride, n, m, lanes, level);
        while (m > 1) {
            const size_t up = (m + F - 1) / F;
            u32* next = level + 8 * lanes * m;
            hipLaunchKernelGGL(k_commit_level<false>, dim3(grid_cap(ctx, lanes * up)), dim3(256), 0, ctx->stream, T_NODE, (const void*)level, m, m, up, lanes, next);
            level = next, m = up;
        }
        hipLaunchKernelGGL(k_commit_root, dim3(grid_cap(ctx, lanes)), dim3(256), 0, ctx->stream, T_ROOT, (unsigned long long)n, (const u32*)level, (const u32*)rnd, lanes, out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out32, out, lanes * 32, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // the commitment is the call's result
    if (e != hipSuccess) rc = set_err(ctx, CZK_ERR_HIP, std::string("czk_fr_vec_commit: ") + hipGetErrorString(e));
    stage_give(ctx, ws);
    return rc;
}
}  // namespace czk

extern "C" int czk_fr_vec_commit(czk_ctx* ctx, const uint64_t* a, size_t lanes, size_t n, size_t stride, const uint8_t* rand32, uint8_t* out32, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (stride < n) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_vec_commit: stride < n");
    if (!lanes) return CZK_OK;
    if (n > SIZE_MAX / 32) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_vec_commit: n x 32 overflows");
    // elements spanned by the lanes: (lanes - 1) stride + n, and its 32-fold in bytes
    if (stride && lanes - 1 > (SIZE_MAX / 32 - n) / stride) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_vec_commit: lanes x stride overflows");
    if (lanes > SIZE_MAX / 64) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_vec_commit: too many lanes");
    if (!rand32 || !out32 || (n && !a)) return set_err(ctx, CZK_ERR_ARG, "czk_fr_vec_commit: null argument");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sa{ctx};
    if (n) CZK_TRY(sa.to_device(a, ((lanes - 1) * stride + n) * 32, mem));
    return commit_tree_device(ctx, (const u64*)sa.dev, lanes, n, stride, rand32, out32);
}
