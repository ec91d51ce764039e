// merkle.hip -- the reference's vector commitment of shared values (mpc-algebra/src/com.rs ComField) and the fold of its FRI commit phase
// (mpc-snarks/src/client.rs:767-771) on share lanes that live on one GPU.
//
//   commit         com.rs:36-59    czk_fr_merkle_commit   every lane's binary SHA-256 tree, all 2n - 1 digests kept: merkle_tree_plain.h
//   open_at        com.rs:68-94    czk_fr_merkle_open     k_merkle_open: one thread per (query, lane, level) copies a sibling, one more per (query, lane) the share
//   check_opening  com.rs:95-123   czk_fr_merkle_verify   k_merkle_verify_lane: one thread per (query, lane) re-hashes the share and walks the path;
//                                                         k_merkle_verify_query: one thread per query sums the lanes' shares and counts the failures
//   f[2i] + alpha f[2i+1]          czk_fr_fri_fold        k_fri_fold: one thread per output element and lane
//
// Everything is linear in the shares, so a lane is whatever the caller passes (an additive share, SPDZ's sh lane, a Shamir evaluation).  Bytes are the
// reference's: no tags, no length prefix (merkle_hash.h).  The other tree form -- a workgroup per subtree, levels through LDS -- is kept in lab/merkle_tree_fused.h and
// built into the lab library only (lab/merkle_probe.hip).
#include "call.h"
#include "merkle_hash.h"
#include "merkle_tree_plain.h"

using namespace czk;

namespace {

// digests the caller owns (paths, roots) are read and written word by word: 4-byte alignment is all they need
__device__ __forceinline__ void load_digest_words(const u32* p, u32* w) {
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(p[j]);
}

// item = (query, lane, level) with level == log_n standing for the share.  Reads idx[0..q), and for an index < n one digest of tree[lane] or a[lane][index];
// an index >= n reads neither and writes zeros.  Writes out_shares[0 .. q lanes) and out_paths[0 .. q lanes log_n): nothing else.
__global__ void __launch_bounds__(256) k_merkle_open(const u64* a, size_t stride, size_t n, unsigned log_n, size_t lanes, const u32* tree, size_t tree_stride,
                                                     const unsigned long long* idx, size_t q, u64* out_shares, u32* out_paths) {
    const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per_q = lanes * (log_n + 1);
    if (item >= q * per_q) return;
    const size_t qi = item / per_q, r = item - qi * per_q, lane = r / (log_n + 1);
    const unsigned level = (unsigned)(r - lane * (log_n + 1));
    const unsigned long long i = idx[qi];
    const bool in = i < n;
    if (level == log_n) {
        u64* o = out_shares + 4 * (qi * lanes + lane);
        const u64* s = a + 4 * (lane * stride + (in ? i : 0));
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = in ? s[j] : 0;
    } else {
        u32* o = out_paths + 8 * ((qi * lanes + lane) * log_n + level);
        const u32* s = tree + 8 * (lane * tree_stride + merkle_level_offset(n, level) + (in ? (i >> level) ^ 1 : 0));
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = in ? s[j] : 0;
    }
}

// lane_ok[query lanes + lane] = the share's leaf hash, walked up the path with bit j of the index choosing the side (com.rs:105-121), is roots[lane]
__global__ void __launch_bounds__(256) k_merkle_verify_lane(const u32* roots, size_t lanes, size_t n, unsigned log_n, const unsigned long long* idx, size_t q,
                                                            const u64* shares, const u32* paths, uint8_t* lane_ok) {
    const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= q * lanes) return;
    const size_t qi = item / lanes, lane = item - qi * lanes;
    const unsigned long long i = idx[qi];
    u32 st[8], w[16];
    merkle_leaf_hash(fp_load<FrParams>(shares + 4 * item), st);
    const u32* path = paths + 8 * item * log_n;
#pragma unroll 1
    for (unsigned j = 0; j < log_n; j++) {
        const bool right = (i >> j) & 1;   // this hash is the right child: the sibling goes first
        u32 sib[8];
        load_digest_words(path + 8 * j, sib);
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = right ? sib[k] : st[k], w[8 + k] = right ? st[k] : sib[k];
        merkle_node_hash(w, st);
    }
    load_digest_words(roots + 8 * lane, w);
    bool ok = i < n;
#pragma unroll
    for (int k = 0; k < 8; k++) ok = ok && st[k] == w[k];
    lane_ok[item] = ok;
}

// ok[query] = every lane's path holds and (values given) the lanes' shares sum to values[query] (com.rs:96-98); *bad counts the zeros
__global__ void __launch_bounds__(256) k_merkle_verify_query(size_t lanes, size_t q, const u64* shares, const u64* values, const uint8_t* lane_ok, uint8_t* ok,
                                                             unsigned long long* bad) {
    const size_t qi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= q) return;
    bool good = true;
    Fr sum = Fr::zero();
    for (size_t l = 0; l < lanes; l++) {
        good = good && lane_ok[qi * lanes + l];
        if (values) sum = fp_add(sum, fp_load<FrParams>(shares + 4 * (qi * lanes + l)));
    }
    if (values) {
        const Fr v = fp_load<FrParams>(values + 4 * qi);
#pragma unroll
        for (int k = 0; k < 8; k++) good = good && sum.l[k] == v.l[k];
    }
    ok[qi] = good;
    if (!good) atomicAdd(bad, 1ull);
}

// out[l][j] = f[l][2j] + alpha f[l][2j+1], j < half.  Reads f[l][0 .. 2 half), writes out[l][0 .. half): nothing else.
__global__ void __launch_bounds__(256) k_fri_fold(const u64* f, size_t stride, size_t half, size_t lanes, Fr alpha, u64* out, size_t out_stride) {
    const size_t total = lanes * half;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t lane = idx / half, j = idx - lane * half;
        const u64* p = f + 4 * (lane * stride + 2 * j);
        fp_store<FrParams>(out + 4 * (lane * out_stride + j), fp_add(fp_load<FrParams>(p), fp_mul(alpha, fp_load<FrParams>(p + 4))));
    }
}

// the same with alpha read from device memory (one Montgomery Fr): a challenge a device transcript squeezed, never seen by the host
__global__ void __launch_bounds__(256) k_fri_fold_at(const u64* f, size_t stride, size_t half, size_t lanes, const u64* alpha_at, u64* out, size_t out_stride) {
    const Fr alpha = fp_load<FrParams>(alpha_at);
    const size_t total = lanes * half;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t lane = idx / half, j = idx - lane * half;
        const u64* p = f + 4 * (lane * stride + 2 * j);
        fp_store<FrParams>(out + 4 * (lane * out_stride + j), fp_add(fp_load<FrParams>(p), fp_mul(alpha, fp_load<FrParams>(p + 4))));
    }
}

// n = 2^*log_n, or CZK_ERR_SIZE
int check_pow2(czk_ctx* ctx, const char* who, size_t n, unsigned* log_n) {
    if (!n || (n & (n - 1))) return set_err(ctx, CZK_ERR_SIZE, std::string(who) + ": n must be a power of two");
    unsigned k = 0;
    while (((size_t)1 << k) < n) k++;
    *log_n = k;
    return CZK_OK;
}
// bytes of `lanes` lanes `stride` items of 32 bytes apart, the last of `len` items; CZK_ERR_SIZE when that overflows
int lane_span_bytes(czk_ctx* ctx, const char* who, size_t lanes, size_t stride, size_t len, size_t* bytes) {
    if (len > SIZE_MAX / 32 || (stride && lanes - 1 > (SIZE_MAX / 32 - len) / stride)) return set_err(ctx, CZK_ERR_SIZE, std::string(who) + ": lanes x stride overflows");
    *bytes = ((lanes - 1) * stride + len) * 32;
    return CZK_OK;
}
int check_indices(czk_ctx* ctx, const char* who, const uint64_t* idx, size_t q, size_t n) {
    for (size_t i = 0; i < q; i++)
        if (idx[i] >= n) return set_err(ctx, CZK_ERR_ARG, std::string(who) + ": index beyond the vector");
    return CZK_OK;
}
}  // namespace

extern "C" int czk_fr_merkle_commit(czk_ctx* ctx, const uint64_t* a, size_t lanes, size_t n, size_t stride, uint8_t* tree, size_t tree_stride, uint8_t* roots32,
                                    int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    unsigned log_n = 0;
    CZK_TRY(check_pow2(ctx, "czk_fr_merkle_commit", n, &log_n));
    if (stride < n) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_merkle_commit: stride < n");
    if (n > SIZE_MAX / 64 || tree_stride < 2 * n - 1) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_merkle_commit: tree_stride < 2n - 1");
    if (!lanes) return CZK_OK;
    size_t a_bytes = 0, tree_bytes = 0;
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_merkle_commit", lanes, stride, n, &a_bytes));
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_merkle_commit", lanes, tree_stride, 2 * n - 1, &tree_bytes));
    if (!a || !tree) return set_err(ctx, CZK_ERR_ARG, "czk_fr_merkle_commit: null argument");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sa{ctx}, st{ctx};
    CZK_TRY(sa.to_device(a, a_bytes, mem));
    // a host caller's padding between lanes (tree_stride > 2n - 1) is not the call's to change: it goes up with the buffer and comes back as it was
    CZK_TRY(st.to_device(mem == CZK_MEM_HOST && tree_stride == 2 * n - 1 ? nullptr : tree, tree_bytes, mem));
    {
        ProfScope ps(ctx, "merkle_commit");
        merkle_tree_plain(ctx, (const u64*)sa.dev, lanes, n, log_n, stride, (u32*)st.dev, tree_stride);
    }
    CZK_HIP(ctx, hipGetLastError());
    if (roots32) {   // lane l's root is digest 2n - 2 of its tree
        CZK_HIP(ctx, hipMemcpy2DAsync(roots32, 32, (const uint8_t*)st.dev + (2 * n - 2) * 32, tree_stride * 32, 32, lanes, hipMemcpyDeviceToHost, ctx->stream));
        if (mem == CZK_MEM_DEVICE) CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return st.to_host(tree, tree_bytes);   // (host callers: the blocking point)
}

extern "C" int czk_fr_merkle_open(czk_ctx* ctx, const uint64_t* a, size_t lanes, size_t n, size_t stride, const uint8_t* tree, size_t tree_stride,
                                  const uint64_t* idx, size_t q, uint64_t* out_shares, uint8_t* out_paths, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    unsigned log_n = 0;
    CZK_TRY(check_pow2(ctx, "czk_fr_merkle_open", n, &log_n));
    if (stride < n) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_merkle_open: stride < n");
    if (n > SIZE_MAX / 64 || tree_stride < 2 * n - 1) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_merkle_open: tree_stride < 2n - 1");
    if (!lanes || !q) return CZK_OK;
    size_t a_bytes = 0, tree_bytes = 0;
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_merkle_open", lanes, stride, n, &a_bytes));
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_merkle_open", lanes, tree_stride, 2 * n - 1, &tree_bytes));
    // one thread per (query, lane, level) and per (query, lane): q lanes (log_n + 1) of them, in blocks of 256 of which a launch holds 2^31 - 1
    if (lanes > (((size_t)1 << 38) / (log_n + 1)) / q) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_merkle_open: more openings than one launch holds");
    if (!a || !tree || !idx || !out_shares || (log_n && !out_paths)) return set_err(ctx, CZK_ERR_ARG, "czk_fr_merkle_open: null argument");
    if (mem == CZK_MEM_HOST) CZK_TRY(check_indices(ctx, "czk_fr_merkle_open", idx, q, n));
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t share_bytes = q * lanes * 32, path_bytes = share_bytes * log_n;
    Staged sa{ctx}, st{ctx}, si{ctx}, ss{ctx}, sp{ctx};
    CZK_TRY(sa.to_device(a, a_bytes, mem));
    CZK_TRY(st.to_device(tree, tree_bytes, mem));
    CZK_TRY(si.to_device(idx, q * 8, mem));
    CZK_TRY(ss.to_device(mem == CZK_MEM_HOST ? nullptr : out_shares, share_bytes, mem));
    if (log_n) CZK_TRY(sp.to_device(mem == CZK_MEM_HOST ? nullptr : out_paths, path_bytes, mem));
    {
        ProfScope ps(ctx, "merkle_open");
        hipLaunchKernelGGL(k_merkle_open, grid_for(q * lanes * (log_n + 1), 256), dim3(256), 0, ctx->stream, (const u64*)sa.dev, stride, n, log_n, lanes,
                           (const u32*)st.dev, tree_stride, (const unsigned long long*)si.dev, q, (u64*)ss.dev, (u32*)sp.dev);
    }
    CZK_HIP(ctx, hipGetLastError());
    if (mem == CZK_MEM_HOST && log_n) CZK_HIP(ctx, hipMemcpyAsync(out_paths, sp.dev, path_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return ss.to_host(out_shares, share_bytes);   // (host callers: the blocking point)
}

extern "C" int czk_fr_merkle_verify(czk_ctx* ctx, const uint8_t* roots, size_t lanes, size_t n, const uint64_t* idx, size_t q, const uint64_t* shares,
                                    const uint8_t* paths, const uint64_t* values, uint8_t* ok, size_t* out_bad, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    unsigned log_n = 0;
    CZK_TRY(check_pow2(ctx, "czk_fr_merkle_verify", n, &log_n));
    if (!lanes || !q) return CZK_OK;
    if (lanes > (((size_t)1 << 38) / (log_n + 1)) / q) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_merkle_verify: more openings than one launch holds");
    if (!roots || !idx || !shares || (log_n && !paths) || !ok || !out_bad) return set_err(ctx, CZK_ERR_ARG, "czk_fr_merkle_verify: null argument");
    if (mem == CZK_MEM_HOST) CZK_TRY(check_indices(ctx, "czk_fr_merkle_verify", idx, q, n));
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t share_bytes = q * lanes * 32, path_bytes = share_bytes * log_n;
    Staged sr{ctx}, si{ctx}, ss{ctx}, sp{ctx}, sv{ctx}, so{ctx};
    CZK_TRY(sr.to_device(roots, lanes * 32, mem));
    CZK_TRY(si.to_device(idx, q * 8, mem));
    CZK_TRY(ss.to_device(shares, share_bytes, mem));
    if (log_n) CZK_TRY(sp.to_device(paths, path_bytes, mem));
    if (values) CZK_TRY(sv.to_device(values, q * 32, mem));
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST ? nullptr : ok, q, mem));
    StageHold ws(ctx);   // the failure count, then one flag per (query, lane)
    CZK_TRY(ws.take(8 + q * lanes));
    unsigned long long* bad = (unsigned long long*)ws.b.p;
    uint8_t* lane_ok = (uint8_t*)ws.b.p + 8;
    CZK_HIP(ctx, hipMemsetAsync(bad, 0, 8, ctx->stream));
    {
        ProfScope ps(ctx, "merkle_verify");
        hipLaunchKernelGGL(k_merkle_verify_lane, grid_for(q * lanes, 256), dim3(256), 0, ctx->stream, (const u32*)sr.dev, lanes, n, log_n,
                           (const unsigned long long*)si.dev, q, (const u64*)ss.dev, (const u32*)sp.dev, lane_ok);
        hipLaunchKernelGGL(k_merkle_verify_query, grid_for(q, 256), dim3(256), 0, ctx->stream, lanes, q, (const u64*)ss.dev, (const u64*)sv.dev,
                           (const uint8_t*)lane_ok, (uint8_t*)so.dev, bad);
    }
    CZK_HIP(ctx, hipGetLastError());
    unsigned long long count = 0;
    if (mem == CZK_MEM_HOST) CZK_HIP(ctx, hipMemcpyAsync(ok, so.dev, q, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipMemcpyAsync(&count, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the count is the call's result
    *out_bad = (size_t)count;
    return CZK_OK;
}

extern "C" int czk_fr_fri_fold(czk_ctx* ctx, const uint64_t* f, size_t lanes, size_t n, size_t stride, const uint64_t* alpha, uint64_t* out, size_t out_stride,
                               int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (n < 2) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_fri_fold: n < 2");   // (any n >= 2, as the reference's loop: an odd n leaves its last element out)
    const size_t half = n / 2;
    if (stride < n || out_stride < half) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_fri_fold: a lane stride is shorter than the lane");
    if (!lanes) return CZK_OK;
    size_t f_bytes = 0, out_bytes = 0;
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_fri_fold", lanes, stride, n, &f_bytes));
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_fri_fold", lanes, out_stride, half, &out_bytes));
    if (!f || !alpha || !out) return set_err(ctx, CZK_ERR_ARG, "czk_fr_fri_fold: null argument");
    if (mem == CZK_MEM_DEVICE && (uintptr_t)out < (uintptr_t)f + f_bytes && (uintptr_t)f < (uintptr_t)out + out_bytes)
        return set_err(ctx, CZK_ERR_ARG, "czk_fr_fri_fold: out overlaps f");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sf{ctx}, so{ctx};
    CZK_TRY(sf.to_device(f, f_bytes, mem));
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST && out_stride == half ? nullptr : out, out_bytes, mem));
    const size_t blocks = (lanes * half + 255) / 256, cap = merkle_max_blocks(ctx);
    {
        ProfScope ps(ctx, "fri_fold");
        hipLaunchKernelGGL(k_fri_fold, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, ctx->stream, (const u64*)sf.dev, stride, half, lanes,
                           host_fr(alpha), (u64*)so.dev, out_stride);
    }
    CZK_HIP(ctx, hipGetLastError());
    return so.to_host(out, out_bytes);
}

extern "C" int czk_fr_fri_fold_at(czk_ctx* ctx, const uint64_t* f, size_t lanes, size_t n, size_t stride, const uint64_t* alpha_dev, uint64_t* out, size_t out_stride) {
    if (!ctx) return CZK_ERR_ARG;
    if (n < 2) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_fri_fold_at: n < 2");
    const size_t half = n / 2;
    if (stride < n || out_stride < half) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_fri_fold_at: a lane stride is shorter than the lane");
    if (!lanes) return CZK_OK;
    size_t f_bytes = 0, out_bytes = 0;
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_fri_fold_at", lanes, stride, n, &f_bytes));
    CZK_TRY(lane_span_bytes(ctx, "czk_fr_fri_fold_at", lanes, out_stride, half, &out_bytes));
    if (!f || !alpha_dev || !out) return set_err(ctx, CZK_ERR_ARG, "czk_fr_fri_fold_at: null argument");
    if (((uintptr_t)f | (uintptr_t)alpha_dev | (uintptr_t)out) & 15) return set_err(ctx, CZK_ERR_ARG, "czk_fr_fri_fold_at: device pointers to elements are 16-byte aligned");
    if ((uintptr_t)out < (uintptr_t)f + f_bytes && (uintptr_t)f < (uintptr_t)out + out_bytes) return set_err(ctx, CZK_ERR_ARG, "czk_fr_fri_fold_at: out overlaps f");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t blocks = (lanes * half + 255) / 256, cap = merkle_max_blocks(ctx);
    {
        ProfScope ps(ctx, "fri_fold");
        hipLaunchKernelGGL(k_fri_fold_at, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, ctx->stream, (const u64*)f, stride, half, lanes, (const u64*)alpha_dev,
                           (u64*)out, out_stride);
    }
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}
