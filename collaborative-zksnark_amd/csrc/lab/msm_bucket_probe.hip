// msm_bucket_probe.hip -- LAB BUILD ONLY (build.py LAB_SOURCES): the bucket accumulation and the bucket reduction of one MSM call run on their own, on
// entry lists the caller wrote, for tests/test_msm_buckets.py, which holds every bucket, every lane result and the counters of the rare paths to an
// integer model (tests/msm_buckets_model.py).
//
// Not part of the product ABI (include/czk.h): exported by libczk_hip_lab.so alone.  The tables are a registered key's own (czk_bases: twisted Edwards,
// u-form XYZZ or table-free, as registration made them); the workspace comes from the helpers msm_plan and msm_carve use (czk_internal.h: msm_red_dims,
// msm_red_bytes, msm_red_carve); the launches are msm_accumulate_enqueue, msm_fixup_enqueue and msm_reduce_enqueue themselves (msm.hip), on the context's
// stream, under the context's options ("msm_lane_interleave", "msm_reduce_lean").  The lists are validated on the host first: a bad list is an error
// code, never a read outside a buffer.
#include <vector>

#include "call.h"
#include "czk_internal.h"
#include "fq2pu.h"
#include "te.h"

namespace czk {
namespace {
enum { DIM_C, DIM_W, DIM_NB, DIM_FAMILY, DIM_HEAVY_CHUNK, DIM_HEAVY_SUB, DIM_EXC_CAP, DIM_HEAVY_CAP, DIM_COUNT };
enum { FAM_TE = 0, FAM_U = 1, FAM_SAT = 2 };   // bucket arithmetic: twisted Edwards (G1), u-form XYZZ, saturated XYZZ (lab options only)
enum { CNT_EXC, CNT_DIRTY, CNT_ITEMS, CNT_HEAVY, CNT_OVERFLOW, CNT_COUNT };
// msm_acc.h / msm_acc_g1.hip / msm_acc_g2.hip (those headers define kernels and cannot be included twice in one library); pinned by tests/test_msm_buckets_cpu.py
constexpr u32 PROBE_HEAVY_CHUNK = 1024, PROBE_HEAVY_SUB = 256, PROBE_EXC_CAP = 4096;

// buckets -> Jacobian triples with the converters the reduction's last step uses
__global__ void k_probe_buckets_g1(const u64* buckets, size_t n, int family, u64* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64* p = buckets + 24 * i;
    Jac<Fq> j;
    if (family == FAM_TE) j = teu_to_jac(teu_load(p));
    else if (family == FAM_U) j = xyzz_to_jac(xyzzu_to_sat(xyzzu_load(p)));
    else j = xyzz_to_jac(xyzz_load<Fq>(p));
    jac_store<Fq>(out + 18 * i, j);
}
__global__ void k_probe_buckets_g2(const u64* buckets, size_t n, int family, u64* out) {   // one point per lane PAIR (fq2pu.h)
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
    if (i >= n) return;
    const u64* p = buckets + 48 * i;
    if (family == FAM_U) jac_store<Fq2P>(out + 36 * i, xyzz_to_jac(xyzzu2_to_sat(xyzzu2_load(p))));
    else jac_store<Fq2P>(out + 36 * i, xyzz_to_jac(xyzz_load<Fq2P>(p)));
}
}  // namespace
}  // namespace czk

using namespace czk;

// bases: a registered key.  lanes: bucket sets; B: buckets per set, a power of two, 128 .. 2^15; total: entries per lane (the stride of `sorted`).
// sorted: lanes x total entry codes (w * nb + i) | sign << 31; offsets, counts, perm: lanes x B (all host).  Per lane every segment [offsets[b],
// offsets[b] + counts[b]) must lie in [0, total), the counts must sum to at most `total`, every entry of a segment must name a table entry that is not
// at infinity (the sort drops those), and perm must be a permutation of 0 .. B - 1: CZK_ERR_ARG otherwise.
// dims (host, 8 u64): the key's window width c (0: table-free), W and nb (windows and points per window of its tables), the bucket arithmetic (0 twisted
// Edwards, 1 u-form XYZZ, 2 saturated XYZZ), HEAVY_CHUNK, HEAVY_SUB, the exception cap, the work-item cap.  With buckets_jac == null only `dims` is written.
// buckets_jac: lanes x B Jacobian triples (18 | 36 u64) after the fix-up; counters: 5 u32 -- raw exc_count, dirty buckets, heavy_hdr[0..2] (work items,
// over-full buckets, overflow flag), the first two 0 for the twisted Edwards family, which has no exception list; result_jac: lanes triples.
extern "C" int czk_lab_msm_buckets(czk_ctx* ctx, const czk_bases* bases, size_t lanes, size_t B, size_t total, const uint32_t* sorted, const uint32_t* offsets,
                                   const uint32_t* counts, const uint32_t* perm, uint64_t* dims, uint64_t* buckets_jac, uint32_t* counters, uint64_t* result_jac) {
    if (!ctx || !bases || !dims) return ctx ? set_err(ctx, CZK_ERR_ARG, "null msm_buckets probe argument") : CZK_ERR_ARG;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const czk_bases* b = bases;
    const bool g1 = b->group == CZK_G1;
    if (!b->te && !b->unsat) return set_err(ctx, CZK_ERR_ARG, "msm_buckets probe: keys with saturated window tables are not probed");
    const size_t nb = b->n, W = b->split ? 1 : b->W;
    if (!lanes || lanes > 64 || B < 128 || B > ((size_t)1 << 15) || (B & (B - 1)) || total > ((size_t)1 << 24))
        return set_err(ctx, CZK_ERR_ARG, "msm_buckets probe: 1 .. 64 lanes, B a power of two in 128 .. 2^15, at most 2^24 entries per lane");
    // (the lab options that move the reduction to the saturated form apply as in msm_plan)
    const int ub = (b->te || !(g1 ? ctx->msm_reduce_sat : ctx->msm_reduce_sat || ctx->msm_reduce_sat_g2)) ? 1 : 0;
    const int family = b->te ? FAM_TE : ub ? FAM_U : FAM_SAT;
    MsmRedDims rd;
    msm_red_dims(rd, g1, lanes, B, total);
    dims[DIM_C] = b->split ? 0 : b->c, dims[DIM_W] = W, dims[DIM_NB] = nb, dims[DIM_FAMILY] = (uint64_t)family;
    dims[DIM_HEAVY_CHUNK] = PROBE_HEAVY_CHUNK, dims[DIM_HEAVY_SUB] = PROBE_HEAVY_SUB, dims[DIM_EXC_CAP] = b->te ? 0 : PROBE_EXC_CAP, dims[DIM_HEAVY_CAP] = rd.heavy_cap;
    if (!buckets_jac) return CZK_OK;
    if (!counters || !result_jac || !offsets || !counts || !perm || (total && !sorted)) return set_err(ctx, CZK_ERR_ARG, "null msm_buckets probe argument");

    // ---- validation (host) ----
    std::vector<uint8_t> inf(W * nb);
    if (!inf.empty()) CZK_HIP(ctx, hipMemcpy(inf.data(), b->inf, inf.size(), hipMemcpyDeviceToHost));
    std::vector<uint8_t> seen(B);
    for (size_t ln = 0; ln < lanes; ln++) {
        std::fill(seen.begin(), seen.end(), 0);
        size_t sum = 0;
        for (size_t k = 0; k < B; k++) {
            const size_t off = offsets[ln * B + k], cnt = counts[ln * B + k], pb = perm[ln * B + k];
            if (off > total || cnt > total - off) return set_err(ctx, CZK_ERR_ARG, "msm_buckets probe: a segment lies outside `sorted`");
            sum += cnt;
            if (pb >= B || seen[pb]) return set_err(ctx, CZK_ERR_ARG, "msm_buckets probe: perm is not a permutation");
            seen[pb] = 1;
            for (size_t e = 0; e < cnt; e++) {
                const size_t idx = sorted[ln * total + off + e] & 0x7fffffffu;
                if (idx >= W * nb) return set_err(ctx, CZK_ERR_ARG, "msm_buckets probe: an entry index outside the table");
                if (inf[idx]) return set_err(ctx, CZK_ERR_ARG, "msm_buckets probe: an entry names a table entry at infinity");
            }
        }
        if (sum > total) return set_err(ctx, CZK_ERR_ARG, "msm_buckets probe: the counts of a lane exceed `total`");
    }

    // ---- device arrays ----
    CallMem mem(ctx, "msm_buckets probe");
    MsmSortBufs s{};
    u32 *d_sorted, *d_offsets, *d_counts, *d_perm;
    CZK_TRY(mem.get(&d_sorted, lanes * total * 4));
    CZK_TRY(mem.get(&d_offsets, lanes * B * 4));
    CZK_TRY(mem.get(&d_counts, lanes * B * 4));
    CZK_TRY(mem.get(&d_perm, lanes * B * 4));
    hipStream_t st = ctx->stream;
    if (total) CZK_HIP(ctx, hipMemcpyAsync(d_sorted, sorted, lanes * total * 4, hipMemcpyHostToDevice, st));
    CZK_HIP(ctx, hipMemcpyAsync(d_offsets, offsets, lanes * B * 4, hipMemcpyHostToDevice, st));
    CZK_HIP(ctx, hipMemcpyAsync(d_counts, counts, lanes * B * 4, hipMemcpyHostToDevice, st));
    CZK_HIP(ctx, hipMemcpyAsync(d_perm, perm, lanes * B * 4, hipMemcpyHostToDevice, st));
    s.sorted = d_sorted, s.offsets = d_offsets, s.counts = d_counts, s.perm = d_perm;
    char* ws;
    const size_t ws_bytes = msm_red_bytes(rd);
    CZK_TRY(mem.get(&ws, ws_bytes));
    CZK_HIP(ctx, hipMemsetAsync(ws, 0, ws_bytes, st));
    MsmRedBufs w;
    msm_red_carve(rd, ws, w);
    u64* d_jac;
    CZK_TRY(mem.get(&d_jac, lanes * B * rd.JW * 8));

    // ---- the stages, in the pipeline's order ----
    const bool list = b->unsat && !b->te;   // the families with dirty flags and an exception list
    const MsmStageArgs a{g1, b->te, b->unsat, ub, ctx->msm_reduce_lean, (unsigned)lanes, B, total, b->pts, rd.heavy_cap, nullptr};
    if (list) (g1 ? launch_accumulate_g1_u_prepare : launch_accumulate_g2_u_prepare)(st, w.dirty, B, (unsigned)lanes);
    const bool split_before = ctx->msm_launch_split;
    ctx->msm_launch_split = b->split;   // (the default interleave rule reads it)
    const int rc = msm_accumulate_enqueue(ctx, st, a, s, w);
    ctx->msm_launch_split = split_before;
    CZK_TRY(rc);
    msm_fixup_enqueue(st, a, s, w);
    CZK_HIP(ctx, hipGetLastError());
    const size_t n = lanes * B, flags = (n + 15) & ~(size_t)15;
    if (g1) hipLaunchKernelGGL(k_probe_buckets_g1, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, w.buckets, n, family, d_jac);
    else hipLaunchKernelGGL(k_probe_buckets_g2, dim3((unsigned)((2 * n + 127) / 128)), dim3(128), 0, st, w.buckets, n, family, d_jac);
    std::vector<uint8_t> dirty(n);
    u32 exc = 0, hdr[4] = {0, 0, 0, 0};
    if (list) {
        CZK_HIP(ctx, hipMemcpyAsync(dirty.data(), w.dirty, n, hipMemcpyDeviceToHost, st));
        CZK_HIP(ctx, hipMemcpyAsync(&exc, w.dirty + flags, 4, hipMemcpyDeviceToHost, st));
    }
    CZK_HIP(ctx, hipMemcpyAsync(hdr, w.heavy_hdr, 16, hipMemcpyDeviceToHost, st));
    CZK_HIP(ctx, hipMemcpyAsync(buckets_jac, d_jac, n * rd.JW * 8, hipMemcpyDeviceToHost, st));
    msm_reduce_enqueue(st, a, w);
    CZK_HIP(ctx, hipGetLastError());
    CZK_HIP(ctx, hipMemcpyAsync(result_jac, w.result, lanes * rd.JW * 8, hipMemcpyDeviceToHost, st));
    CZK_HIP(ctx, hipStreamSynchronize(st));
    u32 n_dirty = 0;
    for (uint8_t d : dirty) n_dirty += d != 0;
    counters[CNT_EXC] = exc, counters[CNT_DIRTY] = n_dirty, counters[CNT_ITEMS] = hdr[0], counters[CNT_HEAVY] = hdr[1], counters[CNT_OVERFLOW] = hdr[2];
    return CZK_OK;
}
