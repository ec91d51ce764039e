// ntt_pass_probe.hip -- LAB BUILD ONLY (build.py LAB_SOURCES): ONE pass of the second-generation NTT run on its own, on a buffer the caller wrote, for
// tests/test_ntt_pass.py, which holds every element of every lane, the elements the pass must leave alone and a guard tail to the integer model of
// tests/ntt_pass_model.py.
//
// Not part of the product ABI (include/czk.h): exported by libczk_hip_lab.so alone.  The launch is launch_ntt2_pass / launch_ntt2_final_first themselves
// (ntt_pass.hip), on the context's stream, with a Pass2Args made by pass2_common; the tables are the domain's own (get_domain / ensure_tables: twu_*,
// cosetu_*, size_inv) -- nothing is rebuilt here.  What a product run cannot do and this can: write the scratch lanes a middle or last pass reads (values
// up to 2 r - 1, residues that cancel), and run a kernel instantiation at a (log_d, s_lo, K) no plan produces, e.g. k_ntt2_strided<7, true> at 2^11.
// The description is validated on the host first: a bad one is CZK_ERR_ARG, never a read or write outside a buffer.
#include "ntt_pass_probe.h"

#include "call.h"
#include "ntt_pass.h"

namespace czk {
namespace {
constexpr unsigned PROBE_NTT2_T = 16;   // ntt_pass.hip NTT2_T (that file defines kernels and cannot be included twice in one library); pinned by tests/test_ntt_pass_cpu.py
constexpr unsigned PROBE_LOG_MIN = NTT2_MIN_LOG, PROBE_LOG_MAX = 14, PROBE_LANES_MAX = 8;

void write_dims(unsigned log_d, uint64_t* dims) {
    const PassPlan pl = pass_plan(log_d);
    dims[CZK_NTT_PROBE_DIM_FORMAT] = (uint64_t)NTT2_SCRATCH_FORMAT, dims[CZK_NTT_PROBE_DIM_ELEM_BYTES] = NTT2_SCRATCH_ELEM_BYTES;
    dims[CZK_NTT_PROBE_DIM_MIN_LOG] = NTT2_MIN_LOG, dims[CZK_NTT_PROBE_DIM_T] = PROBE_NTT2_T, dims[CZK_NTT_PROBE_DIM_GUARD] = CZK_NTT_PROBE_GUARD;
    dims[CZK_NTT_PROBE_DIM_M] = pl.m, dims[CZK_NTT_PROBE_DIM_EQUAL_GROUPS] = pl.equal_groups() ? 1 : 0;
    for (unsigned p = 0; p < 7; p++) {
        dims[CZK_NTT_PROBE_DIM_K + p] = p < pl.m ? pl.K[p] : 0;
        dims[CZK_NTT_PROBE_DIM_S_LO + p] = p < pl.m ? pl.s_lo[p] : 0;
    }
}
}  // namespace
}  // namespace czk

using namespace czk;

extern "C" int czk_lab_ntt_pass(czk_ctx* ctx, const czk_lab_ntt_pass_desc* desc, const void* in, size_t in_bytes, const uint64_t* addend,
                                const uint64_t* postconst2, uint64_t* dims, void* out, size_t out_bytes) {
    if (!ctx || !desc || !dims) return ctx ? set_err(ctx, CZK_ERR_ARG, "null ntt_pass probe argument") : CZK_ERR_ARG;
    const czk_lab_ntt_pass_desc& p = *desc;
    if (!in && !out) {   // the dimensions alone
        if (in_bytes || out_bytes || addend || postconst2) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: null data with sizes or an addend");
        if (p.log_d > 47) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: no plan above 2^47");
        write_dims(p.log_d, dims);
        return CZK_OK;
    }
    if (!in || !out) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: `in` and `out` go together");

    // ---- validation (host): everything the kernels index with
    if (p.log_d < PROBE_LOG_MIN || p.log_d > PROBE_LOG_MAX) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: log_d 11 .. 14");
    if (p.K < 5 || p.K > 7) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: K in {5, 6, 7}");
    if (!p.lanes || p.lanes > PROBE_LANES_MAX) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: 1 .. 8 lanes");
    const size_t D = (size_t)1 << p.log_d;
    const bool fused = p.mode == CZK_NTT_PROBE_FUSED;
    if (p.mode != CZK_NTT_PROBE_PASS && !fused) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: unknown mode");
    if (fused) {
        if (4 + p.K > p.log_d) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: the fused pass wants 4 + C <= log_d");
        if (p.inverse || p.s_lo || p.first || p.last || p.prescale || p.posttab || p.post_mode || p.in_len || p.in_lane_stride || addend || postconst2)
            return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: the fused pass takes log_d, C and lanes alone");
    } else if (p.last) {
        if (p.s_lo != 0) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: a last pass owns the stage bits [0, K)");
        if (p.first || p.prescale) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: a last pass reads scratch lanes");
        if (p.post_mode > 4) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: post_mode 0 .. 4");
        if ((p.post_mode == 2 || p.post_mode == 3) != (p.posttab != 0)) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: post modes 2 and 3, and they alone, read the table");
        if ((p.post_mode == 3 || p.post_mode == 4) != (addend != nullptr)) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: post modes 3 and 4, and they alone, read an addend");
        if ((p.post_mode == 3) != (postconst2 != nullptr)) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: post mode 3, and it alone, takes postconst2");
    } else {
        if (p.s_lo < 4 || p.s_lo + p.K > p.log_d) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: a strided pass wants 4 <= s_lo and s_lo + K <= log_d");
        if (p.post_mode || p.posttab || addend || postconst2) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: post modes belong to a last pass");
        if (p.prescale && !p.first) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: the pre-scale belongs to a first pass");
    }
    const bool first = !fused && p.first, last = !fused && p.last;
    if (first) {
        if (p.in_len > D || p.in_len > p.in_lane_stride || p.in_lane_stride > 2 * D)
            return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: in_len <= min(D, in_lane_stride), in_lane_stride <= 2 D");
    } else if (p.in_len || p.in_lane_stride) {
        return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: in_len and in_lane_stride belong to a first pass");
    }
    const size_t in_elem = first ? 32 : NTT2_SCRATCH_ELEM_BYTES, out_elem = last ? 32 : NTT2_SCRATCH_ELEM_BYTES;
    const size_t in_need = p.lanes * (first ? (size_t)p.in_lane_stride : D) * in_elem, out_need = (p.lanes * D + CZK_NTT_PROBE_GUARD) * out_elem;
    if (in_bytes != in_need || out_bytes != out_need) return set_err(ctx, CZK_ERR_ARG, "ntt_pass probe: in_bytes / out_bytes do not match the description");

    CZK_HIP(ctx, hipSetDevice(ctx->device));
    DomainTables* d = nullptr;
    CZK_TRY(get_domain(ctx, p.log_d, &d));
    CZK_TRY(ensure_tables(ctx, d, fused || p.prescale, p.posttab));
    write_dims(p.log_d, dims);

    // ---- device arrays
    CallMem mem(ctx, "ntt_pass probe");
    hipStream_t st = ctx->stream;
    char *d_in, *d_out;
    u64* d_add = nullptr;
    CZK_TRY(mem.get(&d_in, in_need));
    CZK_TRY(mem.get(&d_out, out_need));
    if (in_need) CZK_HIP(ctx, hipMemcpyAsync(d_in, in, in_need, hipMemcpyHostToDevice, st));
    CZK_HIP(ctx, hipMemsetAsync(d_out, CZK_NTT_PROBE_SENTINEL, out_need, st));
    if (addend) {
        CZK_TRY(mem.get(&d_add, p.lanes * D * 32));
        CZK_HIP(ctx, hipMemcpyAsync(d_add, addend, p.lanes * D * 32, hipMemcpyHostToDevice, st));
    }

    // ---- the one launch
    if (fused) {
        Pass2Args inv = pass2_common(d, true, D, D), fwd = pass2_common(d, false, D, D);   // as witness_map.hip's ifft_coset_fft_device builds them
        inv.s_lo = 0, inv.first = 0, inv.post_mode = 1, inv.in = (const u64*)d_in, inv.out = nullptr;
        fwd.s_lo = p.log_d - p.K, fwd.first = 0, fwd.prescale = d->cosetu_fwd, fwd.in = nullptr, fwd.out = (u64*)d_out;
        CZK_TRY(launch_ntt2_final_first(ctx, inv, fwd, p.K, p.lanes));
    } else {
        Pass2Args a = pass2_common(d, p.inverse != 0, first ? (size_t)p.in_len : D, first ? (size_t)p.in_lane_stride : D);
        a.s_lo = p.s_lo;
        a.first = first ? 1 : 0;
        a.prescale = p.prescale ? d->cosetu_fwd : nullptr;
        a.posttab = p.posttab ? d->cosetu_inv : nullptr;
        a.post_mode = (int)p.post_mode;
        a.addend = d_add;
        if (postconst2) {
            Fr c2;
            for (int i = 0; i < 4; i++) c2.l[2 * i] = (u32)postconst2[i], c2.l[2 * i + 1] = (u32)(postconst2[i] >> 32);
            a.postconst2 = host_fr_to_u(c2);
        }
        a.in = (const u64*)d_in;
        a.out = (u64*)d_out;
        CZK_TRY(launch_ntt2_pass(ctx, a, p.K, last, p.lanes));
    }
    CZK_HIP(ctx, hipMemcpyAsync(out, d_out, out_need, hipMemcpyDeviceToHost, st));
    CZK_HIP(ctx, hipStreamSynchronize(st));
    return CZK_OK;
}
