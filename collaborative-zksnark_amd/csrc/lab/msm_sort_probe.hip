// msm_sort_probe.hip -- LAB BUILD ONLY (build.py LAB_SOURCES): the digit sort of one MSM call (msm_sort.hip) run on its own, its arrays copied
// back for tests/test_msm_digits.py, which holds them to a big-integer model (tests/msm_digits_model.py).
//
// Not part of the product ABI (include/czk.h): exported by libczk_hip_lab.so alone.  The dimensions, the size of the staging area of k_part_sort
// and the layout of the arrays come from the helpers msm_plan and msm_carve use (czk_internal.h: msm_sort_dims, part_sort_cap, msm_sort_bytes,
// msm_sort_carve); the sort is msm_sort_enqueue itself, on the context's stream.
#include "call.h"
#include "czk_internal.h"

namespace czk {
namespace {
enum { DIM_C, DIM_WD, DIM_W, DIM_LANES, DIM_B, DIM_TOTAL, DIM_N_PARTS, DIM_PART_SHIFT, DIM_CAP, DIM_COUNT };
}
}  // namespace czk

using namespace czk;

// c: the window width, 2 .. 22; 0 with split != 0 asks for the width a table-free key's call of `size` pairs gets.  split: the table-free form (every
// digit window a bucket set of its own); one_pass: the sort of the option "msm_sort_onepass" (ignored with split, as in msm_plan).
// scalars: lanes x n_scalars x 4 u64 (host), of which the first `size` of each vector are used; scalar_form: CZK_SCALAR_*.
// inf: the infinity flags of the table set, Wd x nb bytes (split: nb bytes), or null = none; nb: points per window.  size <= n_scalars, size <= nb.
// dims (host, 9 u64): c, Wd, W, virtual lanes, B, total, n_parts, part_shift, cap.  With digits == null only `dims` is written.  Otherwise (all host):
// digits, sorted: virtual lanes x total u32 (`sorted` holds 0xFFFFFFFF where the sort wrote nothing); counts, offsets, perm: virtual lanes x B u32.
extern "C" int czk_lab_msm_sort(czk_ctx* ctx, unsigned c, int split, int one_pass, const uint64_t* scalars, size_t n_scalars, size_t lanes, size_t size,
                                int scalar_form, const uint8_t* inf, size_t nb, uint64_t* dims, uint32_t* digits, uint32_t* sorted, uint32_t* counts,
                                uint32_t* offsets, uint32_t* perm) {
    if (!ctx || !dims) return ctx ? set_err(ctx, CZK_ERR_ARG, "null msm_sort probe argument") : CZK_ERR_ARG;
    CZK_TRY(check_scalar_form(ctx, scalar_form));
    if (split && c == 0) {
        czk_bases key;
        key.split = true;
        c = msm_width_for(&key, size);
    }
    if (c < 2 || c > 22) return set_err(ctx, CZK_ERR_ARG, "msm_sort probe: the window width is 2 .. 22");
    if (!lanes || size > n_scalars || size > nb) return set_err(ctx, CZK_ERR_ARG, "msm_sort probe: lanes > 0, size <= n_scalars and size <= nb");
    MsmSortDims d{};
    d.n_scalars = n_scalars;
    d.size = size;
    d.nb = nb;
    d.form = scalar_form;
    msm_sort_dims(d, c, msm_num_windows(c), split != 0, lanes, true, one_pass != 0, ctx->lds_per_block);
    if (d.lanes > 65535) return set_err(ctx, CZK_ERR_SIZE, "too many MSM lanes");
    if ((size_t)d.W * d.nb >= ((size_t)1 << 31)) return set_err(ctx, CZK_ERR_SIZE, "W * n_bases exceeds the 31-bit point index");
    if (d.split && (size_t)d.Wd * d.n_parts > MAX_PARTS) return set_err(ctx, CZK_ERR_SIZE, "msm_sort probe: Wd * n_parts exceeds MAX_PARTS at this width");
    if (d.lanes * d.total > ((size_t)1 << 28) || (size_t)d.Wd * d.nb > ((size_t)1 << 28)) return set_err(ctx, CZK_ERR_SIZE, "msm_sort probe: at most 2^28 entries");
    dims[DIM_C] = d.c, dims[DIM_WD] = d.Wd, dims[DIM_W] = d.W, dims[DIM_LANES] = d.lanes, dims[DIM_B] = d.B, dims[DIM_TOTAL] = d.total;
    dims[DIM_N_PARTS] = d.n_parts, dims[DIM_PART_SHIFT] = d.part_shift, dims[DIM_CAP] = part_sort_cap(d);
    if (!digits) return CZK_OK;
    if (!sorted || !counts || !offsets || !perm || (size && !scalars)) return set_err(ctx, CZK_ERR_ARG, "null msm_sort probe argument");

    CallMem mem(ctx, "msm_sort probe");
    const size_t inf_bytes = (d.split ? 1 : (size_t)d.Wd) * nb;
    CZK_TRY(mem.in(scalars, lanes * n_scalars * 32, CZK_MEM_HOST, &d.scalars));
    uint8_t* inf_dev;
    CZK_TRY(mem.get(&inf_dev, inf_bytes));
    if (inf) CZK_HIP(ctx, hipMemcpyAsync(inf_dev, inf, inf_bytes, hipMemcpyHostToDevice, ctx->stream));
    else CZK_HIP(ctx, hipMemsetAsync(inf_dev, 0, inf_bytes, ctx->stream));
    d.tv.c = d.c, d.tv.W = d.Wd, d.tv.cover = nb, d.tv.inf = inf_dev;
    char* ws;
    const size_t ws_bytes = msm_sort_bytes(d);
    CZK_TRY(mem.get(&ws, ws_bytes));
    MsmSortBufs s;
    msm_sort_carve(d, ws, s);
    CZK_HIP(ctx, hipMemsetAsync(ws, 0, ws_bytes, ctx->stream));
    CZK_HIP(ctx, hipMemsetAsync(s.sorted, 0xFF, d.lanes * d.total * 4, ctx->stream));
    CZK_HIP(ctx, msm_sort_enqueue(ctx->stream, d, s));
    CZK_HIP(ctx, hipGetLastError());
    CZK_HIP(ctx, hipMemcpyAsync(digits, s.digits, d.lanes * d.total * 4, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipMemcpyAsync(sorted, s.sorted, d.lanes * d.total * 4, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipMemcpyAsync(counts, s.counts, d.lanes * d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipMemcpyAsync(offsets, s.offsets, d.lanes * d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipMemcpyAsync(perm, s.perm, d.lanes * d.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CZK_OK;
}
