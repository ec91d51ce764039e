// point_ops.hip -- elementwise group arithmetic on device arrays of BLS12-377 G1 / G2 points for gfx950.
//
// The O(n) group steps a verifier runs around its pairings (poly-commit/src/kzg10/mod.rs:295-371), which the host calls czk_jac_add /
// czk_jac_scalar_mul (core.hip) only offer one point at a time:
//   czk_points_add ... out[i] = a[i] +- b[i]       add_assign_mixed with its full case analysis (short_weierstrass_jacobian.rs:570-638)
//   czk_points_mul ... out[i] = [k_i] P_i          ProjectiveCurve::mul (algebra/ec/src/lib.rs:215-230): double-and-add from the top bit
//   czk_points_sum ... out[j] = sum of a segment   add_assign (:666-728) in a tree: one wave per segment, partial sums combined through LDS
// Points are affine Montgomery + one infinity byte, as everywhere in the ABI; no call makes a subgroup assumption (curve.h's jac_add_mixed /
// jac_add / jac_double are complete: P = Q doubles, P = -Q and 2 * (x, 0) leave z = 0).  Each kernel writes Jacobian triples into a workspace and
// ONE batched normalisation per launch (msm_bases.hip's k_batch_to_affine through launch_batch_to_affine, as fixed_base.hip) writes the affine results:
// infinity is flag 1 with the coordinates (0, 1).
// All arithmetic is the 32-bit-limb integer VALU code of field.h / curve.h, with the Montgomery multiply out of line (-DCZK_NOINLINE_MUL).
#include "call.h"

namespace czk {

// out[i] = a[i * a_stride] +- b[i * b_stride] (Jacobian); a stride of 0 repeats one point
template <class F>
__global__ __launch_bounds__(128) void k_points_add(const u64* a, const uint8_t* a_inf, size_t a_stride, const u64* b, const uint8_t* b_inf, size_t b_stride,
                                                    size_t n, int negate_b, u64* out_jac) {
    constexpr int AW = GT<F>::AW, JW = GT<F>::JW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t ia = a_stride ? i : 0, ib = b_stride ? i : 0;
    const bool ai = a_inf && a_inf[ia], bi = b_inf && b_inf[ib];
    Affine<F> q = aff_load<F>(b + (size_t)AW * ib);
    if (negate_b) q.y = f_neg(q.y);
    Jac<F> p = Jac<F>::zero();
    if (!ai) {
        const Affine<F> pa = aff_load<F>(a + (size_t)AW * ia);
        p = Jac<F>{pa.x, pa.y, F::one()};
    }
    jac_store<F>(out_jac + (size_t)JW * i, jac_add_mixed(p, q, bi));
}

// out[i] = [k_i] P_(i * stride) (Jacobian): 256 doublings and one mixed addition per set bit, the same loop for every thread
template <class F>
__global__ __launch_bounds__(128) void k_points_mul(const u64* pts, const uint8_t* inf, size_t stride, const u64* scalars, size_t n, int montgomery,
                                                    u64* out_jac) {
    constexpr int AW = GT<F>::AW, JW = GT<F>::JW;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = fp_load<FrParams>(scalars + 4 * i);
    if (montgomery) s = fp_into_repr(s);   // ec/src/lib.rs:305-307
    const size_t ip = stride ? i : 0;
    const bool p_inf = inf && inf[ip];
    const Affine<F> q = aff_load<F>(pts + (size_t)AW * ip);
    Jac<F> acc = Jac<F>::zero();
#pragma unroll 1
    for (int limb = 7; limb >= 0; limb--) {
        u32 w = 0;   // (selected, not indexed: a register array indexed by a loop counter goes to scratch)
#pragma unroll
        for (int j = 0; j < 8; j++) w = j == limb ? s.l[j] : w;
#pragma unroll 1
        for (int b = 31; b >= 0; b--) {
            acc = jac_double(acc);
            if ((w >> b) & 1) acc = jac_add_mixed(acc, q, p_inf);
        }
    }
    jac_store<F>(out_jac + (size_t)JW * i, acc);
}

// out[j] = sum of pts[offs[j] .. offs[j + 1]) (Jacobian).  One wave per segment, two segments per block: lane l adds the points l, l + 64, ...
// of its segment, then six halving steps through LDS add lane l + s into lane l with the complete jac_add (equal partial sums double, opposite
// ones give infinity).
template <class F>
__global__ __launch_bounds__(128) void k_points_sum(const u64* pts, const uint8_t* inf, const size_t* offs, size_t k, u64* out_jac) {
    constexpr int AW = GT<F>::AW, JW = GT<F>::JW;
    __shared__ __align__(16) u64 lds[128 * JW];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t seg = (size_t)blockIdx.x * 2 + wave;
    Jac<F> acc = Jac<F>::zero();
    if (seg < k) {
        const size_t lo = offs[seg], hi = offs[seg + 1];
#pragma unroll 1
        for (size_t i = lo + lane; i < hi; i += 64) acc = jac_add_mixed(acc, aff_load<F>(pts + (size_t)AW * i), inf && inf[i]);
    }
    u64* mine = lds + (size_t)JW * threadIdx.x;
#pragma unroll 1
    for (unsigned s = 32; s; s >>= 1) {   // (every thread of the block takes every barrier: a wave without a segment carries infinity)
        if (lane >= s && lane < 2 * s) jac_store<F>(mine, acc);
        __syncthreads();
        if (lane < s) acc = jac_add(acc, jac_load<F>(mine + (size_t)JW * s));
        __syncthreads();
    }
    if (lane == 0 && seg < k) jac_store<F>(out_jac + (size_t)JW * seg, acc);
}

int points_add_device(czk_ctx* ctx, int group, const u64* a, const uint8_t* a_inf, size_t a_stride, const u64* b, const uint8_t* b_inf, size_t b_stride,
                      size_t n, int negate_b, u64* out, uint8_t* out_inf) {
    if (!n) return CZK_OK;
    return launch_to_affine(ctx, "points_add", "points_add", group, n, out, out_inf, [&](auto tag, u64* jac) {
        hipLaunchKernelGGL(k_points_add<typename decltype(tag)::type>, grid_for(n), dim3(128), 0, ctx->stream, a, a_inf, a_stride, b, b_inf, b_stride, n,
                           negate_b, jac);
    });
}

int points_mul_device(czk_ctx* ctx, int group, const u64* pts, const uint8_t* inf, size_t stride, const u64* scalars, size_t n, int scalar_form, u64* out,
                      uint8_t* out_inf) {
    if (!n) return CZK_OK;
    const int mont = scalar_form == CZK_SCALAR_MONTGOMERY ? 1 : 0;
    return launch_to_affine(ctx, "points_mul", "points_mul", group, n, out, out_inf, [&](auto tag, u64* jac) {
        hipLaunchKernelGGL(k_points_mul<typename decltype(tag)::type>, grid_for(n), dim3(128), 0, ctx->stream, pts, inf, stride, scalars, n, mont, jac);
    });
}

// offs_host: k + 1 offsets, checked by the caller; they travel through the context's pinned transfer buffer, so the call only enqueues
int points_sum_device(czk_ctx* ctx, int group, const u64* pts, const uint8_t* inf, const size_t* offs_host, size_t k, u64* out, uint8_t* out_inf) {
    if (!k) return CZK_OK;
    DeviceBuf ws, ob;   // (the workspace first, then the offsets: the order the pool has always been asked in)
    CZK_TRY(stage_take(ctx, affine_ws_bytes(group, k), &ws));
    int rc = stage_take(ctx, (k + 1) * sizeof(size_t), &ob);
    if (rc == CZK_OK) rc = upload_pageable(ctx, ob.p, offs_host, (k + 1) * sizeof(size_t));
    if (rc == CZK_OK)
        rc = launch_to_affine(ctx, "points_sum", "points_sum", group, k, out, out_inf, [&](auto tag, u64* jac) {
            hipLaunchKernelGGL(k_points_sum<typename decltype(tag)::type>, grid_for(k, 2), dim3(128), 0, ctx->stream, pts, inf, (const size_t*)ob.p, k, jac);
        }, &ws);
    stage_give(ctx, ob);
    stage_give(ctx, ws);
    return rc;
}

}  // namespace czk

using namespace czk;

// Host-memory callers: every input staged into HBM, the results copied back (blocking); device-memory callers: used in place.
extern "C" int czk_points_add(czk_ctx* ctx, int group, const uint64_t* a, const uint8_t* a_inf, const uint64_t* b, const uint8_t* b_inf, size_t n,
                              int negate_b, uint64_t* out, uint8_t* out_inf, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_group_mem(ctx, group, mem));
    if (!n) return CZK_OK;
    if (!a || !b || !out) return set_err(ctx, CZK_ERR_ARG, "null points_add buffer");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t aw = group == CZK_G1 ? 12 : 24;
    Staged sa{ctx}, sai{ctx}, sb{ctx}, sbi{ctx};
    AffineOut so(ctx);
    CZK_TRY(sa.to_device(a, n * aw * 8, mem));
    CZK_TRY(sb.to_device(b, n * aw * 8, mem));
    if (a_inf) CZK_TRY(sai.to_device(a_inf, n, mem));
    if (b_inf) CZK_TRY(sbi.to_device(b_inf, n, mem));
    CZK_TRY(so.open(group, out, out_inf, n, mem));
    CZK_TRY(points_add_device(ctx, group, (const u64*)sa.dev, (const uint8_t*)sai.dev, 1, (const u64*)sb.dev, (const uint8_t*)sbi.dev, 1, n, negate_b ? 1 : 0,
                              so.pts.words(), so.inf.flags()));
    return so.close();
}

extern "C" int czk_points_mul(czk_ctx* ctx, int group, const uint64_t* pts, const uint8_t* inf, size_t pts_stride, const uint64_t* scalars, size_t n,
                              int scalar_form, uint64_t* out, uint8_t* out_inf, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_group_mem(ctx, group, mem));
    if (pts_stride > 1) return set_err(ctx, CZK_ERR_ARG, "pts_stride must be 1, or 0 for one point");
    CZK_TRY(check_scalar_form(ctx, scalar_form));
    if (!n) return CZK_OK;
    if (!pts || !scalars || !out) return set_err(ctx, CZK_ERR_ARG, "null points_mul buffer");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t aw = group == CZK_G1 ? 12 : 24, np = pts_stride ? n : 1;
    Staged sp{ctx}, si{ctx}, sk{ctx};
    AffineOut so(ctx);
    CZK_TRY(sp.to_device(pts, np * aw * 8, mem));
    if (inf) CZK_TRY(si.to_device(inf, np, mem));
    CZK_TRY(sk.to_device(scalars, n * 32, mem));
    CZK_TRY(so.open(group, out, out_inf, n, mem));
    CZK_TRY(points_mul_device(ctx, group, (const u64*)sp.dev, (const uint8_t*)si.dev, pts_stride, (const u64*)sk.dev, n, scalar_form, so.pts.words(),
                              so.inf.flags()));
    return so.close();
}

extern "C" int czk_points_sum(czk_ctx* ctx, int group, const uint64_t* pts, const uint8_t* inf, const size_t* offsets, size_t k, uint64_t* out,
                              uint8_t* out_inf, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_group_mem(ctx, group, mem));
    if (!k) return CZK_OK;
    if (!offsets || !out) return set_err(ctx, CZK_ERR_ARG, "null points_sum buffer");
    size_t n;
    CZK_TRY(check_offsets(ctx, offsets, k, &n));
    if (n && !pts) return set_err(ctx, CZK_ERR_ARG, "null points");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sp{ctx}, si{ctx};
    AffineOut so(ctx);
    CZK_TRY(sp.to_device(pts, n * (group == CZK_G1 ? 96 : 192), mem));
    if (inf) CZK_TRY(si.to_device(inf, n, mem));
    CZK_TRY(so.open(group, out, out_inf, k, mem));
    CZK_TRY(points_sum_device(ctx, group, (const u64*)sp.dev, (const uint8_t*)si.dev, offsets, k, so.pts.words(), so.inf.flags()));
    return so.close();
}
