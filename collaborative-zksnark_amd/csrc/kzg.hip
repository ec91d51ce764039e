// kzg.hip -- KZG10::check and KZG10::batch_check (poly-commit/src/kzg10/mod.rs:295-371) on gfx950.
//
// Both are compositions of calls the library already has: the group steps are point_ops.hip's elementwise kernels (czk_points_mul with one
// base for every scalar, czk_points_add, czk_points_sum), the scalar products czk_fr_vec_op, and the verdicts pairing.hip's product-of-pairings
// kernel with two pairs per verdict.  What this file adds is the verifier key (the four points in HBM, plus -beta_h), two small kernels -- the
// per-batch sums of Fr products, and the interleaving of the two pairs of each product -- and the sequencing.
//   check:        ok[i]  iff  e(C_i - [v_i] g - [rv_i] gamma_g, h) * e(W_i, [z_i] h - beta_h) == 1
//                 (the reference compares e(inner, h) with e(W, beta_h - [z] h): the same decision, the final exponentiation is a homomorphism
//                 and e(W, -Q) = e(-W, Q))
//   batch_check:  total_c = sum r_i (C_i + [z_i] W_i) - [sum r_i v_i] g - [sum r_i rv_i] gamma_g,  total_w = sum r_i W_i,
//                 ok[j]  iff  e(total_w, -beta_h) * e(total_c, h) == 1   (mod.rs:358-367 negates total_w instead of beta_h)
// As in the reference no point gets a subgroup or on-curve check, and a pair with infinity on either side is skipped by the Miller loop.
#include "call.h"
#include "tower.h"

struct czk_kzg10_vk {
    int device = 0;
    // one allocation: g (12 u64) | gamma_g (12) | h (24) | beta_h (24) | -beta_h (24)
    czk::u64* pts = nullptr;
    const czk::u64* g() const { return pts; }
    const czk::u64* gamma_g() const { return pts + 12; }
    const czk::u64* h() const { return pts + 24; }
    const czk::u64* beta_h() const { return pts + 48; }
    const czk::u64* neg_beta_h() const { return pts + 72; }
};

namespace czk {

// out[j] = sum of x[offs[j] .. offs[j + 1]) over Fr (Montgomery form in, Montgomery form out)
__global__ __launch_bounds__(128) void k_fr_segment_sum(const u64* x, const size_t* offs, size_t b, u64* out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b) return;
    Fr acc = Fr::zero();
#pragma unroll 1
    for (size_t i = offs[j]; i < offs[j + 1]; i++) acc = fp_add(acc, fp_load<FrParams>(x + 4 * i));
    fp_store<FrParams>(out + 4 * j, acc);
}

// The two pairs of product t, next to each other: g1[2t] = p[t], g1[2t + 1] = q[t]; g2[2t] = r[t * r_stride], g2[2t + 1] = s[t * s_stride]
// (a stride of 0 repeats one point, which is finite).  Flags: null = none infinite.
__global__ __launch_bounds__(128) void k_kzg_pairs(const u64* p, const uint8_t* p_inf, const u64* q, const uint8_t* q_inf, const u64* r, size_t r_stride,
                                                   const uint8_t* r_inf, const u64* s, size_t s_stride, const uint8_t* s_inf, size_t k, u64* g1,
                                                   uint8_t* g1_inf, u64* g2, uint8_t* g2_inf) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    for (int w = 0; w < 12; w++) {
        g1[24 * t + w] = p[12 * t + w];
        g1[24 * t + 12 + w] = q[12 * t + w];
    }
    const size_t ir = r_stride ? t : 0, is = s_stride ? t : 0;
    for (int w = 0; w < 24; w++) {
        g2[48 * t + w] = r[24 * ir + w];
        g2[48 * t + 24 + w] = s[24 * is + w];
    }
    g1_inf[2 * t] = p_inf ? p_inf[t] : 0;
    g1_inf[2 * t + 1] = q_inf ? q_inf[t] : 0;
    g2_inf[2 * t] = r_inf ? r_inf[ir] : 0;
    g2_inf[2 * t + 1] = s_inf ? s_inf[is] : 0;
}

// the per-opening arrays of both calls, staged into HBM for host callers
struct KzgIn {
    Staged comm, comm_inf, points, values, w, w_inf, random_v;
    explicit KzgIn(czk_ctx* c) : comm{c}, comm_inf{c}, points{c}, values{c}, w{c}, w_inf{c}, random_v{c} {}
    int open(const uint64_t* c, const uint8_t* ci, const uint64_t* z, const uint64_t* v, const uint64_t* ww, const uint8_t* wi, const uint64_t* rv, size_t k,
             int mem) {
        CZK_TRY(comm.to_device(c, k * 96, mem));
        if (ci) CZK_TRY(comm_inf.to_device(ci, k, mem));
        CZK_TRY(points.to_device(z, k * 32, mem));
        CZK_TRY(values.to_device(v, k * 32, mem));
        CZK_TRY(w.to_device(ww, k * 96, mem));
        if (wi) CZK_TRY(w_inf.to_device(wi, k, mem));
        if (rv) CZK_TRY(random_v.to_device(rv, k * 32, mem));
        return CZK_OK;
    }
};

// verdicts of k products of two pairs each: (p, r) and (q, s)
static int two_pair_verdicts(czk_ctx* ctx, CallMem& bufs, const u64* p, const uint8_t* p_inf, const u64* q, const uint8_t* q_inf, const u64* r,
                             size_t r_stride, const uint8_t* r_inf, const u64* s, size_t s_stride, const uint8_t* s_inf, size_t k, uint8_t* out_ok, int mem) {
    u64 *g1, *g2;
    uint8_t *g1i, *g2i;
    CallOut ok(ctx);
    CZK_TRY(bufs.points(CZK_G1, &g1, &g1i, 2 * k));
    CZK_TRY(bufs.points(CZK_G2, &g2, &g2i, 2 * k));
    CZK_TRY(ok.open(out_ok, k, mem, &bufs));
    hipLaunchKernelGGL(k_kzg_pairs, grid_for(k), dim3(128), 0, ctx->stream, p, p_inf, q, q_inf, r, r_stride, r_inf, s, s_stride, s_inf, k,
                       g1, g1i, g2, g2i);
    CZK_HIP(ctx, hipGetLastError());
    std::vector<size_t> offs(k + 1);
    for (size_t t = 0; t <= k; t++) offs[t] = 2 * t;
    CZK_TRY(pairing_is_one_device(ctx, g1, g1i, g2, g2i, offs.data(), k, ok.flags()));   // (blocks: every buffer of the call is idle afterwards)
    return ok.close();
}

static int kzg_args(czk_ctx* ctx, const czk_kzg10_vk* vk, int mem) {
    if (!vk) return set_err(ctx, CZK_ERR_ARG, "null verifier key");
    CZK_TRY(check_mem(ctx, mem));
    return check_device(ctx, vk->device, "verifier key lives on another device");
}

}  // namespace czk

using namespace czk;

extern "C" void czk_kzg10_vk_release(czk_kzg10_vk* vk) {
    if (!vk) return;
    (void)hipSetDevice(vk->device);
    if (vk->pts) (void)hipFree(vk->pts);
    delete vk;
}

extern "C" int czk_kzg10_vk_create(czk_ctx* ctx, const uint64_t* g, const uint64_t* gamma_g, const uint64_t* h, const uint64_t* beta_h, czk_kzg10_vk** out) {
    if (!ctx || !out) return CZK_ERR_ARG;
    *out = nullptr;
    if (!g || !gamma_g || !h || !beta_h) return set_err(ctx, CZK_ERR_ARG, "null verifier key point");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    u64 host[96];
    for (int i = 0; i < 12; i++) host[i] = g[i], host[12 + i] = gamma_g[i];
    for (int i = 0; i < 24; i++) host[24 + i] = h[i], host[48 + i] = beta_h[i];
    for (int i = 0; i < 12; i++) host[72 + i] = beta_h[i];
    fq2_store_strided(host + 84, 1, f_neg(fq2_load_strided(beta_h + 12, 1)));   // Neg: (x, -y)
    czk_kzg10_vk* vk = new czk_kzg10_vk();
    vk->device = ctx->device;
    hipError_t e = hipMalloc(&vk->pts, sizeof(host));
    if (e == hipSuccess) e = hipMemcpy(vk->pts, host, sizeof(host), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        czk_kzg10_vk_release(vk);
        return set_err(ctx, e == hipErrorOutOfMemory ? CZK_ERR_NOMEM : CZK_ERR_HIP, std::string("verifier key upload: ") + hipGetErrorString(e));
    }
    *out = vk;
    return CZK_OK;
}

extern "C" int czk_kzg10_check(czk_ctx* ctx, const czk_kzg10_vk* vk, const uint64_t* comm, const uint8_t* comm_inf, const uint64_t* points,
                               const uint64_t* values, const uint64_t* w, const uint8_t* w_inf, const uint64_t* random_v, size_t k, uint8_t* out_ok, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(kzg_args(ctx, vk, mem));
    if (!k) return CZK_OK;
    if (!comm || !points || !values || !w || !out_ok) return set_err(ctx, CZK_ERR_ARG, "null opening argument");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CallMem bufs(ctx, "KZG10 workspace");
    KzgIn in(ctx);
    CZK_TRY(in.open(comm, comm_inf, points, values, w, w_inf, random_v, k, mem));
    u64 *t, *inner, *zh, *q;
    uint8_t *ti, *inner_i, *zhi, *qi;
    CZK_TRY(bufs.points(CZK_G1, &t, &ti, k));
    CZK_TRY(bufs.points(CZK_G1, &inner, &inner_i, k));
    CZK_TRY(bufs.points(CZK_G2, &zh, &zhi, k));
    CZK_TRY(bufs.points(CZK_G2, &q, &qi, k));
    const int mont = CZK_SCALAR_MONTGOMERY;
    // inner = C - [v] g - [rv] gamma_g  (mod.rs:303-306)
    CZK_TRY(points_mul_device(ctx, CZK_G1, vk->g(), nullptr, 0, (const u64*)in.values.dev, k, mont, t, ti));
    CZK_TRY(points_add_device(ctx, CZK_G1, (const u64*)in.comm.dev, (const uint8_t*)in.comm_inf.dev, 1, t, ti, 1, k, 1, inner, inner_i));
    if (random_v) {
        CZK_TRY(points_mul_device(ctx, CZK_G1, vk->gamma_g(), nullptr, 0, (const u64*)in.random_v.dev, k, mont, t, ti));
        CZK_TRY(points_add_device(ctx, CZK_G1, inner, inner_i, 1, t, ti, 1, k, 1, inner, inner_i));
    }
    // [z] h - beta_h  (:309, negated)
    CZK_TRY(points_mul_device(ctx, CZK_G2, vk->h(), nullptr, 0, (const u64*)in.points.dev, k, mont, zh, zhi));
    CZK_TRY(points_add_device(ctx, CZK_G2, zh, zhi, 1, vk->beta_h(), nullptr, 0, k, 1, q, qi));
    return two_pair_verdicts(ctx, bufs, inner, inner_i, (const u64*)in.w.dev, (const uint8_t*)in.w_inf.dev, vk->h(), 0, nullptr, q, 1, qi, k, out_ok, mem);
}

extern "C" int czk_kzg10_batch_check(czk_ctx* ctx, const czk_kzg10_vk* vk, const uint64_t* comm, const uint8_t* comm_inf, const uint64_t* points,
                                     const uint64_t* values, const uint64_t* w, const uint8_t* w_inf, const uint64_t* random_v, const uint64_t* randomizers,
                                     const size_t* offsets, size_t b, uint8_t* out_ok, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(kzg_args(ctx, vk, mem));
    if (!b) return CZK_OK;
    if (!offsets || !out_ok) return set_err(ctx, CZK_ERR_ARG, "null batch argument");
    size_t k;
    CZK_TRY(check_offsets(ctx, offsets, b, &k));
    if (k && (!comm || !points || !values || !w || !randomizers)) return set_err(ctx, CZK_ERR_ARG, "null opening argument");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CallMem bufs(ctx, "KZG10 workspace");
    KzgIn in(ctx);
    Staged sr{ctx};
    CZK_TRY(in.open(comm, comm_inf, points, values, w, w_inf, random_v, k, mem));
    CZK_TRY(sr.to_device(randomizers, k * 32, mem));
    u64 *t, *rc, *rw, *tc, *tw, *gs, *rm, *prod, *mult;
    uint8_t *ti, *rci, *rwi, *tci, *twi, *gsi;
    size_t* offs;
    CZK_TRY(bufs.points(CZK_G1, &t, &ti, k));
    CZK_TRY(bufs.points(CZK_G1, &rc, &rci, k));
    CZK_TRY(bufs.points(CZK_G1, &rw, &rwi, k));
    CZK_TRY(bufs.points(CZK_G1, &tc, &tci, b));
    CZK_TRY(bufs.points(CZK_G1, &tw, &twi, b));
    CZK_TRY(bufs.points(CZK_G1, &gs, &gsi, b));
    CZK_TRY(bufs.get(&rm, k * 32));
    CZK_TRY(bufs.get(&prod, k * 32));
    CZK_TRY(bufs.get(&mult, b * 32));
    CZK_TRY(bufs.get(&offs, (b + 1) * sizeof(size_t)));
    CZK_HIP(ctx, hipMemcpyAsync(offs, offsets, (b + 1) * sizeof(size_t), hipMemcpyHostToDevice, ctx->stream));
    const u64 *dw = (const u64*)in.w.dev, *dr = (const u64*)sr.dev;
    const uint8_t* dwi = (const uint8_t*)in.w_inf.dev;
    // r_i (C_i + [z_i] W_i) and r_i W_i  (mod.rs:339-348), then their sums per batch
    CZK_TRY(points_mul_device(ctx, CZK_G1, dw, dwi, 1, (const u64*)in.points.dev, k, CZK_SCALAR_MONTGOMERY, t, ti));
    CZK_TRY(points_add_device(ctx, CZK_G1, (const u64*)in.comm.dev, (const uint8_t*)in.comm_inf.dev, 1, t, ti, 1, k, 0, t, ti));
    CZK_TRY(points_mul_device(ctx, CZK_G1, t, ti, 1, dr, k, CZK_SCALAR_CANONICAL, rc, rci));
    CZK_TRY(points_mul_device(ctx, CZK_G1, dw, dwi, 1, dr, k, CZK_SCALAR_CANONICAL, rw, rwi));
    CZK_TRY(points_sum_device(ctx, CZK_G1, rc, rci, offsets, b, tc, tci));
    CZK_TRY(points_sum_device(ctx, CZK_G1, rw, rwi, offsets, b, tw, twi));
    // total_c -= [sum r_i v_i] g, -= [sum r_i rv_i] gamma_g  (:343-346, :353-354)
    if (k) CZK_TRY(czk_fr_from_repr(ctx, dr, rm, k, CZK_MEM_DEVICE));
    for (int pass = 0; pass < (random_v ? 2 : 1); pass++) {
        const u64* x = (const u64*)(pass ? in.random_v.dev : in.values.dev);
        if (k) CZK_TRY(czk_fr_vec_op(ctx, CZK_OP_MUL, rm, x, prod, k, CZK_MEM_DEVICE));
        hipLaunchKernelGGL(k_fr_segment_sum, grid_for(b), dim3(128), 0, ctx->stream, (const u64*)prod, (const size_t*)offs, b, mult);
        CZK_HIP(ctx, hipGetLastError());
        CZK_TRY(points_mul_device(ctx, CZK_G1, pass ? vk->gamma_g() : vk->g(), nullptr, 0, mult, b, CZK_SCALAR_MONTGOMERY, gs, gsi));
        CZK_TRY(points_add_device(ctx, CZK_G1, tc, tci, 1, gs, gsi, 1, b, 1, tc, tci));
    }
    return two_pair_verdicts(ctx, bufs, tw, twi, tc, tci, vk->neg_beta_h(), 0, nullptr, vk->h(), 0, nullptr, b, out_ok, mem);
}
