// fixed_base.hip -- windowed fixed-base scalar multiplication over BLS12-377 G1 / G2 for gfx950.
//
// Replaces FixedBaseMSM::{get_window_table, windowed_mul, multi_scalar_mul} (algebra/ec/src/msm/fixed_base.rs:12-96) as the reference's
// Groth16 generator uses them (groth16/src/generator.rs:106-187): one table of multiples of ONE base P, then [k_i] P for n scalars with one
// mixed addition per window, normalised to affine (batch_normalization_into_affine, short_weierstrass_jacobian.rs:480-500).  The result is
// the same group element whatever the window width, so the layout is the library's own:
//   * table, resident in HBM:  T[j][d - 1] = d * 2^(w j) * P  for  d = 1 .. H = 2^(w - 1),  j < windows, affine + one infinity byte per entry
//     (an entry IS infinity when P has small order: the base may be any finite curve point, fixed_base.rs makes no subgroup assumption).
//   * signed digits: a window value v > H becomes v - 2^w with a carry into the next window, and adds -T (y -> q - y): half the
//     reference's 2^w entries per window.  windows = ceil(253 / w), plus one where w divides 253 (w = 1, 11): only there is the top window
//     full, so that its carry can leave it (k = r - 1 at w = 11 does).
//   * built on the device: window bases 2^(w j) P by doubling (one thread each), normalised; then one thread per chunk of 32 consecutive
//     multiples -- the chunk's first entry by double-and-add, the rest by a running mixed addition of the window base -- and ONE batched
//     normalisation of the whole table (msm_bases.hip's k_batch_to_affine through launch_batch_to_affine).
//   * multiply: one thread per scalar, Jacobian accumulator, curve.h's complete jac_add_mixed (P = +-Q and infinity included) -- not the
//     twisted Edwards path, which is exact in the subgroup only.  Scalars are decoded from Montgomery form on the fly; bits at and above
//     253 are ignored (fixed_base.rs:72).
// All arithmetic is the 32-bit-limb integer VALU code of field.h / curve.h.
#include "call.h"

struct czk_fixed_base {
    int device = 0;
    int group = 1;
    unsigned w = 0, windows = 0;
    size_t H = 0;               // entries per window = 2^(w - 1)
    uint64_t* pts = nullptr;    // device, windows x H x (12|24) u64 affine Montgomery
    uint8_t* inf = nullptr;     // device, windows x H
    size_t table_bytes = 0;
};

namespace czk {

constexpr unsigned FB_BITS = 253;        // Fr::size_in_bits(), the generator's scalar_bits (generator.rs:87)
constexpr unsigned FB_CHUNK = 32;        // consecutive multiples per thread of the table build
constexpr size_t FB_TABLE_CAP = (size_t)1 << 30;   // the automatic rule never picks a table above 1 GiB
constexpr size_t FB_DEFAULT_HINT = 1024; // n_hint = 0: "not known"

static unsigned fb_windows(unsigned w) { return (FB_BITS + w - 1) / w + (FB_BITS % w == 0 ? 1u : 0u); }
static size_t fb_table_bytes(int group, unsigned w) { return (size_t)fb_windows(w) * ((size_t)1 << (w - 1)) * ((group == CZK_G1 ? 12 : 24) * 8 + 1); }

// Window rule: the width with the fewest group additions for n scalars, table build included -- n additions per window, against about 2.5 per
// table entry (a running addition, its share of the chunk's double-and-add start, and the normalisation) -- among the widths whose table
// fits FB_TABLE_CAP.
static unsigned fb_choose_window(int group, size_t n) {
    if (!n) n = FB_DEFAULT_HINT;
    unsigned best = 1;
    double best_cost = 0;
    for (unsigned w = 1; w <= 20; w++) {
        if (w > 1 && fb_table_bytes(group, w) > FB_TABLE_CAP) break;
        const double W = fb_windows(w), cost = W * (double)n + 2.5 * W * (double)((size_t)1 << (w - 1));
        if (w == 1 || cost < best_cost) {
            best = w;
            best_cost = cost;
        }
    }
    return best;
}

// out[j] = 2^(w j) * base (Jacobian), j < windows
template <class F>
__global__ __launch_bounds__(128) void k_fb_window_bases(const u64* base_aff, unsigned w, unsigned windows, u64* out_jac) {
    unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= windows) return;
    Affine<F> a = aff_load<F>(base_aff);
    Jac<F> p{a.x, a.y, F::one()};
    for (unsigned k = 0; k < w * j; k++) p = jac_double(p);
    jac_store<F>(out_jac + (size_t)GT<F>::JW * j, p);
}

// out[j H + d - 1] = d * B_j (Jacobian) for the chunk d = c FB_CHUNK + 1 .. min((c + 1) FB_CHUNK, H) of window j
template <class F>
__global__ __launch_bounds__(128) void k_fb_table(const u64* win_aff, const uint8_t* win_inf, unsigned windows, size_t H, size_t chunks, u64* out_jac) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)windows * chunks) return;
    const size_t j = t / chunks, d0 = (t % chunks) * FB_CHUNK + 1;
    const Affine<F> q = aff_load<F>(win_aff + (size_t)GT<F>::AW * j);
    const bool q_inf = win_inf[j] != 0;
    Jac<F> s = Jac<F>::zero();
    for (int b = 20; b >= 0; b--) {   // d0 <= H <= 2^19
        s = jac_double(s);
        if ((d0 >> b) & 1) s = jac_add_mixed(s, q, q_inf);
    }
    u64* o = out_jac + (size_t)GT<F>::JW * (j * H + d0 - 1);
    jac_store<F>(o, s);
    for (size_t k = 1; k < FB_CHUNK && d0 + k <= H; k++) {
        s = jac_add_mixed(s, q, q_inf);
        jac_store<F>(o + (size_t)GT<F>::JW * k, s);
    }
}

// out[i] = [k_i] P (Jacobian): one signed digit and at most one mixed addition per window
template <class F>
__global__ __launch_bounds__(128) void k_fb_mul(const u64* table, const uint8_t* tinf, const u64* scalars, size_t n, int montgomery, unsigned w,
                                                unsigned windows, u64* out_jac) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = fp_load<FrParams>(scalars + 4 * i);
    if (montgomery) s = fp_into_repr(s);   // ec/src/lib.rs:305-307
    s.l[7] &= 0x1fffffffu;                 // bits >= 253 are not read (fixed_base.rs:72)
    const u32 H = 1u << (w - 1), mask = (1u << w) - 1u;
    Jac<F> acc = Jac<F>::zero();
    u32 carry = 0;
    for (unsigned j = 0; j < windows; j++) {
        const unsigned bit = j * w;
        u32 v = carry;
        if (bit < FB_BITS) {
            const unsigned limb = bit >> 5, off = bit & 31;
            const u64 two = (u64)s.l[limb] | (limb + 1 < 8 ? (u64)s.l[limb + 1] << 32 : 0);
            v += (u32)(two >> off) & mask;
        }
        const bool neg = v > H;
        const u32 d = neg ? (1u << w) - v : v;
        carry = neg ? 1u : 0u;
        if (!d) continue;
        const size_t e = (size_t)j * H + d - 1;
        if (tinf[e]) continue;             // add_assign_mixed skips infinity (short_weierstrass_jacobian.rs:571-573)
        Affine<F> q = aff_load<F>(table + (size_t)GT<F>::AW * e);
        if (neg) q.y = f_neg(q.y);
        acc = jac_add_mixed(acc, q, false);
    }
    jac_store<F>(out_jac + (size_t)GT<F>::JW * i, acc);
}

template <class F>
static int fb_build(czk_ctx* ctx, czk_fixed_base* fb, const u64* base_host) {
    constexpr int AW = GT<F>::AW, JW = GT<F>::JW, FW = GT<F>::FW;
    const unsigned W = fb->windows;
    const size_t H = fb->H, E = (size_t)W * H, chunks = (H + FB_CHUNK - 1) / FB_CHUNK;
    if (hipMalloc(&fb->pts, E * AW * 8) != hipSuccess || hipMalloc(&fb->inf, E) != hipSuccess)
        return set_err(ctx, CZK_ERR_NOMEM, "hipMalloc fixed-base table");
    // workspace: the base, the window bases (Jacobian, affine, flags), the table in Jacobian form and the normalisation's scratch
    const size_t o_base = 0, o_wjac = o_base + AW * 8, o_waff = o_wjac + (size_t)W * JW * 8, o_jac = o_waff + (size_t)W * AW * 8,
                 o_scr = o_jac + E * JW * 8, o_winf = o_scr + E * FW * 8, total = o_winf + W;
    char* p = nullptr;   // (used once: not taken from the staging pool, which would keep it)
    if (hipMalloc(&p, total) != hipSuccess) return set_err(ctx, CZK_ERR_NOMEM, "hipMalloc fixed-base table workspace");
    hipError_t e = hipMemcpyAsync(p + o_base, base_host, AW * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        ProfScope ps(ctx, "fixed_base_table");
        hipLaunchKernelGGL(k_fb_window_bases<F>, grid_for(W), dim3(128), 0, ctx->stream, (const u64*)(p + o_base), fb->w, W, (u64*)(p + o_wjac));
        launch_batch_to_affine(ctx->stream, fb->group, (const u64*)(p + o_wjac), W, (u64*)(p + o_scr), (u64*)(p + o_waff), (uint8_t*)(p + o_winf));
        hipLaunchKernelGGL(k_fb_table<F>, grid_for((size_t)W * chunks), dim3(128), 0, ctx->stream, (const u64*)(p + o_waff),
                           (const uint8_t*)(p + o_winf), W, H, chunks, (u64*)(p + o_jac));
        launch_batch_to_affine(ctx->stream, fb->group, (const u64*)(p + o_jac), E, (u64*)(p + o_scr), fb->pts, fb->inf);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (base_host has been read; the handle is complete on return)
    (void)hipFree(p);
    if (e != hipSuccess) return set_err(ctx, CZK_ERR_HIP, std::string("fixed-base table: ") + hipGetErrorString(e));
    return CZK_OK;
}

}  // namespace czk

using namespace czk;

extern "C" int czk_fixed_base_create(czk_ctx* ctx, int group, const uint64_t* base_aff, unsigned window, size_t n_hint, czk_fixed_base** out) {
    if (!ctx || !out) return ctx ? set_err(ctx, CZK_ERR_ARG, "null fixed_base_create argument") : CZK_ERR_ARG;
    *out = nullptr;
    CZK_TRY(check_group(ctx, group));
    if (!base_aff) return set_err(ctx, CZK_ERR_ARG, "null base");
    if (window > 20) return set_err(ctx, CZK_ERR_ARG, "window must be 0 (chosen by the library) or 1..20");
    // the base is ONE finite point: x = 0 with y = 0 or y = 1 is how this ABI's affine arrays write the point at infinity
    const size_t fw = group == CZK_G1 ? 6 : 12;
    bool x_zero = true, y_rest_zero = true;
    for (size_t i = 0; i < fw; i++) x_zero = x_zero && base_aff[i] == 0;
    for (size_t i = 6; i < fw; i++) y_rest_zero = y_rest_zero && base_aff[fw + i] == 0;
    if (x_zero && y_rest_zero) {
        const Fq one = Fq::one();
        bool y_zero = true, y_one = true;
        for (size_t i = 0; i < 6; i++) {
            y_zero = y_zero && base_aff[fw + i] == 0;
            y_one = y_one && base_aff[fw + i] == ((u64)one.l[2 * i] | (u64)one.l[2 * i + 1] << 32);
        }
        if (y_zero || y_one) return set_err(ctx, CZK_ERR_ARG, "the base is the point at infinity");
    }
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    czk_fixed_base* fb = new czk_fixed_base();
    fb->device = ctx->device;
    fb->group = group;
    fb->w = window ? window : fb_choose_window(group, n_hint);
    fb->windows = fb_windows(fb->w);
    fb->H = (size_t)1 << (fb->w - 1);
    fb->table_bytes = fb_table_bytes(group, fb->w);
    int rc = group == CZK_G1 ? fb_build<Fq>(ctx, fb, base_aff) : fb_build<Fq2>(ctx, fb, base_aff);
    if (rc != CZK_OK) {
        czk_fixed_base_release(fb);
        return rc;
    }
    *out = fb;
    return CZK_OK;
}

extern "C" void czk_fixed_base_release(czk_fixed_base* fb) {
    if (!fb) return;
    (void)hipSetDevice(fb->device);
    if (fb->pts) (void)hipFree(fb->pts);
    if (fb->inf) (void)hipFree(fb->inf);
    delete fb;
}

extern "C" int czk_fixed_base_layout(const czk_fixed_base* fb, unsigned* window, unsigned* windows, size_t* table_bytes) {
    if (!fb) return CZK_ERR_ARG;
    if (window) *window = fb->w;
    if (windows) *windows = fb->windows;
    if (table_bytes) *table_bytes = fb->table_bytes;
    return CZK_OK;
}

extern "C" int czk_fixed_base_msm(czk_ctx* ctx, const czk_fixed_base* fb, const uint64_t* scalars, size_t n, int scalar_form, uint64_t* out_aff,
                                  uint8_t* out_inf, int mem) {
    if (!ctx || !fb) return ctx ? set_err(ctx, CZK_ERR_ARG, "null fixed_base_msm argument") : CZK_ERR_ARG;
    if (n && (!scalars || !out_aff)) return set_err(ctx, CZK_ERR_ARG, "null fixed_base_msm buffer");
    CZK_TRY(check_scalar_form(ctx, scalar_form));
    CZK_TRY(check_mem(ctx, mem));
    CZK_TRY(check_device(ctx, fb->device, "the fixed-base table lives on another device"));
    if (!n) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sk{ctx};
    AffineOut so(ctx);
    CZK_TRY(sk.to_device(scalars, n * 32, mem));
    CZK_TRY(so.open(fb->group, out_aff, out_inf, n, mem));
    CZK_TRY(launch_to_affine(ctx, "fixed_base_msm", "fixed-base msm", fb->group, n, so.pts.words(), so.inf.flags(), [&](auto tag, u64* jac) {
        hipLaunchKernelGGL(k_fb_mul<typename decltype(tag)::type>, grid_for(n), dim3(128), 0, ctx->stream, (const u64*)fb->pts, (const uint8_t*)fb->inf,
                           (const u64*)sk.dev, n, scalar_form == CZK_SCALAR_MONTGOMERY ? 1 : 0, fb->w, fb->windows, jac);
    }));
    return so.close();
}
