// msm_bases.hip -- everything about an MSM key (czk_bases; the pipeline that runs an MSM over one is msm.hip): generators and fixed-base points, registration with
// its window tables, the subgroup check, the secondary table sets of short calls and the rules that choose a window width.
#include "czk_internal.h"

namespace czk {

// curves/bls12_377/src/curves/g1.rs:46-51, g2.rs:64-86 generators, Montgomery form, 32-bit limbs
__device__ __forceinline__ Affine<Fq> generator(Fq*) {
    const u32 gx[12] = {0x772451f4u, 0x260f33b9u, 0x169d5658u, 0xc54dd773u, 0x69a510ddu, 0x5c1551c4u,
                        0x425e1698u, 0x761662e4u, 0x6f065272u, 0xc97d78ccu, 0xb361fd4du, 0x00a41206u};
    const u32 gy[12] = {0xb8cb81f3u, 0x8193961fu, 0x5f44adb8u, 0x00638d4cu, 0xd4daf54au, 0xfafaf3dau,
                        0xd655cd18u, 0xc27849e2u, 0x01d52814u, 0x2ec3ddb4u, 0x26303c71u, 0x007da933u};
    Affine<Fq> g;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        g.x.l[i] = gx[i];
        g.y.l[i] = gy[i];
    }
    return g;
}
__device__ __forceinline__ Affine<Fq2> generator(Fq2*) {
    const u32 x0[12] = {0xf268725bu, 0x68904082u, 0x4f45328bu, 0x668f2ea7u, 0x802be84fu, 0xebca7a65u,
                        0xc1ada3e6u, 0x1e1850f4u, 0x588ef1e9u, 0x830dc22du, 0x767c0982u, 0x01862a81u};
    const u32 x1[12] = {0xc91c7f39u, 0x5f02a915u, 0x388da2a7u, 0xf8c553bau, 0xbd198850u, 0xd51a416du,
                        0x8ae3073au, 0xe943c6f3u, 0x259a4981u, 0xffe24aa8u, 0x1e73dfddu, 0x01185339u};
    const u32 y0[12] = {0x7881430fu, 0xd5b19b89u, 0xa5b371edu, 0x05be9118u, 0x86c131eeu, 0x6063f91fu,
                        0xe8f4ec19u, 0x3244a61bu, 0x9f9a3a12u, 0xa02e425bu, 0x4f3360d2u, 0x018af8c0u};
    const u32 y1[12] = {0x1a5b96f5u, 0x57601ac7u, 0x14f2440eu, 0xe99acc17u, 0x10118ea9u, 0x2339612fu,
                        0x3b1cd722u, 0x8321e68au, 0x0cc74917u, 0x2b543b05u, 0xb396c112u, 0x00590182u};
    Affine<Fq2> g;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        g.x.c0.l[i] = x0[i];
        g.x.c1.l[i] = x1[i];
        g.y.c0.l[i] = y0[i];
        g.y.c1.l[i] = y1[i];
    }
    return g;
}

// ------------------------------------------------------------------------------------------------
// setup kernels: fixed-base points, window multiples, batched Jacobian -> affine
// ------------------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(128) void k_fixed_base(const u64* k, size_t n, u64* out_jac) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> g = generator((F*)nullptr);
    Jac<F> acc = Jac<F>::zero();
    for (int limb = 3; limb >= 0; limb--) {
        u64 w = k[4 * i + limb];
        for (int b = 63; b >= 0; b--) {
            acc = jac_double(acc);
            if ((w >> b) & 1) acc = jac_add_mixed(acc, g, false);
        }
    }
    jac_store<F>(out_jac + (size_t)GT<F>::JW * i, acc);
}

// out = 2^c * in   (in affine + infinity flag, out Jacobian)
template <class F>
__global__ __launch_bounds__(128) void k_dbl_c(const u64* aff, const uint8_t* inf, size_t n, unsigned c, u64* out_jac) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Jac<F> p;
    if (inf[i]) {
        p = Jac<F>::zero();
    } else {
        Affine<F> a = aff_load<F>(aff + (size_t)GT<F>::AW * i);
        p = Jac<F>{a.x, a.y, F::one()};
        for (unsigned k = 0; k < c; k++) p = jac_double(p);
    }
    jac_store<F>(out_jac + (size_t)GT<F>::JW * i, p);
}

// Montgomery's trick over CH consecutive points per thread (one field inversion per CH points).
// scratch: n field elements.
template <class F>
__global__ __launch_bounds__(128) void k_batch_to_affine(const u64* jac, size_t n, unsigned CH, u64* scratch, u64* out_aff,
                                                        uint8_t* out_inf) {
    constexpr int JW = GT<F>::JW, AW = GT<F>::AW, FW = GT<F>::FW;
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t start = t * CH;
    if (start >= n) return;
    size_t end = start + CH < n ? start + CH : n;
    F acc = F::one();
    for (size_t i = start; i < end; i++) {
        F z = FieldIO<F>::load(jac + JW * i + 2 * FW);
        FieldIO<F>::store(scratch + FW * i, acc);
        if (!z.is_zero()) acc = f_mul(acc, z);
    }
    F inv = f_inv(acc);
    for (size_t i = end; i-- > start;) {
        F z = FieldIO<F>::load(jac + JW * i + 2 * FW);
        Affine<F> a;
        if (z.is_zero()) {
            a.x = F::zero();
            a.y = F::one();
            out_inf[i] = 1;
        } else {
            F zinv = f_mul(inv, FieldIO<F>::load(scratch + FW * i));
            inv = f_mul(inv, z);
            F zi2 = f_sqr(zinv);
            a.x = f_mul(FieldIO<F>::load(jac + JW * i), zi2);
            a.y = f_mul(FieldIO<F>::load(jac + JW * i + FW), f_mul(zi2, zinv));
            out_inf[i] = 0;
        }
        aff_store<F>(out_aff + (size_t)AW * i, a);
    }
}

// k_batch_to_affine for every caller (here and fixed_base.hip): n Jacobian points -> affine + infinity flags; scratch: n field elements
void launch_batch_to_affine(hipStream_t st, int group, const u64* jac, size_t n, u64* scratch, u64* out_aff, uint8_t* out_inf) {
    if (!n) return;
    const unsigned CH = 32;
    const dim3 grid((unsigned)(((n + CH - 1) / CH + 127) / 128));
    if (group == CZK_G1) hipLaunchKernelGGL(k_batch_to_affine<Fq>, grid, dim3(128), 0, st, jac, n, CH, scratch, out_aff, out_inf);
    else hipLaunchKernelGGL(k_batch_to_affine<Fq2>, grid, dim3(128), 0, st, jac, n, CH, scratch, out_aff, out_inf);
}

// window tables 1 .. W - 1 of n points each: table w = 2^(width of window w - 1) times table w - 1.  jac / scr: n Jacobian points / n field elements
template <class F>
static void build_windows(hipStream_t st, u64* pts, uint8_t* inf, size_t n, unsigned c, unsigned W, u64* jac, u64* scr) {
    constexpr int AW = GT<F>::AW;
    for (unsigned w = 1; w < W; w++) {
        hipLaunchKernelGGL(k_dbl_c<F>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, pts + (size_t)(w - 1) * n * AW, inf + (size_t)(w - 1) * n, n,
                           msm_win_width(c, msm_full_windows(c), w - 1), jac);
        launch_batch_to_affine(st, AW == 12 ? CZK_G1 : CZK_G2, jac, n, scr, pts + (size_t)w * n * AW, inf + (size_t)w * n);
    }
}

int fixed_base_points_device(czk_ctx* ctx, int group, const u64* k_dev, size_t n, u64* out_dev) {
    const size_t JW = group == CZK_G1 ? GT<Fq>::JW : GT<Fq2>::JW, FW = group == CZK_G1 ? GT<Fq>::FW : GT<Fq2>::FW;
    if (!n) return CZK_OK;
    u64 *jac = nullptr, *scr = nullptr;
    uint8_t* inf = nullptr;
    CZK_HIP(ctx, hipMalloc(&jac, n * JW * 8));
    CZK_HIP(ctx, hipMalloc(&scr, n * FW * 8));
    CZK_HIP(ctx, hipMalloc(&inf, n));
    const dim3 grid((unsigned)((n + 127) / 128));
    if (group == CZK_G1) hipLaunchKernelGGL(k_fixed_base<Fq>, grid, dim3(128), 0, ctx->stream, k_dev, n, jac);
    else hipLaunchKernelGGL(k_fixed_base<Fq2>, grid, dim3(128), 0, ctx->stream, k_dev, n, jac);
    launch_batch_to_affine(ctx->stream, group, jac, n, scr, out_dev, inf);
    CZK_HIP(ctx, hipGetLastError());
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CZK_HIP(ctx, hipFree(jac));
    CZK_HIP(ctx, hipFree(scr));
    CZK_HIP(ctx, hipFree(inf));
    return CZK_OK;
}

// window width for n bases: minimise W(c) * n mixed additions + ~3 * 2^(c-1) reduction additions.  (In instruction terms
// a bucket costs ~6 mixed additions to reduce, but weighting it so -- c = 17 at n = 2^20 -- lengthens the accumulate kernels,
// which are the critical stream of the pipeline: measured 98 -> 102 ms per proof.)  Widths whose TOP window is only a few
// bits wide are skipped for large n: its digits pile n / 2^t points onto each of ~2^t buckets, and a bucket is one thread's
// serial chain (c = 19: 7 top bits -> 37 buckets of 28 k points at n = 2^20).
static unsigned choose_c(size_t n) {
    unsigned best = 2;
    double best_cost = 1e300;
    for (unsigned c = 2; c <= 22; c++) {
        const unsigned W = msm_num_windows(c), top_bits = 254 - (W - 1) * c;
        if (n >= 16384 && top_bits < 10) continue;
        double cost = (double)W * (double)(n ? n : 1) + 3.0 * (double)((size_t)1 << (c - 1));
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}

// Without window tables every window has its own bucket set: W(c) * n mixed additions + W(c) bucket reductions of 2^(c-1) buckets
// (~4 mixed additions' worth of instructions per bucket).  The per-window partition histograms of k_digits_part must fit its LDS array.
static unsigned choose_c_split(size_t n) {
    unsigned best = 2;
    double best_cost = 1e300;
    for (unsigned c = 2; c <= 20; c++) {
        const unsigned W = msm_num_windows(c), top_bits = 254 - (W - 1) * c;
        const size_t B = (size_t)1 << (c - 1), n_parts = (B + PART_BUCKETS - 1) >> PART_LOG;
        if ((size_t)W * n_parts > MAX_PARTS) continue;
        if (n >= 16384 && top_bits < 10) continue;   // a narrow top window piles n / 2^bits points on each of its few buckets
        double cost = (double)W * (double)(n ? n : 1) + 4.0 * (double)W * (double)B;
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}

// G1 in twisted Edwards form (te.h): a saturated short-Weierstrass table of `count` points -> a freshly allocated niels table
// (count x 24 u64: three coordinates of 14 x 28-bit limbs in 16 u32 each).  *ok = false (and no table) when some point has no image under the map -- such a point has even order
// and is never an element of G1; the caller then keeps the XYZZ path, which is complete on all of E.
// runs `launch(counter)` on `st` with a zeroed device counter and reads the counter back (blocking)
template <class Launch>
static hipError_t count_bad(hipStream_t st, u32* out, Launch launch) {
    u32* bad = nullptr;
    hipError_t e = hipMalloc(&bad, 4);
    if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 4, st);
    if (e == hipSuccess) {
        launch(bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, bad, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (bad) (void)hipFree(bad);
    return e;
}
static int te_table_from_sw(czk_ctx* ctx, const u64* sw, const uint8_t* inf, size_t count, u64** out, bool* ok) {
    *out = nullptr;
    *ok = false;
    u64 *te = nullptr, *scr = nullptr;
    u32 hbad = 1;
    hipError_t e = hipMalloc(&te, count * 24 * 8);
    if (e == hipSuccess) e = hipMalloc(&scr, count * 6 * 8);
    if (e == hipSuccess) e = count_bad(ctx->stream, &hbad, [&](u32* bad) { launch_sw_to_te_niels(ctx->stream, sw, inf, count, scr, te, bad); });
    if (scr) (void)hipFree(scr);
    if (e != hipSuccess || hbad) {
        if (te) (void)hipFree(te);
        if (e != hipSuccess) return set_err(ctx, e == hipErrorOutOfMemory ? CZK_ERR_NOMEM : CZK_ERR_HIP, std::string("twisted Edwards table: ") + hipGetErrorString(e));
        return CZK_OK;
    }
    *out = te;
    *ok = true;
    return CZK_OK;
}

// ------------------------------------------------------------------------------------------------
// Subgroup membership of registered bases: the reference's `is_in_correct_subgroup_assuming_on_curve` is `self.mul(r).is_zero()`
// (short_weierstrass_jacobian.rs:131), enforced when a key is deserialised (:868, :881); its MSM itself is complete on every curve point.
// The twisted Edwards G1 kernels are exception-free exactly on the prime-order subgroup, so a caller that cannot vouch for its bases asks
// for this check (czk_bases_check_subgroup, or CZK_MEM_CHECK_SUBGROUP at registration: a failing base keeps the handle on the XYZZ kernels).
// One thread per point: on-curve test (y^2 = x^3 + b), then [r] P by MSB-first double-and-add with the complete Jacobian formulas of curve.h.
// ------------------------------------------------------------------------------------------------
// (the curve constants CurveB<F> are in czk_internal.h: point_codec.hip's decoder uses them too)
template <class F>
__global__ __launch_bounds__(128) void k_subgroup_check(const u64* aff, const uint8_t* inf, size_t n, u32* bad) {
    // r = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001, 253 bits (curves/bls12_377/src/fields/fr.rs MODULUS)
    constexpr u32 R[8] = {0x00000001u, 0x0a118000u, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu};
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (inf && inf[i])) return;
    const Affine<F> a = aff_load<F>(aff + (size_t)GT<F>::AW * i);
    bool ok = f_sqr(a.y) == f_add(f_mul(f_sqr(a.x), a.x), CurveB<F>::get());
    if (ok) {
        Jac<F> p{a.x, a.y, F::one()};
        for (int bit = 251; bit >= 0; bit--) {   // bit 252 is the leading one
            p = jac_double(p);
            if ((R[bit >> 5] >> (bit & 31)) & 1u) p = jac_add_mixed(p, a, false);
        }
        ok = p.is_zero();
    }
    if (!ok) atomicAdd(bad, 1u);
}
// pts: `n` affine points in the reference's (saturated Montgomery) form, device memory
template <class F>
static int subgroup_check_impl(czk_ctx* ctx, const u64* pts, const uint8_t* inf, size_t n, size_t* out_bad) {
    *out_bad = 0;
    if (!n) return CZK_OK;
    u32 h = 0;
    hipError_t e = count_bad(ctx->stream, &h, [&](u32* bad) { hipLaunchKernelGGL(k_subgroup_check<F>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, ctx->stream, pts, inf, n, bad); });
    if (e != hipSuccess) return set_err(ctx, CZK_ERR_HIP, std::string("subgroup check: ") + hipGetErrorString(e));
    *out_bad = h;
    return CZK_OK;
}

template <class F>
static int register_impl(czk_ctx* ctx, czk_bases* b, const u64* pts_dev, const uint8_t* inf_dev) {
    constexpr int AW = GT<F>::AW, JW = GT<F>::JW, FW = GT<F>::FW;
    const size_t n = b->n;
    const unsigned W = b->split ? 1 : b->W;   // windows held as tables
    CZK_HIP(ctx, hipMalloc(&b->pts, (size_t)W * (n ? n : 1) * AW * 8));
#ifdef CZK_LAB   // keys keep saturated tables / the XYZZ kernels on request (A/B runs of the rejected variants)
    const bool keep_sat = ctx->msm_sat || (GT<F>::AW != 12 && ctx->msm_sat_g2), no_te = ctx->msm_sat || ctx->msm_no_te || ctx->msm_affine_rounds > 0;
#else
    constexpr bool keep_sat = false, no_te = false;
#endif
    CZK_HIP(ctx, hipMalloc(&b->inf, (size_t)W * (n ? n : 1)));
    if (!n) {
        b->unsat = !keep_sat;   // an empty key runs the same kernels as any other (its MSMs are the neutral element)
        return CZK_OK;
    }
    CZK_HIP(ctx, hipMemcpyAsync(b->pts, pts_dev, n * AW * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (inf_dev) CZK_HIP(ctx, hipMemcpyAsync(b->inf, inf_dev, n, hipMemcpyDeviceToDevice, ctx->stream));
    else CZK_HIP(ctx, hipMemsetAsync(b->inf, 0, n, ctx->stream));
    if (b->check_wanted) {   // CZK_MEM_CHECK_SUBGROUP: a base outside the prime-order subgroup keeps the handle on the complete XYZZ kernels
        CZK_TRY(subgroup_check_impl<F>(ctx, b->pts, b->inf, n, &b->n_bad));
        b->checked = true;
        if (b->n_bad) b->te_wanted = false;
    }
    if (W > 1) {
        u64 *jac = nullptr, *scr = nullptr;
        CZK_HIP(ctx, hipMalloc(&jac, n * JW * 8));
        CZK_HIP(ctx, hipMalloc(&scr, n * FW * 8));
        build_windows<F>(ctx->stream, b->pts, b->inf, n, b->c, W, jac, scr);
        CZK_HIP(ctx, hipGetLastError());
        CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        CZK_HIP(ctx, hipFree(jac));
        CZK_HIP(ctx, hipFree(scr));
    }
    if (GT<F>::AW == 12 && b->te_wanted && !no_te) {
        // G1 bases in the prime-order subgroup: window tables as twisted Edwards niels entries (te.h), 7M unified mixed additions
        u64* te = nullptr;
        bool ok = false;
        // The niels table is twice the size of the XYZZ table and is built while that one is still live: a key that fits as XYZZ tables may not fit
        // here.  Running out of memory is not an error -- the handle keeps the XYZZ kernels (same results, ~23 % more arithmetic per addition).
        int rc = te_table_from_sw(ctx, b->pts, b->inf, (size_t)W * n, &te, &ok);
        if (rc == CZK_ERR_NOMEM) {
            (void)hipGetLastError();
            ok = false;
        } else if (rc != CZK_OK) {
            return rc;
        }
        u64* sw0 = nullptr;   // the registered points stay (secondary table sets are built from them)
        if (ok) {
            hipError_t e = hipMalloc(&sw0, n * AW * 8);
            if (e == hipSuccess) e = hipMemcpy(sw0, b->pts, n * AW * 8, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                (void)hipFree(te);
                if (sw0) (void)hipFree(sw0);
                ok = false;
                if (e != hipErrorOutOfMemory) return set_err(ctx, CZK_ERR_HIP, std::string("registered points: ") + hipGetErrorString(e));
            }
        }
        if (ok) {
            (void)hipFree(b->pts);
            b->pts = te;
            b->pts_sw0 = sw0;
            b->te = true;
            b->unsat = true;
            return CZK_OK;
        }
    }
    if (!keep_sat) {
        // window tables go to the unsaturated residue system of fqu.h (infinity flags are unaffected); the lab build's "msm_sat" /
        // "msm_sat_g2" options keep the saturated kernels for A/B runs
        launch_convert_to_u(ctx->stream, b->pts, (size_t)W * n * (GT<F>::AW / 6));
        CZK_HIP(ctx, hipGetLastError());
        CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        b->unsat = true;
    }
    return CZK_OK;
}

// ------------------------------------------------------------------------------------------------
// window width per call.  The reference chooses c from the size of each call (variable_base.rs:21-25); with precomputed window
// multiples the width is a property of the table, so a key registered for n points carries c(n) -- and a SHORT MSM under it (a KZG
// commitment of a degree-2^18 polynomial under a 3 * 2^18-point SRS) would still reduce 2^(c(n)-1) buckets per lane: as much
// work as its whole accumulation.  HBM is plentiful, so such calls get their own, narrower table set over the prefix of the
// key they use: classes c = 13 / 15 / 17 by call size (cost model: W(c) size mixed additions + ~6 mixed additions' worth of
// instructions per bucket), covering the next power of two of the call's size, built on first use (or by czk_bases_prepare)
// and kept with the handle.  A set is only built when the model predicts >= 12 % less work than the key's own tables.
// ------------------------------------------------------------------------------------------------
constexpr double REDUCE_COST_PER_BUCKET = 6.0;   // in mixed additions (measured: profiles/r03_window_classes.txt)
static double msm_cost(unsigned c, size_t size) { return (double)msm_num_windows(c) * (double)size + REDUCE_COST_PER_BUCKET * (double)((size_t)1 << (c - 1)); }
static unsigned width_class(size_t size) { return size < 11586 ? 13u : size < 92682 ? 15u : 17u; }   // boundaries at 2^13.5, 2^16.5

// the window width an MSM of `size` pairs under `b` asks for: the call's own for a table-free key (as in the reference, variable_base.rs:21-25), else a
// narrower class than the key's when the model predicts >= 12 % less work (pick_tables then finds or builds that table set)
unsigned msm_width_for(const czk_bases* b, size_t size) {
    if (b->split) return choose_c_split(size);
    if (!b->per_call_width || size == 0) return b->c;
    const unsigned cc = width_class(size);
    return cc >= b->c || msm_cost(b->c, size) < 1.12 * msm_cost(cc, size) ? b->c : cc;
}

template <class F>
static int build_secondary(czk_ctx* ctx, const czk_bases* b, unsigned c, size_t cover, czk_table_set* out) {
    constexpr int AW = GT<F>::AW, JW = GT<F>::JW, FW = GT<F>::FW;
    const unsigned W = msm_num_windows(c);
    czk_table_set t;
    t.c = c;
    t.W = W;
    t.cover = cover;
    u64 *jac = nullptr, *scr = nullptr;
    hipError_t e = hipMalloc(&t.pts, (size_t)W * cover * AW * 8);
    if (e == hipSuccess) e = hipMalloc(&t.inf, (size_t)W * cover);
    if (e == hipSuccess) e = hipMalloc(&jac, cover * JW * 8);
    if (e == hipSuccess) e = hipMalloc(&scr, cover * FW * 8);
    if (e == hipSuccess) e = hipMemcpyAsync(t.pts, b->te ? b->pts_sw0 : b->pts, cover * AW * 8, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t.inf, b->inf, cover, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) {
        if (b->unsat && !b->te) launch_convert_from_u(ctx->stream, t.pts, cover * (AW / 6));   // the key's window 0 back to Montgomery form
        build_windows<F>(ctx->stream, t.pts, t.inf, cover, c, W, jac, scr);
        if (b->unsat && !b->te) launch_convert_to_u(ctx->stream, t.pts, (size_t)W * cover * (AW / 6));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (jac) (void)hipFree(jac);
    if (scr) (void)hipFree(scr);
    if (e == hipSuccess && b->te) {   // the key is in twisted Edwards form: so is this set (its points have images: they are the key's)
        u64* te = nullptr;
        bool ok = false;
        int rc = te_table_from_sw(ctx, t.pts, t.inf, (size_t)W * cover, &te, &ok);
        (void)hipFree(t.pts);
        t.pts = te;
        if (rc != CZK_OK || !ok) {
            if (t.inf) (void)hipFree(t.inf);
            if (te) (void)hipFree(te);
            return rc != CZK_OK ? rc : set_err(ctx, CZK_ERR_ARG, "secondary window tables: a multiple of a registered point has no twisted Edwards image");
        }
    }
    if (e != hipSuccess) {
        if (t.pts) (void)hipFree(t.pts);
        if (t.inf) (void)hipFree(t.inf);
        return set_err(ctx, e == hipErrorOutOfMemory ? CZK_ERR_NOMEM : CZK_ERR_HIP, std::string("secondary window tables: ") + hipGetErrorString(e));
    }
    *out = t;
    return CZK_OK;
}

// the table set an MSM of `size` pairs runs on (builds a secondary set when the model asks for one and none fits)
int pick_tables(czk_ctx* ctx, const czk_bases* cb, size_t size, czk_table_set* tv, bool build) {
    czk_bases* b = const_cast<czk_bases*>(cb);   // the secondary sets are a cache behind the const handle
    *tv = czk_table_set{b->c, b->W, b->n, b->pts, b->inf};   // the key's own tables, seen as a set that covers all of it
    if (b->split) return CZK_OK;
    const unsigned cc = msm_width_for(b, size);
    if (cc == b->c) return CZK_OK;
    auto find = [&]() -> const czk_table_set* {
        const int n = b->n_extra.load(std::memory_order_acquire);
        const czk_table_set* best = nullptr;
        for (int i = 0; i < n; i++)
            if (b->extra[i].c == cc && b->extra[i].cover >= size && (!best || b->extra[i].cover < best->cover)) best = &b->extra[i];
        return best;
    };
    const czk_table_set* t = find();
    if (!t && build && b->nomem_class.load(std::memory_order_acquire) & (1u << (cc & 31))) return CZK_OK;   // see below: no room last time
    if (!t && build) {
        std::lock_guard<std::mutex> lk(b->build_mu);
        t = find();   // another context may have built it meanwhile
        const int n = b->n_extra.load(std::memory_order_acquire);
        if (!t && n < czk_bases::MAX_EXTRA) {
            // ONE set per narrow class (c = 13: 2^14 points, c = 15: 2^17 -- they are small), powers of two for c = 17: at most 2 + (log2 n - 16) sets per
            // key, so a prover that commits polynomials of many different lengths cannot run out of slots and fall back to the wide tables
            size_t cover = cc == 13 ? ((size_t)1 << 14) : cc == 15 ? ((size_t)1 << 17) : 1;
            while (cover < size) cover <<= 1;
            if (cover > b->n) cover = b->n;
            CZK_TRY(msm_pipeline_sync(ctx));   // (the build synchronises ctx->stream; drain the MSM streams too so that timing stays attributable)
            int rc = b->group == CZK_G1 ? build_secondary<Fq>(ctx, b, cc, cover, &b->extra[n]) : build_secondary<Fq2>(ctx, b, cc, cover, &b->extra[n]);
            if (rc == CZK_ERR_NOMEM) {
                // no room for another table set: this call and later ones of its width class run on the key's own tables.  The class is
                // remembered on the handle, so later calls do not drain the pipeline and retry four failing allocations each time
                // (czk_bases_prepare tries again: a caller that freed memory asks for the set explicitly); the swallowed error is cleared.
                (void)hipGetLastError();
                b->nomem_class.fetch_or(1u << (cc & 31), std::memory_order_release);
                ctx->err.clear();
                return CZK_OK;
            }
            CZK_TRY(rc);
            b->n_extra.store(n + 1, std::memory_order_release);
            t = &b->extra[n];
        }
    }
    if (t) *tv = *t;
    return CZK_OK;
}

}  // namespace czk

using namespace czk;

// ------------------------------------------------------------------------------------------------
// C ABI (keys and fixed-base points)
// ------------------------------------------------------------------------------------------------
extern "C" int czk_bases_register(czk_ctx* ctx, int group, const uint64_t* bases, const uint8_t* inf, size_t n, int mem, czk_bases** out) {
    if (!ctx || !out) return CZK_ERR_ARG;
    *out = nullptr;
    if (group != CZK_G1 && group != CZK_G2) return set_err(ctx, CZK_ERR_ARG, "group must be CZK_G1 or CZK_G2");
    if (n && !bases) return set_err(ctx, CZK_ERR_ARG, "null bases");
    const bool no_tables = (mem & CZK_MEM_NO_TABLES) != 0, any_points = (mem & CZK_MEM_ANY_POINTS) != 0, check = (mem & CZK_MEM_CHECK_SUBGROUP) != 0;
    mem &= ~(CZK_MEM_NO_TABLES | CZK_MEM_ANY_POINTS | CZK_MEM_CHECK_SUBGROUP);
    if (!valid_mem(mem))
        return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE (optionally | CZK_MEM_NO_TABLES | CZK_MEM_ANY_POINTS | CZK_MEM_CHECK_SUBGROUP)");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t aw = group == CZK_G1 ? 12 : 24;
    czk_bases* b = new czk_bases();
    b->device = ctx->device;
    b->group = group;
    b->n = n;
    b->split = no_tables;
    b->te_wanted = !any_points;
    b->check_wanted = check;
    b->per_call_width = !ctx->msm_fixed_c;
    b->c = no_tables ? choose_c_split(n) : choose_c(n);
    if (const unsigned v = group == CZK_G1 ? ctx->msm_c_g1 : ctx->msm_c_g2)   // option "msm_window_g1" / "_g2": the primary table set's width
        if (!no_tables && v >= 8 && v <= 22) b->c = v;
    b->W = msm_num_windows(b->c);
    const u64* pts_dev = bases;
    const uint8_t* inf_dev = inf;
    void *tmp_p = nullptr, *tmp_i = nullptr;
    int rc = CZK_OK;
    if (mem == CZK_MEM_HOST && n) {
        if (hipMalloc(&tmp_p, n * aw * 8) != hipSuccess) rc = set_err(ctx, CZK_ERR_NOMEM, "hipMalloc bases staging");
        if (rc == CZK_OK && hipMemcpyAsync(tmp_p, bases, n * aw * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            rc = set_err(ctx, CZK_ERR_HIP, "H2D bases");
        pts_dev = (const u64*)tmp_p;
        if (rc == CZK_OK && inf) {
            if (hipMalloc(&tmp_i, n) != hipSuccess) rc = set_err(ctx, CZK_ERR_NOMEM, "hipMalloc inf staging");
            if (rc == CZK_OK && hipMemcpyAsync(tmp_i, inf, n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                rc = set_err(ctx, CZK_ERR_HIP, "H2D inf");
            inf_dev = (const uint8_t*)tmp_i;
        }
    }
    if (rc == CZK_OK) rc = group == CZK_G1 ? register_impl<Fq>(ctx, b, pts_dev, inf_dev) : register_impl<Fq2>(ctx, b, pts_dev, inf_dev);
    (void)hipStreamSynchronize(ctx->stream);
    if (tmp_p) (void)hipFree(tmp_p);
    if (tmp_i) (void)hipFree(tmp_i);
    const size_t n_flags = (no_tables ? 1 : (size_t)b->W) * n;   // (a multiple 2^(c w) P of a point outside the subgroup can be infinity where P is not: every window counts)
    if (rc == CZK_OK && !ctx->msm_sort_reuse) {   // (the lists are only read under the option: a key registered without it never shares a sort)
    } else if (rc == CZK_OK && n && n_flags < ((size_t)1 << 32)) {   // which table entries are infinity (CZK_MEM_SAME_SCALARS compares two keys' lists)
        std::vector<uint8_t> flags(n_flags);
        if (hipMemcpy(flags.data(), b->inf, n_flags, hipMemcpyDeviceToHost) != hipSuccess) rc = set_err(ctx, CZK_ERR_HIP, "D2H infinity flags");
        else {
            b->inf_listed = true;
            for (size_t i = 0; i < n_flags && b->inf_listed; i++)
                if (flags[i]) {
                    if (b->inf_idx.size() == czk_bases::INF_LIST_MAX) {
                        b->inf_listed = false;
                        b->inf_idx.clear();
                    } else b->inf_idx.push_back((uint32_t)i);
                }
        }
    } else if (rc == CZK_OK) b->inf_listed = n == 0;
    if (rc != CZK_OK) {
        czk_bases_release(b);
        return rc;
    }
    *out = b;
    return CZK_OK;
}

extern "C" void czk_bases_release(czk_bases* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->pts) (void)hipFree(b->pts);
    if (b->inf) (void)hipFree(b->inf);
    if (b->pts_sw0) (void)hipFree(b->pts_sw0);
    for (int i = 0; i < b->n_extra.load(); i++) {
        if (b->extra[i].pts) (void)hipFree(b->extra[i].pts);
        if (b->extra[i].inf) (void)hipFree(b->extra[i].inf);
    }
    delete b;
}

extern "C" size_t czk_bases_len(const czk_bases* b) { return b ? b->n : 0; }
extern "C" int czk_bases_layout(const czk_bases* b, unsigned* c, unsigned* windows) {
    if (!b) return CZK_ERR_ARG;
    if (c) *c = b->c;
    if (windows) *windows = b->W;
    return CZK_OK;
}

extern "C" int czk_bases_layout_for(const czk_bases* b, size_t n_scalars, unsigned* c, unsigned* windows) {
    if (!b) return CZK_ERR_ARG;
    const size_t size = b->n < n_scalars ? b->n : n_scalars;
    const unsigned cc = msm_width_for(b, size);
    if (c) *c = cc;
    if (windows) *windows = msm_num_windows(cc);
    return CZK_OK;
}
extern "C" int czk_bases_check_subgroup(czk_ctx* ctx, const czk_bases* b, size_t* out_bad) {
    if (!ctx || !b || !out_bad) return ctx ? set_err(ctx, CZK_ERR_ARG, "null check_subgroup argument") : CZK_ERR_ARG;
    if (b->checked) {   // CZK_MEM_CHECK_SUBGROUP ran at registration
        *out_bad = b->n_bad;
        return CZK_OK;
    }
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t aw = b->group == CZK_G1 ? 12 : 24;
    const u64* pts = b->te ? b->pts_sw0 : b->pts;   // window 0 = the registered points
    u64* tmp = nullptr;
    if (b->unsat && !b->te && b->n) {   // the table is in the unsaturated residue system: check a converted copy
        CZK_HIP(ctx, hipMalloc(&tmp, b->n * aw * 8));
        hipError_t e = hipMemcpyAsync(tmp, b->pts, b->n * aw * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) {
            launch_convert_from_u(ctx->stream, tmp, b->n * (aw / 6));
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            (void)hipFree(tmp);
            return set_err(ctx, CZK_ERR_HIP, std::string("subgroup check copy: ") + hipGetErrorString(e));
        }
        pts = tmp;
    }
    int rc = b->group == CZK_G1 ? subgroup_check_impl<Fq>(ctx, pts, b->inf, b->n, out_bad) : subgroup_check_impl<Fq2>(ctx, pts, b->inf, b->n, out_bad);
    if (tmp) (void)hipFree(tmp);
    return rc;
}
extern "C" int czk_bases_arith(const czk_bases* b) { return !b ? -1 : b->te ? 2 : b->unsat ? 1 : 0; }
extern "C" int czk_bases_prepare(czk_ctx* ctx, const czk_bases* b, size_t n_scalars) {
    if (!ctx || !b) return ctx ? set_err(ctx, CZK_ERR_ARG, "null bases") : CZK_ERR_ARG;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t size = b->n < n_scalars ? b->n : n_scalars;
    czk_table_set tv;
    const_cast<czk_bases*>(b)->nomem_class.store(0, std::memory_order_release);   // an explicit request retries a set that did not fit earlier
    return pick_tables(ctx, b, size, &tv, true);
}

extern "C" int czk_fixed_base_points(czk_ctx* ctx, int group, const uint64_t* k, size_t n, uint64_t* out, int mem) {
    if (!ctx || (n && (!k || !out))) return ctx ? set_err(ctx, CZK_ERR_ARG, "null fixed_base argument") : CZK_ERR_ARG;
    if (group != CZK_G1 && group != CZK_G2) return set_err(ctx, CZK_ERR_ARG, "group must be CZK_G1 or CZK_G2");
    if (!valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE");
    if (!n) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t aw = group == CZK_G1 ? 12 : 24;
    if (mem == CZK_MEM_DEVICE) return fixed_base_points_device(ctx, group, k, n, out);
    void *kd = nullptr, *od = nullptr;
    CZK_HIP(ctx, hipMalloc(&kd, n * 32));
    CZK_HIP(ctx, hipMalloc(&od, n * aw * 8));
    CZK_HIP(ctx, hipMemcpyAsync(kd, k, n * 32, hipMemcpyHostToDevice, ctx->stream));
    int rc = fixed_base_points_device(ctx, group, (const u64*)kd, n, (u64*)od);
    if (rc == CZK_OK) {
        CZK_HIP(ctx, hipMemcpyAsync(out, od, n * aw * 8, hipMemcpyDeviceToHost, ctx->stream));
        CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    (void)hipFree(kd);
    (void)hipFree(od);
    return rc;
}
