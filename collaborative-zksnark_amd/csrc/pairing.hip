// pairing.hip -- the BLS12-377 pairing and batched Groth16 verification on gfx950.
//
// The reference's engine is `Bls12::<Parameters>` (X = 0x8508c00000000001, X_IS_NEGATIVE = false, TwistType::D;
// curves/bls12_377/src/curves/mod.rs:16-19) over the tower of tower.h:
//   G2Prepared::from ........ algebra/ec/src/models/bls12/g2.rs:69-157   k_g2_prepare (one G2 point per thread)
//   miller_loop / ell ....... algebra/ec/src/models/bls12/mod.rs:54-126  miller_loop() (all pairs of one product in one thread)
//   final_exponentiation .... mod.rs:128-193, the same chain             final_exponentiation()
//   verify_proof ............ groth16/src/verifier.rs:23-58              k_groth16_gic + k_groth16_check
// One thread computes one product of pairings (one Groth16 check): proofs are independent, and the prepared lines of -gamma and
// -delta are shared by every thread of a verification, so those reads are uniform across the wave.
//
// Register budget: an Fq12 is 144 VGPRs.  The Miller loop keeps f and one line in registers.  The final exponentiation has up to
// four Fq12 live in the reference's order (r, y0, y1, y2); the three that are not being worked on are parked in a per-thread
// workspace in global memory, laid out SoA across threads (word w of thread t at ws[w * k + t]) so the loads coalesce.
// Lines of the per-proof G2 points (B) come from k_g2_prepare into a k x 19.9 KB buffer, also SoA: one code path for every
// G2 operand (shared key lines read with stride 1, per-thread lines with stride k), and the doubling / addition steps run once
// per point instead of once per product that uses it (czk_pairing_product may repeat a point).
// The line steps, ell, the Miller loop and the final exponentiation are in pairing_steps.h, which pairing_share.hip includes as well.
#include "call.h"
#include "pairing_steps.h"

namespace czk {

// ------------------------------------------------------------------------------------------------- G2 preparation
CZK_D void store_line(u64* lines, size_t stride, int j, const Fq2& l0, const Fq2& l1, const Fq2& l2) {
    u64* p = lines + (size_t)j * 36 * stride;
    fq2_store_strided(p, stride, l0);
    fq2_store_strided(p + 12 * stride, stride, l1);
    fq2_store_strided(p + 24 * stride, stride, l2);
}

// G2Prepared::from for n affine points (n x 24 u64): line j of point t at lines[(36 j + w) n + t].  Points at infinity write
// nothing (their pairs are skipped by the Miller loop, as the reference's empty ell_coeffs are).
__global__ __launch_bounds__(PAIR_BLOCK) void k_g2_prepare(const u64* q_aff, const uint8_t* q_inf, size_t n, u64* lines) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n || (q_inf && q_inf[t])) return;
    const G2Affine q = aff_load<Fq2>(q_aff + 24 * t);
    Fq2 rx = q.x, ry = q.y, rz = Fq2::one(), l0, l1, l2;
    int j = 0;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        doubling_step(rx, ry, rz, l0, l1, l2);
        store_line(lines + t, n, j++, l0, l1, l2);
        if ((PAIRING_X >> b) & 1) {
            addition_step(rx, ry, rz, q.x, q.y, l0, l1, l2);
            store_line(lines + t, n, j++, l0, l1, l2);
        }
    }
}

// ------------------------------------------------------------------------------------------------- products of pairings
// Product t multiplies pairs [offs[t], offs[t+1]) of the n_pairs inputs (G1 affine n x 12, G2 lines from k_g2_prepare with stride
// n_pairs).  out: k x 72 packed (may be null); is_one: k flags (may be null).
__global__ __launch_bounds__(PAIR_BLOCK) void k_pairing_product(const u64* g1, const uint8_t* g1_inf, const uint8_t* g2_inf, const u64* lines,
                                                                size_t n_pairs, const size_t* offs, size_t k, u64* ws, u64* out,
                                                                uint8_t* is_one) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const size_t lo = offs[t], hi = offs[t + 1];
    Fq12 f = miller_loop([&](Fq12& f, int j) {
#pragma unroll 1
        for (size_t i = lo; i < hi; i++) {
            if ((g1_inf && g1_inf[i]) || (g2_inf && g2_inf[i])) continue;   // mod.rs:99-103
            ell(f, lines + i, n_pairs, j, aff_load<Fq>(g1 + 12 * i));
        }
    });
    const Fq12 r = final_exponentiation(f, ws + t, k);
    if (out) fq12_store_strided(out + 72 * t, 1, r);
    if (is_one) is_one[t] = r.is_one() ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------- Groth16
// verifier.rs:31-35: g_ic = gamma_abc[0] + sum_i x_i gamma_abc[i + 1] (public inputs Montgomery Fr, k x m x 4), then affine.
__global__ __launch_bounds__(PAIR_BLOCK) void k_groth16_gic(const u64* gabc, const uint8_t* gabc_inf, const u64* inputs, size_t m, size_t k,
                                                            u64* gic, uint8_t* gic_inf) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    G1Jac acc = gabc_inf[0] ? G1Jac::zero() : G1Jac{fp_load<FqParams>(gabc), fp_load<FqParams>(gabc + 6), Fq::one()};
#pragma unroll 1
    for (size_t i = 0; i < m; i++) {
        if (gabc_inf[i + 1]) continue;
        const G1Affine base = aff_load<Fq>(gabc + 12 * (i + 1));
        const Fr x = fp_into_repr(fp_load<FrParams>(inputs + 4 * (m * t + i)));   // `i.into_repr()`
        G1Jac term = G1Jac::zero();
#pragma unroll 1
        for (int b = 252; b >= 0; b--) {   // ProjectiveCurve::mul: double-and-add from the top bit
            term = jac_double(term);
            if ((x.l[b >> 5] >> (b & 31)) & 1) term = jac_add_mixed(term, base, false);
        }
        acc = jac_add(acc, term);
    }
    G1Affine a;
    gic_inf[t] = jac_to_affine(acc, a) ? 1 : 0;
    aff_store<Fq>(gic + 12 * t, a);
}

// verifier.rs:37-58: product_of_pairings([(A, B), (g_ic, -gamma), (C, -delta)]) == e(alpha, beta), one final exponentiation.
// b_lines: the proofs' B from k_g2_prepare (stride k); ng / nd: the key's prepared -gamma / -delta (stride `ls`); inf: k x 3 (A, B, C).
__global__ __launch_bounds__(PAIR_BLOCK) void k_groth16_check(const u64* a, const u64* c, const uint8_t* inf, const u64* b_lines, const u64* gic,
                                                              const uint8_t* gic_inf, const u64* ng, const u64* nd, size_t ls,
                                                              const u64* alpha_beta, size_t k, u64* ws, uint8_t* ok) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const bool skip_ab = inf && (inf[3 * t] || inf[3 * t + 1]), skip_c = inf && inf[3 * t + 2], skip_ic = gic_inf[t];
    Fq12 f = miller_loop([&](Fq12& f, int j) {
        if (!skip_ab) ell(f, b_lines + t, k, j, aff_load<Fq>(a + 12 * t));
        if (!skip_ic) ell(f, ng, ls, j, aff_load<Fq>(gic + 12 * t));
        if (!skip_c) ell(f, nd, ls, j, aff_load<Fq>(c + 12 * t));
    });
    const Fq12 r = final_exponentiation(f, ws + t, k);
    ok[t] = r == fq12_load_strided(alpha_beta, 1) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------- host side
// products of pairings over device inputs; offs_host: k + 1 offsets; out / is_one device (either may be null)
static int pairing_products_device(czk_ctx* ctx, CallMem& cb, const u64* g1, const uint8_t* g1_inf, const u64* g2, const uint8_t* g2_inf,
                                   const size_t* offs_host, size_t k, u64* out, uint8_t* is_one) {
    const size_t n = offs_host[k];
    u64 *lines = nullptr, *ws = nullptr;
    size_t* offs = nullptr;
    CZK_TRY(cb.get(&lines, n * LINE_WORDS * 8));
    CZK_TRY(cb.get(&ws, k * 216 * 8));
    CZK_TRY(cb.get(&offs, (k + 1) * sizeof(size_t)));
    CZK_HIP(ctx, hipMemcpyAsync(offs, offs_host, (k + 1) * sizeof(size_t), hipMemcpyHostToDevice, ctx->stream));
    if (n) {
        ProfScope ps(ctx, "pairing_g2_prepare", ctx->stream);
        hipLaunchKernelGGL(k_g2_prepare, grid_for(n, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, g2, g2_inf, n, lines);
    }
    {
        ProfScope ps(ctx, "pairing_miller_fexp", ctx->stream);
        hipLaunchKernelGGL(k_pairing_product, grid_for(k, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, g1, g1_inf, g2_inf, lines, n, offs, k, ws, out,
                           is_one);
    }
    CZK_HIP(ctx, hipGetLastError());
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CZK_OK;
}

// k_g2_prepare for callers in other files (pairing_share.hip): n DEVICE points -> lines, stride n.  Only enqueues on the context's stream.
void g2_prepare_enqueue(czk_ctx* ctx, const u64* q_aff, const uint8_t* q_inf, size_t n, u64* lines) {
    hipLaunchKernelGGL(k_g2_prepare, grid_for(n, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, q_aff, q_inf, n, lines);
}

// the KZG10 verifier's entry (kzg.hip)
int pairing_is_one_device(czk_ctx* ctx, const u64* g1, const uint8_t* g1_inf, const u64* g2, const uint8_t* g2_inf, const size_t* offs_host, size_t k,
                          uint8_t* is_one) {
    CallMem cb(ctx, "pairing workspace");
    return pairing_products_device(ctx, cb, g1, g1_inf, g2, g2_inf, offs_host, k, nullptr, is_one);
}

static int pairing_products(czk_ctx* ctx, const uint64_t* g1, const uint8_t* g1_inf, const uint64_t* g2, const uint8_t* g2_inf,
                            const size_t* offs, size_t k, uint64_t* out, uint8_t* out_is_one, int mem) {
    const size_t n = offs[k];
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CallMem cb(ctx, "pairing workspace");
    const u64 *dg1, *dg2;
    const uint8_t *dg1i, *dg2i;
    CZK_TRY(cb.in(g1, n * 96, mem, &dg1));
    CZK_TRY(cb.in(g2, n * 192, mem, &dg2));
    CZK_TRY(cb.in(g1_inf, n, mem, &dg1i));
    CZK_TRY(cb.in(g2_inf, n, mem, &dg2i));
    CallOut so(ctx), sone(ctx);   // (either may be null: the kernel then leaves it out)
    if (out) CZK_TRY(so.open(out, k * 576, mem, &cb));
    if (out_is_one) CZK_TRY(sone.open(out_is_one, k, mem, &cb));
    CZK_TRY(pairing_products_device(ctx, cb, dg1, dg1i, dg2, dg2i, offs, k, so.words(), sone.flags()));
    CZK_TRY(so.close());
    return sone.close();
}

}  // namespace czk

using namespace czk;

struct czk_groth16_pvk {
    int device = 0;
    size_t n_gamma_abc = 0;
    u64* alpha_beta = nullptr;   // e(alpha, beta), 72 u64 (device)
    u64* lines = nullptr;        // -gamma (point 0) and -delta (point 1) prepared, stride 2 (device)
    u64* gabc = nullptr;         // gamma_abc_g1, n x 12 (device)
    uint8_t* gabc_inf = nullptr; // n flags (device)
};

extern "C" int czk_pairing(czk_ctx* ctx, const uint64_t* g1, const uint8_t* g1_inf, const uint64_t* g2, const uint8_t* g2_inf, size_t n, uint64_t* out,
                           int mem) {
    if (!ctx || (n && (!g1 || !g2 || !out))) return ctx ? set_err(ctx, CZK_ERR_ARG, "null pairing argument") : CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (!n) return CZK_OK;
    std::vector<size_t> offs(n + 1);
    for (size_t i = 0; i <= n; i++) offs[i] = i;
    return pairing_products(ctx, g1, g1_inf, g2, g2_inf, offs.data(), n, out, nullptr, mem);
}

extern "C" int czk_pairing_product(czk_ctx* ctx, const uint64_t* g1, const uint8_t* g1_inf, const uint64_t* g2, const uint8_t* g2_inf,
                                   const size_t* offsets, size_t k, uint64_t* out, uint8_t* out_is_one, int mem) {
    if (!ctx || (k && !offsets)) return ctx ? set_err(ctx, CZK_ERR_ARG, "null pairing_product argument") : CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (!k) return CZK_OK;
    size_t n;
    CZK_TRY(check_offsets(ctx, offsets, k, &n));
    if (n && (!g1 || !g2)) return set_err(ctx, CZK_ERR_ARG, "null points");
    return pairing_products(ctx, g1, g1_inf, g2, g2_inf, offsets, k, out, out_is_one, mem);
}

void czk_groth16_pvk_release(czk_groth16_pvk* pvk) {
    if (!pvk) return;
    (void)hipSetDevice(pvk->device);
    (void)hipFree(pvk->alpha_beta);
    (void)hipFree(pvk->lines);
    (void)hipFree(pvk->gabc);
    (void)hipFree(pvk->gabc_inf);
    delete pvk;
}

extern "C" int czk_groth16_pvk_create(czk_ctx* ctx, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2,
                                      const uint64_t* delta_g2, const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t n_gamma_abc,
                                      czk_groth16_pvk** out) {
    if (!ctx || !out) return CZK_ERR_ARG;
    *out = nullptr;
    if (!alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !n_gamma_abc || !gamma_abc_g1)
        return set_err(ctx, CZK_ERR_ARG, "null verifying key argument (gamma_abc_g1 needs at least one point)");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    czk_groth16_pvk* pvk = new czk_groth16_pvk();
    pvk->device = ctx->device;
    pvk->n_gamma_abc = n_gamma_abc;
    int rc = CZK_OK;
    auto alloc = [&](void** p, size_t bytes) {
        if (rc == CZK_OK && hipMalloc(p, bytes) != hipSuccess) rc = set_err(ctx, CZK_ERR_NOMEM, "hipMalloc verifying key");
    };
    alloc((void**)&pvk->alpha_beta, 576);
    alloc((void**)&pvk->lines, 2 * LINE_WORDS * 8);
    alloc((void**)&pvk->gabc, n_gamma_abc * 96);
    alloc((void**)&pvk->gabc_inf, n_gamma_abc);
    if (rc == CZK_OK) {
        // verifier.rs:12-20: -gamma, -delta (Neg: (x, -y)); the G2 points of a key are finite
        u64 neg[48];
        for (int p = 0; p < 2; p++) {
            const uint64_t* src = p ? delta_g2 : gamma_g2;
            for (int w = 0; w < 12; w++) neg[24 * p + w] = src[w];
            fq2_store_strided(neg + 24 * p + 12, 1, f_neg(fq2_load_strided(src + 12, 1)));
        }
        std::vector<uint8_t> inf(n_gamma_abc, 0);
        if (gamma_abc_inf) inf.assign(gamma_abc_inf, gamma_abc_inf + n_gamma_abc);
        CallMem cb(ctx, "pairing workspace");
        u64* dneg = nullptr;
        rc = cb.get(&dneg, sizeof(neg));
        if (rc == CZK_OK && (hipMemcpyAsync(dneg, neg, sizeof(neg), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                             hipMemcpyAsync(pvk->gabc, gamma_abc_g1, n_gamma_abc * 96, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                             hipMemcpyAsync(pvk->gabc_inf, inf.data(), n_gamma_abc, hipMemcpyHostToDevice, ctx->stream) != hipSuccess))
            rc = set_err(ctx, CZK_ERR_HIP, "verifying key upload");
        if (rc == CZK_OK) {
            ProfScope ps(ctx, "pairing_g2_prepare", ctx->stream);
            hipLaunchKernelGGL(k_g2_prepare, dim3(1), dim3(PAIR_BLOCK), 0, ctx->stream, (const u64*)dneg, (const uint8_t*)nullptr, (size_t)2, pvk->lines);
        }
        if (rc == CZK_OK && hipGetLastError() != hipSuccess) rc = set_err(ctx, CZK_ERR_HIP, "k_g2_prepare launch");
        // e(alpha, beta) (prepare_verifying_key's alpha_g1_beta_g2)
        if (rc == CZK_OK) {
            const u64 *da, *db;
            size_t offs[2] = {0, 1};
            rc = cb.in(alpha_g1, 96, CZK_MEM_HOST, &da);
            if (rc == CZK_OK) rc = cb.in(beta_g2, 192, CZK_MEM_HOST, &db);
            if (rc == CZK_OK) rc = pairing_products_device(ctx, cb, da, nullptr, db, nullptr, offs, 1, pvk->alpha_beta, nullptr);
        }
    }
    if (rc != CZK_OK) {
        czk_groth16_pvk_release(pvk);
        return rc;
    }
    *out = pvk;
    return CZK_OK;
}

extern "C" int czk_groth16_verify(czk_ctx* ctx, const czk_groth16_pvk* pvk, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                                  const uint8_t* inf, const uint64_t* public_inputs, size_t m, size_t k, uint8_t* out_ok, int mem) {
    if (!ctx || !pvk) return ctx ? set_err(ctx, CZK_ERR_ARG, "null verifying key") : CZK_ERR_ARG;
    if (m + 1 != pvk->n_gamma_abc) return set_err(ctx, CZK_ERR_ARG, "MalformedVerifyingKey");   // verifier.rs:28-30
    CZK_TRY(check_mem(ctx, mem));
    CZK_TRY(check_device(ctx, pvk->device, "verifying key lives on another device"));
    if (!k) return CZK_OK;
    if (!a || !b || !c || !out_ok || (m && !public_inputs)) return set_err(ctx, CZK_ERR_ARG, "null proof argument");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CallMem cb(ctx, "pairing workspace");
    const u64 *da, *db, *dc, *dx;
    const uint8_t* dinf;
    CZK_TRY(cb.in(a, k * 96, mem, &da));
    CZK_TRY(cb.in(b, k * 192, mem, &db));
    CZK_TRY(cb.in(c, k * 96, mem, &dc));
    CZK_TRY(cb.in(inf, k * 3, mem, &dinf));
    CZK_TRY(cb.in(m ? public_inputs : nullptr, k * m * 32, mem, &dx));
    u64 *lines, *gic, *ws;
    uint8_t* gic_inf;
    CallOut sok(ctx);
    CZK_TRY(cb.get(&lines, k * LINE_WORDS * 8));
    CZK_TRY(cb.get(&gic, k * 96));
    CZK_TRY(cb.get(&gic_inf, k));
    CZK_TRY(cb.get(&ws, k * 216 * 8));
    CZK_TRY(sok.open(out_ok, k, mem, &cb));
    // B's infinity flag is column 1 of inf: prepare every B (an infinite B's lines are never read)
    {
        ProfScope ps(ctx, "pairing_g2_prepare", ctx->stream);
        hipLaunchKernelGGL(k_g2_prepare, grid_for(k, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, db, (const uint8_t*)nullptr, k, lines);
    }
    {
        ProfScope ps(ctx, "groth16_gic", ctx->stream);
        hipLaunchKernelGGL(k_groth16_gic, grid_for(k, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, (const u64*)pvk->gabc, (const uint8_t*)pvk->gabc_inf, dx,
                           m, k, gic, gic_inf);
    }
    {
        ProfScope ps(ctx, "groth16_check", ctx->stream);
        hipLaunchKernelGGL(k_groth16_check, grid_for(k, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, da, dc, dinf, (const u64*)lines, (const u64*)gic,
                           (const uint8_t*)gic_inf, (const u64*)pvk->lines, (const u64*)(pvk->lines + 1), (size_t)2,
                           (const u64*)pvk->alpha_beta, k, ws, sok.flags());
    }
    CZK_HIP(ctx, hipGetLastError());
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return sok.close();
}
