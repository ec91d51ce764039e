// pairing_share.hip -- pairings of a SHARED G1 point with a SHARED G2 point, and the multiplicative target-group shares they yield, on gfx950:
// MpcPairingEngine::pairing (mpc-algebra/src/wire/pairing.rs:194-229) through a pairing triple, and MulFieldShare (share/add.rs:407-480) /
// SpdzMulFieldShare (share/spdz.rs:459-541) in Fq12.  Lanes form only: every party's lanes are on this GPU, in czk_share_group_batch_scale's
// lane order (lane 2 p = party p's sh, lane 2 p + 1 = its mac for SPDZ), so an open of points is a sum over lanes and an open of target-group
// shares a product over lanes.
//   czk_share_pairing: with xa = open(a + tx), yb = open(b + ty) the reference computes z / e(xa, y) / e(x, yb) * e(xa, yb) (pairing.rs:225), the
//     last factor scaled into the share (spdz.rs:500-506).  Here every (lane, element) is ONE product of pairings,
//         out_l = tz_l * FE( ML( (-xa, ty_l), (-tx_l, yb), ([k_l] xa, yb) ) )     k_l = 1 on lane 0, mac_share_j on party j's mac lane, 0 elsewhere
//     (negating the G1 point inverts a pairing value; e(P, Q)^k = e([k] P, Q) in the prime-order subgroup): one Miller loop over two or three pairs,
//     one final exponentiation, one Fq12 product, against 2 L + 1 pairings and two Fq12 inversions per element.
//     k_share_pairing_open: one thread per (element, slot), each ONE double-and-add chain deep.  Every G1 thread sums the sh lanes of a + tx itself;
//       slot 0 writes xa and (SPDZ) checks [alpha] xa - the sum of the mac lanes of a + tx; slot 1 + j writes [mac_share_j] xa; the last slot does
//       for b + ty in G2 what slot 0 does in G1.  A failed check sets the element's flag byte, so an element counts once.
//     k_g2_prepare (pairing.hip) over the L n points ty_l and over the n points yb.
//     k_share_pairing: one thread per (lane, element): pairing.hip's register discipline -- f is 144 VGPRs, the G1 points are reloaded per line, the
//       lines are read strided from the prepare buffers, the final exponentiation parks three Fq12 in the SoA workspace and tz_l is loaded after it.
//       Pairs with an infinite member are skipped (mod.rs:99-103).  Lane 0's thread adds the element's flag to the counter.
//     Nothing is synchronised between the launches; the counter is read back once.
//   czk_gt_share_open / _scale, czk_fq12_vec_op: reveal, scale / from_public and the lane-wise mul / div / inv, one thread per output element.
// Scalars (the parties' mac shares, the key, the integer sum of the shares) are read bit by bit from a DEVICE array: a register array indexed by
// a loop counter, or an array in the argument block, would be copied to scratch by every lane.
// Integer VALU code of field.h / curve.h / tower.h with the Montgomery multiply out of line (-DCZK_NOINLINE_MUL), as pairing.hip.
#include "call.h"
#include "pairing_steps.h"

namespace czk {

template <class F>
CZK_D Jac<F> sp_point(const u64* pts, const uint8_t* inf, size_t idx) {
    if (inf && inf[idx]) return Jac<F>::zero();
    const Affine<F> a = aff_load<F>(pts + (size_t)GT<F>::AW * idx);
    return Jac<F>{a.x, a.y, F::one()};
}

// [k] p; k: 4 canonical u64 (below r < 2^253) in DEVICE memory
template <class F>
CZK_D Jac<F> sp_chain(const Jac<F>& p, const u64* k) {
    Jac<F> acc = Jac<F>::zero();
#pragma unroll 1
    for (int b = 252; b >= 0; b--) {
        acc = jac_double(acc);
        if ((k[b >> 6] >> (b & 63)) & 1) acc = jac_add(acc, p);
    }
    return acc;
}

struct SharePairArgs {
    const u64 *a, *b, *tx, *ty, *tz;                       // L lanes of n G1 points (a, tx), G2 points (b, ty), Fq12 (tz)
    const uint8_t *a_inf, *b_inf, *tx_inf, *ty_inf;        // L n infinity bytes each; null: no point is infinity
    size_t n;
    unsigned lpp, parties;
    const u64* keys;                                       // DEVICE, canonical: the parties' mac shares (4 u64 each), then their sum mod r
    u64 *xa, *kxa, *yb;                                    // the opened points: n G1, parties x n G1 ([mac_share_j] xa), n G2
    uint8_t *xa_inf, *kxa_inf, *yb_inf, *flag;             // their infinity bytes; flag: n bytes, 1 = a MAC check of the element failed (zeroed by the host)
    const u64 *lines_ty, *lines_yb;                        // k_g2_prepare of ty (stride L n) and of yb (stride n)
    u64 *ws, *out;                                         // the final exponentiation's workspace (L n x 216, SoA); L x n x 72
};

// one side of the open: the sum of the sh lanes of v + t; slot 0 writes it and checks its MAC, slot 1 + j writes [mac_share_j] of it
template <class F>
CZK_D void sp_open_side(const SharePairArgs& a, const u64* v, const uint8_t* v_inf, const u64* t, const uint8_t* t_inf, size_t i, unsigned slot, u64* open,
                        uint8_t* open_inf, u64* scaled, uint8_t* scaled_inf) {
    constexpr int AW = GT<F>::AW;
    const unsigned L = a.lpp * a.parties;
    Jac<F> s = Jac<F>::zero();
#pragma unroll 1
    for (unsigned ln = 0; ln < L; ln += a.lpp) {
        const size_t at = (size_t)ln * a.n + i;
        s = jac_add(jac_add(s, sp_point<F>(v, v_inf, at)), sp_point<F>(t, t_inf, at));
    }
    Affine<F> o;
    if (slot == 0) {
        open_inf[i] = jac_to_affine(s, o) ? 1 : 0;
        aff_store<F>(open + (size_t)AW * i, o);
        if (a.lpp != 2) return;
        Jac<F> m = Jac<F>::zero();   // share/spdz.rs:392-402 with the key's shares combined mod r (the points are in the prime-order subgroup)
#pragma unroll 1
        for (unsigned ln = 1; ln < L; ln += 2) {
            const size_t at = (size_t)ln * a.n + i;
            m = jac_add(jac_add(m, sp_point<F>(v, v_inf, at)), sp_point<F>(t, t_inf, at));
        }
        m.y = f_neg(m.y);
        if (!jac_add(sp_chain(s, a.keys + 4 * (size_t)a.parties), m).is_zero()) a.flag[i] = 1;
    } else {
        const size_t at = (size_t)(slot - 1) * a.n + i;
        scaled_inf[at] = jac_to_affine(sp_chain(s, a.keys + 4 * (size_t)(slot - 1)), o) ? 1 : 0;
        aff_store<F>(scaled + (size_t)AW * at, o);
    }
}

// slots per element: the G1 side's (1, and one per party for SPDZ), then the G2 side's one
__global__ __launch_bounds__(128) void k_share_pairing_open(SharePairArgs a) {
    const unsigned g1_slots = a.lpp == 2 ? 1 + a.parties : 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)(g1_slots + 1) * a.n) return;
    const unsigned slot = (unsigned)(idx / a.n);
    const size_t i = idx % a.n;
    if (slot < g1_slots) sp_open_side<Fq>(a, a.a, a.a_inf, a.tx, a.tx_inf, i, slot, a.xa, a.xa_inf, a.kxa, a.kxa_inf);
    else sp_open_side<Fq2>(a, a.b, a.b_inf, a.ty, a.ty_inf, i, 0, a.yb, a.yb_inf, nullptr, nullptr);
}

__global__ __launch_bounds__(PAIR_BLOCK) void k_share_pairing(SharePairArgs a, unsigned long long* bad) {
    const size_t total = (size_t)a.lpp * a.parties * a.n;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const unsigned l = (unsigned)(t / a.n);
    const size_t i = t % a.n;
    const bool spdz = a.lpp == 2, xa_inf = a.xa_inf[i] != 0, yb_inf = a.yb_inf[i] != 0;
    // the third pair's G1 point: xa on lane 0 (k_l = 1), [mac_share_j] xa on party j's mac lane, none elsewhere
    const size_t kat = (size_t)(l >> 1) * a.n + i;
    const u64* p3 = l == 0 ? a.xa + 12 * i : spdz && (l & 1) ? a.kxa + 12 * kat : nullptr;
    const bool skip1 = xa_inf || (a.ty_inf && a.ty_inf[t]);   // mod.rs:99-103
    const bool skip2 = yb_inf || (a.tx_inf && a.tx_inf[t]);
    const bool skip3 = !p3 || yb_inf || (l == 0 ? xa_inf : a.kxa_inf[kat] != 0);
    const Fq12 f = miller_loop([&](Fq12& f, int j) {
        if (!skip1) {
            G1Affine p = aff_load<Fq>(a.xa + 12 * i);
            p.y = fp_neg(p.y);
            ell(f, a.lines_ty + t, total, j, p);
        }
        if (!skip2) {
            G1Affine p = aff_load<Fq>(a.tx + 12 * t);
            p.y = fp_neg(p.y);
            ell(f, a.lines_yb + i, a.n, j, p);
        }
        if (!skip3) ell(f, a.lines_yb + i, a.n, j, aff_load<Fq>(p3));
    });
    const Fq12 r = final_exponentiation(f, a.ws + t, total);
    fq12_store_strided(a.out + 72 * t, 1, f_mul(fq12_load_strided(a.tz + 72 * t, 1), r));
    if (l == 0 && spdz && a.flag[i]) atomicAdd(bad, 1ull);
}

// reveal (share/add.rs:414-416, share/spdz.rs:469-478): out_i = the product of the sh lanes; SPDZ: counted unless x^A / (the product of the mac lanes) is
// one, A = the INTEGER sum of the canonical mac shares (keys + 4 parties + 4: 5 u64, `abits` bits).  minv: n x 72, SoA.
__global__ __launch_bounds__(PAIR_BLOCK) void k_gt_share_open(const u64* v, size_t n, unsigned lpp, unsigned parties, const u64* keys, unsigned abits,
                                                              u64* minv, u64* out, unsigned long long* bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned L = lpp * parties;
    {
        Fq12 x = fq12_load_strided(v + 72 * i, 1);
#pragma unroll 1
        for (unsigned ln = lpp; ln < L; ln += lpp) x = f_mul(x, fq12_load_strided(v + 72 * ((size_t)ln * n + i), 1));
        fq12_store_strided(out + 72 * i, 1, x);
    }
    if (lpp != 2) return;
    {
        Fq12 m = fq12_load_strided(v + 72 * (n + i), 1);
#pragma unroll 1
        for (unsigned ln = 3; ln < L; ln += 2) m = f_mul(m, fq12_load_strided(v + 72 * ((size_t)ln * n + i), 1));
        fq12_store_strided(minv + i, n, f_inv(m));
    }
    const u64* A = keys + 4 * (size_t)parties + 4;
    Fq12 r = Fq12::one();
#pragma unroll 1
    for (int b = (int)abits - 1; b >= 0; b--) {
        r = f_sqr(r);
        if ((A[b >> 6] >> (b & 63)) & 1) r = f_mul(r, fq12_load_strided(out + 72 * i, 1));
    }
    r = f_mul(r, fq12_load_strided(minv + i, n));
    if (!r.is_one()) atomicAdd(bad, 1ull);
}

// scale (share/spdz.rs:500-506, share/add.rs:444-449): lane 0 times f_i, party j's mac lane times f_i^(mac_share_j), the other lanes copied.
// v null: from_public (spdz.rs:479-485, add.rs:417-421), every lane starts at one.
__global__ __launch_bounds__(PAIR_BLOCK) void k_gt_share_scale(const u64* v, const u64* f, size_t n, unsigned lpp, unsigned parties, const u64* keys, u64* out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)lpp * parties * n) return;
    const unsigned l = (unsigned)(t / n);
    const size_t i = t % n;
    Fq12 r;
    if (l == 0) r = fq12_load_strided(f + 72 * i, 1);
    else if (lpp == 2 && (l & 1)) {
        const u64* k = keys + 4 * (size_t)(l >> 1);
        r = Fq12::one();
#pragma unroll 1
        for (int b = 252; b >= 0; b--) {
            r = f_sqr(r);
            if ((k[b >> 6] >> (b & 63)) & 1) r = f_mul(r, fq12_load_strided(f + 72 * i, 1));
        }
    } else {
        fq12_store_strided(out + 72 * t, 1, v ? fq12_load_strided(v + 72 * t, 1) : Fq12::one());
        return;
    }
    if (v) r = f_mul(fq12_load_strided(v + 72 * t, 1), r);
    fq12_store_strided(out + 72 * t, 1, r);
}

// elementwise on flat Fq12 arrays; the inverse of zero is zero (Fermat's inversion at the bottom of the tower)
__global__ __launch_bounds__(PAIR_BLOCK) void k_fq12_vec_op(int op, const u64* a, const u64* b, u64* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fq12 r;
    if (op == CZK_FQ12_OP_INV) r = f_inv(fq12_load_strided(a + 72 * i, 1));
    else {
        r = fq12_load_strided(b + 72 * i, 1);
        if (op == CZK_FQ12_OP_DIV) r = f_inv(r);
        r = f_mul(fq12_load_strided(a + 72 * i, 1), r);
    }
    fq12_store_strided(out + 72 * i, 1, r);
}

static int gt_share_head(czk_ctx* ctx, const char* what, size_t lpp, size_t parties) {
    if ((lpp != 1 && lpp != 2) || parties > 32) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": lpp is 1 (additive) or 2 (SPDZ), parties at most 32");
    return CZK_OK;
}

// the scalars the kernels read, canonical, on the device: the parties' mac shares, their sum mod r, their integer sum (5 u64, padded to 8); *abits: its bit length
static int upload_keys(czk_ctx* ctx, size_t parties, const uint64_t* mac_shares, StageHold& hold, const u64** dev, unsigned* abits) {
    std::vector<u64> h(4 * parties + 12, 0);
    Fr alpha = Fr::zero();
    u64* A = h.data() + 4 * parties + 4;
    for (size_t p = 0; p < parties; p++) {
        const Fr m = host_fr(mac_shares + 4 * p), c = fp_into_repr(m);
        alpha = fp_add(alpha, m);
        unsigned __int128 carry = 0;
        for (int w = 0; w < 5; w++) {
            const u64 cw = w < 4 ? (u64)c.l[2 * w] | ((u64)c.l[2 * w + 1] << 32) : 0;
            if (w < 4) h[4 * p + w] = cw;
            carry += (unsigned __int128)A[w] + cw;
            A[w] = (u64)carry;
            carry >>= 64;
        }
    }
    const Fr ac = fp_into_repr(alpha);
    for (int w = 0; w < 4; w++) h[4 * parties + w] = (u64)ac.l[2 * w] | ((u64)ac.l[2 * w + 1] << 32);
    *abits = 0;
    for (int b = 319; b >= 0 && !*abits; b--)
        if ((A[b >> 6] >> (b & 63)) & 1) *abits = (unsigned)b + 1;
    CZK_TRY(hold.take(h.size() * 8));
    CZK_TRY(upload_pageable(ctx, hold.b.p, h.data(), h.size() * 8));
    *dev = (const u64*)hold.b.p;
    return CZK_OK;
}

}  // namespace czk

using namespace czk;

extern "C" int czk_share_pairing(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* a, const uint8_t* a_inf, const uint64_t* b,
                                 const uint8_t* b_inf, const uint64_t* tx, const uint8_t* tx_inf, const uint64_t* ty, const uint8_t* ty_inf, const uint64_t* tz,
                                 uint64_t* out, size_t n, uint64_t* out_bad) {
    const char* what = "czk_share_pairing";
    if (!ctx) return CZK_ERR_ARG;
    if (!out_bad) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null count output");
    *out_bad = 0;
    CZK_TRY(gt_share_head(ctx, what, lpp, parties));
    if (!n || !parties) return CZK_OK;
    if (!a || !b || !tx || !ty || !tz || !out || (lpp == 2 && !mac_shares)) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    const size_t L = lpp * parties, total = L * n;
    if (n > ((size_t)1 << 36) / (L + 1)) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more outputs than one launch covers");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    SharePairArgs k;
    k.a = (const u64*)a, k.b = (const u64*)b, k.tx = (const u64*)tx, k.ty = (const u64*)ty, k.tz = (const u64*)tz;
    k.a_inf = a_inf, k.b_inf = b_inf, k.tx_inf = tx_inf, k.ty_inf = ty_inf;
    k.n = n, k.lpp = (unsigned)lpp, k.parties = (unsigned)parties, k.out = (u64*)out;
    StageHold ks(ctx), ws(ctx);
    unsigned abits = 0;
    k.keys = nullptr;
    if (lpp == 2) CZK_TRY(upload_keys(ctx, parties, mac_shares, ks, &k.keys, &abits));
    const size_t scaled = lpp == 2 ? parties * n : 0;
    u64 *lines_ty = nullptr, *lines_yb = nullptr;
    auto carve = [&](char* base) {   // the workspace's pieces; with a null base: its size
        Bump bp{base};
        k.xa = bp.take<u64>(n * 12), k.kxa = bp.take<u64>(scaled * 12), k.yb = bp.take<u64>(n * 24);
        lines_ty = bp.take<u64>(total * LINE_WORDS), lines_yb = bp.take<u64>(n * LINE_WORDS);
        k.ws = bp.take<u64>(total * 216);
        k.xa_inf = bp.take<uint8_t>(n), k.kxa_inf = bp.take<uint8_t>(scaled), k.yb_inf = bp.take<uint8_t>(n), k.flag = bp.take<uint8_t>(n);
        return bp.off;
    };
    CZK_TRY(ws.take(carve(nullptr)));
    carve((char*)ws.b.p);
    k.lines_ty = lines_ty, k.lines_yb = lines_yb;
    CZK_TRY(share_counters(ctx));
    CZK_HIP(ctx, hipMemsetAsync(k.flag, 0, n, ctx->stream));
    {
        ProfScope ps(ctx, "share_pairing_open");
        hipLaunchKernelGGL(k_share_pairing_open, grid_for((lpp == 2 ? parties + 2 : 2) * n), dim3(128), 0, ctx->stream, k);
    }
    {
        ProfScope ps(ctx, "pairing_g2_prepare");
        g2_prepare_enqueue(ctx, k.ty, k.ty_inf, total, lines_ty);
        g2_prepare_enqueue(ctx, k.yb, k.yb_inf, n, lines_yb);
    }
    {
        ProfScope ps(ctx, "share_pairing");
        hipLaunchKernelGGL(k_share_pairing, grid_for(total, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, k, ctx->share_cnt);
    }
    CZK_HIP(ctx, hipGetLastError());
    return share_counters_read(ctx, out_bad, nullptr);   // the one read-back
}

extern "C" int czk_gt_share_open(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* v, size_t n, uint64_t* out,
                                 uint64_t* out_bad) {
    const char* what = "czk_gt_share_open";
    if (!ctx) return CZK_ERR_ARG;
    if (!out_bad) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null count output");
    *out_bad = 0;
    CZK_TRY(gt_share_head(ctx, what, lpp, parties));
    if (!n || !parties) return CZK_OK;
    if (!v || !out || (lpp == 2 && !mac_shares)) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    if (n > ((size_t)1 << 36)) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more outputs than one launch covers");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    StageHold ks(ctx), ws(ctx);
    const u64* keys = nullptr;
    unsigned abits = 0;
    if (lpp == 2) {
        CZK_TRY(upload_keys(ctx, parties, mac_shares, ks, &keys, &abits));
        CZK_TRY(ws.take(n * 576));
    }
    CZK_TRY(share_counters(ctx));
    {
        ProfScope ps(ctx, "gt_share_open");
        hipLaunchKernelGGL(k_gt_share_open, grid_for(n, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, (const u64*)v, n, (unsigned)lpp, (unsigned)parties, keys, abits,
                           (u64*)ws.b.p, (u64*)out, ctx->share_cnt);
    }
    CZK_HIP(ctx, hipGetLastError());
    return share_counters_read(ctx, out_bad, nullptr);
}

extern "C" int czk_gt_share_scale(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* v, const uint64_t* f, uint64_t* out,
                                  size_t n) {
    const char* what = "czk_gt_share_scale";
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(gt_share_head(ctx, what, lpp, parties));
    if (!n || !parties) return CZK_OK;
    if (!f || !out || (lpp == 2 && !mac_shares)) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    const size_t total = lpp * parties * n;
    if (n > ((size_t)1 << 36) / (lpp * parties)) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more outputs than one launch covers");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    StageHold ks(ctx);
    const u64* keys = nullptr;
    unsigned abits = 0;
    if (lpp == 2) CZK_TRY(upload_keys(ctx, parties, mac_shares, ks, &keys, &abits));
    {
        ProfScope ps(ctx, "gt_share_scale");
        hipLaunchKernelGGL(k_gt_share_scale, grid_for(total, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, (const u64*)v, (const u64*)f, n, (unsigned)lpp,
                           (unsigned)parties, keys, (u64*)out);
    }
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;   // only enqueues: the keys are read in stream order, their buffer is the staging pool's
}

extern "C" int czk_fq12_vec_op(czk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (op != CZK_FQ12_OP_MUL && op != CZK_FQ12_OP_DIV && op != CZK_FQ12_OP_INV) return set_err(ctx, CZK_ERR_ARG, "czk_fq12_vec_op: unknown op");
    if (!n) return CZK_OK;
    if (!a || !out || (op != CZK_FQ12_OP_INV && !b)) return set_err(ctx, CZK_ERR_ARG, "czk_fq12_vec_op: null argument");
    if (n > ((size_t)1 << 36)) return set_err(ctx, CZK_ERR_SIZE, "czk_fq12_vec_op: more outputs than one launch covers");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CallMem cb(ctx, "fq12 vectors");
    const u64 *da, *db;
    CZK_TRY(cb.in((const u64*)a, n * 576, mem, &da));
    CZK_TRY(cb.in(op == CZK_FQ12_OP_INV ? nullptr : (const u64*)b, n * 576, mem, &db));
    CallOut so(ctx);
    CZK_TRY(so.open(out, n * 576, mem, &cb));
    {
        ProfScope ps(ctx, "fq12_vec_op");
        hipLaunchKernelGGL(k_fq12_vec_op, grid_for(n, PAIR_BLOCK), dim3(PAIR_BLOCK), 0, ctx->stream, op, da, db, so.words(), n);
    }
    CZK_HIP(ctx, hipGetLastError());
    if (mem == CZK_MEM_DEVICE) return CZK_OK;   // only enqueues
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return so.close();
}
