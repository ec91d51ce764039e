// share_mul.hip -- products, inverses and running products of SHARED vectors: FieldShare::batch_mul / batch_inv / partial_products
// (mpc-algebra/src/share/field.rs:97-127, :135-148, :163-182) on device lanes, for additive (1 lane per party) and SPDZ (sh + mac lane per party)
// shares with any MAC key.  Bandwidth-bound passes over 32-byte elements: what counts is how often a vector crosses HBM.
//   lanes form: every party's lanes are on this GPU, so an open is a sum over lanes inside the thread that owns the element.  k_share_mul is the
//     whole batch_mul in ONE launch: both masked factors, their sums, both MAC checks and every lane's combine; each of x, y, tx, ty, tz is read
//     once, the output lanes are written once (for up to SHARE_MUL_REG_LANES lanes the triple's x / y shares stay in registers between the open and
//     the combine; beyond that they are read a second time by the thread that just read them).  Where the product only feeds an open
//     (batch_inv's x b, partial_products' m x m_inv) the kernel opens it on the spot and writes the n opened values instead of the lanes.
//   net form: one party per communicator (net_rounds.hip): k_share_mask writes both masked factors of the party's lanes into the contiguous 2n open
//     buffer -- the two opens of a batch_mul are independent and go out as ONE open -- and k_share_combine combines the lanes after it.
//   k_share_scale: out_l = c_l * (k * prefix), the last step of batch_inv (prefix absent) and of partial_products (the running products of the
//     opened values are never written per lane).
// No LDS, no scratch; the counts go by vector atomics to two device counters.
#include "czk_internal.h"

namespace czk {

constexpr size_t SHARE_MUL_BLOCKS_PER_CU = 8;   // grid-stride cap of every kernel here, on blocks of 256 threads
constexpr unsigned SHARE_MUL_REG_LANES = 8;     // k_share_mul keeps the triple's x / y shares in registers up to this many lanes

__device__ __forceinline__ Fr sv_load(const ShareVec& v, unsigned lane, size_t i) {
    return fp_load<FrParams>(v.p + 4 * ((size_t)lane * v.lane_stride + i * v.elem_stride));
}
__device__ __forceinline__ Fr mfr_load(const u64* base, size_t idx) { return fp_load<FrParams>(base + 4 * idx); }
__device__ __forceinline__ void mfr_store(u64* base, size_t idx, const Fr& v) { fp_store<FrParams>(base + 4 * idx, v); }

struct ShareMulArgs {
    ShareVec x, y, tx, ty, tz;
    u64* out;            // L lanes, out_stride apart; null: the product's shares are not written
    size_t out_stride;
    u64* open_out;       // non-null: the product is opened right here: n values, its MAC check counted
    size_t n;
    unsigned lpp, parties;
    Fr alpha;            // the MAC key: sum of the parties' shares
    Fr mac_share[32];
};

// LANES > 0: exactly that many lanes, triple shares in registers; LANES == 0: any number of lanes, tx / ty read again for the combine
template <unsigned LANES>
__global__ __launch_bounds__(256) void k_share_mul(ShareMulArgs a, unsigned long long* bad) {
    const unsigned L = LANES ? LANES : a.lpp * a.parties;
    const bool spdz = a.lpp == 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (size_t)gridDim.x * blockDim.x) {
        Fr kx[LANES ? LANES : 1], ky[LANES ? LANES : 1];
        Fr sx = Fr::zero(), oy = Fr::zero(), ma = Fr::zero(), mb = Fr::zero();   // open(x + tx), open(y + ty) and the sums of their mac lanes
#pragma unroll
        for (unsigned ln = 0; ln < L; ln++) {
            const Fr txl = sv_load(a.tx, ln, i), tyl = sv_load(a.ty, ln, i);
            if (LANES) kx[LANES ? ln : 0] = txl, ky[LANES ? ln : 0] = tyl;
            const Fr fa = fp_add(sv_load(a.x, ln, i), txl), fb = fp_add(sv_load(a.y, ln, i), tyl);
            if (spdz && (ln & 1)) ma = fp_add(ma, fa), mb = fp_add(mb, fb);
            else sx = fp_add(sx, fa), oy = fp_add(oy, fb);
        }
        unsigned nbad = 0;
        if (spdz) {   // sum_p (mac_share_p * value - mac_p) must vanish (share/spdz.rs:176-183)
            if (!fp_sub(fp_mul(a.alpha, sx), ma).is_zero()) nbad++;
            if (!fp_sub(fp_mul(a.alpha, oy), mb).is_zero()) nbad++;
        }
        const Fr open = fp_mul(sx, oy);
        Fr pv = Fr::zero(), pm = Fr::zero();
#pragma unroll
        for (unsigned ln = 0; ln < L; ln++) {
            const Fr txl = LANES ? kx[LANES ? ln : 0] : sv_load(a.tx, ln, i), tyl = LANES ? ky[LANES ? ln : 0] : sv_load(a.ty, ln, i);
            Fr r = fp_sub(fp_sub(sv_load(a.tz, ln, i), fp_mul(tyl, sx)), fp_mul(txl, oy));
            if (spdz && (ln & 1)) {
                r = fp_add(r, fp_mul(a.mac_share[ln >> 1], open));   // shift: mac += mac_share * v (share/spdz.rs:204-208)
                pm = fp_add(pm, r);
            } else {
                if (ln == 0) r = fp_add(r, open);                    // shift: the king's sh lane (share/add.rs:141-146)
                pv = fp_add(pv, r);
            }
            if (a.out) mfr_store(a.out + 4 * (size_t)ln * a.out_stride, i, r);
        }
        if (a.open_out) {
            mfr_store(a.open_out, i, pv);
            if (spdz && !fp_sub(fp_mul(a.alpha, pv), pm).is_zero()) nbad++;
        }
        if (nbad) atomicAdd(bad, (unsigned long long)nbad);
    }
}

__global__ __launch_bounds__(256) void k_share_mask(ShareVec x, ShareVec y, ShareVec tx, ShareVec ty, unsigned lanes, u64* open, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        for (unsigned ln = 0; ln < lanes; ln++) {
            mfr_store(open + 4 * (size_t)ln * 2 * n, i, fp_add(sv_load(x, ln, i), sv_load(tx, ln, i)));
            mfr_store(open + 4 * ((size_t)ln * 2 * n + n), i, fp_add(sv_load(y, ln, i), sv_load(ty, ln, i)));
        }
}

__global__ __launch_bounds__(256) void k_share_combine(const u64* opened, ShareVec tx, ShareVec ty, ShareVec tz, unsigned lpp, int king, Fr mac_share, u64* out,
                                                       size_t out_stride, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const Fr sx = mfr_load(opened, i), oy = mfr_load(opened, n + i), open = fp_mul(sx, oy);
        for (unsigned ln = 0; ln < lpp; ln++) {
            Fr r = fp_sub(fp_sub(sv_load(tz, ln, i), fp_mul(sv_load(ty, ln, i), sx)), fp_mul(sv_load(tx, ln, i), oy));
            if (ln == 1) r = fp_add(r, fp_mul(mac_share, open));
            else if (king) r = fp_add(r, open);
            mfr_store(out + 4 * (size_t)ln * out_stride, i, r);
        }
    }
}

__global__ __launch_bounds__(256) void k_share_scale(ShareVec c, unsigned lanes, const u64* k, const u64* prefix, u64* out, size_t out_stride, size_t n,
                                                     unsigned long long* zero) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr s = mfr_load(k, i);
        if (s.is_zero()) atomicAdd(zero, 1ull);   // an inverse is never zero: the opened divisor was (the reference unwraps there)
        if (prefix) s = fp_mul(s, mfr_load(prefix, i));
        for (unsigned ln = 0; ln < lanes; ln++) mfr_store(out + 4 * (size_t)ln * out_stride, i, fp_mul(sv_load(c, ln, i), s));
    }
}

static unsigned share_mul_grid(czk_ctx* ctx, size_t n) {
    size_t blocks = (n + 255) / 256;
    const size_t cap = SHARE_MUL_BLOCKS_PER_CU * (size_t)ctx->num_cu;
    if (blocks > cap) blocks = cap;
    return blocks ? (unsigned)blocks : 1u;
}

int share_counters(czk_ctx* ctx) {
    if (!ctx->share_cnt) CZK_HIP(ctx, hipMalloc(&ctx->share_cnt, 16));
    CZK_HIP(ctx, hipMemsetAsync(ctx->share_cnt, 0, 16, ctx->stream));
    return CZK_OK;
}

int share_counters_read(czk_ctx* ctx, uint64_t* out_bad, uint64_t* out_zero) {
    unsigned long long h[2] = {0, 0};
    CZK_HIP(ctx, hipMemcpyAsync(h, ctx->share_cnt, 16, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the counts are the call's result (the reference asserts / unwraps right here)
    if (out_bad) *out_bad = h[0];
    if (out_zero) *out_zero = h[1];
    return CZK_OK;
}

int share_mask_launch(czk_ctx* ctx, unsigned lanes, ShareVec x, ShareVec y, ShareVec tx, ShareVec ty, u64* open, size_t n) {
    ProfScope ps(ctx, "share_mask");
    hipLaunchKernelGGL(k_share_mask, dim3(share_mul_grid(ctx, n)), dim3(256), 0, ctx->stream, x, y, tx, ty, lanes, open, n);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

int share_combine_launch(czk_ctx* ctx, unsigned lpp, bool king, const Fr& mac_share, const u64* opened, ShareVec tx, ShareVec ty, ShareVec tz, u64* out,
                         size_t out_stride, size_t n) {
    ProfScope ps(ctx, "share_combine");
    hipLaunchKernelGGL(k_share_combine, dim3(share_mul_grid(ctx, n)), dim3(256), 0, ctx->stream, opened, tx, ty, tz, lpp, king ? 1 : 0, mac_share, out, out_stride, n);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

int share_scale_launch(czk_ctx* ctx, unsigned lanes, ShareVec c, const u64* k, const u64* prefix, u64* out, size_t out_stride, size_t n) {
    ProfScope ps(ctx, "share_scale");
    hipLaunchKernelGGL(k_share_scale, dim3(share_mul_grid(ctx, n)), dim3(256), 0, ctx->stream, c, lanes, k, prefix, out, out_stride, n, ctx->share_cnt + 1);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

// one batch_mul of the lanes form, enqueued: shares to `out` (may be null) and / or the opened product to `open_out` (may be null)
static int share_mul_launch(czk_ctx* ctx, ShareMulArgs& a, ShareVec x, ShareVec y, const u64* tx, const u64* ty, const u64* tz, size_t t_stride, size_t t_first,
                            u64* out, u64* open_out) {
    a.x = x, a.y = y;
    a.tx = ShareVec{tx + 4 * t_first, t_stride, 1};
    a.ty = ShareVec{ty + 4 * t_first, t_stride, 1};
    a.tz = ShareVec{tz + 4 * t_first, t_stride, 1};
    a.out = out, a.out_stride = a.n, a.open_out = open_out;
    const dim3 g(share_mul_grid(ctx, a.n)), b(256);
    ProfScope ps(ctx, "share_mul");
    switch (a.lpp * a.parties) {
#define CZK_SHARE_MUL_CASE(LN)                                                                  \
    case LN:                                                                                    \
        hipLaunchKernelGGL(k_share_mul<LN>, g, b, 0, ctx->stream, a, ctx->share_cnt);           \
        break;
        CZK_SHARE_MUL_CASE(1)
        CZK_SHARE_MUL_CASE(2)
        CZK_SHARE_MUL_CASE(3)
        CZK_SHARE_MUL_CASE(4)
        CZK_SHARE_MUL_CASE(6)
        CZK_SHARE_MUL_CASE(8)
#undef CZK_SHARE_MUL_CASE
        default:
            hipLaunchKernelGGL(k_share_mul<0>, g, b, 0, ctx->stream, a, ctx->share_cnt);
    }
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}
static_assert(SHARE_MUL_REG_LANES == 8, "the register-resident instantiations above end at SHARE_MUL_REG_LANES");

// The argument rules of the three lanes-form calls; *work = there is something to do.  Fills the scheme, the key and n into `a`.
static int share_lanes_args(czk_ctx* ctx, const char* what, size_t lpp, size_t parties, const uint64_t* mac_shares, bool null_vec, size_t n, uint64_t* out_bad,
                            uint64_t* out_zero, ShareMulArgs* a, bool* work) {
    *work = false;
    if (!ctx) return CZK_ERR_ARG;
    if (!out_bad || !out_zero) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null count output");
    *out_bad = *out_zero = 0;
    if ((lpp != 1 && lpp != 2) || parties > 32) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": lpp is 1 (additive) or 2 (SPDZ), parties at most 32");
    if (!n || !parties) return CZK_OK;
    if (null_vec || (lpp == 2 && !mac_shares)) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    if (n > ((size_t)1 << 56) / (lpp * parties)) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": the lane arrays' byte count overflows");
    a->n = n, a->lpp = (unsigned)lpp, a->parties = (unsigned)parties;
    a->alpha = Fr::zero();
    for (size_t p = 0; p < 32; p++) {
        a->mac_share[p] = lpp == 2 && p < parties ? host_fr(mac_shares + 4 * p) : Fr::zero();
        a->alpha = fp_add(a->alpha, a->mac_share[p]);
    }
    *work = true;
    return CZK_OK;
}

}  // namespace czk

using namespace czk;

extern "C" int czk_share_material_counts(int op, size_t n, size_t* triples, size_t* pairs) {
    if (!triples || !pairs) return CZK_ERR_ARG;
    *triples = *pairs = 0;
    if (n > ((size_t)1 << 58)) return CZK_ERR_SIZE;
    switch (op) {
        case CZK_SHARE_OP_MUL: *triples = n; return CZK_OK;
        case CZK_SHARE_OP_INV: *triples = n, *pairs = n; return CZK_OK;
        case CZK_SHARE_OP_PARTIAL_PRODUCTS: *triples = 4 * n, *pairs = n ? 2 * n + 1 : 0; return CZK_OK;
    }
    return CZK_ERR_ARG;
}

extern "C" int czk_share_batch_mul(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* x, const uint64_t* y, const uint64_t* tx,
                                   const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero) {
    ShareMulArgs a;
    bool work;
    CZK_TRY(share_lanes_args(ctx, "czk_share_batch_mul", lpp, parties, mac_shares, !x || !y || !tx || !ty || !tz || !out, n, out_bad, out_zero, &a, &work));
    if (!work) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CZK_TRY(share_counters(ctx));
    CZK_TRY(share_mul_launch(ctx, a, ShareVec{(const u64*)x, n, 1}, ShareVec{(const u64*)y, n, 1}, (const u64*)tx, (const u64*)ty, (const u64*)tz, n, 0, (u64*)out, nullptr));
    return share_counters_read(ctx, out_bad, out_zero);
}

extern "C" int czk_share_batch_inv(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* x, const uint64_t* pb, const uint64_t* pc,
                                   const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero) {
    ShareMulArgs a;
    bool work;
    CZK_TRY(share_lanes_args(ctx, "czk_share_batch_inv", lpp, parties, mac_shares, !x || !pb || !pc || !tx || !ty || !tz || !out, n, out_bad, out_zero, &a, &work));
    if (!work) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    StageHold ws(ctx);
    CZK_TRY(ws.take(2 * n * 32));
    u64 *v = (u64*)ws.b.p, *vinv = v + 4 * n;
    CZK_TRY(share_counters(ctx));
    // open(batch_mul(x, b)) in one launch: the product's shares only feed the open
    CZK_TRY(share_mul_launch(ctx, a, ShareVec{(const u64*)x, n, 1}, ShareVec{(const u64*)pb, n, 1}, (const u64*)tx, (const u64*)ty, (const u64*)tz, n, 0, nullptr, v));
    CZK_TRY(czk_fr_batch_inverse(ctx, v, n, nullptr, vinv, CZK_MEM_DEVICE));
    CZK_TRY(share_scale_launch(ctx, a.lpp * a.parties, ShareVec{(const u64*)pc, n, 1}, vinv, nullptr, (u64*)out, n, n));
    return share_counters_read(ctx, out_bad, out_zero);
}

extern "C" int czk_share_partial_products(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* x, const uint64_t* pb,
                                          const uint64_t* pc, const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, uint64_t* out_bad,
                                          uint64_t* out_zero) {
    ShareMulArgs a;
    bool work;
    CZK_TRY(share_lanes_args(ctx, "czk_share_partial_products", lpp, parties, mac_shares, !x || !pb || !pc || !tx || !ty || !tz || !out, n, out_bad, out_zero, &a,
                             &work));
    if (!work) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t L = lpp * parties, T = 4 * n, P = 2 * n + 1;
    StageHold ws(ctx);
    CZK_TRY(ws.take((L + 4) * n * 32));
    u64 *lanes = (u64*)ws.b.p, *mxm = lanes + 4 * L * n, *run = mxm + 4 * n, *mms = run + 4 * n, *inv = mms + 4 * n;
    const u64 *b = (const u64*)pb, *c = (const u64*)pc, *t0 = (const u64*)tx, *t1 = (const u64*)ty, *t2 = (const u64*)tz;
    const ShareVec m_inv1{c + 4, P, 1};                                                                             // m_inv[1..]
    CZK_TRY(share_counters(ctx));
    CZK_TRY(share_mul_launch(ctx, a, ShareVec{b, P, 1}, ShareVec{(const u64*)x, n, 1}, t0, t1, t2, T, 0, lanes, nullptr));   // mx = m[..n] x
    CZK_TRY(share_mul_launch(ctx, a, ShareVec{lanes, n, 1}, m_inv1, t0, t1, t2, T, n, nullptr, mxm));                        // open(mx m_inv[1..])
    CZK_TRY(czk_fr_prefix_product(ctx, mxm, n, run, CZK_MEM_DEVICE));                                                        // the local loop :169-172
    CZK_TRY(share_mul_launch(ctx, a, ShareVec{b, P, 0}, m_inv1, t0, t1, t2, T, 2 * n, lanes, nullptr));                      // mms = m_0 m_inv[1..]
    CZK_TRY(share_mul_launch(ctx, a, ShareVec{lanes, n, 1}, ShareVec{b + 4 * (n + 1), P, 1}, t0, t1, t2, T, 3 * n, nullptr, mms));   // batch_inv(mms): open(mms b)
    CZK_TRY(czk_fr_batch_inverse(ctx, mms, n, nullptr, inv, CZK_MEM_DEVICE));
    CZK_TRY(share_scale_launch(ctx, (unsigned)L, ShareVec{c + 4 * (n + 1), P, 1}, inv, run, (u64*)out, n, n));               // c / open, scaled by the running product
    return share_counters_read(ctx, out_bad, out_zero);
}
