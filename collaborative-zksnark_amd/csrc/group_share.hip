// group_share.hip -- products of a SHARED point and a SHARED scalar on device lanes, for BLS12-377 G1 / G2 on gfx950: GroupShare::scale
// (mpc-algebra/src/share/group.rs:70-109, SPDZ forms share/spdz.rs:385-446) for additive and SPDZ shares, and gsz20's group mult
// (share/gsz20/mod.rs:1112-1130) for GSZ shares, in the lanes form: every party's lanes are on this GPU, so an open is a sum (resp. an inverse
// DFT in the exponent) over lanes.  A proof needs three such products, so n is small and what counts is how many 256-step double-and-add chains
// run one after the other: each call here runs ONE chain deep, whatever the scheme.
//   joint_chain: [a] P + [b] Q as ONE double-and-add: one doubling per bit and one complete addition of P, Q or P + Q per bit, selected.  The
//     table entry P + Q may be a doubling or infinity (P = +-Q): curve.h's jac_add is complete.  Scalar limbs and table entries are selected, not
//     indexed (a register array indexed by a loop counter goes to scratch).
//   k_group_scale: one thread per (lane, element) output, plus -- for SPDZ -- one thread per element for the MAC checks, all in the same launch.
//     Every thread sums the lanes it needs itself (sx = open(s + x), oy = open(o + y): 2 * parties mixed additions against the 256 doublings of
//     its chain), so nothing waits for an opening kernel.  Output thread: z_l + [-oy] x_l + [k_l oy - y_l] sx.  Check thread: [alpha] sx - sum of the
//     mac lanes of s + x must be infinity (alpha = the sum of the mac shares: the points are in the prime-order subgroup, scalars combine mod r),
//     alpha oy - sum of the mac lanes of o + y must be 0.
//   k_gsz_group_mask: one thread per (coefficient, party, element): W_c,j = [m_c,j x_j] Y_j + [m_c,j] R2_j with m_0,j = 1 / P (so that V = sum_j W_0,j)
//     and m_c,j = (1 / P) w^(-j (2 d + c)) for the coefficients above the king's bound: the inverse DFT's scalars go INTO the parties' chains instead
//     of a second chain on the king's side.
//   k_gsz_group_king: no chain: out_j = sum_j W_0,j - R_j per (party, element), and one thread per element adds up each high coefficient and counts.
//   the check (hadamard_check -> ip_check for group triples, :1132-1349): k_gcheck_hadamard, then per halving round k_gcheck_ip (both inner products,
//     block partials through LDS), k_gcheck_round (one block: the king's two opens, the coin, the parabola as ONE five-term chain per lane) and
//     k_gcheck_fold; k_gcheck_final does the end of :1317-1328 one chain deep.  3 R + 2 launches, nothing read back in between.
// Each product call: its kernels write Jacobian triples, launch_to_affine's shared batch normalisation writes the affine lanes, ONE read-back of the counter.
// Integer VALU code of field.h / curve.h with the Montgomery multiply out of line (-DCZK_NOINLINE_MUL), as point_ops.hip.
#include "call.h"

namespace czk {

constexpr unsigned GROUP_GSZ_MAX_PARTIES = 96;   // k_gsz_open's limit (share.hip)

__device__ __forceinline__ Fr gs_fr(const u64* base, size_t idx) { return fp_load<FrParams>(base + 4 * idx); }
template <class F>
__device__ __forceinline__ Jac<F> gs_point(const u64* pts, const uint8_t* inf, size_t idx) {
    if (inf && inf[idx]) return Jac<F>::zero();
    const Affine<F> a = aff_load<F>(pts + (size_t)GT<F>::AW * idx);
    return Jac<F>{a.x, a.y, F::one()};
}
template <class F>
__device__ __forceinline__ Jac<F> gs_neg(Jac<F> p) {
    p.y = f_neg(p.y);
    return p;
}

// [a] p + [b] q, a and b canonical (not Montgomery)
template <class F>
__device__ __forceinline__ Jac<F> joint_chain(const Jac<F>& p, const Jac<F>& q, const Fr& a, const Fr& b) {
    const Jac<F> pq = jac_add(p, q);
    Jac<F> acc = Jac<F>::zero();
#pragma unroll 1
    for (int limb = 7; limb >= 0; limb--) {
        u32 wa = 0, wb = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) wa = j == limb ? a.l[j] : wa, wb = j == limb ? b.l[j] : wb;
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = jac_double(acc);
            const u32 sel = ((wa >> bit) & 1u) | (((wb >> bit) & 1u) << 1);
            if (sel) acc = jac_add(acc, sel == 1 ? p : sel == 2 ? q : pq);
        }
    }
    return acc;
}

struct GroupScaleArgs {
    const u64 *s, *o, *tx, *ty, *tz;             // L lanes of n points (s, tx, tz) / Montgomery Fr (o, ty)
    const uint8_t *s_inf, *tx_inf, *tz_inf;      // L n infinity bytes each; null: no point is infinity
    size_t n;
    unsigned lpp, parties;
    Fr alpha;                                    // the MAC key: sum of the parties' shares
    const u64* mac_share;                        // the parties' shares, DEVICE (an array in the argument block would be copied to scratch by every lane)
};

template <class F>
__global__ __launch_bounds__(128) void k_group_scale(GroupScaleArgs a, u64* out_jac, unsigned long long* bad) {
    constexpr int JW = GT<F>::JW;
    const unsigned L = a.lpp * a.parties;
    const bool spdz = a.lpp == 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)(L + (spdz ? 1u : 0u)) * a.n) return;
    const unsigned v = (unsigned)(idx / a.n);
    const size_t i = idx % a.n;
    // open(s + x) and open(o + y): the sh lanes
    Jac<F> sx = Jac<F>::zero();
    Fr oy = Fr::zero();
#pragma unroll 1
    for (unsigned ln = 0; ln < L; ln += a.lpp) {
        const size_t at = (size_t)ln * a.n + i;
        sx = jac_add(jac_add(sx, gs_point<F>(a.s, a.s_inf, at)), gs_point<F>(a.tx, a.tx_inf, at));
        oy = fp_add(oy, fp_add(gs_fr(a.o, at), gs_fr(a.ty, at)));
    }
    // both kinds of thread run the SAME chain, [ca] p + [cb] q, and add z: an output thread z_l + [-oy] x_l + [k_l oy - y_l] sx, a check thread
    // [alpha] sx - (the sum of the mac lanes of s + x)
    const size_t at = (size_t)v * a.n + i;
    Jac<F> p, q, z;
    Fr ca, cb, mo = Fr::zero();
    if (v < L) {
        // k_l: 1 on the king's sh lane (share/add.rs shift), mac_share_j on party j's mac lane (share/spdz.rs:430-438), 0 elsewhere
        const Fr k = spdz && (v & 1) ? gs_fr(a.mac_share, v >> 1) : v == 0 ? Fr::one() : Fr::zero();
        p = gs_point<F>(a.tx, a.tx_inf, at), q = sx, z = gs_point<F>(a.tz, a.tz_inf, at);
        ca = fp_into_repr(fp_neg(oy)), cb = fp_into_repr(fp_sub(fp_mul(k, oy), gs_fr(a.ty, at)));
    } else {   // the element's MAC checks (share/spdz.rs:392-402 for the point, :176-183 for the scalar)
        z = Jac<F>::zero();
#pragma unroll 1
        for (unsigned ln = 1; ln < L; ln += 2) {
            const size_t am = (size_t)ln * a.n + i;
            z = jac_add(jac_add(z, gs_point<F>(a.s, a.s_inf, am)), gs_point<F>(a.tx, a.tx_inf, am));
            mo = fp_add(mo, fp_add(gs_fr(a.o, am), gs_fr(a.ty, am)));
        }
        p = sx, q = Jac<F>::zero(), z = gs_neg(z);
        ca = fp_into_repr(a.alpha), cb = Fr::zero();
    }
    const Jac<F> r = jac_add(joint_chain(p, q, ca, cb), z);
    if (v < L) jac_store<F>(out_jac + (size_t)JW * at, r);
    else if (!r.is_zero() || !fp_sub(fp_mul(a.alpha, oy), mo).is_zero()) atomicAdd(bad, 1ull);
}

struct GroupGszArgs {
    const u64 *x, *y, *gr, *gr2;                 // P lanes of n Montgomery Fr (x) / points (y, gr, gr2)
    const uint8_t *y_inf, *gr_inf, *gr2_inf;
    const u64* tab;                              // size_inv w^(-j k), P x P (ctx->share_tab)
    u64* w;                                      // (1 + nchk) x P x n Jacobian triples
    size_t n;
    unsigned P, first_high, nchk;                // coefficients first_high .. first_high + nchk - 1 = P - 1 must vanish
};

template <class F>
__global__ __launch_bounds__(128) void k_gsz_group_mask(GroupGszArgs a) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = (size_t)a.P * a.n;
    if (idx >= (size_t)(1 + a.nchk) * per) return;
    const unsigned c = (unsigned)(idx / per), j = (unsigned)((idx % per) / a.n);
    const size_t at = idx % per;                 // j * n + i
    const Fr m = gs_fr(a.tab, c ? (size_t)j * a.P + a.first_high + (c - 1) : 0);
    const Jac<F> r = joint_chain(gs_point<F>(a.y, a.y_inf, at), gs_point<F>(a.gr2, a.gr2_inf, at), fp_into_repr(fp_mul(m, gs_fr(a.x, at))), fp_into_repr(m));
    jac_store<F>(a.w + (size_t)GT<F>::JW * idx, r);
}

template <class F>
__global__ __launch_bounds__(128) void k_gsz_group_king(GroupGszArgs a, u64* out_jac, unsigned long long* bad) {
    constexpr int JW = GT<F>::JW;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = (size_t)a.P * a.n;
    if (idx >= per + (a.nchk ? a.n : 0)) return;
    const size_t i = idx % a.n;
    if (idx < per) {   // out_j = V - R_j, V = the king's opened value (he sends it to everyone, :1095-1101)
        Jac<F> v = Jac<F>::zero();
#pragma unroll 1
        for (unsigned j = 0; j < a.P; j++) v = jac_add(v, jac_load<F>(a.w + (size_t)JW * ((size_t)j * a.n + i)));
        jac_store<F>(out_jac + (size_t)JW * idx, jac_add(v, gs_neg(gs_point<F>(a.gr, a.gr_inf, idx))));
        return;
    }
    bool high = false;   // the king's degree bound (open_degree_vec, :1070-1078)
#pragma unroll 1
    for (unsigned c = 1; c <= a.nchk; c++) {
        Jac<F> s = Jac<F>::zero();
#pragma unroll 1
        for (unsigned j = 0; j < a.P; j++) s = jac_add(s, jac_load<F>(a.w + (size_t)JW * ((size_t)c * per + (size_t)j * a.n + i)));
        if (!s.is_zero()) high = true;
    }
    if (high) atomicAdd(bad, 1ull);
}

// ---- the product check for group triples: hadamard_check -> ip_check -> ip_compress / ip_compute (:1132-1349) ------------------------------------
// sum_m [s_m] p_m as one double-and-add: one doubling per bit, up to M additions per bit (M is small: no table of subsets)
template <class F, int M>
__device__ __forceinline__ Jac<F> multi_chain(const Jac<F> (&p)[M], const Fr (&s)[M]) {
    Jac<F> acc = Jac<F>::zero();
#pragma unroll 1
    for (int limb = 7; limb >= 0; limb--) {
        u32 w[M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            w[m] = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) w[m] = j == limb ? s[m].l[j] : w[m];
        }
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = jac_double(acc);
#pragma unroll
            for (int m = 0; m < M; m++)
                if ((w[m] >> bit) & 1u) acc = jac_add(acc, p[m]);
        }
    }
    return acc;
}
template <class F>
__device__ __forceinline__ Jac<F> single_chain(const Jac<F>& p, const Fr& a) {
    return joint_chain(p, Jac<F>::zero(), a, Fr::zero());
}

// the sum of acc over the block's 128 threads, on thread 0; lds: 128 Jacobian triples
template <class F>
__device__ __forceinline__ Jac<F> gs_block_sum(Jac<F> acc, u64* lds) {
    constexpr int JW = GT<F>::JW;
    const unsigned t = threadIdx.x;
    u64* mine = lds + (size_t)JW * t;
#pragma unroll 1
    for (unsigned s = 64; s; s >>= 1) {
        if (t >= s && t < 2 * s) jac_store<F>(mine, acc);
        __syncthreads();
        if (t < s) acc = jac_add(acc, jac_load<F>(mine + (size_t)JW * s));
        __syncthreads();
    }
    return acc;
}

struct GroupCheckArgs {
    const u64 *gr, *gr2;                  // group doubles: P lanes of GD points
    const uint8_t *gr_inf, *gr2_inf;
    size_t GD;
    const u64 *fr, *fr2;                  // field doubles: P lanes of 2 Fr
    const u64* rands;                     // P lanes of Rn Fr
    size_t Rn;
    const u64* tab;                       // size_inv w^(-j k)
    unsigned P, degree;
    const u64 *xs, *zs;                   // the caller's xs (P lanes of n Fr) and zs (points)
    const uint8_t* zs_inf;
    size_t n;
    u64* xw;                              // r^i x_i, folded in place: P lanes, n apart
    const u64* y;                         // the current ys: the caller's affine points (y_jac = 0, lanes n apart) or yw
    const uint8_t* y_inf;
    size_t ystride;
    int y_jac;
    u64* yw;                              // folded ys: P lanes of Jacobian triples, ywstride apart
    size_t ywstride;
    u64* hpart;                           // k_gcheck_hadamard's block partials: P x g0
    unsigned g0;
    u64* part;                            // k_gcheck_ip's block partials: 2 P x g
    unsigned g;
    unsigned* flag;                       // set when the hadamard coin exceeds its bound (zeroed by the host)
    u64 *ip, *coin, *sc;                  // the running inner product (P triples), the latest coin, the single-block kernels' scratch triples
    size_t d0, r0;                        // the first group double / random share the kernel consumes
    size_t m, h;                          // the round's length and half
    int first;                            // the running inner product is still hpart
    Fr inv2;
};
template <class F>
__device__ __forceinline__ Jac<F> gc_y(const GroupCheckArgs& a, unsigned lane, size_t i) {
    const size_t at = (size_t)lane * a.ystride + i;
    return a.y_jac ? jac_load<F>(a.y + (size_t)GT<F>::JW * at) : gs_point<F>(a.y, a.y_inf, at);
}
__device__ __forceinline__ Fr gc_rand(const GroupCheckArgs& a, unsigned lane, size_t k) { return gs_fr(a.rands, (size_t)lane * a.Rn + k); }
template <class F>
__device__ __forceinline__ Jac<F> gc_gr(const GroupCheckArgs& a, unsigned lane, size_t k) { return gs_point<F>(a.gr, a.gr_inf, (size_t)lane * a.GD + k); }
template <class F>
__device__ __forceinline__ Jac<F> gc_gr2(const GroupCheckArgs& a, unsigned lane, size_t k) { return gs_point<F>(a.gr2, a.gr2_inf, (size_t)lane * a.GD + k); }

// open_degree_vec of the field (:440-459) by the whole block: vals[P] in LDS, written and synchronised -> p(0) on every thread; *bad = 1 when a
// coefficient above `bound` is non-zero.  `slot` and `bad` belong to this open alone.
__device__ __forceinline__ Fr gc_field_open(const Fr* vals, unsigned P, unsigned bound, const u64* tab, Fr* slot, unsigned* bad) {
    const unsigned k = threadIdx.x;
    if (k < P && (k == 0 || k > bound)) {
        Fr c = Fr::zero();
        for (unsigned j = 0; j < P; j++) c = fp_add(c, fp_mul(vals[j], gs_fr(tab, (size_t)j * P + k)));
        if (k == 0) *slot = c;
        else if (!c.is_zero()) atomicOr(bad, 1u);
    }
    __syncthreads();
    return *slot;
}

// hadamard_check's loop (:1339-1347): the coin rho opened by every thread for itself (P additions), xw_i = rho^i x_i, and the block's share of
// sum_i [rho^i] Z_i per lane.  Grid (blocks over i, lane); one chain per thread.
template <class F>
__global__ __launch_bounds__(128) void k_gcheck_hadamard(GroupCheckArgs a) {
    constexpr int JW = GT<F>::JW;
    __shared__ __align__(16) u64 lds[128 * JW];
    const unsigned lane = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
    Fr s = Fr::zero();
    for (unsigned j = 0; j < a.P; j++) s = fp_add(s, gc_rand(a, j, 0));
    const Fr rho = fp_mul(gs_fr(a.tab, 0), s);
    if (blockIdx.x == 0 && lane == 0 && threadIdx.x > a.degree && threadIdx.x < a.P) {   // the coin's own degree bound
        Fr c = Fr::zero();
        for (unsigned j = 0; j < a.P; j++) c = fp_add(c, fp_mul(gc_rand(a, j, 0), gs_fr(a.tab, (size_t)j * a.P + threadIdx.x)));
        if (!c.is_zero()) atomicOr(a.flag, 1u);   // (added to cnt[0] by the last kernel)
    }
    Jac<F> acc = Jac<F>::zero();
    if (i < a.n) {
        const Fr p = fp_pow_u64(rho, (u64)i);
        const size_t at = (size_t)lane * a.n + i;
        fp_store<FrParams>(a.xw + 4 * at, fp_mul(p, gs_fr(a.xs, at)));
        acc = single_chain(gs_point<F>(a.zs, a.zs_inf, at), fp_into_repr(p));
    }
    acc = gs_block_sum<F>(acc, lds);
    if (threadIdx.x == 0) jac_store<F>(a.hpart + (size_t)JW * ((size_t)lane * a.g0 + blockIdx.x), acc);
}

// one round's two inner products (ip_compute, :1132-1155, for ip_l and for ip3 of :1231): grid (blocks over i < h, 2 P): blockIdx.y < P: the block's
// share of sum [xl] Yl; else of sum [2 xr - xl](2 Yr - Yl).  An odd length reads a zero scalar and an infinite point past its end.
template <class F>
__global__ __launch_bounds__(128) void k_gcheck_ip(GroupCheckArgs a) {
    constexpr int JW = GT<F>::JW;
    __shared__ __align__(16) u64 lds[128 * JW];
    const unsigned which = blockIdx.y / a.P, lane = blockIdx.y % a.P;
    const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
    Jac<F> acc = Jac<F>::zero();
    if (i < a.h) {
        const bool right = i + a.h < a.m;
        const Fr xl = gs_fr(a.xw, (size_t)lane * a.n + i);
        Jac<F> y = gc_y<F>(a, lane, i);
        Fr x = xl;
        if (which) {
            const Fr xr = right ? gs_fr(a.xw, (size_t)lane * a.n + i + a.h) : Fr::zero();
            const Jac<F> yr = right ? gc_y<F>(a, lane, i + a.h) : Jac<F>::zero();
            y = jac_add(jac_double(yr), gs_neg(y)), x = fp_sub(fp_dbl(xr), xl);
        }
        acc = single_chain(y, fp_into_repr(x));
    }
    acc = gs_block_sum<F>(acc, lds);
    if (threadIdx.x == 0) jac_store<F>(a.part + (size_t)JW * ((size_t)blockIdx.y * a.g + blockIdx.x), acc);
}

// one block per round: the king's opens of ip_l + r2 and ip3 + r2 in the exponent, the round's coin, ip_r = ip - ip_l and the parabola through
// (1, ip_l), (2, ip_r), (3, ip3) at the coin (:1253-1273).  With S = the sum over parties of what they send, the opened value is [1 / P] S, so
//   ip'_t = [(f1 - f2) / P] S_l + [f3 / P] S_3 + [f2] ip_t + [f2 - f1] R_l,t + [-f3] R_3,t        one five-term chain per lane
// and the degree bound's terms [w^(-j k) / P] (what party j sent) are one chain each, in the same pass.  sc: 2 P sent values, then the terms.
template <class F>
__global__ __launch_bounds__(256) void k_gcheck_round(GroupCheckArgs a, unsigned long long* cnt) {
    constexpr int JW = GT<F>::JW;
    __shared__ Fr vr[GROUP_GSZ_MAX_PARTIES], slot;
    __shared__ unsigned bad[3];
    const unsigned P = a.P, t = threadIdx.x;
    const unsigned first_high = 2 * a.degree + 1, nchk = first_high < P ? P - first_high : 0;
    u64* sent = a.sc;
    u64* terms = a.sc + (size_t)JW * 2 * P;
    if (t < 3) bad[t] = 0;
    for (unsigned w = t; w < 3 * P; w += 256) {
        const unsigned which = w / P, j = w % P;
        if (which < 2) {
            Jac<F> s = gc_gr2<F>(a, j, a.d0 + which);
            for (unsigned b = 0; b < a.g; b++) s = jac_add(s, jac_load<F>(a.part + (size_t)JW * ((size_t)w * a.g + b)));
            jac_store<F>(sent + (size_t)JW * w, s);
        } else if (a.first) {
            Jac<F> s = Jac<F>::zero();
            for (unsigned b = 0; b < a.g0; b++) s = jac_add(s, jac_load<F>(a.hpart + (size_t)JW * ((size_t)j * a.g0 + b)));
            jac_store<F>(a.ip + (size_t)JW * j, s);
        }
    }
    if (t < P) vr[t] = gc_rand(a, t, a.r0);
    __syncthreads();
    const Fr c = gc_field_open(vr, P, a.degree, a.tab, &slot, &bad[2]);
    const Fr size_inv = gs_fr(a.tab, 0);
    for (unsigned w = t; w < P + 2 * nchk * P; w += 256) {
        if (w < P) {
            const Fr one = Fr::one(), two = fp_dbl(one), three = fp_add(two, one);
            const Fr c1 = fp_sub(c, one), c2 = fp_sub(c, two), c3 = fp_sub(c, three);
            const Fr f1 = fp_mul(fp_mul(c2, c3), a.inv2), f2 = fp_neg(fp_mul(c1, c3)), f3 = fp_mul(fp_mul(c1, c2), a.inv2), f12 = fp_sub(f1, f2);
            Jac<F> p[5];
            p[0] = p[1] = Jac<F>::zero();
            for (unsigned j = 0; j < P; j++) {
                p[0] = jac_add(p[0], jac_load<F>(sent + (size_t)JW * j));
                p[1] = jac_add(p[1], jac_load<F>(sent + (size_t)JW * (P + j)));
            }
            p[2] = jac_load<F>(a.ip + (size_t)JW * w);
            p[3] = gc_gr<F>(a, w, a.d0);
            p[4] = gc_gr<F>(a, w, a.d0 + 1);
            const Fr s[5] = {fp_into_repr(fp_mul(f12, size_inv)), fp_into_repr(fp_mul(f3, size_inv)), fp_into_repr(f2), fp_into_repr(fp_neg(f12)),
                             fp_into_repr(fp_neg(f3))};
            jac_store<F>(a.ip + (size_t)JW * w, multi_chain<F, 5>(p, s));   // (lane w reads and writes its own triple only)
        } else {
            const unsigned e = w - P, which = e / (nchk * P), k = (e / P) % nchk, j = e % P;
            jac_store<F>(terms + (size_t)JW * e,
                         single_chain(jac_load<F>(sent + (size_t)JW * (which * P + j)), fp_into_repr(gs_fr(a.tab, (size_t)j * P + first_high + k))));
        }
    }
    __syncthreads();
    for (unsigned w = t; w < 2 * nchk; w += 256) {
        Jac<F> s = Jac<F>::zero();
        for (unsigned j = 0; j < P; j++) s = jac_add(s, jac_load<F>(terms + (size_t)JW * ((size_t)w * P + j)));
        if (!s.is_zero()) atomicOr(&bad[w / nchk], 1u);
    }
    __syncthreads();
    if (t == 0) {
        fp_store<FrParams>(a.coin, c);
        const unsigned nb = bad[0] + bad[1] + bad[2];
        if (nb) atomicAdd(cnt, (unsigned long long)nb);
    }
}

// ip_compress's lines at the coin (:1237-1252): x <- (xr - xl) c + (2 xl - xr) in place, Y <- [c](Yr - Yl) + (2 Yl - Yr) = [2 - c] Yl + [c - 1] Yr as one
// joint chain into yw.  Grid (blocks over i < h, lane).  In place is safe: thread i writes element i < h only and nobody else reads it.
template <class F>
__global__ __launch_bounds__(128) void k_gcheck_fold(GroupCheckArgs a) {
    const unsigned lane = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= a.h) return;
    const Fr c = gs_fr(a.coin, 0), one = Fr::one();
    const bool right = i + a.h < a.m;
    const size_t at = (size_t)lane * a.n + i;
    const Fr xl = gs_fr(a.xw, at), xr = right ? gs_fr(a.xw, at + a.h) : Fr::zero();
    const Jac<F> yl = gc_y<F>(a, lane, i), yr = right ? gc_y<F>(a, lane, i + a.h) : Jac<F>::zero();
    fp_store<FrParams>(a.xw + 4 * at, fp_add(fp_mul(fp_sub(xr, xl), c), fp_sub(fp_dbl(xl), xr)));
    jac_store<F>(a.yw + (size_t)GT<F>::JW * ((size_t)lane * a.ywstride + i),
                 joint_chain(yl, yr, fp_into_repr(fp_sub(fp_dbl(one), c)), fp_into_repr(fp_sub(c, one))));
}

// the end of ip_check (:1317-1328) on the one element left, one block.  Field side first: ip_r = mult(xr, yr), x_blind = mult(x, xr), xo = open(x_blind).
// Then every chain of the group side in ONE pass (xo is known before it starts, so [xo] open(y_blind) needs no second chain):
//   [xo] open(y_blind) = sum_j A_j - B    A_j = [xo yr_j / P] Y_j + [xo / P] gr2y_j    B = [xo / P] sum_j gry_j
//   open(ip_blind)     = sum_j C_j - E    C_j = [ip_r_j / P] ip_j + [1 / P] gr2z_j      E = [1 / P] sum_j grz_j
// and one chain per (bound, coefficient, party): the king's bound 2 d on what the parties send for the two group mults, the bound d on the two opens
// (coefficient k > 0 of V - gr_j is minus gr's).  cnt[1] = 1 when [x] y == z fails.
template <class F>
__global__ __launch_bounds__(256) void k_gcheck_final(GroupCheckArgs a, unsigned long long* cnt) {
    constexpr int JW = GT<F>::JW;
    __shared__ Fr va[GROUP_GSZ_MAX_PARTIES], ipr[GROUP_GSZ_MAX_PARTIES], slot[3];
    __shared__ unsigned bad[7];
    const unsigned P = a.P, t = threadIdx.x, jt = t < P ? t : 0;
    const unsigned hi2 = 2 * a.degree + 1, n2 = hi2 < P ? P - hi2 : 0, hi1 = a.degree + 1, n1 = hi1 < P ? P - hi1 : 0;
    if (t < 7) bad[t] = 0;
    if (a.first)
        for (unsigned j = t; j < P; j += 256) {
            Jac<F> s = Jac<F>::zero();
            for (unsigned b = 0; b < a.g0; b++) s = jac_add(s, jac_load<F>(a.hpart + (size_t)JW * ((size_t)j * a.g0 + b)));
            jac_store<F>(a.ip + (size_t)JW * j, s);
        }
    const Fr x = gs_fr(a.xw, (size_t)jt * a.n), xr = gc_rand(a, jt, a.r0), yr = gc_rand(a, jt, a.r0 + 1);
    if (t < P) va[t] = fp_add(fp_mul(xr, yr), gs_fr(a.fr2, (size_t)jt * 2));
    __syncthreads();
    const Fr m0 = fp_sub(gc_field_open(va, P, 2 * a.degree, a.tab, &slot[0], &bad[0]), gs_fr(a.fr, (size_t)jt * 2));
    if (t < P) va[t] = fp_add(fp_mul(x, xr), gs_fr(a.fr2, (size_t)jt * 2 + 1)), ipr[t] = m0;
    __syncthreads();
    const Fr xb = fp_sub(gc_field_open(va, P, 2 * a.degree, a.tab, &slot[1], &bad[1]), gs_fr(a.fr, (size_t)jt * 2 + 1));
    __syncthreads();
    if (t < P) va[t] = xb;
    __syncthreads();
    const Fr xo = gc_field_open(va, P, a.degree, a.tab, &slot[2], &bad[4]);
    const Fr size_inv = gs_fr(a.tab, 0), xop = fp_mul(xo, size_inv);
    const size_t dy = a.d0, dz = a.d0 + 1;
    const unsigned W0 = 2 * P + 2, W1 = W0 + 2 * n2 * P, W2 = W1 + 2 * n1 * P;
    for (unsigned w = t; w < W2; w += 256) {   // every item is [ca] p + [cb] q: one chain, one call site
        Jac<F> p, q = Jac<F>::zero();
        Fr ca, cb = Fr::zero();
        if (w < 2 * P) {                       // A_j, then C_j
            const unsigned z = w / P, j = w % P;
            const Fr m = z ? size_inv : xop;
            p = z ? jac_load<F>(a.ip + (size_t)JW * j) : gc_y<F>(a, j, 0), q = gc_gr2<F>(a, j, z ? dz : dy);
            ca = fp_mul(m, z ? ipr[j] : gc_rand(a, j, a.r0 + 1)), cb = m;
        } else if (w < W0) {                   // B, E
            const bool z = w == 2 * P + 1;
            p = Jac<F>::zero();
            for (unsigned j = 0; j < P; j++) p = jac_add(p, gc_gr<F>(a, j, z ? dz : dy));
            ca = z ? size_inv : xop;
        } else if (w < W1) {                   // the king's bound on what the parties send for the two group mults
            const unsigned e = w - W0, z = e / (n2 * P), k = (e / P) % n2, j = e % P;
            const Fr m = gs_fr(a.tab, (size_t)j * P + hi2 + k);
            p = z ? jac_load<F>(a.ip + (size_t)JW * j) : gc_y<F>(a, j, 0), q = gc_gr2<F>(a, j, z ? dz : dy);
            ca = fp_mul(m, z ? ipr[j] : gc_rand(a, j, a.r0 + 1)), cb = m;
        } else {                               // the bound on the two opens
            const unsigned e = w - W1, z = e / (n1 * P), k = (e / P) % n1, j = e % P;
            p = gc_gr<F>(a, j, z ? dz : dy);
            ca = gs_fr(a.tab, (size_t)j * P + hi1 + k);
        }
        const Jac<F> r = joint_chain(p, q, fp_into_repr(ca), fp_into_repr(cb));
        jac_store<F>(a.sc + (size_t)JW * w, r);
    }
    __syncthreads();
    for (unsigned w = t; w < 1 + 2 * n2 + 2 * n1; w += 256) {
        if (w == 0) {
            Jac<F> l = Jac<F>::zero(), z = Jac<F>::zero();
            for (unsigned j = 0; j < P; j++) {
                l = jac_add(l, jac_load<F>(a.sc + (size_t)JW * j));
                z = jac_add(z, jac_load<F>(a.sc + (size_t)JW * (P + j)));
            }
            l = jac_add(l, gs_neg(jac_load<F>(a.sc + (size_t)JW * (2 * P))));
            z = jac_add(z, gs_neg(jac_load<F>(a.sc + (size_t)JW * (2 * P + 1))));
            if (!jac_add(l, gs_neg(z)).is_zero()) atomicExch(cnt + 1, 1ull);
        } else {
            const unsigned e = w - 1;   // sums e of P terms each: 2 n2 of the king's bound, then 2 n1 of the opens'
            Jac<F> s = Jac<F>::zero();
            for (unsigned j = 0; j < P; j++) s = jac_add(s, jac_load<F>(a.sc + (size_t)JW * (W0 + (size_t)e * P + j)));
            if (!s.is_zero()) atomicOr(&bad[e < 2 * n2 ? 2 + e / n2 : 5 + (e - 2 * n2) / n1], 1u);
        }
    }
    __syncthreads();
    if (t == 0) {
        unsigned nb = *a.flag;   // the hadamard coin's bound
        for (unsigned s = 0; s < 7; s++) nb += bad[s];
        if (nb) atomicAdd(cnt, (unsigned long long)nb);
    }
}

static unsigned group_check_rounds(size_t n) {   // ceil(log2 n)
    unsigned r = 0;
    while (((size_t)1 << r) < n) r++;
    return r;
}

static int group_share_head(czk_ctx* ctx, const char* what, int group, uint64_t* out_bad) {
    if (!ctx) return CZK_ERR_ARG;
    if (!out_bad) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null count output");
    *out_bad = 0;
    return check_group(ctx, group);
}

}  // namespace czk

using namespace czk;

extern "C" int czk_gsz_group_material_counts(int op, size_t n, size_t* group_doubles, size_t* field_doubles, size_t* rands) {
    if (!group_doubles || !field_doubles || !rands) return CZK_ERR_ARG;
    *group_doubles = *field_doubles = *rands = 0;
    if (n > ((size_t)1 << 58)) return CZK_ERR_SIZE;
    if (op == CZK_GSZ_GROUP_OP_MUL) {
        *group_doubles = n;
        return CZK_OK;
    }
    if (op == CZK_GSZ_GROUP_OP_PRODUCT_CHECK) {
        if (n) *group_doubles = 2 * (size_t)group_check_rounds(n) + 2, *field_doubles = 2, *rands = (size_t)group_check_rounds(n) + 3;
        return CZK_OK;
    }
    return CZK_ERR_ARG;
}

extern "C" int czk_gsz_group_product_check(czk_ctx* ctx, int group, size_t parties, unsigned degree, const uint64_t* xs, const uint64_t* ys, const uint8_t* ys_inf,
                                           const uint64_t* zs, const uint8_t* zs_inf, size_t n, const uint64_t* gr, const uint8_t* gr_inf, const uint64_t* gr2,
                                           const uint8_t* gr2_inf, const uint64_t* fr, const uint64_t* fr2, const uint64_t* rands, uint64_t* out_ok,
                                           uint64_t* out_bad) {
    const char* what = "czk_gsz_group_product_check";
    CZK_TRY(group_share_head(ctx, what, group, out_bad));
    if (!out_ok) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null result output");
    *out_ok = 1;   // no triples: nothing to refute
    if (parties > GROUP_GSZ_MAX_PARTIES) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more than 96 parties");
    u64 dom[12];
    CZK_TRY(czk_share_domain_constants(ctx, parties, dom));   // CZK_ERR_SIZE: no share domain of that size
    if (!n) return CZK_OK;
    if (!xs || !ys || !zs || !gr || !gr2 || !fr || !fr2 || !rands) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    if (n >> 32) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more than 2^32 - 1 triples");
    const unsigned P = (unsigned)parties, R = group_check_rounds(n), d = degree < P ? degree : P;
    const size_t jw = group == CZK_G1 ? 18 : 36, h0 = (n + 1) / 2;
    const unsigned g0 = (unsigned)((n + 127) / 128), g1 = (unsigned)((h0 + 127) / 128);
    const unsigned n2 = 2 * d + 1 < P ? P - 2 * d - 1 : 0, n1 = d + 1 < P ? P - d - 1 : 0;
    const size_t sc_triples = (size_t)2 * P + 2 + (size_t)2 * (n2 + n1) * P;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CZK_TRY(gsz_open_table(ctx, parties));
    StageHold ws(ctx);
    // u64 words: xw | coin | flag (padded) | yw | hpart | part | ip | sc
    const size_t words = 4 * (size_t)P * n + 4 + 4 + jw * ((size_t)P * h0 + (size_t)P * g0 + (size_t)2 * P * g1 + P + sc_triples);
    CZK_TRY(ws.take(words * 8));
    GroupCheckArgs a;
    a.xw = (u64*)ws.b.p, a.coin = a.xw + 4 * (size_t)P * n, a.flag = (unsigned*)(a.coin + 4), a.yw = a.coin + 8, a.hpart = a.yw + jw * (size_t)P * h0;
    a.part = a.hpart + jw * (size_t)P * g0, a.ip = a.part + jw * (size_t)2 * P * g1, a.sc = a.ip + jw * P;
    a.gr = (const u64*)gr, a.gr2 = (const u64*)gr2, a.gr_inf = gr_inf, a.gr2_inf = gr2_inf, a.GD = (size_t)2 * R + 2;
    a.fr = (const u64*)fr, a.fr2 = (const u64*)fr2, a.rands = (const u64*)rands, a.Rn = (size_t)R + 3;
    a.tab = (const u64*)ctx->share_tab.p, a.P = P, a.degree = d;
    a.xs = (const u64*)xs, a.zs = (const u64*)zs, a.zs_inf = zs_inf, a.n = n;
    a.y = (const u64*)ys, a.y_inf = ys_inf, a.ystride = n, a.y_jac = 0, a.ywstride = h0;   // the first round reads y where the caller left it
    a.g0 = g0, a.g = 0, a.d0 = 0, a.r0 = 1, a.m = n, a.h = 0, a.first = 1;
    a.inv2 = fp_inv(fp_dbl(Fr::one()));
    CZK_TRY(share_counters(ctx));
    CZK_HIP(ctx, hipMemsetAsync(a.flag, 0, 8, ctx->stream));
    {
        ProfScope ps(ctx, "gsz_group_product_check");
        by_group(group, [&](auto tag) {
            using F = typename decltype(tag)::type;
            hipLaunchKernelGGL(k_gcheck_hadamard<F>, dim3(g0, P), dim3(128), 0, ctx->stream, a);
            for (unsigned round = 0; round < R; round++) {
                a.h = (a.m + 1) / 2;
                a.g = (unsigned)((a.h + 127) / 128);
                hipLaunchKernelGGL(k_gcheck_ip<F>, dim3(a.g, 2 * P), dim3(128), 0, ctx->stream, a);
                hipLaunchKernelGGL(k_gcheck_round<F>, dim3(1), dim3(256), 0, ctx->stream, a, ctx->share_cnt);
                hipLaunchKernelGGL(k_gcheck_fold<F>, dim3(a.g, P), dim3(128), 0, ctx->stream, a);
                a.y = a.yw, a.y_inf = nullptr, a.ystride = h0, a.y_jac = 1;
                a.m = a.h, a.d0 += 2, a.r0 += 1, a.first = 0;
            }
            hipLaunchKernelGGL(k_gcheck_final<F>, dim3(1), dim3(256), 0, ctx->stream, a, ctx->share_cnt);
        });
    }
    CZK_HIP(ctx, hipGetLastError());
    uint64_t failed = 0;
    CZK_TRY(share_counters_read(ctx, out_bad, &failed));   // the one read-back of the check
    *out_ok = failed ? 0 : 1;
    return CZK_OK;
}

extern "C" int czk_share_group_batch_scale(czk_ctx* ctx, int group, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* s, const uint8_t* s_inf,
                                           const uint64_t* o, const uint64_t* tx, const uint8_t* tx_inf, const uint64_t* ty, const uint64_t* tz,
                                           const uint8_t* tz_inf, uint64_t* out, uint8_t* out_inf, size_t n, uint64_t* out_bad) {
    const char* what = "czk_share_group_batch_scale";
    CZK_TRY(group_share_head(ctx, what, group, out_bad));
    if ((lpp != 1 && lpp != 2) || parties > 32) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": lpp is 1 (additive) or 2 (SPDZ), parties at most 32");
    if (!n || !parties) return CZK_OK;
    if (!s || !o || !tx || !ty || !tz || !out || !out_inf || (lpp == 2 && !mac_shares)) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    const size_t L = lpp * parties;
    if (n > ((size_t)1 << 36) / (L + 1)) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more outputs than one launch covers");
    GroupScaleArgs a;
    a.s = (const u64*)s, a.o = (const u64*)o, a.tx = (const u64*)tx, a.ty = (const u64*)ty, a.tz = (const u64*)tz;
    a.s_inf = s_inf, a.tx_inf = tx_inf, a.tz_inf = tz_inf;
    a.n = n, a.lpp = (unsigned)lpp, a.parties = (unsigned)parties;
    a.alpha = Fr::zero();
    for (size_t p = 0; lpp == 2 && p < parties; p++) a.alpha = fp_add(a.alpha, host_fr(mac_shares + 4 * p));
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    StageHold ms(ctx);
    a.mac_share = nullptr;
    if (lpp == 2) {
        CZK_TRY(ms.take(parties * 32));
        CZK_TRY(upload_pageable(ctx, ms.b.p, mac_shares, parties * 32));
        a.mac_share = (const u64*)ms.b.p;
    }
    CZK_TRY(share_counters(ctx));
    const size_t threads = (L + (lpp == 2 ? 1 : 0)) * n;
    CZK_TRY(launch_to_affine(ctx, "group_scale", what, group, L * n, (u64*)out, out_inf, [&](auto tag, u64* jac) {
        hipLaunchKernelGGL(k_group_scale<typename decltype(tag)::type>, grid_for(threads), dim3(128), 0, ctx->stream, a, jac, ctx->share_cnt);
    }));
    return share_counters_read(ctx, out_bad, nullptr);
}

extern "C" int czk_gsz_group_batch_mul(czk_ctx* ctx, int group, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* y, const uint8_t* y_inf,
                                       const uint64_t* gr, const uint8_t* gr_inf, const uint64_t* gr2, const uint8_t* gr2_inf, uint64_t* out, uint8_t* out_inf,
                                       size_t n, uint64_t* out_bad) {
    const char* what = "czk_gsz_group_batch_mul";
    CZK_TRY(group_share_head(ctx, what, group, out_bad));
    if (parties > GROUP_GSZ_MAX_PARTIES) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more than 96 parties");
    u64 dom[12];
    CZK_TRY(czk_share_domain_constants(ctx, parties, dom));   // CZK_ERR_SIZE: no share domain of that size
    if (!n) return CZK_OK;
    if (!x || !y || !gr || !gr2 || !out || !out_inf) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    const unsigned P = (unsigned)parties, d = degree < P ? degree : P;
    GroupGszArgs a;
    a.first_high = 2 * d + 1;
    a.nchk = a.first_high < P ? P - a.first_high : 0;
    if (n > ((size_t)1 << 36) / ((size_t)(1 + a.nchk) * P)) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more chains than one launch covers");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CZK_TRY(gsz_open_table(ctx, parties));
    const size_t jw = group == CZK_G1 ? 18 : 36, chains = (size_t)(1 + a.nchk) * P * n;
    StageHold ws(ctx);
    CZK_TRY(ws.take(chains * jw * 8));
    a.x = (const u64*)x, a.y = (const u64*)y, a.gr = (const u64*)gr, a.gr2 = (const u64*)gr2;
    a.y_inf = y_inf, a.gr_inf = gr_inf, a.gr2_inf = gr2_inf;
    a.tab = (const u64*)ctx->share_tab.p, a.w = (u64*)ws.b.p, a.n = n, a.P = P;
    CZK_TRY(share_counters(ctx));
    CZK_TRY(launch_to_affine(ctx, "gsz_group_mul", what, group, (size_t)P * n, (u64*)out, out_inf, [&](auto tag, u64* jac) {
        using F = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_gsz_group_mask<F>, grid_for(chains), dim3(128), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_gsz_group_king<F>, grid_for((size_t)P * n + (a.nchk ? n : 0)), dim3(128), 0, ctx->stream, a, jac, ctx->share_cnt);
    }));
    return share_counters_read(ctx, out_bad, nullptr);
}
