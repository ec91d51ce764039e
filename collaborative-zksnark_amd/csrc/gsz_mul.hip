// gsz_mul.hip -- products, inverses and running products of GSZ (Shamir) SHARED vectors and the product check that guards them: batch_mult
// (mpc-algebra/src/share/gsz20/mod.rs:559-594), batch_inv (:325-342), partial_products (:343-366), hadamard_check -> ip_check -> ip_compress /
// ip_compute (:596-808), in the lanes form: every party's lane is on this GPU (party j's lane holds p(w^j), w as in czk_share_domain_constants),
// so the king's open is an inverse DFT over lanes inside the thread that owns the element.  Bandwidth-bound passes over 32-byte elements.
//   k_gsz_mul: a whole batch_mult in ONE launch: d_j = x_j y_j + r2_j, coefficient 0 and the coefficients above 2 degree of its interpolating
//     polynomial (k_gsz_open's table), out_j = p(0) - r_j; each of x, y, r, r2 is read once, the lanes written once (3, 4, 6 and 8 parties keep d in
//     registers; any other count reads x, y, r2 again per coefficient).  Where the product only feeds an open (batch_inv's x r, partial_products'
//     mxm) the kernel opens it on the spot from the r lanes it already holds and writes n values instead of the lanes.
//   the check: k_gsz_coin (opens a random share to a device-resident coin), k_gsz_pow_tables, k_gsz_hadamard (x_i <- r^i x_i and per-lane partial
//     sums of r^i z_i), then per halving round k_gsz_ip (both inner products of the round in one pass, block partials), k_gsz_round (one block: the
//     king's two opens, the round's coin, the parabola through ip_l, ip_r, ip3) and k_gsz_fold; k_gsz_final does the four single-element products
//     and three opens of :775-786.  Nothing is read back between the launches: coins, the running inner product and the verdict stay on the device.
//   powers of the hadamard coin: per-byte power tables as in pow_tables.h, but built by a kernel that READS the coin from device memory (the host
//     never sees it before the final read-back).  A scan would need its own passes over n; a square-and-multiply per thread costs ~ 60 multiplies
//     against the 2 parties multiplies of an element's real work.  The tables are 1024 elements and every r^i is at most three multiplies.
//   one party per communicator (czk_net_gsz_*, host code in net_rounds.hip): the same protocols on ONE lane, the kernels cut where values cross the wire:
//     k_gsz_net_mask (d = x y + r2, to the king) and k_gsz_net_unmask (out = v - r, from his answer) for the products; for the check the one-lane
//     instantiations of k_gsz_hadamard / k_gsz_ip / k_gsz_fold and the single-block k_gsz_net_round_send / _round_recv / _final_send / _final_mid /
//     _verdict in place of k_gsz_round / k_gsz_final.  The king's side is k_gsz_open (share.hip) on the gathered elements.
// No scratch; LDS only for the block reductions and the single-block round kernels.  Counts go by vector atomics to ctx->share_cnt.
#include "czk_internal.h"
#include "pow_tables.h"

namespace czk {

constexpr size_t GSZ_MUL_BLOCKS_PER_CU = 8;   // grid-stride cap of every kernel here, on blocks of 256 threads
constexpr unsigned GSZ_MAX_PARTIES = 96;      // k_gsz_open's limit; the single-block kernels keep one value per party in LDS

__device__ __forceinline__ Fr gv_load(const ShareVec& v, unsigned lane, size_t i) {
    return fp_load<FrParams>(v.p + 4 * ((size_t)lane * v.lane_stride + i * v.elem_stride));
}
__device__ __forceinline__ Fr g_load(const u64* base, size_t idx) { return fp_load<FrParams>(base + 4 * idx); }
__device__ __forceinline__ void g_store(u64* base, size_t idx, const Fr& v) { fp_store<FrParams>(base + 4 * idx, v); }

struct GszMulArgs {
    ShareVec x, y, r, r2;
    const u64* tab;      // size_inv w^(-j k), parties x parties (ctx->share_tab)
    u64* out;            // parties lanes, out_stride apart; null: the product's shares are not written
    size_t out_stride;
    u64* open_out;       // non-null: the product is opened right here: n values, its degree check counted
    size_t n;
    unsigned parties, degree;
};

// LANES > 0: exactly that many parties, d (then r) in registers; LANES == 0: any number, the operands are read again per coefficient
template <unsigned LANES>
__global__ __launch_bounds__(256) void k_gsz_mul(GszMulArgs a, unsigned long long* bad) {
    const unsigned P = LANES ? LANES : a.parties;
    const Fr size_inv = g_load(a.tab, 0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (size_t)gridDim.x * blockDim.x) {
        Fr d[LANES ? LANES : 1];
        Fr s = Fr::zero();
#pragma unroll
        for (unsigned j = 0; j < P; j++) {
            const Fr dj = fp_add(fp_mul(gv_load(a.x, j, i), gv_load(a.y, j, i)), gv_load(a.r2, j, i));
            if (LANES) d[LANES ? j : 0] = dj;
            s = fp_add(s, dj);
        }
        const Fr v = fp_mul(size_inv, s);   // coefficient 0: every table entry of column 0 is size_inv
        unsigned nbad = 0;
        bool high = false;
        for (unsigned k = 2 * a.degree + 1; k < P; k++) {   // the king's degree bound on x y + r2 (open_degree_vec, :440-455)
            Fr c = Fr::zero();
#pragma unroll
            for (unsigned j = 0; j < P; j++) {
                const Fr dj = LANES ? d[LANES ? j : 0] : fp_add(fp_mul(gv_load(a.x, j, i), gv_load(a.y, j, i)), gv_load(a.r2, j, i));
                c = fp_add(c, fp_mul(dj, g_load(a.tab, (size_t)j * P + k)));
            }
            if (!c.is_zero()) high = true;
        }
        if (high) nbad++;
        Fr rs = Fr::zero();
#pragma unroll
        for (unsigned j = 0; j < P; j++) {
            const Fr rj = gv_load(a.r, j, i);
            if (LANES) d[LANES ? j : 0] = rj;
            rs = fp_add(rs, rj);
            if (a.out) g_store(a.out + 4 * (size_t)j * a.out_stride, i, fp_sub(v, rj));   // the king sends the opened value itself (:478, :509)
        }
        if (a.open_out) {   // open(v - r): coefficient 0 is v - r's, coefficient k > 0 is minus r's
            g_store(a.open_out, i, fp_sub(v, fp_mul(size_inv, rs)));
            high = false;
            for (unsigned k = a.degree + 1; k < P; k++) {
                Fr c = Fr::zero();
#pragma unroll
                for (unsigned j = 0; j < P; j++) c = fp_add(c, fp_mul(LANES ? d[LANES ? j : 0] : gv_load(a.r, j, i), g_load(a.tab, (size_t)j * P + k)));
                if (!c.is_zero()) high = true;
            }
            if (high) nbad++;
        }
        if (nbad) atomicAdd(bad, (unsigned long long)nbad);
    }
}

// ---- the product check ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fr gsz_wave_sum(Fr v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        Fr o;
#pragma unroll
        for (int w = 0; w < 8; w++) o.l[w] = __shfl_down(v.l[w], off, 64);
        v = fp_add(v, o);   // Fr addition is exact: the order is free
    }
    return v;
}
// the sum of v over the 256 threads of the block, on every thread; sm: 4 elements of LDS, free again on return
__device__ __forceinline__ Fr gsz_block_sum(const Fr& v, Fr* sm) {
    const Fr w = gsz_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = w;
    __syncthreads();
    const Fr t = fp_add(fp_add(sm[0], sm[1]), fp_add(sm[2], sm[3]));
    __syncthreads();
    return t;
}
// sum_b part[b * stride + q] over nblocks block partials, on every thread of the (one) block
__device__ __forceinline__ Fr gsz_sum_partials(const u64* part, unsigned nblocks, unsigned stride, unsigned q, Fr* sm) {
    Fr a = Fr::zero();
    for (unsigned b = threadIdx.x; b < nblocks; b += 256) a = fp_add(a, g_load(part, (size_t)b * stride + q));
    return gsz_block_sum(a, sm);
}
// open_degree_vec by the whole block: vals[P] in LDS (written and synchronised) -> p(0) on every thread; *bad = 1 when a coefficient above `bound`
// is non-zero.  Thread k computes coefficient k.  `slot` and `bad` belong to this open alone.
__device__ __forceinline__ Fr gsz_lds_open(const Fr* vals, unsigned P, unsigned bound, const u64* tab, Fr* slot, unsigned* bad) {
    const unsigned k = threadIdx.x;
    if (k < P && (k == 0 || k > bound)) {
        Fr c = Fr::zero();
        for (unsigned j = 0; j < P; j++) c = fp_add(c, fp_mul(vals[j], g_load(tab, (size_t)j * P + k)));
        if (k == 0) *slot = c;
        else if (!c.is_zero()) atomicOr(bad, 1u);
    }
    __syncthreads();
    return *slot;
}

// where the check's material lies: doubles (r, r2) `D` elements per lane, random shares `Rn` per lane
struct GszMaterial {
    const u64 *dr, *dr2, *rands;
    size_t D, Rn;
};
__device__ __forceinline__ Fr gsz_dr(const GszMaterial& m, unsigned lane, size_t k) { return g_load(m.dr, (size_t)lane * m.D + k); }
__device__ __forceinline__ Fr gsz_dr2(const GszMaterial& m, unsigned lane, size_t k) { return g_load(m.dr2, (size_t)lane * m.D + k); }
__device__ __forceinline__ Fr gsz_rand(const GszMaterial& m, unsigned lane, size_t k) { return g_load(m.rands, (size_t)lane * m.Rn + k); }

// coin() (:529-531): opens random share `r0` to *coin
__global__ __launch_bounds__(256) void k_gsz_coin(GszMaterial m, size_t r0, unsigned P, unsigned degree, const u64* tab, u64* coin, unsigned long long* cnt) {
    __shared__ Fr vals[GSZ_MAX_PARTIES], slot;
    __shared__ unsigned bad;
    if (threadIdx.x == 0) bad = 0;
    if (threadIdx.x < P) vals[threadIdx.x] = gsz_rand(m, threadIdx.x, r0);
    __syncthreads();
    const Fr c = gsz_lds_open(vals, P, degree, tab, &slot, &bad);
    if (threadIdx.x == 0) {
        g_store(coin, 0, c);
        if (bad) atomicAdd(cnt, 1ull);
    }
}

// T_j[b] = coin^(b 2^(8 j)) (pow_tables.h's layout), the coin read from device memory: 4 blocks of 256
__global__ __launch_bounds__(256) void k_gsz_pow_tables(u64* tab, const u64* coin) {
    Fr root = g_load(coin, 0);
    for (unsigned s = 0; s < 8 * blockIdx.x; s++) root = fp_sqr(root);
    g_store(tab, 256 * (size_t)blockIdx.x + threadIdx.x, fp_pow_u64(root, (u64)threadIdx.x));
}

// hadamard_check's loop (:604-612): xw_i = r^i x_i on every lane; part[block][lane] = the block's share of sum_i r^i z_i.  CH lanes per sweep.
template <unsigned CH>
__global__ __launch_bounds__(256) void k_gsz_hadamard(const u64* x, const u64* z, u64* xw, const u64* pow, unsigned nb, size_t n, unsigned P, u64* part) {
    __shared__ Fr sm[4];
    for (unsigned base = 0; base < P; base += CH) {
        Fr acc[CH];
#pragma unroll
        for (unsigned l = 0; l < CH; l++) acc[l] = Fr::zero();
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
            const Fr p = marlin_domain_element(pow, (u32)i, nb);
#pragma unroll
            for (unsigned l = 0; l < CH; l++)
                if (base + l < P) {
                    const size_t at = (size_t)(base + l) * n + i;
                    g_store(xw, at, fp_mul(p, g_load(x, at)));
                    acc[l] = fp_add(acc[l], fp_mul(p, g_load(z, at)));
                }
        }
#pragma unroll
        for (unsigned l = 0; l < CH; l++)
            if (base + l < P) {
                const Fr s = gsz_block_sum(acc[l], sm);
                if (threadIdx.x == 0) g_store(part, (size_t)blockIdx.x * P + base + l, s);
            }
    }
}

// one round's two inner products (:757, :690) in one pass over both halves: length m (an odd m is padded with a zero), half h;
// part[block][lane][0] = sum xl yl (ip_l), [1] = sum (2 xr - xl)(2 yr - yl) (ip3's operands are the lines through (1, xl), (2, xr) at 3)
template <unsigned CH>
__global__ __launch_bounds__(256) void k_gsz_ip(const u64* x, const u64* y, size_t stride, size_t m, size_t h, unsigned P, u64* part) {
    __shared__ Fr sm[4];
    for (unsigned base = 0; base < P; base += CH) {
        Fr al[CH], a3[CH];
#pragma unroll
        for (unsigned l = 0; l < CH; l++) al[l] = a3[l] = Fr::zero();
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < h; i += (size_t)gridDim.x * blockDim.x) {
            const bool right = i + h < m;
#pragma unroll
            for (unsigned l = 0; l < CH; l++)
                if (base + l < P) {
                    const size_t at = (size_t)(base + l) * stride + i;
                    const Fr xl = g_load(x, at), yl = g_load(y, at);
                    const Fr xr = right ? g_load(x, at + h) : Fr::zero(), yr = right ? g_load(y, at + h) : Fr::zero();
                    al[l] = fp_add(al[l], fp_mul(xl, yl));
                    a3[l] = fp_add(a3[l], fp_mul(fp_sub(fp_dbl(xr), xl), fp_sub(fp_dbl(yr), yl)));
                }
        }
#pragma unroll
        for (unsigned l = 0; l < CH; l++)
            if (base + l < P) {
                const Fr s0 = gsz_block_sum(al[l], sm), s1 = gsz_block_sum(a3[l], sm);
                if (threadIdx.x == 0) {
                    g_store(part, ((size_t)blockIdx.x * P + base + l) * 2, s0);
                    g_store(part, ((size_t)blockIdx.x * P + base + l) * 2 + 1, s1);
                }
            }
    }
}

struct GszRoundArgs {
    GszMaterial m;
    size_t d0, r0;          // the first double and random share this kernel consumes
    const u64* tab;
    const u64* part;        // k_gsz_ip's partials
    unsigned nblocks;
    const u64* ip_part;     // non-null: the running inner product is still k_gsz_hadamard's partials
    unsigned ip_blocks;
    u64 *ip, *coin;         // device state: the running inner product (parties elements) and the latest coin
    const u64 *x, *y;       // k_gsz_final: lanes `stride` apart, element 0
    size_t stride;
    unsigned P, degree;
    Fr inv2;
};

// the running inner product's lane j into vi[j] (LDS), by the whole block
__device__ __forceinline__ void gsz_load_ip(const GszRoundArgs& a, Fr* vi, Fr* sm) {
    if (a.ip_part) {
        for (unsigned j = 0; j < a.P; j++) {
            const Fr s = gsz_sum_partials(a.ip_part, a.ip_blocks, a.P, j, sm);
            if (threadIdx.x == 0) vi[j] = s;
        }
    } else if (threadIdx.x < a.P) {
        vi[threadIdx.x] = g_load(a.ip, threadIdx.x);
    }
    __syncthreads();
}

// one block per round: ip_compute's king steps for ip_l and ip3 (:802-807), the coin (:692), ip_r = ip - ip_l (:758-762) and the parabola through
// (1, ip_l), (2, ip_r), (3, ip3) at the coin (:717-731)
__global__ __launch_bounds__(256) void k_gsz_round(GszRoundArgs a, unsigned long long* cnt) {
    __shared__ Fr sm[4], va[GSZ_MAX_PARTIES], vb[GSZ_MAX_PARTIES], vr[GSZ_MAX_PARTIES], vi[GSZ_MAX_PARTIES], slot[3];
    __shared__ unsigned bad[3];
    const unsigned P = a.P, t = threadIdx.x;
    if (t < 3) bad[t] = 0;
    gsz_load_ip(a, vi, sm);
    for (unsigned j = 0; j < P; j++) {
        const Fr sl = gsz_sum_partials(a.part, a.nblocks, 2 * P, 2 * j, sm), s3 = gsz_sum_partials(a.part, a.nblocks, 2 * P, 2 * j + 1, sm);
        if (t == 0) va[j] = fp_add(sl, gsz_dr2(a.m, j, a.d0)), vb[j] = fp_add(s3, gsz_dr2(a.m, j, a.d0 + 1));
    }
    if (t < P) vr[t] = gsz_rand(a.m, t, a.r0);
    __syncthreads();
    const Fr vl = gsz_lds_open(va, P, 2 * a.degree, a.tab, &slot[0], &bad[0]);
    const Fr v3 = gsz_lds_open(vb, P, 2 * a.degree, a.tab, &slot[1], &bad[1]);
    const Fr c = gsz_lds_open(vr, P, a.degree, a.tab, &slot[2], &bad[2]);
    if (t < P) {
        const Fr one = Fr::one(), two = fp_dbl(one), three = fp_add(two, one);
        const Fr c1 = fp_sub(c, one), c2 = fp_sub(c, two), c3 = fp_sub(c, three);
        const Fr f1 = fp_mul(fp_mul(c2, c3), a.inv2), f2 = fp_neg(fp_mul(c1, c3)), f3 = fp_mul(fp_mul(c1, c2), a.inv2);
        const Fr ipl = fp_sub(vl, gsz_dr(a.m, t, a.d0)), ip3 = fp_sub(v3, gsz_dr(a.m, t, a.d0 + 1)), ipr = fp_sub(vi[t], ipl);
        g_store(a.ip, t, fp_add(fp_add(fp_mul(f1, ipl), fp_mul(f2, ipr)), fp_mul(f3, ip3)));
    }
    if (t == 0) {
        g_store(a.coin, 0, c);
        const unsigned nb = bad[0] + bad[1] + bad[2];
        if (nb) atomicAdd(cnt, (unsigned long long)nb);
    }
}

// ip_compress's lines at the coin (:696-711): x <- (xr - xl) c + (2 xl - xr), the same for y; in place is safe (thread i writes element i < h only)
__global__ __launch_bounds__(256) void k_gsz_fold(const u64* xs, u64* xd, const u64* ys, u64* yd, size_t stride, size_t m, size_t h, unsigned P, const u64* coin) {
    const Fr c = g_load(coin, 0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < h; i += (size_t)gridDim.x * blockDim.x) {
        const bool right = i + h < m;
        for (unsigned l = 0; l < P; l++) {
            const size_t at = (size_t)l * stride + i;
            const Fr xl = g_load(xs, at), yl = g_load(ys, at);
            const Fr xr = right ? g_load(xs, at + h) : Fr::zero(), yr = right ? g_load(ys, at + h) : Fr::zero();
            g_store(xd, at, fp_add(fp_mul(fp_sub(xr, xl), c), fp_sub(fp_dbl(xl), xr)));
            g_store(yd, at, fp_add(fp_mul(fp_sub(yr, yl), c), fp_sub(fp_dbl(yl), yr)));
        }
    }
}

// the end of ip_check (:775-786) on the one element left: four mults (king's bound 2 degree each), three opens, x y == z -> cnt[1] = 1 when it fails
__global__ __launch_bounds__(256) void k_gsz_final(GszRoundArgs a, unsigned long long* cnt) {
    __shared__ Fr sm[4], va[GSZ_MAX_PARTIES], vi[GSZ_MAX_PARTIES], slot[7];
    __shared__ unsigned bad[7];
    const unsigned P = a.P, t = threadIdx.x, j = t < P ? t : 0;
    if (t < 7) bad[t] = 0;
    gsz_load_ip(a, vi, sm);
    const Fr x = g_load(a.x, (size_t)j * a.stride), y = g_load(a.y, (size_t)j * a.stride), ip = vi[j];
    const Fr xr = gsz_rand(a.m, j, a.r0), yr = gsz_rand(a.m, j, a.r0 + 1);
    Fr m[4];
#pragma unroll
    for (unsigned s = 0; s < 4; s++) {   // mult(xr, yr), mult(x, xr), mult(y, yr), mult(ip, ip_r) in source order
        const Fr u = s == 0 ? xr : s == 1 ? x : s == 2 ? y : ip, w = s == 0 ? yr : s == 1 ? xr : s == 2 ? yr : m[0];
        if (t < P) va[t] = fp_add(fp_mul(u, w), gsz_dr2(a.m, j, a.d0 + s));
        __syncthreads();
        m[s] = fp_sub(gsz_lds_open(va, P, 2 * a.degree, a.tab, &slot[s], &bad[s]), gsz_dr(a.m, j, a.d0 + s));
    }
    Fr o[3];
#pragma unroll
    for (unsigned s = 0; s < 3; s++) {   // open(x_blind), open(y_blind), open(ip_blind)
        if (t < P) va[t] = m[s + 1];
        __syncthreads();
        o[s] = gsz_lds_open(va, P, a.degree, a.tab, &slot[4 + s], &bad[4 + s]);
    }
    if (t == 0) {
        if (!fp_sub(fp_mul(o[0], o[1]), o[2]).is_zero()) atomicExch(cnt + 1, 1ull);
        unsigned nb = 0;
        for (unsigned s = 0; s < 7; s++) nb += bad[s];
        if (nb) atomicAdd(cnt, (unsigned long long)nb);
    }
}

// ---- one party per communicator (czk_net_gsz_*, host code in net_rounds.hip): this party's ONE lane, the kernels split at the wire ---------------------
// what a party sends to the king in a batch_mult: d = x y + r2 (:570-577)
__global__ __launch_bounds__(256) void k_gsz_net_mask(ShareVec x, ShareVec y, const u64* r2, u64* d, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        g_store(d, i, fp_add(fp_mul(gv_load(x, 0, i), gv_load(y, 0, i)), g_load(r2, i)));
}
// ... and what it makes of the king's answer: out = v - r (:580-592)
__global__ __launch_bounds__(256) void k_gsz_net_unmask(const u64* v, const u64* r, u64* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        g_store(out, i, fp_sub(g_load(v, i), g_load(r, i)));
}

// k_gsz_round / k_gsz_final for one lane, cut where the values cross the wire.  `wire` leaves for the king, `king` is his answer, `opened` what a
// broadcast opened, `blind` the three blinded shares of the last open.
struct GszNetArgs {
    const u64 *dr, *dr2, *rands;   // this party's lanes of the material
    size_t d0, r0;                 // the first double and random share the step consumes
    const u64* part;               // k_gsz_ip<1>'s partials
    unsigned nblocks;
    const u64* ip_part;            // non-null: the running inner product is still k_gsz_hadamard<1>'s partials
    unsigned ip_blocks;
    u64 *ip, *coin;                // device state: this lane's running inner product and the latest coin
    u64* wire;
    const u64 *king, *opened;
    u64* blind;
    const u64 *x, *y;              // the one element left of each folded vector
    Fr inv2;
};
// before the king: ip_l + r2 and ip3 + r2 of the round (ip_compute, :802-804) from the block partials; the first round also settles the running inner product
__global__ __launch_bounds__(256) void k_gsz_net_round_send(GszNetArgs a) {
    __shared__ Fr sm[4];
    if (a.ip_part) {
        const Fr s = gsz_sum_partials(a.ip_part, a.ip_blocks, 1, 0, sm);
        if (threadIdx.x == 0) g_store(a.ip, 0, s);
    }
    const Fr sl = gsz_sum_partials(a.part, a.nblocks, 2, 0, sm), s3 = gsz_sum_partials(a.part, a.nblocks, 2, 1, sm);
    if (threadIdx.x == 0) {
        g_store(a.wire, 0, fp_add(sl, g_load(a.dr2, a.d0)));
        g_store(a.wire, 1, fp_add(s3, g_load(a.dr2, a.d0 + 1)));
    }
}
// after the king and the coin's open: ip_r = ip - ip_l (:758-762), the parabola through (1, ip_l), (2, ip_r), (3, ip3) at the coin (:717-731)
__global__ __launch_bounds__(64) void k_gsz_net_round_recv(GszNetArgs a) {
    if (threadIdx.x) return;
    const Fr c = g_load(a.opened, 0);
    const Fr one = Fr::one(), two = fp_dbl(one), three = fp_add(two, one);
    const Fr c1 = fp_sub(c, one), c2 = fp_sub(c, two), c3 = fp_sub(c, three);
    const Fr f1 = fp_mul(fp_mul(c2, c3), a.inv2), f2 = fp_neg(fp_mul(c1, c3)), f3 = fp_mul(fp_mul(c1, c2), a.inv2);
    const Fr ipl = fp_sub(g_load(a.king, 0), g_load(a.dr, a.d0)), ip3 = fp_sub(g_load(a.king, 1), g_load(a.dr, a.d0 + 1)), ipr = fp_sub(g_load(a.ip, 0), ipl);
    g_store(a.ip, 0, fp_add(fp_add(fp_mul(f1, ipl), fp_mul(f2, ipr)), fp_mul(f3, ip3)));
    g_store(a.coin, 0, c);
}
// the end (:775-786), first trip: mult(xr, yr), mult(x, xr), mult(y, yr) masked; n = 1 comes here with the hadamard partials still unsummed
__global__ __launch_bounds__(256) void k_gsz_net_final_send(GszNetArgs a) {
    __shared__ Fr sm[4];
    if (a.ip_part) {
        const Fr s = gsz_sum_partials(a.ip_part, a.ip_blocks, 1, 0, sm);
        if (threadIdx.x == 0) g_store(a.ip, 0, s);
    }
    if (threadIdx.x) return;
    const Fr x = g_load(a.x, 0), y = g_load(a.y, 0), xr = g_load(a.rands, a.r0), yr = g_load(a.rands, a.r0 + 1);
    g_store(a.wire, 0, fp_add(fp_mul(xr, yr), g_load(a.dr2, a.d0)));
    g_store(a.wire, 1, fp_add(fp_mul(x, xr), g_load(a.dr2, a.d0 + 1)));
    g_store(a.wire, 2, fp_add(fp_mul(y, yr), g_load(a.dr2, a.d0 + 2)));
}
// second trip: mult(ip, ip_r) masked, ip_r = the first trip's mult(xr, yr); the other two answers are the blinded x and y
__global__ __launch_bounds__(64) void k_gsz_net_final_mid(GszNetArgs a) {
    if (threadIdx.x) return;
    const Fr ipr = fp_sub(g_load(a.king, 0), g_load(a.dr, a.d0));
    g_store(a.wire, 0, fp_add(fp_mul(g_load(a.ip, 0), ipr), g_load(a.dr2, a.d0 + 3)));
    g_store(a.blind, 0, fp_sub(g_load(a.king, 1), g_load(a.dr, a.d0 + 1)));
    g_store(a.blind, 1, fp_sub(g_load(a.king, 2), g_load(a.dr, a.d0 + 2)));
}
// x y == z on the three opened values (:786): cnt[1] = 1 when it fails
__global__ __launch_bounds__(64) void k_gsz_net_verdict(const u64* opened, unsigned long long* cnt) {
    if (threadIdx.x) return;
    if (!fp_sub(fp_mul(g_load(opened, 0), g_load(opened, 1)), g_load(opened, 2)).is_zero()) atomicExch(cnt + 1, 1ull);
}

static unsigned gsz_mul_grid(czk_ctx* ctx, size_t n) {
    size_t blocks = (n + 255) / 256;
    const size_t cap = GSZ_MUL_BLOCKS_PER_CU * (size_t)ctx->num_cu;
    if (blocks > cap) blocks = cap;
    return blocks ? (unsigned)blocks : 1u;
}

// one batch_mult, enqueued: shares to `out` (may be null) and / or the opened product to `open_out` (may be null); doubles [d_first, d_first + a.n)
static int gsz_mul_launch(czk_ctx* ctx, GszMulArgs& a, ShareVec x, ShareVec y, const u64* dr, const u64* dr2, size_t D, size_t d_first, u64* out, u64* open_out) {
    a.x = x, a.y = y;
    a.r = ShareVec{dr + 4 * d_first, D, 1};
    a.r2 = ShareVec{dr2 + 4 * d_first, D, 1};
    a.tab = (const u64*)ctx->share_tab.p;
    a.out = out, a.out_stride = a.n, a.open_out = open_out;
    const dim3 g(gsz_mul_grid(ctx, a.n)), b(256);
    ProfScope ps(ctx, "gsz_mul");
    switch (a.parties) {
#define CZK_GSZ_MUL_CASE(LN)                                                                  \
    case LN:                                                                                  \
        hipLaunchKernelGGL(k_gsz_mul<LN>, g, b, 0, ctx->stream, a, ctx->share_cnt);           \
        break;
        CZK_GSZ_MUL_CASE(3)
        CZK_GSZ_MUL_CASE(4)
        CZK_GSZ_MUL_CASE(6)
        CZK_GSZ_MUL_CASE(8)
#undef CZK_GSZ_MUL_CASE
        default:
            hipLaunchKernelGGL(k_gsz_mul<0>, g, b, 0, ctx->stream, a, ctx->share_cnt);
    }
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

// The argument rules of the lanes-form calls; *work = there is something to do.  Uploads the share domain's table.
static int gsz_lanes_args(czk_ctx* ctx, const char* what, size_t parties, bool null_vec, size_t n, uint64_t* out_a, uint64_t* out_b, bool* work) {
    *work = false;
    if (!ctx) return CZK_ERR_ARG;
    if (!out_a || !out_b) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null result output");
    *out_a = *out_b = 0;
    if (parties > GSZ_MAX_PARTIES) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more than 96 parties");
    u64 dom[12];
    CZK_TRY(czk_share_domain_constants(ctx, parties, dom));   // CZK_ERR_SIZE: no share domain of that size
    if (!n) return CZK_OK;
    if (null_vec) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": null argument");
    if (n > ((size_t)1 << 52) / parties) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": the lane arrays' byte count overflows");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CZK_TRY(gsz_open_table(ctx, parties));
    *work = true;
    return CZK_OK;
}

static unsigned ceil_log2(size_t n) {
    unsigned r = 0;
    while (((size_t)1 << r) < n) r++;
    return r;
}

// lanes per sweep of the reducing kernels: the smallest instantiation that holds min(parties, 8)
#define CZK_GSZ_SWEEP(KERNEL, P, ...)                                              \
    do {                                                                           \
        if ((P) <= 3) hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__);                  \
        else if ((P) == 4) hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__);             \
        else if ((P) <= 6) hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__);             \
        else hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__);                           \
    } while (0)

// ---- the party side of czk_net_gsz_* (declared in czk_internal.h; every function enqueues on ctx->stream and returns) ------------------------------
// a party sweeps ONE lane: instantiations of their own (the lanes form never takes fewer than 3 lanes per sweep, and its kernels stay as they are)
constexpr auto k_gsz_hadamard_lane = k_gsz_hadamard<1>;
constexpr auto k_gsz_ip_lane = k_gsz_ip<1>;
int gsz_net_mask_launch(czk_ctx* ctx, ShareVec x, ShareVec y, const u64* r2, u64* d, size_t n) {
    ProfScope ps(ctx, "gsz_net_mask");
    hipLaunchKernelGGL(k_gsz_net_mask, dim3(gsz_mul_grid(ctx, n)), dim3(256), 0, ctx->stream, x, y, r2, d, n);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}
int gsz_net_unmask_launch(czk_ctx* ctx, const u64* v, const u64* r, u64* out, size_t n) {
    ProfScope ps(ctx, "gsz_net_unmask");
    hipLaunchKernelGGL(k_gsz_net_unmask, dim3(gsz_mul_grid(ctx, n)), dim3(256), 0, ctx->stream, v, r, out, n);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

size_t gsz_net_check_ws(czk_ctx* ctx, size_t n) { return 2 * n + 1024 + (size_t)3 * gsz_mul_grid(ctx, n) + 2 + 4 * GszNetCheck::SLOT; }

void gsz_net_check_carve(czk_ctx* ctx, GszNetCheck& c, u64* ws, size_t n, const u64* dr, const u64* dr2, const u64* rands) {
    const size_t g0 = gsz_mul_grid(ctx, n);
    c.n = n, c.dr = dr, c.dr2 = dr2, c.rands = rands;
    c.xw = ws, c.yw = c.xw + 4 * n, c.pow = c.yw + 4 * n, c.part = c.pow + 4 * 1024, c.hpart = c.part + 4 * 2 * g0, c.ip = c.hpart + 4 * g0, c.coin = c.ip + 4;
    c.wire = c.coin + 4, c.king = c.wire + 4 * GszNetCheck::SLOT, c.opened = c.king + 4 * GszNetCheck::SLOT, c.blind = c.opened + 4 * GszNetCheck::SLOT;
    c.ysrc = nullptr, c.m = n, c.d0 = 0, c.r0 = 1, c.ip_summed = false;
}

static GszNetArgs gsz_net_args(const GszNetCheck& c, unsigned ip_blocks) {
    GszNetArgs a;
    a.dr = c.dr, a.dr2 = c.dr2, a.rands = c.rands, a.d0 = c.d0, a.r0 = c.r0;
    a.part = c.part, a.nblocks = 0;
    a.ip_part = c.ip_summed ? nullptr : c.hpart, a.ip_blocks = ip_blocks;
    a.ip = c.ip, a.coin = c.coin, a.wire = c.wire, a.king = c.king, a.opened = c.opened, a.blind = c.blind;
    a.x = c.xw, a.y = c.ysrc;
    a.inv2 = fp_inv(fp_dbl(Fr::one()));
    return a;
}

// the hadamard coin is in c.coin: its power tables, then xw = r^i x_i and the partial sums of r^i z_i
int gsz_net_check_hadamard(czk_ctx* ctx, GszNetCheck& c, const u64* xs, const u64* ys, const u64* zs) {
    unsigned nb = 1;
    while (nb < 4 && ((c.n - 1) >> (8 * nb))) nb++;
    ProfScope ps(ctx, "gsz_net_check");
    hipLaunchKernelGGL(k_gsz_pow_tables, dim3(4), dim3(256), 0, ctx->stream, c.pow, (const u64*)c.coin);
    hipLaunchKernelGGL(k_gsz_hadamard_lane, dim3(gsz_mul_grid(ctx, c.n)), dim3(256), 0, ctx->stream, xs, zs, c.xw, (const u64*)c.pow, nb, c.n, 1u, c.hpart);
    CZK_HIP(ctx, hipGetLastError());
    c.ysrc = ys;   // the first round reads y where the caller left it
    return CZK_OK;
}
// a round's local pass: both inner products of this lane, c.wire[0, 2) = ip_l + r2, ip3 + r2
int gsz_net_check_round_send(czk_ctx* ctx, GszNetCheck& c) {
    const size_t h = (c.m + 1) / 2;
    const unsigned g = gsz_mul_grid(ctx, h);
    GszNetArgs a = gsz_net_args(c, gsz_mul_grid(ctx, c.n));
    a.nblocks = g;
    ProfScope ps(ctx, "gsz_net_check");
    hipLaunchKernelGGL(k_gsz_ip_lane, dim3(g), dim3(256), 0, ctx->stream, (const u64*)c.xw, c.ysrc, c.n, c.m, h, 1u, c.part);
    hipLaunchKernelGGL(k_gsz_net_round_send, dim3(1), dim3(256), 0, ctx->stream, a);
    CZK_HIP(ctx, hipGetLastError());
    c.ip_summed = true;
    return CZK_OK;
}
// c.king[0, 2) and c.opened[0] (the round's coin) have arrived: the new running inner product, the fold; on to the next round's material
int gsz_net_check_round_recv(czk_ctx* ctx, GszNetCheck& c) {
    const size_t h = (c.m + 1) / 2;
    const GszNetArgs a = gsz_net_args(c, 0);
    ProfScope ps(ctx, "gsz_net_check");
    hipLaunchKernelGGL(k_gsz_net_round_recv, dim3(1), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_gsz_fold, dim3(gsz_mul_grid(ctx, h)), dim3(256), 0, ctx->stream, (const u64*)c.xw, c.xw, c.ysrc, c.yw, c.n, c.m, h, 1u, (const u64*)c.coin);
    CZK_HIP(ctx, hipGetLastError());
    c.ysrc = c.yw, c.m = h, c.d0 += 2, c.r0 += 1;
    return CZK_OK;
}
// the end: step 0 -> c.wire[0, 3); step 1 (c.king[0, 3) arrived) -> c.wire[0], c.blind[0, 2); step 2 (c.king[0] arrived) -> c.blind[2];
// step 3 (c.opened[0, 3) arrived) -> the verdict in ctx->share_cnt[1]
int gsz_net_check_final(czk_ctx* ctx, GszNetCheck& c, int step) {
    const GszNetArgs a = gsz_net_args(c, gsz_mul_grid(ctx, c.n));
    ProfScope ps(ctx, "gsz_net_check");
    if (step == 0) {
        hipLaunchKernelGGL(k_gsz_net_final_send, dim3(1), dim3(256), 0, ctx->stream, a);
        c.ip_summed = true;
    } else if (step == 1) {
        hipLaunchKernelGGL(k_gsz_net_final_mid, dim3(1), dim3(64), 0, ctx->stream, a);
    } else if (step == 2) {
        hipLaunchKernelGGL(k_gsz_net_unmask, dim3(1), dim3(256), 0, ctx->stream, (const u64*)c.king, c.dr + 4 * (c.d0 + 3), c.blind + 4 * 2, (size_t)1);
    } else {
        hipLaunchKernelGGL(k_gsz_net_verdict, dim3(1), dim3(64), 0, ctx->stream, (const u64*)c.opened, ctx->share_cnt);
    }
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

}  // namespace czk

using namespace czk;

extern "C" int czk_gsz_material_counts(int op, size_t n, size_t* doubles, size_t* rands) {
    if (!doubles || !rands) return CZK_ERR_ARG;
    *doubles = *rands = 0;
    if (n > ((size_t)1 << 58)) return CZK_ERR_SIZE;
    const size_t R = n ? ceil_log2(n) : 0;
    switch (op) {
        case CZK_GSZ_OP_MUL: *doubles = n; return CZK_OK;
        case CZK_GSZ_OP_INV: *doubles = n, *rands = n; return CZK_OK;
        case CZK_GSZ_OP_PARTIAL_PRODUCTS: *doubles = n ? 5 * n + 1 : 0, *rands = n ? 3 * n + 2 : 0; return CZK_OK;
        case CZK_GSZ_OP_PRODUCT_CHECK: *doubles = n ? 2 * R + 4 : 0, *rands = n ? R + 3 : 0; return CZK_OK;
    }
    return CZK_ERR_ARG;
}

extern "C" int czk_gsz_share_batch_mul(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* y, const uint64_t* doubles_r,
                                       const uint64_t* doubles_r2, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero) {
    bool work;
    CZK_TRY(gsz_lanes_args(ctx, "czk_gsz_share_batch_mul", parties, !x || !y || !doubles_r || !doubles_r2 || !out, n, out_bad, out_zero, &work));
    if (!work) return CZK_OK;
    GszMulArgs a;
    a.n = n, a.parties = (unsigned)parties, a.degree = degree < parties ? degree : (unsigned)parties;
    CZK_TRY(share_counters(ctx));
    CZK_TRY(gsz_mul_launch(ctx, a, ShareVec{(const u64*)x, n, 1}, ShareVec{(const u64*)y, n, 1}, (const u64*)doubles_r, (const u64*)doubles_r2, n, 0, (u64*)out, nullptr));
    return share_counters_read(ctx, out_bad, out_zero);
}

// batch_inv (:325-342) of `cnt` elements, enqueued: rs = rands [r_first, ..), doubles [d_first, ..); v / vinv: cnt elements of workspace each;
// out_l = rs_l / open(x rs) (times prefix, when given)
static int gsz_inv_enqueue(czk_ctx* ctx, GszMulArgs& a, ShareVec x, const u64* dr, const u64* dr2, size_t D, size_t d_first, const u64* rands, size_t Rn, size_t r_first,
                           u64* v, u64* vinv, const u64* prefix, u64* out, size_t out_stride, size_t cnt) {
    const ShareVec rs{rands + 4 * r_first, Rn, 1};
    a.n = cnt;
    CZK_TRY(gsz_mul_launch(ctx, a, x, rs, dr, dr2, D, d_first, nullptr, v));   // open(batch_mult(x, rs)) in one launch
    CZK_TRY(czk_fr_batch_inverse(ctx, v, cnt, nullptr, vinv, CZK_MEM_DEVICE));
    return share_scale_launch(ctx, a.parties, rs, vinv, prefix, out, out_stride, cnt);
}

extern "C" int czk_gsz_share_batch_inv(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                                       const uint64_t* rands, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero) {
    bool work;
    CZK_TRY(gsz_lanes_args(ctx, "czk_gsz_share_batch_inv", parties, !x || !doubles_r || !doubles_r2 || !rands || !out, n, out_bad, out_zero, &work));
    if (!work) return CZK_OK;
    StageHold ws(ctx);
    CZK_TRY(ws.take(2 * n * 32));
    u64 *v = (u64*)ws.b.p, *vinv = v + 4 * n;
    GszMulArgs a;
    a.parties = (unsigned)parties, a.degree = degree < parties ? degree : (unsigned)parties;
    CZK_TRY(share_counters(ctx));
    CZK_TRY(gsz_inv_enqueue(ctx, a, ShareVec{(const u64*)x, n, 1}, (const u64*)doubles_r, (const u64*)doubles_r2, n, 0, (const u64*)rands, n, 0, v, vinv, nullptr, (u64*)out,
                            n, n));
    return share_counters_read(ctx, out_bad, out_zero);
}

extern "C" int czk_gsz_share_partial_products(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                                              const uint64_t* rands, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero) {
    bool work;
    CZK_TRY(gsz_lanes_args(ctx, "czk_gsz_share_partial_products", parties, !x || !doubles_r || !doubles_r2 || !rands || !out, n, out_bad, out_zero, &work));
    if (!work) return CZK_OK;
    const size_t P = parties, D = 5 * n + 1, Rn = 3 * n + 2;
    StageHold ws(ctx);
    CZK_TRY(ws.take((P * (2 * n + 1) + 4 * (n + 1)) * 32));
    u64 *m_inv = (u64*)ws.b.p, *lanes = m_inv + 4 * P * (n + 1), *v = lanes + 4 * P * n, *vinv = v + 4 * (n + 1), *mxm = vinv + 4 * (n + 1), *run = mxm + 4 * (n + 1);
    const u64 *dr = (const u64*)doubles_r, *dr2 = (const u64*)doubles_r2, *rd = (const u64*)rands;
    const ShareVec m_inv1{m_inv + 4, n + 1, 1};                                                                        // m_inv[1..]
    GszMulArgs a;
    a.parties = (unsigned)parties, a.degree = degree < parties ? degree : (unsigned)parties;
    CZK_TRY(share_counters(ctx));
    CZK_TRY(gsz_inv_enqueue(ctx, a, ShareVec{rd, Rn, 1}, dr, dr2, D, 0, rd, Rn, n + 1, v, vinv, nullptr, m_inv, n + 1, n + 1));   // m_inv = batch_inv(m), m = rands [0, n]
    a.n = n;
    CZK_TRY(gsz_mul_launch(ctx, a, ShareVec{rd, Rn, 1}, ShareVec{(const u64*)x, n, 1}, dr, dr2, D, n + 1, lanes, nullptr));        // mx = m[..n] x
    CZK_TRY(gsz_mul_launch(ctx, a, ShareVec{lanes, n, 1}, m_inv1, dr, dr2, D, 2 * n + 1, nullptr, mxm));                           // open(mx m_inv[1..])
    CZK_TRY(czk_fr_prefix_product(ctx, mxm, n, run, CZK_MEM_DEVICE));                                                              // the local loop :353-356
    CZK_TRY(gsz_mul_launch(ctx, a, ShareVec{rd, Rn, 0}, m_inv1, dr, dr2, D, 3 * n + 1, lanes, nullptr));                           // mms = m_0 m_inv[1..]
    CZK_TRY(gsz_inv_enqueue(ctx, a, ShareVec{lanes, n, 1}, dr, dr2, D, 4 * n + 1, rd, Rn, 2 * n + 2, v, vinv, run, (u64*)out, n, n));   // batch_inv(mms), scaled by the running product
    return share_counters_read(ctx, out_bad, out_zero);
}

extern "C" int czk_gsz_product_check(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* xs, const uint64_t* ys, const uint64_t* zs, size_t n,
                                     const uint64_t* doubles_r, const uint64_t* doubles_r2, const uint64_t* rands, uint64_t* out_ok, uint64_t* out_bad) {
    bool work;
    CZK_TRY(gsz_lanes_args(ctx, "czk_gsz_product_check", parties, !xs || !ys || !zs || !doubles_r || !doubles_r2 || !rands, n, out_ok, out_bad, &work));
    if (out_ok) *out_ok = 1;   // no triples: nothing to refute
    if (!work) return CZK_OK;
    if (n >> 32) return set_err(ctx, CZK_ERR_SIZE, "czk_gsz_product_check: more than 2^32 - 1 triples");
    const unsigned P = (unsigned)parties, R = ceil_log2(n), g0 = gsz_mul_grid(ctx, n);
    StageHold ws(ctx);
    CZK_TRY(ws.take(((size_t)2 * P * n + 1024 + (size_t)3 * g0 * P + P + 1) * 32));
    u64 *xw = (u64*)ws.b.p, *yw = xw + 4 * (size_t)P * n, *pow = yw + 4 * (size_t)P * n, *part = pow + 4 * 1024, *hpart = part + 4 * (size_t)2 * g0 * P,
        *ip = hpart + 4 * (size_t)g0 * P, *coin = ip + 4 * P;
    GszRoundArgs a;
    a.m = GszMaterial{(const u64*)doubles_r, (const u64*)doubles_r2, (const u64*)rands, (size_t)2 * R + 4, (size_t)R + 3};
    a.tab = (const u64*)ctx->share_tab.p;
    a.part = part, a.ip_part = hpart, a.ip_blocks = g0, a.ip = ip, a.coin = coin, a.P = P, a.degree = degree < P ? degree : P, a.stride = n;
    Fr two = fp_dbl(Fr::one());
    a.inv2 = fp_inv(two);
    unsigned nb = 1;
    while (nb < 4 && ((n - 1) >> (8 * nb))) nb++;
    const dim3 b(256);
    CZK_TRY(share_counters(ctx));
    ProfScope ps(ctx, "gsz_product_check");
    hipLaunchKernelGGL(k_gsz_coin, dim3(1), b, 0, ctx->stream, a.m, (size_t)0, P, a.degree, a.tab, coin, ctx->share_cnt);                     // the hadamard coin
    hipLaunchKernelGGL(k_gsz_pow_tables, dim3(4), b, 0, ctx->stream, pow, (const u64*)coin);
    CZK_GSZ_SWEEP(k_gsz_hadamard, P, dim3(g0), b, 0, ctx->stream, (const u64*)xs, (const u64*)zs, xw, (const u64*)pow, nb, n, P, hpart);
    const u64* ysrc = (const u64*)ys;   // the first round reads y where the caller left it
    size_t m = n;
    a.d0 = 0, a.r0 = 1;
    for (unsigned round = 0; round < R; round++) {
        const size_t h = (m + 1) / 2;
        const unsigned g = gsz_mul_grid(ctx, h);
        a.nblocks = g;
        // two accumulators per lane: at most 4 lanes per sweep (8 would leave one wave per SIMD)
        if (P % 3 == 0 && P % 4) hipLaunchKernelGGL(k_gsz_ip<3>, dim3(g), b, 0, ctx->stream, (const u64*)xw, ysrc, n, m, h, P, part);
        else hipLaunchKernelGGL(k_gsz_ip<4>, dim3(g), b, 0, ctx->stream, (const u64*)xw, ysrc, n, m, h, P, part);
        hipLaunchKernelGGL(k_gsz_round, dim3(1), b, 0, ctx->stream, a, ctx->share_cnt);
        hipLaunchKernelGGL(k_gsz_fold, dim3(g), b, 0, ctx->stream, (const u64*)xw, xw, ysrc, yw, n, m, h, P, (const u64*)coin);
        a.ip_part = nullptr, a.ip_blocks = 0;
        ysrc = yw, m = h, a.d0 += 2, a.r0 += 1;
    }
    a.x = xw, a.y = ysrc;
    hipLaunchKernelGGL(k_gsz_final, dim3(1), b, 0, ctx->stream, a, ctx->share_cnt);
    CZK_HIP(ctx, hipGetLastError());
    uint64_t failed = 0;
    CZK_TRY(share_counters_read(ctx, out_bad, &failed));   // the one read-back of the check
    *out_ok = failed ? 0 : 1;
    return CZK_OK;
}
