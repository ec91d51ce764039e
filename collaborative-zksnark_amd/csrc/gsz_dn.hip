// gsz_dn.hip -- the GSZ (Shamir) material made on the device: random shares and double shares by the Damgard-Nielsen preparation that gsz20 assumes
// and the reference stubs out (mpc-algebra/src/share/gsz20/mod.rs:383-406 hand every party a one).  Every party deals a random sharing, one
// all-to-all carries the shares, a Vandermonde matrix extracts parties - degree uniformly random sharings from every `parties` dealt.
//   k_fr_random: the keyed generator.  Element i = the ChaCha20 block (RFC 8439, 20 rounds, 32-bit counter) at (key, nonce, first + i), its two
//     32-byte halves reduced mod 2^252 and taken to Montgomery form by ONE multiply each (FrParams::r2, ::r2_252).  One thread per element, the block
//     in registers, no memory traffic but the store.
//   k_gsz_dn: a whole generation in ONE launch, lanes form.  Thread t owns output t = k deal + b (so the stores coalesce over b).  The extraction
//     sum_i w^(ik) commutes with the dealers' polynomials, so the thread extracts the COEFFICIENTS first -- S = sum_i w^(ik) s_i, C_m = sum_i w^(ik) c_im,
//     E_m likewise, every draw recomputed from its key and counter -- and then evaluates ONE polynomial per half at the parties' points by Horner.
//     That is draws parties blocks and multiplies plus 3 degree parties multiplies per output, against parties^2 draws for the definition read
//     literally; fully reduced Montgomery limbs do not depend on the order.  3, 4, 6 and 8 parties keep the coefficients of one half in registers
//     (1 + 2 degree Fr at most: the halves run one after the other, only S is shared); any other count parks them in a per-thread column of workspace.
//   the consistency check: k_gsz_dn_gather (the sacrificed output -> the coin's open), the per-byte power tables of the coin read from device memory
//     (pow_tables.h's layout), k_gsz_dn_fold (block partials of sum_m coin^(m + 1) r[m], both halves in one pass), k_gsz_dn_finish (one block: the
//     combination per lane), k_gsz_open on the combinations (share.hip, without its read-back) and k_gsz_dn_verdict.  One read-back, at the end.
//   one party per communicator (czk_net_gsz_dn_*, host code in net_rounds.hip): the generation cut where the shares cross the wire -- k_gsz_dn_deal (this
//     party's draws evaluated at every party's point, [destination][half][b]) before the all-to-all, k_gsz_dn_extract (this party's ONE lane) after it;
//     the check's local pass (gsz_dn_combine_launch) on one lane, its three opens through broadcasts.
// No scratch in any kernel here (profiles/gsz_dn_resource_usage.txt); LDS only for the block reductions.
#include <cstring>

#include "chacha20.h"
#include "czk_internal.h"
#include "pow_tables.h"

namespace czk {

constexpr size_t GSZ_DN_BLOCKS_PER_CU = 4;    // grid-stride cap of every kernel here, on blocks of 256 threads
constexpr unsigned GSZ_DN_MAX_PARTIES = 96;   // k_gsz_open's limit

__device__ __forceinline__ Fr dn_load(const u64* base, size_t idx) { return fp_load<FrParams>(base + 4 * idx); }
__device__ __forceinline__ void dn_store(u64* base, size_t idx, const Fr& v) { fp_store<FrParams>(base + 4 * idx, v); }

struct DnKey {
    u32 w[8];   // the 32 key bytes as little-endian words
};
struct DnNonce {
    u32 w[3];
};

// The field element of one ChaCha20 block (chacha20.h): lo = bytes 0..31, hi = bytes 32..63, little-endian, each mod 2^252; (lo + 2^252 hi) mod r, Montgomery form.
// r > 2^252, so both halves are canonical and fp_mul takes them as they are: lo R2 / R = lo R, hi (2^252 R2) / R = 2^252 hi R.
__device__ __forceinline__ Fr dn_sample(const u32* key, const DnNonce& nonce, u32 counter) {
    u32 x[16];
    chacha20_block(key, counter, nonce.w[0], nonce.w[1], nonce.w[2], x);
    Fr lo, hi, c_hi;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        lo.l[i] = x[i];
        hi.l[i] = x[8 + i];
        c_hi.l[i] = FrParams::r2_252(i);
    }
    lo.l[7] &= 0x0fffffffu;
    hi.l[7] &= 0x0fffffffu;
    return fp_add(fp_mul(lo, Fr::r2()), fp_mul(hi, c_hi));
}

__global__ __launch_bounds__(256) void k_fr_random(DnKey key, DnNonce nonce, u32 first, size_t n, u64* out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dn_store(out, i, dn_sample(key.w, nonce, first + (u32)i));
}

// tab[e] = w^e for e < parties: the parties' points, and the rows of the extraction matrix (w^(ik) = tab[i k mod parties])
__global__ __launch_bounds__(128) void k_gsz_dn_points(u64* tab, Fr w, unsigned P) {
    if (threadIdx.x < P) dn_store(tab, threadIdx.x, fp_pow_u64(w, (u64)threadIdx.x));
}

struct DnArgs {
    const u32* keys;     // parties x 8 words
    const u64* points;   // k_gsz_dn_points' table
    DnNonce nonce;
    u64 *out_r, *out_r2;   // parties lanes, `outputs` elements apart; out_r2 null: random shares only
    u64* park;           // LANES == 0: draws columns of one element per thread of the grid
    size_t deal, outputs;
    unsigned parties, degree, draws;
};

// coefficient `m` of dealer-combination k for item b: sum_i w^(ik) (draw m of dealer i's item b)
template <unsigned LANES>
__device__ __forceinline__ Fr dn_extract(const DnArgs& a, unsigned k, u32 counter) {
    const unsigned P = LANES ? LANES : a.parties;
    Fr s = Fr::zero();
    unsigned e = 0;   // i k mod P
#pragma unroll 1
    for (unsigned i = 0; i < P; i++) {
        s = fp_add(s, fp_mul(dn_load(a.points, e), dn_sample(a.keys + 8 * i, a.nonce, counter)));
        e += k;
        if (e >= P) e -= P;
    }
    return s;
}

// LANES > 0: exactly that many parties, the coefficients of one half in registers; LANES == 0: any number, the coefficients parked in a.park.
// DOUBLES: both halves (degree d and 2 d); else the degree-d half alone.
template <unsigned LANES, bool DOUBLES>
__global__ __launch_bounds__(256) void k_gsz_dn(DnArgs a) {
    constexpr unsigned MAXD = LANES ? (DOUBLES ? (LANES - 1) / 2 : LANES - 1) : 0;   // the largest degree the argument rules let through
    const unsigned P = LANES ? LANES : a.parties, d = a.degree;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, T = (size_t)gridDim.x * blockDim.x;
    for (size_t t = tid; t < a.outputs; t += T) {
        const unsigned k = (unsigned)(t / a.deal);
        const u32 c0 = (u32)((t - (size_t)k * a.deal) * a.draws);   // deal draws <= 2^32: no counter wraps
        const Fr S = dn_extract<LANES>(a, k, c0);
        if constexpr (LANES != 0) {
#pragma unroll
            for (unsigned half = 0; half < (DOUBLES ? 2u : 1u); half++) {
                constexpr unsigned CAP = (DOUBLES ? 2 : 1) * MAXD;
                const unsigned deg = half ? 2 * d : d;
                Fr C[CAP ? CAP : 1];
#pragma unroll
                for (unsigned m = 0; m < CAP; m++)
                    if (m < deg) C[m] = dn_extract<LANES>(a, k, c0 + 1 + (half ? d : 0) + m);
                u64* out = half ? a.out_r2 : a.out_r;
#pragma unroll 1
                for (unsigned j = 0; j < P; j++) {
                    const Fr x = dn_load(a.points, j);
                    Fr v = Fr::zero();
#pragma unroll
                    for (unsigned m = CAP; m-- > 0;)
                        if (m < deg) v = fp_mul(fp_add(v, C[m]), x);
                    dn_store(out, (size_t)j * a.outputs + t, fp_add(v, S));
                }
            }
        } else {
            for (unsigned m = 1; m < a.draws; m++) dn_store(a.park, (size_t)m * T + tid, dn_extract<0>(a, k, c0 + m));
            for (unsigned half = 0; half < (DOUBLES ? 2u : 1u); half++) {
                const unsigned deg = half ? 2 * d : d, base = half ? d : 0;
                u64* out = half ? a.out_r2 : a.out_r;
                for (unsigned j = 0; j < P; j++) {
                    const Fr x = dn_load(a.points, j);
                    Fr v = Fr::zero();
                    for (unsigned m = deg; m > 0; m--) v = fp_mul(fp_add(v, dn_load(a.park, (size_t)(base + m) * T + tid)), x);
                    dn_store(out, (size_t)j * a.outputs + t, fp_add(v, S));
                }
            }
        }
    }
}

// ---- one party per communicator (czk_net_gsz_dn_*, host code in net_rounds.hip): the same generation cut where the shares cross the wire ---------------------
// Before the all-to-all: this party's item b evaluated at every party's point, send[(j halves + half) deal + b] = its share for party j.  The draws are
// recomputed per destination: nothing is kept but the Horner accumulator.
__global__ __launch_bounds__(256) void k_gsz_dn_deal(DnKey key, DnNonce nonce, const u64* points, unsigned P, unsigned d, unsigned halves, unsigned draws, size_t deal, u64* send) {
    for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < deal; b += (size_t)gridDim.x * blockDim.x) {
        const u32 c0 = (u32)(b * draws);
        const Fr s = dn_sample(key.w, nonce, c0);
        for (unsigned j = 0; j < P; j++) {
            const Fr x = dn_load(points, j);
            for (unsigned half = 0; half < halves; half++) {
                const unsigned deg = half ? 2 * d : d, base = half ? d : 0;
                Fr v = Fr::zero();
                for (unsigned m = deg; m > 0; m--) v = fp_mul(fp_add(v, dn_sample(key.w, nonce, c0 + base + m)), x);
                dn_store(send, ((size_t)j * halves + half) * deal + b, fp_add(v, s));
            }
        }
    }
}
// After it: recv[(i halves + half) deal + b] = dealer i's share for this party; output k deal + b of this party's ONE lane = sum_i w^(ik) of them
__global__ __launch_bounds__(256) void k_gsz_dn_extract(const u64* recv, const u64* points, unsigned P, unsigned halves, size_t deal, size_t outputs, u64* out_r, u64* out_r2) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < outputs; t += (size_t)gridDim.x * blockDim.x) {
        const unsigned k = (unsigned)(t / deal);
        const size_t b = t - (size_t)k * deal;
        Fr a0 = Fr::zero(), a1 = Fr::zero();
        unsigned e = 0;   // i k mod P
        for (unsigned i = 0; i < P; i++) {
            const Fr w = dn_load(points, e);
            a0 = fp_add(a0, fp_mul(w, dn_load(recv, (size_t)i * halves * deal + b)));
            if (halves == 2) a1 = fp_add(a1, fp_mul(w, dn_load(recv, ((size_t)i * 2 + 1) * deal + b)));
            e += k;
            if (e >= P) e -= P;
        }
        dn_store(out_r, t, a0);
        if (halves == 2) dn_store(out_r2, t, a1);
    }
}

// ---- the consistency check --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fr dn_wave_sum(Fr v) {
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
__device__ __forceinline__ Fr dn_block_sum(const Fr& v, Fr* sm) {
    const Fr w = dn_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = w;
    __syncthreads();
    const Fr t = fp_add(fp_add(sm[0], sm[1]), fp_add(sm[2], sm[3]));
    __syncthreads();
    return t;
}

// dst[j] = src[j * stride + at] for j < P: one element of every lane, side by side for k_gsz_open
__global__ __launch_bounds__(128) void k_gsz_dn_gather(const u64* src, size_t stride, size_t at, unsigned P, u64* dst) {
    if (threadIdx.x < P) dn_store(dst, threadIdx.x, dn_load(src, (size_t)threadIdx.x * stride + at));
}

// T_j[b] = coin^(b 2^(8 j)) (pow_tables.h's layout), the coin read from device memory: 4 blocks of 256
__global__ __launch_bounds__(256) void k_gsz_dn_pow_tables(u64* tab, const u64* coin) {
    Fr root = dn_load(coin, 0);
    for (unsigned s = 0; s < 8 * blockIdx.x; s++) root = fp_sqr(root);
    dn_store(tab, 256 * (size_t)blockIdx.x + threadIdx.x, fp_pow_u64(root, (u64)threadIdx.x));
}

// part[(block * P + lane) * 2 + half] = the block's share of sum_{m < cnt} coin^(m + 1) r_lane[m] (half 1: r2, when given)
__global__ __launch_bounds__(256) void k_gsz_dn_fold(const u64* r, const u64* r2, size_t stride, size_t cnt, unsigned P, const u64* pow, unsigned nb, u64* part) {
    __shared__ Fr sm[4];
    for (unsigned lane = 0; lane < P; lane++) {
        Fr a0 = Fr::zero(), a1 = Fr::zero();
        for (size_t m = (size_t)blockIdx.x * blockDim.x + threadIdx.x; m < cnt; m += (size_t)gridDim.x * blockDim.x) {
            const Fr p = marlin_domain_element(pow, (u32)(m + 1), nb);
            a0 = fp_add(a0, fp_mul(p, dn_load(r, (size_t)lane * stride + m)));
            if (r2) a1 = fp_add(a1, fp_mul(p, dn_load(r2, (size_t)lane * stride + m)));
        }
        const Fr s0 = dn_block_sum(a0, sm), s1 = dn_block_sum(a1, sm);
        if (threadIdx.x == 0) {
            dn_store(part, ((size_t)blockIdx.x * P + lane) * 2, s0);
            dn_store(part, ((size_t)blockIdx.x * P + lane) * 2 + 1, s1);
        }
    }
}

// one block: u[half * P + lane] = r_lane[last] + the lane's partials
__global__ __launch_bounds__(256) void k_gsz_dn_finish(const u64* r, const u64* r2, size_t stride, size_t last, unsigned P, const u64* part, unsigned nblocks, u64* u) {
    __shared__ Fr sm[4];
    for (unsigned q = 0; q < 2 * P; q++) {
        const unsigned half = q / P, lane = q - half * P;
        if (half && !r2) break;
        Fr a = Fr::zero();
        for (unsigned b = threadIdx.x; b < nblocks; b += 256) a = fp_add(a, dn_load(part, ((size_t)b * P + lane) * 2 + half));
        const Fr s = dn_block_sum(a, sm);
        if (threadIdx.x == 0) dn_store(u, q, fp_add(s, dn_load(half ? r2 : r, (size_t)lane * stride + last)));
    }
}

// the two opened combinations must be the same value: cnt[1] = 1 when they are not
__global__ __launch_bounds__(64) void k_gsz_dn_verdict(const u64* opened, unsigned long long* cnt) {
    if (threadIdx.x) return;
    if (dn_load(opened, 0) != dn_load(opened, 1)) atomicExch(cnt + 1, 1ull);
}

static unsigned dn_grid(czk_ctx* ctx, size_t n) {
    size_t blocks = (n + 255) / 256;
    const size_t cap = GSZ_DN_BLOCKS_PER_CU * (size_t)ctx->num_cu;
    if (blocks > cap) blocks = cap;
    return blocks ? (unsigned)blocks : 1u;
}

static unsigned dn_draws(int kind, unsigned degree) { return kind == CZK_GSZ_DN_DOUBLES ? 1 + 3 * degree : 1 + degree; }

// the argument rules every call here shares: kind, the share domain, the degree against the parties, the counter's range
int gsz_dn_shape(czk_ctx* ctx, const char* what, int kind, size_t parties, unsigned degree, size_t deal) {
    if (kind != CZK_GSZ_DN_DOUBLES && kind != CZK_GSZ_DN_RANDS) return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": kind is CZK_GSZ_DN_DOUBLES or CZK_GSZ_DN_RANDS");
    if (parties > GSZ_DN_MAX_PARTIES) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": more than 96 parties");
    u64 dom[12];
    CZK_TRY(czk_share_domain_constants(ctx, parties, dom));   // CZK_ERR_SIZE: no share domain of that size
    if (kind == CZK_GSZ_DN_DOUBLES ? 2 * (size_t)degree >= parties : (size_t)degree >= parties)
        return set_err(ctx, CZK_ERR_ARG, std::string(what) + ": the degree leaves no sharing to extract (doubles need 2 degree < parties, random shares degree < parties)");
    if (deal > ((size_t)1 << 32) / dn_draws(kind, degree)) return set_err(ctx, CZK_ERR_SIZE, std::string(what) + ": the 32-bit block counter would wrap (deal draws > 2^32)");
    return CZK_OK;
}

// points[e] = w^e, e < parties (parties: a size the share domain exists for, at most 96), enqueued
int gsz_dn_points_launch(czk_ctx* ctx, size_t parties, u64* points) {
    u64 dom[12];
    CZK_TRY(czk_share_domain_constants(ctx, parties, dom));
    hipLaunchKernelGGL(k_gsz_dn_points, dim3(1), dim3(128), 0, ctx->stream, points, host_fr(dom + 4), (unsigned)parties);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

// the party side of czk_net_gsz_dn_generate: send = parties x halves x deal elements, [destination][half][b]
int gsz_dn_deal_launch(czk_ctx* ctx, int kind, size_t parties, unsigned degree, const uint8_t* key, const uint8_t* nonce, size_t deal, const u64* points, u64* send) {
    DnKey k;
    DnNonce nc;
    memcpy(k.w, key, 32);
    memcpy(nc.w, nonce, 12);
    ProfScope ps(ctx, "gsz_dn_deal");
    hipLaunchKernelGGL(k_gsz_dn_deal, dim3(dn_grid(ctx, deal)), dim3(256), 0, ctx->stream, k, nc, points, (unsigned)parties, degree, kind == CZK_GSZ_DN_DOUBLES ? 2u : 1u,
                       dn_draws(kind, degree), deal, send);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}
// recv = parties x halves x deal elements, [dealer][half][b] -> this party's lane of the deal (parties - degree) outputs
int gsz_dn_extract_launch(czk_ctx* ctx, int kind, size_t parties, unsigned degree, size_t deal, const u64* points, const u64* recv, u64* out_r, u64* out_r2) {
    const size_t outputs = deal * (parties - degree);
    ProfScope ps(ctx, "gsz_dn_extract");
    hipLaunchKernelGGL(k_gsz_dn_extract, dim3(dn_grid(ctx, outputs)), dim3(256), 0, ctx->stream, recv, points, (unsigned)parties, kind == CZK_GSZ_DN_DOUBLES ? 2u : 1u, deal,
                       outputs, out_r, out_r2);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

// The check's local pass over `lanes` lanes (`stride` apart) of `outputs` elements, the coin in device memory: u[half lanes + lane] = the lane's combination
// r[outputs - 1] + sum_{m < outputs - 2} coin^(m + 1) r[m] (half 1: of r2, when given).  ws: gsz_dn_combine_ws elements.  outputs: 3 .. 2^32 - 1.
size_t gsz_dn_combine_ws(czk_ctx* ctx, size_t lanes, size_t outputs) { return 1024 + (size_t)2 * dn_grid(ctx, outputs - 2) * lanes; }
int gsz_dn_combine_launch(czk_ctx* ctx, size_t lanes, const u64* r, const u64* r2, size_t stride, size_t outputs, const u64* coin, u64* ws, u64* u) {
    const size_t cnt = outputs - 2;
    const unsigned g = dn_grid(ctx, cnt), P = (unsigned)lanes;
    u64 *pow = ws, *part = ws + 4 * 1024;
    unsigned nb = 1;
    while (nb < 4 && (cnt >> (8 * nb))) nb++;   // the largest exponent is cnt
    ProfScope ps(ctx, "gsz_dn_check");
    hipLaunchKernelGGL(k_gsz_dn_pow_tables, dim3(4), dim3(256), 0, ctx->stream, pow, coin);
    hipLaunchKernelGGL(k_gsz_dn_fold, dim3(g), dim3(256), 0, ctx->stream, r, r2, stride, cnt, P, (const u64*)pow, nb, part);
    hipLaunchKernelGGL(k_gsz_dn_finish, dim3(1), dim3(256), 0, ctx->stream, r, r2, stride, outputs - 1, P, (const u64*)part, g, u);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}
// opened[0] != opened[1] -> ctx->share_cnt[1] = 1
int gsz_dn_verdict_launch(czk_ctx* ctx, const u64* opened) {
    hipLaunchKernelGGL(k_gsz_dn_verdict, dim3(1), dim3(64), 0, ctx->stream, opened, ctx->share_cnt);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

}  // namespace czk

using namespace czk;

extern "C" int czk_fr_random(czk_ctx* ctx, const uint8_t* key, const uint8_t* nonce, uint32_t first, size_t n, uint64_t* out, int mem) {
    if (!ctx || !key || !nonce || (n && !out)) return ctx ? set_err(ctx, CZK_ERR_ARG, "null fr_random argument") : CZK_ERR_ARG;
    if (!valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE");
    if (n > ((size_t)1 << 32) - first) return set_err(ctx, CZK_ERR_SIZE, "czk_fr_random: the 32-bit block counter would wrap (first + n > 2^32)");
    if (!n) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    DnKey k;
    DnNonce nc;
    memcpy(k.w, key, 32);
    memcpy(nc.w, nonce, 12);
    Staged so{ctx};
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST ? nullptr : out, n * 32, mem));
    hipLaunchKernelGGL(k_fr_random, dim3(dn_grid(ctx, n)), dim3(256), 0, ctx->stream, k, nc, (u32)first, n, (u64*)so.dev);
    CZK_HIP(ctx, hipGetLastError());
    return so.to_host(out, n * 32);
}

extern "C" int czk_gsz_dn_counts(int kind, size_t parties, unsigned degree, size_t want, size_t* deal, size_t* outputs) {
    if (!deal || !outputs) return CZK_ERR_ARG;
    *deal = *outputs = 0;
    if (kind != CZK_GSZ_DN_DOUBLES && kind != CZK_GSZ_DN_RANDS) return CZK_ERR_ARG;
    if (kind == CZK_GSZ_DN_DOUBLES ? 2 * (size_t)degree >= parties : (size_t)degree >= parties) return CZK_ERR_ARG;
    if (parties > GSZ_DN_MAX_PARTIES || want > ((size_t)1 << 58)) return CZK_ERR_SIZE;
    const size_t per = parties - degree;
    *deal = (want + per - 1) / per;
    *outputs = *deal * per;
    return CZK_OK;
}

extern "C" int czk_gsz_dn_generate(czk_ctx* ctx, int kind, size_t parties, unsigned degree, const uint8_t* keys, const uint8_t* nonce, size_t deal, uint64_t* out_r,
                                   uint64_t* out_r2) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_TRY(gsz_dn_shape(ctx, "czk_gsz_dn_generate", kind, parties, degree, deal));
    if (!deal) return CZK_OK;
    const bool doubles = kind == CZK_GSZ_DN_DOUBLES;
    if (!keys || !nonce || !out_r || (doubles && !out_r2)) return set_err(ctx, CZK_ERR_ARG, "czk_gsz_dn_generate: null argument");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    DnArgs a;
    a.deal = deal, a.outputs = deal * (parties - degree);
    a.parties = (unsigned)parties, a.degree = degree, a.draws = dn_draws(kind, degree);
    a.out_r = (u64*)out_r, a.out_r2 = doubles ? (u64*)out_r2 : nullptr;
    memcpy(a.nonce.w, nonce, 12);
    const unsigned g = dn_grid(ctx, a.outputs);
    const bool generic = parties != 3 && parties != 4 && parties != 6 && parties != 8;
    const size_t head = 2 * (size_t)GSZ_DN_MAX_PARTIES;   // elements: the points, then the keys (32 bytes each)
    StageHold ws(ctx);
    CZK_TRY(ws.take((head + (generic ? (size_t)a.draws * g * 256 : 0)) * 32));
    u64* points = (u64*)ws.b.p;
    u32* dkeys = (u32*)(points + 4 * GSZ_DN_MAX_PARTIES);
    a.points = points, a.keys = dkeys, a.park = points + 4 * head;
    CZK_TRY(upload_pageable(ctx, dkeys, keys, parties * 32));
    CZK_TRY(gsz_dn_points_launch(ctx, parties, points));
    ProfScope ps(ctx, "gsz_dn_generate");
    const dim3 grid(g), b(256);
#define CZK_GSZ_DN_CASE(LN)                                                                \
    case LN:                                                                               \
        if (doubles) hipLaunchKernelGGL((k_gsz_dn<LN, true>), grid, b, 0, ctx->stream, a); \
        else hipLaunchKernelGGL((k_gsz_dn<LN, false>), grid, b, 0, ctx->stream, a);        \
        break;
    switch (parties) {
        CZK_GSZ_DN_CASE(3)
        CZK_GSZ_DN_CASE(4)
        CZK_GSZ_DN_CASE(6)
        CZK_GSZ_DN_CASE(8)
        default:
            if (doubles) hipLaunchKernelGGL((k_gsz_dn<0, true>), grid, b, 0, ctx->stream, a);
            else hipLaunchKernelGGL((k_gsz_dn<0, false>), grid, b, 0, ctx->stream, a);
    }
#undef CZK_GSZ_DN_CASE
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}

extern "C" int czk_gsz_dn_check(czk_ctx* ctx, int kind, size_t parties, unsigned degree, const uint64_t* r, const uint64_t* r2, size_t outputs, uint64_t* out_ok,
                                uint64_t* out_bad) {
    if (!ctx) return CZK_ERR_ARG;
    if (!out_ok || !out_bad) return set_err(ctx, CZK_ERR_ARG, "czk_gsz_dn_check: null result output");
    *out_ok = *out_bad = 0;
    CZK_TRY(gsz_dn_shape(ctx, "czk_gsz_dn_check", kind, parties, degree, 0));
    const bool doubles = kind == CZK_GSZ_DN_DOUBLES;
    if (outputs < 3) return set_err(ctx, CZK_ERR_ARG, "czk_gsz_dn_check: fewer than 3 outputs (two are sacrificed)");
    if (!r || (doubles && !r2)) return set_err(ctx, CZK_ERR_ARG, "czk_gsz_dn_check: null argument");
    if (outputs >> 32) return set_err(ctx, CZK_ERR_SIZE, "czk_gsz_dn_check: more than 2^32 - 1 outputs");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned P = (unsigned)parties;
    const u64 *dr = (const u64*)r, *dr2 = doubles ? (const u64*)r2 : nullptr;
    const size_t cws = gsz_dn_combine_ws(ctx, P, outputs);
    StageHold ws(ctx);
    CZK_TRY(ws.take((cws + 3 * (size_t)P + 3) * 32));
    u64 *cv = (u64*)ws.b.p + 4 * cws, *u = cv + 4 * P, *coin = u + 4 * 2 * P, *opened = coin + 4;
    CZK_TRY(share_counters(ctx));
    hipLaunchKernelGGL(k_gsz_dn_gather, dim3(1), dim3(128), 0, ctx->stream, dr, outputs, outputs - 2, P, cv);
    CZK_TRY(gsz_open_enqueue(ctx, cv, P, 1, nullptr, degree, coin, ctx->share_cnt));   // the coin: the first sacrificed output, opened
    CZK_TRY(gsz_dn_combine_launch(ctx, P, dr, dr2, outputs, outputs, coin, (u64*)ws.b.p, u));
    CZK_TRY(gsz_open_enqueue(ctx, u, P, 1, nullptr, degree, opened, ctx->share_cnt));
    if (doubles) {
        CZK_TRY(gsz_open_enqueue(ctx, u + 4 * P, P, 1, nullptr, 2 * degree, opened + 4, ctx->share_cnt));
        CZK_TRY(gsz_dn_verdict_launch(ctx, opened));
    }
    uint64_t differ = 0;
    CZK_TRY(share_counters_read(ctx, out_bad, &differ));   // the one read-back of the check
    *out_ok = (differ || *out_bad) ? 0 : 1;
    return CZK_OK;
}
