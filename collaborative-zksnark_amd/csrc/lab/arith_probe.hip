// arith_probe.hip -- LAB BUILD ONLY (build.py LAB_SOURCES): one small kernel per function of the unsaturated arithmetic headers, fed raw
// limbs from memory and storing raw limbs back.  See arith_probe.h for the item layouts and tests/test_lazy_arith.py for the user.
// The headers are compiled here in their own translation unit, with the hot kernels' flags (the Montgomery multiply inlined).
// Ops from CZK_PROBE_SAT_BASE up are the saturated field.h / curve.h (sat_probe.h): the inlined form is compiled here, the
// -DCZK_NOINLINE_MUL form (and the tower) in sat_probe.hip, which the switch below dispatches to.
#include "arith_probe.h"

#include "curve.h"
#include "czk_internal.h"
#include "fq2pu.h"
#include "fru.h"
#include "te.h"
#include "tower.h"

namespace czk {
namespace {

__device__ __forceinline__ FqU ldq(const u32* p) {
    FqU r;
#pragma unroll
    for (int i = 0; i < 14; i++) r.l[i] = p[i];
    return r;
}
__device__ __forceinline__ void stq(u32* p, const FqU& a) {
#pragma unroll
    for (int i = 0; i < 14; i++) p[i] = a.l[i];
}
__device__ __forceinline__ FrU ldr(const u32* p) {
    FrU r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
    return r;
}
__device__ __forceinline__ void str(u32* p, const FrU& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = a.l[i];
}
template <class F>
__device__ __forceinline__ F ldsat(const u32* p) {
    F r;
#pragma unroll
    for (int i = 0; i < F::N; i++) r.l[i] = p[i];
    return r;
}
template <class F>
__device__ __forceinline__ void stsat(u32* p, const F& a) {
#pragma unroll
    for (int i = 0; i < F::N; i++) p[i] = a.l[i];
}
__device__ __forceinline__ Fq2U ldq2(const u32* p) { return Fq2U{ldq(p), ldq(p + 14)}; }
__device__ __forceinline__ void stq2(u32* p, const Fq2U& a) {
    stq(p, a.c0);
    stq(p + 14, a.c1);
}
__device__ __forceinline__ XYZZU ldxu(const u32* p) {
    XYZZU r;
    r.x = ldq(p), r.y = ldq(p + 14), r.zz = ldq(p + 28), r.zzz = ldq(p + 42);
    r.inf = p[56] != 0;
    return r;
}
__device__ __forceinline__ void stxu(u32* p, const XYZZU& a) {
    stq(p, a.x), stq(p + 14, a.y), stq(p + 28, a.zz), stq(p + 42, a.zzz);
    p[56] = a.inf ? 1u : 0u;
}
__device__ __forceinline__ TEU ldte(const u32* p) { return TEU{ldq(p), ldq(p + 14), ldq(p + 28), ldq(p + 42)}; }
__device__ __forceinline__ void stte(u32* p, const TEU& a) { stq(p, a.x), stq(p + 14, a.y), stq(p + 28, a.z), stq(p + 42, a.t); }
// lane-pair points: memory holds (x.c0, x.c1, y.c0, ..., zzz.c1, inf); lane `par` takes its halves
__device__ __forceinline__ XYZZU2 ldxu2(const u32* p, unsigned par) {
    XYZZU2 r;
    r.x = ldq(p + 14 * par), r.y = ldq(p + 28 + 14 * par), r.zz = ldq(p + 56 + 14 * par), r.zzz = ldq(p + 84 + 14 * par);
    r.inf = p[112] != 0;
    return r;
}
__device__ __forceinline__ void stxu2(u32* p, const XYZZU2& a, unsigned par) {
    stq(p + 14 * par, a.x), stq(p + 28 + 14 * par, a.y), stq(p + 56 + 14 * par, a.zz), stq(p + 84 + 14 * par, a.zzz);
    if (par == 0) p[112] = a.inf ? 1u : 0u;
}

// ---- one functor per probed function: IW / OW words per item, LANES threads per item
#define PROBE(NAME, IWORDS, OWORDS, ...)                                    \
    struct NAME {                                                           \
        static constexpr int IW = IWORDS, OW = OWORDS, LANES = 1;           \
        static __device__ __forceinline__ void run(const u32* i, u32* o, unsigned) { __VA_ARGS__ } \
    };
#define PROBE2(NAME, IWORDS, OWORDS, ...)                                   \
    struct NAME {                                                           \
        static constexpr int IW = IWORDS, OW = OWORDS, LANES = 2;           \
        static __device__ __forceinline__ void run(const u32* i, u32* o, unsigned par) { __VA_ARGS__ } \
    };

PROBE(PFquMul, 28, 14, stq(o, fqu_mul(ldq(i), ldq(i + 14)));)
PROBE(PFquSqr, 14, 14, stq(o, fqu_sqr(ldq(i)));)
PROBE(PFquMulAdd, 56, 14, stq(o, fqu_mul_add(ldq(i), ldq(i + 14), ldq(i + 28), ldq(i + 42)));)
PROBE(PFquMulAddHi, 70, 14, stq(o, fqu_mul_add_hi(ldq(i), ldq(i + 14), ldq(i + 28), ldq(i + 42), ldq(i + 56)));)
PROBE(PFquMulHi, 42, 14, stq(o, fqu_mul_hi(ldq(i), ldq(i + 14), ldq(i + 28)));)
PROBE(PFquMulAdd4, 112, 14,
      stq(o, fqu_mul_add4(ldq(i), ldq(i + 14), ldq(i + 28), ldq(i + 42), ldq(i + 56), ldq(i + 70), ldq(i + 84), ldq(i + 98)));)
PROBE(PFquMulS, 28, 14, stq(o, fqu_mul_s(ldq(i), ldq(i + 14)));)
PROBE(PFquSqrS, 14, 14, stq(o, fqu_sqr_s(ldq(i)));)
PROBE(PFquMulAddS, 56, 14, stq(o, fqu_mul_add_s(ldq(i), ldq(i + 14), ldq(i + 28), ldq(i + 42)));)
PROBE(PFquMulAddHiS, 70, 14, stq(o, fqu_mul_add_hi_s(ldq(i), ldq(i + 14), ldq(i + 28), ldq(i + 42), ldq(i + 56)));)
PROBE(PFquMulHiS, 42, 14, stq(o, fqu_mul_hi_s(ldq(i), ldq(i + 14), ldq(i + 28)));)
PROBE(PFquMulAdd4S, 112, 14,
      stq(o, fqu_mul_add4_s(ldq(i), ldq(i + 14), ldq(i + 28), ldq(i + 42), ldq(i + 56), ldq(i + 70), ldq(i + 84), ldq(i + 98)));)
PROBE(PFquNormalize, 14, 14, stq(o, fqu_normalize(ldq(i)));)
PROBE(PFquSubLazy4, 28, 14, stq(o, fqu_sub_lazy<4>(ldq(i), ldq(i + 14)));)
PROBE(PFquSubLazy8, 28, 14, stq(o, fqu_sub_lazy<8>(ldq(i), ldq(i + 14)));)
PROBE(PFquSubLazy16, 28, 14, stq(o, fqu_sub_lazy<16>(ldq(i), ldq(i + 14)));)
PROBE(PFquSub3Norm, 42, 14, stq(o, fqu_sub3_norm(ldq(i), ldq(i + 14), ldq(i + 28)));)
PROBE(PFquUnpack, 12, 14, stq(o, fqu_unpack(ldsat<Fq>(i)));)
PROBE(PFquPack, 14, 12, stsat<Fq>(o, fqu_pack(ldq(i)));)
PROBE(PFquNeg5, 14, 14, stq(o, fqu_neg5<false>(ldq(i)));)
PROBE(PFquNeg5Big, 14, 14, stq(o, fqu_neg5<true>(ldq(i)));)
PROBE(PFquAddLazy, 28, 14, stq(o, fqu_add_lazy(ldq(i), ldq(i + 14)));)
PROBE(PFquSubn32, 28, 14, stq(o, fqu_subn_32(ldq(i), ldq(i + 14)));)
PROBE(PFquSubn64, 28, 14, stq(o, fqu_subn_64(ldq(i), ldq(i + 14)));)
PROBE(PFquSubn128, 28, 14, stq(o, fqu_subn_128(ldq(i), ldq(i + 14)));)

PROBE(PFq2uMul, 56, 28, stq2(o, fq2u_mul(ldq2(i), ldq2(i + 28)));)
PROBE(PFq2uSqr, 28, 28, stq2(o, fq2u_sqr(ldq2(i)));)
PROBE(PFq2uMulN5, 56, 28, const Fq2U b = ldq2(i + 28); stq2(o, fq2u_mul_n5(ldq2(i), b, fqu_neg5<false>(b.c1)));)

PROBE(PFquXyzzAccMixed, 84, 57,
      FqU ax = ldq(i), ay = ldq(i + 14), azz = ldq(i + 28), azzz = ldq(i + 42);
      const bool ok = fqu_xyzz_acc_mixed(ax, ay, azz, azzz, ldq(i + 56), ldq(i + 70));
      stq(o, ax), stq(o + 14, ay), stq(o + 28, azz), stq(o + 42, azzz);
      o[56] = ok ? 1u : 0u;)
PROBE(PXyzzuAdd, 114, 57, XYZZU a = ldxu(i); xyzzu_add(a, ldxu(i + 57)); stxu(o, a);)
PROBE(PXyzzuDouble, 57, 57, XYZZU a = ldxu(i); xyzzu_double(a); stxu(o, a);)
PROBE(PXyzzuToSat, 57, 48, const XYZZ<Fq> s = xyzzu_to_sat(ldxu(i));
      stsat<Fq>(o, s.x), stsat<Fq>(o + 12, s.y), stsat<Fq>(o + 24, s.zz), stsat<Fq>(o + 36, s.zzz);)
PROBE(PXyzzuFromSat, 48, 57, stxu(o, xyzzu_from_sat(XYZZ<Fq>{ldsat<Fq>(i), ldsat<Fq>(i + 12), ldsat<Fq>(i + 24), ldsat<Fq>(i + 36)}));)
PROBE(PFq2uXyzzAccMixed, 168, 113,
      Fq2U ax = ldq2(i), ay = ldq2(i + 28), azz = ldq2(i + 56), azzz = ldq2(i + 84);
      const bool ok = fq2u_xyzz_acc_mixed(ax, ay, azz, azzz, ldq2(i + 112), ldq2(i + 140));
      stq2(o, ax), stq2(o + 28, ay), stq2(o + 56, azz), stq2(o + 84, azzz);
      o[112] = ok ? 1u : 0u;)

PROBE(PTeuFromNiels, 42, 56, stte(o, teu_from_niels(ldq(i), ldq(i + 14), ldq(i + 28)));)
PROBE(PTeuMadd, 98, 56, TEU a = ldte(i); teu_madd(a, ldq(i + 56), ldq(i + 70), ldq(i + 84)); stte(o, a);)
PROBE(PTeuAdd, 112, 56, TEU a = ldte(i); teu_add(a, ldte(i + 56)); stte(o, a);)
PROBE(PTeuDouble, 56, 56, TEU a = ldte(i); teu_double(a); stte(o, a);)
PROBE(PTeuToJac, 56, 36, const Jac<Fq> j = teu_to_jac(ldte(i)); stsat<Fq>(o, j.x), stsat<Fq>(o + 12, j.y), stsat<Fq>(o + 24, j.z);)
PROBE(PTeLoadNiels, 52, 42, FqU ym, yp, k2; te_load_niels(reinterpret_cast<const u64*>(i), i[48] != 0, ym, yp, k2);
      stq(o, ym), stq(o + 14, yp), stq(o + 28, k2);)

PROBE2(PP2Mul, 57, 28, const FqU a = ldq(i + 14 * par), b = ldq(i + 28 + 14 * par);
       const FqU r = i[56] ? p2_mul(p2_a(a), p2_b<true>(b)) : p2_mul(p2_a(a), p2_b<false>(b));
       stq(o + 14 * par, r);)
PROBE2(PXyzzu2Add, 226, 113, XYZZU2 a = ldxu2(i, par); xyzzu2_add(a, ldxu2(i + 113, par)); stxu2(o, a, par);)
PROBE2(PXyzzu2Double, 113, 113, XYZZU2 a = ldxu2(i, par); xyzzu2_double(a); stxu2(o, a, par);)
PROBE2(PXyzzu2AccMixed, 168, 113,
       FqU ax = ldq(i + 14 * par), ay = ldq(i + 28 + 14 * par), azz = ldq(i + 56 + 14 * par), azzz = ldq(i + 84 + 14 * par);
       const bool ok = xyzzu2_acc_mixed(ax, ay, azz, azzz, ldq(i + 112 + 14 * par), ldq(i + 140 + 14 * par));
       stq(o + 14 * par, ax), stq(o + 28 + 14 * par, ay), stq(o + 56 + 14 * par, azz), stq(o + 84 + 14 * par, azzz);
       if (par == 0) o[112] = ok ? 1u : 0u;)

PROBE(PFruMul, 18, 9, str(o, fru_mul(ldr(i), ldr(i + 9)));)
PROBE(PFruNormalize, 9, 9, str(o, fru_normalize(ldr(i)));)
PROBE(PFruUnpack, 8, 9, str(o, fru_unpack(ldsat<Fr>(i)));)
PROBE(PFruPack, 9, 8, stsat<Fr>(o, fru_pack(ldr(i)));)
PROBE(PFruReduce2r, 9, 9, str(o, fru_reduce_2r(ldr(i)));)
PROBE(PFruCanon, 9, 8, stsat<Fr>(o, fru_canon(ldr(i)));)
PROBE(PFruCanonMulout, 9, 8, stsat<Fr>(o, fru_canon_mulout(ldr(i)));)
PROBE(PFruAdd, 18, 9, str(o, fru_add(ldr(i), ldr(i + 9)));)
template <int K, int U>
struct PFruSub {
    static constexpr int IW = 18, OW = 9, LANES = 1;
    static __device__ __forceinline__ void run(const u32* i, u32* o, unsigned) { str(o, fru_sub<K, U>(ldr(i), ldr(i + 9))); }
};
#undef PROBE
#undef PROBE2

// thread t works on item t / LANES; the lanes of a pair share an item and leave together
template <class OP>
__global__ __launch_bounds__(128) void k_arith_probe(const u32* in, u32* out, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t item = t / OP::LANES;
    if (item >= n) return;
    OP::run(in + item * OP::IW, out + item * OP::OW, (unsigned)(t % OP::LANES));
}

template <class OP>
int probe(czk_ctx* ctx, const uint32_t* in, size_t iw, uint32_t* out, size_t ow, size_t n, int mem) {
    if (iw != (size_t)OP::IW || ow != (size_t)OP::OW)
        return set_err(ctx, CZK_ERR_ARG, "arith_probe: this op takes " + std::to_string(OP::IW) + " words per item and returns " + std::to_string(OP::OW));
    if (!n) return CZK_OK;
    Staged si{ctx}, so{ctx};
    CZK_TRY(si.to_device(in, n * iw * 4, mem));
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST ? nullptr : out, n * ow * 4, mem));
    const size_t threads = n * OP::LANES;
    hipLaunchKernelGGL(k_arith_probe<OP>, dim3((unsigned)((threads + 127) / 128)), dim3(128), 0, ctx->stream, (const u32*)si.dev, (u32*)so.dev, n);
    CZK_HIP(ctx, hipGetLastError());
    return so.to_host(out, n * ow * 4);
}

// the saturated arithmetic, compiled in this translation unit's form: the Montgomery multiply inlined
#include "sat_probe.h"

}  // namespace
}  // namespace czk

using namespace czk;

extern "C" int czk_lab_arith_probe(czk_ctx* ctx, int op, const uint32_t* in, size_t in_words_per_item, uint32_t* out, size_t out_words_per_item,
                                   size_t n, int mem) {
    if (!ctx || (n && (!in || !out))) return ctx ? set_err(ctx, CZK_ERR_ARG, "null arith_probe argument") : CZK_ERR_ARG;
    if (!valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE");
    if (n > ((size_t)1 << 24)) return set_err(ctx, CZK_ERR_SIZE, "arith_probe: at most 2^24 items");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
#define RUN(...) return probe<__VA_ARGS__>(ctx, in, in_words_per_item, out, out_words_per_item, n, mem)
    switch (op) {
    case CZK_PROBE_FQU_MUL: RUN(PFquMul);
    case CZK_PROBE_FQU_SQR: RUN(PFquSqr);
    case CZK_PROBE_FQU_MUL_ADD: RUN(PFquMulAdd);
    case CZK_PROBE_FQU_MUL_ADD_HI: RUN(PFquMulAddHi);
    case CZK_PROBE_FQU_MUL_HI: RUN(PFquMulHi);
    case CZK_PROBE_FQU_MUL_ADD4: RUN(PFquMulAdd4);
    case CZK_PROBE_FQU_MUL_S: RUN(PFquMulS);
    case CZK_PROBE_FQU_SQR_S: RUN(PFquSqrS);
    case CZK_PROBE_FQU_MUL_ADD_S: RUN(PFquMulAddS);
    case CZK_PROBE_FQU_MUL_ADD_HI_S: RUN(PFquMulAddHiS);
    case CZK_PROBE_FQU_MUL_HI_S: RUN(PFquMulHiS);
    case CZK_PROBE_FQU_MUL_ADD4_S: RUN(PFquMulAdd4S);
    case CZK_PROBE_FQU_NORMALIZE: RUN(PFquNormalize);
    case CZK_PROBE_FQU_SUB_LAZY_4: RUN(PFquSubLazy4);
    case CZK_PROBE_FQU_SUB_LAZY_8: RUN(PFquSubLazy8);
    case CZK_PROBE_FQU_SUB_LAZY_16: RUN(PFquSubLazy16);
    case CZK_PROBE_FQU_SUB3_NORM: RUN(PFquSub3Norm);
    case CZK_PROBE_FQU_UNPACK: RUN(PFquUnpack);
    case CZK_PROBE_FQU_PACK: RUN(PFquPack);
    case CZK_PROBE_FQU_NEG5: RUN(PFquNeg5);
    case CZK_PROBE_FQU_NEG5_BIG: RUN(PFquNeg5Big);
    case CZK_PROBE_FQU_ADD_LAZY: RUN(PFquAddLazy);
    case CZK_PROBE_FQU_SUBN_32: RUN(PFquSubn32);
    case CZK_PROBE_FQU_SUBN_64: RUN(PFquSubn64);
    case CZK_PROBE_FQU_SUBN_128: RUN(PFquSubn128);
    case CZK_PROBE_FQ2U_MUL: RUN(PFq2uMul);
    case CZK_PROBE_FQ2U_SQR: RUN(PFq2uSqr);
    case CZK_PROBE_FQ2U_MUL_N5: RUN(PFq2uMulN5);
    case CZK_PROBE_FQU_XYZZ_ACC_MIXED: RUN(PFquXyzzAccMixed);
    case CZK_PROBE_XYZZU_ADD: RUN(PXyzzuAdd);
    case CZK_PROBE_XYZZU_DOUBLE: RUN(PXyzzuDouble);
    case CZK_PROBE_XYZZU_TO_SAT: RUN(PXyzzuToSat);
    case CZK_PROBE_XYZZU_FROM_SAT: RUN(PXyzzuFromSat);
    case CZK_PROBE_FQ2U_XYZZ_ACC_MIXED: RUN(PFq2uXyzzAccMixed);
    case CZK_PROBE_TEU_FROM_NIELS: RUN(PTeuFromNiels);
    case CZK_PROBE_TEU_MADD: RUN(PTeuMadd);
    case CZK_PROBE_TEU_ADD: RUN(PTeuAdd);
    case CZK_PROBE_TEU_DOUBLE: RUN(PTeuDouble);
    case CZK_PROBE_TEU_TO_JAC: RUN(PTeuToJac);
    case CZK_PROBE_TE_LOAD_NIELS: RUN(PTeLoadNiels);
    case CZK_PROBE_P2_MUL: RUN(PP2Mul);
    case CZK_PROBE_XYZZU2_ADD: RUN(PXyzzu2Add);
    case CZK_PROBE_XYZZU2_DOUBLE: RUN(PXyzzu2Double);
    case CZK_PROBE_XYZZU2_ACC_MIXED: RUN(PXyzzu2AccMixed);
    case CZK_PROBE_FRU_MUL: RUN(PFruMul);
    case CZK_PROBE_FRU_NORMALIZE: RUN(PFruNormalize);
    case CZK_PROBE_FRU_UNPACK: RUN(PFruUnpack);
    case CZK_PROBE_FRU_PACK: RUN(PFruPack);
    case CZK_PROBE_FRU_REDUCE_2R: RUN(PFruReduce2r);
    case CZK_PROBE_FRU_CANON: RUN(PFruCanon);
    case CZK_PROBE_FRU_CANON_MULOUT: RUN(PFruCanonMulout);
    case CZK_PROBE_FRU_ADD: RUN(PFruAdd);
#define SUBS(LG)                                                   \
    case CZK_PROBE_FRU_SUB_BASE + 2 * LG: RUN(PFruSub<(1 << LG), 1>); \
    case CZK_PROBE_FRU_SUB_BASE + 2 * LG + 1: RUN(PFruSub<(1 << LG), 2>);
        SUBS(1) SUBS(2) SUBS(3) SUBS(4) SUBS(5) SUBS(6) SUBS(7) SUBS(8)
#undef SUBS
    default: break;
    }
#undef RUN
    if (op >= CZK_PROBE_SAT_BASE && op < CZK_PROBE_SAT_BASE + 2 * CZK_SAT_FN_COUNT) {
        const int fn = (op - CZK_PROBE_SAT_BASE) / 2;
        if ((op - CZK_PROBE_SAT_BASE) % 2) return sat_probe_noinline(ctx, fn, in, in_words_per_item, out, out_words_per_item, n, mem);
        return sat_probe_dispatch(ctx, fn, in, in_words_per_item, out, out_words_per_item, n, mem);
    }
    return set_err(ctx, CZK_ERR_ARG, "arith_probe: unknown op");
}
