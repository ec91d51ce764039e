// sat_probe.h -- LAB BUILD ONLY: the probes of the SATURATED arithmetic (field.h, tower.h, curve.h), one small kernel per function, fed raw
// u32 limbs from memory and storing raw limbs back.  See arith_probe.h for the op codes and tests/test_sat_arith.py for the user.
//
// This header is program text for TWO translation units, because build.py compiles field.h in two forms:
//   arith_probe.hip   the hot kernels' form (the Montgomery multiply inlined at every call site)
//   sat_probe.hip     -DCZK_NOINLINE_MUL, the form pairing.hip / point_codec.hip / msm.hip / lanes.hip / net.hip / net_rounds.hip are built with
// Each includes it inside its own anonymous namespace (inside namespace czk), so the functors and kernels have internal linkage and the
// two forms never meet at link time.  The Fq6 / Fq12 probes exist in the no-inline form only (#ifdef CZK_NOINLINE_MUL below): that
// is the only form the tower is ever compiled in.
//
// Item layouts: an Fr is 8 words, an Fq 12, an Fq2 24 (c0, c1), an Fq6 72 (c0, c1, c2), an Fq12 144 (c0, c1): the reference's nesting.
// Jac = (x, y, z), Affine = (x, y), XYZZ = (x, y, zz, zzz) of the base field.  A bool is one word (0 / 1).
//
// Not a stand-alone header: the including file has already included czk_internal.h, curve.h and tower.h.

template <class T>
struct SW;   // u32 words of a value in memory
template <class P>
struct SW<Fp<P>> {
    static constexpr int n = P::N;
};
template <>
struct SW<Fq2> {
    static constexpr int n = 24;
};
template <>
struct SW<Fq6> {
    static constexpr int n = 72;
};
template <>
struct SW<Fq12> {
    static constexpr int n = 144;
};
template <class F>
struct SW<Affine<F>> {
    static constexpr int n = 2 * SW<F>::n;
};
template <class F>
struct SW<Jac<F>> {
    static constexpr int n = 3 * SW<F>::n;
};
template <class F>
struct SW<XYZZ<F>> {
    static constexpr int n = 4 * SW<F>::n;
};

template <class P>
__device__ __forceinline__ void sp_ld(const u32* p, Fp<P>& r) {
#pragma unroll
    for (int i = 0; i < P::N; i++) r.l[i] = p[i];
}
template <class P>
__device__ __forceinline__ void sp_st(u32* p, const Fp<P>& a) {
#pragma unroll
    for (int i = 0; i < P::N; i++) p[i] = a.l[i];
}
__device__ __forceinline__ void sp_ld(const u32* p, Fq2& r) { sp_ld(p, r.c0), sp_ld(p + 12, r.c1); }
__device__ __forceinline__ void sp_st(u32* p, const Fq2& a) { sp_st(p, a.c0), sp_st(p + 12, a.c1); }
__device__ __forceinline__ void sp_ld(const u32* p, Fq6& r) { sp_ld(p, r.c0), sp_ld(p + 24, r.c1), sp_ld(p + 48, r.c2); }
__device__ __forceinline__ void sp_st(u32* p, const Fq6& a) { sp_st(p, a.c0), sp_st(p + 24, a.c1), sp_st(p + 48, a.c2); }
__device__ __forceinline__ void sp_ld(const u32* p, Fq12& r) { sp_ld(p, r.c0), sp_ld(p + 72, r.c1); }
__device__ __forceinline__ void sp_st(u32* p, const Fq12& a) { sp_st(p, a.c0), sp_st(p + 72, a.c1); }
template <class F>
__device__ __forceinline__ void sp_ld(const u32* p, Affine<F>& r) {
    sp_ld(p, r.x), sp_ld(p + SW<F>::n, r.y);
}
template <class F>
__device__ __forceinline__ void sp_st(u32* p, const Affine<F>& a) {
    sp_st(p, a.x), sp_st(p + SW<F>::n, a.y);
}
template <class F>
__device__ __forceinline__ void sp_ld(const u32* p, Jac<F>& r) {
    sp_ld(p, r.x), sp_ld(p + SW<F>::n, r.y), sp_ld(p + 2 * SW<F>::n, r.z);
}
template <class F>
__device__ __forceinline__ void sp_st(u32* p, const Jac<F>& a) {
    sp_st(p, a.x), sp_st(p + SW<F>::n, a.y), sp_st(p + 2 * SW<F>::n, a.z);
}
template <class F>
__device__ __forceinline__ void sp_ld(const u32* p, XYZZ<F>& r) {
    sp_ld(p, r.x), sp_ld(p + SW<F>::n, r.y), sp_ld(p + 2 * SW<F>::n, r.zz), sp_ld(p + 3 * SW<F>::n, r.zzz);
}
template <class F>
__device__ __forceinline__ void sp_st(u32* p, const XYZZ<F>& a) {
    sp_st(p, a.x), sp_st(p + SW<F>::n, a.y), sp_st(p + 2 * SW<F>::n, a.zz), sp_st(p + 3 * SW<F>::n, a.zzz);
}
template <class T>
__device__ __forceinline__ T sp_get(const u32* p) {
    T r;
    sp_ld(p, r);
    return r;
}

// ---- one functor per probed function.  IW / OW: words per item; run() sees the whole buffers, the item index and the item count.
// SPROBE's body sees i / o = this item's words, and W = the words of T.
#define SPROBE(NAME, TPARAM, T, IWORDS, OWORDS, ...)                                              \
    template <class TPARAM>                                                                       \
    struct NAME {                                                                                 \
        static constexpr int W = SW<T>::n, IW = IWORDS, OW = OWORDS;                              \
        static __device__ __forceinline__ void run(const u32* in, u32* out, size_t item, size_t) { \
            const u32* i = in + item * IW;                                                        \
            u32* o = out + item * OW;                                                             \
            __VA_ARGS__                                                                           \
        }                                                                                         \
    };
#define G sp_get

// Fp<P>
SPROBE(SFpAdd, P, Fp<P>, 2 * W, W, sp_st(o, fp_add(G<Fp<P>>(i), G<Fp<P>>(i + W)));)
SPROBE(SFpSub, P, Fp<P>, 2 * W, W, sp_st(o, fp_sub(G<Fp<P>>(i), G<Fp<P>>(i + W)));)
SPROBE(SFpDbl, P, Fp<P>, W, W, sp_st(o, fp_dbl(G<Fp<P>>(i)));)
SPROBE(SFpNeg, P, Fp<P>, W, W, sp_st(o, fp_neg(G<Fp<P>>(i)));)
SPROBE(SFpReduce, P, Fp<P>, W, W, Fp<P> a = G<Fp<P>>(i); fp_reduce(a); sp_st(o, a);)
SPROBE(SFpMul, P, Fp<P>, 2 * W, W, sp_st(o, fp_mul(G<Fp<P>>(i), G<Fp<P>>(i + W)));)
SPROBE(SFpSqr, P, Fp<P>, W, W, sp_st(o, fp_sqr(G<Fp<P>>(i)));)
SPROBE(SFpIntoRepr, P, Fp<P>, W, W, sp_st(o, fp_into_repr(G<Fp<P>>(i)));)
SPROBE(SFpFromRepr, P, Fp<P>, W, W, sp_st(o, fp_from_repr(G<Fp<P>>(i)));)
SPROBE(SFpInv, P, Fp<P>, W, W, sp_st(o, fp_inv(G<Fp<P>>(i)));)
SPROBE(SFqMulByNonresidue, X, Fq, W, W, sp_st(o, fq_mul_by_nonresidue(G<Fq>(i)));)

// the f_* overload set, for F = Fq2 and Fq6
SPROBE(SFAdd, F, F, 2 * W, W, sp_st(o, f_add(G<F>(i), G<F>(i + W)));)
SPROBE(SFSub, F, F, 2 * W, W, sp_st(o, f_sub(G<F>(i), G<F>(i + W)));)
SPROBE(SFDbl, F, F, W, W, sp_st(o, f_dbl(G<F>(i)));)
SPROBE(SFNeg, F, F, W, W, sp_st(o, f_neg(G<F>(i)));)
SPROBE(SFMul, F, F, 2 * W, W, sp_st(o, f_mul(G<F>(i), G<F>(i + W)));)
SPROBE(SFSqr, F, F, W, W, sp_st(o, f_sqr(G<F>(i)));)
SPROBE(SFInv, F, F, W, W, sp_st(o, f_inv(G<F>(i)));)
SPROBE(SFq2MulByU, X, Fq2, W, W, sp_st(o, fq2_mul_by_u(G<Fq2>(i)));)
SPROBE(SFq2MulFq, X, Fq2, W + 12, W, sp_st(o, fq2_mul_fq(G<Fq2>(i), G<Fq>(i + W)));)
SPROBE(SFq2Conj, X, Fq2, W, W, sp_st(o, fq2_conj(G<Fq2>(i)));)

// curve.h for F = Fq (G1) and Fq2 (G2); W = words of F
SPROBE(SJacDouble, F, F, 3 * W, 3 * W, sp_st(o, jac_double(G<Jac<F>>(i)));)
SPROBE(SJacAddMixed, F, F, 5 * W + 1, 3 * W, sp_st(o, jac_add_mixed(G<Jac<F>>(i), G<Affine<F>>(i + 3 * W), i[5 * W] != 0));)
SPROBE(SJacAdd, F, F, 6 * W, 3 * W, sp_st(o, jac_add(G<Jac<F>>(i), G<Jac<F>>(i + 3 * W)));)
SPROBE(SJacToAffine, F, F, 3 * W, 2 * W + 1, Affine<F> a; const bool inf = jac_to_affine(G<Jac<F>>(i), a); sp_st(o, a); o[2 * W] = inf ? 1u : 0u;)
SPROBE(SXyzzDoubleAffine, F, F, 2 * W, 4 * W, sp_st(o, xyzz_double_affine(G<Affine<F>>(i)));)
SPROBE(SXyzzDouble, F, F, 4 * W, 4 * W, sp_st(o, xyzz_double(G<XYZZ<F>>(i)));)
SPROBE(SXyzzAddMixed, F, F, 6 * W, 4 * W, sp_st(o, xyzz_add_mixed(G<XYZZ<F>>(i), G<Affine<F>>(i + 4 * W)));)
SPROBE(SXyzzAccMixed, F, F, 6 * W, 4 * W, XYZZ<F> a = G<XYZZ<F>>(i); const Affine<F> q = G<Affine<F>>(i + 4 * W);
       xyzz_acc_mixed(a.x, a.y, a.zz, a.zzz, q.x, q.y); sp_st(o, a);)
SPROBE(SXyzzAdd, F, F, 8 * W, 4 * W, sp_st(o, xyzz_add(G<XYZZ<F>>(i), G<XYZZ<F>>(i + 4 * W)));)
SPROBE(SXyzzToJac, F, F, 4 * W, 3 * W, sp_st(o, xyzz_to_jac(G<XYZZ<F>>(i)));)

#ifdef CZK_NOINLINE_MUL
// tower.h beyond the f_* set
SPROBE(SFq6MulByV, X, Fq6, W, W, sp_st(o, fq6_mul_by_v(G<Fq6>(i)));)
SPROBE(SFq6MulBy01, X, Fq6, W + 48, W, sp_st(o, fq6_mul_by_01(G<Fq6>(i), G<Fq2>(i + W), G<Fq2>(i + W + 24)));)
SPROBE(SFq6MulBy1, X, Fq6, W + 24, W, sp_st(o, fq6_mul_by_1(G<Fq6>(i), G<Fq2>(i + W)));)
template <int POWER>
struct SFq6Frobenius {
    static constexpr int IW = 72, OW = 72;
    static __device__ __forceinline__ void run(const u32* in, u32* out, size_t item, size_t) { sp_st(out + item * 72, fq6_frobenius(G<Fq6>(in + item * 72), POWER)); }
};
SPROBE(SFq12Conj, X, Fq12, W, W, sp_st(o, fq12_conj(G<Fq12>(i)));)
SPROBE(SFq12MulBy034, X, Fq12, W + 72, W, sp_st(o, fq12_mul_by_034(G<Fq12>(i), G<Fq2>(i + W), G<Fq2>(i + W + 24), G<Fq2>(i + W + 48)));)
SPROBE(SFq12CyclotomicSquare, X, Fq12, W, W, sp_st(o, fq12_cyclotomic_square(G<Fq12>(i)));)
template <int POWER>
struct SFq12Frobenius {
    static constexpr int IW = 144, OW = 144;
    static __device__ __forceinline__ void run(const u32* in, u32* out, size_t item, size_t) { sp_st(out + item * 144, fq12_frobenius(G<Fq12>(in + item * 144), POWER)); }
};
// fq12_load_strided: SoA across the n items (u64 word w of item t at in[w * stride + t]; SOA = false: stride 1, packed) -> packed words
// through sp_st, which shares nothing with the strided code.  fq12_store_strided: the other way round.  Every index is below 72 n u64.
template <bool SOA>
struct SFq12LoadStrided {
    static constexpr int IW = 144, OW = 144;
    static __device__ __forceinline__ void run(const u32* in, u32* out, size_t item, size_t n) {
        const u64* p = reinterpret_cast<const u64*>(in);
        sp_st(out + item * 144, SOA ? fq12_load_strided(p + item, n) : fq12_load_strided(p + item * 72, 1));
    }
};
template <bool SOA>
struct SFq12StoreStrided {
    static constexpr int IW = 144, OW = 144;
    static __device__ __forceinline__ void run(const u32* in, u32* out, size_t item, size_t n) {
        u64* p = reinterpret_cast<u64*>(out);
        const Fq12 a = G<Fq12>(in + item * 144);
        if (SOA)
            fq12_store_strided(p + item, n, a);
        else
            fq12_store_strided(p + item * 72, 1, a);
    }
};
#endif
#undef G
#undef SPROBE

// PAIR_BLOCK's launch bounds: the Fq12 probes hold 288+ words live and spill, as the pairing does
template <class OP>
__global__ __launch_bounds__(64) void k_sat_probe(const u32* in, u32* out, size_t n) {
    const size_t item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= n) return;
    OP::run(in, out, item, n);
}

template <class OP>
int sat_probe_run(czk_ctx* ctx, const uint32_t* in, size_t iw, uint32_t* out, size_t ow, size_t n, int mem) {
    if (iw != (size_t)OP::IW || ow != (size_t)OP::OW)
        return set_err(ctx, CZK_ERR_ARG, "arith_probe: this op takes " + std::to_string(OP::IW) + " words per item and returns " + std::to_string(OP::OW));
    if (!n) return CZK_OK;
    Staged si{ctx}, so{ctx};
    CZK_TRY(si.to_device(in, n * iw * 4, mem));
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST ? nullptr : out, n * ow * 4, mem));
    hipLaunchKernelGGL(k_sat_probe<OP>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, (const u32*)si.dev, (u32*)so.dev, n);
    CZK_HIP(ctx, hipGetLastError());
    return so.to_host(out, n * ow * 4);
}

// `fn` = index into enum czk_lab_sat_fn (arith_probe.h); the caller has validated ctx, the pointers, mem and n
inline int sat_probe_dispatch(czk_ctx* ctx, int fn, const uint32_t* in, size_t iw, uint32_t* out, size_t ow, size_t n, int mem) {
#define RUN(...) return sat_probe_run<__VA_ARGS__>(ctx, in, iw, out, ow, n, mem)
#define FP_CASES(BASE, P)                                   \
    case BASE + CZK_SAT_FP_ADD: RUN(SFpAdd<P>);             \
    case BASE + CZK_SAT_FP_SUB: RUN(SFpSub<P>);             \
    case BASE + CZK_SAT_FP_DBL: RUN(SFpDbl<P>);             \
    case BASE + CZK_SAT_FP_NEG: RUN(SFpNeg<P>);             \
    case BASE + CZK_SAT_FP_REDUCE: RUN(SFpReduce<P>);       \
    case BASE + CZK_SAT_FP_MUL: RUN(SFpMul<P>);             \
    case BASE + CZK_SAT_FP_SQR: RUN(SFpSqr<P>);             \
    case BASE + CZK_SAT_FP_INTO_REPR: RUN(SFpIntoRepr<P>);  \
    case BASE + CZK_SAT_FP_FROM_REPR: RUN(SFpFromRepr<P>);  \
    case BASE + CZK_SAT_FP_INV: RUN(SFpInv<P>);
#define CURVE_CASES(BASE, F)                                        \
    case BASE + CZK_SAT_JAC_DOUBLE: RUN(SJacDouble<F>);             \
    case BASE + CZK_SAT_JAC_ADD_MIXED: RUN(SJacAddMixed<F>);        \
    case BASE + CZK_SAT_JAC_ADD: RUN(SJacAdd<F>);                   \
    case BASE + CZK_SAT_JAC_TO_AFFINE: RUN(SJacToAffine<F>);        \
    case BASE + CZK_SAT_XYZZ_DOUBLE_AFFINE: RUN(SXyzzDoubleAffine<F>); \
    case BASE + CZK_SAT_XYZZ_DOUBLE: RUN(SXyzzDouble<F>);           \
    case BASE + CZK_SAT_XYZZ_ADD_MIXED: RUN(SXyzzAddMixed<F>);      \
    case BASE + CZK_SAT_XYZZ_ACC_MIXED: RUN(SXyzzAccMixed<F>);      \
    case BASE + CZK_SAT_XYZZ_ADD: RUN(SXyzzAdd<F>);                 \
    case BASE + CZK_SAT_XYZZ_TO_JAC: RUN(SXyzzToJac<F>);
    switch (fn) {
        FP_CASES(CZK_SAT_FR_BASE, FrParams)
        FP_CASES(CZK_SAT_FQ_BASE, FqParams)
    case CZK_SAT_FQ_MUL_BY_NONRESIDUE: RUN(SFqMulByNonresidue<void>);
    case CZK_SAT_FQ2_ADD: RUN(SFAdd<Fq2>);
    case CZK_SAT_FQ2_SUB: RUN(SFSub<Fq2>);
    case CZK_SAT_FQ2_DBL: RUN(SFDbl<Fq2>);
    case CZK_SAT_FQ2_NEG: RUN(SFNeg<Fq2>);
    case CZK_SAT_FQ2_MUL: RUN(SFMul<Fq2>);
    case CZK_SAT_FQ2_SQR: RUN(SFSqr<Fq2>);
    case CZK_SAT_FQ2_INV: RUN(SFInv<Fq2>);
    case CZK_SAT_FQ2_MUL_BY_U: RUN(SFq2MulByU<void>);
    case CZK_SAT_FQ2_MUL_FQ: RUN(SFq2MulFq<void>);
    case CZK_SAT_FQ2_CONJ: RUN(SFq2Conj<void>);
        CURVE_CASES(CZK_SAT_G1_BASE, Fq)
        CURVE_CASES(CZK_SAT_G2_BASE, Fq2)
#ifdef CZK_NOINLINE_MUL
    case CZK_SAT_FQ6_ADD: RUN(SFAdd<Fq6>);
    case CZK_SAT_FQ6_SUB: RUN(SFSub<Fq6>);
    case CZK_SAT_FQ6_NEG: RUN(SFNeg<Fq6>);
    case CZK_SAT_FQ6_MUL_BY_V: RUN(SFq6MulByV<void>);
    case CZK_SAT_FQ6_MUL: RUN(SFMul<Fq6>);
    case CZK_SAT_FQ6_MUL_BY_01: RUN(SFq6MulBy01<void>);
    case CZK_SAT_FQ6_MUL_BY_1: RUN(SFq6MulBy1<void>);
    case CZK_SAT_FQ6_INV: RUN(SFInv<Fq6>);
    case CZK_SAT_FQ6_FROBENIUS_1: RUN(SFq6Frobenius<1>);
    case CZK_SAT_FQ6_FROBENIUS_2: RUN(SFq6Frobenius<2>);
    case CZK_SAT_FQ12_MUL: RUN(SFMul<Fq12>);
    case CZK_SAT_FQ12_SQR: RUN(SFSqr<Fq12>);
    case CZK_SAT_FQ12_CONJ: RUN(SFq12Conj<void>);
    case CZK_SAT_FQ12_INV: RUN(SFInv<Fq12>);
    case CZK_SAT_FQ12_MUL_BY_034: RUN(SFq12MulBy034<void>);
    case CZK_SAT_FQ12_FROBENIUS_1: RUN(SFq12Frobenius<1>);
    case CZK_SAT_FQ12_FROBENIUS_2: RUN(SFq12Frobenius<2>);
    case CZK_SAT_FQ12_CYCLOTOMIC_SQUARE: RUN(SFq12CyclotomicSquare<void>);
    case CZK_SAT_FQ12_LOAD_STRIDED_1: RUN(SFq12LoadStrided<false>);
    case CZK_SAT_FQ12_STORE_STRIDED_1: RUN(SFq12StoreStrided<false>);
    case CZK_SAT_FQ12_LOAD_STRIDED_N: RUN(SFq12LoadStrided<true>);
    case CZK_SAT_FQ12_STORE_STRIDED_N: RUN(SFq12StoreStrided<true>);
#endif
    default: return set_err(ctx, CZK_ERR_ARG, "arith_probe: unknown op (the Fq6 / Fq12 probes exist in the no-inline form only)");
    }
#undef CURVE_CASES
#undef FP_CASES
#undef RUN
}
