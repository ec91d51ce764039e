// fr_vec.hip -- the pointwise kernels over vectors of BLS12-377 Fr and their entry points: czk_fr_vec_op, czk_fr_vec_scale,
// czk_fr_beaver_combine, czk_fr_spdz_open, czk_fr_into_repr / czk_fr_from_repr and czk_spdz_open_combine.
//
// Every kernel is a grid-stride loop, one Fr per thread-iteration (2 x 16 B accesses per element), launched with blocks of 256 under the
// cap of fr_grid.  The build has no relocatable device code, so a kernel is launched from this unit only: the transform (ntt.hip) and the
// witness map (witness_map.hip) reach k_vec_op and k_sub_scale through fr_vec_op_launch / fr_sub_scale_launch.
// Arithmetic is integer VALU (v_mad_u64_u32); there is no MFMA-shaped work here.
#include "call.h"

namespace czk {

__device__ __forceinline__ Fr gfr_load(const u64* base, size_t idx) { return fp_load<FrParams>(base + 4 * idx); }
__device__ __forceinline__ void gfr_store(u64* base, size_t idx, const Fr& v) { fp_store<FrParams>(base + 4 * idx, v); }

// ------------------------------------------------------------------------------------------------
// pointwise kernels (grid-stride, one Fr per thread-iteration, 2 x 16 B accesses per element)
// ------------------------------------------------------------------------------------------------
__global__ void k_vec_op(int op, const u64* a, const u64* b, u64* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr x = gfr_load(a, i), y = gfr_load(b, i), r;
        if (op == CZK_OP_ADD) r = fp_add(x, y);
        else if (op == CZK_OP_SUB) r = fp_sub(x, y);
        else r = fp_mul(x, y);
        gfr_store(out, i, r);
    }
}
__global__ void k_vec_scale(const u64* a, Fr k, u64* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        gfr_store(out, i, fp_mul(gfr_load(a, i), k));
}
// the same with the scalar read from DEVICE memory (czk_fr_vec_scale with CZK_MEM_DEVICE): no host round trip, no stream synchronisation
__global__ void k_vec_scale_dev(const u64* a, const u64* kp, u64* out, size_t n) {
    const Fr k = gfr_load(kp, 0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        gfr_store(out, i, fp_mul(gfr_load(a, i), k));
}
// (ab - c) * k  -- r1cs_to_qap.rs:105-109 fused
__global__ void k_sub_scale(const u64* ab, const u64* c, Fr k, u64* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        gfr_store(out, i, fp_mul(fp_sub(gfr_load(ab, i), gfr_load(c, i)), k));
}
__global__ void k_beaver(const u64* x, const u64* y, const u64* z, const u64* sx, const u64* oy, int add_open, u64* out,
                         size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr vsx = gfr_load(sx, i), voy = gfr_load(oy, i);
        Fr r = fp_sub(gfr_load(z, i), fp_mul(gfr_load(y, i), vsx));
        r = fp_sub(r, fp_mul(gfr_load(x, i), voy));
        if (add_open) r = fp_add(r, fp_mul(vsx, voy));
        gfr_store(out, i, r);
    }
}
__global__ void k_repr(int to_mont, const u64* a, u64* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr v = gfr_load(a, i);
        gfr_store(out, i, to_mont ? fp_from_repr(v) : fp_into_repr(v));
    }
}

// SpdzFieldShare::batch_open, local part (share/spdz.rs:166-185): value = sum of the parties' sh lanes; the MAC
// check sum_p (mac_share_p * value - mac_p) must vanish; non-zero entries are counted
__global__ void k_spdz_open(const u64* shares, size_t parties, size_t n, u64* out_value, unsigned long long* bad) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr v = gfr_load(shares, i);                       // party 0, sh lane
        Fr chk = fp_neg(gfr_load(shares + 4 * n, i));     // - mac_0
        for (size_t p = 1; p < parties; p++) {
            v = fp_add(v, gfr_load(shares + 4 * n * (2 * p), i));
            chk = fp_sub(chk, gfr_load(shares + 4 * n * (2 * p + 1), i));
        }
        chk = fp_add(chk, v);                             // + mac_share_0 * value, mac_share_0 = 1 (king)
        gfr_store(out_value, i, v);
        if (!chk.is_zero()) atomicAdd(bad, 1ull);
    }
}

// blocks of 256 for n elements, at most 8 per CU (the loops above take the rest)
static unsigned fr_grid(czk_ctx* ctx, size_t n) {
    size_t blocks = (n + 255) / 256;
    size_t cap = (size_t)ctx->num_cu * 8;
    if (blocks > cap) blocks = cap;
    return blocks ? (unsigned)blocks : 1u;
}

// The two local opens of S::batch_mul and its combine (share/field.rs:97-127, share/spdz.rs:166-185) for the layout where every party's (sh, mac) lanes are on
// this GPU: per index the masked a = s + x and b = o + y lanes are read once, sx / oy / the two MAC-check values are written once and every lane's product share
// z - y sx - x oy (+ sx oy on the lanes of `king_mask`) follows from registers.  The values of k_vec_op ADD / SUB per open and k_beaver per lane.
__global__ void k_spdz_open_combine(const u64* a, const u64* b, const u64* tx, const u64* ty, const u64* tz, unsigned parties, unsigned long long king_mask, u64* sx,
                                    u64* oy, u64* chk_a, u64* chk_b, u64* ab, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr vsx = gfr_load(a, i), voy = gfr_load(b, i);                           // party 0, sh lane
        for (unsigned p = 1; p < parties; p++) {
            vsx = fp_add(vsx, gfr_load(a + 4 * n * (2 * p), i));
            voy = fp_add(voy, gfr_load(b + 4 * n * (2 * p), i));
        }
        Fr ca = vsx, cb = voy;                                                   // mac_share * value - sum of the mac lanes, mac_share = 1
        for (unsigned p = 0; p < parties; p++) {
            ca = fp_sub(ca, gfr_load(a + 4 * n * (2 * p + 1), i));
            cb = fp_sub(cb, gfr_load(b + 4 * n * (2 * p + 1), i));
        }
        gfr_store(sx, i, vsx);
        gfr_store(oy, i, voy);
        gfr_store(chk_a, i, ca);
        gfr_store(chk_b, i, cb);
        const Fr open = fp_mul(vsx, voy);
        for (unsigned ln = 0; ln < 2 * parties; ln++) {
            Fr r = fp_sub(gfr_load(tz + 4 * n * ln, i), fp_mul(gfr_load(ty + 4 * n * ln, i), vsx));
            r = fp_sub(r, fp_mul(gfr_load(tx + 4 * n * ln, i), voy));
            if ((king_mask >> ln) & 1ull) r = fp_add(r, open);
            gfr_store(ab + 4 * n * ln, i, r);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers for the other units (device buffers; enqueue only, the caller asks hipGetLastError)
// ------------------------------------------------------------------------------------------------
void fr_vec_op_launch(czk_ctx* ctx, int op, const u64* a, const u64* b, u64* out, size_t n) {
    hipLaunchKernelGGL(k_vec_op, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, op, a, b, out, n);
}
void fr_sub_scale_launch(czk_ctx* ctx, const u64* ab, const u64* c, const Fr& k, u64* out, size_t n) {
    hipLaunchKernelGGL(k_sub_scale, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, ab, c, k, out, n);
}

// The host side of a non-empty pointwise call whose arguments have been checked: N input vectors and one output of n Fr each, all in `mem`.
// The staging pool is asked for the inputs in argument order, then for the output; launch(in, out) enqueues the kernel on the device
// pointers; to_host of the output is the call's single blocking point (device memory: nothing to copy, the call only enqueues).
template <size_t N, class Launch>
static int fr_pointwise(czk_ctx* ctx, const uint64_t* const (&in)[N], uint64_t* out, size_t n, int mem, Launch&& launch) {
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    Staged si[N]{}, so{ctx};
    const u64* d[N];
    for (size_t i = 0; i < N; i++) {
        si[i].ctx = ctx;
        CZK_TRY(si[i].to_device(in[i], n * 32, mem));
        d[i] = (const u64*)si[i].dev;
    }
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST ? nullptr : out, n * 32, mem));
    launch(d, (u64*)so.dev);
    CZK_HIP(ctx, hipGetLastError());
    return so.to_host(out, n * 32);
}

}  // namespace czk

using namespace czk;

// ------------------------------------------------------------------------------------------------
// C ABI (pointwise part)
// ------------------------------------------------------------------------------------------------
extern "C" int czk_fr_vec_op(czk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, int mem) {
    if (!ctx || (n && (!a || !b || !out)) || op < 0 || op > 2) return ctx ? set_err(ctx, CZK_ERR_ARG, "bad vec_op argument") : CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (!n) return CZK_OK;
    return fr_pointwise(ctx, {a, b}, out, n, mem, [&](const u64* const* d, u64* o) {
        hipLaunchKernelGGL(k_vec_op, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, op, d[0], d[1], o, n);
    });
}

extern "C" int czk_fr_vec_scale(czk_ctx* ctx, const uint64_t* a, const uint64_t* k, uint64_t* out, size_t n, int mem) {
    if (!ctx || !k || (n && (!a || !out))) return ctx ? set_err(ctx, CZK_ERR_ARG, "bad vec_scale argument") : CZK_ERR_ARG;
    const bool host_scalar = mem == (CZK_MEM_DEVICE | CZK_MEM_SCALAR_HOST);
    if (!host_scalar && !valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST, CZK_MEM_DEVICE or CZK_MEM_DEVICE | CZK_MEM_SCALAR_HOST");
    if (!n) return CZK_OK;
    if (host_scalar) {   // device vectors, the scalar by value with the launch
        CZK_HIP(ctx, hipSetDevice(ctx->device));
        hipLaunchKernelGGL(k_vec_scale, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, (const u64*)a, host_fr(k), (u64*)out, n);
        CZK_HIP(ctx, hipGetLastError());
        return CZK_OK;
    }
    if (mem == CZK_MEM_DEVICE) {
        // the scalar lives in device memory like the vectors: read it in the kernel (a copy to the host would synchronise the stream -- a
        // full pipeline stall in the middle of a prover's round, which is what this call cost the Plonk / Marlin drivers until round 4)
        CZK_HIP(ctx, hipSetDevice(ctx->device));
        hipLaunchKernelGGL(k_vec_scale_dev, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, a, k, out, n);
        CZK_HIP(ctx, hipGetLastError());
        return CZK_OK;
    }
    const Fr kk = host_fr(k);   // host memory: the vectors are staged, the scalar goes by value with the launch
    return fr_pointwise(ctx, {a}, out, n, mem, [&](const u64* const* d, u64* o) {
        hipLaunchKernelGGL(k_vec_scale, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, d[0], kk, o, n);
    });
}

extern "C" int czk_fr_beaver_combine(czk_ctx* ctx, const uint64_t* x, const uint64_t* y, const uint64_t* z, const uint64_t* sx,
                                     const uint64_t* oy, int add_open, uint64_t* out, size_t n, int mem) {
    if (!ctx || (n && (!x || !y || !z || !sx || !oy || !out))) return ctx ? set_err(ctx, CZK_ERR_ARG, "null beaver argument") : CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (!n) return CZK_OK;
    return fr_pointwise(ctx, {x, y, z, sx, oy}, out, n, mem, [&](const u64* const* d, u64* o) {
        hipLaunchKernelGGL(k_beaver, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, d[0], d[1], d[2], d[3], d[4], add_open, o, n);
    });
}

extern "C" int czk_fr_spdz_open(czk_ctx* ctx, const uint64_t* shares, size_t parties, size_t n, uint64_t* out_value, uint64_t* out_bad) {
    if (!ctx || !out_bad || (n && (!shares || !out_value)) || parties == 0) return ctx ? set_err(ctx, CZK_ERR_ARG, "bad spdz_open argument") : CZK_ERR_ARG;
    *out_bad = 0;
    if (!n) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->open_bad) CZK_HIP(ctx, hipMalloc(&ctx->open_bad, 8));
    unsigned long long* bad = ctx->open_bad;
    CZK_HIP(ctx, hipMemsetAsync(bad, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_spdz_open, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, (const u64*)shares, parties, n, (u64*)out_value, bad);
    CZK_HIP(ctx, hipGetLastError());
    unsigned long long hb = 0;
    CZK_HIP(ctx, hipMemcpyAsync(&hb, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the count is the call's result: the reference asserts on it right here
    *out_bad = hb;
    return CZK_OK;
}

static int repr_common(czk_ctx* ctx, int to_mont, const uint64_t* a, uint64_t* out, size_t n, int mem) {
    if (!ctx || (n && (!a || !out))) return ctx ? set_err(ctx, CZK_ERR_ARG, "null repr argument") : CZK_ERR_ARG;
    CZK_TRY(check_mem(ctx, mem));
    if (!n) return CZK_OK;
    return fr_pointwise(ctx, {a}, out, n, mem, [&](const u64* const* d, u64* o) {
        hipLaunchKernelGGL(k_repr, dim3(fr_grid(ctx, n)), dim3(256), 0, ctx->stream, to_mont, d[0], o, n);
    });
}
extern "C" int czk_fr_into_repr(czk_ctx* ctx, const uint64_t* a, uint64_t* out, size_t n, int mem) { return repr_common(ctx, 0, a, out, n, mem); }
extern "C" int czk_fr_from_repr(czk_ctx* ctx, const uint64_t* a, uint64_t* out, size_t n, int mem) { return repr_common(ctx, 1, a, out, n, mem); }

extern "C" int czk_spdz_open_combine(czk_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, size_t parties,
                                     uint64_t king_mask, uint64_t* sx, uint64_t* oy, uint64_t* chk_a, uint64_t* chk_b, uint64_t* ab, size_t n) {
    if (!ctx) return CZK_ERR_ARG;
    if (parties == 0 || parties > 32) return set_err(ctx, CZK_ERR_ARG, "spdz_open_combine: 1 to 32 parties (the king mask has one bit per lane)");
    if (n && (!a || !b || !tx || !ty || !tz || !sx || !oy || !chk_a || !chk_b || !ab)) return set_err(ctx, CZK_ERR_ARG, "null spdz_open_combine argument");
    if (!n) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned g = fr_grid(ctx, n);
    if (!(ctx->witness_map_short & 4)) {   // the sequence of before: three pointwise kernels per open (P = 2), one combine per lane
        auto op = [&](int o, const u64* x, const u64* y, u64* out) { hipLaunchKernelGGL(k_vec_op, dim3(g), dim3(256), 0, ctx->stream, o, x, y, out, n); };
        const u64* src[2] = {(const u64*)a, (const u64*)b};
        u64* val[2] = {(u64*)sx, (u64*)oy};
        u64* chk[2] = {(u64*)chk_a, (u64*)chk_b};
        for (int v = 0; v < 2; v++) {
            if (parties == 1) {
                CZK_HIP(ctx, hipMemcpyAsync(val[v], src[v], n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            } else {
                op(CZK_OP_ADD, src[v], src[v] + 4 * n * 2, val[v]);
                for (size_t p = 2; p < parties; p++) op(CZK_OP_ADD, val[v], src[v] + 4 * n * 2 * p, val[v]);
            }
            op(CZK_OP_SUB, val[v], src[v] + 4 * n, chk[v]);
            for (size_t p = 1; p < parties; p++) op(CZK_OP_SUB, chk[v], src[v] + 4 * n * (2 * p + 1), chk[v]);
        }
        for (size_t ln = 0; ln < 2 * parties; ln++)
            hipLaunchKernelGGL(k_beaver, dim3(g), dim3(256), 0, ctx->stream, (const u64*)tx + 4 * n * ln, (const u64*)ty + 4 * n * ln, (const u64*)tz + 4 * n * ln,
                               (const u64*)sx, (const u64*)oy, (int)((king_mask >> ln) & 1), (u64*)ab + 4 * n * ln, n);
        CZK_HIP(ctx, hipGetLastError());
        return CZK_OK;
    }
    hipLaunchKernelGGL(k_spdz_open_combine, dim3(g), dim3(256), 0, ctx->stream, (const u64*)a, (const u64*)b, (const u64*)tx, (const u64*)ty, (const u64*)tz,
                       (unsigned)parties, (unsigned long long)king_mask, (u64*)sx, (u64*)oy, (u64*)chk_a, (u64*)chk_b, (u64*)ab, n);
    CZK_HIP(ctx, hipGetLastError());
    return CZK_OK;
}
