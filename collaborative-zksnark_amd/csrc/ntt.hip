// ntt.hip -- batched in-order radix-2 NTT over BLS12-377 Fr for gfx950: the first-generation pass kernels, the domain object and its
// tables, the driver ntt_device and the entry points czk_ntt_fr / czk_ntt_fr_to / czk_domain_constants.  (The second-generation passes:
// ntt_pass.hip.  The pointwise Fr calls: fr_vec.hip.  The Groth16 witness map, a client of the transform: witness_map.hip.)
//
// Replaces (value-for-value, every output limb identical):
//   Radix2EvaluationDomain::{fft,ifft,coset_ifft}_in_place   algebra/poly/src/domain/radix2/mod.rs:99-117
//   EvaluationDomain::coset_fft_in_place (trait default)        algebra/poly/src/domain/mod.rs:139-142
//   io_helper / oi_helper / derange                             algebra/poly/src/domain/radix2/fft.rs:140-260
//
// Design (MI355X-first, not the reference's stage-by-stage sweep over DRAM):
//   * log2 D stages are split into ceil(n/7) passes; a pass keeps a (2^K rows x T columns) tile of Fr in
//     LDS (K<=7, T<=16: 64 KiB, 68.5 KiB for the padded last pass at K = 7 -- within gfx950's 160 KiB per CU for two workgroups;
//     checked against the device at launch) and runs its K decimation-in-frequency stages there,
//     so a 2^21 transform touches HBM 3 times instead of 21 (+ a separate bit-reversal sweep).
//   * strided passes read/write T consecutive elements per row (512 B runs); the last pass owns T contiguous
//     2^K chunks whose bit-reversed chunk ids are consecutive, so its transposed store is the bit-reversal
//     permutation AND is written in 512 B runs: natural order in, natural order out, no derange kernel.
//   * coset pre-scale (g^i), zero-extension to D, and the inverse's 1/D (or 1/D * g^-i) post-scale are fused
//     into the first load / last store.
//   * twiddles: one per-stage-compacted table per domain (D-1 entries, like the reference's cache-aligned
//     root compaction fft.rs:194-200) so a wave reads consecutive entries; the last pass stages its 2^K-1
//     twiddles in LDS.
//   * lanes (sh / mac share lanes, several parties) ride on gridDim.y.
// Arithmetic is integer VALU (v_mad_u64_u32); there is no MFMA-shaped work here.
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "czk_internal.h"
#include "ntt_pass.h"

namespace czk {

// ------------------------------------------------------------------------------------------------
// LDS helpers: an Fr is two 16-byte slots
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fr lds_get(const uint4* s, unsigned idx) {
    uint4 a = s[2 * idx], b = s[2 * idx + 1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}
__device__ __forceinline__ void lds_put(uint4* s, unsigned idx, const Fr& v) {
    s[2 * idx] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    s[2 * idx + 1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ Fr gfr_load(const u64* base, size_t idx) { return fp_load<FrParams>(base + 4 * idx); }
__device__ __forceinline__ void gfr_store(u64* base, size_t idx, const Fr& v) { fp_store<FrParams>(base + 4 * idx, v); }

__device__ __forceinline__ unsigned bitrev(unsigned v, unsigned bits) {
    return bits ? (__brev(v) >> (32 - bits)) : 0u;
}

struct PassArgs {
    const u64* in;
    u64* out;
    const u64* tw;        // per-stage compacted twiddles
    const u64* prescale;  // g^i table or null (first pass of a coset fft)
    const u64* posttab;   // size_inv * g^-i table or null (last pass of a coset ifft)
    Fr postconst;         // size_inv (last pass of an ifft)
    int post_mode;        // 0 none, 1 constant, 2 table
    unsigned n;           // log2 D
    unsigned s_lo;        // lowest stage bit of this pass
    unsigned K;           // stages in this pass
    unsigned logT;        // log2 columns
    size_t in_len;        // elements >= in_len read as zero (only honoured when `first`)
    int first;
    size_t lane_stride;   // elements between lanes (= D)
    size_t in_lane_stride;   // ... of `in` in the first pass (out-of-place transforms read the caller's source lanes)
};

// One strided pass: stage bits [s_lo, s_lo + K), s_lo > 0.
__global__ __launch_bounds__(256) void k_ntt_strided(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    const unsigned tid = threadIdx.x;
    const unsigned T = 1u << a.logT;
    const unsigned rows = 1u << a.K;
    const unsigned lb_bits = a.s_lo - a.logT;
    const unsigned B = blockIdx.x;
    const unsigned Lb = B & ((1u << lb_bits) - 1u);
    const size_t H = B >> lb_bits;
    const size_t base = (H << (a.s_lo + a.K)) | ((size_t)Lb << a.logT);
    const u64* in = a.in + 4 * (a.first ? a.in_lane_stride : a.lane_stride) * blockIdx.y;
    u64* out = a.out + 4 * a.lane_stride * blockIdx.y;

    for (unsigned e = tid; e < rows * T; e += 256) {
        unsigned r = e >> a.logT, t = e & (T - 1);
        size_t gi = base | ((size_t)r << a.s_lo) | t;
        Fr v;
        if (!a.first || gi < a.in_len) {
            v = gfr_load(in, gi);
            if (a.prescale) v = fp_mul(v, gfr_load(a.prescale, gi));
        } else {
            v = Fr::zero();
        }
        lds_put(smem, e, v);
    }
    __syncthreads();
    const unsigned low0 = Lb << a.logT;
    for (int q = (int)a.K - 1; q >= 0; q--) {
        const unsigned s = a.s_lo + q;
        const u64* tws = a.tw + 4 * (((size_t)1 << s) - 1);
        for (unsigned bf = tid; bf < (rows >> 1) * T; bf += 256) {
            unsigned t = bf & (T - 1), rr = bf >> a.logT;
            unsigned rlow = rr & ((1u << q) - 1u);
            unsigned r0 = ((rr >> q) << (q + 1)) | rlow;
            unsigned r1 = r0 | (1u << q);
            Fr lo = lds_get(smem, r0 * T + t), hi = lds_get(smem, r1 * T + t);
            size_t j = ((size_t)rlow << a.s_lo) | (low0 | t);   // element index mod 2^s
            Fr w = gfr_load(tws, j);
            lds_put(smem, r0 * T + t, fp_add(lo, hi));
            lds_put(smem, r1 * T + t, fp_mul(fp_sub(lo, hi), w));
        }
        __syncthreads();
    }
    for (unsigned e = tid; e < rows * T; e += 256) {
        unsigned r = e >> a.logT, t = e & (T - 1);
        size_t gi = base | ((size_t)r << a.s_lo) | t;
        gfr_store(out, gi, lds_get(smem, e));
    }
}

// Last pass: stage bits [0, K); T contiguous chunks of 2^K; transposed (bit-reversing) store.
__global__ __launch_bounds__(256) void k_ntt_final(PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    const unsigned tid = threadIdx.x;
    const unsigned T = 1u << a.logT;
    const unsigned c = a.K;
    const unsigned len = 1u << c;
    const unsigned RS = len + 1;   // padded row stride (elements): transposed reads stay <= 2-way conflicted
    uint4* tw_lds = smem + 2 * (size_t)RS * T;
    const unsigned hb = a.n - c;   // bits of the chunk id
    const unsigned B = blockIdx.x;
    const u64* in = a.in + 4 * (a.first ? a.in_lane_stride : a.lane_stride) * blockIdx.y;
    u64* out = a.out + 4 * a.lane_stride * blockIdx.y;

    for (unsigned e = tid; e + 1 < len; e += 256) lds_put(tw_lds, e, gfr_load(a.tw, e));   // stages 0..c-1: 2^c - 1 entries
    for (unsigned e = tid; e < len * T; e += 256) {
        unsigned t = e >> c, l = e & (len - 1);
        size_t h = bitrev(B * T + t, hb);
        size_t gi = (h << c) | l;
        Fr v;
        if (!a.first || gi < a.in_len) {
            v = gfr_load(in, gi);
            if (a.prescale) v = fp_mul(v, gfr_load(a.prescale, gi));
        } else {
            v = Fr::zero();
        }
        lds_put(smem, t * RS + l, v);
    }
    __syncthreads();
    for (int q = (int)c - 1; q >= 0; q--) {
        for (unsigned bf = tid; bf < (len >> 1) * T; bf += 256) {
            unsigned t = bf >> (c - 1), rr = bf & ((len >> 1) - 1);
            unsigned llow = rr & ((1u << q) - 1u);
            unsigned l0 = ((rr >> q) << (q + 1)) | llow;
            unsigned l1 = l0 | (1u << q);
            Fr lo = lds_get(smem, t * RS + l0), hi = lds_get(smem, t * RS + l1);
            lds_put(smem, t * RS + l0, fp_add(lo, hi));
            // the last stage's only twiddle is w^0 = 1 (the reference multiplies by roots[0] = 1, fft.rs:167-180: same value)
            Fr d = fp_sub(lo, hi);
            lds_put(smem, t * RS + l1, q == 0 ? d : fp_mul(d, lds_get(tw_lds, ((1u << q) - 1u) + llow)));
        }
        __syncthreads();
    }
    for (unsigned e = tid; e < len * T; e += 256) {
        unsigned t = e & (T - 1), l = e >> a.logT;
        size_t k = ((size_t)bitrev(l, c) << hb) | (size_t)(B * T + t);
        Fr v = lds_get(smem, t * RS + l);
        if (a.post_mode == 1) v = fp_mul(v, a.postconst);
        else if (a.post_mode == 2) v = fp_mul(v, gfr_load(a.posttab, k));
        gfr_store(out, k, v);
    }
}

// ------------------------------------------------------------------------------------------------
// table generation
// ------------------------------------------------------------------------------------------------
// out[i] = c * base^i for i < count; each thread owns 64 consecutive entries.
__global__ void k_pow_table(u64* out, size_t count, Fr base, Fr c) {
    size_t chunk = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t start = chunk * 64;
    if (start >= count) return;
    Fr v = fp_mul(c, fp_pow_u64(base, (u64)start));
    size_t end = start + 64 < count ? start + 64 : count;
    for (size_t i = start; i < end; i++) {
        gfr_store(out, i, v);
        v = fp_mul(v, base);
    }
}

struct StageRoots {
    Fr w[48];   // w[s] = root^(2^(n-1-s)) for s < n  (TWO_ADICITY = 47 bounds n)
};
// flat per-stage table: entry (2^s - 1 + j) = w[s]^j, j < 2^s
__global__ void k_twiddle_table(u64* out, unsigned n, const StageRoots* roots) {
    size_t chunk = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = ((size_t)1 << n) - 1;
    size_t start = chunk * 64;
    if (start >= total) return;
    size_t end = start + 64 < total ? start + 64 : total;
    unsigned s_prev = 0xffffffffu;
    Fr v = Fr::one(), w = Fr::one();
    for (size_t i = start; i < end; i++) {
        unsigned s = 63 - __clzll((unsigned long long)(i + 1));
        size_t j = (i + 1) - ((size_t)1 << s);
        if (s != s_prev) {
            w = roots->w[s];
            v = fp_pow_u64(w, (u64)j);
            s_prev = s;
        }
        gfr_store(out, i, v);
        v = fp_mul(v, w);
    }
}

// ------------------------------------------------------------------------------------------------
// domain object (host side of Radix2EvaluationDomain::new, radix2/mod.rs:51-82)
// ------------------------------------------------------------------------------------------------
static Fr host_root_of_unity(unsigned log_n) {
    // fr.rs:21-28 LARGE_SUBGROUP_ROOT_OF_UNITY (Montgomery), cubed, then squared 47 - log_n times
    Fr large;
    const u32 lr[8] = {0xc790c167u, 0x9bfe9d90u, 0x39013bffu, 0x7175a69eu, 0xadabcf93u, 0x3fbbb698u, 0xd6f0dc97u, 0x0c59f8d8u};
    for (int i = 0; i < 8; i++) large.l[i] = lr[i];
    Fr w = fp_pow_u64(large, 3);
    for (unsigned i = log_n; i < 47; i++) w = fp_sqr(w);
    return w;
}
static Fr host_generator() {
    // fr.rs:69-74 GENERATOR: the Montgomery limbs there encode 22 (22 * R mod r), so build it from 22
    Fr g = Fr::zero();
    g.l[0] = 22;
    return fp_from_repr(g);
}

int get_domain(czk_ctx* ctx, unsigned log_d, DomainTables** out) {
    if (log_d > 47) return set_err(ctx, CZK_ERR_SIZE, "domain larger than 2^TWO_ADICITY (radix2/mod.rs:61-63)");
    auto it = ctx->domains.find(log_d);
    if (it != ctx->domains.end()) {
        *out = &it->second;
        return CZK_OK;
    }
    DomainTables d;
    d.log_d = log_d;
    const u64 D = (u64)1 << log_d;
    d.group_gen = host_root_of_unity(log_d);
    d.group_gen_inv = fp_inv(d.group_gen);
    Fr dsz = Fr::zero();
    dsz.l[0] = (u32)D;
    dsz.l[1] = (u32)(D >> 32);
    d.size_inv = fp_inv(fp_from_repr(dsz));
    d.generator = host_generator();
    d.generator_inv = fp_inv(d.generator);
    d.vanishing_inv = fp_inv(fp_sub(fp_pow_u64(d.generator, D), Fr::one()));
    ctx->domains[log_d] = d;
    *out = &ctx->domains[log_d];
    return CZK_OK;
}

// device tables are built lazily (a 2^47 domain has valid constants but no tables)
int ensure_tables(czk_ctx* ctx, DomainTables* d, bool need_coset_fwd, bool need_coset_inv) {
    const unsigned n = d->log_d;
    const size_t D = (size_t)1 << n;
    if ((!d->tw_fwd || !d->tw_inv) && n > 0) {
        StageRoots hr[2];
        for (unsigned s = 0; s < n; s++) {
            Fr wf = d->group_gen, wi = d->group_gen_inv;
            for (unsigned k = 0; k < n - 1 - s; k++) {
                wf = fp_sqr(wf);
                wi = fp_sqr(wi);
            }
            hr[0].w[s] = wf;
            hr[1].w[s] = wi;
        }
        StageRoots* dr = nullptr;
        CZK_HIP(ctx, hipMalloc(&dr, sizeof(hr)));
        CZK_HIP(ctx, hipMemcpyAsync(dr, hr, sizeof(hr), hipMemcpyHostToDevice, ctx->stream));
        if (alloc_table_pair(ctx, &d->tw_fwd, &d->tw_inv, (D - 1 ? D - 1 : 1) * 32) != CZK_OK) {
            (void)hipFree(dr);
            return CZK_ERR_NOMEM;
        }
        size_t chunks = (D - 1 + 63) / 64;
        unsigned blocks = (unsigned)((chunks + 127) / 128);
        hipLaunchKernelGGL(k_twiddle_table, dim3(blocks), dim3(128), 0, ctx->stream, d->tw_fwd, n, dr);
        hipLaunchKernelGGL(k_twiddle_table, dim3(blocks), dim3(128), 0, ctx->stream, d->tw_inv, n, dr + 1);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(dr);
        if (e != hipSuccess) return drop_table_pair(ctx, &d->tw_fwd, &d->tw_inv, e);
    }
    size_t chunks = (D + 63) / 64;
    unsigned blocks = (unsigned)((chunks + 127) / 128);
    if (need_coset_fwd && !d->coset_fwd) {
        CZK_HIP(ctx, hipMalloc(&d->coset_fwd, D * 32));
        hipLaunchKernelGGL(k_pow_table, dim3(blocks), dim3(128), 0, ctx->stream, d->coset_fwd, D, d->generator, Fr::one());
        CZK_HIP(ctx, hipGetLastError());
    }
    if (need_coset_inv && !d->coset_inv) {
        CZK_HIP(ctx, hipMalloc(&d->coset_inv, D * 32));
        hipLaunchKernelGGL(k_pow_table, dim3(blocks), dim3(128), 0, ctx->stream, d->coset_inv, D, d->generator_inv, d->size_inv);
        CZK_HIP(ctx, hipGetLastError());
    }
    if (n >= NTT2_MIN_LOG) {   // second-generation passes: the same tables in the unsaturated residue system (fru.h)
        if (!d->twu_fwd || !d->twu_inv) {
            CZK_TRY(alloc_table_pair(ctx, &d->twu_fwd, &d->twu_inv, (D - 1) * 36));
            launch_table_to_u(ctx->stream, d->tw_fwd, D - 1, d->twu_fwd);
            launch_table_to_u(ctx->stream, d->tw_inv, D - 1, d->twu_inv);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return drop_table_pair(ctx, &d->twu_fwd, &d->twu_inv, e);
        }
        if (need_coset_fwd && !d->cosetu_fwd) {
            CZK_HIP(ctx, hipMalloc(&d->cosetu_fwd, D * 36));
            launch_table_to_u(ctx->stream, d->coset_fwd, D, d->cosetu_fwd);
            CZK_HIP(ctx, hipGetLastError());
        }
        if (need_coset_inv && !d->cosetu_inv) {
            CZK_HIP(ctx, hipMalloc(&d->cosetu_inv, D * 36));
            launch_table_to_u(ctx->stream, d->coset_inv, D, d->cosetu_inv);
            CZK_HIP(ctx, hipGetLastError());
        }
    }
    return CZK_OK;
}

// ------------------------------------------------------------------------------------------------
// driver
// ------------------------------------------------------------------------------------------------
int ntt_device(czk_ctx* ctx, u64* data, unsigned log_d, size_t lanes, int kind, size_t in_len, const u64* src, size_t src_stride, const u64* addend,
               const Fr* scale) {
    if (kind < 0 || kind > 3) return set_err(ctx, CZK_ERR_ARG, "bad ntt kind");
    if (addend && (kind == CZK_IFFT || (kind == CZK_COSET_IFFT && !scale))) return set_err(ctx, CZK_ERR_ARG, "ntt addend: unsupported kind");
    if (!src) {   // in place
        src = data;
        src_stride = (size_t)1 << log_d;
    }
    DomainTables* d = nullptr;
    CZK_TRY(get_domain(ctx, log_d, &d));
    const size_t D = (size_t)1 << log_d;
    if (in_len > D) return set_err(ctx, CZK_ERR_SIZE, "coeffs.len() > domain size (radix2/mod.rs:100)");
    if (lanes == 0) return CZK_OK;
    if (log_d > 30) return set_err(ctx, CZK_ERR_SIZE, "domain above 2^30 exceeds this build's table budget");
    const bool inverse = (kind == CZK_IFFT || kind == CZK_COSET_IFFT);
    CZK_TRY(ensure_tables(ctx, d, kind == CZK_COSET_FFT, kind == CZK_COSET_IFFT));

    const unsigned n = log_d;
    const PassPlan plan = pass_plan(n);
    u64* scratch = nullptr;
    if (plan.multi()) {
        CZK_TRY(ensure_buf(ctx, ctx->ntt_scratch, ntt_scratch_bytes(n, lanes, 1)));
        scratch = (u64*)ctx->ntt_scratch.p;
    }
    if (n >= NTT2_MIN_LOG && !ctx->ntt_gen1) {
        // second-generation passes (ntt_pass.hip): register-resident radix-8 / radix-4 groups, unsaturated arithmetic
        Pass2Args b = pass2_common(d, inverse, in_len, src_stride);
        for (unsigned p = 0; p < plan.m; p++) {
            const bool first = plan.first(p), last = plan.last(p);
            b.s_lo = plan.s_lo[p];
            b.first = first ? 1 : 0;
            b.prescale = (first && kind == CZK_COSET_FFT) ? d->cosetu_fwd : nullptr;
            b.posttab = (last && kind == CZK_COSET_IFFT) ? d->cosetu_inv : nullptr;
            b.post_mode = !last ? 0 : (kind == CZK_IFFT ? 1 : (kind == CZK_COSET_IFFT ? (addend ? 3 : 2) : (addend ? 4 : 0)));
            b.addend = addend;
            if (addend && scale) b.postconst2 = host_fr_to_u(*scale);
            b.in = first ? src : scratch;
            b.out = last ? data : scratch;
#ifdef CZK_LAB
            // TIMING EXPERIMENT ONLY (wrong results): the first pass of every coset FFT is not launched -- an upper bound on what fusing it into the last pass
            // of the inverse transform in front of it (witness_map: ifft -> coset_fft on a, b, c) could save: the fused kernel would still run its seven stages
            if (ctx->ntt_skip_coset_first && first && !last && kind == CZK_COSET_FFT) continue;
#endif
            ProfScope ps(ctx, "ntt_pass");
            CZK_TRY(launch_ntt2_pass(ctx, b, plan.K[p], last, lanes));
        }
        return CZK_OK;
    }
    PassArgs a;
    a.tw = inverse ? d->tw_inv : d->tw_fwd;
    a.n = n;
    a.in_len = in_len;
    a.lane_stride = D;
    a.in_lane_stride = src_stride;
    a.postconst = d->size_inv;
    for (unsigned p = 0; p < plan.m; p++) {
        const bool first = plan.first(p), last = plan.last(p);
        a.K = plan.K[p];
        a.s_lo = plan.s_lo[p];
        a.first = first ? 1 : 0;
        a.prescale = (first && kind == CZK_COSET_FFT) ? d->coset_fwd : nullptr;
        a.posttab = nullptr;
        a.post_mode = 0;
        a.in = first ? src : scratch;
        a.out = last ? data : scratch;
        ProfScope ps(ctx, "ntt_pass");
        if (!last) {
            a.logT = a.s_lo < 4 ? a.s_lo : 4;
            unsigned blocks = (unsigned)(D >> (a.K + a.logT));
            size_t lds = ((size_t)1 << (a.K + a.logT)) * 32;
            hipLaunchKernelGGL(k_ntt_strided, dim3(blocks, (unsigned)lanes), dim3(256), lds, ctx->stream, a);
        } else {
            unsigned hb = n - a.K;
            a.logT = hb < 4 ? hb : 4;
            if (kind == CZK_IFFT) a.post_mode = 1;
            if (kind == CZK_COSET_IFFT) {
                a.post_mode = 2;
                a.posttab = d->coset_inv;
            }
            unsigned blocks = (unsigned)(D >> (a.K + a.logT));
            size_t lds = ((((size_t)1 << a.K) + 1) << a.logT) * 32 + ((size_t)1 << a.K) * 32;
            if (lds > ctx->lds_per_block) return set_err(ctx, CZK_ERR_HIP, "NTT last pass needs more LDS per workgroup than this device offers");
            hipLaunchKernelGGL(k_ntt_final, dim3(blocks, (unsigned)lanes), dim3(256), lds, ctx->stream, a);
        }
        CZK_HIP(ctx, hipGetLastError());
    }
    if (addend) {   // first-generation passes: the addend as one pointwise kernel behind the transform (fr_vec.hip)
        const size_t cnt = lanes * D;
        if (kind == CZK_COSET_IFFT) fr_sub_scale_launch(ctx, data, addend, *scale, data, cnt);
        else fr_vec_op_launch(ctx, CZK_OP_ADD, data, addend, data, cnt);
        CZK_HIP(ctx, hipGetLastError());
    }
    return CZK_OK;
}

}  // namespace czk

using namespace czk;

// ------------------------------------------------------------------------------------------------
// C ABI (NTT part)
// ------------------------------------------------------------------------------------------------
// Host-memory callers with several large lanes (the reference's Vec<MpcField> repacked into share lanes): lane k + 1 goes up
// while lane k comes down -- PCIe is full duplex, but a copy from / to pageable memory blocks its calling thread, so the
// downloads run on a second host thread and a second stream.  The transform of a lane is a fraction of its transfer time.
static int ntt_host_lanes_pipelined(czk_ctx* ctx, uint64_t* data, unsigned log_d, size_t lanes, int kind, size_t in_len) {
    const size_t lane_words = (size_t)4 << log_d, lane_bytes = lane_words * 8;
    DeviceBuf buf;
    CZK_TRY(stage_take(ctx, lanes * lane_bytes, &buf));
    std::vector<hipEvent_t> done(lanes, nullptr);
    hipStream_t down = nullptr;
    hipError_t setup = hipStreamCreateWithFlags(&down, hipStreamNonBlocking);
    for (auto& e : done)
        if (setup == hipSuccess) setup = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    // producer -> downloader hand-over: lanes whose transform has been enqueued / a failure flag, under one mutex
    std::mutex mu;
    std::condition_variable cv;
    size_t ready = 0;
    int failed = 0;
    int rc = CZK_OK;
    if (setup != hipSuccess) {
        rc = set_err(ctx, CZK_ERR_HIP, std::string("NTT lane pipeline set-up: ") + hipGetErrorString(setup));
    } else {
        const int device = ctx->device;
        std::thread downloader([&] {
            (void)hipSetDevice(device);
            for (size_t k = 0; k < lanes; k++) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return ready > k || failed; });   // sleeps; no host core is spun while the GPU works
                    if (failed) return;
                }
                if (hipStreamWaitEvent(down, done[k], 0) != hipSuccess ||
                    hipMemcpyAsync(data + k * lane_words, (char*)buf.p + k * lane_bytes, lane_bytes, hipMemcpyDeviceToHost, down) != hipSuccess ||
                    hipStreamSynchronize(down) != hipSuccess) {
                    std::lock_guard<std::mutex> lk(mu);
                    failed = 2;
                    return;
                }
            }
        });
        for (size_t k = 0; k < lanes && rc == CZK_OK; k++) {
            u64* lane = (u64*)((char*)buf.p + k * lane_bytes);
            // only the first in_len elements are read by the transform (the tail is taken as zero)
            const size_t up = (in_len < ((size_t)1 << log_d) ? in_len : ((size_t)1 << log_d)) * 32;
            if (up && hipMemcpyAsync(lane, data + k * lane_words, up, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                rc = set_err(ctx, CZK_ERR_HIP, "H2D lane");
            if (rc == CZK_OK) rc = ntt_device(ctx, lane, log_d, 1, kind, in_len);
            if (rc == CZK_OK && hipEventRecord(done[k], ctx->stream) != hipSuccess) rc = set_err(ctx, CZK_ERR_HIP, "event record");
            if (rc == CZK_OK) {
                {
                    std::lock_guard<std::mutex> lk(mu);
                    ready = k + 1;
                }
                cv.notify_one();
            }
        }
        if (rc != CZK_OK) {
            {
                std::lock_guard<std::mutex> lk(mu);
                if (!failed) failed = 1;
            }
            cv.notify_one();
        }
        downloader.join();
        if (rc == CZK_OK && failed == 2) rc = set_err(ctx, CZK_ERR_HIP, "D2H lane");
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& e : done)
        if (e) (void)hipEventDestroy(e);
    if (down) (void)hipStreamDestroy(down);
    stage_give(ctx, buf);
    return rc;
}

extern "C" int czk_ntt_fr_to(czk_ctx* ctx, const uint64_t* src, size_t src_stride, uint64_t* dst, unsigned log_d, size_t lanes, int kind, size_t in_len,
                             int mem) {
    if (!ctx) return CZK_ERR_ARG;
    if (!dst || (in_len && !src)) return set_err(ctx, CZK_ERR_ARG, "null ntt argument");
    if (mem != CZK_MEM_DEVICE) return set_err(ctx, CZK_ERR_ARG, "czk_ntt_fr_to takes device memory (host callers copy and use czk_ntt_fr)");
    if (log_d > 47) return set_err(ctx, CZK_ERR_SIZE, "domain too large: log2 D exceeds TWO_ADICITY = 47 (radix2/mod.rs:61-63)");
    if (in_len > src_stride && lanes > 1) return set_err(ctx, CZK_ERR_ARG, "in_len exceeds the source lane stride");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    return ntt_device(ctx, (u64*)dst, log_d, lanes, kind, in_len, in_len ? (const u64*)src : (const u64*)dst, in_len ? src_stride : ((size_t)1 << log_d));
}

extern "C" int czk_ntt_fr(czk_ctx* ctx, uint64_t* data, unsigned log_d, size_t lanes, int kind, size_t in_len, int mem) {
    if (!ctx) return CZK_ERR_ARG;
    if (!data && lanes) return set_err(ctx, CZK_ERR_ARG, "null data");
    if (log_d > 47) return set_err(ctx, CZK_ERR_SIZE, "domain larger than 2^TWO_ADICITY (radix2/mod.rs:61-63)");
    if (!valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE");
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    size_t bytes = lanes * ((size_t)32 << log_d);
    if (mem == CZK_MEM_HOST && lanes > 1 && log_d >= 16) return ntt_host_lanes_pipelined(ctx, data, log_d, lanes, kind, in_len);
    Staged s{ctx};
    CZK_TRY(s.to_device(data, bytes, mem));
    CZK_TRY(ntt_device(ctx, (u64*)s.dev, log_d, lanes, kind, in_len));
    return s.to_host(data, bytes);
}

extern "C" int czk_domain_constants(czk_ctx* ctx, unsigned log_d, uint64_t* out24) {
    if (!ctx || !out24) return CZK_ERR_ARG;
    DomainTables* d = nullptr;
    CZK_TRY(get_domain(ctx, log_d, &d));
    const Fr* v[6] = {&d->size_inv, &d->group_gen, &d->group_gen_inv, &d->generator, &d->generator_inv, &d->vanishing_inv};
    for (int k = 0; k < 6; k++)
        for (int i = 0; i < 4; i++) out24[4 * k + i] = (u64)v[k]->l[2 * i] | ((u64)v[k]->l[2 * i + 1] << 32);
    return CZK_OK;
}

// czk_ctx_reserve: the tables of one radix-2 domain (all four kinds) and the pass scratch for `lanes` lanes, built now instead of by the first transform
int czk::ntt_reserve(czk_ctx* ctx, unsigned log_d, size_t lanes) {
    DomainTables* d = nullptr;
    CZK_TRY(get_domain(ctx, log_d, &d));
    CZK_TRY(ensure_tables(ctx, d, true, true));
    // scratch where there is more than one pass (ceil(log_d / 7) > 1: for every log_d the same as log_d > 7).  Two sets with "ntt_fuse_pairs": the fused pass of an
    // ifft -> coset_fft pair writes a second set of scratch lanes; set later, the witness map (witness_map.hip) grows the buffer
    if (pass_plan(log_d).multi() && lanes) CZK_TRY(ensure_buf(ctx, ctx->ntt_scratch, ntt_scratch_bytes(log_d, lanes, ctx->ntt_fuse_pairs ? 2 : 1)));
    CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CZK_OK;
}
