// witness_map.hip -- the Groth16 witness map (R1CStoQAP::witness_map, mpc-snarks/src/groth/r1cs_to_qap.rs:58-115) on device lanes:
// czk_witness_map_pre / _pre_masked / _post / _post_h.  Host code only: a client of the radix-2 transform (ntt.hip ntt_device, the pass
// launchers of ntt_pass.hip) and of the pointwise launchers of fr_vec.hip.
#include "ntt_pass.h"

using namespace czk;

// data <- coset_fft(ifft(data)) per lane: the pair R1CStoQAP::witness_map applies to a, b and c (mpc-snarks/src/groth/r1cs_to_qap.rs:85-89, 102-103).  Where the
// two transforms' pass structures line up (the stage bits split into equal groups: 2^21 = 7 + 7 + 7, also 2^12, 2^14, 2^15, 2^18) the last pass of the
// inverse and the first pass of the forward transform run as ONE kernel (ntt_pass.hip k_ntt2_final_first): five trips through HBM instead of six, same values.
static int ifft_coset_fft_device(czk_ctx* ctx, u64* data, unsigned log_d, size_t lanes, size_t in_len, const u64* addend = nullptr) {
    const unsigned n = log_d;
    // equal groups: the two passes own the same tiles.  (A log_d without a domain, above TWO_ADICITY = 47, has no plan: ntt_device rejects it.)
    const bool fuse = ctx->ntt_fuse_pairs && !ctx->ntt_gen1 && n >= NTT2_MIN_LOG && n <= 47 && pass_plan(n).equal_groups();
    if (!fuse) {
        CZK_TRY(ntt_device(ctx, data, log_d, lanes, CZK_IFFT, in_len));
        return ntt_device(ctx, data, log_d, lanes, CZK_COSET_FFT, (size_t)1 << log_d, nullptr, 0, addend);
    }
    DomainTables* d = nullptr;
    CZK_TRY(get_domain(ctx, log_d, &d));
    const size_t D = (size_t)1 << log_d;
    if (in_len > D) return set_err(ctx, CZK_ERR_SIZE, "coeffs.len() > domain size (radix2/mod.rs:100)");
    if (lanes == 0) return CZK_OK;
    CZK_TRY(ensure_tables(ctx, d, true, false));
    const PassPlan plan = pass_plan(n);
    const unsigned K = plan.K[0];
    // two sets of scratch lanes: the fused pass reads one and writes the other (a block's inputs and outputs are different element sets)
    CZK_TRY(ensure_buf(ctx, ctx->ntt_scratch, ntt_scratch_bytes(n, lanes, 2)));
    u64* sa = (u64*)ctx->ntt_scratch.p;
    u64* sb = (u64*)((char*)ctx->ntt_scratch.p + ntt_scratch_bytes(n, lanes, 1));
    Pass2Args inv = pass2_common(d, true, in_len, D), fwd = pass2_common(d, false, D, D);
    // the inverse transform's passes but the last: data -> scratch A
    for (unsigned p = 0; !plan.last(p); p++) {
        inv.s_lo = plan.s_lo[p];
        inv.first = plan.first(p) ? 1 : 0;
        inv.post_mode = 0;
        inv.in = plan.first(p) ? data : sa;
        inv.out = sa;
        ProfScope ps(ctx, "ntt_pass");
        CZK_TRY(launch_ntt2_pass(ctx, inv, K, false, lanes));
    }
    {   // its last pass (bits [0, K), 1 / D) with the forward transform's first (g^i, bits [n - K, n)): scratch A -> scratch B
        inv.s_lo = plan.s_lo[plan.m - 1], inv.first = 0, inv.post_mode = 1, inv.in = sa, inv.out = nullptr;
        fwd.s_lo = plan.s_lo[0], fwd.first = 0, fwd.prescale = d->cosetu_fwd, fwd.in = nullptr, fwd.out = sb;
        ProfScope ps(ctx, "ntt_pass");
        CZK_TRY(launch_ntt2_final_first(ctx, inv, fwd, K, lanes));
    }
    for (unsigned p = 1; p < plan.m; p++) {   // the forward transform's passes after the first: scratch B -> data
        const bool last = plan.last(p);
        fwd.s_lo = plan.s_lo[p];
        fwd.first = 0, fwd.prescale = nullptr;
        fwd.in = sb;
        fwd.out = last ? data : sb;
        if (last && addend) fwd.post_mode = 4, fwd.addend = addend;
        ProfScope ps(ctx, "ntt_pass");
        CZK_TRY(launch_ntt2_pass(ctx, fwd, K, last, lanes));
    }
    return CZK_OK;
}

extern "C" int czk_witness_map_pre(czk_ctx* ctx, uint64_t* a, size_t a_len, uint64_t* b, size_t b_len, unsigned log_d, size_t lanes) {
    if (!ctx || !a || !b) return ctx ? set_err(ctx, CZK_ERR_ARG, "null witness_map argument") : CZK_ERR_ARG;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t D = (size_t)1 << log_d;
    if (a_len > D || b_len > D) return set_err(ctx, CZK_ERR_SIZE, "witness_map: more evaluations than the domain holds");
    // elements [len, D) are the `vec![zero; domain_size]` padding (r1cs_to_qap.rs:66-67): the first pass zero-extends
    CZK_TRY(ifft_coset_fft_device(ctx, a, log_d, lanes, a_len));
    CZK_TRY(ifft_coset_fft_device(ctx, b, log_d, lanes, b_len));
    return CZK_OK;
}

extern "C" int czk_witness_map_pre_masked(czk_ctx* ctx, uint64_t* a, size_t a_len, uint64_t* b, size_t b_len, const uint64_t* mask_a, const uint64_t* mask_b,
                                          unsigned log_d, size_t lanes) {
    if (!ctx || !a || !b || !mask_a || !mask_b) return ctx ? set_err(ctx, CZK_ERR_ARG, "null witness_map argument") : CZK_ERR_ARG;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    if (log_d > 47) return set_err(ctx, CZK_ERR_SIZE, "domain larger than 2^TWO_ADICITY (radix2/mod.rs:61-63)");
    const size_t D = (size_t)1 << log_d;
    if (a_len > D || b_len > D) return set_err(ctx, CZK_ERR_SIZE, "witness_map: more evaluations than the domain holds");
    if (!(ctx->witness_map_short & 2)) {   // the sequence of before: the transforms, then one pointwise addition per vector
        CZK_TRY(czk_witness_map_pre(ctx, a, a_len, b, b_len, log_d, lanes));
        const size_t n = lanes * D;
        if (!n) return CZK_OK;
        fr_vec_op_launch(ctx, CZK_OP_ADD, a, mask_a, a, n);
        fr_vec_op_launch(ctx, CZK_OP_ADD, b, mask_b, b, n);
        CZK_HIP(ctx, hipGetLastError());
        return CZK_OK;
    }
    CZK_TRY(ifft_coset_fft_device(ctx, a, log_d, lanes, a_len, (const u64*)mask_a));
    CZK_TRY(ifft_coset_fft_device(ctx, b, log_d, lanes, b_len, (const u64*)mask_b));
    return CZK_OK;
}

static int witness_map_post_common(czk_ctx* ctx, uint64_t* ab, uint64_t* c, size_t c_len, unsigned log_d, size_t lanes, bool c_is_scratch) {
    if (!ctx || !ab || !c) return ctx ? set_err(ctx, CZK_ERR_ARG, "null witness_map argument") : CZK_ERR_ARG;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t D = (size_t)1 << log_d;
    if (c_len > D) return set_err(ctx, CZK_ERR_SIZE, "witness_map: more evaluations than the domain holds");
    DomainTables* d = nullptr;
    CZK_TRY(get_domain(ctx, log_d, &d));
    if (c_is_scratch && (ctx->witness_map_short & 1)) {
        // transforms are linear and coset_ifft(coset_fft(x)) = x, so coset_ifft((ab - coset_fft(ifft(c))) k) = k (coset_ifft(ab) - ifft(c)) in the field, and both sides
        // are stored canonical: c is transformed once, and the subtraction and k ride on the last store of the coset inverse transform
        CZK_TRY(ntt_device(ctx, (u64*)c, log_d, lanes, CZK_IFFT, c_len));
        return ntt_device(ctx, (u64*)ab, log_d, lanes, CZK_COSET_IFFT, D, nullptr, 0, (const u64*)c, &d->vanishing_inv);
    }
    CZK_TRY(ifft_coset_fft_device(ctx, c, log_d, lanes, c_len));
    size_t n = lanes * D;
    fr_sub_scale_launch(ctx, ab, c, d->vanishing_inv, ab, n);
    CZK_HIP(ctx, hipGetLastError());
    CZK_TRY(ntt_device(ctx, ab, log_d, lanes, CZK_COSET_IFFT, D));
    return CZK_OK;
}

extern "C" int czk_witness_map_post(czk_ctx* ctx, uint64_t* ab, uint64_t* c, size_t c_len, unsigned log_d, size_t lanes) {
    return witness_map_post_common(ctx, ab, c, c_len, log_d, lanes, false);
}

// czk_witness_map_post for a caller that needs h alone: `c` is scratch, which lets the call transform it once instead of twice
extern "C" int czk_witness_map_post_h(czk_ctx* ctx, uint64_t* ab, uint64_t* c, size_t c_len, unsigned log_d, size_t lanes) {
    return witness_map_post_common(ctx, ab, c, c_len, log_d, lanes, true);
}
