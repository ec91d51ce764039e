// ntt_pass.h -- the radix-2 NTT's internal interface: the pass plan and the domain tables (ntt.hip), the second-generation pass kernels
// (ntt_pass.hip), and what the Groth16 witness map (witness_map.hip) needs of both for its fused ifft -> coset_fft pair
#pragma once
#include "czk_internal.h"
#include "fru.h"

namespace czk {

constexpr unsigned NTT2_MIN_LOG = 11;   // domains from 2^11 on run the second-generation passes (pass sizes 5..7)

// The passes of a 2^n transform: the n stage bits split into ceil(n/7) near-equal groups, highest bits first.  Pass p runs the K[p] stage
// bits [s_lo[p], s_lo[p] + K[p]); the last pass owns bits [0, K[m - 1]).  n <= 47 (TWO_ADICITY): at most seven passes.
struct PassPlan {
    unsigned n, m, K[7], s_lo[7];
    bool first(unsigned p) const { return p == 0; }
    bool last(unsigned p) const { return p + 1 == m; }
    bool multi() const { return m > 1; }                       // more than one pass: scratch lanes between them
    bool equal_groups() const { return m >= 2 && n % m == 0; }   // every pass owns tiles of one shape: an inverse transform's last pass and a forward one's first can share a kernel
};
inline PassPlan pass_plan(unsigned n) {
    PassPlan pl{};
    pl.n = n;
    pl.m = n == 0 ? 1 : (n + 6) / 7;
    unsigned s = n;
    for (unsigned p = 0; p < pl.m; p++) {
        pl.K[p] = n / pl.m + (p < n % pl.m ? 1 : 0);
        pl.s_lo[p] = s -= pl.K[p];
    }
    return pl;
}

// Format of the scratch lanes between passes:
//   0  canonical elements (8 x u32, < r);
//   1  LAZY elements of nine 29-bit limbs = 36 bytes, value < 2 r: saves the pack / conditional subtraction / unpack round trip but
//      reads and writes 36-byte elements with 4-byte accesses -- measured SLOWER on MI355X (2^21 x 4 lanes: 0.914 ms against 0.881 ms);
//   2  (default) values < 2 r PACKED into the same 8 x u32 as format 0 (2 r < 2^254): 16-byte accesses like format 0, but the
//      conditional subtraction that makes the value canonical is only done by the last pass.
// In formats 1 and 2 a pass after the first starts from the bound 2 instead of 1.003 and uses the next larger constants (see the
// bound analysis in ntt_pass.hip).  All three are kept compilable; tests run against whichever is selected.
constexpr int NTT2_SCRATCH_FORMAT = 2;
constexpr bool NTT2_LAZY_SCRATCH = NTT2_SCRATCH_FORMAT == 1;
constexpr bool NTT2_SCRATCH_2R = NTT2_SCRATCH_FORMAT != 0;
constexpr size_t NTT2_SCRATCH_ELEM_BYTES = NTT2_LAZY_SCRATCH ? 36 : 32;

struct Pass2Args {
    const u64* in;        // first pass: the caller's lanes (canonical 8 x u32 per element); later passes: the scratch lanes
    u64* out;             //   (see NTT2_LAZY_SCRATCH); the last pass writes canonical elements to the caller's lanes
    const u32* tw;        // per-stage compacted twiddles, unsaturated form: entry (2^s - 1 + j) = 9 limbs of w_s^j 2^261 mod r
    const u32* prescale;  // g^i 2^261 (first pass of a coset fft) or null
    const u32* posttab;   // size_inv g^-i 2^261 (last pass of a coset ifft) or null
    FrU postconst;        // size_inv 2^261 (last pass of an ifft)
    int post_mode;        // 0 none, 1 constant, 2 table, 3 table then (v - addend[k]) * postconst2, 4 canonical v + addend[k]
    const u64* addend;    // post_mode 3 / 4: canonical lanes read at the OUTPUT index (lane stride = lane_stride), never the lanes being written
    FrU postconst2;       // post_mode 3: the constant that follows the subtraction, 2^261 form
    unsigned n;           // log2 D
    unsigned s_lo;        // lowest stage bit of this pass
    size_t in_len;        // elements >= in_len read as zero (only honoured when `first`)
    int first;
    size_t lane_stride;   // elements between lanes (= D)
    size_t in_lane_stride;   // ... of `in` in the first pass (out-of-place transforms read the caller's source lanes)
};

// implemented in ntt_pass.hip
int launch_ntt2_pass(czk_ctx* ctx, const Pass2Args& a, unsigned K, bool last, size_t lanes);
int launch_ntt2_final_first(czk_ctx* ctx, const Pass2Args& ai, const Pass2Args& af, unsigned C, size_t lanes);
void launch_table_to_u(hipStream_t st, const u64* sat, size_t count, u32* dst);
FrU host_fr_to_u(const Fr& sat);
// implemented in ntt.hip: the device tables of a domain, built on first use (the coset tables only when asked for)
int ensure_tables(czk_ctx* ctx, DomainTables* d, bool need_coset_fwd, bool need_coset_inv);

// ctx->ntt_scratch for `lanes` lanes of a 2^n domain with more than one pass, in bytes.  sets: 1, or 2 for the fused ifft -> coset_fft pair, whose
// shared pass reads one set of scratch lanes and writes the other.
inline size_t ntt_scratch_bytes(unsigned n, size_t lanes, unsigned sets) {
    return sets * lanes * ((size_t)1 << n) * (n >= NTT2_MIN_LOG ? NTT2_SCRATCH_ELEM_BYTES : 32);
}

// The fields of a second-generation pass's arguments that do not change from pass to pass (everything else zero): the transform of domain d,
// forward or inverse, that reads in_len elements per lane at lane stride in_lane_stride in its first pass.
inline Pass2Args pass2_common(const DomainTables* d, bool inverse, size_t in_len, size_t in_lane_stride) {
    Pass2Args a{};
    a.tw = inverse ? d->twu_inv : d->twu_fwd;
    a.n = d->log_d;
    a.in_len = in_len;
    a.lane_stride = (size_t)1 << d->log_d;
    a.in_lane_stride = in_lane_stride;
    a.postconst = host_fr_to_u(d->size_inv);
    return a;
}

}  // namespace czk
