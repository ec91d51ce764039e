// ntt_pass_probe.h -- LAB BUILD ONLY: one pass of the second-generation NTT (ntt_pass.hip) on a buffer the caller wrote (ntt_pass_probe.hip).
//
// Not part of the product ABI (include/czk.h): exported by libczk_hip_lab.so alone, for tests/test_ntt_pass.py, which holds every element a pass
// writes -- and every element it must not write -- to the integer model of tests/ntt_pass_model.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct czk_ctx czk_ctx;

enum czk_lab_ntt_pass_mode {
    CZK_NTT_PROBE_PASS = 0,    // one launch_ntt2_pass
    CZK_NTT_PROBE_FUSED = 1,   // one launch_ntt2_final_first: the last pass of an ifft and the first pass of a coset fft over the same tiles
};

// What the pass is.  Single pass: log_d 11 .. 14; K in {5, 6, 7}; a strided pass (last == 0) owns the stage bits [s_lo, s_lo + K) with 4 <= s_lo and
// s_lo + K <= log_d -- ANY such triple, not only those of pass_plan(log_d); a last pass has s_lo == 0 and is never `first`.  Fused pass: K = C in {5, 6, 7},
// 4 + C <= log_d <= 14; the other fields but `lanes` must be zero (the inverse half has s_lo = 0 and 1 / D, the forward half s_lo = log_d - C and g^i).
typedef struct czk_lab_ntt_pass_desc {
    uint32_t mode;             // enum czk_lab_ntt_pass_mode
    uint32_t log_d;
    uint32_t inverse;          // the domain's inverse twiddles instead of the forward ones
    uint32_t K;
    uint32_t s_lo;
    uint32_t first;            // input: canonical 8 x u32 elements, `in_len` of them per lane at stride `in_lane_stride`; the rest reads as zero
    uint32_t last;             // output: canonical elements, bit-reversed store, post_mode applied
    uint32_t prescale;         // first passes: times g^i on load (the domain's cosetu_fwd)
    uint32_t posttab;          // last passes, post_mode 2 and 3: the domain's cosetu_inv (g^-k / D)
    uint32_t post_mode;        // Pass2Args::post_mode, 0 .. 4; non-zero only with `last`
    uint64_t lanes;            // 1 .. 8
    uint64_t in_len;           // first passes: <= min(2^log_d, in_lane_stride); otherwise 0
    uint64_t in_lane_stride;   // first passes: elements between the lanes of `in`, <= 2^(log_d + 1); otherwise 0
} czk_lab_ntt_pass_desc;

enum {
    CZK_NTT_PROBE_DIM_FORMAT = 0,        // NTT2_SCRATCH_FORMAT
    CZK_NTT_PROBE_DIM_ELEM_BYTES = 1,    // NTT2_SCRATCH_ELEM_BYTES
    CZK_NTT_PROBE_DIM_MIN_LOG = 2,       // NTT2_MIN_LOG
    CZK_NTT_PROBE_DIM_T = 3,             // NTT2_T
    CZK_NTT_PROBE_DIM_GUARD = 4,         // elements of guard tail behind the last lane of `out`
    CZK_NTT_PROBE_DIM_M = 5,             // pass_plan(log_d): m, equal_groups(), K[0 .. 7), s_lo[0 .. 7)
    CZK_NTT_PROBE_DIM_EQUAL_GROUPS = 6,
    CZK_NTT_PROBE_DIM_K = 7,
    CZK_NTT_PROBE_DIM_S_LO = 14,
    CZK_NTT_PROBE_DIM_COUNT = 21
};
#define CZK_NTT_PROBE_GUARD 64
#define CZK_NTT_PROBE_SENTINEL 0xA5   // every byte of `out` before the launch (as a scratch element: a value above 2 r)

// All arrays are host memory; the probe stages them through device buffers of its own and launches on the context's stream.
//   dims      CZK_NTT_PROBE_DIM_COUNT u64.  With in == out == null (and both sizes 0) only `dims` is written, for any desc->log_d <= 47.
//   in        first pass: lanes x in_lane_stride canonical elements (32 bytes each); otherwise lanes x 2^log_d scratch elements.
//   addend    post_mode 3 and 4: lanes x 2^log_d canonical elements, null otherwise.
//   postconst2  post_mode 3: one canonical Montgomery element (4 u64), null otherwise.
//   out       lanes x 2^log_d + CZK_NTT_PROBE_GUARD elements: canonical (32 bytes) for a last pass, scratch elements otherwise.  Pre-filled with the
//             sentinel, so elements the pass did not write come back as the sentinel.
// in_bytes / out_bytes must be exactly those sizes.  Anything else: CZK_ERR_ARG, before any launch.
int czk_lab_ntt_pass(czk_ctx* ctx, const czk_lab_ntt_pass_desc* desc, const void* in, size_t in_bytes, const uint64_t* addend, const uint64_t* postconst2,
                     uint64_t* dims, void* out, size_t out_bytes);

#ifdef __cplusplus
}
#endif
