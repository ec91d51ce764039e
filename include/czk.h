/* czk.h -- C ABI of libczk_hip.so: the MI355X (gfx950) implementation of the per-party local compute
 * of collaborative-zksnark's MPC provers (radix-2 NTT over BLS12-377 Fr on share lanes; variable-base MSM
 * over BLS12-377 G1/G2).  Plain pointers and sizes only -- no torch / HIP types in any signature.
 *
 * The reference (alex-ozdemir/collaborative-zksnark) has no FFI; its seams are Rust trait impls.  Each
 * entry point below names the reference interface it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the Rust `extern "C"` shim a maintainer would add at each seam.
 *
 * Data formats (identical to the reference's in-memory values):
 *   Fr  : 4 x u64 little-endian limbs, Montgomery form R = 2^256   (algebra/ff/src/fields/macros.rs:103-108,
 *         curves/bls12_377/src/fields/fr.rs:48-53); "canonical" = `into_repr()` BigInteger256.
 *   Fq  : 6 x u64, Montgomery form R = 2^384                         (curves/bls12_377/src/fields/fq.rs:43-50)
 *   Fq2 : c0, c1 (12 x u64)                                           (fields/models/quadratic_extension.rs:136-142)
 *   G1 affine  : x, y          = 12 u64  + a separate u8 infinity flag per point
 *   G1 Jacobian: x, y, z       = 18 u64  (infinity <=> z == 0)        (short_weierstrass_jacobian.rs:338-344)
 *   G2 affine  : x.c0 x.c1 y.c0 y.c1 = 24 u64 + u8 flag;  G2 Jacobian = 36 u64
 * Rust's struct layout is unspecified (no #[repr(C)]), so the shim repacks into these arrays.
 *
 * Memory: every buffer argument is either host memory (CZK_MEM_HOST: the library stages it through
 * HBM) or device memory on the context's GPU (CZK_MEM_DEVICE: used in place, no copies).
 * Threading: one czk_ctx = one GPU + one HIP stream = one MPC party; calls on a ctx are serialized by
 * the caller (the reference prover is single-threaded; mpc-net/src/multi.rs:15-23).
 * Errors: every call returns a czk_status; the reference's `None`/`assert!`/`unwrap()` sites map to
 * CZK_ERR_SIZE / CZK_ERR_ARG and the shim `expect()`s them, preserving panic behaviour.
 */
#ifndef CZK_H
#define CZK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct czk_ctx czk_ctx;
typedef struct czk_bases czk_bases;

typedef enum {
    CZK_OK = 0,
    CZK_ERR_SIZE = 1,  /* domain too large (log2 D > TWO_ADICITY = 47: radix2/mod.rs:61-63) or len > D (:100) */
    CZK_ERR_HIP = 2,   /* HIP runtime failure (message via czk_last_error) */
    CZK_ERR_ARG = 3,   /* null / inconsistent argument */
    CZK_ERR_NOMEM = 4,
    CZK_ERR_NET = 5,   /* czk_net_*: transport failure or a peer that did not arrive within the communicator's timeout (message via czk_net_last_error) */
    CZK_ERR_CHECK = 6  /* czk_net_atomic_broadcast: a party's data does not match its commitment (the reference's assert_eq!, channel.rs:63-66) */
} czk_status;

typedef enum {
    CZK_MEM_HOST = 0,
    CZK_MEM_DEVICE = 1,
    /* czk_msm_async only, OR-ed with CZK_MEM_DEVICE: the caller will not modify the scalar buffer before the next
     * czk_ctx_sync(), so the context's stream need not wait for the MSM's digit extraction (lets independent work
     * enqueued afterwards on that stream -- e.g. the witness-map NTTs -- overlap with the MSM). */
    CZK_MEM_STABLE = 16,
    /* czk_bases_register only, OR-ed with CZK_MEM_HOST / CZK_MEM_DEVICE: keep the points only, no precomputed window
     * multiples.  Registration is then a copy (instead of ~240 point doublings per point: 65 ms per 2^20 G1 points), and
     * each MSM runs one bucket set per window plus the Horner combination of variable_base.rs:92-105 -- about 1.4x the
     * arithmetic of the table form.  For callers that use a set of bases once or a few times; czk_msm_g1 / czk_msm_g2 use it. */
    CZK_MEM_NO_TABLES = 32,
    /* czk_bases_register only, OR-ed in: the bases are arbitrary points of the curve, not necessarily elements of the prime-order
     * subgroup.  G1 handles then keep short-Weierstrass (XYZZ) bucket arithmetic with the reference's complete case analysis
     * (short_weierstrass_jacobian.rs:570-597).  Without the flag G1 bases are taken to lie in G1 -- as every proving-key and SRS element
     * does (the reference deserialises them with a subgroup check) -- and the bucket kernels use the curve's twisted Edwards form, whose
     * unified 7-multiplication addition is exception-free exactly on that subgroup.  Results are the same group elements either way.
     * A base of even order registered WITHOUT this flag (and without the check below) can meet an exceptional pair of the unified law
     * and yield a wrong group element with status CZK_OK: a caller that cannot vouch for its bases passes one of the two flags. */
    CZK_MEM_ANY_POINTS = 64,
    /* czk_bases_register only, OR-ed in: verify the assumption instead of trusting it.  Registration runs the reference's
     * is_in_correct_subgroup_assuming_on_curve ([r] P == infinity, short_weierstrass_jacobian.rs:131; plus y^2 = x^3 + b) on every base
     * -- what the reference does when it deserialises a key (:868, :881) -- and keeps the handle on the complete XYZZ kernels when any
     * base fails, exactly as CZK_MEM_ANY_POINTS would.  czk_bases_check_subgroup then reports the count without re-running.  Costs about
     * as much as building the window tables (252 doublings + 87 additions per point; 2^20 G1 points: ~0.1 s). */
    CZK_MEM_CHECK_SUBGROUP = 128,
    /* czk_fr_vec_scale only, OR-ed with CZK_MEM_DEVICE: the vectors are device memory, the scalar `k` is HOST memory, read when the call is
     * made and handed to the kernel with the launch -- no device copy of a 32-byte value, no lifetime to observe. */
    CZK_MEM_SCALAR_HOST = 256,
    /* czk_msm_async only, OR-ed with CZK_MEM_DEVICE | CZK_MEM_STABLE: the scalars are those of the most recent czk_msm_async call on this context that
     * did NOT carry this flag (the leader of a group of calls over one vector) -- same pointer, count, lanes and form, that call CZK_MEM_STABLE too,
     * the buffer unchanged -- as when one assignment vector meets several queries (Groth16's a, b_g1, b_g2: groth16/src/prover.rs:130-166 passes
     * `assignment` three times).  The library may then read a digit sort made by the leader (or by a later member of the group) instead of sorting
     * again; it does while that sort is still in one of the pipeline's workspace slots and both keys run the same table layout (size, window width)
     * and have the same points at infinity, otherwise the flag changes nothing (nor does it unless the option "msm_sort_reuse" is set).  Results are the same either way.  Nothing is carried from one
     * group to the next or across czk_ctx_sync / czk_ctx_wait_mark: the next proof's first call over the same buffer sorts again. */
    CZK_MEM_SAME_SCALARS = 512
} czk_mem;

/* EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}_in_place (algebra/poly/src/domain/mod.rs:79,90,139,155) */
typedef enum { CZK_FFT = 0, CZK_IFFT = 1, CZK_COSET_FFT = 2, CZK_COSET_IFFT = 3 } czk_ntt_kind;

/* scalar encodings accepted by the MSM */
typedef enum {
    CZK_SCALAR_CANONICAL = 0, /* BigInteger256, as VariableBaseMSM::multi_scalar_mul takes (msm/variable_base.rs:12-15) */
    CZK_SCALAR_MONTGOMERY = 1 /* Fr, as AffineCurve::multi_scalar_mul takes; into_repr runs on the GPU (ec/src/lib.rs:300-311) */
} czk_scalar_form;

typedef enum { CZK_G1 = 1, CZK_G2 = 2 } czk_group;

/* ---- context ------------------------------------------------------------------------------------ */
/* `hip_stream`: a hipStream_t to enqueue on (e.g. torch's current stream), or NULL for a private one. */
int czk_ctx_create(czk_ctx** out, int device, void* hip_stream);
void czk_ctx_destroy(czk_ctx* ctx);
int czk_ctx_sync(czk_ctx* ctx);
/* Waiting for PART of a context's work.  The reference's polynomial provers stop at every transcript point for what the transcript absorbs there
 * (the commitments and evaluations sent so far: mpc-plonk/src/lib.rs:430-448, marlin/src/lib.rs:176-318) -- not for everything the prover has
 * started: work that depends on no pending challenge (the next round's transforms of public data, commitments of polynomials that are already
 * known) can be enqueued before the wait and runs through it.  czk_ctx_mark names the work enqueued on the context so far -- kernels on its stream,
 * czk_msm_async calls, czk_lanes_download_deferred copies; czk_ctx_wait_mark blocks until THAT work is done and delivers its host results (what
 * czk_ctx_sync does for all work), while calls made after the mark keep running.  A mark covers the marks taken before it; waiting for a retired mark
 * returns at once; czk_ctx_sync retires every mark. */
int czk_ctx_mark(czk_ctx* ctx, uint64_t* out_mark);
int czk_ctx_wait_mark(czk_ctx* ctx, uint64_t mark);
/* The hipStream_t the context enqueues on (the one given to czk_ctx_create, or its private stream): lets a caller order its own
 * streams against the context's with events (hipStreamWaitEvent) instead of czk_ctx_sync -- e.g. an RCCL exchange between two opens. */
void* czk_ctx_stream(const czk_ctx* ctx);
/* What the library otherwise allocates and builds on FIRST use, done now: the twiddle / coset tables of the radix-2 domain 2^ntt_log_d and the
 * pass scratch for `ntt_lanes` lanes (ntt_lanes = 0: skip), and -- for MSMs of n_scalars scalars x msm_lanes lanes over `bases` (NULL: skip) --
 * the MSM pipeline's streams, the table set such calls use and every workspace of its ring.  A prover that cares about the latency of its first
 * proof after loading a key calls this once per (domain, key); results are unaffected.  Blocking. */
int czk_ctx_reserve(czk_ctx* ctx, unsigned ntt_log_d, size_t ntt_lanes, const czk_bases* bases, size_t n_scalars, size_t msm_lanes);
const char* czk_last_error(const czk_ctx* ctx);
const char* czk_version(void);
/* Tuning options of one context.  The library reads NO environment variables: everything a caller may select is named here.
 *   "msm_slots" 1..4            depth of the MSM pipeline's workspace ring (default 4)                          [before the first MSM]
 *   "msm_stream_priority" 0..2  0 = equal priorities (default), 1 = sort / reduce streams above accumulate, 2 = the reverse [before the first MSM]
 *   "msm_lane_interleave" 0..64 lanes per interleave group of the bucket accumulation kernels: neighbouring threads take the same bucket rank of G
 *                               neighbouring share lanes (1 = one lane per workgroup row, the layout of rounds 1 - 5; 0 = the library's default: 4 for keys
 *                               with window tables, 1 on the table-free path)
 *   "msm_sort_reuse" 0/1        honour CZK_MEM_SAME_SCALARS between keys registered AFTERWARDS (default 0 = every call sorts: sharing b_g2's sort with b_g1 measured + 0.5 % per proof when the two
 *                               calls are neighbours, - 0.6 % two calls apart -- the sorts run beside the accumulate kernels anyway, and entries sorted a moment
 *                               ago are still in the last-level cache when their own accumulate kernel reads them)
 *   "msm_sort_onepass" 0/1      single-pass digit sort for every call (default: never -- the partitioned sort)
 *   "msm_fixed_c" 0/1           keys registered AFTERWARDS keep their own window width for short calls (no secondary table sets)
 *   "msm_window_g1" / "msm_window_g2" 0, 8..22   primary window width of keys registered AFTERWARDS (0 = the cost model, default)
 *   "msm_reduce_lean" 0..3      a bit set (default 3) for the bucket reduction of keys in twisted Edwards form: 1 = its running sums start from the entries themselves
 *                               instead of the neutral element, 2 = (with 1) one 2 D T product serves both additions a running sum takes part in; a clear bit = the
 *                               same group element from the kernel of before (the Jacobian triple of a result may differ by a projective factor)
 *   "ntt_gen1" 0/1              first-generation NTT passes (the small-domain kernels) for every size
 *   "ntt_fuse_pairs" 0/1        czk_witness_map_pre/post: the last pass of an inverse transform and the first pass of the coset transform that follows it
 *                               as one kernel where their tiles line up (2^21, 2^18, 2^15, 2^14, 2^12); same values; default 0 (+ 0.5 % per proof measured)
 *   "witness_map_short" 0..7    a bit set (default 7): 1 = czk_witness_map_post_h transforms c once (6 transforms per witness map instead of 7), 2 = czk_witness_map_pre_masked
 *                               adds its masks on the transforms' last store, 4 = czk_spdz_open_combine is one kernel; a clear bit = the same values from the longer
 *                               kernel sequence (without bit 1, `c` holds coset_fft(ifft(c)) instead of ifft(c) after czk_witness_map_post_h: scratch either way)
 *   "net_create_timeout_ms" 0..3600000   how long czk_net_create on this context waits for its peers at the rendezvous (0 = the default, 120 s;
 *                               afterwards the communicator's own "timeout_ms" option applies)
 * Any other name is CZK_ERR_ARG.  The call drains the context's enqueued work first, so an option never changes under a running proof.
 * (libczk_hip_lab.so, the -DCZK_LAB build of the same sources, additionally knows the switches of the measured-and-rejected kernel
 * variants it alone contains -- EXPERIMENTS.md; czk_build_is_lab() tells the two apart.) */
int czk_ctx_set_option(czk_ctx* ctx, const char* name, long value);
int czk_build_is_lab(void);

/* ---- device-resident share lanes ---------------------------------------------------------------------- */
/* A caller without a HIP allocator of its own (the Rust shim, a C++ host) keeps share vectors on the GPU between calls through
 * these handles: R1CStoQAP::witness_map holds `a`, `b`, `c` across seven transforms and hands `h` straight to the MSM
 * (mpc-snarks/src/groth/r1cs_to_qap.rs:85-110, mpc-snarks/src/groth/prover.rs:104) -- with a handle none of that crosses PCIe.
 * A czk_lanes is `lanes` x `len` Fr (lane-major, 4 u64 per element: the layout every `lanes x D x 4 u64` argument of this
 * header has), allocated zero-filled (`vec![T::zero(); domain_size]`, r1cs_to_qap.rs:66-67) on the context's GPU.
 * czk_lanes_data(l, lane, elem) is the address of one element: pass it wherever a buffer argument is taken with
 * CZK_MEM_DEVICE (czk_ntt_fr, czk_fr_vec_op, czk_witness_map_pre/post, czk_r1cs_matvec, czk_msm(_async), ...).  NULL when
 * (lane, elem) is outside the allocation.  The handle must be freed before its context is destroyed.
 * czk_lanes_upload: n Fr from pageable HOST memory (a Rust Vec) into lane `lane` at element `elem`, staged through the context's
 * pinned buffers; returns once `host` has been read (the caller may drop the Vec), the last DMA completes in stream order
 * before any later call on the context (a run may continue into the following lanes: the array is contiguous).  czk_lanes_download: the reverse, blocking (the values are in `host` on return).
 * czk_lanes_copy: device-to-device, in stream order (`let mut ab = a.clone()`).  CZK_ERR_ARG when a range leaves the lanes. */
typedef struct czk_lanes czk_lanes;
int czk_lanes_alloc(czk_ctx* ctx, size_t lanes, size_t len, czk_lanes** out);
void czk_lanes_free(czk_lanes* l);
size_t czk_lanes_count(const czk_lanes* l);
size_t czk_lanes_len(const czk_lanes* l);
uint64_t* czk_lanes_data(const czk_lanes* l, size_t lane, size_t elem);
int czk_lanes_upload(czk_ctx* ctx, czk_lanes* dst, size_t lane, size_t elem, const uint64_t* host, size_t n);
int czk_lanes_download(czk_ctx* ctx, const czk_lanes* src, size_t lane, size_t elem, uint64_t* host, size_t n);
/* czk_lanes_download without the wait: the copy is enqueued in stream order (through the library's pinned result staging, at most 4 MiB pending) and
 * `host` is filled when a mark taken after this call is waited for (czk_ctx_wait_mark) or at the next czk_ctx_sync -- the delivery rule of
 * czk_msm_async's results.  `host` must stay valid until then. */
int czk_lanes_download_deferred(czk_ctx* ctx, const czk_lanes* src, size_t lane, size_t elem, uint64_t* host, size_t n);
int czk_lanes_copy(czk_ctx* ctx, czk_lanes* dst, size_t dst_lane, size_t dst_elem, const czk_lanes* src, size_t src_lane, size_t src_elem,
                   size_t n);
int czk_lanes_zero(czk_ctx* ctx, czk_lanes* dst, size_t lane, size_t elem, size_t n);

/* Strided copy / zero fill of Fr elements in DEVICE memory, in stream order: for i0 < n[0], i1 < n[1], i2 < n[2]
 *     dst[i0 * dst_stride[0] + i1 * dst_stride[1] + i2 * dst_stride[2]] = src[i0 * src_stride[0] + i1 * src_stride[1] + i2 * src_stride[2]]
 * (strides in Fr elements; src NULL: the destination elements become zero).  One kernel for every re-layout a prover's polynomial code does
 * between transforms -- `resize`, `coeffs[k..].to_vec()`, concatenation of coefficient ranges, stacking share lanes, and the interleave /
 * de-interleave by a stride of mpc-plonk's `shift` products (mpc-plonk/src/lib.rs:150-200) and Marlin's matrix polynomials
 * (marlin/src/ahp/prover.rs:500-640) -- so a host needs no tensor library for them.  Source and destination ranges must not overlap. */
int czk_fr_copy_3d(czk_ctx* ctx, uint64_t* dst, const size_t* dst_stride, const uint64_t* src, const size_t* src_stride, const size_t* n);

/* ---- NTT ---------------------------------------------------------------------------------------- */
/* Replaces Radix2EvaluationDomain<Fr>::{fft,ifft,coset_ifft}_in_place (algebra/poly/src/domain/radix2/mod.rs:99-117)
 * and the trait-default coset_fft_in_place (domain/mod.rs:139-142) for T = Fr lanes (an MpcField<Fr, SpdzFieldShare>
 * vector is two lanes: sh and mac; mpc-algebra/src/share/spdz.rs:186-202).
 * data: lanes x D x 4 u64, D = 2^log_d, lane-major, transformed in place, natural order in and out.
 * in_len <= D: entries [in_len, D) of every lane are taken as zero (`resize(size, T::zero())`) whatever they hold.
 * Root of unity = get_root_of_unity(D) = LARGE_SUBGROUP_ROOT_OF_UNITY^3 squared down (ff/src/fields/mod.rs:360-367);
 * coset shift = Fr::multiplicative_generator() = 22.
 * On an error return `data` is undefined (host memory: lanes are written back as they finish, so some may already hold their
 * transform); the reference panics at the corresponding points, so no caller continues with the vector. */
int czk_ntt_fr(czk_ctx* ctx, uint64_t* data, unsigned log_d, size_t lanes, int kind, size_t in_len, int mem);
/* The non-in-place forms EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}(&self, coeffs: &[T]) -> Vec<T> (algebra/poly/src/domain/mod.rs:
 * 72-76, 83-87, 130-134, 146-150: `coeffs.to_vec()` then the in-place transform): reads in_len elements per lane from src (lane k at
 * src + 4 * k * src_stride u64) and writes the 2^log_d results per lane to dst (lane stride 2^log_d); the copy the reference makes is the
 * transform's first load.  src and dst must not overlap unless they are equal with src_stride = 2^log_d.  DEVICE memory only. */
int czk_ntt_fr_to(czk_ctx* ctx, const uint64_t* src, size_t src_stride, uint64_t* dst, unsigned log_d, size_t lanes, int kind,
                  size_t in_len, int mem);

/* Domain constants as the reference's Radix2EvaluationDomain::new computes them (radix2/mod.rs:51-82), Montgomery
 * limbs: out[0..4) size_inv, [4..8) group_gen, [8..12) group_gen_inv, [12..16) generator (22), [16..20) generator_inv,
 * [20..24) (generator^D - 1)^-1 used by divide_by_vanishing_poly_on_coset_in_place (domain/mod.rs:184-191). */
int czk_domain_constants(czk_ctx* ctx, unsigned log_d, uint64_t* out24);

/* MixedRadixEvaluationDomain<Fr>::{fft, ifft, coset_fft, coset_ifft}_in_place (algebra/poly/src/domain/mixed_radix.rs:130-157,
 * 286-404): domains of `size` = 2^a or 3 * 2^a (SMALL_SUBGROUP_BASE = 3 with adicity 1, fr.rs:19-20) -- the Plonk prover's wire
 * domain has 3 * n_gates elements (mpc-plonk/src/relations/flat.rs:282-300).  Same conventions as czk_ntt_fr (data: lanes x size
 * x 4 u64, natural order in and out, in_len <= size, tail taken as zero); root = get_root_of_unity(size)
 * (algebra/ff/src/fields/mod.rs:337-367).  CZK_ERR_SIZE when no such domain exists.  A power-of-two size is the radix-2 transform.
 * czk_mixed_domain_constants: the six constants of czk_domain_constants for MixedRadixEvaluationDomain::new(size). */
int czk_ntt_fr_mixed(czk_ctx* ctx, uint64_t* data, size_t size, size_t lanes, int kind, size_t in_len, int mem);
int czk_mixed_domain_constants(czk_ctx* ctx, size_t size, uint64_t* out24);

/* ---- element-wise Fr vector ops (the share-local pointwise steps of witness_map) ------------------ */
/* out[i] = a[i] op b[i], n elements of 4 u64; out may alias a or b.  r1cs_to_qap.rs:92 (plain product), :105-107 (sub). */
typedef enum { CZK_OP_ADD = 0, CZK_OP_SUB = 1, CZK_OP_MUL = 2 } czk_binop;
int czk_fr_vec_op(czk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, int mem);
/* out[i] = a[i] * k  (k: one Montgomery Fr in the SAME memory space as a / out; domain/mod.rs:184-191).  In DEVICE memory the call only
 * enqueues and the kernel reads `k` in stream order: `k` must stay valid and unmodified until the context's stream has passed this call (the
 * same holds for czk_ntt_fr_to's `src`). */
int czk_fr_vec_scale(czk_ctx* ctx, const uint64_t* a, const uint64_t* k, uint64_t* out, size_t n, int mem);
/* out[i] = c * g^i for i < n (g, c: one Montgomery Fr each, HOST memory; c NULL = one): the table behind
 * EvaluationDomain::distribute_powers / distribute_powers_and_mul_by_const (algebra/poly/src/domain/mod.rs:93-106) for any g --
 * coset shifts other than the generator, and `shift(p, w)` of the Plonk prover (mpc-plonk/src/util.rs).  Multiply with
 * czk_fr_vec_op(CZK_OP_MUL) per lane. */
int czk_fr_powers(czk_ctx* ctx, const uint64_t* g, const uint64_t* c, size_t n, uint64_t* out, int mem);
/* Local half of Beaver multiplication (mpc-algebra/src/share/field.rs:97-127), per lane:
 *   out[i] = z[i] - y[i]*sx[i] - x[i]*oy[i] + (add_open ? sx[i]*oy[i] : 0)
 * x, y, z: this party's triple shares; sx, oy: the opened values; add_open = this party applies `shift`
 * (king for the sh lane, mac_share != 0 for the mac lane; share/spdz.rs:31-37,204-208). */
int czk_fr_beaver_combine(czk_ctx* ctx, const uint64_t* x, const uint64_t* y, const uint64_t* z, const uint64_t* sx,
                          const uint64_t* oy, int add_open, uint64_t* out, size_t n, int mem);
/* Local arithmetic of SpdzFieldShare::batch_open (mpc-algebra/src/share/spdz.rs:166-185) once every party's shares
 * are on this GPU (parties as lanes, or after the all-gather of mpc-net's broadcast):
 *   shares: parties x 2 x n Fr (party-major; lane 0 = sh, lane 1 = mac), DEVICE memory
 *   value[i]  = sum_p sh_p[i]                                             -> out_value (n Fr, device)
 *   check[i]  = sum_p (mac_share_p * value[i] - mac_p[i]),  mac_share_p = (p == 0)   (spdz.rs:31-37, :176-183)
 * *out_bad (host) receives the number of i with check[i] != 0 (the reference asserts it is 0). */
int czk_fr_spdz_open(czk_ctx* ctx, const uint64_t* shares, size_t parties, size_t n, uint64_t* out_value, uint64_t* out_bad);
/* Both opens of S::batch_mul and its local combine (share/field.rs:97-127, share/spdz.rs:166-185) in one kernel, for `parties` (1..32) parties whose lanes are all on
 * this GPU.  DEVICE memory, every vector n Fr per lane, lanes party-major (lane 2 p = sh, 2 p + 1 = mac of party p) and n elements apart:
 *   a, b        2 parties lanes each: the masked factors s + x and o + y        tx, ty, tz   2 parties lanes each: the triple's shares
 *   sx[i] = sum_p a_sh_p[i], oy[i] = sum_p b_sh_p[i]                                      (n Fr each)
 *   chk_a[i] = sx[i] - sum_p a_mac_p[i], chk_b[i] = oy[i] - sum_p b_mac_p[i]             (n Fr each; all zero unless a MAC is broken)
 *   ab_ln[i] = tz_ln[i] - ty_ln[i] sx[i] - tx_ln[i] oy[i] + (bit ln of king_mask ? sx[i] oy[i] : 0)      (2 parties lanes)
 * The outputs must not overlap the inputs or one another.  Same values as czk_fr_vec_op per open and czk_fr_beaver_combine per lane. */
int czk_spdz_open_combine(czk_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, size_t parties,
                          uint64_t king_mask, uint64_t* sx, uint64_t* oy, uint64_t* chk_a, uint64_t* chk_b, uint64_t* ab, size_t n);

/* The same open round by round, as the reference runs it when every party is its own process (share/spdz.rs:166-185) --
 * between the calls the caller moves the vectors with mpc-net's broadcast / atomic_broadcast (RCCL all-gather here):
 *   round 1: every party broadcasts its `sh` lane;  values = czk_fr_lanes_sum(gathered sh lanes)
 *   local  : dx_t = czk_fr_spdz_dx(values, own mac lane, own mac_share)      (mac_share: one Montgomery Fr, HOST memory)
 *   round 2: atomic_broadcast(dx_t);  czk_fr_lanes_sum(gathered dx_t, out = NULL, &nonzero) must report 0.
 * czk_fr_lanes_sum: out[i] = sum_{j<k} x[j][i] over k vectors of n Fr (x: k x n, DEVICE); out (device, may be NULL) receives
 * the sums, *out_nonzero (host, may be NULL) the number of non-zero sums. */
int czk_fr_lanes_sum(czk_ctx* ctx, const uint64_t* x, size_t k, size_t n, uint64_t* out, uint64_t* out_nonzero);
int czk_fr_spdz_dx(czk_ctx* ctx, const uint64_t* value, const uint64_t* mac, const uint64_t* mac_share, uint64_t* out, size_t n);

/* GSZ / Shamir shares (mpc-algebra/src/share/gsz20/mod.rs): party j of n holds p(w^j), w = the order-n root of
 * MixedRadixEvaluationDomain::new(n_parties) (gsz20/mod.rs:98-105; algebra/poly/src/domain/mixed_radix.rs:57-107; root rule
 * algebra/ff/src/fields/mod.rs:337-367 with SMALL_SUBGROUP_BASE = 3).  A GSZ share vector is ONE Fr lane for the NTT / MSM
 * entry points (add / scale are lane-wise, gsz20/mod.rs:260-284).
 * czk_share_domain_constants: out[0..4) size_inv, [4..8) group_gen, [8..12) group_gen_inv (Montgomery limbs); CZK_ERR_SIZE when
 * n_parties is not 2^a or 3 * 2^a (the reference's `domain()` panics).
 * czk_fr_gsz_open = the local part of batch_open (:286-300) -> open_degree_vec (:440-466) once all parties' values are on this
 * GPU: shares: parties x n Fr (party-major, DEVICE); per element the size-n inverse DFT, p(0) -> out_value (n Fr, device);
 * *out_bad (host) = number of elements whose interpolating polynomial exceeds its degree bound (the reference asserts
 * p.degree() <= d): bound = degrees[i] (device u32 array) or `degree` when degrees is NULL. */
int czk_share_domain_constants(czk_ctx* ctx, size_t parties, uint64_t* out12);
int czk_fr_gsz_open(czk_ctx* ctx, const uint64_t* shares, size_t parties, size_t n, const uint32_t* degrees, unsigned degree,
                    uint64_t* out_value, uint64_t* out_bad);

/* ---- mpc-net between GPUs: the opens' transport, behind the C ABI -------------------------------- */
/* The reference's parties talk through the process-global MpcMultiNet (mpc-net/src/multi.rs:15-23: one TCP connection per pair of
 * parties) with four primitives -- broadcast (:145-173), send_to_king (:175-210), recv_from_king (:211-242) and, on top of them,
 * MpcSerNet::atomic_broadcast (mpc-algebra/src/channel.rs:50-75).  A czk_net is the same thing for parties that are czk contexts:
 * one communicator per (context, party), its exchanges enqueued on the context's stream (czk_ctx_stream), so a share vector that
 * the context's kernels produce is exchanged, summed and checked WITHOUT leaving HBM and without a host synchronisation between
 * the kernels and the exchange.  Two transports:
 *   CZK_NET_RCCL  one party per GPU of one node: RCCL over xGMI (ncclCommInitRank).  id = the 128 bytes czk_net_unique_id returned on
 *                 rank 0, carried to the other parties by whatever channel started them (the reference's host has mpc-net's TCP for it).
 *                 librccl.so.1 is dlopen-ed on first use: the library has no link-time dependency on RCCL.
 *   CZK_NET_SHM   parties are processes of one node in ANY assignment to GPUs -- several parties on ONE GPU included -- staged through a
 *                 POSIX shared-memory segment named by the id bytes (pinned by every party: two DMA copies per buffer).  For rigs with
 *                 fewer GPUs than parties and for tests; blocks the host for the duration of each exchange.  id: 1..32 arbitrary bytes
 *                 the launcher chooses, the same on every rank and FRESH for every communicator (czk_net_unique_id(CZK_NET_SHM) draws 16 random
 *                 bytes: a rank that finds the segment of an earlier run under its id would wait there until the timeout).  ctx may be NULL:
 *                 host-memory primitives only (no composite opens).  A failure on one rank aborts the communicator for all of them.
 *   CZK_NET_IPC   like CZK_NET_SHM (same id rule, same control block and barrier in shared memory), but the staging slots are DEVICE memory:
 *                 every rank owns a mailbox on its GPU and maps the others' with hipIpc, so an exchange is device-to-device copies (on one GPU: inside
 *                 HBM; across GPUs of a node: peer copies) and only the barrier touches the host.  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment
 *                 of this driver stack; a context is required.
 * czk_net_create is collective (returns once every rank has joined; CZK_ERR_NET after the timeout).  All ranks call the same
 * sequence of exchanges, like the reference's lock-step rounds.  Buffers: `mem` = CZK_MEM_DEVICE (on the context's GPU, used in
 * stream order) or CZK_MEM_HOST (read / written before the call returns).  Byte counts must be equal on all ranks (mpc-net asserts it).
 * Options (czk_net_set_option): "exchange" 0 = ring (one ncclAllGather), 1 = p2p (world - 1 grouped ncclSend / ncclRecv pairs: every
 * pair of GPUs of an MI355X node has its own xGMI link -- mpc-net's own star shape); "timeout_ms" (default 120000);
 * "slot_bytes" (SHM: staging slot per rank, default 16 MiB; before the first exchange). */
typedef struct czk_net czk_net;
typedef enum { CZK_NET_RCCL = 1, CZK_NET_SHM = 2, CZK_NET_IPC = 3 } czk_net_transport;
#define CZK_NET_UNIQUE_ID_BYTES 128
int czk_net_unique_id(int transport, uint8_t* out, size_t cap, size_t* len);
int czk_net_create(czk_ctx* ctx, int transport, int rank, int world, const uint8_t* id, size_t id_len, czk_net** out);
void czk_net_destroy(czk_net* net);
int czk_net_rank(const czk_net* net);    /* MpcNet::party_id */
int czk_net_world(const czk_net* net);   /* MpcNet::n_parties */
int czk_net_set_option(czk_net* net, const char* name, long value);
const char* czk_net_last_error(const czk_net* net);
/* mpc-net's Stats (mpc-net/src/lib.rs: bytes_sent, bytes_recv, broadcasts, to_king, from_king), counted by the reference's rules:
 * out[0..5) in that order.  czk_net_stats_reset = MpcNet::reset_stats. */
int czk_net_stats(const czk_net* net, uint64_t* out5);
void czk_net_stats_reset(czk_net* net);
/* broadcast (multi.rs:145-173): every party contributes `bytes` bytes; recv (world x bytes, party order) receives all of them. */
int czk_net_broadcast(czk_net* net, const void* send, size_t bytes, void* recv, int mem);
/* send_to_king (multi.rs:175-210): recv (world x bytes, party order) is written on the king (rank 0) only and may be NULL elsewhere. */
int czk_net_send_to_king(czk_net* net, const void* send, size_t bytes, void* recv, int mem);
/* recv_from_king (multi.rs:211-242): the king hands party p the p-th of `world` equally long buffers (send: world x bytes on the
 * king, ignored elsewhere); recv (bytes) receives this party's.  The reference prefixes each message with its u64 length
 * (multi.rs:219-228); here lengths are arguments and only the stats count the 8 bytes. */
int czk_net_recv_from_king(czk_net* net, const void* send, size_t bytes, void* recv, int mem);
/* All-to-all (mpc-net has no such primitive; the GSZ material's dealing needs one): send is world x bytes and part p goes to party p; recv is
 * world x bytes and part p came from party p; the caller's own part is a local copy.  Over CZK_NET_SHM / CZK_NET_IPC a rank's slot carries `world`
 * segments per chunk step, so the chunk per destination is slot_bytes / world rounded down to 16 bytes (less than 16: CZK_ERR_SIZE); over
 * CZK_NET_RCCL it is one group of world - 1 send / receive pairs.  Stats: (world - 1) bytes go into out[0] and out[1]; none of the three exchange
 * counters moves. */
int czk_net_alltoall(czk_net* net, const void* send, size_t bytes, void* recv, int mem);
int czk_net_barrier(czk_net* net);
/* MpcSerNet::atomic_broadcast of one Vec<Fr> (channel.rs:50-75): round 1 broadcasts SHA-256(serialize(x) || 32 random bytes), round 2
 * the vector and the randomness; every receiver re-hashes what the others sent (CZK_ERR_CHECK on a mismatch).  x: n Montgomery Fr
 * (`mem`), recv: world x n Fr.  The commitment runs over the reference's wire bytes (czk_fr_vec_serialize), so equal data and
 * randomness give the reference's hashes.  rand32: the 32 commitment bytes (tests), NULL = drawn from the OS.  Hashing is host
 * work over a download of the vectors: the protocol's check, not hot-path arithmetic -- the opens below take it as an option. */
int czk_net_atomic_broadcast(czk_net* net, const uint64_t* x, size_t n, uint64_t* recv, const uint8_t* rand32, int mem);

/* "czk tree commitment v1": a second, opt-in commitment for the same round, computed on the GPU where the vector lives (commit_tree.hip).
 * NOT the reference's bytes: for parties that are all this library (every czk_net transport), never for a party on the reference's sockets.
 *   E = CZK_COMMIT_LEAF_ELEMS, F = CZK_COMMIT_FANOUT.  TAG_LEAF / TAG_NODE / TAG_ROOT = the ASCII strings "czk-commit-v1/leaf", "czk-commit-v1/node",
 *   "czk-commit-v1/root", zero-padded to 64 bytes (one SHA-256 block each).  bytes(a_k) = into_repr() as 32 little-endian bytes (czk_fr_vec_serialize's).
 *   leaf_i = SHA256(TAG_LEAF || bytes(a[i E]) .. bytes(a[min(n, (i + 1) E) - 1])), max(1, ceil(n / E)) leaves (n = 0: the one leaf is SHA256(TAG_LEAF));
 *   node_j = SHA256(TAG_NODE || up to F consecutive digests of the level below), level by level until one digest `top` is left (one leaf: top = leaf_0);
 *   commitment = SHA256(TAG_ROOT || u64_le(n) || top || rand32).
 * czk_fr_vec_commit: a = `lanes` vectors of n Montgomery Fr, `stride` elements apart, in `mem` (host memory is uploaded and hashed by the same
 * kernels); rand32 and out32: lanes x 32 bytes, HOST.  Blocks.  Reads a[lane][0..n) only.  stride < n or byte counts that overflow: CZK_ERR_SIZE;
 * lanes = 0: CZK_OK, nothing touched; n = 0: the empty vector's commitment. */
#define CZK_COMMIT_LEAF_ELEMS 32
#define CZK_COMMIT_FANOUT 32
int czk_fr_vec_commit(czk_ctx* ctx, const uint64_t* a, size_t lanes, size_t n, size_t stride, const uint8_t* rand32, uint8_t* out32, int mem);
/* czk_net_atomic_broadcast with the tree commitment: same contract, rounds, byte counts and stats.  The receiver checks all `world` gathered vectors
 * in one czk_fr_vec_commit pass (lanes = world, stride = n) and compares digests on the host: with CZK_MEM_DEVICE no element byte crosses to the host,
 * only commitments, randomness and world x 32 digest bytes.  All ranks must make the same call: against a rank that used czk_net_atomic_broadcast
 * nothing hangs (equal byte counts) and every honest rank gets CZK_ERR_CHECK. */
int czk_net_atomic_broadcast_tree(czk_net* net, const uint64_t* x, size_t n, uint64_t* recv, const uint8_t* rand32, int mem);

/* The reference's batch opens as ONE call each on device lanes (all buffers CZK_MEM_DEVICE on the communicator's context; gathered
 * shares live in the communicator's own scratch).  flags: CZK_OPEN_COMMIT = the second round goes through czk_net_atomic_broadcast;
 * CZK_OPEN_COMMIT_TREE (with or without CZK_OPEN_COMMIT) = through czk_net_atomic_broadcast_tree.
 *   czk_spdz_batch_open  SpdzFieldShare::batch_open (mpc-algebra/src/share/spdz.rs:166-185): broadcast of the sh lane, value = sum;
 *                        dx_t = mac_share * value - mac; (atomic_)broadcast of dx_t; *out_bad = number of i whose dx_t do not sum to
 *                        zero (the reference asserts 0).  sh, mac: n Fr each; mac_share: one Montgomery Fr, HOST (1 on the king, 0
 *                        elsewhere with the reference's stand-in key, spdz.rs:30-37); MAC shares never leave the party.
 *   czk_add_batch_open   AdditiveFieldShare::batch_open (share/add.rs:256-259): broadcast, sum.
 *   czk_gsz_batch_open   GszFieldShare::batch_open (share/gsz20/mod.rs:286-300) -> open_degree_vec (:440-466): broadcast, per element
 *                        the size-world inverse DFT, degree check, p(0); degrees / degree / out_bad as in czk_fr_gsz_open.
 * out_value may alias the input share lane.  Each call ends with the read-back of its check count (the reference asserts right there). */
#define CZK_OPEN_COMMIT 1
#define CZK_OPEN_COMMIT_TREE 2
int czk_spdz_batch_open(czk_net* net, const uint64_t* sh, const uint64_t* mac, const uint64_t* mac_share, size_t n, uint64_t* out_value,
                        int flags, uint64_t* out_bad);
int czk_add_batch_open(czk_net* net, const uint64_t* val, size_t n, uint64_t* out_value);
int czk_gsz_batch_open(czk_net* net, const uint64_t* val, size_t n, const uint32_t* degrees, unsigned degree, uint64_t* out_value,
                       uint64_t* out_bad);
/* ---- products, inverses and running products of SHARED vectors (mpc-algebra/src/share/field.rs) ------------------------------------ */
/* FieldShare::batch_mul (:97-127), batch_inv (:135-148) and partial_products (:163-182) as one call each on device lanes, for additive shares
 * (lpp = 1 lane per party) and SPDZ shares (lpp = 2: lane lpp p = party p's sh, lane lpp p + 1 = its mac -- czk_spdz_open_combine's order).
 * batch_div is czk_share_batch_mul after czk_share_batch_inv.  GSZ shares have calls of their own: czk_gsz_share_* below.
 *   lanes form (czk_share_*)     all `parties` (1..32) parties' lanes on this GPU: every vector is L = lpp parties lanes.  Nothing leaves the device
 *                                but the two counts.  mac_shares: parties x 4 limbs, one Montgomery Fr per party, HOST (NULL allowed for lpp = 1).
 *   net form (czk_net_share_*)   one party per communicator: every vector is this party's lpp lanes; the opens go through czk_add_batch_open
 *                                (lpp = 1) / czk_spdz_batch_open (lpp = 2) with `flags`.  mac_share: this party's Montgomery Fr, HOST.
 * Operands and `out`: n Fr per lane, lanes n elements apart.  Material: the caller's correlated randomness in the same lane order, T triples
 * (tx, ty, tz with tz = tx ty) resp. P pairs (pb, pc) of BeaverSource::inv_pair per lane, lanes T resp. P elements apart, consumed in the
 * reference's order (czk_share_material_counts reports T and P):
 *   CZK_SHARE_OP_MUL               T = n, P = 0
 *   CZK_SHARE_OP_INV               T = n, P = n       pair i is (b, c) of element i; triple i multiplies x_i b_i
 *   CZK_SHARE_OP_PARTIAL_PRODUCTS  T = 4 n, P = 2 n + 1   pairs [0, n] are (m, m_inv), pairs [n + 1, 2 n] the inner batch_inv's; triples [0, n) m x,
 *                                  [n, 2 n) (m x) m_inv, [2 n, 3 n) m_0 m_inv, [3 n, 4 n) the inner batch_inv's product
 * The calls apply the reference's formulas to whatever pairs they are given.  Its only source hands out (1, 1); for the results to be the inverse
 * and the running products with random material, each slot needs the relation its formula uses: (m, m_inv) are inverses, m m_inv = 1, and a
 * batch_inv pair is a mask and itself, c = b (c / open(x b) = 1 / x).
 * Values (every lane equals the reference's for that party, limb for limb; a public addend v goes to the king's sh lane and as mac_share_p v to
 * party p's mac lane, share/spdz.rs:204-208):
 *   batch_mul          out = tz - ty open(x + tx) - tx open(y + ty) + shift(open(x + tx) open(y + ty)).  The two opens are independent: they run as ONE open
 *                      of the 2 n-element concatenation (same values; the net form counts half the reference's broadcasts in czk_net_stats).
 *   batch_inv          out = c open(batch_mul(x, b))^-1
 *   partial_products   out_i = shares of x_0 ... x_i, exactly :163-182
 * *out_bad (host): opened elements whose MAC check failed, over all opens of the call (always 0 for lpp = 1; the reference asserts 0).
 * *out_zero (host): opened values that had to be inverted and were zero (the reference unwraps): that element's output is zero on every lane, as
 * czk_fr_batch_inverse keeps zeros.  Always 0 for batch_mul.  Both are read back at the end of the call (it blocks, like the opens).
 * n = 0 or parties = 0: CZK_OK, nothing touched but the counts.  NULL vectors with work to do, lpp not 1 or 2, parties > 32: CZK_ERR_ARG; lane
 * arrays whose byte count overflows: CZK_ERR_SIZE.  `out` must not overlap an input.  Workspace comes from the context's staging pool. */
#define CZK_SHARE_OP_MUL 0
#define CZK_SHARE_OP_INV 1
#define CZK_SHARE_OP_PARTIAL_PRODUCTS 2
int czk_share_material_counts(int op, size_t n, size_t* triples, size_t* pairs);
int czk_share_batch_mul(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* x, const uint64_t* y, const uint64_t* tx,
                        const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_share_batch_inv(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* x, const uint64_t* pb, const uint64_t* pc,
                        const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_share_partial_products(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* x, const uint64_t* pb,
                               const uint64_t* pc, const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, uint64_t* out_bad,
                               uint64_t* out_zero);
int czk_net_share_batch_mul(czk_net* net, size_t lpp, const uint64_t* mac_share, const uint64_t* x, const uint64_t* y, const uint64_t* tx,
                            const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, int flags, uint64_t* out_bad, uint64_t* out_zero);
int czk_net_share_batch_inv(czk_net* net, size_t lpp, const uint64_t* mac_share, const uint64_t* x, const uint64_t* pb, const uint64_t* pc,
                            const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, int flags, uint64_t* out_bad,
                            uint64_t* out_zero);
int czk_net_share_partial_products(czk_net* net, size_t lpp, const uint64_t* mac_share, const uint64_t* x, const uint64_t* pb, const uint64_t* pc,
                                   const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t n, int flags, uint64_t* out_bad,
                                   uint64_t* out_zero);

/* ---- products, inverses, running products and the product check of GSZ (Shamir) SHARED vectors (mpc-algebra/src/share/gsz20/mod.rs) ---- */
/* gsz20's batch_mult (:559-594), batch_inv (:325-342), partial_products (:343-366) and the malicious-security product check hadamard_check ->
 * ip_check -> ip_compress / ip_compute (:596-808) as one call each, in the lanes form: all `parties` (1..96, a size czk_share_domain_constants
 * accepts) parties' lanes on this GPU.  A GSZ vector is `parties` lanes of n Fr, party-major, lanes n elements apart; party j's lane holds p(w^j),
 * w = czk_share_domain_constants' group_gen.  Nothing leaves the device but the counts and the verdict.  The same calls with one party per
 * communicator, the product check between processes included, are czk_net_gsz_* below.
 * `degree`: the operands' degree d (normally t = (parties - 1) / 2).  The king's bound on x y + r2 is 2 d; results are shares of degree d.
 * Material: the caller's, in the same lane order, consumed in the reference's order (czk_gsz_material_counts reports D and Rn):
 *   doubles_r / doubles_r2   D double shares (:395-406), lanes D elements apart: the SAME random value under a polynomial of degree d and one of 2 d
 *   rands                    Rn random shares of degree d (:383-388), lanes Rn elements apart
 *   CZK_GSZ_OP_MUL               D = n, Rn = 0
 *   CZK_GSZ_OP_INV               D = n, Rn = n           random share i masks element i (rs of :329); double i multiplies x_i rs_i
 *   CZK_GSZ_OP_PARTIAL_PRODUCTS  D = 5 n + 1, Rn = 3 n + 2   rands [0, n] are m, [n + 1, 2 n + 1] batch_inv(m)'s, [2 n + 2, 3 n + 1] the inner batch_inv's;
 *                                doubles [0, n] batch_inv(m), then n each for m x, (m x) m_inv, m_0 m_inv and the inner batch_inv (m_inv is itself a
 *                                batch_inv here, unlike share/field.rs)
 *   CZK_GSZ_OP_PRODUCT_CHECK     R = ceil(log2 n) (0 for n = 1): D = 2 R + 4, Rn = R + 3.  rands: the hadamard coin, one coin per round, xr, yr; doubles:
 *                                ip_l and ip3 per round, then mult(xr, yr), mult(x, xr), mult(y, yr), mult(ip, ip_r) (:779-782)
 * Values (every output lane equals the reference's arithmetic for that party, limb for limb; tests/gsz_mul_model.py restates it):
 *   batch_mul          out_j = open_2d(x y + r2) - r_j: the king sends the opened value itself to every party (:478, :509)
 *   batch_inv          out_j = rs_j / open_d(batch_mul(x, rs))
 *   partial_products   out_i = shares of x_0 ... x_i, exactly :343-366
 *   product_check      *out_ok = 1 when the final x y == z of :786 holds for the triples (xs_i, ys_i, zs_i), 0 when it does not (a result, not an error).
 *                      xs, ys, zs are not modified.  n < 2^32.
 * Degrees follow the TRUE degrees, where the reference's add / sub leave `degree` alone (rzs_sum stays "degree 0", :605-610): a sum of degree-d shares
 * is a degree-d share, every mult of the check bounds at 2 d and every open at d.
 * *out_bad (host): opens whose interpolating polynomial exceeded its bound (the king's, 2 d, and plain opens, d), over the whole call; the reference asserts.
 * *out_zero (host): as for czk_share_batch_inv.  All are read back once, at the end of the call (it blocks); the check's rounds run without a host
 * synchronisation in between.  n = 0: CZK_OK, nothing touched (*out_ok = 1).  NULL vectors with work to do: CZK_ERR_ARG; no share domain of that size
 * (parties = 0, 5, ...), parties > 96, byte counts that overflow: CZK_ERR_SIZE.  `out` must not overlap an input.  Workspace: the staging pool. */
#define CZK_GSZ_OP_MUL 0
#define CZK_GSZ_OP_INV 1
#define CZK_GSZ_OP_PARTIAL_PRODUCTS 2
#define CZK_GSZ_OP_PRODUCT_CHECK 3
int czk_gsz_material_counts(int op, size_t n, size_t* doubles, size_t* rands);
int czk_gsz_share_batch_mul(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* y, const uint64_t* doubles_r,
                            const uint64_t* doubles_r2, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_gsz_share_batch_inv(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                            const uint64_t* rands, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_gsz_share_partial_products(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* doubles_r,
                                   const uint64_t* doubles_r2, const uint64_t* rands, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_gsz_product_check(czk_ctx* ctx, size_t parties, unsigned degree, const uint64_t* xs, const uint64_t* ys, const uint64_t* zs, size_t n,
                          const uint64_t* doubles_r, const uint64_t* doubles_r2, const uint64_t* rands, uint64_t* out_ok, uint64_t* out_bad);
/* The same four calls with one party per communicator (czk_net_gsz_*): the party is czk_net_rank(net) of czk_net_world(net) parties and every vector is
 * its ONE lane of n Fr, CZK_MEM_DEVICE on the communicator's context.  The material is the party's own lane of the lanes-form material, counted by
 * czk_gsz_material_counts and consumed in the same order.  Give rank j lane j of every input: its `out` is lane j of what czk_gsz_share_* writes on that
 * material, limb for limb, and *out_ok is the lanes form's verdict on every rank.  `degree` and the degree rule are those above.
 * Exchanges per call, as czk_net_stats counts them (a king round trip = one to_king and one from_king; R = ceil(log2 n), 0 for n = 1):
 *   batch_mul          1 king round trip (x y + r2 at bound 2 d), no broadcast
 *   batch_inv          1 king round trip, then 1 broadcast (open of x rs at bound d)
 *   partial_products   5 king round trips, 3 broadcasts: the lanes form's sequence, batch_inv(m); m x; open((m x) m_inv); m_0 m_inv; batch_inv of that
 *   product_check      R + 2 king round trips, R + 2 broadcasts: the hadamard coin (1 broadcast); per round ip_l and ip3 in ONE king round trip of two
 *                      elements, and only then the round's coin (1 broadcast); at the end mult(xr, yr), mult(x, xr), mult(y, yr) in one king round trip,
 *                      mult(ip, ip_r), which needs the first, in a second, and the three blinded values in one broadcast.  All n-sized passes are local;
 *                      the wire carries 2 R + 4 elements to the king and R + 4 broadcast elements per party.  No coin travels in or before the exchange
 *                      that carries the values it challenges.
 * *out_bad counts what this rank can see: the king's bound (2 d) is checked on rank 0 only, as for czk_gsz_batch_king_compute; plain opens (d) are
 * checked, and counted, on every rank.  *out_zero and *out_ok come out equal on all ranks (they follow from broadcast opens).  Counts and verdict are
 * accumulated on the device and read back once, at the end of the call; every rank must make the same call with the same n.
 * A communicator without a context, NULL vectors with work to do: CZK_ERR_ARG.  A world the share domain does not exist for (5, ...), more than 96
 * parties, n >= 2^32 for the check, byte counts that overflow: CZK_ERR_SIZE.  n = 0: CZK_OK, nothing touched, *out_ok = 1.  `out` must not overlap an
 * input; xs, ys, zs are not modified.  Workspace: the context's staging pool, and the communicator's gather scratch on the king. */
int czk_net_gsz_share_batch_mul(czk_net* net, unsigned degree, const uint64_t* x, const uint64_t* y, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                                uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_net_gsz_share_batch_inv(czk_net* net, unsigned degree, const uint64_t* x, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                                const uint64_t* rands, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_net_gsz_share_partial_products(czk_net* net, unsigned degree, const uint64_t* x, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                                       const uint64_t* rands, uint64_t* out, size_t n, uint64_t* out_bad, uint64_t* out_zero);
int czk_net_gsz_product_check(czk_net* net, unsigned degree, const uint64_t* xs, const uint64_t* ys, const uint64_t* zs, size_t n,
                              const uint64_t* doubles_r, const uint64_t* doubles_r2, const uint64_t* rands, uint64_t* out_ok, uint64_t* out_bad);

/* ---- products of a SHARED point and a SHARED scalar (mpc-algebra/src/share/group.rs, share/gsz20/mod.rs) ------------------------------------ */
/* GroupShare::scale (group.rs:70-109, with the SPDZ forms of share/spdz.rs:385-446) and gsz20's group mult (share/gsz20/mod.rs:1112-1130): what a
 * prover needs to multiply a shared point by a shared scalar (mpc-snarks/src/groth/prover.rs:110-114, :135, :156).  Lanes form only: every party's
 * lanes on this GPU, in czk_share_batch_mul's resp. czk_gsz_share_batch_mul's lane order.  All arrays are CZK_MEM_DEVICE on the context's GPU.
 *   a point vector    L lanes of n affine Montgomery points (12 u64 each for CZK_G1, 24 for CZK_G2), lanes n points apart, plus L n infinity bytes in
 *                     the same order.  An input's infinity array may be NULL: no point of it is infinity.  Outputs: infinity is flag 1 with (0, 1).
 *   a scalar vector   L lanes of n Montgomery Fr, lanes n elements apart.
 * SUBGROUP ASSUMPTION: every point is assumed to lie in the prime-order subgroup (they are shares of MSM results under a checked key); the calls do
 * not check it.  Under it scalars may be combined mod r before they multiply a point, and the calls do so; every algebraically equal formulation
 * gives the same affine limbs.
 *
 * czk_share_group_batch_scale: lpp = 1 additive shares, lpp = 2 SPDZ shares (lane 2 p = party p's sh, lane 2 p + 1 = its mac); mac_shares: one
 * Montgomery Fr per party, HOST, any key (NULL allowed for lpp = 1).  s: the shared points, o: the shared scalars; (tx, ty, tz): n group triples,
 * tx and tz points, ty scalars, tz = [ty] tx.  With sx = open(s + tx) (the sum of the sh lanes) and oy = open(o + ty):
 *     out_l = tz_l - [oy] tx_l + [k_l oy - ty_l] sx      k_l = 1 on the king's sh lane (lane 0), mac_share_j on party j's mac lane, 0 elsewhere
 * which is out = z - scale_pub_group(sx, y) - x oy, shifted by [oy] sx (group.rs:90-94).  The lanes of out open to [open(o)] open(s).
 * *out_bad (host): the elements where a MAC check fails: sum_j ([mac_share_j] sx - mac_j(s + x)) is not infinity, or sum_j (mac_share_j oy -
 * mac_j(o + y)) is not 0.  Always 0 for lpp = 1: additive shares carry nothing that could catch a changed share.
 * One kernel, one thread per (lane, element) -- each computes its output as ONE joint double-and-add chain -- plus one thread per element for the
 * MAC checks in the same launch; then the shared batch normalisation; one read-back of the count (the call blocks).
 *
 * czk_gsz_group_batch_mul: `parties` GSZ lanes (party j's lane is the value at w^j); x: shared scalars of degree `degree` d, y: shared points of
 * degree d; (gr, gr2): n group double shares, the SAME random point under a polynomial of degree d (gr) and one of degree 2 d (gr2) in the exponent.
 *     D_j = [x_j] y_j + gr2_j;   V = [1 / P] sum_j D_j  (the king's inverse DFT in the exponent, coefficient 0);   out_j = V - gr_j
 * *out_bad (host): the elements where sum_j [w^(-j k)] D_j is not infinity for some k in (2 d, P): the king's degree bound.
 * The transform is the field version's (czk_fr_gsz_open); the reference's group open_degree_vec (:1048-1080) multiplies shares[i] where the
 * transform needs shares[j], which only works for its constant stand-in shares.  The inverse DFT's scalars go into the parties' chains
 * ([x_j / P] y_j + [1 / P] gr2_j, and one more chain per (party, high coefficient)), so the call is one chain deep: two kernels, the normalisation,
 * one read-back.  czk_gsz_group_material_counts(CZK_GSZ_GROUP_OP_MUL, n): n group doubles, no field doubles, no random shares.
 * czk_share_group_batch_scale consumes n group triples.
 *
 * czk_gsz_group_product_check: hadamard_check -> ip_check -> ip_compress / ip_compute for group triples (:1132-1349) over the n triples (xs_i, ys_i,
 * zs_i), xs scalars, ys and zs points: x_i <- rho^i x_i and ip = sum_i [rho^i] zs_i per lane; R = ceil(log2 n) halving rounds (an odd length reads a
 * zero scalar and an infinite point past its end), each with ip_l = sum [xl] Yl and ip3 = sum [2 xr - xl](2 Yr - Yl) through the king at bound 2 d,
 * the round's coin c, ip_r = ip - ip_l, the parabola [f_1] ip_l + [f_2] ip_r + [f_3] ip3 (:1253-1273) and the fold x <- (xr - xl) c + (2 xl - xr),
 * Y <- [c](Yr - Yl) + (2 Yl - Yr); the end is :1317-1328: two field mults, two group mults, three opens and the verdict [x] y == z.
 * *out_ok = 1 when it holds, 0 when not (a result, not an error); *out_bad: the opens whose polynomial exceeded its bound (the king's, 2 d, and plain
 * opens, d), over the whole call.  Degrees follow the TRUE degrees, as for czk_gsz_product_check.  Coins stay on the device; counts and verdict are
 * read back once, at the end (the call blocks); 3 R + 2 kernel launches, none separated by a host synchronisation.  xs, ys, zs are not modified.
 * Material, consumed in the reference's order (czk_gsz_group_material_counts(CZK_GSZ_GROUP_OP_PRODUCT_CHECK, n) = (2 R + 2, 2, R + 3); 0, 0, 0 for n = 0):
 *   gr / gr2    group doubles, lanes 2 R + 2 points apart: ip_l and ip3 per round, then mult(yr, y), mult(ip_r, ip)
 *   fr / fr2    field doubles (as doubles_r / doubles_r2 of czk_gsz_share_*), lanes 2 elements apart: mult(xr, yr), mult(x, xr)
 *   rands       random shares of degree d, lanes R + 3 apart: the hadamard coin, a coin per round, xr, yr
 * n = 0: CZK_OK, *out_ok = 1.  n >= 2^32: CZK_ERR_SIZE.
 *
 * n = 0 (or parties = 0 for czk_share_group_batch_scale): CZK_OK, nothing touched but *out_bad.  NULL ctx / out_bad, a bad group, lpp not 1 or 2,
 * more than 32 parties, NULL vectors with work to do: CZK_ERR_ARG.  No share domain of that size (0, 5, ...), more than 96 GSZ parties, more
 * outputs than one launch covers (2^36 threads): CZK_ERR_SIZE.  out / out_inf must not overlap an input.  Workspace: the staging pool. */
#define CZK_GSZ_GROUP_OP_MUL 0
#define CZK_GSZ_GROUP_OP_PRODUCT_CHECK 1
int czk_gsz_group_material_counts(int op, size_t n, size_t* group_doubles, size_t* field_doubles, size_t* rands);
int czk_gsz_group_product_check(czk_ctx* ctx, int group, size_t parties, unsigned degree, const uint64_t* xs, const uint64_t* ys, const uint8_t* ys_inf,
                                const uint64_t* zs, const uint8_t* zs_inf, size_t n, const uint64_t* gr, const uint8_t* gr_inf, const uint64_t* gr2,
                                const uint8_t* gr2_inf, const uint64_t* fr, const uint64_t* fr2, const uint64_t* rands, uint64_t* out_ok, uint64_t* out_bad);
int czk_share_group_batch_scale(czk_ctx* ctx, int group, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* s, const uint8_t* s_inf,
                                const uint64_t* o, const uint64_t* tx, const uint8_t* tx_inf, const uint64_t* ty, const uint64_t* tz, const uint8_t* tz_inf,
                                uint64_t* out, uint8_t* out_inf, size_t n, uint64_t* out_bad);
int czk_gsz_group_batch_mul(czk_ctx* ctx, int group, size_t parties, unsigned degree, const uint64_t* x, const uint64_t* y, const uint8_t* y_inf,
                            const uint64_t* gr, const uint8_t* gr_inf, const uint64_t* gr2, const uint8_t* gr2_inf, uint64_t* out, uint8_t* out_inf, size_t n,
                            uint64_t* out_bad);

/* ---- pairings of a SHARED G1 point with a SHARED G2 point; multiplicative target-group shares (mpc-algebra/src/wire/pairing.rs, share/add.rs, share/spdz.rs) -- */
/* MpcPairingEngine::pairing (wire/pairing.rs:194-229) through a pairing triple, and the shares it yields: MulFieldShare (share/add.rs:407-480) and
 * SpdzMulFieldShare (share/spdz.rs:459-541) in Fq12 -- what the reference's PairingDh / PairingProd / PairingDiv computations run on
 * (mpc-snarks/src/client.rs:503-581).  Lanes form only: every party's lanes on this GPU, in czk_share_group_batch_scale's lane order: lpp = 1
 * additive shares, lpp = 2 SPDZ shares (lane 2 p = party p's sh, lane 2 p + 1 = its mac), L = lpp parties lanes, at most 32 parties.  mac_shares:
 * one Montgomery Fr per party, HOST, any key (NULL allowed for lpp = 1).  Every other array is CZK_MEM_DEVICE on the context's GPU (czk_fq12_vec_op
 * takes `mem`).
 *   a G1 / G2 vector        L lanes of n affine Montgomery points (12 / 24 u64 each), lanes n points apart, plus L n infinity bytes in the same order.
 *                           An infinity array may be NULL: no point of it is infinity.
 *   a target-group vector   L lanes of n Fq12 (72 u64 each: c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1, each Fq 6 Montgomery limbs), lanes n
 *                           elements apart.  The shares are MULTIPLICATIVE: the value is the product of the sh lanes, the mac lanes multiply to
 *                           value^key.
 * SUBGROUP ASSUMPTION: as for czk_share_group_batch_scale, every point is assumed to lie in the prime-order subgroup; the calls do not check it.
 *
 * czk_share_pairing: a, b: the shared G1 / G2 operands; (tx, ty, tz): n pairing triples, tx in G1, ty in G2, tz in Fq12, the product of tz's sh
 * lanes = e(open tx, open ty).  With xa = open(a + tx) and yb = open(b + ty) (the sums of the sh lanes) the reference computes
 * z / e(xa, y) / e(x, yb) * e(xa, yb) (pairing.rs:225), the last factor scaled into the share (spdz.rs:500-506, add.rs:444-449).  Here
 *     out_l = tz_l * FE( ML( (-xa, ty_l), (-tx_l, yb), ([k_l] xa, yb) ) )   k_l = 1 on the king's sh lane (lane 0), mac_share_j on party j's mac lane,
 *                                                                           0 elsewhere (the third pair is then left out)
 * -- one Miller loop over two or three pairs, one final exponentiation and one Fq12 product per (lane, element); the same field element, limb for
 * limb, since negating the G1 point inverts a pairing value and e(P, Q)^k = e([k] P, Q) in the prime-order subgroup.  Pairs with an infinite member
 * are skipped (algebra/ec/src/models/bls12/mod.rs:99-103): xa, yb, tx_l, ty_l may all be infinity.  The lanes of out open to e(open a, open b).
 * *out_bad (host): the elements where a MAC check fails: [key] xa - (the sum of the mac lanes of a + tx) is not infinity, or the same for yb in G2
 * (key = the sum of the mac shares mod r; an element counts once).  Always 0 for lpp = 1.  A changed mac lane of tz is not seen here: it travels
 * into out's mac lane and czk_gt_share_open counts it.
 * Three kernels -- the open (one thread per (element, slot), one double-and-add chain deep), G2Prepared::from over the (L + 1) n points ty_l and yb,
 * the product of pairings (one thread per (lane, element)) -- none separated by a host synchronisation; one read-back of the count (the call blocks).
 *
 * czk_gt_share_open: reveal (add.rs:414-416, spdz.rs:469-478): out_i (n x 72) = the product of the sh lanes of v.  For SPDZ the element is counted in
 * *out_bad unless x^A * (the product of the mac lanes)^(-1) is one, A = the INTEGER sum of the canonical mac shares (not reduced mod r): the verdict
 * of the reference's prod_j x^(mac_share_j) / mac_j for any x, inside the order-r subgroup or not.  The reference asserts; here it is a count.
 *
 * czk_gt_share_scale: scale by the public f (n x 72) (spdz.rs:500-506, add.rs:444-449): lane 0 is multiplied by f_i, party j's mac lane by
 * f_i^(mac_share_j), the other lanes are copied.  v = NULL is from_public (spdz.rs:479-485, add.rs:417-421): the lanes start at one.  Only enqueues.
 *
 * czk_fq12_vec_op: out_i = a_i b_i (CZK_FQ12_OP_MUL), a_i / b_i (CZK_FQ12_OP_DIV) or 1 / a_i (CZK_FQ12_OP_INV, b ignored) on flat arrays of n Fq12 in
 * `mem`; device memory: only enqueues.  The lane-wise mul / inv of multiplicative shares (add.rs:455-479) is exactly this on L n elements.  A zero
 * divisor yields ZERO (the inversion is Fermat's at the bottom of the tower); the reference panics there.
 *
 * Deliberate differences from the reference:
 *   (a) its SPDZ mul / batch_mul of multiplicative shares drop their products (spdz.rs:512-528: the by-value mul results are never assigned); here both
 *       lanes are multiplied, as the additive form does;
 *   (b) pairing() builds the mac of e(xa, y) from the process-global stand-in key (from_add_shared, spdz.rs:486-492); here it is e(xa, mac lane of y),
 *       which needs no key;
 *   (c) with only one operand shared the reference reveals both (pairing.rs:226-228); pair the public point with every lane through czk_pairing
 *       instead -- by bilinearity the lanes are shares of the pairing and nothing is revealed.
 * GSZ pairing shares are commented out in the reference (mpc-algebra/src/lib.rs:56-62) and are not built.
 *
 * n = 0 or parties = 0: CZK_OK, nothing touched but *out_bad.  NULL ctx / out_bad, lpp not 1 or 2, more than 32 parties, an unknown op or mem, NULL
 * vectors with work to do (mac_shares for lpp = 2 included): CZK_ERR_ARG.  More outputs than one launch covers (2^36 threads): CZK_ERR_SIZE.  `out`
 * must not overlap an input.  Workspace: the staging pool (czk_fq12_vec_op from host memory: per-call allocations). */
#define CZK_FQ12_OP_MUL 0
#define CZK_FQ12_OP_DIV 1
#define CZK_FQ12_OP_INV 2
int czk_share_pairing(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* a, const uint8_t* a_inf, const uint64_t* b,
                      const uint8_t* b_inf, const uint64_t* tx, const uint8_t* tx_inf, const uint64_t* ty, const uint8_t* ty_inf, const uint64_t* tz,
                      uint64_t* out, size_t n, uint64_t* out_bad);
int czk_gt_share_open(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* v, size_t n, uint64_t* out, uint64_t* out_bad);
int czk_gt_share_scale(czk_ctx* ctx, size_t lpp, size_t parties, const uint64_t* mac_shares, const uint64_t* v, const uint64_t* f, uint64_t* out, size_t n);
int czk_fq12_vec_op(czk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, int mem);

/* ---- GSZ material made on the device: a keyed generator of field elements, Damgard-Nielsen dealing and extraction, its consistency check ---- */
/* czk_fr_random: a keyed stream of field elements.  Element i comes from the ChaCha20 block (RFC 8439 block function, 20 rounds, 32-bit block counter) at
 * (key, nonce, counter = first + i): lo = bytes 0..31 of the block as a little-endian integer reduced mod 2^252, hi = bytes 32..63 likewise,
 * value = (lo + 2^252 hi) mod r, written as Montgomery limbs to out (n Fr, `mem`).  r lies between 2^252 and 2^253, so both halves are canonical
 * as they stand; the 504-bit sample leaves every residue within r / 2^504 < 2^-251 of uniform (statistical distance below r / 2^504).  The library
 * supplies no entropy: the key is the caller's, and a (key, nonce, counter) triple must never serve twice.  first + n > 2^32 (the counter would
 * wrap): CZK_ERR_SIZE.  n = 0: CZK_OK, nothing touched.  NULL key / nonce / out with work to do: CZK_ERR_ARG.
 *
 * czk_gsz_dn_generate: the preparation gsz20 assumes and the reference stubs out (share/gsz20/mod.rs:383-406 hand every party a one), in the lanes
 * form: all `parties` dealers' keys are on this GPU (ONE process knows every value: a fast dealer, not a secure one).  P = parties, d = degree,
 * w = czk_share_domain_constants' group_gen, draws = 1 + d (CZK_GSZ_DN_RANDS) or 1 + 3 d (CZK_GSZ_DN_DOUBLES).
 *   Dealer i takes element m of its item b from czk_fr_random's stream under keys[i] (32 bytes each) and `nonce` at counter b draws + m: m = 0 is the
 *   secret s, then c_1 .. c_d, then (doubles) e_1 .. e_2d.  Its share for party j is s + sum_k c_k w^(jk), in the second half s + sum_k e_k w^(jk).
 *   Output k deal + b, k = 0 .. P - d - 1, is sum_i w^(ik) (dealer i's item b), share-wise.  outputs = deal (P - d).
 * Row k of the extraction matrix is (w^(ik))_i, so every (P - d)-column minor is a Vandermonde determinant in distinct nodes: the outputs are uniform
 * and unknown to any d dealers as long as the other P - d dealt honestly.  out_r / out_r2 (DEVICE): P lanes, party-major, `outputs` elements apart --
 * the layout of doubles_r / doubles_r2 and of rands in czk_gsz_share_*; out_r2 (the same values under degree 2 d) is NULL for CZK_GSZ_DN_RANDS.
 * tests/gsz_dn_model.py restates the definition; the kernel extracts the coefficients before it evaluates them (fully reduced limbs do not depend on
 * the order).  The call only enqueues.  czk_gsz_dn_counts: the `deal` that yields at least `want` outputs, and that `outputs`.
 * 2 d >= P for doubles, d >= P for random shares, an unknown kind: CZK_ERR_ARG.  deal draws > 2^32, no share domain of that size (0, 5, ...),
 * P > 96: CZK_ERR_SIZE.  deal = 0: CZK_OK, nothing touched.  Workspace: the staging pool (for P other than 3, 4, 6, 8 it grows with the grid).
 *
 * czk_gsz_dn_check: the consistency check, which sacrifices the LAST TWO outputs; the first outputs - 2 are the usable ones.  Output outputs - 2's
 * degree-d half opens at bound d to the coin rho; u = r[outputs - 1] + sum_{m < outputs - 2} rho^(m + 1) r[m] opens at bound d; for doubles the same
 * combination of r2 opens at bound 2 d and the two opened values must be equal.  *out_bad counts the opens that exceeded their bound (0 .. 3);
 * *out_ok = 1 when none did and (doubles) the values were equal, else 0 -- a result, not an error.  A batch with one inconsistent sharing passes with
 * probability at most outputs / r over the coin (a non-zero polynomial of degree < outputs in rho vanishing).  At odd P the bound 2 d = P - 1 is
 * vacuous -- every P values interpolate -- and the equality of the two opened values is what binds the second half.  Dealers that cheat are detected,
 * not tolerated: a failed check says that the batch must be thrown away, not who spoiled it.  The coin stays on the device; counts and verdict are
 * read back once, at the end (the call blocks).  r, r2: as czk_gsz_dn_generate wrote them (r2 ignored for CZK_GSZ_DN_RANDS); not modified.
 * outputs < 3, NULL arguments, the degree rules above: CZK_ERR_ARG; the size rules above, outputs >= 2^32: CZK_ERR_SIZE. */
#define CZK_GSZ_DN_DOUBLES 0   /* the same value under degree d and degree 2 d */
#define CZK_GSZ_DN_RANDS 1     /* degree d only */
int czk_fr_random(czk_ctx* ctx, const uint8_t* key, const uint8_t* nonce, uint32_t first, size_t n, uint64_t* out, int mem);
int czk_gsz_dn_counts(int kind, size_t parties, unsigned degree, size_t want, size_t* deal, size_t* outputs);
int czk_gsz_dn_generate(czk_ctx* ctx, int kind, size_t parties, unsigned degree, const uint8_t* keys, const uint8_t* nonce, size_t deal, uint64_t* out_r,
                        uint64_t* out_r2);
int czk_gsz_dn_check(czk_ctx* ctx, int kind, size_t parties, unsigned degree, const uint64_t* r, const uint64_t* r2, size_t outputs, uint64_t* out_ok,
                     uint64_t* out_bad);

/* The same generation and check with one party per communicator: the party is czk_net_rank(net) of P = czk_net_world(net) parties, deals under its
 * OWN key (32 bytes) alone and holds ONE lane of `outputs` Fr, CZK_MEM_DEVICE on the communicator's context.  No rank learns another's key; `degree`
 * colluding ranks learn nothing about an output as long as the other P - degree dealt honestly; the guarantee is for semi-honest dealing plus the
 * consistency check (a cheating dealer is detected, not tolerated).  The shared-memory transports expose their mailboxes to every process of the node.
 *   czk_net_gsz_dn_generate   the party's draws evaluated at every party's point, [destination][half][b]; ONE czk_net_alltoall of halves deal 32 bytes per
 *                             peer (halves = 2 for doubles); the extraction of this party's lane.  Rank j's out_r / out_r2 are lane j of what
 *                             czk_gsz_dn_generate writes on the same keys (keys[j] = rank j's) and nonce, limb for limb.  Every rank passes the same nonce.
 *   czk_net_gsz_dn_check      the coin and the combinations open through broadcasts of ONE element each: three for doubles, two for random shares.
 *                             *out_ok comes out equal on all ranks, and equal to czk_gsz_dn_check's on the lanes; *out_bad counts the opens (every rank
 *                             checks every bound).
 * Argument rules: those of the lanes form with parties = the world; a communicator without a context: CZK_ERR_ARG. */
int czk_net_gsz_dn_generate(czk_net* net, int kind, unsigned degree, const uint8_t* key, const uint8_t* nonce, size_t deal, uint64_t* out_r, uint64_t* out_r2);
int czk_net_gsz_dn_check(czk_net* net, int kind, unsigned degree, const uint64_t* r, const uint64_t* r2, size_t outputs, uint64_t* out_ok, uint64_t* out_bad);

/* The king's side of king_compute (mpc-algebra/src/channel.rs:77-80; gsz20's degree reduction, share/gsz20/mod.rs:470-500): every
 * party's n Fr to the king, who receives world x n (device, party order) -- czk_net_send_to_king on Fr lanes -- and the way back. */
int czk_fr_send_to_king(czk_net* net, const uint64_t* x, size_t n, uint64_t* gathered);
int czk_fr_recv_from_king(czk_net* net, const uint64_t* parts, size_t n, uint64_t* out);
/* gsz20::batch_king_compute with f = the identity -- the only f the reference passes (share/gsz20/mod.rs:494-527, called at :547,
 * :578, :805: "king just reduces the sharing degree" of a product share x * y + r2): every party's lane to the king, the king opens
 * each element with the degree bound (czk_fr_gsz_open) and sends the opened VALUE back to every party as its new share (:478
 * `vec![output; n]`, "TODO: randomize").  val: n Fr (device); out (n Fr, device; may alias val) = from_king; *out_bad is meaningful
 * on the king (0 elsewhere). */
int czk_gsz_batch_king_compute(czk_net* net, const uint64_t* val, size_t n, const uint32_t* degrees, unsigned degree, uint64_t* out,
                               uint64_t* out_bad);

/* `Vec<Fr>::serialize` / `deserialize` (algebra/serialize/src/lib.rs:220-229 with impl_prime_field_serializer, fields/macros.rs:
 * 532-537): u64 little-endian length, then into_repr() of every element as 32 little-endian bytes.  For a host that still carries
 * some vectors over the reference's own sockets.  serialize: a = n Montgomery Fr (`mem`), out = 8 + 32 n bytes, HOST.  deserialize:
 * bytes / len as received; writes at most cap Fr (Montgomery) to out (`mem`), *n = the length prefix; CZK_ERR_ARG when the prefix
 * does not match len (the reference's deserialize fails) or exceeds cap. */
int czk_fr_vec_serialize(czk_ctx* ctx, const uint64_t* a, size_t n, int mem, uint8_t* out);
int czk_fr_vec_deserialize(czk_ctx* ctx, const uint8_t* bytes, size_t len, uint64_t* out, size_t cap, int mem, size_t* n);
/* SHA-256 (FIPS 180-4) of `len` host bytes: the reference's CommitHash (channel.rs:92).  Exported so a host can reproduce / verify
 * commitments; no context needed. */
void czk_sha256(const void* data, size_t len, uint8_t* out32);

/* ---- callers either side of the NTT: constraint evaluation and division by (X - z) ------------------ */
/* R1CS matrix (one of ConstraintMatrices::{a, b, c}, Vec<Vec<(F, usize)>>) in CSR form, pinned on the GPU once per
 * circuit: row_ptr m+1 offsets (row_ptr[0] = 0, row_ptr[m] = nnz), col_idx nnz variable indices into the full
 * assignment [instance | witness] (r1cs_to_qap.rs:56-61), coeff nnz Montgomery Fr.  CZK_ERR_ARG for a malformed
 * row_ptr or an index >= n_vars (the reference panics on assignment[index]). */
typedef struct czk_r1cs_matrix czk_r1cs_matrix;
int czk_r1cs_matrix_register(czk_ctx* ctx, const uint64_t* row_ptr, const uint32_t* col_idx, const uint64_t* coeff, size_t m,
                             size_t nnz, size_t n_vars, int mem, czk_r1cs_matrix** out);
void czk_r1cs_matrix_release(czk_r1cs_matrix* a);
/* evaluate_constraint over every row (mpc-snarks/src/groth/r1cs_to_qap.rs:12-42, called at :70-77 and :95-100):
 *   out[lane][i] = sum_t coeff[t] * z[lane][col_idx[t]],  i < m
 * z: lanes x z_stride Fr (z_stride >= n_vars), the share lanes of the full assignment with Public entries lifted as for
 * the NTT (wire/field.rs Public * coeff stays public; lifting commutes with the sum); out: lanes x out_stride Fr
 * (out_stride >= m; elements [m, out_stride) are not written, so the caller's zero padding to the domain size stays). */
int czk_r1cs_matvec(czk_ctx* ctx, const czk_r1cs_matrix* a, const uint64_t* z, size_t z_stride, size_t lanes, uint64_t* out,
                    size_t out_stride, int mem);
/* arithmetize_matrix (marlin/src/ahp/constraint_systems.rs:152-262) for one matrix of a squared, balanced R1CS, up to the evaluations on K: the CSR
 * arrays as czk_r1cs_matrix_register takes them (m rows = constraints, col_idx into [instance | witness] with n_instance formatted inputs, coeff
 * Montgomery Fr), H = 2^log_h (the constraint domain), X = 2^log_x (the input domain), k = |K| slots.  out: 4 x k Fr, row | col | val | row_col.
 * For entry t of constraint r at variable i: i' = i for i < n_instance, else i + (X - n_instance) (pad_input_for_indexer_and_prover),
 * p = reindex_by_subdomain(H, X, i'), and with w = get_root_of_unity(H)
 *   row[t] = w^p, col[t] = w^r (the transpose of M, :191-194), val[t] = coeff[t] w^p / |H| (= coeff / u_H(w^p, w^p), :195-204), row_col[t] = row[t] col[t];
 * slots nnz <= t < k hold row = col = row_col = 1, val = 0 (:207-211).  Entries keep their order: the caller sorts each row by column (:183-185).
 * CZK_ERR_SIZE for m > H, k < nnz, log_x > log_h, n_instance > X or log_h > 31.  CZK_MEM_HOST: CZK_ERR_ARG for a malformed row_ptr or an index that
 * has no position on H (>= H - X + n_instance); the call blocks.  CZK_MEM_DEVICE: the call only enqueues on the context's stream and cannot read the
 * arrays, so their contents are the caller's to check; slots of malformed entries are unspecified, and nothing outside the arrays is accessed. */
int czk_marlin_arithmetize(czk_ctx* ctx, const uint64_t* row_ptr, const uint32_t* col_idx, const uint64_t* coeff, size_t m, size_t nnz,
                           unsigned log_h, unsigned log_x, size_t n_instance, size_t k, uint64_t* out, int mem);
/* CircuitLayout::from_circuit (mpc-plonk/src/relations/flat.rs:35-137) up to the evaluation vectors of the two index polynomials, for a circuit of
 * n_gates gates (a power of two) of which the first n_prods are products (:40-46).  W = 3 n_gates wire slots (in0, in1, out per gate), w =
 * get_root_of_unity(W) of the mixed-radix domain (:282-300; the group_gen of czk_mixed_domain_constants(W)).  succ: W slot indices, the wiring
 * permutation -- each slot of a variable names the variable's next slot, the last the first (:75-80).
 *   w_evals[i] = w^succ[i] (W Fr),   s_evals[j] = 0 for j < n_prods, 1 for n_prods <= j < n_gates (n_gates Fr).
 * CZK_ERR_SIZE for n_gates zero or not a power of two, 3 n_gates >= 2^32, a size without a domain, or n_prods > n_gates.  CZK_MEM_HOST: CZK_ERR_ARG
 * unless succ is a permutation of [0, W); the call blocks.  CZK_MEM_DEVICE: the call only enqueues on the context's stream and cannot read succ: a
 * slot with succ[i] >= W gets the value 0 (no domain element), and nothing outside succ[0..W) is accessed whatever it holds. */
int czk_plonk_layout(czk_ctx* ctx, const uint32_t* succ, size_t n_gates, size_t n_prods, uint64_t* w_evals, uint64_t* s_evals, int mem);
/* out[l][i] = src[l][index[i]] for i < n on every lane l < lanes: the step p_evals[i] = vals[var] of flat.rs:91-100 over share lanes (the index
 * array is public, the values are shares).  src: lanes x src_stride Fr of which src_len per lane are valid (src_stride >= src_len); out: lanes x
 * out_stride Fr (out_stride >= n; elements [n, out_stride) of a lane are not written).  n = 0 or lanes = 0: CZK_OK, nothing is touched.
 * CZK_ERR_SIZE for a stride shorter than its lane, src_len = 0 or lanes > 65535.  CZK_MEM_HOST: CZK_ERR_ARG for an index >= src_len; the call
 * blocks.  CZK_MEM_DEVICE: the call only enqueues on the context's stream; an index >= src_len writes 0, and nothing outside the arrays is accessed. */
int czk_fr_gather(czk_ctx* ctx, const uint64_t* src, size_t src_len, size_t src_stride, size_t lanes, const uint32_t* index, size_t n,
                  uint64_t* out, size_t out_stride, int mem);

/* The reference's vector commitment of shared values, ComField (mpc-algebra/src/com.rs), and the fold of its FRI commit phase (mpc-snarks/src/client.rs
 * :739-842), for share lanes that all live on one GPU (merkle.hip).  Linear in the shares: a lane is whatever the caller passes (an additive share, the sh
 * lane of SPDZ, a Shamir evaluation); no call looks at a MAC.  The bytes are the reference's:
 *   bytes(v) = into_repr() as 32 little-endian bytes (czk_fr_vec_serialize's);  leaf_i = SHA256(bytes(a[i]));  node = SHA256(left || right); no tags, no
 *   length prefix.  A TREE of n = 2^k leaves is 2n - 1 digests of 32 bytes (digest order) per lane, level by level: level 0 = the n leaf hashes at digest
 *   offset 0, level 1 at offset n, level L (n >> L digests) at offset 2n - 2 (n >> L), the root at offset 2n - 2.  The reference's Key is these levels
 *   without the root.  A PATH for index i is k digests: tree[level][(i >> level) ^ 1] for level = 0 .. k - 1 (the reference's OpeningProof holds one per
 *   party).  n = 1 is valid: the tree is the one leaf hash and every path is empty.
 * Common rules.  CZK_ERR_SIZE, before any pointer is read: n zero or not a power of two (the fold: n < 2, any other n is taken), stride < n,
 * tree_stride < 2n - 1, a byte count that overflows.  lanes = 0 or q = 0: CZK_OK, nothing is touched.  Device pointers to elements and trees are 16-byte aligned (digests a caller
 * passes as roots or paths: 4-byte).
 * czk_fr_merkle_commit (ComField::commit, com.rs:36-67): a = `lanes` vectors of n Montgomery Fr, `stride` elements apart; tree: lane l at tree + 32 l
 *   tree_stride bytes; roots32: lanes x 32 bytes in HOST memory, or NULL.  Reads a[l][0..n) only and writes digests [0, 2n - 1) of tree[l] only.  With
 *   CZK_MEM_DEVICE and roots32 == NULL the call only enqueues on the context's stream; otherwise it blocks for the roots.
 * czk_fr_merkle_open (open_at, :68-94): idx = q uint64 indices in `mem`; out_shares[query][lane] = a[lane][idx[query]] (q x lanes Montgomery Fr),
 *   out_paths[query][lane][level] (q x lanes x log2 n x 32 bytes) = the path above.  CZK_MEM_HOST: CZK_ERR_ARG for an index >= n; blocks.
 *   CZK_MEM_DEVICE: only enqueues; an index >= n writes zero shares and zero paths and reads nothing outside the arrays.
 * czk_fr_merkle_verify (check_opening, :95-123): roots = lanes x 32 bytes, idx, shares, paths as the open wrote them, values = q Montgomery Fr or NULL,
 *   ok = q bytes, all in `mem`; out_bad: HOST.  Per (query, lane) the share is hashed and walked up its path, bit j of the index putting the sibling left
 *   or right at level j, and the result compared with roots[lane]; per query, with values != NULL, the lanes' shares must sum to values[query] mod r.
 *   ok[query] = 1 or 0 and *out_bad = the number of zeros.  Blocks (the count's read-back).  An index >= n: CZK_ERR_ARG with CZK_MEM_HOST, a bad query
 *   with CZK_MEM_DEVICE.
 * czk_fr_fri_fold (client.rs:767-771): out[l][j] = f[l][2j] + alpha f[l][2j+1] for j < n / 2 (rounded down); elements [n / 2, out_stride) of a lane
 *   are not written.
 *   alpha: one Montgomery Fr in HOST memory.  out may not overlap f (CZK_ERR_ARG where the call can tell).  CZK_MEM_DEVICE: only enqueues. */
int czk_fr_merkle_commit(czk_ctx* ctx, const uint64_t* a, size_t lanes, size_t n, size_t stride, uint8_t* tree, size_t tree_stride, uint8_t* roots32,
                         int mem);
int czk_fr_merkle_open(czk_ctx* ctx, const uint64_t* a, size_t lanes, size_t n, size_t stride, const uint8_t* tree, size_t tree_stride,
                       const uint64_t* idx, size_t q, uint64_t* out_shares, uint8_t* out_paths, int mem);
int czk_fr_merkle_verify(czk_ctx* ctx, const uint8_t* roots, size_t lanes, size_t n, const uint64_t* idx, size_t q, const uint64_t* shares,
                         const uint8_t* paths, const uint64_t* values, uint8_t* ok, size_t* out_bad, int mem);
int czk_fr_fri_fold(czk_ctx* ctx, const uint64_t* f, size_t lanes, size_t n, size_t stride, const uint64_t* alpha, uint64_t* out, size_t out_stride,
                    int mem);
/* czk_fr_fri_fold on DEVICE arrays with alpha_dev a pointer to one Montgomery Fr in DEVICE memory (16-byte aligned), read by the kernel: a challenge that
 * czk_fs_squeeze_fr wrote there and the host never saw.  Only enqueues.  Same rules and the same values as czk_fr_fri_fold with CZK_MEM_DEVICE. */
int czk_fr_fri_fold_at(czk_ctx* ctx, const uint64_t* f, size_t lanes, size_t n, size_t stride, const uint64_t* alpha_dev, uint64_t* out, size_t out_stride);

/* ---- Fiat-Shamir transcripts: the reference's FiatShamirRng<Blake2s> (marlin/src/rng.rs, mpc-plonk/src/util.rs:44-108), fs.hip -----------------------------
 * State: a 32-byte seed and rand_chacha 0.2's ChaChaRng keyed with it (ChaCha20, 64-bit block counter, stream id 0).  from_seed(m): seed = Blake2s(m);
 * absorb(m): seed = Blake2s(m || seed); both reseed the generator and reset its position, counted in 32-bit keystream words.  A message is PUT piece by
 * piece (it streams into the hash) and closed by czk_fs_seed (as from_seed) or czk_fs_absorb (as absorb); an empty message is allowed.
 * ToBytes of what is put: bytes as they are; Fr (Montgomery limbs, as everywhere in this header) as into_repr() in 32 little-endian bytes; an affine point
 * (czk_msm's layout, flags in `inf` or NULL = none infinite) as x || y || infinity byte, Fq = 48 bytes, Fq2 = c0 then c1: 97 bytes for G1, 193 for G2; a
 * flagged point is written as the reference's zero(), x = 0 and y = 1.  No length prefixes (algebra/ff/src/bytes.rs: Vec and slices write their items).
 * Draws: u64 = two keystream words, low first (a u128 is two u64, low first); Fr::rand = four u64 into the limbs low first, the top limb masked with
 * u64::MAX >> 3, the limbs taken AS the Montgomery representation, redrawn until < r.  Fr results are Montgomery limbs.
 * mem at creation: CZK_MEM_HOST = the state lives in host memory, plain C++, ctx may be NULL (a verifier without a GPU); CZK_MEM_DEVICE = the state lives in
 * device memory and every operation is a kernel of one workgroup on the context's stream.  The `mem` of a put or a squeeze says where THAT array lives:
 *   host transcript: CZK_MEM_HOST only (a DEVICE array with work to do: CZK_ERR_ARG).
 *   device transcript, put: HOST data is copied in stream order (the buffer is free on return), DEVICE data is read by the kernel; both only enqueue.
 *     Byte pointers need 1-byte alignment, Fr and point pointers 8-byte.
 *   device transcript, squeeze: DEVICE only enqueues, HOST blocks for the read-back.
 * A squeeze before the first czk_fs_seed, or while the pending message is not empty: CZK_ERR_ARG.  n = 0 / len = 0: CZK_OK, nothing changes.
 * A squeeze_fr gives up after 256 rejected draws of one element (probability 0.42^256), writes zero and sets the state's sticky error word: no device loop
 * is unbounded.  czk_fs_state and every blocking call of a transcript whose word is set return CZK_ERR_CHECK.
 * czk_fs_state: blocking; seed32 (32 bytes) and word_pos in HOST memory, either may be NULL.  For tests and for comparing the two forms.
 * czk_blake2s: BLAKE2s-256 (RFC 7693, no key) of `len` host bytes; czk_fs_keystream: n keystream words of the generator under seed32 from word word_pos on
 * (out[i] = word word_pos + i).  Both are host code and need no context. */
typedef struct czk_fs czk_fs;
void czk_blake2s(const void* data, size_t len, uint8_t* out32);
int czk_fs_keystream(const uint8_t* seed32, uint64_t word_pos, uint32_t* out, size_t n);
int czk_fs_create(czk_ctx* ctx, int mem, czk_fs** out);
void czk_fs_release(czk_fs* fs);
int czk_fs_put_bytes(czk_fs* fs, const void* p, size_t len, int mem);
int czk_fs_put_fr(czk_fs* fs, const uint64_t* v, size_t n, int mem);
int czk_fs_put_points(czk_fs* fs, int group, const uint64_t* pts, const uint8_t* inf, size_t n, int mem);
int czk_fs_seed(czk_fs* fs);
int czk_fs_absorb(czk_fs* fs);
int czk_fs_squeeze_fr(czk_fs* fs, uint64_t* out, size_t n, int mem);
int czk_fs_squeeze_u64(czk_fs* fs, uint64_t* out, size_t n, int mem);
int czk_fs_state(czk_fs* fs, uint8_t* seed32, uint64_t* word_pos);

/* DensePolynomial / (X - z): KZG10::compute_witness_polynomial (poly-commit/src/kzg10/mod.rs:200-224; shares divide
 * lane-wise because the divisor is public, mpc-algebra/src/share/add.rs:148-156).  coeffs: lanes x n Fr, low degree
 * first; quotient: lanes x (n-1) Fr; remainder (may be NULL): lanes Fr = p(z), which is also
 * Polynomial::evaluate (kzg10/mod.rs:247).  z: one Montgomery Fr in HOST memory. */
int czk_poly_div_linear(czk_ctx* ctx, const uint64_t* coeffs, size_t n, size_t lanes, const uint64_t* z, uint64_t* quotient,
                        uint64_t* remainder, int mem);
/* DensePolynomial::evaluate (algebra/poly/src/polynomial/univariate/dense.rs:59-96, Horner) per lane, without the quotient: the
 * evaluations a prover publishes at its challenge points (mpc-plonk/src/lib.rs:273, :360; poly-commit/src/kzg10/mod.rs:246, :525;
 * Marlin's evaluation round).  coeffs: lanes x n Fr, low degree first; values: lanes Fr = p(z); z: one Montgomery Fr in HOST
 * memory.  Same result as czk_poly_div_linear's remainder, at half its memory traffic. */
int czk_poly_evaluate(czk_ctx* ctx, const uint64_t* coeffs, size_t n, size_t lanes, const uint64_t* z, uint64_t* values, int mem);
/* DensePolynomial::divide_by_vanishing_poly (algebra/poly/src/polynomial/univariate/dense.rs:172-179) for the radix-2 / mixed-radix vanishing polynomial
 * X^n - 1, per lane (the divisor is public): a = q (X^n - 1) + r.  coeffs: lanes x m Fr, low degree first, m >= n; quotient: lanes x (m - n) Fr;
 * remainder (may be NULL): lanes x n Fr.  The quotients h of mpc-plonk's gate / product arguments (mpc-plonk/src/lib.rs:190, :332) and Marlin's h_1, h_2
 * (marlin/src/ahp/prover.rs:533, :696); one pass over the coefficients.  (For n of a few units -- Marlin's v_X with |X| = 2 -- the residue classes are long
 * chains: divide them with czk_poly_div_linear at z = 1 instead, as tools/polyvm_host.hpp does.) */
/* czk_poly_evaluate for `count` polynomials in one call, DEVICE memory: polynomial k = n[k] coefficients on lanes[k] lanes at coeffs[k], evaluated at
 * z + 4 k (HOST, Montgomery), its lanes[k] values written to values[k].  One launch per 32-fold reduction level for all of them: Marlin's evaluation round
 * (marlin/src/lib.rs:283-292 through EvaluationsProvider::get_lc_eval, marlin/src/ahp/mod.rs:288-312) evaluates two dozen polynomials at two points,
 * and the upper levels of one evaluation are a few dozen elements -- launch-bound when issued one polynomial at a time. */
int czk_poly_evaluate_many(czk_ctx* ctx, size_t count, const uint64_t* const* coeffs, const size_t* n, const size_t* lanes, const uint64_t* z,
                           uint64_t* const* values);
/* out[l][i] = constant + sum_k coeffs[k] * terms[k][l][i], i < out_len, over `count` <= 12 DEVICE arrays of different lengths (term_len[k] elements per lane; shorter
 * terms end early, longer ones are cut at out_len), coeffs: count x 4 u64, HOST, Montgomery; constant: one Fr, HOST, Montgomery, or NULL (zero).  A term has
 * `lanes` lanes (term_lanes[k] == lanes) or is PUBLIC (term_lanes[k] == 1): a public term -- and the constant, which is public -- is added on the lanes whose
 * bit is set in `lift_mask` only -- the rule by which the reference adds a public
 * value to a shared one (AdditiveFieldShare::shift, mpc-algebra/src/share/add.rs:141-146: the king; GszFieldShare: every party).  One pass: the linear
 * combinations of polynomials a prover forms -- `poly += (*coeff, cur_poly.polynomial())` per term (poly-commit/src/marlin/mod.rs:275; the batch opening's
 * fold, marlin_pc/mod.rs:259-316; marlin/src/ahp/prover.rs:468-476) -- where a scale / resize / add chain makes a pass over memory per call. */
int czk_fr_lincomb(czk_ctx* ctx, size_t count, const uint64_t* const* terms, const size_t* term_len, const size_t* term_lanes, const uint64_t* coeffs,
                   const uint64_t* constant, size_t lanes, uint64_t lift_mask, uint64_t* out, size_t out_len);
int czk_poly_div_vanishing(czk_ctx* ctx, const uint64_t* coeffs, size_t m, size_t lanes, size_t n, uint64_t* quotient, uint64_t* remainder, int mem);

/* out[i] = x[0] * x[1] * ... * x[i] over a PUBLIC vector: the sequential loop of partial_products between its
 * batch_open and the final scale (mpc-algebra/src/share/field.rs:169-172; Plonk's grand product).  The share-side
 * scale that follows (:177-179) is czk_fr_vec_op(CZK_OP_MUL) per lane.  out may alias x only in HOST mode. */
int czk_fr_prefix_product(czk_ctx* ctx, const uint64_t* x, size_t n, uint64_t* out, int mem);

/* batch_inversion_and_mul (algebra/ff/src/fields/mod.rs:616-677): out[i] = coeff * v[i]^-1, zero elements stay zero
 * (the reference skips them, :651, :666).  coeff: one Montgomery Fr in HOST memory, NULL = one (batch_inversion, :616).
 * In device memory out must not alias v. */
int czk_fr_batch_inverse(czk_ctx* ctx, const uint64_t* v, size_t n, const uint64_t* coeff, uint64_t* out, int mem);

/* Fr::into_repr / from_repr over a vector (fields/arithmetic.rs:59-81, macros.rs:443-454) -- also the wire format.  out may alias a
 * (conversion in place); any other overlap of the two is not allowed. */
int czk_fr_into_repr(czk_ctx* ctx, const uint64_t* a, uint64_t* out, size_t n, int mem);
int czk_fr_from_repr(czk_ctx* ctx, const uint64_t* a, uint64_t* out, size_t n, int mem);

/* ---- MSM ---------------------------------------------------------------------------------------- */
/* Pin a public base array (a proving-key query) on the GPU once; it is reused across proofs
 * (groth16/src/data_structures.rs:132-149).  bases: n x (12|24) u64 affine Montgomery; inf: n bytes (may be NULL =
 * no infinity points). */
int czk_bases_register(czk_ctx* ctx, int group, const uint64_t* bases, const uint8_t* inf, size_t n, int mem,
                       czk_bases** out);
void czk_bases_release(czk_bases* b);
size_t czk_bases_len(const czk_bases* b);
/* Pippenger layout chosen at registration (reporting only): *c = signed-digit window width, *windows = ceil(254 / c) =
 * mixed additions per (point, lane) of an MSM over this array.  Where c * windows overshoots the 254 bits by `slack` bits and the top window
 * would be narrower than 10 bits (widths chosen for fewer than 2^14 points), the last `slack` windows are c - 1 bits wide instead, so that
 * no window is narrow and no bucket collects more than twice the average (csrc/czk_internal.h: msm_full_windows). */
int czk_bases_layout(const czk_bases* b, unsigned* c, unsigned* windows);
/* Window width per CALL.  The reference derives c from the size of each MSM (variable_base.rs:21-25); a precomputed table fixes
 * it per key, so a short MSM under a long key (KZG10::commit of a low-degree polynomial under `powers_of_g`,
 * poly-commit/src/kzg10/mod.rs:159-162) would reduce the key's 2^(c-1) buckets on every call.  MSMs that use a short prefix of
 * the array therefore run on a second table set at a narrower width (c = 13 / 15 / 17 by size, covering the next power of two of
 * the call), built on first use and kept with the handle; czk_bases_prepare builds the set for calls of `n_scalars` scalars up
 * front (e.g. at SRS load), czk_bases_layout_for reports the (c, windows) such a call runs with.  Handles registered with
 * CZK_MEM_NO_TABLES choose c per call outright. */
int czk_bases_layout_for(const czk_bases* b, size_t n_scalars, unsigned* c, unsigned* windows);
/* Bucket arithmetic the handle's MSMs run with (reporting only): 0 = XYZZ, saturated limbs; 1 = XYZZ, unsaturated limbs (8M + 2S per mixed
 * addition); 2 = twisted Edwards extended coordinates, unsaturated limbs (G1 in the prime-order subgroup: 7M per mixed addition). */
int czk_bases_arith(const czk_bases* b);
int czk_bases_prepare(czk_ctx* ctx, const czk_bases* b, size_t n_scalars);

/* Replaces VariableBaseMSM::multi_scalar_mul (algebra/ec/src/msm/variable_base.rs:12-106) / AffineCurve::
 * multi_scalar_mul (ec/src/lib.rs:300-311) as reached from MpcG{1,2}Affine::multi_scalar_mul
 * (mpc-algebra/src/wire/pairing.rs:746-809) -> GroupShare::multi_scale_pub_group (share/spdz.rs:440-446).
 * scalars: lanes x n_scalars x 4 u64 (lane-major); `lanes` scalar vectors share the bases (SPDZ: sh and mac).
 * size = min(czk_bases_len, n_scalars) pairs are used (variable_base.rs:16; h has D scalars vs D-1 bases).
 * out_jac: lanes x (18|36) u64 Jacobian, Montgomery, HOST memory.  Jacobian triples are not canonical: compare in
 * affine (czk_jac_to_affine), as the reference's own MSM test does (algebra/test-templates/src/msm.rs:16-33). */
int czk_msm(czk_ctx* ctx, const czk_bases* bases, const uint64_t* scalars, size_t n_scalars, size_t lanes,
            int scalar_form, int mem, uint64_t* out_jac);

/* Same, but only enqueues: consecutive calls overlap on the context's internal streams (sort / accumulate / reduce
 * stages of neighbouring MSMs run concurrently).  `out_jac` (host) is valid after the next czk_ctx_sync(), or after czk_ctx_wait_mark on a
 * mark taken after this call.  Device
 * scalars may be overwritten by later work on the context's stream (the library orders that itself). */
int czk_msm_async(czk_ctx* ctx, const czk_bases* bases, const uint64_t* scalars, size_t n_scalars, size_t lanes,
                  int scalar_form, int mem, uint64_t* out_jac);

/* One-shot forms with the reference's argument order (bases not kept on the GPU).  These are VariableBaseMSM::multi_scalar_mul's
 * signature, which is complete on every curve point, so they make NO subgroup assumption: the bases are registered with
 * CZK_MEM_NO_TABLES | CZK_MEM_ANY_POINTS for the call (G1: XYZZ bucket arithmetic with the reference's case analysis). */
int czk_msm_g1(czk_ctx* ctx, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n,
               size_t lanes, int scalar_form, uint64_t* out_jac);
int czk_msm_g2(czk_ctx* ctx, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n,
               size_t lanes, int scalar_form, uint64_t* out_jac);

/* GroupAffine::is_in_correct_subgroup_assuming_on_curve (short_weierstrass_jacobian.rs:131: `self.mul(r).is_zero()`) over the
 * registered bases, on the GPU: *out_bad = number of bases that are not on the curve or not annihilated by r (points at infinity
 * pass).  0 means the default (twisted Edwards) G1 arithmetic is exact for this handle.  Blocking.  For a handle registered with
 * CZK_MEM_CHECK_SUBGROUP the stored result of the registration-time check is returned. */
int czk_bases_check_subgroup(czk_ctx* ctx, const czk_bases* bases, size_t* out_bad);

/* From<GroupProjective> for GroupAffine (short_weierstrass_jacobian.rs:768-789): n host Jacobian points ->
 * n host affine points + infinity flags.  This is what AffineMsm::msm's `.into()` does (share/msm.rs:31-37).
 * Host-side arithmetic (one inversion per point); `ctx` may be NULL. */
int czk_jac_to_affine(czk_ctx* ctx, int group, const uint64_t* jac, size_t n, uint64_t* out_aff, uint8_t* out_inf);

/* GroupProjective += (add_assign, short_weierstrass_jacobian.rs:666-728) and += affine (add_assign_mixed, :570-638) on
 * host Jacobian values: the O(1) group steps around the MSMs (calculate_coeff, prover.rs:216-232; KZG10::commit's
 * `commitment.add_assign_mixed(&random_commitment)`, poly-commit/src/kzg10/mod.rs:188).  Host arithmetic; ctx may be NULL. */
int czk_jac_add(czk_ctx* ctx, int group, const uint64_t* a_jac, const uint64_t* b_jac, uint64_t* out_jac);
int czk_jac_add_mixed(czk_ctx* ctx, int group, const uint64_t* a_jac, const uint64_t* b_aff, int b_inf, uint64_t* out_jac);
/* ProjectiveCurve::mul / scalar_mul (algebra/ec/src/lib.rs:215-230: double-and-add over the scalar's bits, most significant first) and Neg
 * (short_weierstrass_jacobian.rs:737-748: (x, -y, z)) on host Jacobian values: `pk.delta_g1.scalar_mul(r)`, `g_a.scalar_mul(&s)`,
 * `g_c -= &r_s_delta_g1` of create_proof (mpc-snarks/src/groth/prover.rs:113-165).  k: one Fr, HOST memory, `scalar_form` as for the MSM.
 * Host arithmetic (about a millisecond per G1 multiplication); ctx may be NULL. */
int czk_jac_scalar_mul(czk_ctx* ctx, int group, const uint64_t* a_jac, const uint64_t* k, int scalar_form, uint64_t* out_jac);
int czk_jac_neg(czk_ctx* ctx, int group, const uint64_t* a_jac, uint64_t* out_jac);

/* Synthetic public bases P_i = [k_i] * generator for i < n, k_i = canonical scalars (n x 4 u64), written as
 * affine Montgomery points to `out` (device or host).  Stands in for a trusted-setup run when benchmarking
 * (SURVEY.md section 8d); also how tests obtain on-curve points with known discrete logs. */
int czk_fixed_base_points(czk_ctx* ctx, int group, const uint64_t* k, size_t n, uint64_t* out, int mem);

/* ---- fixed-base MSM: the generator's side (groth16/src/generator.rs:106-187) ---------------------- */
/* FixedBaseMSM::get_window_table (algebra/ec/src/msm/fixed_base.rs:20-58) for ONE finite affine base (HOST memory, 12|24 u64 Montgomery; a base
 * written as the point at infinity -- x = 0 with y = 0 or 1 -- is CZK_ERR_ARG), built on the context's GPU and kept in HBM until
 * czk_fixed_base_release.  The base may be ANY finite point of the curve: like the reference's windowed_mul (:60-80) the multiplication makes no
 * subgroup assumption.  window = 1..20 forces the width; window = 0 lets the library choose it for n_hint scalars (n_hint = 0: not known): the
 * width with the fewest group additions, table build included, whose table stays below 1 GiB -- not the reference's get_mul_window_size
 * (msm/mod.rs:10-13); the affine results do not depend on it.  Digits are signed: 2^(window - 1) entries per window.
 * czk_fixed_base_layout (reporting only): *window, *windows = ceil(253 / window), plus one where window divides 253 (the signed form's carry can
 * leave the top window there), *table_bytes = HBM the table occupies. */
typedef struct czk_fixed_base czk_fixed_base;
int czk_fixed_base_create(czk_ctx* ctx, int group, const uint64_t* base_aff, unsigned window, size_t n_hint, czk_fixed_base** out);
void czk_fixed_base_release(czk_fixed_base* fb);
int czk_fixed_base_layout(const czk_fixed_base* fb, unsigned* window, unsigned* windows, size_t* table_bytes);
/* FixedBaseMSM::multi_scalar_mul (fixed_base.rs:82-95) + batch_normalization_into_affine (short_weierstrass_jacobian.rs:480-500):
 * out_aff[i] = [k_i] base for i < n, one mixed addition per window.  scalars: n x 4 u64 in `scalar_form` (Montgomery scalars are decoded on the
 * GPU); bits at and above 253 are ignored (fixed_base.rs:72).  out_aff: n x (12|24) u64 affine Montgomery; out_inf: n infinity bytes, may be
 * NULL; k_i = 0 (mod the base's order) gives flag 1 and the coordinates (0, 1).  Buffers follow `mem`; with CZK_MEM_DEVICE the call only
 * enqueues.  n = 0 is CZK_OK and writes nothing. */
int czk_fixed_base_msm(czk_ctx* ctx, const czk_fixed_base* fb, const uint64_t* scalars, size_t n, int scalar_form, uint64_t* out_aff,
                       uint8_t* out_inf, int mem);
/* EvaluationDomain::evaluate_all_lagrange_coefficients (algebra/poly/src/domain/radix2/mod.rs:119-185) over the radix-2 domain of 2^log_d
 * elements: out[j] = L_j(tau) for j < n_out <= 2^log_d (Montgomery Fr; `mem`).  tau: one Montgomery Fr, HOST memory.  Includes the branch for
 * tau inside the domain (:136-150: the coefficient of the element tau equals is one, every other zero).  CZK_ERR_SIZE beyond 2^47. */
int czk_fr_lagrange_coefficients(czk_ctx* ctx, unsigned log_d, const uint64_t* tau, uint64_t* out, size_t n_out, int mem);

/* ---- Groth16 per-party local compute (callers of the two kernels) -------------------------------- */
/* R1CStoQAP::witness_map minus its communication step (mpc-snarks/src/groth/r1cs_to_qap.rs:47-113), on `lanes`
 * Fr lanes of D = 2^log_d elements, all buffers lanes x D x 4 u64 in DEVICE memory:
 *   czk_witness_map_pre : a <- coset_fft(ifft(a)), b <- coset_fft(ifft(b))                       (:85-89)
 *   [caller: ab = batch_product(a, b) -- Beaver opens for shares, czk_fr_vec_op(MUL) for a single prover] (:92)
 *   czk_witness_map_post: c <- coset_fft(ifft(c)); ab <- coset_ifft((ab - c) * Z(g)^-1)          (:102-110)
 *   czk_witness_map_post_h: the same ab for a caller that needs h alone: c <- ifft(c); ab <- (coset_ifft(ab) - c) * Z(g)^-1 -- the same field elements
 *     (transforms are linear and coset_ifft undoes coset_fft), with c transformed once instead of twice; `c` is scratch afterwards
 *   czk_witness_map_pre_masked: a <- coset_fft(ifft(a)) + mask_a, b <- coset_fft(ifft(b)) + mask_b -- what a Beaver product needs of a and b
 *     (share/field.rs:103-104); masks: lanes x D canonical Fr, not overlapping a or b
 * h = ab on return.  a_len / b_len / c_len <= D: evaluations present in each lane (num_constraints + num_inputs for a,
 * num_constraints for b and c); elements beyond them are the reference's `vec![zero; domain_size]` padding (:66-67, :94)
 * and are never read -- the first NTT pass zero-extends. */
int czk_witness_map_pre(czk_ctx* ctx, uint64_t* a, size_t a_len, uint64_t* b, size_t b_len, unsigned log_d, size_t lanes);
int czk_witness_map_pre_masked(czk_ctx* ctx, uint64_t* a, size_t a_len, uint64_t* b, size_t b_len, const uint64_t* mask_a, const uint64_t* mask_b, unsigned log_d,
                               size_t lanes);
int czk_witness_map_post(czk_ctx* ctx, uint64_t* ab, uint64_t* c, size_t c_len, unsigned log_d, size_t lanes);
int czk_witness_map_post_h(czk_ctx* ctx, uint64_t* ab, uint64_t* c, size_t c_len, unsigned log_d, size_t lanes);

/* ---- square roots and the reference's byte format of curve points -------------------------------- */
/* SquareRootField::sqrt over Fq (ext = 1: n x 6 u64) or Fq2 (ext = 2: n x 12 u64), Montgomery form, one thread per element.
 * out_exists[i] = 1 and out[i] = a root of a[i], or out_exists[i] = 0 and out[i] = 0 when a[i] has none.  The root of 0 is 0 and exists.
 * ROOT CHOICE: of the two roots, the y with y <= -y in the reference's order (Fq by into_repr(); Fq2 by c1, then c0:
 * quadratic_extension.rs:412-418).  This DIFFERS from SquareRootField::sqrt, which returns whichever root its Tonelli-Shanks loop lands on
 * (ff/src/fields/arithmetic.rs:259-320); no serialization path observes that choice (get_point_from_x normalises it,
 * short_weierstrass_jacobian.rs:108-118).  Fq2 elements with c1 = 0 and c0 a non-residue of Fq have the root (0, sqrt(c0 / -5)) here; the
 * reference's Fq2 sqrt answers None for them (quadratic_extension.rs:363-365).  Buffers follow `mem`; with CZK_MEM_DEVICE the call only enqueues. */
int czk_fq_sqrt(czk_ctx* ctx, int ext, const uint64_t* a, size_t n, uint64_t* out, uint8_t* out_exists, int mem);

/* CanonicalSerialize / CanonicalDeserialize for GroupAffine (short_weierstrass_jacobian.rs:792-895): n affine Montgomery points + infinity
 * bytes <-> the reference's bytes.  Per point: G1 48 (compressed) / 96 bytes, G2 96 / 192 bytes; each Fq is the 48 little-endian bytes of
 * into_repr(), an Fq2 is c0 then c1; SWFlags (serialize/src/flags.rs:110-135) sit in the top two bits of the point's LAST byte: bit 7 =
 * PositiveY (y > -y; compressed finite points only), bit 6 = Infinity.  Byte buffers in DEVICE memory must be 8-byte aligned (CZK_ERR_ARG).
 *
 * czk_points_serialize: serialize (compressed != 0) or serialize_uncompressed.  inf: n bytes, NULL = none infinite; a point flagged infinite
 *   is written as GroupAffine::zero() whatever its coordinates hold: x = 0 with the infinity bit, or (0, 1) with the bit on y.
 * czk_points_deserialize: flags = CZK_POINTS_COMPRESSED and / or CZK_POINTS_CHECKED --
 *     COMPRESSED | CHECKED = deserialize, CHECKED = deserialize_uncompressed, 0 = deserialize_unchecked, COMPRESSED alone = get_point_from_x
 *     without the subgroup test (the reference has no such entry point).
 *   Per point, in this order: both flag bits set -> CZK_POINT_BAD_FLAGS; a coordinate >= q (a flag bit on any Fq but the last included) ->
 *   CZK_POINT_NOT_CANONICAL; the infinity bit -> infinity, written as flag 1 with the coordinates (0, 1) (uncompressed input too, where the
 *   reference keeps the coordinates it read); compressed: y^2 = x^3 + b has no root -> CZK_POINT_NO_POINT, else y by the PositiveY bit;
 *   uncompressed: (x, y) as read, bit 7 ignored.  CHECKED then tests [r] P == 0 -> CZK_POINT_NOT_IN_SUBGROUP, and for uncompressed input
 *   first y^2 == x^3 + b -> CZK_POINT_NOT_ON_CURVE.  That on-curve test is STRICTER than the reference, whose deserialize_uncompressed
 *   assumes it (is_in_correct_subgroup_assuming_on_curve).  Without CHECKED uncompressed points get no test at all, as in the reference.
 *   A failing point gets flag 0 and zero coordinates; the others are unaffected (the reference fails the whole read with InvalidData).
 *   out_status: n bytes of czk_point_status, follows `mem`, may be NULL.  out_bad / out_first_bad: HOST size_t, each may be NULL: the number
 *   of failing points and the smallest failing index (n when none fails).  With CZK_MEM_DEVICE and both NULL the call only enqueues.
 * n = 0 is CZK_OK. */
typedef enum { CZK_POINTS_COMPRESSED = 1, CZK_POINTS_CHECKED = 2 } czk_points_flags;
typedef enum {
    CZK_POINT_OK = 0,
    CZK_POINT_BAD_FLAGS = 1,
    CZK_POINT_NOT_CANONICAL = 2,
    CZK_POINT_NO_POINT = 3,
    CZK_POINT_NOT_ON_CURVE = 4,
    CZK_POINT_NOT_IN_SUBGROUP = 5
} czk_point_status;
int czk_points_serialize(czk_ctx* ctx, int group, const uint64_t* pts, const uint8_t* inf, size_t n, int compressed, uint8_t* out_bytes, int mem);
int czk_points_deserialize(czk_ctx* ctx, int group, const uint8_t* bytes, size_t n, int flags, uint64_t* out_pts, uint8_t* out_inf,
                           uint8_t* out_status, size_t* out_bad, size_t* out_first_bad, int mem);

/* ---- pairing and Groth16 verification ------------------------------------------------------------ */
/* The reference's pairing engine Bls12::<Parameters> (X = 0x8508c00000000001, TwistType::D; curves/bls12_377/src/curves/mod.rs:16-19,
 * algebra/ec/src/models/bls12/mod.rs) on the GPU, one product of pairings per thread.  Points are affine Montgomery (G1: 12 u64, G2: 24 u64)
 * plus infinity flags (NULL = none infinite); a pair with infinity on either side is skipped, as in miller_loop (mod.rs:99-103).
 * GT elements: Fq12 = 72 u64 in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1 (Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - u)),
 * each Fq 6 Montgomery limbs: bit for bit the reference's value.  No subgroup checks are made on any point.  All calls block.
 *
 * czk_pairing: PairingEngine::pairing (algebra/ec/src/lib.rs:111) of n independent pairs; out: n x 72 u64.
 * czk_pairing_product: PairingEngine::product_of_pairings (lib.rs:102) of k products, product j over pairs [offsets[j], offsets[j+1]) of the
 *   offsets[k] inputs; offsets (k + 1 entries, offsets[0] == 0, non-decreasing) are HOST memory whatever `mem` says.  out (k x 72) and
 *   out_is_one (k flags: the product is one) may each be NULL.  An empty product is one.
 * Buffers follow `mem` (CZK_MEM_HOST or CZK_MEM_DEVICE). */
int czk_pairing(czk_ctx* ctx, const uint64_t* g1, const uint8_t* g1_inf, const uint64_t* g2, const uint8_t* g2_inf, size_t n, uint64_t* out, int mem);
int czk_pairing_product(czk_ctx* ctx, const uint64_t* g1, const uint8_t* g1_inf, const uint64_t* g2, const uint8_t* g2_inf, const size_t* offsets,
                        size_t k, uint64_t* out, uint8_t* out_is_one, int mem);

/* prepare_verifying_key (groth16/src/verifier.rs:12-20) into device memory of the context's GPU: e(alpha, beta), -gamma and -delta
 * prepared (G2Prepared, g2.rs:69-97), gamma_abc_g1.  Inputs are HOST memory: alpha (12 u64), beta / gamma / delta (24 u64 each, finite
 * points), gamma_abc_g1 (n_gamma_abc x 12 u64, flags NULL = none infinite; n_gamma_abc >= 1).  The handle stays valid until
 * czk_groth16_pvk_release and may be used by any context of the same device. */
typedef struct czk_groth16_pvk czk_groth16_pvk;
int czk_groth16_pvk_create(czk_ctx* ctx, const uint64_t* alpha_g1, const uint64_t* beta_g2, const uint64_t* gamma_g2, const uint64_t* delta_g2,
                           const uint64_t* gamma_abc_g1, const uint8_t* gamma_abc_inf, size_t n_gamma_abc, czk_groth16_pvk** out);
void czk_groth16_pvk_release(czk_groth16_pvk* pvk);
/* verify_proof (verifier.rs:23-58) over k proofs: out_ok[j] = 1 iff e(A, B) e(g_ic, -gamma) e(C, -delta) == e(alpha, beta) with
 * g_ic = gamma_abc[0] + sum_i x_i gamma_abc[i + 1] -- one Miller loop over the three pairs and one final exponentiation per proof (the
 * same decision as the reference's three pairings: the final exponentiation is a homomorphism).  a: k x 12, b: k x 24, c: k x 12 u64;
 * inf: k x 3 flags (A, B, C; NULL = none infinite); public_inputs: k x m x 4 u64, Montgomery Fr (as E::Fr).  m + 1 != n_gamma_abc is
 * CZK_ERR_ARG "MalformedVerifyingKey" (verifier.rs:28-30).  As in verify_proof, the proof's points get NO subgroup or on-curve check.
 * Buffers follow `mem`. */
int czk_groth16_verify(czk_ctx* ctx, const czk_groth16_pvk* pvk, const uint64_t* a, const uint64_t* b, const uint64_t* c, const uint8_t* inf,
                       const uint64_t* public_inputs, size_t m, size_t k, uint8_t* out_ok, int mem);

/* ---- elementwise group arithmetic on arrays of points --------------------------------------------- */
/* The O(n) group steps of a verifier, on the GPU (the host calls czk_jac_add / czk_jac_scalar_mul above take one point at a time).  Points are
 * affine Montgomery (G1: 12 u64, G2: 24 u64) plus infinity bytes (input flags NULL = none infinite); results are normalised to affine with one
 * shared batch inversion per call (batch_normalization_into_affine, short_weierstrass_jacobian.rs:480-500): infinity is flag 1 with the
 * coordinates (0, 1); out_inf may be NULL.  NO subgroup assumption: every point of the curve is a valid input -- (0, 1) with flag 0 is the
 * order-3 point, not infinity.  Buffers follow `mem`; with CZK_MEM_DEVICE a call only enqueues.  n = 0 (k = 0) is CZK_OK and writes nothing.
 *
 * czk_points_add: out[i] = a[i] + b[i], or a[i] - b[i] with negate_b != 0 -- add_assign_mixed with its whole case analysis (:570-638): either side
 *   infinite, a = b (doubling), a = -b (infinity).  out may alias a or b.
 * czk_points_mul: out[i] = [k_i] P_i, ProjectiveCurve::mul (algebra/ec/src/lib.rs:215-230): double-and-add over ALL 256 bits of the canonical
 *   scalar, most significant first (a scalar >= r is not reduced first: the points need not have order r).  scalars: n x 4 u64 in `scalar_form`
 *   (Montgomery scalars are decoded on the GPU).  pts_stride = 1: n points and flags; pts_stride = 0: ONE point (and flag) for every scalar.
 * czk_points_sum: k segmented sums, out[j] = sum of pts[offsets[j] .. offsets[j+1]); an empty segment is infinity.  offsets (k + 1 entries,
 *   offsets[0] == 0, non-decreasing) are HOST memory whatever `mem` says and are read before the call returns.  One wave per segment, the lanes'
 *   partial sums combined by the complete addition (:666-728): equal and opposite partial sums are handled. */
int czk_points_add(czk_ctx* ctx, int group, const uint64_t* a, const uint8_t* a_inf, const uint64_t* b, const uint8_t* b_inf, size_t n, int negate_b,
                   uint64_t* out, uint8_t* out_inf, int mem);
int czk_points_mul(czk_ctx* ctx, int group, const uint64_t* pts, const uint8_t* inf, size_t pts_stride, const uint64_t* scalars, size_t n,
                   int scalar_form, uint64_t* out, uint8_t* out_inf, int mem);
int czk_points_sum(czk_ctx* ctx, int group, const uint64_t* pts, const uint8_t* inf, const size_t* offsets, size_t k, uint64_t* out, uint8_t* out_inf,
                   int mem);

/* ---- KZG10 verification (poly-commit/src/kzg10/mod.rs:295-371) ------------------------------------- */
/* VerifierKey (poly-commit/src/kzg10/data_structures.rs:173-190) into device memory of the context's GPU: g, gamma_g (G1, 12 u64 each), h, beta_h
 * (G2, 24 u64 each), HOST memory, finite points.  The handle stays valid until czk_kzg10_vk_release and may be used by any context of the same
 * device. */
typedef struct czk_kzg10_vk czk_kzg10_vk;
int czk_kzg10_vk_create(czk_ctx* ctx, const uint64_t* g, const uint64_t* gamma_g, const uint64_t* h, const uint64_t* beta_h, czk_kzg10_vk** out);
void czk_kzg10_vk_release(czk_kzg10_vk* vk);
/* KZG10::check (mod.rs:295-314) over k independent openings: out_ok[i] = 1 iff e(C_i - [v_i] g - [rv_i] gamma_g, h) * e(-W_i, beta_h - [z_i] h)
 * is one -- the same decision as the reference's lhs == rhs (the final exponentiation is a homomorphism), one Miller loop over two pairs and one
 * final exponentiation per opening.  comm, w: k x 12 u64 with flags (NULL = none infinite); points, values: k x 4 u64 Montgomery Fr; random_v:
 * k x 4 Montgomery Fr, NULL = no opening is hiding (Proof::random_v = None; a zero entry decides the same as None).  As in the reference no point
 * gets a subgroup or on-curve check; a pair with infinity on either side is skipped (z = beta, the zero polynomial).  Buffers follow `mem`; blocks. */
int czk_kzg10_check(czk_ctx* ctx, const czk_kzg10_vk* vk, const uint64_t* comm, const uint8_t* comm_inf, const uint64_t* points, const uint64_t* values,
                    const uint64_t* w, const uint8_t* w_inf, const uint64_t* random_v, size_t k, uint8_t* out_ok, int mem);
/* KZG10::batch_check (mod.rs:318-371) over b batches: batch j covers openings [offsets[j], offsets[j+1]) of the same per-opening arrays, and
 * out_ok[j] = 1 iff e(-total_w, beta_h) * e(total_c, h) is one, with total_c = sum r_i (C_i + [z_i] W_i) - [sum r_i v_i] g - [sum r_i rv_i] gamma_g
 * and total_w = sum r_i W_i.  randomizers: one per opening, n x 4 u64 CANONICAL, supplied by the caller (the reference uses 1 for a batch's first
 * opening and 128-bit random values after it).  offsets (b + 1 entries, offsets[0] == 0, non-decreasing): HOST memory.  An empty batch is ok. */
int czk_kzg10_batch_check(czk_ctx* ctx, const czk_kzg10_vk* vk, const uint64_t* comm, const uint8_t* comm_inf, const uint64_t* points,
                          const uint64_t* values, const uint64_t* w, const uint8_t* w_inf, const uint64_t* random_v, const uint64_t* randomizers,
                          const size_t* offsets, size_t b, uint8_t* out_ok, int mem);

/* ---- measurement hooks --------------------------------------------------------------------------- */
/* When enabled, the library brackets its kernel launches with HIP events on the context's stream (the stream the
 * kernels run on) and accumulates per-kernel elapsed time.  Names: "msm_accumulate_g1", "msm_accumulate_g2",
 * "msm_sort", "msm_reduce", "ntt_pass", "pointwise".  czk_profile_read synchronises the stream. */
int czk_profile_enable(czk_ctx* ctx, int on);
int czk_profile_reset(czk_ctx* ctx);
int czk_profile_read(czk_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches);
/* The same brackets as intervals: (start, stop) of every bracket of `kernel` in milliseconds after the context's profile origin (an
 * event czk_profile_reset records on the context's stream).  Writes at most `cap` pairs, *n = the number available.  Summed elapsed
 * times of brackets on different streams overlap; the UNION of the intervals is the time a kernel of that name was running -- what
 * bench.py reports as accumulate-busy time.  czk_profile_base_offset: origin of `b` minus origin of `a` (same device), to merge the
 * intervals of several contexts onto one clock. */
int czk_profile_intervals(czk_ctx* ctx, const char* kernel, double* start_ms, double* stop_ms, size_t cap, size_t* n);
int czk_profile_base_offset(czk_ctx* a, czk_ctx* b, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* CZK_H */
