// msm.hip -- variable-base multi-scalar multiplication over BLS12-377 G1 / G2 for gfx950.
//
// Replaces VariableBaseMSM::multi_scalar_mul (algebra/ec/src/msm/variable_base.rs:12-106) and
// AffineCurve::multi_scalar_mul (algebra/ec/src/lib.rs:300-311) as reached from the MPC wrappers
// (mpc-algebra/src/wire/pairing.rs:746-809, share/spdz.rs:440-446).  The result is the same group element
// sum_i s_i * P_i; Jacobian representatives differ from the reference's (they are not canonical), so parity is
// checked in affine form, as the reference's own MSM test does (algebra/test-templates/src/msm.rs:16-33).
//
// MI355X-first design -- NOT the reference's serial "for each window: fill 2^c-1 buckets, running-sum them,
// then Horner over windows with c doublings":
//   * HBM capacity is traded for arithmetic.  The bases are public and reused across proofs
//     (groth16/src/data_structures.rs:132-149), so registration (msm_bases.hip) stores 2^(c*w) * P_i for every window w
//     (W x the table; ~9 GB for a 2^20-constraint Groth16 key, out of 288 GB).  Every (scalar, window)
//     digit then lands in ONE shared bucket set: a single bucket reduction per MSM and no window-combine
//     doubling chain (256 dependent doublings in the reference) at all.
//   * signed digits: 2^(c-1) buckets of weight 1..2^(c-1); a negative digit adds -P (y -> p - y).
//   * digits are counting-sorted by bucket (msm_sort.hip), then one thread owns one bucket and folds its points with the mixed addition (same edge cases
//     as short_weierstrass_jacobian.rs:570-597) -- no atomics or locks on group elements; buckets are visited in descending-population order so the 64 lanes
//     of a wave do equal work; a bucket with more than 1024 entries is cut into work items (msm_acc.h, over-full buckets).
//   * buckets live in XYZZ coordinates (curve.h): mixed addition 8M + 2S instead of 7M + 4S, addition 12M + 2S
//     instead of 11M + 5S; one conversion back to the reference's Jacobian triple per result.
//   * bucket reduction sum_b (b+1) * B_b: multi-level chunked running sums (the reference's :82-86 running
//     sum, applied per chunk, with the chunk offsets folded in at the next level) down to 1024 entries per lane,
//     then bit-sum tree reductions (msm_acc.h k_reduce_tail_*).
//   * consecutive MSMs pipeline over three internal streams (msm_enqueue below).
//   * `lanes` scalar vectors that share the bases (SPDZ sh / mac lanes) ride on gridDim.y.
//   * bases registered WITHOUT tables (CZK_MEM_NO_TABLES; one-shot callers): the W digit windows of a lane become W virtual lanes
//     of the same kernels, one bucket set each, and the per-window results are combined on the host (msm_enqueue, b->split).
// All arithmetic is 32-bit-limb integer VALU (field.h); nothing here is MFMA-shaped.
// This file is the pipeline: plan, workspaces, the three stages and their events, results, marks.  Keys, window tables and window widths: msm_bases.hip.
#include <string.h>

#include "czk_internal.h"

namespace czk {

// Everything a call decides before it touches a stream (msm_plan), the options included: the stages branch on these fields.  The head is the sort's view of
// the call (MsmSortDims): size = pairs that count (variable_base.rs:16), lanes = bucket sets = gridDim.y of every kernel after the digits.
struct MsmPlan : MsmSortDims {
    const czk_bases* b;
    MsmRedDims red;                  // the bucket / reduction workspace (czk_internal.h)
    size_t need_sort, need_red, need_aff, aff_scratch, out_bytes;
    int lean;                        // "msm_reduce_lean" as this call found it (twisted Edwards reduction kernels, msm_acc.h)
    int ub;                          // buckets stay in u-form through the reduction (b->te: twisted Edwards tables and buckets, te.h; b->unsat: u-form tables)
    bool g1, stable, same, key_valid, may_reuse, any_inf, drop_wait;
    AffArgs aff;                     // lab, batched-affine rounds (rounds != 0): the sizes
};
// The arrays of one call, carved from the workspaces of its slot (the sort's: of the slot whose sorted entries it reads) -- msm_carve.
struct MsmBufs : MsmRedBufs {
    MsmSortBufs sort;
    char* pinned;                    // host staging of the result
    AffArgs aff;
};

static int msm_plan(czk_ctx* ctx, const czk_bases* b, const u64* scalars, size_t n_scalars, size_t lanes, int form, bool stable, bool same, MsmPlan& p) {
    p.b = b;
    p.scalars = scalars;
    p.n_scalars = n_scalars;
    p.form = form;
    p.stable = stable;
    p.same = same;
    p.g1 = b->group == CZK_G1;
    p.size = b->n < n_scalars ? b->n : n_scalars;
    CZK_TRY(pick_tables(ctx, b, p.size, &p.tv, true));
    // no tables (b->split): the width follows the call, every digit window is a lane of its own with one bucket set (see the head of the file)
    p.nb = p.tv.cover;
    // (the long-call partition rule: not under the lab's batched-affine record builders, whose partitions are 1024 buckets)
    const unsigned c = b->split ? msm_width_for(b, p.size) : p.tv.c;
    msm_sort_dims(p, c, b->split ? msm_num_windows(c) : p.tv.W, b->split, lanes, ctx->msm_affine_rounds == 0, ctx->msm_sort_onepass, ctx->lds_per_block);
    if (p.lanes > 65535) return set_err(ctx, CZK_ERR_SIZE, "too many MSM lanes");
    if ((size_t)p.W * p.nb >= ((size_t)1 << 31)) return set_err(ctx, CZK_ERR_SIZE, "W * n_bases exceeds the 31-bit point index");
    p.need_sort = msm_sort_bytes(p);
    msm_red_dims(p.red, p.g1, p.lanes, p.B, p.total);
    p.need_red = msm_red_bytes(p.red);
    p.out_bytes = p.lanes * p.red.JW * 8;
    p.lean = ctx->msm_reduce_lean;
    p.ub = 1;   // product build: every key's tables are in the unsaturated residue system, buckets stay in u-form through the reduction
#ifdef CZK_LAB
    // G1 buckets stay in u-form through the reduction (k_reduce_*_u) unless the batched-affine rounds (which finish on saturated level points) or
    // "msm_reduce_sat" ask for the saturated form
    const bool aff_on = ctx->msm_affine_rounds > 0 && p.size > 0;
    p.ub = (p.b->te || (p.b->unsat && !(p.g1 ? ctx->msm_reduce_sat || aff_on : ctx->msm_reduce_sat || ctx->msm_reduce_sat_g2))) ? 1 : 0;
    if (p.g1 && p.b->unsat && !p.b->te && aff_on) {   // batched-affine pre-reduction (G1, unsaturated tables): records, two level arrays, per-level bucket offsets / counts
        AffArgs& a = p.aff = AffArgs{ctx->msm_affine_rounds, (unsigned)p.lanes, p.one_pass ? 0 : p.n_parts, p.part_shift, PART_LOG, p.B, p.total};
        aff_plan(p.total, p.B, a.rounds, a.S);
        p.aff_scratch = aff_scratch_bytes(ctx);
        for (unsigned r = 0; r < a.rounds; r++) p.need_aff += p.lanes * a.S[r] * (8 + 1) + 512;
        p.need_aff += p.lanes * a.S[0] * 128 + (a.rounds > 1 ? p.lanes * a.S[1] * 128 : 0) + 4 * p.lanes * p.B * 4 + p.aff_scratch + (1 << 16);
    }
#endif
    // CZK_MEM_SAME_SCALARS: an earlier call's digit sort stands for this one when nothing that enters it differs (msm_sort_source).  Only sorts over the
    // primary table set of a key with tables are kept for that; the lab's batched-affine rounds and broken schedule never share one.
    p.key_valid = stable && !p.split && p.tv.pts == b->pts;
    p.may_reuse = same && p.key_valid && ctx->msm_sort_reuse && !p.aff.rounds && !ctx->chaos_drop_wait;
    p.any_inf = ctx->msm_sort_reuse_any_inf;
    p.drop_wait = ctx->chaos_drop_wait != 0;   // (msm_affine_rounds, chaos_drop_wait and msm_sort_reuse_any_inf have setters in the lab build only: defaults here otherwise)
    return CZK_OK;
}

// Workspaces are grow-only.  Growing drains the pipeline and calls hipMalloc (a device-wide synchronisation): EVERY slot of the ring grows to the new size
// at once, so that a prover whose MSMs differ in size (KZG commitments of many lengths) stalls once per new maximum, not once per slot.
static int msm_grow(czk_ctx* ctx, const MsmSlot& slot, const MsmPlan& p) {
    if (slot.ws_sort.bytes >= p.need_sort && slot.ws_red.bytes >= p.need_red && slot.ws_aff.bytes >= p.need_aff) return CZK_OK;
    CZK_TRY(msm_pipeline_sync(ctx));
    for (int i = 0; i < ctx->msm_slots_in_use; i++) {
        MsmSlot& sl = ctx->msm_slots[i];
        CZK_TRY(ensure_buf(ctx, sl.ws_sort, p.need_sort));
        CZK_TRY(ensure_buf(ctx, sl.ws_red, p.need_red));
        if (p.need_aff) CZK_TRY(ensure_buf(ctx, sl.ws_aff, p.need_aff));
    }
    return CZK_OK;
}

// `slot`: the call's own (buckets, reduction, batched-affine arrays); `src`: the slot whose sort workspace holds the call's entries.  The order and the
// alignment of the sort arrays are fixed by the sizes alone: a later call that shares the sort computes the same offsets into `src`.
static void msm_carve(const MsmPlan& p, const MsmSlot& slot, const MsmSlot& src, MsmBufs& w) {
    const size_t lanes = p.lanes, B = p.B;
    MsmSortBufs& s = w.sort;
    msm_sort_carve(p, (char*)src.ws_sort.p, s);
    msm_red_carve(p.red, (char*)slot.ws_red.p, w);
    AffArgs& a = w.aff = p.aff;
    if (a.rounds) {   // (lab)
        Bump ba{(char*)slot.ws_aff.p};
        for (unsigned r = 0; r < a.rounds; r++) {
            a.rec[r] = ba.take<u64>(lanes * a.S[r]);
            a.pend[r] = ba.take<uint8_t>(lanes * a.S[r]);
        }
        a.lvl[0] = ba.take<char>(lanes * a.S[0] * 128);
        a.lvl[1] = a.rounds > 1 ? ba.take<char>(lanes * a.S[1] * 128) : nullptr;
        for (int k = 0; k < 2; k++) {
            a.off[k] = ba.take<u32>(lanes * B);
            a.cnt[k] = ba.take<u32>(lanes * B);
        }
        a.scratch = ba.take<char>(p.aff_scratch);
        a.sorted = s.sorted;
        a.offsets = s.offsets;
        a.counts = s.counts;
    }
}

// two keys of one length and window layout drop the same digits: the same table entries (window w, point i) are infinity
static bool same_infinities(const czk_bases* x, const czk_bases* y) {
    if (x == y) return true;
    return x->inf_listed && y->inf_listed && x->n == y->n && x->c == y->c && x->W == y->W && x->inf_idx == y->inf_idx;
}

// CZK_MEM_SAME_SCALARS: the slot of an earlier call whose digit sort stands for this one -- nothing that enters the sort differs: scalars, their form, the
// window layout, the table stride (entries are table indices) and the digits dropped for points at infinity.  The entries stay in THAT call's slot; this call
// takes its own slot for the buckets and the reduction as always.  -1: the call sorts into its own slot, whose key is filled in for later calls.
static int msm_sort_source(czk_ctx* ctx, MsmSlot& slot, const MsmPlan& p) {
    const uint64_t seq = ++ctx->msm_seq;
    if (!p.same) ctx->msm_leader_seq = seq;
    for (int i = 0; p.may_reuse && i < ctx->msm_slots_in_use; i++) {
        const MsmSortKey& k = ctx->msm_slots[i].key;
        if (k.valid && k.seq >= ctx->msm_leader_seq && k.scalars == (const void*)p.scalars && k.n_scalars == p.n_scalars && k.lanes == p.lanes && k.size == p.size &&
            k.nb == p.nb && k.form == p.form && k.c == p.c && k.W == p.W && (p.any_inf || same_infinities(k.bases, p.b)))
            return i;
    }
    // NOTE: the key is valid from here on, before its sort is enqueued, and keeps the raw `bases` pointer (open review findings; kept as they were)
    slot.key = MsmSortKey{p.key_valid, seq, p.scalars, p.n_scalars, p.lanes, p.size, p.nb, p.form, p.c, p.W, p.b};
    return -1;
}

static int msm_stage_sort(czk_ctx* ctx, MsmSlot& slot, bool reuse, const MsmPlan& p, const MsmBufs& w) {
    hipStream_t ss = ctx->s_sort;
    CZK_HIP(ctx, hipEventRecord(ctx->ev_in, ctx->stream));
    CZK_HIP(ctx, hipStreamWaitEvent(ss, ctx->ev_in, 0));                                   // S1
    if (slot.used) CZK_HIP(ctx, hipStreamWaitEvent(ss, slot.ev_fix, 0));                   // S2
    if (p.drop_wait && slot.used) CZK_HIP(ctx, hipStreamWaitEvent(ss, slot.ev_acc, 0));    // S2'
    {
        ProfScope ps(ctx, reuse ? "msm_sort_reused" : "msm_sort", ss);
        if (!reuse) CZK_HIP(ctx, msm_sort_enqueue(ss, p, w.sort));
#ifdef CZK_LAB
        if (w.aff.rounds) launch_affine_build_g1(ss, w.aff);
#endif
        if (p.b->unsat && !p.b->te) {   // clear the dirty flags / exception list here rather than on the accumulate stream (the critical one)
            if (slot.used) CZK_HIP(ctx, hipStreamWaitEvent(ss, slot.ev_red, 0));           // S3
            (p.g1 ? launch_accumulate_g1_u_prepare : launch_accumulate_g2_u_prepare)(ss, w.dirty, p.B, (unsigned)p.lanes);
        }
    }
    CZK_HIP(ctx, hipEventRecord(slot.ev_sorted, ss));
    if (!p.stable) CZK_HIP(ctx, hipStreamWaitEvent(ctx->stream, slot.ev_sorted, 0));       // C1
    return CZK_OK;
}

static MsmStageArgs stage_args(const MsmPlan& p, const MsmBufs& w) {
    return MsmStageArgs{p.g1, p.b->te, p.b->unsat, p.ub, p.lean, (unsigned)p.lanes, p.B, p.total, p.tv.pts, p.red.heavy_cap, &w.aff};
}

// (the unsaturated and twisted Edwards launchers bracket their main kernel with the "msm_accumulate_g{1,2}" profiling scope themselves)
int msm_accumulate_enqueue(czk_ctx* ctx, hipStream_t sa, const MsmStageArgs& a, const MsmSortBufs& s, const MsmRedBufs& w) {
    const unsigned lanes = a.lanes;
    if (a.te) launch_accumulate_g1_te(ctx, sa, a.pts, s.sorted, s.offsets, s.counts, s.perm, a.B, a.total, w.buckets, lanes);
#ifdef CZK_LAB
    else if (a.aff && a.aff->rounds) launch_affine_accumulate_g1(ctx, sa, *a.aff, a.pts, s.perm, w.buckets, w.dirty);
    else if (!a.unsat) {   // saturated tables ("msm_sat"): the round-1 kernels
        ProfScope ps(ctx, a.g1 ? "msm_accumulate_g1" : "msm_accumulate_g2", sa);
        (a.g1 ? launch_accumulate_g1 : launch_accumulate_g2)(sa, a.pts, s.sorted, s.offsets, s.counts, s.perm, a.B, a.total, w.buckets, lanes);
    }
#else
    else if (!a.unsat) return set_err(ctx, CZK_ERR_ARG, "bases with saturated window tables: not part of the product build");
#endif
    else (a.g1 ? launch_accumulate_g1_u : launch_accumulate_g2_u)(ctx, sa, a.pts, s.sorted, s.offsets, s.counts, s.perm, a.B, a.total, w.buckets, lanes, w.dirty, a.ub);
    return CZK_OK;
}
static int msm_stage_accumulate(czk_ctx* ctx, MsmSlot& slot, const MsmPlan& p, const MsmBufs& w) {
    hipStream_t sa = ctx->s_acc;
    CZK_HIP(ctx, hipStreamWaitEvent(sa, slot.ev_sorted, 0));                               // A1
    if (slot.used) CZK_HIP(ctx, hipStreamWaitEvent(sa, slot.ev_red, 0));                   // A2
    ctx->msm_launch_split = p.split;
    CZK_TRY(msm_accumulate_enqueue(ctx, sa, stage_args(p, w), w.sort, w));
    CZK_HIP(ctx, hipGetLastError());
    CZK_HIP(ctx, hipEventRecord(slot.ev_acc, sa));
    return CZK_OK;
}

static void launch_reduce_level(hipStream_t sr, const MsmStageArgs& a, const u64* P, const u64* E, size_t n_in, unsigned scale_dbl, u64* Po, u64* Eo, size_t n_out) {
    if (!a.g1) launch_reduce_level_g2(sr, P, E, n_in, MSM_L, scale_dbl, Po, Eo, n_out, a.lanes, a.ub);
    else if (a.ub) launch_reduce_level_g1_u(sr, P, E, n_in, MSM_L, scale_dbl, Po, Eo, n_out, a.lanes, a.te, a.lean);
#ifdef CZK_LAB
    else launch_reduce_level_g1(sr, P, E, n_in, MSM_L, scale_dbl, Po, Eo, n_out, a.lanes);
#endif
}
// the end of the reduction, n_in <= 1024 entries per lane: latency-bound from here, so bit-sum tree reductions instead of more levels (one entry: a conversion)
static void launch_reduce_end(hipStream_t sr, const MsmStageArgs& a, const MsmRedBufs& w, const u64* P, const u64* E, size_t n_in, unsigned scale_dbl) {
    const unsigned lanes = a.lanes;
    if (!a.g1) n_in > 1 ? launch_reduce_tail_g2(sr, P, E, n_in, scale_dbl, w.tail_scratch, w.tail_sums, w.result, lanes, a.ub) : launch_finish_g2(sr, P, E, lanes, w.result, a.ub);
    else if (a.ub) n_in > 1 ? launch_reduce_tail_g1_u(sr, P, E, n_in, scale_dbl, w.tail_scratch, w.tail_sums, w.result, lanes, a.te, a.lean) : launch_finish_g1_u(sr, P, E, lanes, w.result, a.te);
#ifdef CZK_LAB
    else n_in > 1 ? launch_reduce_tail_g1(sr, P, E, n_in, scale_dbl, w.tail_scratch, w.tail_sums, w.result, lanes) : launch_finish_g1(sr, P, E, lanes, w.result);
#endif
}
// work items beyond the first 1024 entries of over-full buckets (none with uniformly random scalars), then the dirty buckets / deferred points of the
// unsaturated kernels (normally none): on the reduce stream, so the accumulate stream goes straight on
void msm_fixup_enqueue(hipStream_t sr, const MsmStageArgs& a, const MsmSortBufs& s, const MsmRedBufs& w) {
    const unsigned lanes = a.lanes;
    if (a.te) launch_heavy_g1_te(sr, a.pts, s.sorted, s.offsets, s.counts, a.B, a.total, w.buckets, lanes, w.heavy_hdr, w.heavy_items, w.heavy_list, w.heavy_partials, a.heavy_cap);
    else (a.g1 ? launch_heavy_g1 : launch_heavy_g2)(sr, a.pts, s.sorted, s.offsets, s.counts, a.B, a.total, w.buckets, lanes, a.unsat ? w.dirty : nullptr, w.heavy_hdr,
                                                    w.heavy_items, w.heavy_list, w.heavy_partials, a.heavy_cap, a.unsat ? 1 : 0, a.ub);
    if (a.unsat && !a.te) {
#ifdef CZK_LAB
        if (a.aff && a.aff->rounds) launch_accumulate_g1_u_fixup_lvl(sr, a.pts, s.sorted, s.offsets, s.counts, a.B, a.total, w.buckets, lanes, w.dirty, a.aff->lvl[(a.aff->rounds - 1) & 1]);
        else
#endif
        (a.g1 ? launch_accumulate_g1_u_fixup : launch_accumulate_g2_u_fixup)(sr, a.pts, s.sorted, s.offsets, s.counts, a.B, a.total, w.buckets, lanes, w.dirty, a.ub);
    }
}
void msm_reduce_enqueue(hipStream_t sr, const MsmStageArgs& a, const MsmRedBufs& w) {
    const u64 *P = w.buckets, *E = nullptr;
    size_t n_in = a.B;
    unsigned level = 0;
    for (; n_in > 1024; level++) {   // chunked running sums: MSM_L entries per chunk, the chunk offsets folded in at the next level
        const size_t n_out = (n_in + MSM_L - 1) / MSM_L;
        u64 *Po = w.lv[(level & 1) * 2], *Eo = w.lv[(level & 1) * 2 + 1];
        launch_reduce_level(sr, a, P, E, n_in, level * MSM_LOG_L, Po, Eo, n_out);
        P = Po;
        E = Eo;
        n_in = n_out;
    }
    launch_reduce_end(sr, a, w, P, E, n_in, level * MSM_LOG_L);
}
// `borrowed`: the slot whose sort this call read, when it is not its own
static int msm_stage_reduce(czk_ctx* ctx, MsmSlot& slot, MsmSlot* borrowed, const MsmPlan& p, const MsmBufs& w) {
    hipStream_t sr = ctx->s_red;
    CZK_HIP(ctx, hipStreamWaitEvent(sr, p.drop_wait ? slot.ev_sorted : slot.ev_acc, 0));   // R1 (R1': the broken schedule)
    const MsmStageArgs a = stage_args(p, w);
    msm_fixup_enqueue(sr, a, w.sort, w);
    CZK_HIP(ctx, hipEventRecord(slot.ev_fix, sr));
    if (borrowed) CZK_HIP(ctx, hipEventRecord(borrowed->ev_fix, sr));
    {
        ProfScope ps(ctx, "msm_reduce", sr);
        msm_reduce_enqueue(sr, a, w);
    }
    CZK_HIP(ctx, hipGetLastError());
    chaos_point(ctx, sr);
    CZK_HIP(ctx, hipMemcpyAsync(w.pinned, w.result, p.out_bytes, hipMemcpyDeviceToHost, sr));
    CZK_HIP(ctx, hipEventRecord(slot.ev_red, sr));
    slot.used = true;
    return CZK_OK;
}

// Enqueue one MSM on the context's three-stage pipeline:
//   s_sort : digits -> partition -> per-partition sort -> population order; flag clearing  (memory bound)
//   s_acc  : the bucket accumulation kernel, nothing else                            (integer-VALU bound, fills the chip)
//   s_red  : over-full-bucket items, fix-up kernels, bucket reduction, result copy   (mostly latency bound)
// Consecutive MSMs overlap stage-wise (sort of k+1 and reduce of k-1 hide under accumulate of k); a ring of workspace slots is guarded by events.
// Results land in a pinned staging area and are handed to the caller's buffer by msm_pipeline_sync / ctx_wait_mark.
//
// Event schedule of a call in slot S.  It records ev_in (caller's stream), S.ev_sorted (s_sort), S.ev_acc (s_acc), S.ev_fix and S.ev_red (s_red) once each, in
// that order; "if S.used": an earlier call ran in S, and until this call records them S's events stand for that one.
//   S1  s_sort waits ev_in                   the scalars are produced on the caller's stream
//   S2  s_sort waits S.ev_fix    if S.used   S's sort arrays are read by the earlier call's accumulate, over-full-bucket and fix-up kernels
//   S2' s_sort waits S.ev_acc    if S.used, broken schedule only: ev_fix no longer implies ev_acc there, and the sort arrays stay protected
//   S3  s_sort waits S.ev_red    if S.used, before the dirty flags are cleared (u-form XYZZ keys): they live in S's reduce workspace
//   C1  caller's stream waits S.ev_sorted    unless CZK_MEM_STABLE: the scalars may be overwritten once the digits are extracted
//   A1  s_acc waits S.ev_sorted              entries, counts, offsets, order; cleared flags
//   A2  s_acc waits S.ev_red     if S.used   S's buckets are read by the earlier call's reduction
//   R1  s_red waits S.ev_acc                 the buckets are complete
//   R1' s_red waits S.ev_sorted  INSTEAD of R1 under lab "chaos_drop_wait" (tests/test_chaos.py): the reduction folds stale or half-written buckets -- wrong results,
//       which the harness must notice -- while the lists, counts and offsets it reads are complete.  (Dropping A1 instead lets kernels read another call's
//       buffer layout as counts and indices: memory faults and minute-long loops.)
// S.ev_fix follows the fix-up: S's sort arrays are free from there.  A call that reads the sort of another slot R (CZK_MEM_SAME_SCALARS) enqueues no sort (s_sort
// is in order: R's entries are complete before anything recorded on it from here), makes the same waits and records R.ev_fix too: the next sort into R waits for
// the LATEST record, which covers R's own accumulate and fix-up (s_red is in order).  S.ev_red follows the result copy.  Lab "chaos" hands out the slots in
// random order: any slot is valid, its events order the reuse.
static int msm_enqueue(czk_ctx* ctx, const czk_bases* b, const u64* scalars, size_t n_scalars, size_t lanes, int form, u64* out_host, bool scalars_stable,
                       bool same_scalars) {
    MsmPlan p{};
    CZK_TRY(msm_plan(ctx, b, scalars, n_scalars, lanes, form, scalars_stable, same_scalars, p));
    CZK_TRY(msm_pipeline_init(ctx));
#ifdef CZK_LAB
    if (ctx->chaos) ctx->msm_next_slot = (int)(chaos_rand(ctx) % (unsigned)ctx->msm_slots_in_use);
#endif
    MsmSlot& slot = ctx->msm_slots[ctx->msm_next_slot];
    ctx->msm_next_slot = (ctx->msm_next_slot + 1) % ctx->msm_slots_in_use;
    CZK_TRY(msm_grow(ctx, slot, p));
    const int src_idx = msm_sort_source(ctx, slot, p);
    MsmSlot& src = src_idx >= 0 ? ctx->msm_slots[src_idx] : slot;
    MsmBufs w;
    msm_carve(p, slot, src, w);
    CZK_TRY(msm_pinned_take(ctx, p.out_bytes, &w.pinned));
    CZK_TRY(msm_stage_sort(ctx, slot, src_idx >= 0, p, w));
    CZK_TRY(msm_stage_accumulate(ctx, slot, p, w));
    CZK_TRY(msm_stage_reduce(ctx, slot, &src != &slot ? &src : nullptr, p, w));
    ctx->msm_pending.push_back(MsmPending{w.pinned, out_host, p.out_bytes, false, p.split ? p.Wd : 0, p.c, b->group, p.real_lanes});   // (split: combined at delivery)
    return CZK_OK;
}

int msm_pipeline_init(czk_ctx* ctx) {
    if (ctx->s_sort) return CZK_OK;
    // (stream priorities for the short sort / reduce stages were measured: no gain, so all three are equal)
    if (ctx->msm_stream_prio) {   // option "msm_stream_priority": 1 = sort / reduce streams above the accumulate stream, 2 = the reverse
        int least = 0, greatest = 0;
        CZK_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        const bool rev = ctx->msm_stream_prio == 2;
        CZK_HIP(ctx, hipStreamCreateWithPriority(&ctx->s_sort, hipStreamNonBlocking, rev ? least : greatest));
        CZK_HIP(ctx, hipStreamCreateWithPriority(&ctx->s_acc, hipStreamNonBlocking, rev ? greatest : least));
        CZK_HIP(ctx, hipStreamCreateWithPriority(&ctx->s_red, hipStreamNonBlocking, rev ? least : greatest));
    } else {
        CZK_HIP(ctx, hipStreamCreateWithFlags(&ctx->s_sort, hipStreamNonBlocking));
        CZK_HIP(ctx, hipStreamCreateWithFlags(&ctx->s_acc, hipStreamNonBlocking));
        CZK_HIP(ctx, hipStreamCreateWithFlags(&ctx->s_red, hipStreamNonBlocking));
    }
    CZK_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming));
    for (auto& s : ctx->msm_slots) {
        CZK_HIP(ctx, hipEventCreateWithFlags(&s.ev_sorted, hipEventDisableTiming));
        CZK_HIP(ctx, hipEventCreateWithFlags(&s.ev_acc, hipEventDisableTiming));
        CZK_HIP(ctx, hipEventCreateWithFlags(&s.ev_fix, hipEventDisableTiming));
        CZK_HIP(ctx, hipEventCreateWithFlags(&s.ev_red, hipEventDisableTiming));
    }
    ctx->msm_pinned_bytes = 4 << 20;
    CZK_HIP(ctx, hipHostMalloc((void**)&ctx->msm_pinned, ctx->msm_pinned_bytes, hipHostMallocDefault));
    return CZK_OK;
}

static void deliver(const MsmPending& p) {
    if (p.split_W) host_combine_windows(p.group, p.src, p.split_W, p.c, p.lanes, (uint64_t*)p.dst);
    else memcpy(p.dst, p.src, p.bytes);
}
static void retire_mark(czk_ctx* ctx, CtxMark& m) {
    ctx->mark_events.push_back(m.ev_stream);
    ctx->mark_events.push_back(m.ev_red);
}

// wait for every enqueued MSM and deliver the results (and those of deferred downloads: their copies run on the context's stream)
int msm_pipeline_sync(czk_ctx* ctx) {
    if (!ctx->s_sort) return CZK_OK;
    for (auto& p : ctx->msm_pending)
        if (p.on_stream) {
            CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            break;
        }
    CZK_HIP(ctx, hipStreamSynchronize(ctx->s_sort));
    CZK_HIP(ctx, hipStreamSynchronize(ctx->s_acc));
    CZK_HIP(ctx, hipStreamSynchronize(ctx->s_red));
    for (auto& p : ctx->msm_pending) deliver(p);
    for (auto& sl : ctx->msm_slots) sl.key.valid = false;   // CZK_MEM_STABLE promises the scalars up to here
    ctx->msm_delivered += ctx->msm_pending.size();
    ctx->msm_pending.clear();
    ctx->msm_pinned_used = 0;
    // NOTE: ctx->stream is synchronised above only when a deferred download is pending, yet every mark is retired (an open review finding; kept as it was)
    for (auto& m : ctx->marks) retire_mark(ctx, m);
    ctx->marks.clear();
    return CZK_OK;
}

// Staging for one host result: a ring over the pinned area.  Results are delivered oldest first, so the free space runs from the tail (`used`) round to
// the oldest pending result; when a request does not fit, everything pending is drained (a full synchronisation -- 4 MiB hold > 10^4 MSM results).
int msm_pinned_take(czk_ctx* ctx, size_t bytes, char** out) {
    CZK_TRY(msm_pipeline_init(ctx));
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (need > ctx->msm_pinned_bytes) return set_err(ctx, CZK_ERR_SIZE, "host result larger than the result staging area");
    if (ctx->msm_pending.empty()) ctx->msm_pinned_used = 0;
    else {
        const size_t head = (size_t)(ctx->msm_pending.front().src - ctx->msm_pinned), tail = ctx->msm_pinned_used;
        bool fits;
        if (tail > head) {                         // [head, tail) in use
            fits = tail + need <= ctx->msm_pinned_bytes;
            if (!fits && need <= head) {           // wrap: [0, head) is free
                ctx->msm_pinned_used = 0;
                fits = true;
            }
        } else fits = tail + need <= head;         // wrapped: [tail, head) is free (tail == head with results pending: full)
        if (!fits) {
            CZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            CZK_TRY(msm_pipeline_sync(ctx));
        }
    }
    *out = ctx->msm_pinned + ctx->msm_pinned_used;
    ctx->msm_pinned_used += need;
    return CZK_OK;
}

// ---- marks (include/czk.h: czk_ctx_mark / czk_ctx_wait_mark / czk_lanes_download_deferred) -------------------------------------------
static hipEvent_t mark_event(czk_ctx* ctx) {
    if (!ctx->mark_events.empty()) {
        hipEvent_t e = ctx->mark_events.back();
        ctx->mark_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    return e;
}
int ctx_mark(czk_ctx* ctx, uint64_t* out) {
    CZK_TRY(msm_pipeline_init(ctx));
    CtxMark m;
    m.id = ctx->next_mark++;
    m.ev_stream = mark_event(ctx);
    m.ev_red = mark_event(ctx);
    if (!m.ev_stream || !m.ev_red) return set_err(ctx, CZK_ERR_HIP, "czk_ctx_mark: no event");
    CZK_HIP(ctx, hipEventRecord(m.ev_stream, ctx->stream));
    CZK_HIP(ctx, hipEventRecord(m.ev_red, ctx->s_red));   // every MSM enqueued so far ends with its result copy on this stream, in order
    m.upto = ctx->msm_delivered + ctx->msm_pending.size();
    ctx->marks.push_back(m);
    *out = m.id;
    return CZK_OK;
}
int ctx_wait_mark(czk_ctx* ctx, uint64_t id) {
    if (id == 0 || id >= ctx->next_mark) return set_err(ctx, CZK_ERR_ARG, "czk_ctx_wait_mark: not a mark of this context");
    for (auto& sl : ctx->msm_slots) sl.key.valid = false;   // a transcript point: what follows is another round's (or another proof's) work
    while (!ctx->marks.empty() && ctx->marks.front().id <= id) {   // older marks first: a mark covers the ones before it
        CtxMark m = ctx->marks.front();
        CZK_HIP(ctx, hipEventSynchronize(m.ev_stream));
        CZK_HIP(ctx, hipEventSynchronize(m.ev_red));
        size_t k = 0;
        while (k < ctx->msm_pending.size() && ctx->msm_delivered + k < m.upto) deliver(ctx->msm_pending[k++]);
        ctx->msm_pending.erase(ctx->msm_pending.begin(), ctx->msm_pending.begin() + k);
        ctx->msm_delivered += k;
        retire_mark(ctx, m);
        ctx->marks.erase(ctx->marks.begin());
    }
    return CZK_OK;   // (a mark retired earlier -- by a later mark's wait or by czk_ctx_sync -- has nothing left to wait for)
}

void msm_pipeline_destroy(czk_ctx* ctx) {
    if (!ctx->s_sort) return;
    // drain the streams, but do NOT deliver pending czk_msm_async results: the caller's `out_jac` buffers may be gone by
    // now (an exception between msm_async and sync, then garbage collection in any order); results are only ever
    // delivered by an explicit czk_ctx_sync / czk_msm
    (void)hipStreamSynchronize(ctx->s_sort);
    (void)hipStreamSynchronize(ctx->s_acc);
    (void)hipStreamSynchronize(ctx->s_red);
    ctx->msm_pending.clear();
    for (auto& m : ctx->marks) retire_mark(ctx, m);
    ctx->marks.clear();
    for (hipEvent_t e : ctx->mark_events) (void)hipEventDestroy(e);
    ctx->mark_events.clear();
    for (auto& s : ctx->msm_slots) {
        if (s.ws_sort.p) (void)hipFree(s.ws_sort.p);
        if (s.ws_red.p) (void)hipFree(s.ws_red.p);
        if (s.ws_aff.p) (void)hipFree(s.ws_aff.p);
        (void)hipEventDestroy(s.ev_sorted);
        (void)hipEventDestroy(s.ev_acc);
        (void)hipEventDestroy(s.ev_fix);
        (void)hipEventDestroy(s.ev_red);
    }
    (void)hipEventDestroy(ctx->ev_in);
    (void)hipHostFree(ctx->msm_pinned);
    (void)hipStreamDestroy(ctx->s_sort);
    (void)hipStreamDestroy(ctx->s_acc);
    (void)hipStreamDestroy(ctx->s_red);
    ctx->s_sort = nullptr;
}

// czk_ctx_reserve: table set chosen (and built), streams created, every workspace of the ring sized
int msm_reserve(czk_ctx* ctx, const czk_bases* bases, size_t n_scalars, size_t lanes) {
    MsmPlan p{};
    CZK_TRY(msm_plan(ctx, bases, nullptr, n_scalars, lanes, CZK_SCALAR_CANONICAL, false, false, p));
    CZK_TRY(msm_pipeline_init(ctx));
    return msm_grow(ctx, ctx->msm_slots[ctx->msm_next_slot], p);
}

int msm_device(czk_ctx* ctx, const czk_bases* bases, const u64* scalars_dev, size_t n_scalars, size_t lanes, int scalar_form,
               u64* out_jac_host, bool blocking, bool scalars_stable, bool same_scalars) {
    int rc = msm_enqueue(ctx, bases, scalars_dev, n_scalars, lanes, scalar_form, out_jac_host, scalars_stable, same_scalars);
    if (rc != CZK_OK || !blocking) return rc;
    return msm_pipeline_sync(ctx);
}

}  // namespace czk

using namespace czk;

// ------------------------------------------------------------------------------------------------
// C ABI (MSM part)
// ------------------------------------------------------------------------------------------------
static int msm_common(czk_ctx* ctx, const czk_bases* bases, const uint64_t* scalars, size_t n_scalars, size_t lanes, int scalar_form, int mem,
                      uint64_t* out_jac, bool blocking) {
    if (!ctx || !bases || !out_jac) return ctx ? set_err(ctx, CZK_ERR_ARG, "null msm argument") : CZK_ERR_ARG;
    if (n_scalars && !scalars) return set_err(ctx, CZK_ERR_ARG, "null scalars");
    if (scalar_form != CZK_SCALAR_CANONICAL && scalar_form != CZK_SCALAR_MONTGOMERY) return set_err(ctx, CZK_ERR_ARG, "bad scalar_form");
    if (!lanes) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    const bool stable = (mem & CZK_MEM_STABLE) != 0, same = (mem & CZK_MEM_SAME_SCALARS) != 0;
    mem &= ~(CZK_MEM_STABLE | CZK_MEM_SAME_SCALARS);
    if (!valid_mem(mem) || (stable && (blocking || mem != CZK_MEM_DEVICE)) || (same && !stable))
        return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE (CZK_MEM_STABLE: czk_msm_async with device scalars only; CZK_MEM_SAME_SCALARS: with CZK_MEM_STABLE only)");
    const u64* sdev = scalars;
    DeviceBuf tmp;
    if (mem == CZK_MEM_HOST && n_scalars) {
        CZK_TRY(stage_take(ctx, lanes * n_scalars * 32, &tmp));   // pooled: hipMalloc / hipFree per call cost more than the copy
        hipError_t e = hipMemcpyAsync(tmp.p, scalars, lanes * n_scalars * 32, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            stage_give(ctx, tmp);
            return set_err(ctx, CZK_ERR_HIP, "H2D scalars");
        }
        sdev = (const u64*)tmp.p;
    }
    // host scalars: always blocking (the digits have been extracted from the staging buffer by the time this returns)
    int rc = msm_device(ctx, bases, sdev, n_scalars, lanes, scalar_form, out_jac, blocking || tmp.p != nullptr, stable && !blocking, same);
    if (tmp.p) stage_give(ctx, tmp);
    return rc;
}
extern "C" int czk_msm(czk_ctx* ctx, const czk_bases* bases, const uint64_t* scalars, size_t n_scalars, size_t lanes, int scalar_form, int mem,
                       uint64_t* out_jac) {
    return msm_common(ctx, bases, scalars, n_scalars, lanes, scalar_form, mem, out_jac, true);
}
extern "C" int czk_msm_async(czk_ctx* ctx, const czk_bases* bases, const uint64_t* scalars, size_t n_scalars, size_t lanes, int scalar_form,
                             int mem, uint64_t* out_jac) {
    return msm_common(ctx, bases, scalars, n_scalars, lanes, scalar_form, mem, out_jac, false);
}
extern "C" int czk_ctx_mark(czk_ctx* ctx, uint64_t* out_mark) {
    if (!ctx || !out_mark) return ctx ? set_err(ctx, CZK_ERR_ARG, "null czk_ctx_mark argument") : CZK_ERR_ARG;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    return ctx_mark(ctx, out_mark);
}
extern "C" int czk_ctx_wait_mark(czk_ctx* ctx, uint64_t mark) {
    if (!ctx) return CZK_ERR_ARG;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    return ctx_wait_mark(ctx, mark);
}

static int msm_oneshot(czk_ctx* ctx, int group, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, size_t lanes,
                       int scalar_form, uint64_t* out_jac) {
    czk_bases* b = nullptr;   // (a null ctx is refused by czk_bases_register)
    // used once: no window tables (building them costs ~20 point doublings per point and window -- more than the MSM itself)
    // ... and CZK_MEM_ANY_POINTS: this is the reference's own signature (VariableBaseMSM::multi_scalar_mul, complete on every curve point), so the
    // one-shot entry points make no subgroup assumption; registered keys (czk_bases_register) choose it themselves
    CZK_TRY(czk_bases_register(ctx, group, bases_xy, inf, n, CZK_MEM_HOST | CZK_MEM_NO_TABLES | CZK_MEM_ANY_POINTS, &b));
    int rc = czk_msm(ctx, b, scalars, n, lanes, scalar_form, CZK_MEM_HOST, out_jac);
    czk_bases_release(b);
    return rc;
}
extern "C" int czk_msm_g1(czk_ctx* ctx, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, size_t lanes,
                          int scalar_form, uint64_t* out_jac) {
    return msm_oneshot(ctx, CZK_G1, bases_xy, inf, scalars, n, lanes, scalar_form, out_jac);
}
extern "C" int czk_msm_g2(czk_ctx* ctx, const uint64_t* bases_xy, const uint8_t* inf, const uint64_t* scalars, size_t n, size_t lanes,
                          int scalar_form, uint64_t* out_jac) {
    return msm_oneshot(ctx, CZK_G2, bases_xy, inf, scalars, n, lanes, scalar_form, out_jac);
}
