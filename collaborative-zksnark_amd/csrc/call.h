// call.h -- the host-side plumbing every extern "C" entry point of point_ops / fixed_base / point_codec / pairing / kzg.hip needs: argument
// checks, grid size, G1 / G2 dispatch, per-call device memory, outputs for host or device callers, and the "kernel -> Jacobian -> affine" launch.
#pragma once
#include "czk_internal.h"

namespace czk {

// ---- argument checks: each leaves its message in the context and returns CZK_ERR_ARG (entry points run them in their documented order)
inline int check_group(czk_ctx* ctx, int group) {
    return group == CZK_G1 || group == CZK_G2 ? CZK_OK : set_err(ctx, CZK_ERR_ARG, "group must be CZK_G1 or CZK_G2");
}
inline int check_mem(czk_ctx* ctx, int mem) { return valid_mem(mem) ? CZK_OK : set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE"); }
inline int check_group_mem(czk_ctx* ctx, int group, int mem) {
    CZK_TRY(check_group(ctx, group));
    return check_mem(ctx, mem);
}
inline int check_scalar_form(czk_ctx* ctx, int form) {
    return form == CZK_SCALAR_CANONICAL || form == CZK_SCALAR_MONTGOMERY ? CZK_OK : set_err(ctx, CZK_ERR_ARG, "bad scalar_form");
}
// k + 1 host offsets of k segments (non-null, k > 0): *n = offsets[k], the number of items
inline int check_offsets(czk_ctx* ctx, const size_t* offsets, size_t k, size_t* n) {
    if (offsets[0] != 0) return set_err(ctx, CZK_ERR_ARG, "offsets[0] must be 0");
    for (size_t j = 0; j < k; j++)
        if (offsets[j + 1] < offsets[j]) return set_err(ctx, CZK_ERR_ARG, "offsets must be non-decreasing");
    *n = offsets[k];
    return CZK_OK;
}
// a handle (key, table) is only usable on the GPU it was made on; `msg` names the handle
inline int check_device(czk_ctx* ctx, int handle_device, const char* msg) {
    return handle_device == ctx->device ? CZK_OK : set_err(ctx, CZK_ERR_ARG, msg);
}

// blocks for n items at `per_block` items each (one per thread of a block of 128 unless said otherwise)
inline dim3 grid_for(size_t n, unsigned per_block = 128) { return dim3((unsigned)((n + per_block - 1) / per_block)); }

// G1 / G2 dispatch: fn(FieldTag<Fq>{}) or fn(FieldTag<Fq2>{}); a generic lambda reads the field as `typename decltype(tag)::type`
template <class F>
struct FieldTag {
    using type = F;
};
template <class Fn>
inline auto by_group(int group, Fn&& fn) {
    if (group == CZK_G1) return fn(FieldTag<Fq>{});
    return fn(FieldTag<Fq2>{});
}

// Device allocations of ONE call of the pairing / KZG entry points: hipMalloc per piece, owned by this object and freed by its destructor, i.e. on
// every return path (hipFree waits for the device, so a piece still in use by enqueued work is safe).  `what` completes the CZK_ERR_NOMEM message.
// NOTE: this per-call hipMalloc / hipFree is a known cost of the pairing and KZG calls, left as it is (the staging pool would keep the memory).
struct CallMem {
    czk_ctx* ctx;
    const char* what;
    std::vector<void*> ps;
    CallMem(czk_ctx* c, const char* w) : ctx(c), what(w) {}
    ~CallMem() {
        for (void* p : ps) (void)hipFree(p);
    }
    template <class T>
    int get(T** out, size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return set_err(ctx, CZK_ERR_NOMEM, std::string("hipMalloc ") + what);
        ps.push_back(p);
        *out = (T*)p;
        return CZK_OK;
    }
    int points(int group, u64** pts, uint8_t** inf, size_t n) {   // n affine points and their infinity flags
        CZK_TRY(get(pts, n * (group == CZK_G1 ? 96 : 192)));
        return get(inf, n);
    }
    // an input: used in place (device memory) or copied in on the context's stream (host memory); null stays null
    template <class T>
    int in(const T* src, size_t bytes, int mem, const T** out) {
        if (!src || mem == CZK_MEM_DEVICE) {
            *out = src;
            return CZK_OK;
        }
        T* d;
        CZK_TRY(get(&d, bytes));
        CZK_HIP(ctx, hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        *out = d;
        return CZK_OK;
    }
};

// One output of a call, for either kind of caller.  open(): the caller's buffer itself when it is device memory; scratch otherwise -- for a host
// caller, and for a caller that passes null for an optional output the kernel writes regardless.  (An optional output the kernel skips when null is
// simply not opened: dev stays null.)  Two sources of scratch:
//   staging pool (default): goes back in the destructor; re-use is ordered, every later user enqueues on the same stream.  copy_back() enqueues the
//     copy to a host caller that asked for the output; close() does the same and WAITS for the stream: a call closes ONE such output, last, and
//     that is its single blocking point.
//   the call's CallMem (`from`): owned and freed by it.  close() does NOT wait for the stream: it is a synchronous hipMemcpy per output, valid
//     only after the owner has synchronised the stream itself (the pairing and KZG calls do, right after their last kernel).
struct CallOut {
    Staged st;
    void *dev = nullptr, *user = nullptr;
    size_t bytes = 0;
    bool host = false;
    explicit CallOut(czk_ctx* c) : st{c} {}
    int open(void* out, size_t n_bytes, int mem, CallMem* from = nullptr) {
        user = out, bytes = n_bytes, host = mem == CZK_MEM_HOST;
        if (!host && out) dev = out;
        else if (from) return from->get(&dev, bytes);
        else {
            CZK_TRY(st.to_device(nullptr, bytes, CZK_MEM_HOST));
            dev = st.dev;
        }
        return CZK_OK;
    }
    int copy_back() {
        if (host && user) CZK_HIP(st.ctx, hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, st.ctx->stream));
        return CZK_OK;
    }
    int close() {
        if (!host || !user) return CZK_OK;
        if (st.owned) return st.to_host(user, bytes);
        CZK_HIP(st.ctx, hipMemcpy(user, dev, bytes, hipMemcpyDeviceToHost));
        return CZK_OK;
    }
    u64* words() const { return (u64*)dev; }
    uint8_t* flags() const { return (uint8_t*)dev; }
};

// n affine points + their infinity flags, the result of every point kernel.  The normalisation always writes flags, so `inf` is the optional kind.
struct AffineOut {
    CallOut pts, inf;
    explicit AffineOut(czk_ctx* c) : pts(c), inf(c) {}
    int open(int group, uint64_t* out, uint8_t* out_inf, size_t n, int mem) {
        CZK_TRY(pts.open(out, n * (group == CZK_G1 ? 96 : 192), mem));
        return inf.open(out_inf, n, mem);
    }
    int close() {   // (blocks for host callers)
        CZK_TRY(inf.copy_back());
        return pts.close();
    }
};

// launch(tag, jac) enqueues the kernel of the group's field (by_group) that writes n Jacobian results; the shared batch normalisation
// (msm_bases.hip) then writes them as affine points + flags to out / out_inf (device).  The workspace -- the n triples and the normalisation's
// running products -- is the staging pool's and goes back as soon as the work is enqueued (re-use is ordered by the stream).  Only enqueues.
// `prof` names the profile bracket, `what` the error.  A caller that must take the workspace itself (points_sum_device: before its offsets
// buffer, so that the pool is asked in the same order as ever) passes it as `own_ws` and gives it back itself.
inline size_t affine_ws_bytes(int group, size_t n) { return n * (group == CZK_G1 ? 18 + 6 : 36 + 12) * 8; }
template <class Launch>
inline int launch_to_affine(czk_ctx* ctx, const char* prof, const char* what, int group, size_t n, u64* out, uint8_t* out_inf, Launch&& launch,
                            const DeviceBuf* own_ws = nullptr) {
    DeviceBuf ws = own_ws ? *own_ws : DeviceBuf{};
    if (!own_ws) CZK_TRY(stage_take(ctx, affine_ws_bytes(group, n), &ws));
    u64* jac = (u64*)ws.p;
    {
        ProfScope ps(ctx, prof);
        by_group(group, [&](auto tag) { launch(tag, jac); });
        launch_batch_to_affine(ctx->stream, group, jac, n, jac + n * (group == CZK_G1 ? 18 : 36), out, out_inf);
    }
    const hipError_t e = hipGetLastError();
    if (!own_ws) stage_give(ctx, ws);
    return e == hipSuccess ? CZK_OK : set_err(ctx, CZK_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace czk
