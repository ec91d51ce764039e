// fs.hip -- Fiat-Shamir transcripts: the reference's FiatShamirRng<Blake2s> (marlin/src/rng.rs, mpc-plonk/src/util.rs:44-108) restated exactly, with its
// state in host memory (plain C++, no context: a verifier without a GPU) or in device memory (every operation a kernel on the context's stream).
//   state      seed (32 bytes) and a generator; from_seed(m): seed = Blake2s(m); absorb(m): seed = Blake2s(m || seed); both reseed the generator and
//              put its position back to 0.  The pending message streams into the hash (blake2s.h) as it is put, so no message is ever held whole.
//   generator  rand_chacha 0.2's ChaChaRng: ChaCha20 (chacha20.h) under key = seed, a 64-bit block counter in words 12-13, stream id 0 in words 14-15, the
//              keystream's little-endian words in order; next_u64 = two consecutive words, low first.  The position counts 32-bit words from the start of
//              the keystream.  Only u64-granular draws exist here, so the position stays even and a u64 never straddles a 16-word block: BlockRng's
//              odd-index case (a u64 assembled from the last word of one buffer and the first of the next) cannot arise and is not restated.
//   Fr::rand   (algebra/ff/src/fields/arithmetic.rs:193-216) four next_u64 fill the limbs low first, the top limb is masked with u64::MAX >> 3, the limbs are
//              taken AS the Montgomery representation and accepted when < r, otherwise drawn again: r / 2^253 = 0.58 of the draws pass.  The loop gives
//              up after FS_MAX_DRAWS draws of one element (probability 0.42^256) and sets the state's sticky error word instead of spinning.
//   ToBytes    Fr: into_repr() as 32 little-endian bytes; an affine point: x || y || infinity as one byte (short_weierstrass_jacobian.rs:260-267), Fq 48
//              bytes, Fq2 c0 then c1 -- 97 bytes for G1, 193 for G2.  A point whose flag is set is written as the reference's zero(): x = 0, y = 1.
//   device     one workgroup of 64 threads per operation.  The state is copied into LDS, thread 0 runs the hash and the generator -- both are chains --
//              while all 64 threads fetch the bytes or convert the elements of the next chunk, and the state is copied back.  No spin waits, no loop
//              without a bound.  Scratch only where the out-of-line Montgomery multiply takes its operands by address (put_fr 80, put_points 112 bytes
//              per lane; the hash, the generator and the byte path have none: profiles/fs_resource_usage.txt).
#include <cstring>

#include "blake2s.h"
#include "chacha20.h"
#include "czk_internal.h"

namespace czk {

constexpr unsigned FS_MAX_DRAWS = 256;   // draws per element before a squeeze gives up
constexpr u32 FS_ERR_DRAWS = 1;          // error word: a squeeze_fr gave up
constexpr unsigned FS_CHUNK = 64;        // elements per cooperative step: one per thread

struct FsState {
    Blake2s hash;   // of the pending message
    uint8_t seed[32];
    u64 pos;        // generator position, in 32-bit words
    u32 seeded;     // a from_seed has happened
    u32 error;      // sticky
};
struct FsBlock {    // the keystream block the generator stands in
    u32 w[16];
    u64 index;
    u32 valid;
};

CZK_HD void fs_init(FsState& s) {
    s.hash.init();
    for (int i = 0; i < 32; i++) s.seed[i] = 0;
    s.pos = 0, s.seeded = 0, s.error = 0;
}
// closes the pending message as from_seed (absorb = false) or as absorb
CZK_HD void fs_close(FsState& s, bool absorb) {
    if (absorb) s.hash.update(s.seed, 32);
    s.hash.finish(s.seed);
    s.hash.init();
    s.pos = 0;
    if (!absorb) s.seeded = 1;
}
CZK_HD void fs_keystream_block(const uint8_t* seed, u64 index, FsBlock& b) {
    u32 key[8];
    for (int i = 0; i < 8; i++) key[i] = (u32)seed[4 * i] | (u32)seed[4 * i + 1] << 8 | (u32)seed[4 * i + 2] << 16 | (u32)seed[4 * i + 3] << 24;
    u32 x[16];   // (registers: b may live in LDS)
    chacha20_block(key, (u32)index, (u32)(index >> 32), 0, 0, x);
    for (int i = 0; i < 16; i++) b.w[i] = x[i];
    b.index = index, b.valid = 1;
}
CZK_HD u64 fs_next_u64(FsState& s, FsBlock& b) {
    const u64 index = s.pos >> 4;
    if (!b.valid || b.index != index) fs_keystream_block(s.seed, index, b);
    const unsigned i = (unsigned)(s.pos & 15);   // even
    s.pos += 2;
    return (u64)b.w[i] | (u64)b.w[i + 1] << 32;
}
// Fr::rand: out = 4 limbs, Montgomery form as drawn
CZK_HD void fs_next_fr(FsState& s, FsBlock& b, u64* out) {
    constexpr u64 R[4] = {0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull, 0x12ab655e9a2ca556ull};   // fr.rs:33-40 MODULUS
    for (unsigned draw = 0; draw < FS_MAX_DRAWS; draw++) {
        u64 l[4];
        for (int i = 0; i < 4; i++) l[i] = fs_next_u64(s, b);
        l[3] &= ~(u64)0 >> 3;
        bool less = false;   // l < r, from the top limb down
        for (int i = 3; i >= 0; i--) {
            if (l[i] != R[i]) {
                less = l[i] < R[i];
                break;
            }
        }
        if (less) {
            for (int i = 0; i < 4; i++) out[i] = l[i];
            return;
        }
    }
    s.error |= FS_ERR_DRAWS;
    for (int i = 0; i < 4; i++) out[i] = 0;
}

// limbs of any alignment a u64 has (host callers promise no more)
template <class P>
CZK_HD Fp<P> fs_load(const u64* p) {
    Fp<P> r;
    for (int i = 0; i < P::N / 2; i++) r.l[2 * i] = (u32)p[i], r.l[2 * i + 1] = (u32)(p[i] >> 32);
    return r;
}
// into_repr() as little-endian bytes: 4 N of them
template <class P>
CZK_HD void fs_field_bytes(const Fp<P>& mont, uint8_t* out) {
    const Fp<P> c = fp_into_repr(mont);
    for (int i = 0; i < P::N; i++)
        for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(c.l[i] >> (8 * j));
}
CZK_HD void fs_fr_bytes(const u64* v, uint8_t* out) { fs_field_bytes(fs_load<FrParams>(v), out); }
CZK_HD constexpr unsigned fs_point_bytes(int group) { return group == CZK_G1 ? 97u : 193u; }
// the ToBytes of one affine point: nf = 2 (G1) or 4 (G2) base-field coordinates of 6 u64 each, x first; then the flag
CZK_HD void fs_point_to_bytes(const u64* pt, bool inf, unsigned nf, uint8_t* out) {
#pragma unroll 1
    for (unsigned k = 0; k < nf; k++) {
        Fq c = fs_load<FqParams>(pt + 6 * k);
        if (inf) c = (k == nf / 2) ? Fq::one() : Fq::zero();   // zero(): x = 0, y = 1 (for Fq2: c0 = 1, c1 = 0)
        fs_field_bytes(c, out + 48 * k);
    }
    out[48 * nf] = inf ? 1 : 0;
}

// ---- device transcripts ---------------------------------------------------------------------------------------------------------------------------
struct FsShared {
    FsState st;
    FsBlock blk;
    uint8_t chunk[FS_CHUNK * 193];   // the step's bytes: 64 G2 points at most
};
__device__ __forceinline__ void fs_dev_enter(FsShared& sh, const FsState* g) {
    if (threadIdx.x == 0) {
        sh.st = *g;
        sh.blk.valid = 0;
    }
    __syncthreads();
}
__device__ __forceinline__ void fs_dev_leave(FsShared& sh, FsState* g) {
    __syncthreads();
    if (threadIdx.x == 0) *g = sh.st;
}

// reads p[0, len) only
__global__ __launch_bounds__(64) void k_fs_put_bytes(FsState* g, const uint8_t* p, size_t len) {
    __shared__ FsShared sh;
    fs_dev_enter(sh, g);
    constexpr size_t STEP = sizeof sh.chunk;
    for (size_t off = 0; off < len; off += STEP) {
        const size_t cnt = len - off < STEP ? len - off : STEP;
        for (size_t i = threadIdx.x; i < cnt; i += blockDim.x) sh.chunk[i] = p[off + i];
        __syncthreads();
        if (threadIdx.x == 0) sh.st.hash.update(sh.chunk, cnt);
        __syncthreads();
    }
    fs_dev_leave(sh, g);
}
// reads v[0, 4 n) only
__global__ __launch_bounds__(64) void k_fs_put_fr(FsState* g, const u64* v, size_t n) {
    __shared__ FsShared sh;
    fs_dev_enter(sh, g);
    for (size_t off = 0; off < n; off += FS_CHUNK) {
        const size_t cnt = n - off < FS_CHUNK ? n - off : FS_CHUNK;
        if (threadIdx.x < cnt) fs_fr_bytes(v + 4 * (off + threadIdx.x), sh.chunk + 32 * threadIdx.x);
        __syncthreads();
        if (threadIdx.x == 0) sh.st.hash.update(sh.chunk, 32 * cnt);
        __syncthreads();
    }
    fs_dev_leave(sh, g);
}
// reads pts[0, 6 nf n) and, when given, inf[0, n) only
__global__ __launch_bounds__(64) void k_fs_put_points(FsState* g, const u64* pts, const uint8_t* inf, size_t n, unsigned nf) {
    __shared__ FsShared sh;
    fs_dev_enter(sh, g);
    const unsigned each = 48 * nf + 1;
    for (size_t off = 0; off < n; off += FS_CHUNK) {
        const size_t cnt = n - off < FS_CHUNK ? n - off : FS_CHUNK;
        if (threadIdx.x < cnt) fs_point_to_bytes(pts + 6 * nf * (off + threadIdx.x), inf && inf[off + threadIdx.x], nf, sh.chunk + each * threadIdx.x);
        __syncthreads();
        if (threadIdx.x == 0) sh.st.hash.update(sh.chunk, each * cnt);
        __syncthreads();
    }
    fs_dev_leave(sh, g);
}
__global__ __launch_bounds__(64) void k_fs_init(FsState* g) {
    if (threadIdx.x == 0) fs_init(*g);
}
__global__ __launch_bounds__(64) void k_fs_close(FsState* g, int absorb) {
    __shared__ FsShared sh;
    fs_dev_enter(sh, g);
    if (threadIdx.x == 0) fs_close(sh.st, absorb != 0);
    fs_dev_leave(sh, g);
}
// writes out[0, 4 n) (fr) or out[0, n) only.  The draws are a chain: thread 0 makes them, at most FS_MAX_DRAWS per element.
__global__ __launch_bounds__(64) void k_fs_squeeze(FsState* g, u64* out, size_t n, int fr) {
    __shared__ FsShared sh;
    fs_dev_enter(sh, g);
    if (threadIdx.x == 0) {
        for (size_t i = 0; i < n; i++) {
            if (fr) {
                u64 l[4];
                fs_next_fr(sh.st, sh.blk, l);
                for (int j = 0; j < 4; j++) out[4 * i + j] = l[j];
            } else {
                out[i] = fs_next_u64(sh.st, sh.blk);
            }
        }
    }
    fs_dev_leave(sh, g);
}

}  // namespace czk

using namespace czk;

struct czk_fs {
    czk_ctx* ctx = nullptr;
    int mem = CZK_MEM_HOST;
    FsState host;             // host transcripts: the state
    FsState* dev = nullptr;   // device transcripts: the state
    // what the host knows of a device transcript without waiting for it: the argument rules need no read-back
    bool seeded = false;
    u64 pending = 0;
};

namespace {
int fs_err(czk_fs* fs, int code, const char* msg) { return set_err(fs ? fs->ctx : nullptr, code, msg); }
int fs_error_word(czk_fs* fs, u32 word) {
    return word ? fs_err(fs, CZK_ERR_CHECK, "czk_fs: the transcript's error word is set (a squeeze gave up after 256 rejected draws of one element)") : CZK_OK;
}
// the common head of the put calls: 0 = go on, 1 = nothing to do, else an error
int fs_put_head(czk_fs* fs, const void* p, size_t n, int mem, int* rc) {
    *rc = CZK_OK;
    if (!fs || !valid_mem(mem)) return *rc = fs_err(fs, CZK_ERR_ARG, "czk_fs_put: null transcript or mem neither CZK_MEM_HOST nor CZK_MEM_DEVICE"), 2;
    if (!n) return 1;
    if (fs->mem == CZK_MEM_HOST && mem == CZK_MEM_DEVICE) return *rc = fs_err(fs, CZK_ERR_ARG, "czk_fs_put: device pointers given to a host transcript"), 2;
    if (!p) return *rc = fs_err(fs, CZK_ERR_ARG, "czk_fs_put: null data"), 2;
    return 0;
}
// device transcripts: `bytes` of host data staged in stream order (mem = HOST), or the device pointer itself
struct FsInput {
    StageHold hold;
    const void* dev = nullptr;
    explicit FsInput(czk_ctx* ctx) : hold(ctx) {}
    int take(const void* p, size_t bytes, int mem) {
        if (mem == CZK_MEM_DEVICE) return dev = p, CZK_OK;
        CZK_TRY(hold.take(bytes));
        dev = hold.b.p;
        return upload_pageable(hold.ctx, hold.b.p, p, bytes);
    }
};
}  // namespace

extern "C" void czk_blake2s(const void* data, size_t len, uint8_t* out32) {
    Blake2s h;
    h.init();
    h.update((const uint8_t*)data, len);
    h.finish(out32);
}

extern "C" int czk_fs_keystream(const uint8_t* seed32, uint64_t word_pos, uint32_t* out, size_t n) {
    if (!seed32 || (n && !out)) return CZK_ERR_ARG;
    FsBlock b;
    b.valid = 0;
    for (size_t i = 0; i < n; i++, word_pos++) {
        if (!b.valid || b.index != word_pos >> 4) fs_keystream_block(seed32, word_pos >> 4, b);
        out[i] = b.w[word_pos & 15];
    }
    return CZK_OK;
}

extern "C" int czk_fs_create(czk_ctx* ctx, int mem, czk_fs** out) {
    if (!out) return set_err(ctx, CZK_ERR_ARG, "czk_fs_create: null output");
    *out = nullptr;
    if (!valid_mem(mem) || (mem == CZK_MEM_DEVICE && !ctx)) return set_err(ctx, CZK_ERR_ARG, "czk_fs_create: mem is CZK_MEM_HOST, or CZK_MEM_DEVICE with a context");
    czk_fs* fs = new czk_fs;
    fs->ctx = ctx, fs->mem = mem;
    fs_init(fs->host);
    if (mem == CZK_MEM_DEVICE) {
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipMalloc((void**)&fs->dev, sizeof(FsState));
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_fs_init, dim3(1), dim3(64), 0, ctx->stream, fs->dev);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            if (fs->dev) (void)hipFree(fs->dev);
            delete fs;
            return set_err(ctx, CZK_ERR_HIP, std::string("czk_fs_create: ") + hipGetErrorString(e));
        }
    }
    *out = fs;
    return CZK_OK;
}

extern "C" void czk_fs_release(czk_fs* fs) {
    if (!fs) return;
    if (fs->dev) {
        (void)hipSetDevice(fs->ctx->device);
        (void)hipStreamSynchronize(fs->ctx->stream);
        (void)hipFree(fs->dev);
    }
    delete fs;
}

extern "C" int czk_fs_put_bytes(czk_fs* fs, const void* p, size_t len, int mem) {
    int rc;
    if (fs_put_head(fs, p, len, mem, &rc)) return rc;
    if (fs->mem == CZK_MEM_HOST) {
        fs->host.hash.update((const uint8_t*)p, len);
        return CZK_OK;
    }
    czk_ctx* ctx = fs->ctx;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    FsInput in(ctx);
    CZK_TRY(in.take(p, len, mem));
    hipLaunchKernelGGL(k_fs_put_bytes, dim3(1), dim3(64), 0, ctx->stream, fs->dev, (const uint8_t*)in.dev, len);
    CZK_HIP(ctx, hipGetLastError());
    fs->pending += len;
    return CZK_OK;
}

extern "C" int czk_fs_put_fr(czk_fs* fs, const uint64_t* v, size_t n, int mem) {
    int rc;
    if (fs_put_head(fs, v, n, mem, &rc)) return rc;
    if (n > SIZE_MAX / 32) return fs_err(fs, CZK_ERR_SIZE, "czk_fs_put_fr: the byte count overflows");
    if (fs->mem == CZK_MEM_HOST) {
        for (size_t i = 0; i < n; i++) {
            uint8_t b[32];
            fs_fr_bytes((const u64*)v + 4 * i, b);
            fs->host.hash.update(b, 32);
        }
        return CZK_OK;
    }
    czk_ctx* ctx = fs->ctx;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    FsInput in(ctx);
    CZK_TRY(in.take(v, n * 32, mem));
    hipLaunchKernelGGL(k_fs_put_fr, dim3(1), dim3(64), 0, ctx->stream, fs->dev, (const u64*)in.dev, n);
    CZK_HIP(ctx, hipGetLastError());
    fs->pending += n * 32;
    return CZK_OK;
}

extern "C" int czk_fs_put_points(czk_fs* fs, int group, const uint64_t* pts, const uint8_t* inf, size_t n, int mem) {
    int rc;
    if (fs_put_head(fs, pts, n, mem, &rc)) return rc;
    if (group != CZK_G1 && group != CZK_G2) return fs_err(fs, CZK_ERR_ARG, "czk_fs_put_points: group is CZK_G1 or CZK_G2");
    const unsigned nf = group == CZK_G1 ? 2 : 4, each = fs_point_bytes(group);
    if (n > SIZE_MAX / 256) return fs_err(fs, CZK_ERR_SIZE, "czk_fs_put_points: the byte count overflows");
    if (fs->mem == CZK_MEM_HOST) {
        for (size_t i = 0; i < n; i++) {
            uint8_t b[193];
            fs_point_to_bytes((const u64*)pts + 6 * nf * i, inf && inf[i], nf, b);
            fs->host.hash.update(b, each);
        }
        return CZK_OK;
    }
    czk_ctx* ctx = fs->ctx;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    FsInput in(ctx), in_inf(ctx);
    CZK_TRY(in.take(pts, n * 48 * nf, mem));
    if (inf) CZK_TRY(in_inf.take(inf, n, mem));
    hipLaunchKernelGGL(k_fs_put_points, dim3(1), dim3(64), 0, ctx->stream, fs->dev, (const u64*)in.dev, (const uint8_t*)in_inf.dev, n, nf);
    CZK_HIP(ctx, hipGetLastError());
    fs->pending += n * each;
    return CZK_OK;
}

static int fs_close_call(czk_fs* fs, bool absorb) {
    if (!fs) return CZK_ERR_ARG;
    if (fs->mem == CZK_MEM_HOST) {
        fs_close(fs->host, absorb);
        return CZK_OK;
    }
    czk_ctx* ctx = fs->ctx;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_fs_close, dim3(1), dim3(64), 0, ctx->stream, fs->dev, absorb ? 1 : 0);
    CZK_HIP(ctx, hipGetLastError());
    fs->pending = 0;
    if (!absorb) fs->seeded = true;
    return CZK_OK;
}
extern "C" int czk_fs_seed(czk_fs* fs) { return fs_close_call(fs, false); }
extern "C" int czk_fs_absorb(czk_fs* fs) { return fs_close_call(fs, true); }

static int fs_squeeze(czk_fs* fs, uint64_t* out, size_t n, int mem, bool fr) {
    if (!fs || !valid_mem(mem)) return fs_err(fs, CZK_ERR_ARG, "czk_fs_squeeze: null transcript or mem neither CZK_MEM_HOST nor CZK_MEM_DEVICE");
    if (!n) return CZK_OK;
    if (fs->mem == CZK_MEM_HOST && mem == CZK_MEM_DEVICE) return fs_err(fs, CZK_ERR_ARG, "czk_fs_squeeze: device pointers given to a host transcript");
    const bool host = fs->mem == CZK_MEM_HOST;
    if (!(host ? fs->host.seeded != 0 : fs->seeded)) return fs_err(fs, CZK_ERR_ARG, "czk_fs_squeeze: no czk_fs_seed yet");
    if (host ? fs->host.hash.length() != 0 : fs->pending != 0) return fs_err(fs, CZK_ERR_ARG, "czk_fs_squeeze: the pending message is not empty (czk_fs_absorb it first)");
    if (!out) return fs_err(fs, CZK_ERR_ARG, "czk_fs_squeeze: null output");
    const size_t each = fr ? 32 : 8;
    if (n > SIZE_MAX / each) return fs_err(fs, CZK_ERR_SIZE, "czk_fs_squeeze: the byte count overflows");
    if (host) {
        FsBlock b;
        b.valid = 0;
        for (size_t i = 0; i < n; i++) {
            if (fr) fs_next_fr(fs->host, b, (u64*)out + 4 * i);
            else out[i] = fs_next_u64(fs->host, b);
        }
        return fs_error_word(fs, fs->host.error);
    }
    czk_ctx* ctx = fs->ctx;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    StageHold ws(ctx);
    u64* dst = (u64*)out;
    if (mem == CZK_MEM_HOST) {
        CZK_TRY(ws.take(n * each));
        dst = (u64*)ws.b.p;
    }
    hipLaunchKernelGGL(k_fs_squeeze, dim3(1), dim3(64), 0, ctx->stream, fs->dev, dst, n, fr ? 1 : 0);
    CZK_HIP(ctx, hipGetLastError());
    if (mem == CZK_MEM_DEVICE) return CZK_OK;
    u32 word = 0;
    CZK_TRY(download_pageable(ctx, out, dst, n * each));   // blocks
    CZK_TRY(download_pageable(ctx, &word, &fs->dev->error, sizeof word));
    return fs_error_word(fs, word);
}
extern "C" int czk_fs_squeeze_fr(czk_fs* fs, uint64_t* out, size_t n, int mem) { return fs_squeeze(fs, out, n, mem, true); }
extern "C" int czk_fs_squeeze_u64(czk_fs* fs, uint64_t* out, size_t n, int mem) { return fs_squeeze(fs, out, n, mem, false); }

extern "C" int czk_fs_state(czk_fs* fs, uint8_t* seed32, uint64_t* word_pos) {
    if (!fs) return CZK_ERR_ARG;
    FsState st = fs->host;
    if (fs->mem == CZK_MEM_DEVICE) {
        CZK_HIP(fs->ctx, hipSetDevice(fs->ctx->device));
        CZK_TRY(download_pageable(fs->ctx, &st, fs->dev, sizeof st));
    }
    if (seed32) memcpy(seed32, st.seed, 32);
    if (word_pos) *word_pos = st.pos;
    return fs_error_word(fs, st.error);
}
