// net_rounds.hip -- the MPC rounds on a communicator (net.h): the reference's commit-then-open round, its batch opens and its shared-value protocols with one
// party per communicator, each as a single call on device lanes.  Host code only (the kernels it launches live in share.hip / share_mul.hip / gsz_mul.hip /
// gsz_dn.hip / commit_tree.hip / fr_vec.hip); every byte crosses the wire through the communicator's exchanges (net.hip).
//
//   reference                                                            here
//   MpcSerNet::atomic_broadcast     mpc-algebra/src/channel.rs:50-75      czk_net_atomic_broadcast
//   SpdzFieldShare::batch_open      mpc-algebra/src/share/spdz.rs:166-185 czk_spdz_batch_open
//   AdditiveFieldShare::batch_open  mpc-algebra/src/share/add.rs:256-259  czk_add_batch_open
//   GszFieldShare::batch_open       share/gsz20/mod.rs:286-300, 440-466   czk_gsz_batch_open
//   gsz20::batch_king_compute       share/gsz20/mod.rs:494-527            czk_gsz_batch_king_compute
//   FieldShare::batch_mul / batch_inv / partial_products  share/field.rs:97-182   czk_net_share_batch_mul / _batch_inv / _partial_products
//   gsz20 batch_mult / batch_inv / partial_products / hadamard_check  share/gsz20/mod.rs:325-366, :559-808   czk_net_gsz_share_* / czk_net_gsz_product_check
//   Vec<Fr> wire format             algebra/serialize/src/lib.rs:220-229  czk_fr_vec_serialize / _deserialize
#include <sys/random.h>

#include <cstring>

#include "net.h"
#include "sha256.h"

using namespace czk;

namespace {
// a null communicator is CZK_ERR_ARG; one created without a context gets `who` + `needs`, every caller's own wording (put together only when it is needed)
int need_ctx(czk_net* n, const char* who, const char* needs = " needs a communicator created with a context") {
    if (!n) return CZK_ERR_ARG;
    if (!n->ctx) return net_err(n, CZK_ERR_ARG, std::string(who) + needs);
    return CZK_OK;
}
}  // namespace

// (SHA-256, the reference's CommitHash of mpc-algebra/src/channel.rs:92: sha256.h)
extern "C" void czk_sha256(const void* data, size_t len, uint8_t* out32) {
    Sha256 s;
    s.update(data, len);
    s.finish(out32);
}

// ---- wire format -----------------------------------------------------------------------------------------------------------------------
extern "C" int czk_fr_vec_serialize(czk_ctx* ctx, const uint64_t* a, size_t n, int mem, uint8_t* out) {
    if (!ctx) return CZK_ERR_ARG;
    if (!out || (n && !a) || !valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "czk_fr_vec_serialize: null / bad argument");
    const uint64_t len = n;
    memcpy(out, &len, 8);   // u64 little-endian length (serialize/src/lib.rs:222-223); the hosts this library runs on are little-endian
    if (!n) return CZK_OK;
    if (mem == CZK_MEM_HOST) {
        std::vector<uint64_t> rep(4 * n);
        CZK_TRY(czk_fr_into_repr(ctx, a, rep.data(), n, CZK_MEM_HOST));
        memcpy(out + 8, rep.data(), 32 * n);
        return CZK_OK;
    }
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    DeviceBuf b;
    CZK_TRY(stage_take(ctx, 32 * n, &b));
    int rc = czk_fr_into_repr(ctx, a, (uint64_t*)b.p, n, CZK_MEM_DEVICE);
    if (rc == CZK_OK) rc = download_pageable(ctx, out + 8, b.p, 32 * n);   // blocking
    stage_give(ctx, b);
    return rc;
}

extern "C" int czk_fr_vec_deserialize(czk_ctx* ctx, const uint8_t* bytes, size_t len, uint64_t* out, size_t cap, int mem, size_t* n_out) {
    if (!ctx) return CZK_ERR_ARG;
    if (!bytes || !n_out || len < 8 || !valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "czk_fr_vec_deserialize: null / short input");
    uint64_t n64;
    memcpy(&n64, bytes, 8);
    if (n64 > (len - 8) / 32 || 8 + 32 * (size_t)n64 != len) return set_err(ctx, CZK_ERR_ARG, "Vec<Fr> wire format: length prefix does not match the payload");
    const size_t n = (size_t)n64;
    *n_out = n;
    if (n > cap || (n && !out)) return set_err(ctx, CZK_ERR_ARG, "czk_fr_vec_deserialize: more elements than the output holds");
    if (!n) return CZK_OK;
    std::vector<uint64_t> rep(4 * n);
    memcpy(rep.data(), bytes + 8, 32 * n);
    // Fp::deserialize -> from_repr fails on a non-canonical value (fields/macros.rs:443-454: `if r.is_valid()`)
    static const uint64_t R_MOD[4] = {0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull, 0x12ab655e9a2ca556ull};
    for (size_t i = 0; i < n; i++) {
        bool lt = false;
        for (int j = 3; j >= 0; j--) {
            if (rep[4 * i + j] != R_MOD[j]) {
                lt = rep[4 * i + j] < R_MOD[j];
                break;
            }
        }
        if (!lt) return set_err(ctx, CZK_ERR_ARG, "Vec<Fr> wire format: element not below the modulus");
    }
    if (mem == CZK_MEM_HOST) return czk_fr_from_repr(ctx, rep.data(), out, n, CZK_MEM_HOST);
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    CZK_TRY(upload_pageable(ctx, out, rep.data(), 32 * n));   // returns once `rep` has been read
    return czk_fr_from_repr(ctx, out, out, n, CZK_MEM_DEVICE);
}

// ---- atomic_broadcast and the batch opens ----------------------------------------------------------------------------------------------
namespace {
int commit_randomness(czk_net* n, const uint8_t* rand32, uint8_t* out32) {   // the caller's, or fresh from the kernel
    if (rand32) memcpy(out32, rand32, 32);
    else if (getrandom(out32, 32, 0) != 32) return net_err(n, CZK_ERR_NET, "getrandom failed");
    return CZK_OK;
}
// MpcSerNet::atomic_broadcast from the point where this party holds its commitment `mine` to x under rnd.  commit(v, lanes, rnds, out) makes the 32-byte
// commitments of `lanes` vectors of cnt elements (cnt apart) under 32 bytes of randomness each.  The gathered vectors are verified either in one call over
// all `world` lanes, this party's own included whatever the world's size (one_pass), or the peers one at a time, this party's own lane not committed again.
template <class Commit>
int atomic_round(czk_net* n, const uint64_t* x, size_t cnt, uint64_t* recv, int mem, const uint8_t* rnd, const uint8_t* mine, bool one_pass, Commit commit) {
    const size_t W = (size_t)n->world;
    std::vector<uint8_t> all_commits(32 * W), all_rnd(32 * W), check(32 * W);
    CZK_TRY(exchange(n, Op::Broadcast, mine, 32, all_commits.data(), CZK_MEM_HOST));   // exchange commitments
    CZK_TRY(exchange(n, Op::Broadcast, x, 32 * cnt, recv, mem));                        // exchange (data || randomness)
    CZK_TRY(exchange(n, Op::Broadcast, rnd, 32, all_rnd.data(), CZK_MEM_HOST));
    count_stats(n, Op::Broadcast, 32);              // the reference's two broadcasts: 32 bytes, then ser + 32 bytes (channel.rs:58-61)
    count_stats(n, Op::Broadcast, 8 + 32 * cnt + 32);
    if (one_pass) CZK_TRY(commit(recv, W, all_rnd.data(), check.data()));
    for (size_t p = 0; p < W; p++) {
        if ((int)p == n->rank) continue;
        if (!one_pass) CZK_TRY(commit(recv + 4 * cnt * p, 1, &all_rnd[32 * p], &check[32 * p]));
        if (memcmp(&check[32 * p], &all_commits[32 * p], 32) != 0)
            return net_err(n, CZK_ERR_CHECK, "atomic_broadcast: party " + std::to_string(p) + "'s data does not match its commitment");
    }
    return CZK_OK;
}
}  // namespace

// commitment = H(data || randomness), SHA-256 over the reference's wire bytes: one serialization per vector, so the peers are verified one at a time.
// czk_fr_vec_serialize is what rejects a bad `mem` here, and it runs before the randomness is drawn.
extern "C" int czk_net_atomic_broadcast(czk_net* n, const uint64_t* x, size_t cnt, uint64_t* recv, const uint8_t* rand32, int mem) {
    CZK_TRY(need_ctx(n, "czk_net_atomic_broadcast"));
    if (cnt && (!x || !recv)) return net_err(n, CZK_ERR_ARG, "czk_net_atomic_broadcast: null buffer");
    const size_t ser = 8 + 32 * cnt;
    std::vector<uint8_t> wire(ser + 32);
    uint8_t rnd[32], mine[32];
    auto commit = [&](const uint64_t* v, size_t, const uint8_t* r, uint8_t* out) -> int {
        NET_CTX(n, czk_fr_vec_serialize(n->ctx, v, cnt, mem, wire.data()));
        memcpy(&wire[ser], r, 32);
        czk_sha256(wire.data(), wire.size(), out);
        return CZK_OK;
    };
    NET_CTX(n, czk_fr_vec_serialize(n->ctx, x, cnt, mem, wire.data()));
    CZK_TRY(commit_randomness(n, rand32, rnd));
    memcpy(&wire[ser], rnd, 32);
    czk_sha256(wire.data(), wire.size(), mine);
    return atomic_round(n, x, cnt, recv, mem, rnd, mine, false, commit);
}

// The same round with the tree commitment of commit_tree.hip: the same three exchanges with the same byte counts (a rank that made the SHA-256 call instead
// meets this one in every exchange, and both fail the check), the same stats; the W gathered vectors are hashed in one pass on the device.
extern "C" int czk_net_atomic_broadcast_tree(czk_net* n, const uint64_t* x, size_t cnt, uint64_t* recv, const uint8_t* rand32, int mem) {
    CZK_TRY(need_ctx(n, "czk_net_atomic_broadcast_tree"));
    if (!valid_mem(mem)) return net_err(n, CZK_ERR_ARG, "czk_net: mem must be CZK_MEM_HOST or CZK_MEM_DEVICE");
    if (cnt && (!x || !recv)) return net_err(n, CZK_ERR_ARG, "czk_net_atomic_broadcast_tree: null buffer");
    uint8_t rnd[32], mine[32];
    auto commit = [&](const uint64_t* v, size_t lanes, const uint8_t* r, uint8_t* out) -> int {
        NET_CTX(n, czk_fr_vec_commit(n->ctx, v, lanes, cnt, cnt, r, out, mem));   // (waits for the gathered vectors: stream order)
        return CZK_OK;
    };
    CZK_TRY(commit_randomness(n, rand32, rnd));
    CZK_TRY(commit(x, 1, rnd, mine));
    return atomic_round(n, x, cnt, recv, mem, rnd, mine, true, commit);
}

namespace {
int open_args(czk_net* n, const void* a, const void* b, size_t cnt) {
    CZK_TRY(need_ctx(n, "batch opens", " need a communicator created with a context"));
    if (cnt && (!a || !b)) return net_err(n, CZK_ERR_ARG, "batch open: null buffer");
    NET_HIP(n, hipSetDevice(n->ctx->device));
    return CZK_OK;
}
}  // namespace

extern "C" int czk_spdz_batch_open(czk_net* n, const uint64_t* sh, const uint64_t* mac, const uint64_t* mac_share, size_t cnt, uint64_t* out_value,
                                   int flags, uint64_t* out_bad) {
    CZK_TRY(open_args(n, sh, out_value, cnt));
    if (!out_bad || !mac_share || (cnt && !mac)) return net_err(n, CZK_ERR_ARG, "czk_spdz_batch_open: null argument");
    *out_bad = 0;
    if (!cnt) return CZK_OK;
    const size_t W = (size_t)n->world;
    CZK_TRY(net_buf(n, n->gather, W * cnt * 32));
    CZK_TRY(net_buf(n, n->dx, cnt * 32));
    uint64_t* g = (uint64_t*)n->gather.p;
    uint64_t* dx = (uint64_t*)n->dx.p;
    CZK_TRY(czk_net_broadcast(n, sh, cnt * 32, g, CZK_MEM_DEVICE));                       // let all_vals = Net::broadcast(&s_vals)
    NET_CTX(n, czk_fr_lanes_sum(n->ctx, g, W, cnt, out_value, nullptr));                  // vals[i] = sum over the parties
    NET_CTX(n, czk_fr_spdz_dx(n->ctx, out_value, mac, mac_share, dx, cnt));               // dx_t = mac_share * val - mac
    if (flags & CZK_OPEN_COMMIT_TREE) CZK_TRY(czk_net_atomic_broadcast_tree(n, dx, cnt, g, nullptr, CZK_MEM_DEVICE));
    else if (flags & CZK_OPEN_COMMIT) CZK_TRY(czk_net_atomic_broadcast(n, dx, cnt, g, nullptr, CZK_MEM_DEVICE));   // Net::atomic_broadcast(&dx_ts)
    else CZK_TRY(czk_net_broadcast(n, dx, cnt * 32, g, CZK_MEM_DEVICE));
    NET_CTX(n, czk_fr_lanes_sum(n->ctx, g, W, cnt, nullptr, out_bad));                    // assert!(sum.is_zero()) -- the caller's, on *out_bad
    return CZK_OK;
}

extern "C" int czk_add_batch_open(czk_net* n, const uint64_t* val, size_t cnt, uint64_t* out_value) {
    CZK_TRY(open_args(n, val, out_value, cnt));
    if (!cnt) return CZK_OK;
    const size_t W = (size_t)n->world;
    CZK_TRY(net_buf(n, n->gather, W * cnt * 32));
    CZK_TRY(czk_net_broadcast(n, val, cnt * 32, n->gather.p, CZK_MEM_DEVICE));
    NET_CTX(n, czk_fr_lanes_sum(n->ctx, (const uint64_t*)n->gather.p, W, cnt, out_value, nullptr));
    return CZK_OK;
}

namespace {
// GszFieldShare::batch_open's exchange and launch, enqueued: `bad` non-null adds the violations to that device counter (no read-back); null makes the
// blocking czk_fr_gsz_open count into *out_bad
int gsz_open_trip(czk_net* n, const uint64_t* val, size_t cnt, const uint32_t* degrees, unsigned degree, uint64_t* out_value, unsigned long long* bad, uint64_t* out_bad) {
    const size_t W = (size_t)n->world;
    CZK_TRY(net_buf(n, n->gather, W * cnt * 32));
    CZK_TRY(czk_net_broadcast(n, val, cnt * 32, n->gather.p, CZK_MEM_DEVICE));
    if (bad) NET_CTX(n, gsz_open_enqueue(n->ctx, (const u64*)n->gather.p, W, cnt, degrees, degree, (u64*)out_value, bad));
    else NET_CTX(n, czk_fr_gsz_open(n->ctx, (const uint64_t*)n->gather.p, W, cnt, degrees, degree, out_value, out_bad));
    return CZK_OK;
}
// gsz20::batch_king_compute's two exchanges around the king's open, the same way
int gsz_king_trip(czk_net* n, const uint64_t* val, size_t cnt, const uint32_t* degrees, unsigned degree, uint64_t* out, unsigned long long* bad, uint64_t* out_bad) {
    const size_t W = (size_t)n->world;
    const bool king = n->rank == 0;
    // the king's scratch: world gathered lanes, then world identical answers (`vec![output; n]`, gsz20/mod.rs:508-512)
    if (king) CZK_TRY(net_buf(n, n->gather, 2 * W * cnt * 32));
    uint64_t* g = (uint64_t*)n->gather.p;
    CZK_TRY(czk_net_send_to_king(n, val, cnt * 32, king ? g : nullptr, CZK_MEM_DEVICE));
    uint64_t* ans = king ? g + 4 * W * cnt : nullptr;
    if (king) {
        // open_degree_vec per element, f = identity
        if (bad) NET_CTX(n, gsz_open_enqueue(n->ctx, (const u64*)g, W, cnt, degrees, degree, (u64*)ans, bad));
        else NET_CTX(n, czk_fr_gsz_open(n->ctx, g, W, cnt, degrees, degree, ans, out_bad));
        for (size_t p = 1; p < W; p++)
            NET_HIP(n, hipMemcpyAsync(ans + 4 * cnt * p, ans, cnt * 32, hipMemcpyDeviceToDevice, n->ctx->stream));
    }
    return czk_net_recv_from_king(n, ans, cnt * 32, out, CZK_MEM_DEVICE);
}
}  // namespace

extern "C" int czk_gsz_batch_open(czk_net* n, const uint64_t* val, size_t cnt, const uint32_t* degrees, unsigned degree, uint64_t* out_value,
                                  uint64_t* out_bad) {
    CZK_TRY(open_args(n, val, out_value, cnt));
    if (!out_bad) return net_err(n, CZK_ERR_ARG, "czk_gsz_batch_open: null out_bad");
    *out_bad = 0;
    if (!cnt) return CZK_OK;
    return gsz_open_trip(n, val, cnt, degrees, degree, out_value, nullptr, out_bad);
}

extern "C" int czk_fr_send_to_king(czk_net* n, const uint64_t* x, size_t cnt, uint64_t* gathered) {
    if (!n) return CZK_ERR_ARG;
    return czk_net_send_to_king(n, x, cnt * 32, gathered, CZK_MEM_DEVICE);
}
extern "C" int czk_fr_recv_from_king(czk_net* n, const uint64_t* parts, size_t cnt, uint64_t* out) {
    if (!n) return CZK_ERR_ARG;
    return czk_net_recv_from_king(n, parts, cnt * 32, out, CZK_MEM_DEVICE);
}

extern "C" int czk_gsz_batch_king_compute(czk_net* n, const uint64_t* val, size_t cnt, const uint32_t* degrees, unsigned degree, uint64_t* out,
                                          uint64_t* out_bad) {
    CZK_TRY(open_args(n, val, out, cnt));
    if (!out_bad) return net_err(n, CZK_ERR_ARG, "czk_gsz_batch_king_compute: null out_bad");
    *out_bad = 0;
    if (!cnt) return CZK_OK;
    return gsz_king_trip(n, val, cnt, degrees, degree, out, nullptr, out_bad);
}

// ---- FieldShare::batch_mul / batch_inv / partial_products for one party per communicator (share/field.rs:97-182; kernels in share_mul.hip) -----------------
// Every round is the reference's, in its order, except that the two independent opens of a batch_mul go out as ONE open of 2 cnt elements.
namespace {
struct NetShare {
    czk_net* n;
    size_t lpp;
    const uint64_t* mac_share;   // host; SPDZ only
    Fr ms;
    int flags;
    uint64_t bad = 0;
};
int net_share_args(czk_net* n, const char* what, size_t lpp, const uint64_t* mac_share, bool null_vec, size_t cnt, int flags, uint64_t* out_bad, uint64_t* out_zero,
                   NetShare* s, bool* work) {
    *work = false;
    CZK_TRY(need_ctx(n, what));
    if (!out_bad || !out_zero) return net_err(n, CZK_ERR_ARG, std::string(what) + ": null count output");
    *out_bad = *out_zero = 0;
    if (lpp != 1 && lpp != 2) return net_err(n, CZK_ERR_ARG, std::string(what) + ": lpp is 1 (additive) or 2 (SPDZ)");
    if (!cnt) return CZK_OK;
    if (null_vec || (lpp == 2 && !mac_share)) return net_err(n, CZK_ERR_ARG, std::string(what) + ": null argument");
    if (cnt > ((size_t)1 << 54)) return net_err(n, CZK_ERR_SIZE, std::string(what) + ": the lane arrays' byte count overflows");
    NET_HIP(n, hipSetDevice(n->ctx->device));
    s->n = n, s->lpp = lpp, s->mac_share = mac_share, s->flags = flags;
    s->ms = lpp == 2 ? host_fr(mac_share) : Fr::zero();
    *work = true;
    return CZK_OK;
}
// the scheme's batch_open of this party's lanes (cnt apart); failed MAC checks add up in s.bad
int net_share_open(NetShare& s, const u64* lanes, size_t cnt, u64* out_value) {
    if (s.lpp == 1) return czk_add_batch_open(s.n, lanes, cnt, out_value);
    uint64_t b = 0;
    CZK_TRY(czk_spdz_batch_open(s.n, lanes, lanes + 4 * cnt, s.mac_share, cnt, out_value, s.flags, &b));
    s.bad += b;
    return CZK_OK;
}
size_t net_share_mul_ws(size_t lpp, size_t cnt) { return (lpp + 1) * 2 * cnt * 32; }
// ws: lpp x 2 cnt masked factors, then the 2 cnt opened values
int net_share_mul(NetShare& s, ShareVec x, ShareVec y, const u64* tx, const u64* ty, const u64* tz, size_t T, size_t first, u64* ws, u64* out, size_t cnt) {
    czk_net* n = s.n;
    u64* opened = ws + 4 * s.lpp * 2 * cnt;
    const ShareVec vx{tx + 4 * first, T, 1}, vy{ty + 4 * first, T, 1}, vz{tz + 4 * first, T, 1};
    NET_CTX(n, share_mask_launch(n->ctx, (unsigned)s.lpp, x, y, vx, vy, ws, cnt));
    CZK_TRY(net_share_open(s, ws, 2 * cnt, opened));
    NET_CTX(n, share_combine_launch(n->ctx, (unsigned)s.lpp, n->rank == 0, s.ms, opened, vx, vy, vz, out, cnt, cnt));
    return CZK_OK;
}
}  // namespace

extern "C" int czk_net_share_batch_mul(czk_net* n, size_t lpp, const uint64_t* mac_share, const uint64_t* x, const uint64_t* y, const uint64_t* tx,
                                       const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t cnt, int flags, uint64_t* out_bad, uint64_t* out_zero) {
    NetShare s;
    bool work;
    CZK_TRY(net_share_args(n, "czk_net_share_batch_mul", lpp, mac_share, !x || !y || !tx || !ty || !tz || !out, cnt, flags, out_bad, out_zero, &s, &work));
    if (!work) return CZK_OK;
    StageHold ws(n->ctx);
    NET_CTX(n, ws.take(net_share_mul_ws(lpp, cnt)));
    CZK_TRY(net_share_mul(s, ShareVec{x, cnt, 1}, ShareVec{y, cnt, 1}, tx, ty, tz, cnt, 0, (u64*)ws.b.p, out, cnt));
    NET_HIP(n, hipStreamSynchronize(n->ctx->stream));   // like the opens: the call's outputs are complete when it returns
    *out_bad = s.bad;
    return CZK_OK;
}

extern "C" int czk_net_share_batch_inv(czk_net* n, size_t lpp, const uint64_t* mac_share, const uint64_t* x, const uint64_t* pb, const uint64_t* pc,
                                       const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t cnt, int flags, uint64_t* out_bad,
                                       uint64_t* out_zero) {
    NetShare s;
    bool work;
    CZK_TRY(net_share_args(n, "czk_net_share_batch_inv", lpp, mac_share, !x || !pb || !pc || !tx || !ty || !tz || !out, cnt, flags, out_bad, out_zero, &s, &work));
    if (!work) return CZK_OK;
    StageHold ws(n->ctx);
    NET_CTX(n, ws.take(net_share_mul_ws(lpp, cnt) + (lpp + 2) * cnt * 32));
    u64 *mulws = (u64*)ws.b.p, *prod = mulws + net_share_mul_ws(lpp, cnt) / 8, *v = prod + 4 * lpp * cnt, *vinv = v + 4 * cnt;
    CZK_TRY(net_share_mul(s, ShareVec{x, cnt, 1}, ShareVec{pb, cnt, 1}, tx, ty, tz, cnt, 0, mulws, prod, cnt));
    CZK_TRY(net_share_open(s, prod, cnt, v));
    NET_CTX(n, czk_fr_batch_inverse(n->ctx, v, cnt, nullptr, vinv, CZK_MEM_DEVICE));
    NET_CTX(n, share_counters(n->ctx));
    NET_CTX(n, share_scale_launch(n->ctx, (unsigned)lpp, ShareVec{pc, cnt, 1}, vinv, nullptr, out, cnt, cnt));
    NET_CTX(n, share_counters_read(n->ctx, nullptr, out_zero));
    *out_bad = s.bad;
    return CZK_OK;
}

extern "C" int czk_net_share_partial_products(czk_net* n, size_t lpp, const uint64_t* mac_share, const uint64_t* x, const uint64_t* pb, const uint64_t* pc,
                                              const uint64_t* tx, const uint64_t* ty, const uint64_t* tz, uint64_t* out, size_t cnt, int flags, uint64_t* out_bad,
                                              uint64_t* out_zero) {
    NetShare s;
    bool work;
    CZK_TRY(net_share_args(n, "czk_net_share_partial_products", lpp, mac_share, !x || !pb || !pc || !tx || !ty || !tz || !out, cnt, flags, out_bad, out_zero, &s,
                           &work));
    if (!work) return CZK_OK;
    const size_t T = 4 * cnt, P = 2 * cnt + 1;
    StageHold ws(n->ctx);
    NET_CTX(n, ws.take(net_share_mul_ws(lpp, cnt) + (2 * lpp + 4) * cnt * 32));
    u64 *mulws = (u64*)ws.b.p, *la = mulws + net_share_mul_ws(lpp, cnt) / 8, *lb = la + 4 * lpp * cnt, *mxm = lb + 4 * lpp * cnt, *run = mxm + 4 * cnt, *mms = run + 4 * cnt,
        *inv = mms + 4 * cnt;
    const ShareVec m_inv1{pc + 4, P, 1};                                                                     // m_inv[1..]
    CZK_TRY(net_share_mul(s, ShareVec{pb, P, 1}, ShareVec{x, cnt, 1}, tx, ty, tz, T, 0, mulws, la, cnt));   // mx = m[..n] x
    CZK_TRY(net_share_mul(s, ShareVec{la, cnt, 1}, m_inv1, tx, ty, tz, T, cnt, mulws, lb, cnt));            // mxm = mx m_inv[1..]
    CZK_TRY(net_share_open(s, lb, cnt, mxm));
    NET_CTX(n, czk_fr_prefix_product(n->ctx, mxm, cnt, run, CZK_MEM_DEVICE));                               // the local loop :169-172
    CZK_TRY(net_share_mul(s, ShareVec{pb, P, 0}, m_inv1, tx, ty, tz, T, 2 * cnt, mulws, la, cnt));          // mms = m_0 m_inv[1..]
    CZK_TRY(net_share_mul(s, ShareVec{la, cnt, 1}, ShareVec{pb + 4 * (cnt + 1), P, 1}, tx, ty, tz, T, 3 * cnt, mulws, lb, cnt));   // batch_inv(mms)
    CZK_TRY(net_share_open(s, lb, cnt, mms));
    NET_CTX(n, czk_fr_batch_inverse(n->ctx, mms, cnt, nullptr, inv, CZK_MEM_DEVICE));
    NET_CTX(n, share_counters(n->ctx));
    NET_CTX(n, share_scale_launch(n->ctx, (unsigned)lpp, ShareVec{pc + 4 * (cnt + 1), P, 1}, inv, run, out, cnt, cnt));
    NET_CTX(n, share_counters_read(n->ctx, nullptr, out_zero));
    *out_bad = s.bad;
    return CZK_OK;
}

// ---- gsz20's batch_mult / batch_inv / partial_products and its product check for one party per communicator (share/gsz20/mod.rs:559-594, :325-366,
// :596-808; kernels in gsz_mul.hip) ------------------------------------------------------------------------------------------------------------------------
// The party is the communicator's rank and holds ONE lane of every vector.  Every exchange is the reference's, in its dependency order; the king's open
// and the plain opens count their degree violations in ctx->share_cnt, read back once at the end of the call.
namespace {
struct NetGsz {
    czk_net* n;
    unsigned degree;
    const u64 *dr, *dr2, *rands;   // this party's lanes of the material
    unsigned long long* cnt;       // ctx->share_cnt
};
int net_gsz_args(czk_net* n, const char* what, unsigned degree, bool null_vec, size_t cnt, uint64_t* out_a, uint64_t* out_b, NetGsz* s, bool* work) {
    *work = false;
    CZK_TRY(need_ctx(n, what));
    if (!out_a || !out_b) return net_err(n, CZK_ERR_ARG, std::string(what) + ": null result output");
    *out_a = *out_b = 0;
    const size_t W = (size_t)n->world;
    if (W > 96) return net_err(n, CZK_ERR_SIZE, std::string(what) + ": more than 96 parties");
    u64 dom[12];
    NET_CTX(n, czk_share_domain_constants(n->ctx, W, dom));   // CZK_ERR_SIZE: no share domain of that size
    if (!cnt) return CZK_OK;
    if (null_vec) return net_err(n, CZK_ERR_ARG, std::string(what) + ": null argument");
    if (cnt > ((size_t)1 << 52) / W) return net_err(n, CZK_ERR_SIZE, std::string(what) + ": the lane arrays' byte count overflows");
    NET_HIP(n, hipSetDevice(n->ctx->device));
    NET_CTX(n, share_counters(n->ctx));
    s->n = n, s->degree = degree < W ? degree : (unsigned)W, s->cnt = n->ctx->share_cnt;
    *work = true;
    return CZK_OK;
}
int net_gsz_king(NetGsz& s, const u64* val, size_t cnt, u64* out) { return gsz_king_trip(s.n, val, cnt, nullptr, 2 * s.degree, out, s.cnt, nullptr); }
int net_gsz_open(NetGsz& s, const u64* val, size_t cnt, u64* out_value) { return gsz_open_trip(s.n, val, cnt, nullptr, s.degree, out_value, s.cnt, nullptr); }
// one batch_mult with doubles [d_first, d_first + cnt): ws = 2 cnt elements; out = this party's share of x y
int net_gsz_mul(NetGsz& s, ShareVec x, ShareVec y, size_t d_first, u64* ws, u64* out, size_t cnt) {
    u64 *d = ws, *v = ws + 4 * cnt;
    NET_CTX(s.n, gsz_net_mask_launch(s.n->ctx, x, y, s.dr2 + 4 * d_first, d, cnt));
    CZK_TRY(net_gsz_king(s, d, cnt, v));
    NET_CTX(s.n, gsz_net_unmask_launch(s.n->ctx, v, s.dr + 4 * d_first, out, cnt));
    return CZK_OK;
}
// open(batch_mult(x, y)): the product's share goes from the workspace straight to the broadcast; opened: cnt values
int net_gsz_mul_open(NetGsz& s, ShareVec x, ShareVec y, size_t d_first, u64* ws, u64* opened, size_t cnt) {
    CZK_TRY(net_gsz_mul(s, x, y, d_first, ws, ws, cnt));   // (v - r lands on the masked values, which the king already has)
    return net_gsz_open(s, ws, cnt, opened);
}
// batch_inv (:325-342) with rs = rands [r_first, ..), doubles [d_first, ..): ws = 4 cnt elements; out = rs / open(x rs) (times prefix, when given)
int net_gsz_inv(NetGsz& s, ShareVec x, size_t d_first, size_t r_first, u64* ws, const u64* prefix, u64* out, size_t cnt) {
    const ShareVec rs{s.rands + 4 * r_first, 0, 1};
    u64 *v = ws + 4 * 2 * cnt, *vinv = v + 4 * cnt;
    CZK_TRY(net_gsz_mul_open(s, x, rs, d_first, ws, v, cnt));
    NET_CTX(s.n, czk_fr_batch_inverse(s.n->ctx, v, cnt, nullptr, vinv, CZK_MEM_DEVICE));
    NET_CTX(s.n, share_scale_launch(s.n->ctx, 1, rs, vinv, prefix, out, cnt, cnt));
    return CZK_OK;
}
}  // namespace

extern "C" int czk_net_gsz_share_batch_mul(czk_net* n, unsigned degree, const uint64_t* x, const uint64_t* y, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                                           uint64_t* out, size_t cnt, uint64_t* out_bad, uint64_t* out_zero) {
    NetGsz s;
    bool work;
    CZK_TRY(net_gsz_args(n, "czk_net_gsz_share_batch_mul", degree, !x || !y || !doubles_r || !doubles_r2 || !out, cnt, out_bad, out_zero, &s, &work));
    if (!work) return CZK_OK;
    s.dr = doubles_r, s.dr2 = doubles_r2, s.rands = nullptr;
    StageHold ws(n->ctx);
    NET_CTX(n, ws.take(2 * cnt * 32));
    CZK_TRY(net_gsz_mul(s, ShareVec{x, 0, 1}, ShareVec{y, 0, 1}, 0, (u64*)ws.b.p, out, cnt));
    NET_CTX(n, share_counters_read(n->ctx, out_bad, out_zero));
    return CZK_OK;
}

extern "C" int czk_net_gsz_share_batch_inv(czk_net* n, unsigned degree, const uint64_t* x, const uint64_t* doubles_r, const uint64_t* doubles_r2, const uint64_t* rands,
                                           uint64_t* out, size_t cnt, uint64_t* out_bad, uint64_t* out_zero) {
    NetGsz s;
    bool work;
    CZK_TRY(net_gsz_args(n, "czk_net_gsz_share_batch_inv", degree, !x || !doubles_r || !doubles_r2 || !rands || !out, cnt, out_bad, out_zero, &s, &work));
    if (!work) return CZK_OK;
    s.dr = doubles_r, s.dr2 = doubles_r2, s.rands = rands;
    StageHold ws(n->ctx);
    NET_CTX(n, ws.take(4 * cnt * 32));
    CZK_TRY(net_gsz_inv(s, ShareVec{x, 0, 1}, 0, 0, (u64*)ws.b.p, nullptr, out, cnt));
    NET_CTX(n, share_counters_read(n->ctx, out_bad, out_zero));
    return CZK_OK;
}

extern "C" int czk_net_gsz_share_partial_products(czk_net* n, unsigned degree, const uint64_t* x, const uint64_t* doubles_r, const uint64_t* doubles_r2,
                                                  const uint64_t* rands, uint64_t* out, size_t cnt, uint64_t* out_bad, uint64_t* out_zero) {
    NetGsz s;
    bool work;
    CZK_TRY(net_gsz_args(n, "czk_net_gsz_share_partial_products", degree, !x || !doubles_r || !doubles_r2 || !rands || !out, cnt, out_bad, out_zero, &s, &work));
    if (!work) return CZK_OK;
    s.dr = doubles_r, s.dr2 = doubles_r2, s.rands = rands;
    const size_t c1 = cnt + 1;
    StageHold ws(n->ctx);
    NET_CTX(n, ws.take((4 * c1 + c1 + 3 * cnt) * 32));
    u64 *mulws = (u64*)ws.b.p, *m_inv = mulws + 4 * 4 * c1, *lane = m_inv + 4 * c1, *mxm = lane + 4 * cnt, *run = mxm + 4 * cnt;
    const ShareVec m{rands, 0, 1}, m0{rands, 0, 0}, m_inv1{m_inv + 4, 0, 1};                                            // m = rands [0, n]; m_inv[1..]
    CZK_TRY(net_gsz_inv(s, m, 0, cnt + 1, mulws, nullptr, m_inv, c1));                                                   // m_inv = batch_inv(m)
    CZK_TRY(net_gsz_mul(s, m, ShareVec{x, 0, 1}, cnt + 1, mulws, lane, cnt));                                            // mx = m[..n] x
    CZK_TRY(net_gsz_mul_open(s, ShareVec{lane, 0, 1}, m_inv1, 2 * cnt + 1, mulws, mxm, cnt));                            // open(mx m_inv[1..])
    NET_CTX(n, czk_fr_prefix_product(n->ctx, mxm, cnt, run, CZK_MEM_DEVICE));                                            // the local loop :353-356
    CZK_TRY(net_gsz_mul(s, m0, m_inv1, 3 * cnt + 1, mulws, lane, cnt));                                                  // mms = m_0 m_inv[1..]
    CZK_TRY(net_gsz_inv(s, ShareVec{lane, 0, 1}, 4 * cnt + 1, 2 * cnt + 2, mulws, run, out, cnt));                       // batch_inv(mms), scaled by the running product
    NET_CTX(n, share_counters_read(n->ctx, out_bad, out_zero));
    return CZK_OK;
}

extern "C" int czk_net_gsz_product_check(czk_net* n, unsigned degree, const uint64_t* xs, const uint64_t* ys, const uint64_t* zs, size_t cnt, const uint64_t* doubles_r,
                                         const uint64_t* doubles_r2, const uint64_t* rands, uint64_t* out_ok, uint64_t* out_bad) {
    NetGsz s;
    bool work;
    CZK_TRY(net_gsz_args(n, "czk_net_gsz_product_check", degree, !xs || !ys || !zs || !doubles_r || !doubles_r2 || !rands, cnt, out_ok, out_bad, &s, &work));
    *out_ok = 1;   // no triples: nothing to refute
    if (!work) return CZK_OK;
    if (cnt >> 32) return net_err(n, CZK_ERR_SIZE, "czk_net_gsz_product_check: more than 2^32 - 1 triples");
    czk_ctx* ctx = n->ctx;
    unsigned R = 0;
    while (((size_t)1 << R) < cnt) R++;
    StageHold ws(ctx);
    NET_CTX(n, ws.take(gsz_net_check_ws(ctx, cnt) * 32));
    GszNetCheck c;
    gsz_net_check_carve(ctx, c, (u64*)ws.b.p, cnt, doubles_r, doubles_r2, rands);
    CZK_TRY(net_gsz_open(s, rands, 1, c.coin));                       // the hadamard coin (:601): the triples were committed before the call
    NET_CTX(n, gsz_net_check_hadamard(ctx, c, xs, ys, zs));
    for (unsigned round = 0; round < R; round++) {
        NET_CTX(n, gsz_net_check_round_send(ctx, c));
        CZK_TRY(net_gsz_king(s, c.wire, 2, c.king));                  // ip_l and ip3 in ONE round trip (both ip_compute calls precede the coin, :757, :690-692)
        CZK_TRY(net_gsz_open(s, rands + 4 * c.r0, 1, c.opened));      // only now the round's coin
        NET_CTX(n, gsz_net_check_round_recv(ctx, c));
    }
    NET_CTX(n, gsz_net_check_final(ctx, c, 0));
    CZK_TRY(net_gsz_king(s, c.wire, 3, c.king));                      // mult(xr, yr), mult(x, xr), mult(y, yr)
    NET_CTX(n, gsz_net_check_final(ctx, c, 1));
    CZK_TRY(net_gsz_king(s, c.wire, 1, c.king));                      // mult(ip, ip_r) needs the first trip's answer
    NET_CTX(n, gsz_net_check_final(ctx, c, 2));
    CZK_TRY(net_gsz_open(s, c.blind, 3, c.opened));                   // the three blinded values in one broadcast
    NET_CTX(n, gsz_net_check_final(ctx, c, 3));
    uint64_t failed = 0;
    NET_CTX(n, share_counters_read(ctx, out_bad, &failed));          // the one read-back of the check
    *out_ok = failed ? 0 : 1;
    return CZK_OK;
}

// ---- czk_net_gsz_dn_*: the GSZ material dealt and extracted with one party per communicator (kernels in gsz_dn.hip) --------------------------------------
// The party deals under its OWN key alone; one all-to-all carries its shares out and the others' in; the extraction is local.  No rank sees another's key.
extern "C" int czk_net_gsz_dn_generate(czk_net* n, int kind, unsigned degree, const uint8_t* key, const uint8_t* nonce, size_t deal, uint64_t* out_r, uint64_t* out_r2) {
    CZK_TRY(need_ctx(n, "czk_net_gsz_dn_generate"));
    czk_ctx* ctx = n->ctx;
    const size_t W = (size_t)n->world;
    NET_CTX(n, gsz_dn_shape(ctx, "czk_net_gsz_dn_generate", kind, W, degree, deal));
    if (!deal) return CZK_OK;
    const bool doubles = kind == CZK_GSZ_DN_DOUBLES;
    if (!key || !nonce || !out_r || (doubles && !out_r2)) return net_err(n, CZK_ERR_ARG, "czk_net_gsz_dn_generate: null argument");
    NET_HIP(n, hipSetDevice(ctx->device));
    const size_t per = (doubles ? 2 : 1) * deal;   // elements per peer
    StageHold ws(ctx);
    NET_CTX(n, ws.take((96 + 2 * W * per) * 32));
    u64 *points = (u64*)ws.b.p, *send = points + 4 * 96, *recv = send + 4 * W * per;
    NET_CTX(n, gsz_dn_points_launch(ctx, W, points));
    NET_CTX(n, gsz_dn_deal_launch(ctx, kind, W, degree, key, nonce, deal, points, send));
    CZK_TRY(czk_net_alltoall(n, send, per * 32, recv, CZK_MEM_DEVICE));
    NET_CTX(n, gsz_dn_extract_launch(ctx, kind, W, degree, deal, points, recv, out_r, doubles ? out_r2 : nullptr));
    return CZK_OK;
}

extern "C" int czk_net_gsz_dn_check(czk_net* n, int kind, unsigned degree, const uint64_t* r, const uint64_t* r2, size_t outputs, uint64_t* out_ok, uint64_t* out_bad) {
    CZK_TRY(need_ctx(n, "czk_net_gsz_dn_check"));
    if (!out_ok || !out_bad) return net_err(n, CZK_ERR_ARG, "czk_net_gsz_dn_check: null result output");
    *out_ok = *out_bad = 0;
    czk_ctx* ctx = n->ctx;
    NET_CTX(n, gsz_dn_shape(ctx, "czk_net_gsz_dn_check", kind, (size_t)n->world, degree, 0));
    const bool doubles = kind == CZK_GSZ_DN_DOUBLES;
    if (outputs < 3) return net_err(n, CZK_ERR_ARG, "czk_net_gsz_dn_check: fewer than 3 outputs (two are sacrificed)");
    if (!r || (doubles && !r2)) return net_err(n, CZK_ERR_ARG, "czk_net_gsz_dn_check: null argument");
    if (outputs >> 32) return net_err(n, CZK_ERR_SIZE, "czk_net_gsz_dn_check: more than 2^32 - 1 outputs");
    NET_HIP(n, hipSetDevice(ctx->device));
    const size_t cws = gsz_dn_combine_ws(ctx, 1, outputs);
    StageHold ws(ctx);
    NET_CTX(n, ws.take((cws + 5) * 32));
    u64 *u = (u64*)ws.b.p + 4 * cws, *coin = u + 4 * 2, *opened = coin + 4;
    NET_CTX(n, share_counters(ctx));
    CZK_TRY(gsz_open_trip(n, r + 4 * (outputs - 2), 1, nullptr, degree, coin, ctx->share_cnt, nullptr));   // the coin: the first sacrificed output, opened
    NET_CTX(n, gsz_dn_combine_launch(ctx, 1, r, doubles ? r2 : nullptr, outputs, outputs, coin, (u64*)ws.b.p, u));
    CZK_TRY(gsz_open_trip(n, u, 1, nullptr, degree, opened, ctx->share_cnt, nullptr));
    if (doubles) {
        CZK_TRY(gsz_open_trip(n, u + 4, 1, nullptr, 2 * degree, opened + 4, ctx->share_cnt, nullptr));
        NET_CTX(n, gsz_dn_verdict_launch(ctx, opened));
    }
    uint64_t differ = 0;
    NET_CTX(n, share_counters_read(ctx, out_bad, &differ));   // the one read-back of the check
    *out_ok = (differ || *out_bad) ? 0 : 1;
    return CZK_OK;
}
