// merkle_hash.h -- the two hashes of the reference's binary SHA-256 tree (mpc-algebra/src/com.rs:36-59) and the tree's layout, for merkle.hip and the
// tree form kept under lab/.
//
//   leaf_i = SHA256(bytes(a[i]))          32 bytes: one block, the padding behind the element
//   node   = SHA256(left || right)        64 bytes: one block of data and one block of padding
//
// A digest is eight state words, which ARE the big-endian words of its bytes; in memory it is its 32 bytes in digest order, i.e. the words byte-swapped.
// A tree of n = 2^k leaves is 2n - 1 digests per lane: level L (n >> L digests) starts at digest merkle_level_offset(n, L).
#pragma once
#include "sha256_dev.h"

namespace czk {
namespace {

__device__ __forceinline__ void sha256_init(u32 (&st)[8]) {   // FIPS 180-4 section 5.3.3
    st[0] = 0x6a09e667u, st[1] = 0xbb67ae85u, st[2] = 0x3c6ef372u, st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu, st[5] = 0x9b05688cu, st[6] = 0x1f83d9abu, st[7] = 0x5be0cd19u;
}

__host__ __device__ __forceinline__ size_t merkle_level_offset(size_t n, unsigned level) { return 2 * n - 2 * (n >> level); }

// SHA256 of the 32 canonical little-endian bytes of one Montgomery element
__device__ __forceinline__ void merkle_leaf_hash(const Fr& mont, u32 (&st)[8]) {
    const Fr v = fp_into_repr(mont);
    u32 w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(v.l[j]);
    sha256_init(st);
    w[8] = 0x80000000u;
#pragma unroll
    for (int j = 9; j < 15; j++) w[j] = 0;
    w[15] = 256;
    sha256_block(st, w);
}

// SHA256(left || right); w holds the two digests as sixteen state words on entry (and is used up)
__device__ __forceinline__ void merkle_node_hash(u32 (&w)[16], u32 (&st)[8]) {
    sha256_init(st);
    sha256_block(st, w);
    w[0] = 0x80000000u;
#pragma unroll
    for (int j = 1; j < 15; j++) w[j] = 0;
    w[15] = 512;
    sha256_block(st, w);
}

// a digest in memory (32 bytes, 16-byte aligned) <-> state words
__device__ __forceinline__ void merkle_load_digest(const u32* p, u32* w) {
    const uint4 lo = ((const uint4*)p)[0], hi = ((const uint4*)p)[1];
    w[0] = __builtin_bswap32(lo.x), w[1] = __builtin_bswap32(lo.y), w[2] = __builtin_bswap32(lo.z), w[3] = __builtin_bswap32(lo.w);
    w[4] = __builtin_bswap32(hi.x), w[5] = __builtin_bswap32(hi.y), w[6] = __builtin_bswap32(hi.z), w[7] = __builtin_bswap32(hi.w);
}
__device__ __forceinline__ void merkle_store_digest(u32* p, const u32 (&st)[8]) {
    ((uint4*)p)[0] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]), __builtin_bswap32(st[3]));
    ((uint4*)p)[1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]), __builtin_bswap32(st[7]));
}

constexpr unsigned MERKLE_BLOCKS_PER_CU = 8;   // grid limit of the tree kernels' grid-stride loops, in blocks of 256 threads per compute unit
inline size_t merkle_max_blocks(const czk_ctx* ctx) { return (size_t)ctx->num_cu * MERKLE_BLOCKS_PER_CU; }

}  // namespace
}  // namespace czk
