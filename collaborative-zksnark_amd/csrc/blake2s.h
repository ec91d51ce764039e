// blake2s.h -- BLAKE2s-256 (RFC 7693: 64-byte blocks, 32-byte digest, no key, no salt, no personalisation): the hash of the reference's FiatShamirRng<Blake2s>
// (marlin/src/rng.rs) behind czk_blake2s and the transcripts of fs.hip.  One compression function and the streaming wrapper, host and device code.
// The last-block rule: the final flag goes on the block that holds the message's last byte, so a full buffer is only compressed once more input arrives --
// a message of 64 j bytes ends on its j-th full block and gets no empty block after it; the empty message is one zero block with counter 0.
#pragma once
#include "field.h"

namespace czk {

CZK_HD u32 blake2s_iv(int i) {
    constexpr u32 iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    return iv[i];
}
// RFC 7693 section 2.7, two 4-bit indices per byte (row r, entries 2k and 2k + 1 in byte k: low nibble first)
CZK_HD unsigned blake2s_sigma(int r, int i) {
    constexpr uint8_t s[10][8] = {{0x10, 0x32, 0x54, 0x76, 0x98, 0xba, 0xdc, 0xfe}, {0xae, 0x84, 0xf9, 0x6d, 0xc1, 0x20, 0x7b, 0x35}, {0x8b, 0x0c, 0x25, 0xdf, 0xea, 0x63, 0x17, 0x49},
                                  {0x97, 0x13, 0xcd, 0xeb, 0x62, 0xa5, 0x04, 0x8f}, {0x09, 0x75, 0x42, 0xfa, 0x1e, 0xcb, 0x86, 0xd3}, {0xc2, 0xa6, 0xb0, 0x38, 0xd4, 0x57, 0xef, 0x91},
                                  {0x5c, 0xf1, 0xde, 0xa4, 0x70, 0x36, 0x29, 0xb8}, {0xbd, 0xe7, 0x1c, 0x93, 0x05, 0x4f, 0x68, 0xa2}, {0xf6, 0x9e, 0x3b, 0x80, 0x2c, 0x7d, 0x41, 0x5a},
                                  {0x2a, 0x48, 0x67, 0x51, 0xbf, 0xe9, 0xc3, 0x0d}};
    const unsigned b = s[r][i >> 1];
    return (i & 1) ? b >> 4 : b & 15;
}

struct Blake2s {
    u32 h[8];
    u32 t[2];         // bytes compressed so far plus those of the block being compressed, low word first
    u32 fill;         // bytes waiting in buf: 1 .. 64 once anything was put, 0 only for the empty message
    uint8_t buf[64];

    CZK_HD void init() {
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = blake2s_iv(i);
        h[0] ^= 0x01010020u;   // digest length 32, key length 0, fanout 1, depth 1
        t[0] = t[1] = fill = 0;
    }
    static CZK_HD u32 rotr(u32 x, unsigned n) { return __builtin_rotateright32(x, n); }
    // F (RFC 7693 section 3.2) on the block in buf; t already counts its bytes
    CZK_HD void compress(bool last) {
        u32 m[16], v[16];
#pragma unroll
        for (int i = 0; i < 16; i++) m[i] = (u32)buf[4 * i] | (u32)buf[4 * i + 1] << 8 | (u32)buf[4 * i + 2] << 16 | (u32)buf[4 * i + 3] << 24;
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = h[i], v[8 + i] = blake2s_iv(i);
        v[12] ^= t[0];
        v[13] ^= t[1];
        if (last) v[14] = ~v[14];
#define CZK_B2S_G(a, b, c, d, x, y)                                        \
    v[a] += v[b] + (x), v[d] = rotr(v[d] ^ v[a], 16), v[c] += v[d], v[b] = rotr(v[b] ^ v[c], 12), \
    v[a] += v[b] + (y), v[d] = rotr(v[d] ^ v[a], 8), v[c] += v[d], v[b] = rotr(v[b] ^ v[c], 7)
#pragma unroll   // (unrolled: the message schedule becomes constant indices, m stays in registers)
        for (int r = 0; r < 10; r++) {
            CZK_B2S_G(0, 4, 8, 12, m[blake2s_sigma(r, 0)], m[blake2s_sigma(r, 1)]);
            CZK_B2S_G(1, 5, 9, 13, m[blake2s_sigma(r, 2)], m[blake2s_sigma(r, 3)]);
            CZK_B2S_G(2, 6, 10, 14, m[blake2s_sigma(r, 4)], m[blake2s_sigma(r, 5)]);
            CZK_B2S_G(3, 7, 11, 15, m[blake2s_sigma(r, 6)], m[blake2s_sigma(r, 7)]);
            CZK_B2S_G(0, 5, 10, 15, m[blake2s_sigma(r, 8)], m[blake2s_sigma(r, 9)]);
            CZK_B2S_G(1, 6, 11, 12, m[blake2s_sigma(r, 10)], m[blake2s_sigma(r, 11)]);
            CZK_B2S_G(2, 7, 8, 13, m[blake2s_sigma(r, 12)], m[blake2s_sigma(r, 13)]);
            CZK_B2S_G(3, 4, 9, 14, m[blake2s_sigma(r, 14)], m[blake2s_sigma(r, 15)]);
        }
#undef CZK_B2S_G
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
    }
    CZK_HD void count(u32 n) {
        t[0] += n;
        if (t[0] < n) t[1]++;
    }
    CZK_HD void update(const uint8_t* p, size_t n) {
        while (n) {
            if (fill == 64) {   // more input follows: this block is not the last
                count(64);
                compress(false);
                fill = 0;
            }
            size_t take = 64 - fill;
            if (take > n) take = n;
            for (size_t i = 0; i < take; i++) buf[fill + i] = p[i];
            fill += (u32)take, p += take, n -= take;
        }
    }
    // the message's length so far, in bytes (mod 2^64)
    CZK_HD u64 length() const { return ((u64)t[1] << 32 | t[0]) + fill; }
    CZK_HD void finish(uint8_t* out32) {
        count(fill);
        for (u32 i = fill; i < 64; i++) buf[i] = 0;
        compress(true);
#pragma unroll
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 4; j++) out32[4 * i + j] = (uint8_t)(h[i] >> (8 * j));
    }
};

}  // namespace czk
