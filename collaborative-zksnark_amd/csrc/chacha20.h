// chacha20.h -- the ChaCha20 block function (RFC 8439 section 2.3: 20 rounds = 10 column / diagonal double rounds), shared by the keyed generator of
// gsz_dn.hip (a 32-bit counter and a 96-bit nonce, RFC 8439's layout) and the Fiat-Shamir generator of fs.hip (rand_chacha's layout: a 64-bit block counter
// in words 12-13, the stream id in words 14-15).  Host and device code; the state stays in registers.
#pragma once
#include "field.h"

namespace czk {

CZK_HD u32 chacha_rotl(u32 x, unsigned n) { return __builtin_rotateleft32(x, n); }
#define CZK_CHACHA_QR(a, b, c, d)                  \
    a += b, d ^= a, d = chacha_rotl(d, 16);        \
    c += d, b ^= c, b = chacha_rotl(b, 12);        \
    a += b, d ^= a, d = chacha_rotl(d, 8);         \
    c += d, b ^= c, b = chacha_rotl(b, 7)

// the 20 rounds on x, in place (the caller adds the input words: out[i] = x[i] + in[i])
CZK_HD void chacha20_rounds(u32* x) {
#pragma unroll 1
    for (int round = 0; round < 10; round++) {
        CZK_CHACHA_QR(x[0], x[4], x[8], x[12]);
        CZK_CHACHA_QR(x[1], x[5], x[9], x[13]);
        CZK_CHACHA_QR(x[2], x[6], x[10], x[14]);
        CZK_CHACHA_QR(x[3], x[7], x[11], x[15]);
        CZK_CHACHA_QR(x[0], x[5], x[10], x[15]);
        CZK_CHACHA_QR(x[1], x[6], x[11], x[12]);
        CZK_CHACHA_QR(x[2], x[7], x[8], x[13]);
        CZK_CHACHA_QR(x[3], x[4], x[9], x[14]);
    }
}
#undef CZK_CHACHA_QR

// out = the 16 little-endian keystream words of the block with the four words w12 .. w15 under `key`
CZK_HD void chacha20_block(const u32* key, u32 w12, u32 w13, u32 w14, u32 w15, u32* out) {
    const u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7], w12, w13, w14, w15};
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = in[i];
    chacha20_rounds(out);
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] += in[i];
}

}  // namespace czk
