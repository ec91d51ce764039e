// pairing_demo.cpp -- include/czk.hpp's pairing mirror end to end (tests/test_pairing.py compares its output with Python):
//   line 1: e(G1, G2) as 72 hex u64 limbs (czk.h's Fq12 layout, Montgomery)
//   line 2: "verify 1" -- verify_proof of a proof whose discrete logs satisfy a b = alpha beta + (abc_0 + x abc_1) gamma + c delta
//   line 3: "verify 0" -- the same proof with a wrong public input
// Points come from czk_fixed_base_points (canonical scalars), so the demo needs no curve arithmetic of its own.
#include <cstdio>
#include <vector>

#include "czk.hpp"

using namespace czk;

static G1AffinePoint g1(const Context& ctx, BigInteger256 k) {
    G1AffinePoint p;
    ctx.check(czk_fixed_base_points(ctx.raw(), CZK_G1, k.l, 1, p.x.l, CZK_MEM_HOST));
    return p;
}
static G2AffinePoint g2(const Context& ctx, BigInteger256 k) {
    G2AffinePoint p;
    ctx.check(czk_fixed_base_points(ctx.raw(), CZK_G2, k.l, 1, p.x.c0.l, CZK_MEM_HOST));
    return p;
}
static BigInteger256 small(uint64_t v) { return BigInteger256{{v, 0, 0, 0}}; }

int main() {
    try {
        Context ctx(0);
        const Fq12 e = Bls12_377::pairing(ctx, g1(ctx, small(1)), g2(ctx, small(1)));
        const uint64_t* w = &e.c0.c0.c0.l[0];
        for (int i = 0; i < 72; i++) std::printf("%016llx%c", (unsigned long long)w[i], i == 71 ? '\n' : ' ');
        // alpha, beta, gamma, delta = 11, 13, 17, 19; gamma_abc = 31, 37; x = 29; a = 41, c = 23, b = (alpha beta + (31 + 29 * 37) gamma + c delta) / a mod r
        VerifyingKey vk{g1(ctx, small(11)), g2(ctx, small(13)), g2(ctx, small(17)), g2(ctx, small(19)), {g1(ctx, small(31)), g1(ctx, small(37))}};
        const BigInteger256 b{{0x8bb7863e7063e8dfull, 0x145952d985da895eull, 0x5f0a4e521cc5644cull, 0x0feff8e05e261cc0ull}};
        const Proof proof{g1(ctx, small(41)), g2(ctx, b), g1(ctx, small(23))};
        auto pvk = prepare_verifying_key(ctx, vk);
        const Fr x29{{0x62dc7ffffffffe73ull, 0xf2a576d76ffffe63ull, 0x086467eafda40de7ull, 0x0c33cc4ae8c3990cull}};   // 29, Montgomery
        const Fr x30{{0xd5e77ffffffffe65ull, 0x0b52f4e80ffffe54ull, 0xbe883041f2986dd5ull, 0x06d4411e7a528e52ull}};   // 30, Montgomery
        std::printf("verify %d\n", verify_proof(*pvk, proof, {x29}) ? 1 : 0);
        std::printf("verify %d\n", verify_proof(*pvk, proof, {x30}) ? 1 : 0);
    } catch (const Panic& p) {
        std::fprintf(stderr, "panic %d: %s\n", p.code, p.what());
        return 1;
    }
    return 0;
}
