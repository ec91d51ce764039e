// pow_tables.h -- domain elements from per-byte power tables, shared by marlin_index.hip (w = the generator of H) and plonk_layout.hip (w = the generator
// of the mixed-radix wire domain): four tables of 256 powers, T_j[b] = w^(b 2^(8 j)), built on the device per call (1024 field elements); w^e is the
// product of one entry per byte of e, so nothing of the domain's size is built or crosses from the host.  The kernel is `static`: each translation unit
// that includes this header launches its own copy (the libraries are built without relocatable device code).
#pragma once
#include "czk_internal.h"

namespace czk {

struct MarlinRoots {
    Fr w[4];   // w^(2^(8 j))
};

// host: the four roots of a generator, w^(2^(8 j)) by eight squarings each
inline MarlinRoots pow_table_roots(const Fr& w) {
    MarlinRoots roots;
    roots.w[0] = w;
    for (int j = 1; j < 4; j++) {
        roots.w[j] = roots.w[j - 1];
        for (int s = 0; s < 8; s++) roots.w[j] = fp_sqr(roots.w[j]);
    }
    return roots;
}

static __global__ __launch_bounds__(256) void k_marlin_pow_tables(u64* tab, MarlinRoots roots) {   // 4 blocks of 256
    const unsigned j = blockIdx.x, b = threadIdx.x;
    fp_store<FrParams>(tab + 4 * (size_t)(256 * j + b), fp_pow_u64(roots.w[j], (u64)b));
}

// w^e for e < 2^32, nb = the number of bytes of the largest exponent = tables in use (every byte index stays inside a table for any e; the caller
// keeps e below the domain's size)
__device__ __forceinline__ Fr marlin_domain_element(const u64* tab, u32 e, unsigned nb) {
    Fr v = fp_load<FrParams>(tab + 4 * (size_t)(e & 255u));
    for (unsigned j = 1; j < nb; j++) v = fp_mul(v, fp_load<FrParams>(tab + 4 * (size_t)(256 * j + ((e >> (8 * j)) & 255u))));
    return v;
}

}  // namespace czk
