// marlin_index.hip -- the per-matrix step of Marlin's indexer on the GPU: arithmetize_matrix (marlin/src/ahp/constraint_systems.rs:152-262) up to the
// four evaluation vectors on K.  The interpolations on K, the transforms on B and the commitments that follow it are the library's NTT and MSM.
//
// For the entry t of a CSR matrix, in constraint row r at variable i:
//     row[t] = w^p,  col[t] = w^r,  val[t] = coeff[t] w^p / |H|,  row_col[t] = row[t] col[t]          (p = the variable's position on H, below)
// with w = get_root_of_unity(|H|).  row and col are swapped on purpose ("we are dealing with the transpose of M", :191-194).  The reference divides val
// by u_H(e, e) = |H| e^(|H| - 1) through a map and a batch inversion (:169-172, :195-204); on H that is e / |H|, so no inversion is needed here.
// Slots past the last entry hold row = col = row_col = 1, val = 0 (:207-211).
//
// Domain elements (pow_tables.h): four tables of 256 powers, T_j[b] = w^(b 2^(8 j)), built on the device per call (1024 field elements); w^e is the product of one entry
// per byte of e -- ceil(log|H| / 8) - 1 multiplications -- so nothing of size |H| is built or crosses from the host.  One thread per slot; the row of a
// slot is found by a binary search of row_ptr.
#include "pow_tables.h"

namespace czk {

// out: row | col | val | row_col, k Fr each.  The kernel reads nothing outside row_ptr[0..m], col_idx[0..nnz), coeff[0..nnz) and the tables whatever those
// arrays hold: the search ends on an index below m for any row_ptr, and exponents are reduced modulo |H| before they index a table.
__global__ __launch_bounds__(256) void k_marlin_arithmetize(const u64* row_ptr, const u32* col_idx, const u64* coeff, size_t m, size_t nnz, unsigned log_h,
                                                             unsigned log_x, u32 n_instance, Fr size_inv, const u64* tab, size_t k, u64* out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    Fr row = Fr::one(), col = Fr::one(), val = Fr::zero(), row_col = Fr::one();
    if (t < nnz && m) {
        // the last row whose offset is <= t: empty rows before, between and after the occupied ones share an offset with a neighbour and are passed over
        size_t lo = 0, hi = m;
        while (hi - lo > 1) {
            const size_t mid = lo + (hi - lo) / 2;
            if (row_ptr[mid] <= (u64)t) lo = mid;
            else hi = mid;
        }
        const unsigned nb = log_h > 8 ? (log_h + 7) / 8 : 1;
        const u32 mask = log_h >= 32 ? 0xffffffffu : (((u32)1 << log_h) - 1u);
        const u32 X = (u32)1 << log_x;
        u32 i = col_idx[t];
        if (i >= n_instance) i += X - n_instance;           // pad_input_for_indexer_and_prover: the padded inputs shift the witness columns
        u32 p;                                              // reindex_by_subdomain(H, X, i) (algebra/poly/src/domain/mod.rs:196-218)
        if (i < X) {
            p = i << (log_h - log_x);
        } else {
            const u32 j = i - X, x = ((u32)1 << (log_h - log_x)) - 1u;
            p = x ? j + j / x + 1u : j;
        }
        row = marlin_domain_element(tab, p & mask, nb);
        col = marlin_domain_element(tab, (u32)lo & mask, nb);
        val = fp_mul(fp_mul(fp_load<FrParams>(coeff + 4 * t), row), size_inv);
        row_col = fp_mul(row, col);
    }
    fp_store<FrParams>(out + 4 * t, row);
    fp_store<FrParams>(out + 4 * (k + t), col);
    fp_store<FrParams>(out + 4 * (2 * k + t), val);
    fp_store<FrParams>(out + 4 * (3 * k + t), row_col);
}

}  // namespace czk

using namespace czk;

extern "C" int czk_marlin_arithmetize(czk_ctx* ctx, const uint64_t* row_ptr, const uint32_t* col_idx, const uint64_t* coeff, size_t m, size_t nnz,
                                      unsigned log_h, unsigned log_x, size_t n_instance, size_t k, uint64_t* out, int mem) {
    if (!ctx || !row_ptr || (nnz && (!col_idx || !coeff)) || (k && !out))
        return ctx ? set_err(ctx, CZK_ERR_ARG, "null marlin_arithmetize argument") : CZK_ERR_ARG;
    if (!valid_mem(mem)) return set_err(ctx, CZK_ERR_ARG, "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE");
    if (log_h > 31) return set_err(ctx, CZK_ERR_SIZE, "marlin_arithmetize: H above 2^31 exceeds the 32-bit variable indices");
    if (log_x > log_h) return set_err(ctx, CZK_ERR_SIZE, "marlin_arithmetize: the input domain is larger than H");
    const size_t H = (size_t)1 << log_h, X = (size_t)1 << log_x;
    if (n_instance > X) return set_err(ctx, CZK_ERR_SIZE, "marlin_arithmetize: more formatted inputs than the input domain holds");
    if (m > H) return set_err(ctx, CZK_ERR_SIZE, "marlin_arithmetize: more constraints than H holds");
    if (k < nnz) return set_err(ctx, CZK_ERR_SIZE, "marlin_arithmetize: more entries than K holds");
    if (k >= ((size_t)1 << 32)) return set_err(ctx, CZK_ERR_SIZE, "marlin_arithmetize: K too large for 32-bit indices");
    if (mem == CZK_MEM_HOST) {
        // as czk_r1cs_matrix_register: a CSR offset array, and every variable has a position on H
        const size_t n_vars = H - X + n_instance;
        bool ok = row_ptr[0] == 0 && row_ptr[m] == nnz;
        for (size_t r = 0; ok && r < m; r++) ok = row_ptr[r] <= row_ptr[r + 1];
        if (!ok) return set_err(ctx, CZK_ERR_ARG, "marlin_arithmetize: row_ptr is not a monotone CSR offset array ending at nnz");
        for (size_t t = 0; t < nnz; t++)
            if (col_idx[t] >= n_vars) return set_err(ctx, CZK_ERR_ARG, "marlin_arithmetize: variable index beyond the variables H holds");
    }
    if (!k) return CZK_OK;
    CZK_HIP(ctx, hipSetDevice(ctx->device));
    DomainTables* d = nullptr;
    CZK_TRY(get_domain(ctx, log_h, &d));
    const MarlinRoots roots = pow_table_roots(d->group_gen);
    Staged sr{ctx}, sc{ctx}, sv{ctx}, so{ctx}, tab{ctx};
    CZK_TRY(sr.to_device(row_ptr, (m + 1) * 8, mem));
    if (nnz) {
        CZK_TRY(sc.to_device(col_idx, nnz * 4, mem));
        CZK_TRY(sv.to_device(coeff, nnz * 32, mem));
    }
    CZK_TRY(so.to_device(mem == CZK_MEM_HOST ? nullptr : out, 4 * k * 32, mem));
    CZK_TRY(tab.to_device(nullptr, 4 * 256 * 32, CZK_MEM_HOST));   // workspace from the staging pool: given back once the kernels are enqueued
    {
        ProfScope ps(ctx, "marlin_arithmetize");
        hipLaunchKernelGGL(k_marlin_pow_tables, dim3(4), dim3(256), 0, ctx->stream, (u64*)tab.dev, roots);
        hipLaunchKernelGGL(k_marlin_arithmetize, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, ctx->stream, (const u64*)sr.dev, (const u32*)sc.dev,
                           (const u64*)sv.dev, m, nnz, log_h, log_x, (u32)n_instance, d->size_inv, (const u64*)tab.dev, k, (u64*)so.dev);
    }
    CZK_HIP(ctx, hipGetLastError());
    return so.to_host(out, 4 * k * 32);
}
