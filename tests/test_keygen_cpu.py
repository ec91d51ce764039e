"""CPU-only checks of the key generator's host side: the CSR transposition helper against a dense transpose, and the null-context behaviour
of the fixed-base / Lagrange entry points."""
import ctypes as C

import numpy as np


def _dense(ptr, idx, val, m, n):
    """dense m x n matrix of Python integers (limb 0 of each coefficient is enough: the test's coefficients are small); duplicates add up"""
    d = [[0] * n for _ in range(m)]
    for i in range(m):
        for t in range(int(ptr[i]), int(ptr[i + 1])):
            d[i][int(idx[t])] += int(val[t][0])
    return d


def test_csr_transpose_matches_the_dense_transpose():
    from czk_amd.keygen import csr_transpose
    rng = np.random.default_rng(7)
    cases = []
    for m, n in ((1, 1), (5, 7), (16, 3), (40, 33)):
        rows = []
        for i in range(m):
            k = 0 if i % 4 == 1 else int(rng.integers(1, 5))          # empty rows
            cols = [int(c) for c in rng.integers(0, n - 1 if n > 1 else 1, k)]   # the last column stays empty (n > 1)
            if i % 5 == 2 and cols:
                cols.append(cols[0])                                   # a duplicate column index within a row
            rows.append(cols)
        cases.append((m, n, rows))
    cases.append((3, 4, [[], [], []]))                                 # no entries at all
    for m, n, rows in cases:
        ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        idx = np.array([c for r in rows for c in r], dtype=np.uint32)
        val = np.zeros((idx.size, 4), dtype=np.uint64)
        val[:, 0] = rng.integers(1, 1 << 20, idx.size)
        val[:, 1:] = rng.integers(0, 1 << 62, (idx.size, 3))           # the other limbs travel with their entry
        t_ptr, t_idx, t_val = csr_transpose(ptr, idx, val, n)
        assert t_ptr.shape == (n + 1,) and t_ptr[0] == 0 and t_ptr[-1] == idx.size and t_idx.dtype == np.uint32 and t_val.shape == val.shape
        d, dt = _dense(ptr, idx, val, m, n), _dense(t_ptr, t_idx, t_val, n, m)
        assert dt == [[d[i][j] for i in range(m)] for j in range(n)]
        assert sorted(map(tuple, t_val.tolist())) == sorted(map(tuple, val.tolist()))
        for j in range(n):                                             # row indices ascend within a transposed row
            seg = t_idx[int(t_ptr[j]):int(t_ptr[j + 1])]
            assert np.all(seg[1:] >= seg[:-1])
        if n > 1:
            assert t_ptr[n] == t_ptr[n - 1]                            # the empty column is an empty row
    # transposing twice restores the matrix
    m, n, rows = cases[3]
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    idx = np.array([c for r in rows for c in r], dtype=np.uint32)
    val = np.zeros((idx.size, 4), dtype=np.uint64)
    val[:, 0] = np.arange(1, idx.size + 1)
    back = csr_transpose(*csr_transpose(ptr, idx, val, n), m)
    assert _dense(back[0], back[1], back[2], m, n) == _dense(ptr, idx, val, m, n)


def test_csr_transpose_rejects_malformed_input():
    import pytest
    from czk_amd.keygen import csr_transpose
    one = np.ones((2, 4), dtype=np.uint64)
    with pytest.raises(ValueError):
        csr_transpose([0, 1, 3], [0, 1], one, 2)      # row_ptr[m] != nnz
    with pytest.raises(ValueError):
        csr_transpose([0, 2, 1, 2], [0, 1], one, 2)   # decreasing row_ptr
    with pytest.raises(ValueError):
        csr_transpose([0, 1, 2], [0, 2], one, 2)      # column index outside the matrix


def test_null_context_calls_return_err_arg():
    import czk_amd
    L = czk_amd.lib()
    buf = np.zeros(24, dtype=np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(0)
    assert L.czk_fixed_base_create(None, C.c_int(1), p, C.c_uint(0), C.c_size_t(0), C.byref(h)) == 3 and not h.value
    assert L.czk_fixed_base_msm(None, None, p, C.c_size_t(1), C.c_int(0), p, None, C.c_int(0)) == 3
    assert L.czk_fixed_base_layout(None, None, None, None) == 3
    assert L.czk_fr_lagrange_coefficients(None, C.c_uint(3), p, p, C.c_size_t(8), C.c_int(0)) == 3
    L.czk_fixed_base_release(None)   # a null handle is ignored
