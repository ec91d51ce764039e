"""What a null context gets from the pointwise Fr calls (csrc/fr_vec.hip), the radix-2 transforms (csrc/ntt.hip) and the Groth16 witness map
(csrc/witness_map.hip): CZK_ERR_ARG from each, with no GPU in the machine.

Every pointer argument is null and every count is non-zero: the context check comes first in each of these calls, so nothing is dereferenced and
no device is selected, and that order is part of what is pinned here.  (Their other rejections need a context: tests/test_call_contract.py.)"""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ERR_ARG = 3
N = C.c_size_t(8)
U = C.c_uint(3)
I = C.c_int(0)

# (entry point, its arguments after the context)
CALLS = [
    ("czk_fr_vec_op", (I, None, None, None, N, I)),
    ("czk_fr_vec_scale", (None, None, None, N, I)),
    ("czk_fr_beaver_combine", (None, None, None, None, None, I, None, N, I)),
    ("czk_fr_spdz_open", (None, C.c_size_t(2), N, None, None)),
    ("czk_fr_into_repr", (None, None, N, I)),
    ("czk_fr_from_repr", (None, None, N, I)),
    ("czk_spdz_open_combine", (None, None, None, None, None, C.c_size_t(2), C.c_uint64(1), None, None, None, None, None, N)),
    ("czk_ntt_fr", (None, U, C.c_size_t(1), I, N, I)),
    ("czk_ntt_fr_to", (None, N, None, U, C.c_size_t(1), I, N, C.c_int(1))),
    ("czk_domain_constants", (U, None)),
    ("czk_witness_map_pre", (None, N, None, N, U, C.c_size_t(1))),
    ("czk_witness_map_pre_masked", (None, N, None, N, None, None, U, C.c_size_t(1))),
    ("czk_witness_map_post", (None, None, N, U, C.c_size_t(1))),
    ("czk_witness_map_post_h", (None, None, N, U, C.c_size_t(1))),
]


@pytest.fixture(scope="module")
def L():
    sys.path.insert(0, ROOT)
    import czk_amd
    return czk_amd.lib()


@pytest.mark.parametrize("name,args", CALLS, ids=[c[0] for c in CALLS])
def test_null_context(L, name, args):
    assert getattr(L, name)(None, *args) == ERR_ARG
