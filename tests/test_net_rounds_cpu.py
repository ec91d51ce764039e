"""The rejections of the protocol rounds (csrc/net_rounds.hip) and of the communicator's exchanges (csrc/net.hip) that need no GPU: what a null
communicator and a communicator created WITHOUT a context get from every entry point -- the code and, for the latter, the exact text of
czk_net_last_error.

Every pointer argument is null and every count is non-zero: the context check comes before the pointer checks in each of these calls, so nothing is
dereferenced, and that order is part of what is pinned here.  The exchanges are the exception: they look at their buffers first ("czk_net: null
buffer" for a non-empty message), so they are called with a message of 0 bytes.  The calls go through ctypes on czk_amd.lib(): the methods of
czk_amd.Net touch their arguments before the library sees them."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ERR_ARG = 3
MEM_DEVICE = 1
N = C.c_size_t(8)
Z = C.c_size_t(0)
U = C.c_uint(1)
I = C.c_int(0)
NEEDS = " needs a communicator created with a context"
OPENS = "batch opens need a communicator created with a context"
DEVICE = "czk_net: device buffers need a communicator created with a context"

# (entry point, its arguments after the communicator, czk_net_last_error on a communicator without a context)
ROUNDS = [
    ("czk_net_atomic_broadcast", (None, N, None, None, C.c_int(MEM_DEVICE)), "czk_net_atomic_broadcast" + NEEDS),
    ("czk_net_atomic_broadcast_tree", (None, N, None, None, C.c_int(MEM_DEVICE)), "czk_net_atomic_broadcast_tree" + NEEDS),
    ("czk_spdz_batch_open", (None, None, None, N, None, I, None), OPENS),
    ("czk_add_batch_open", (None, N, None), OPENS),
    ("czk_gsz_batch_open", (None, N, None, U, None, None), OPENS),
    ("czk_gsz_batch_king_compute", (None, N, None, U, None, None), OPENS),
    ("czk_net_share_batch_mul", (C.c_size_t(2), None, None, None, None, None, None, None, N, I, None, None), "czk_net_share_batch_mul" + NEEDS),
    ("czk_net_share_batch_inv", (C.c_size_t(2), None, None, None, None, None, None, None, None, N, I, None, None), "czk_net_share_batch_inv" + NEEDS),
    ("czk_net_share_partial_products", (C.c_size_t(2), None, None, None, None, None, None, None, None, N, I, None, None),
     "czk_net_share_partial_products" + NEEDS),
    ("czk_net_gsz_share_batch_mul", (U, None, None, None, None, None, N, None, None), "czk_net_gsz_share_batch_mul" + NEEDS),
    ("czk_net_gsz_share_batch_inv", (U, None, None, None, None, None, N, None, None), "czk_net_gsz_share_batch_inv" + NEEDS),
    ("czk_net_gsz_share_partial_products", (U, None, None, None, None, None, N, None, None), "czk_net_gsz_share_partial_products" + NEEDS),
    ("czk_net_gsz_product_check", (U, None, None, None, N, None, None, None, None, None), "czk_net_gsz_product_check" + NEEDS),
    ("czk_net_gsz_dn_generate", (I, U, None, None, N, None, None), "czk_net_gsz_dn_generate" + NEEDS),
    ("czk_net_gsz_dn_check", (I, U, None, None, N, None, None), "czk_net_gsz_dn_check" + NEEDS),
]
# device buffers on a communicator without a context: the four exchanges (an empty message, see above) and the Fr forms of the king's two
DEVICE_BUFFERS = [
    ("czk_net_broadcast", (None, Z, None, C.c_int(MEM_DEVICE)), DEVICE),
    ("czk_net_send_to_king", (None, Z, None, C.c_int(MEM_DEVICE)), DEVICE),
    ("czk_net_recv_from_king", (None, Z, None, C.c_int(MEM_DEVICE)), DEVICE),
    ("czk_net_alltoall", (None, Z, None, C.c_int(MEM_DEVICE)), DEVICE),
    ("czk_fr_send_to_king", (None, Z, None), DEVICE),
    ("czk_fr_recv_from_king", (None, Z, None), DEVICE),
]
CALLS = ROUNDS + DEVICE_BUFFERS


@pytest.fixture(scope="module")
def bare():
    sys.path.insert(0, ROOT)
    import czk_amd
    net = czk_amd.Net(None, czk_amd.CZK_NET_SHM, 0, 1, os.urandom(16))      # a world of one, host memory only
    yield czk_amd.lib(), net
    net.close()


@pytest.mark.parametrize("name,args,message", CALLS, ids=[c[0] for c in CALLS])
def test_without_a_context(bare, name, args, message):
    L, net = bare
    assert L.czk_net_set_option(net._h, b"exchange", C.c_long(7)) == ERR_ARG     # another call's text in czk_net_last_error: the one below must replace it
    assert L.czk_net_last_error(net._h).decode().startswith("czk_net_set_option:")
    assert getattr(L, name)(net._h, *args) == ERR_ARG
    assert L.czk_net_last_error(net._h).decode() == message


@pytest.mark.parametrize("name,args", [c[:2] for c in CALLS], ids=[c[0] for c in CALLS])
def test_null_communicator(bare, name, args):
    L, _ = bare
    assert getattr(L, name)(None, *args) == ERR_ARG
