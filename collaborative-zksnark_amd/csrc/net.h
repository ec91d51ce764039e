// net.h -- what the protocol rounds (net_rounds.hip) see of the communicator (net.hip): the handle, its error macros, the exchanges and their counting rule.
// The rounds read n->ctx, n->rank and n->world, grow n->gather and n->dx with net_buf, and move every byte through exchange(); the slots, the
// mailboxes, the barrier and the RCCL table are net.hip's alone.
#pragma once
#include <rccl/rccl.h>   // for ncclComm_t in czk_net only: the rounds never call RCCL, and net.hip resolves it with dlopen

#include "czk_internal.h"

namespace czk {
struct ShmHeader;   // the SHM control block (net.hip)
}

struct czk_net {
    czk_ctx* ctx = nullptr;
    int transport = 0, rank = 0, world = 1;
    std::string err;
    long exchange = 0;            // 0 ring, 1 p2p
    long timeout_ms = 120000;
    uint64_t stats[5] = {0, 0, 0, 0, 0};
    // RCCL
    ncclComm_t comm = nullptr;
    // SHM
    std::string shm_name;
    czk::ShmHeader* hdr = nullptr;
    char* slots = nullptr;        // world x 2 x slot_bytes
    size_t slot_bytes = (size_t)16 << 20, data_bytes = 0;
    bool data_pinned = false;
    // IPC (the SHM control block + one device mailbox per rank, mapped into every peer with hipIpc: staging never leaves device memory)
    char* mailbox = nullptr;                 // this rank's 2 x slot_bytes, device memory
    std::vector<char*> peer_mail;            // every rank's mailbox as this process sees it (own entry = mailbox)
    // lab build, IPC transport created WITHOUT a context: a dry run of the mailbox hand-over on a box without GPUs (tests/test_net.py) -- every rank's "device
    // mailbox" is a POSIX segment of its own, its 64-byte handle names the owner's rank and device (= rank: every peer is on another device), and the order
    // allocate -> publish handle -> barrier -> open every peer's handle -> barrier -> exchanges by slot parity is the code the hipIpc path runs
    bool ipc_dry = false;
    size_t dry_mail_bytes = 0;
    bool shm_like() const { return transport == CZK_NET_SHM || transport == CZK_NET_IPC; }
    uint64_t seq = 0;             // chunk steps so far: parity of the slot in use
    bool reads_in_flight = false;
    // scratch on the context's GPU
    czk::DeviceBuf gather, dx, small;
};

namespace czk {
inline int net_err(czk_net* n, int code, const std::string& msg) {
    if (n) n->err = msg;
    return code;
}
#define NET_HIP(n, call)                                                                                  \
    do {                                                                                                  \
        hipError_t e__ = (call);                                                                          \
        if (e__ != hipSuccess) return czk::net_err((n), CZK_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)
// an error of a czk_* call on the communicator's context becomes the communicator's error too
#define NET_CTX(n, expr)                                                      \
    do {                                                                      \
        int rc__ = (expr);                                                    \
        if (rc__ != CZK_OK) return czk::net_err((n), rc__, czk_last_error((n)->ctx)); \
    } while (0)

enum class Op { Broadcast, ToKing, FromKing, AllToAll };

int net_buf(czk_net* n, DeviceBuf& b, size_t bytes);                                          // grows a scratch buffer of the communicator (n->ctx's GPU)
int exchange(czk_net* n, Op op, const void* send, size_t bytes, void* recv, int mem);       // one exchange on either transport; counts nothing
void count_stats(czk_net* n, Op op, size_t m);                                               // mpc-net's counting rules for an exchange of m bytes
}  // namespace czk
