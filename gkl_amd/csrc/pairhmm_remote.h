// Wire protocol between a client context (pairhmm_remote.cpp, inside the product libraries) and the PairHMM server
// (pairhmm_server.cpp, gkl_amd/lib/gklhip_server), and the client's interface to pairhmm_api.hip.  Plain C++: no HIP.
//
// A connection is a Unix-domain stream socket.  Every request is one fixed-size Request; every reply is a ReplyHead,
// then `text_len` bytes of error text, then `payload_len` bytes of payload.  The first request of a connection is a
// Hello: a compute connection (control == 0) gets a context of its own on the server, a control connection
// (control == 1) may only ask for Stats.  Batches travel through a shared-memory arena the client creates with
// memfd_create, seals against shrinking and passes once with SCM_RIGHTS (Arena; again whenever it grows); a Compute
// request holds byte offsets into it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/gkl_hip_pairhmm.h"

namespace gklhip_wire {

constexpr uint32_t kMagic = 0x534c4b47u;   // "GKLS"
// 5-7: the PDHMM side (pdhmm_remote.cpp).  A connection is of one kind, fixed by its first message: a PairHMM
// connection (kHello) refuses kPdCompute, a PDHMM connection (kPdHello) refuses kCompute; kArena and kPdStats work on both.
enum MsgType : uint32_t { kHello = 1, kArena = 2, kCompute = 3, kStats = 4, kPdHello = 5, kPdCompute = 6, kPdStats = 7 };

struct Hello {
  int32_t abi_version;   // GKLHIP_ABI_VERSION of the client
  int32_t protocol;      // GKLHIP_SERVER_PROTOCOL of the client
  int32_t control;       // 0 = compute connection, 1 = control connection (Stats only)
  int32_t reserved;
  gklhip_config cfg;
};
struct Arena {
  uint64_t bytes;        // size of the memfd that comes with this message
};
struct Compute {
  int32_t n_reads, n_haps;
  // byte offsets into the arena: the two int64 offset arrays, the six byte arrays, the n_reads * n_haps output doubles
  uint64_t read_off, hap_off, read_bases, read_quals, ins_gop, del_gop, gcp, hap_bases, out;
};
struct PdHello {
  int32_t abi_version;   // GKLHIP_ABI_VERSION of the client
  int32_t protocol;      // GKLHIP_SERVER_PROTOCOL of the client
  int32_t device;        // -1 = the server's choice
  int32_t reserved;
};
struct PdCompute {
  int32_t layout;        // 0 = paired (gklhip_pdhmm_compute), 1 = cross (gklhip_pdhmm_compute_cross_batched)
  int32_t n_read_items, n_hap_items;   // paired: both = batch
  int32_t max_hap_len, max_read_len;   // row strides of the haplotype and the read arrays
  int32_t flags;         // bit 0 fma_mode, bit 1 tail_mode: per call (both can change on a context)
  int64_t ref_batch_pairs;
  // byte offsets into the arena: the seven byte arrays [items][stride], the two int64 length arrays, the output doubles
  uint64_t hap_bases, hap_pdbases, read_bases, read_qual, read_ins_qual, read_del_qual, gcp, hap_lengths, read_lengths, out;
};
static_assert(sizeof(PdHello) == 16 && sizeof(PdCompute) == 112, "wire format");
struct PdComputeReply {  // from the server's context after the call
  float kernel_ms;
  int32_t routing[3];
};
static_assert(sizeof(PdComputeReply) == 16, "wire format");
struct Request {
  uint32_t magic;
  uint32_t type;
  union {
    Hello hello;
    Arena arena;
    Compute compute;
    PdHello pd_hello;
    PdCompute pd_compute;
    uint8_t raw[112];
  } u;
};
static_assert(sizeof(Request) == 120, "wire format");

struct ReplyHead {
  int32_t status;        // gklhip_status
  uint32_t text_len;     // error text (status != GKLHIP_OK)
  uint32_t payload_len;  // Hello: HelloReply; Compute: gklhip_stats of the call; Stats: gklhip_server_info;
                         // PdHello: int32 device; PdCompute: PdComputeReply; PdStats: gklhip_pdhmm_server_info
  uint32_t reserved;
};
struct HelloReply {
  int32_t device;        // the device ordinal the server gave this connection
  int32_t n_devices;     // gklhip_num_devices of the server's context
};

}  // namespace gklhip_wire

// The client side, used by pairhmm_api.hip (which owns error reporting: every function leaves its message in *err).
namespace gklhip_remote {

struct Client;
int connect(const char* socket_path, const gklhip_config* cfg, Client** out, std::string* err);
// One call: copies the batch into the arena (growing it), sends the request, waits for the reply, copies the results
// out.  `st` receives the server context's gklhip_stats of the call.  Not thread-safe per client (the caller locks).
int compute(Client* c, const gklhip_batch* b, double* out, gklhip_stats* st, std::string* err);
int num_devices(const Client* c);
void close(Client* c);
int server_stats(const char* socket_path, gklhip_server_info* out, std::string* err);

}  // namespace gklhip_remote
