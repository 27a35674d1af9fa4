// The PDHMM client of the server (wire format: pairhmm_remote.h, transport: remote_transport.h), used by pdhmm_api.hip,
// which owns argument checking and error reporting: every function here leaves its message in *err.  Plain C++: no HIP.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/gkl_hip_pdhmm.h"
#include "pairhmm_remote.h"

namespace gklhip_pd_remote {

struct Client;
// One call, already checked (pd_validate / pd_cross_problem / pd_paired_problem of pdhmm_api.hip; sent by its pd_run_remote).  Paired layout: n_read_items == n_hap_items == the batch.
struct Call {
  int32_t layout, n_read_items, n_hap_items, max_hap_len, max_read_len, flags;
  int64_t ref_batch_pairs, n_pairs;
  const int8_t *hap_bases, *hap_pdbases, *read_bases, *read_qual, *read_ins_qual, *read_del_qual, *gcp;
  const int64_t *hap_lengths, *read_lengths;
};

int connect(const char* socket_path, int device, Client** out, std::string* err);
// Copies the arrays into the arena (growing it), sends the request, waits for the reply, copies the results out.  A
// library error on the server comes back with its status and its exact text.  Not thread-safe per client.
int compute(Client* c, const Call& q, double* out, gklhip_wire::PdComputeReply* rep, std::string* err);
size_t arena_bytes(const Client* c);
void close(Client* c);
int server_stats(const char* socket_path, gklhip_pdhmm_server_info* out, std::string* err);

}  // namespace gklhip_pd_remote
