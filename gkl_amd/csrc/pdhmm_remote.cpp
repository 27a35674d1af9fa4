// PDHMM client of the server (pdhmm_remote.h).  Deliberately HIP-free: a client process (a GATK JVM under
// GKL_HIP_SERVER) never opens the GPU.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "pdhmm_remote.h"

#include <unistd.h>

#include <cstring>

#include "remote_transport.h"

#define HIDDEN __attribute__((visibility("hidden")))

namespace gklhip_pd_remote {

using namespace gklhip_wire;
using namespace gklhip_transport;

struct Client {
  Channel ch;
  int32_t device = -1;
};

HIDDEN int connect(const char* socket_path, int device, Client** out, std::string* err) {
  *out = nullptr;
  const int fd = open_socket(socket_path, err);
  if (fd < 0) return GKLHIP_ERR_HIP;
  Client* c = new Client();
  c->ch.path = socket_path;
  c->ch.fd = fd;
  Request r;
  memset(&r, 0, sizeof r);
  r.magic = kMagic; r.type = kPdHello;
  r.u.pd_hello.abi_version = GKLHIP_ABI_VERSION;
  r.u.pd_hello.protocol = GKLHIP_SERVER_PROTOCOL;
  r.u.pd_hello.device = device < 0 ? -1 : device;
  const int st = first_message(fd, r, &c->device, sizeof c->device, err, socket_path);
  if (st != GKLHIP_OK) { close(c); return st; }
  *out = c;
  return GKLHIP_OK;
}

HIDDEN size_t arena_bytes(const Client* c) { return c ? c->ch.cap : 0; }

HIDDEN void close(Client* c) {
  if (!c) return;
  gklhip_transport::close(&c->ch);
  delete c;
}

HIDDEN int compute(Client* cl, const Call& p, double* out, PdComputeReply* rep, std::string* err) {
  Channel* c = &cl->ch;
  if (c->broken) return gone(c, err, "an earlier call lost the connection");
  const size_t hb = (size_t)p.n_hap_items * (size_t)p.max_hap_len, rb = (size_t)p.n_read_items * (size_t)p.max_read_len;
  auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
  PdCompute q{};
  q.layout = p.layout; q.n_read_items = p.n_read_items; q.n_hap_items = p.n_hap_items;
  q.max_hap_len = p.max_hap_len; q.max_read_len = p.max_read_len; q.flags = p.flags;
  q.ref_batch_pairs = p.ref_batch_pairs;
  size_t at = 0;
  q.hap_lengths = at;   at += up((size_t)p.n_hap_items * 8);
  q.read_lengths = at;  at += up((size_t)p.n_read_items * 8);
  q.hap_bases = at;     at += up(hb);
  q.hap_pdbases = at;   at += up(hb);
  q.read_bases = at;    at += up(rb);
  q.read_qual = at;     at += up(rb);
  q.read_ins_qual = at; at += up(rb);
  q.read_del_qual = at; at += up(rb);
  q.gcp = at;           at += up(rb);
  q.out = at;           at += (size_t)p.n_pairs * 8;
  int rc;
  if (at > c->cap && (rc = grow(c, at, err))) return rc;
  uint8_t* a = c->arena;
  memcpy(a + q.hap_lengths, p.hap_lengths, (size_t)p.n_hap_items * 8);
  memcpy(a + q.read_lengths, p.read_lengths, (size_t)p.n_read_items * 8);
  memcpy(a + q.hap_bases, p.hap_bases, hb);
  memcpy(a + q.hap_pdbases, p.hap_pdbases, hb);
  memcpy(a + q.read_bases, p.read_bases, rb);
  memcpy(a + q.read_qual, p.read_qual, rb);
  memcpy(a + q.read_ins_qual, p.read_ins_qual, rb);
  memcpy(a + q.read_del_qual, p.read_del_qual, rb);
  memcpy(a + q.gcp, p.gcp, rb);
  Request r;
  memset(&r, 0, sizeof r);
  r.magic = kMagic; r.type = kPdCompute;
  r.u.pd_compute = q;
  memset(rep, 0, sizeof *rep);
  const int status = call(c, r, rep, sizeof *rep, err);   // (an error of the server's library: its status, its text)
  if (status != GKLHIP_OK) return status;
  memcpy(out, a + q.out, (size_t)p.n_pairs * 8);
  return GKLHIP_OK;
}

// (a control connection of the PairHMM kind: it holds no context on the server and counts as no connection)
HIDDEN int server_stats(const char* socket_path, gklhip_pdhmm_server_info* out, std::string* err) {
  const int fd = open_socket(socket_path, err);
  if (fd < 0) return GKLHIP_ERR_HIP;
  Request r;
  memset(&r, 0, sizeof r);
  r.magic = kMagic; r.type = kHello;
  r.u.hello.abi_version = GKLHIP_ABI_VERSION;
  r.u.hello.protocol = GKLHIP_SERVER_PROTOCOL;
  r.u.hello.control = 1;
  HelloReply hr{};
  int st = first_message(fd, r, &hr, sizeof hr, err, socket_path);
  if (st == GKLHIP_OK) {
    memset(&r, 0, sizeof r);
    r.magic = kMagic; r.type = kPdStats;
    std::string text;
    memset(out, 0, sizeof *out);
    st = send_all(fd, &r, sizeof r) ? read_reply(fd, &text, out, sizeof *out) : -1;
    if (st < 0) { *err = std::string("the PairHMM server at ") + socket_path + " closed the connection (it does not serve PDHMM)"; st = GKLHIP_ERR_HIP; }
    else if (st != GKLHIP_OK) *err = std::string("PairHMM server at ") + socket_path + ": " + text;
  }
  ::close(fd);
  return st;
}

}  // namespace gklhip_pd_remote
