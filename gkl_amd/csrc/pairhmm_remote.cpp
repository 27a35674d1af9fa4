// PairHMM client of the server (pairhmm_remote.h): the hello, the batch laid out in the arena, the stats; the socket,
// the arena and the framing are remote_transport.cpp's, shared with the PDHMM client.
// Deliberately HIP-free: a client process (a GATK JVM under GKL_HIP_SERVER) never opens the GPU.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "pairhmm_remote.h"

#include <unistd.h>

#include <cstring>

#include "remote_transport.h"

#define HIDDEN __attribute__((visibility("hidden")))

namespace gklhip_remote {
namespace {

using namespace gklhip_wire;
using namespace gklhip_transport;

int hello(int fd, const gklhip_config* cfg, int control, HelloReply* hr, std::string* err, const char* path) {
  Request r;
  memset(&r, 0, sizeof r);
  r.magic = kMagic; r.type = kHello;
  r.u.hello.abi_version = GKLHIP_ABI_VERSION;
  r.u.hello.protocol = GKLHIP_SERVER_PROTOCOL;
  r.u.hello.control = control;
  if (cfg) r.u.hello.cfg = *cfg;
  return first_message(fd, r, hr, sizeof *hr, err, path);
}

}  // namespace

struct Client {
  Channel ch;
  HelloReply hr{0, 1};
};

HIDDEN int connect(const char* socket_path, const gklhip_config* cfg, Client** out, std::string* err) {
  *out = nullptr;
  const int fd = open_socket(socket_path, err);
  if (fd < 0) return GKLHIP_ERR_HIP;
  Client* c = new Client();
  c->ch.path = socket_path;
  c->ch.fd = fd;
  const int st = hello(fd, cfg, 0, &c->hr, err, socket_path);
  if (st != GKLHIP_OK) { close(c); return st; }
  *out = c;
  return GKLHIP_OK;
}

HIDDEN int num_devices(const Client* c) { return c ? c->hr.n_devices : 0; }

HIDDEN void close(Client* c) {
  if (!c) return;
  gklhip_transport::close(&c->ch);
  delete c;
}

HIDDEN int compute(Client* cl, const gklhip_batch* b, double* out, gklhip_stats* st, std::string* err) {
  Channel* c = &cl->ch;
  if (c->broken) return gone(c, err, "an earlier call lost the connection");
  const int64_t n_pairs = (int64_t)b->n_reads * b->n_haps;
  const size_t rl = (size_t)b->read_off[b->n_reads], hl = (size_t)b->hap_off[b->n_haps];
  auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
  Compute q{};
  q.n_reads = b->n_reads; q.n_haps = b->n_haps;
  size_t at = 0;
  q.read_off = at;   at += up(((size_t)b->n_reads + 1) * 8);
  q.hap_off = at;    at += up(((size_t)b->n_haps + 1) * 8);
  q.read_bases = at; at += up(rl);
  q.read_quals = at; at += up(rl);
  q.ins_gop = at;    at += up(rl);
  q.del_gop = at;    at += up(rl);
  q.gcp = at;        at += up(rl);
  q.hap_bases = at;  at += up(hl);
  q.out = at;        at += (size_t)n_pairs * 8;
  int rc;
  if (at > c->cap && (rc = grow(c, at, err))) return rc;
  uint8_t* a = c->arena;
  memcpy(a + q.read_off, b->read_off, ((size_t)b->n_reads + 1) * 8);
  memcpy(a + q.hap_off, b->hap_off, ((size_t)b->n_haps + 1) * 8);
  memcpy(a + q.read_bases, b->read_bases, rl);
  memcpy(a + q.read_quals, b->read_quals, rl);
  memcpy(a + q.ins_gop, b->ins_gop, rl);
  memcpy(a + q.del_gop, b->del_gop, rl);
  memcpy(a + q.gcp, b->gcp, rl);
  memcpy(a + q.hap_bases, b->hap_bases, hl);
  Request r;
  memset(&r, 0, sizeof r);
  r.magic = kMagic; r.type = kCompute;
  r.u.compute = q;
  const int status = call(c, r, st, sizeof *st, err);
  if (status != GKLHIP_OK) {
    if (!c->broken) *err = "PairHMM server at " + c->path + ": " + *err;
    return status;
  }
  memcpy(out, a + q.out, (size_t)n_pairs * 8);
  return GKLHIP_OK;
}

HIDDEN int server_stats(const char* socket_path, gklhip_server_info* out, std::string* err) {
  const int fd = open_socket(socket_path, err);
  if (fd < 0) return GKLHIP_ERR_HIP;
  HelloReply hr{};
  int st = hello(fd, nullptr, 1, &hr, err, socket_path);
  if (st == GKLHIP_OK) {
    Request r;
    memset(&r, 0, sizeof r);
    r.magic = kMagic; r.type = kStats;
    std::string text;
    memset(out, 0, sizeof *out);
    st = send_all(fd, &r, sizeof r) ? read_reply(fd, &text, out, sizeof *out) : -1;
    if (st < 0) { *err = std::string("the PairHMM server at ") + socket_path + " closed the connection"; st = GKLHIP_ERR_HIP; }
    else if (st != GKLHIP_OK) *err = std::string("PairHMM server at ") + socket_path + ": " + text;
  }
  ::close(fd);
  return st;
}

}  // namespace gklhip_remote
