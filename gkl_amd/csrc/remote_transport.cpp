// Transport of the server's clients (remote_transport.h).  Deliberately HIP-free: a client process (a GATK JVM under
// GKL_HIP_SERVER) never opens the GPU.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "remote_transport.h"

#include <errno.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#define HIDDEN __attribute__((visibility("hidden")))

namespace gklhip_transport {
namespace {

using namespace gklhip_wire;

bool recv_all(int fd, void* p, size_t n) {
  char* d = static_cast<char*>(p);
  while (n) {
    const ssize_t k = ::recv(fd, d, n, 0);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return false;
    d += k; n -= (size_t)k;
  }
  return true;
}
bool send_with_fd(int fd, const Request& r, int pass_fd) {
  iovec iov{const_cast<Request*>(&r), sizeof r};
  alignas(cmsghdr) char ctl[CMSG_SPACE(sizeof(int))];
  memset(ctl, 0, sizeof ctl);
  msghdr m{};
  m.msg_iov = &iov; m.msg_iovlen = 1;
  m.msg_control = ctl; m.msg_controllen = sizeof ctl;
  cmsghdr* c = CMSG_FIRSTHDR(&m);
  c->cmsg_level = SOL_SOCKET; c->cmsg_type = SCM_RIGHTS; c->cmsg_len = CMSG_LEN(sizeof(int));
  memcpy(CMSG_DATA(c), &pass_fd, sizeof(int));
  ssize_t k;
  do k = ::sendmsg(fd, &m, MSG_NOSIGNAL); while (k < 0 && errno == EINTR);
  if (k <= 0) return false;
  return (size_t)k == sizeof r || send_all(fd, reinterpret_cast<const char*>(&r) + k, sizeof r - (size_t)k);
}

}  // namespace

HIDDEN bool send_all(int fd, const void* p, size_t n) {
  const char* s = static_cast<const char*>(p);
  while (n) {
    const ssize_t k = ::send(fd, s, n, MSG_NOSIGNAL);   // (a server that went away must not SIGPIPE the JVM)
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return false;
    s += k; n -= (size_t)k;
  }
  return true;
}

HIDDEN int read_reply(int fd, std::string* text, void* payload, size_t cap) {
  ReplyHead h;
  if (!recv_all(fd, &h, sizeof h) || h.text_len > (1u << 16) || h.payload_len > (1u << 20)) return -1;
  std::vector<char> buf(std::max<size_t>(h.text_len, h.payload_len) + 1);
  if (h.text_len && !recv_all(fd, buf.data(), h.text_len)) return -1;
  text->assign(buf.data(), h.text_len);
  if (h.payload_len) {
    if (!recv_all(fd, buf.data(), h.payload_len)) return -1;
    if (payload) memcpy(payload, buf.data(), std::min<size_t>(cap, h.payload_len));
  }
  return h.status;
}

HIDDEN int open_socket(const char* path, std::string* err) {
  sockaddr_un a{};
  a.sun_family = AF_UNIX;
  if (!path || !*path || strlen(path) >= sizeof a.sun_path) {
    *err = std::string("PairHMM server socket path is empty or too long: ") + (path ? path : "(null)");
    return -1;
  }
  memcpy(a.sun_path, path, strlen(path) + 1);
  const int fd = ::socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
  if (fd < 0) { *err = std::string("socket(): ") + strerror(errno); return -1; }
  int rc;
  do rc = ::connect(fd, reinterpret_cast<sockaddr*>(&a), sizeof a); while (rc < 0 && errno == EINTR);
  if (rc < 0) {
    *err = std::string("cannot reach the PairHMM server at ") + path + ": " + strerror(errno);
    ::close(fd);
    return -1;
  }
  return fd;
}

HIDDEN int first_message(int fd, const Request& r, void* reply, size_t reply_cap, std::string* err, const char* path) {
  std::string text;
  const int st = send_all(fd, &r, sizeof r) ? read_reply(fd, &text, reply, reply_cap) : -1;
  if (st < 0) { *err = std::string("the PairHMM server at ") + path + " closed the connection during the hello"; return GKLHIP_ERR_HIP; }
  if (st != GKLHIP_OK) *err = std::string("PairHMM server at ") + path + ": " + text;
  return st;
}

HIDDEN int gone(Channel* c, std::string* err, const char* what) {
  c->broken = true;
  *err = "the PairHMM server at " + c->path + " went away (" + what + ")";
  return GKLHIP_ERR_HIP;
}

// (sealed: the memfd can neither shrink nor grow under the server's mapping)
HIDDEN int grow(Channel* c, size_t need, std::string* err) {
  const size_t page = 1 << 16;
  const size_t bytes = (std::max(need, std::max(c->cap * 2, (size_t)1 << 20)) + page - 1) / page * page;
  const int mfd = memfd_create("gklhip-arena", MFD_CLOEXEC | MFD_ALLOW_SEALING);
  if (mfd < 0) { *err = std::string("memfd_create: ") + strerror(errno); return GKLHIP_ERR_OOM; }
  void* p = MAP_FAILED;
  if (ftruncate(mfd, (off_t)bytes) == 0 && fcntl(mfd, F_ADD_SEALS, F_SEAL_SHRINK | F_SEAL_GROW | F_SEAL_SEAL) == 0)
    p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, mfd, 0);
  if (p == MAP_FAILED) {
    *err = std::string("arena of ") + std::to_string(bytes) + " bytes: " + strerror(errno);
    ::close(mfd);
    return GKLHIP_ERR_OOM;
  }
  Request r;
  memset(&r, 0, sizeof r);
  r.magic = kMagic; r.type = kArena;
  r.u.arena.bytes = bytes;
  const bool sent = send_with_fd(c->fd, r, mfd);
  ::close(mfd);   // (the mapping keeps the memory; the server holds its own descriptor)
  std::string text;
  const int st = sent ? read_reply(c->fd, &text, nullptr, 0) : -1;
  if (st < 0) { munmap(p, bytes); return gone(c, err, "passing the arena"); }
  if (st != GKLHIP_OK) { munmap(p, bytes); *err = "PairHMM server at " + c->path + ": " + text; return st; }
  if (c->arena) munmap(c->arena, c->cap);
  c->arena = static_cast<uint8_t*>(p);
  c->cap = bytes;
  return GKLHIP_OK;
}

HIDDEN int call(Channel* c, const Request& r, void* payload, size_t cap, std::string* err) {
  if (!send_all(c->fd, &r, sizeof r)) return gone(c, err, "sending a call");
  std::string text;
  const int status = read_reply(c->fd, &text, payload, cap);
  if (status < 0) return gone(c, err, "connection closed during a call");
  if (status != GKLHIP_OK) *err = text;
  return status;
}

HIDDEN void close(Channel* c) {
  if (c->fd >= 0) ::close(c->fd);
  if (c->arena) munmap(c->arena, c->cap);
  c->fd = -1; c->arena = nullptr; c->cap = 0;
}

}  // namespace gklhip_transport
