// Transport shared by the two clients of the server (pairhmm_remote.cpp, pdhmm_remote.cpp): the Unix-domain socket, the
// request / reply framing of pairhmm_remote.h, the sealed memfd arena and the error texts.  Plain C++: no HIP.  Every
// symbol is hidden: each product library carries its own copy.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "pairhmm_remote.h"

namespace gklhip_transport {

// One connection and its arena.  Not thread-safe (the owning context locks per call).
struct Channel {
  std::string path;
  int fd = -1;
  uint8_t* arena = nullptr;
  size_t cap = 0;
  bool broken = false;
};

bool send_all(int fd, const void* p, size_t n);
// Reads one reply; its payload goes to `payload` (at most `cap` bytes kept).  -1: the connection is gone.
int read_reply(int fd, std::string* text, void* payload, size_t cap);
// A connected socket, or -1 with *err set.
int open_socket(const char* path, std::string* err);
// Sends the first message of a connection and reads its reply (payload to `reply`); the server's refusal text, or that
// the connection closed, goes to *err.
int first_message(int fd, const gklhip_wire::Request& r, void* reply, size_t reply_cap, std::string* err, const char* path);
// Marks the channel broken: every later call fails at once.  Returns GKLHIP_ERR_HIP.
int gone(Channel* c, std::string* err, const char* what);
// A new, bigger arena of at least `need` bytes: a sealed memfd passed to the server, which maps it.
int grow(Channel* c, size_t need, std::string* err);
// One request on an open channel, reply payload to `payload`.  A status other than GKLHIP_OK leaves the server's text,
// as it came, in *err.
int call(Channel* c, const gklhip_wire::Request& r, void* payload, size_t cap, std::string* err);
void close(Channel* c);   // (socket and mapping; the Channel itself belongs to the caller)

}  // namespace gklhip_transport
