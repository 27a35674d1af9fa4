// gklhip_server: one process per node owns the GPU and computes the PairHMM calls of every client process
// (wire format: pairhmm_remote.h).
//
//   gklhip_server --socket PATH [--devices 0,1,...]
//
// One thread and one gklhip context per connection, every call through plain gklhip_compute: calls of concurrent
// clients meet in the process's small-call combiner exactly as the calls of threads of one process do.  Prints `ready`
// on stdout once it listens; SIGTERM (or SIGINT) stops accepting, lets the calls in flight finish, removes the socket
// and exits 0.  Plain C++ over the C ABI (tests/test_server_cpu.py links it against a stub of that ABI).
//
// PDHMM: a connection that opens with a PdHello gets a gklhip_pdhmm context of its own; its calls go, one by one, through
// gklhip_pdhmm_compute / _compute_cross_batched of libgklhip_pdhmm.so.  That library is loaded at run time when the
// first such connection arrives (GKL_HIP_PDHMM_LIB, else next to this program): the server links no PDHMM symbol, and
// without the library it serves PairHMM as before.  GKL_HIP_PDHMM_TABLE / GKL_HIP_PDHMM_PIPELINE are read here, by the
// process that computes.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <dlfcn.h>
#include <errno.h>
#include <fcntl.h>
#include <poll.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/un.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gkl_hip_pairhmm.h"
#include "../../include/gkl_hip_pdhmm.h"
#include "pairhmm_remote.h"

using namespace gklhip_wire;

namespace {

std::string g_socket;
std::vector<int32_t> g_devices;          // --devices (empty: each connection's own cfg.device)
bool g_try_register = true;              // GKL_HIP_SERVER_REGISTER=0: always the copy path
std::mutex g_mu;                         // guards g_conn_per_entry, g_used
std::vector<int32_t> g_conn_per_entry;   // live compute connections per --devices entry
std::vector<int32_t> g_used;             // without --devices: device ordinals connections asked for
std::atomic<int64_t> g_calls{0}, g_failed{0}, g_conns_total{0}, g_registered{0}, g_copied{0}, g_refused{0};
std::atomic<int32_t> g_active{0}, g_live{0};
int g_stop_pipe[2] = {-1, -1};

// ---- PDHMM: the library (loaded on the first PdHello) and its counters (gklhip_pdhmm_server_info) ----
struct PdLib {
  decltype(&gklhip_pdhmm_init) init = nullptr;
  decltype(&gklhip_pdhmm_set_fma_mode) set_fma_mode = nullptr;
  decltype(&gklhip_pdhmm_set_tail_mode) set_tail_mode = nullptr;
  decltype(&gklhip_pdhmm_compute) compute = nullptr;
  decltype(&gklhip_pdhmm_compute_cross_batched) compute_cross_batched = nullptr;
  decltype(&gklhip_pdhmm_last_kernel_ms) last_kernel_ms = nullptr;
  decltype(&gklhip_pdhmm_last_routing) last_routing = nullptr;
  decltype(&gklhip_pdhmm_done) done = nullptr;
  decltype(&gklhip_pdhmm_last_error) last_error = nullptr;
  decltype(&gklhip_pdhmm_combine_counts) combine_counts = nullptr;   // (optional: reported when the library has it)
} g_pd;
std::mutex g_pd_mu;                      // guards the load and g_pd_load_err
std::atomic<int32_t> g_pd_state{0};      // 0 not yet asked for, 1 loaded, -1 failed
std::string g_pd_load_err;
std::vector<int32_t> g_pd_conn_per_entry;   // live PDHMM connections per --devices entry (g_mu)
std::atomic<int64_t> g_pd_calls{0}, g_pd_failed{0}, g_pd_conns_total{0}, g_pd_pairs{0};
std::atomic<int32_t> g_pd_active{0}, g_pd_live{0};

// Loads the PDHMM library once; false (and why, naming the file) when it or one of its functions is missing.
bool pd_load(std::string* err) {
  std::lock_guard<std::mutex> l(g_pd_mu);
  if (g_pd_state == 0) {
    std::string path;
    if (const char* v = getenv("GKL_HIP_PDHMM_LIB")) path = v;
    if (path.empty()) {
      char exe[4096];
      const ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
      path = n > 0 ? std::string(exe, (size_t)n) : std::string();
      const size_t slash = path.rfind('/');
      path = (slash == std::string::npos ? std::string() : path.substr(0, slash + 1)) + "libgklhip_pdhmm.so";
    }
    void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      const char* e = dlerror();
      g_pd_load_err = "this server cannot serve PDHMM: " + path + " does not load (" + (e ? e : "dlopen failed") + ")";
    } else {
      const char* missing = nullptr;
      auto sym = [&](const char* name) { void* p = dlsym(h, name); if (!p && !missing) missing = name; return p; };
      g_pd.init = reinterpret_cast<decltype(g_pd.init)>(sym("gklhip_pdhmm_init"));
      g_pd.set_fma_mode = reinterpret_cast<decltype(g_pd.set_fma_mode)>(sym("gklhip_pdhmm_set_fma_mode"));
      g_pd.set_tail_mode = reinterpret_cast<decltype(g_pd.set_tail_mode)>(sym("gklhip_pdhmm_set_tail_mode"));
      g_pd.compute = reinterpret_cast<decltype(g_pd.compute)>(sym("gklhip_pdhmm_compute"));
      g_pd.compute_cross_batched = reinterpret_cast<decltype(g_pd.compute_cross_batched)>(sym("gklhip_pdhmm_compute_cross_batched"));
      g_pd.last_kernel_ms = reinterpret_cast<decltype(g_pd.last_kernel_ms)>(sym("gklhip_pdhmm_last_kernel_ms"));
      g_pd.last_routing = reinterpret_cast<decltype(g_pd.last_routing)>(sym("gklhip_pdhmm_last_routing"));
      g_pd.done = reinterpret_cast<decltype(g_pd.done)>(sym("gklhip_pdhmm_done"));
      g_pd.last_error = reinterpret_cast<decltype(g_pd.last_error)>(sym("gklhip_pdhmm_last_error"));
      g_pd.combine_counts = reinterpret_cast<decltype(g_pd.combine_counts)>(dlsym(h, "gklhip_pdhmm_combine_counts"));
      if (missing) {
        g_pd.combine_counts = nullptr;
        g_pd_load_err = "this server cannot serve PDHMM: " + path + " has no " + missing;
        dlclose(h);
      }
    }
    g_pd_state = g_pd_load_err.empty() ? 1 : -1;
  }
  *err = g_pd_load_err;
  return g_pd_state == 1;
}

void fill_pd_info(gklhip_pdhmm_server_info* o) {
  memset(o, 0, sizeof *o);
  o->protocol = GKLHIP_SERVER_PROTOCOL;
  o->pid = (int32_t)getpid();
  o->library_state = g_pd_state;
  o->calls_served = g_pd_calls; o->calls_failed = g_pd_failed; o->calls_active = g_pd_active;
  o->live_connections = g_pd_live; o->connections_total = g_pd_conns_total;
  o->pairs_served = g_pd_pairs;
  if (g_pd_state == 1 && g_pd.combine_counts) (void)g_pd.combine_counts(-1, o->combine_counts, 0);
}

void on_signal(int) {
  const char b = 1;
  if (write(g_stop_pipe[1], &b, 1) < 0) {}
}

bool send_all(int fd, const void* p, size_t n) {
  const char* s = static_cast<const char*>(p);
  while (n) {
    const ssize_t k = ::send(fd, s, n, MSG_NOSIGNAL);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return false;
    s += k; n -= (size_t)k;
  }
  return true;
}

bool reply(int fd, int status, const std::string& text, const void* payload = nullptr, uint32_t payload_len = 0) {
  ReplyHead h{status, (uint32_t)std::min<size_t>(text.size(), 4096), payload ? payload_len : 0u, 0u};
  std::string msg;
  msg.reserve(sizeof h + h.text_len + h.payload_len);
  msg.append(reinterpret_cast<const char*>(&h), sizeof h);
  msg.append(text.data(), h.text_len);
  if (payload) msg.append(static_cast<const char*>(payload), payload_len);
  return send_all(fd, msg.data(), msg.size());
}

// One request, and the descriptor that came with it (-1 if none; any further descriptors are closed).  False on EOF,
// a reset or a short message.
bool read_request(int fd, Request* r, int* passed_fd) {
  *passed_fd = -1;
  char* d = reinterpret_cast<char*>(r);
  size_t got = 0;
  while (got < sizeof *r) {
    iovec iov{d + got, sizeof *r - got};
    alignas(cmsghdr) char ctl[CMSG_SPACE(sizeof(int) * 4)];
    msghdr m{};
    m.msg_iov = &iov; m.msg_iovlen = 1;
    m.msg_control = ctl; m.msg_controllen = sizeof ctl;
    const ssize_t k = recvmsg(fd, &m, MSG_CMSG_CLOEXEC);
    if (k < 0 && errno == EINTR) continue;
    for (cmsghdr* c = CMSG_FIRSTHDR(&m); k > 0 && c; c = CMSG_NXTHDR(&m, c)) {
      if (c->cmsg_level != SOL_SOCKET || c->cmsg_type != SCM_RIGHTS) continue;
      const size_t n = (c->cmsg_len - CMSG_LEN(0)) / sizeof(int);
      for (size_t i = 0; i < n; i++) {
        int f;
        memcpy(&f, CMSG_DATA(c) + i * sizeof(int), sizeof f);
        if (*passed_fd < 0) *passed_fd = f; else close(f);
      }
    }
    if (k <= 0) { if (*passed_fd >= 0) { close(*passed_fd); *passed_fd = -1; } return false; }
    got += (size_t)k;
  }
  return true;
}

struct Mapped {
  uint8_t* p = nullptr;
  size_t bytes = 0;
  bool registered = false;
  void release() {
    if (registered) (void)gklhip_host_unregister(p);
    if (p) munmap(p, bytes);
    p = nullptr; bytes = 0; registered = false;
  }
};

// A client arena: the descriptor must be a memfd sealed against shrinking, at least `bytes` long.
int map_arena(int fd, uint64_t bytes, Mapped* out, std::string* err) {
  struct stat sb;
  const int seals = fcntl(fd, F_GET_SEALS);
  if (bytes == 0 || bytes > ((uint64_t)1 << 40)) { *err = "arena size out of range"; return GKLHIP_ERR_INVALID_ARG; }
  if (seals < 0 || !(seals & F_SEAL_SHRINK)) { *err = "the arena must be a memfd sealed against shrinking (F_SEAL_SHRINK)"; return GKLHIP_ERR_INVALID_ARG; }
  if (fstat(fd, &sb) != 0 || (uint64_t)sb.st_size < bytes) { *err = "the arena is smaller than announced"; return GKLHIP_ERR_INVALID_ARG; }
  void* p = mmap(nullptr, (size_t)bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  if (p == MAP_FAILED) { *err = std::string("mmap of the arena: ") + strerror(errno); return GKLHIP_ERR_OOM; }
  out->p = static_cast<uint8_t*>(p);
  out->bytes = (size_t)bytes;
  // page-locked in place: the H2D copies of a call are then DMA straight from the client's pages; else calls are copied
  // into the connection's own pinned staging first (same bits either way)
  out->registered = g_try_register && gklhip_host_register(p, (size_t)bytes) == GKLHIP_OK;
  (out->registered ? g_registered : g_copied)++;
  return GKLHIP_OK;
}

void fill_info(gklhip_server_info* o);

struct Conn {
  int fd = -1;
  std::thread th;
  std::atomic<bool> finished{false};
};

class Session {
 public:
  explicit Session(int fd) : fd_(fd) {}
  ~Session() {
    if (ctx_) gklhip_done(ctx_);
    if (pd_ctx_) (void)g_pd.done(pd_ctx_);
    if (pd_entry_ >= 0) { std::lock_guard<std::mutex> l(g_mu); g_pd_conn_per_entry[(size_t)pd_entry_]--; }
    if (pd_counted_) g_pd_live--;
    if (stage_) gklhip_host_free(stage_);
    arena_.release();
    if (entry_ >= 0) { std::lock_guard<std::mutex> l(g_mu); g_conn_per_entry[(size_t)entry_]--; }
    if (counted_) g_live--;
  }
  void run() {
    Request r;
    int pfd = -1;
    if (!read_request(fd_, &r, &pfd)) return;
    if (pfd >= 0) close(pfd);
    if (r.magic == kMagic && r.type == kPdHello ? !pd_hello(r) : !hello(r)) return;
    while (read_request(fd_, &r, &pfd)) {
      const int keep_fd = pfd;
      pfd = -1;
      if (r.magic != kMagic) { if (keep_fd >= 0) close(keep_fd); refuse(GKLHIP_ERR_INVALID_ARG, "bad magic"); return; }
      if (r.type == kStats) {
        if (keep_fd >= 0) close(keep_fd);
        gklhip_server_info info;
        fill_info(&info);
        if (!reply(fd_, GKLHIP_OK, "", &info, sizeof info)) return;
        continue;
      }
      if (r.type == kPdStats) {
        if (keep_fd >= 0) close(keep_fd);
        gklhip_pdhmm_server_info info;
        fill_pd_info(&info);
        if (!reply(fd_, GKLHIP_OK, "", &info, sizeof info)) return;
        continue;
      }
      if (control_) { if (keep_fd >= 0) close(keep_fd); refuse(GKLHIP_ERR_INVALID_ARG, "a control connection may only ask for stats"); return; }
      if (r.type == kArena) {
        if (keep_fd < 0) { refuse(GKLHIP_ERR_INVALID_ARG, "arena message without a descriptor"); return; }
        Mapped m;
        std::string err;
        const int st = map_arena(keep_fd, r.u.arena.bytes, &m, &err);
        close(keep_fd);
        if (st != GKLHIP_OK) { refuse(st, err); return; }
        arena_.release();
        arena_ = m;
        if (!reply(fd_, GKLHIP_OK, "")) return;
        continue;
      }
      if (keep_fd >= 0) close(keep_fd);
      // a connection is of one kind: a PDHMM connection knows no Compute, a PairHMM connection no PdCompute
      if (r.type != (pd_ ? kPdCompute : kCompute)) { refuse(GKLHIP_ERR_INVALID_ARG, "unknown request type " + std::to_string(r.type)); return; }
      if (pd_ ? !pd_compute(r.u.pd_compute) : !compute(r.u.compute)) return;
    }
  }

 private:
  int fd_;
  bool control_ = false, counted_ = false;
  int entry_ = -1;
  gklhip_ctx* ctx_ = nullptr;
  Mapped arena_;
  uint8_t* stage_ = nullptr;
  size_t stage_cap_ = 0;
  std::vector<int64_t> read_off_, hap_off_;
  // a PDHMM connection: its context, the modes that context is in (-1: as the library made it), its private copies of
  // the two length arrays
  bool pd_ = false, pd_counted_ = false;
  int pd_entry_ = -1;
  gklhip_pdhmm_ctx* pd_ctx_ = nullptr;
  int pd_fma_ = -1, pd_tail_ = -1;
  std::vector<int64_t> pd_hap_len_, pd_read_len_;

  void refuse(int status, const std::string& why) {
    g_refused++;
    (void)reply(fd_, status, why);
  }

  bool hello(const Request& r) {
    if (r.magic != kMagic || r.type != kHello) { refuse(GKLHIP_ERR_INVALID_ARG, "the first message must be a hello"); return false; }
    const Hello& h = r.u.hello;
    if (h.protocol != GKLHIP_SERVER_PROTOCOL || h.abi_version != GKLHIP_ABI_VERSION) {
      refuse(GKLHIP_ERR_UNSUPPORTED, "client speaks protocol " + std::to_string(h.protocol) + " / ABI " + std::to_string(h.abi_version) +
                                         ", this server protocol " + std::to_string(GKLHIP_SERVER_PROTOCOL) + " / ABI " + std::to_string(GKLHIP_ABI_VERSION));
      return false;
    }
    if (h.control) { control_ = true; HelloReply hr{-1, 0}; return reply(fd_, GKLHIP_OK, "", &hr, sizeof hr); }
    gklhip_config cfg = h.cfg;
    cfg.abi_version = GKLHIP_ABI_VERSION;
    cfg.record_events = 0;   // (step times and raw sums are not available remotely)
    {
      std::lock_guard<std::mutex> l(g_mu);
      if (!g_devices.empty()) {
        // the listed device with the fewest connections (the first of them on a tie)
        entry_ = (int)(std::min_element(g_conn_per_entry.begin(), g_conn_per_entry.end()) - g_conn_per_entry.begin());
        g_conn_per_entry[(size_t)entry_]++;
        cfg.device = g_devices[(size_t)entry_];
      } else {
        const int32_t d = std::max(0, cfg.device);
        if (std::find(g_used.begin(), g_used.end(), d) == g_used.end() && g_used.size() < GKLHIP_SERVER_MAX_DEVICES) g_used.push_back(d);
      }
    }
    const int st = gklhip_init(&cfg, &ctx_);
    if (st != GKLHIP_OK) {
      const char* e = gklhip_last_error();
      ctx_ = nullptr;
      (void)reply(fd_, st, std::string("gklhip_init on the server: ") + (e ? e : ""));
      return false;
    }
    counted_ = true;
    g_live++;
    g_conns_total++;
    HelloReply hr{cfg.device, gklhip_num_devices(ctx_)};
    return reply(fd_, GKLHIP_OK, "", &hr, sizeof hr);
  }

  bool pd_hello(const Request& r) {
    const PdHello& h = r.u.pd_hello;
    if (h.protocol != GKLHIP_SERVER_PROTOCOL || h.abi_version != GKLHIP_ABI_VERSION) {
      refuse(GKLHIP_ERR_UNSUPPORTED, "client speaks protocol " + std::to_string(h.protocol) + " / ABI " + std::to_string(h.abi_version) +
                                         ", this server protocol " + std::to_string(GKLHIP_SERVER_PROTOCOL) + " / ABI " + std::to_string(GKLHIP_ABI_VERSION));
      return false;
    }
    std::string err;
    if (!pd_load(&err)) { refuse(GKLHIP_ERR_UNSUPPORTED, err); return false; }
    pd_ = true;
    int32_t device = std::max(0, h.device);
    if (!g_devices.empty()) {
      // the listed device with the fewest connections of both kinds (the first of them on a tie)
      std::lock_guard<std::mutex> l(g_mu);
      pd_entry_ = 0;
      for (size_t i = 1; i < g_devices.size(); i++)
        if (g_conn_per_entry[i] + g_pd_conn_per_entry[i] < g_conn_per_entry[(size_t)pd_entry_] + g_pd_conn_per_entry[(size_t)pd_entry_]) pd_entry_ = (int)i;
      g_pd_conn_per_entry[(size_t)pd_entry_]++;
      device = g_devices[(size_t)pd_entry_];
    }
    const int st = g_pd.init(device, &pd_ctx_);
    if (st != GKLHIP_OK) {
      const char* e = g_pd.last_error();
      pd_ctx_ = nullptr;
      (void)reply(fd_, st, std::string("gklhip_pdhmm_init on the server: ") + (e ? e : ""));
      return false;
    }
    pd_counted_ = true;
    g_pd_live++;
    g_pd_conns_total++;
    return reply(fd_, GKLHIP_OK, "", &device, sizeof device);
  }

  // [off, off + len) inside the arena, 8-byte aligned where `align8`
  bool inside(uint64_t off, uint64_t len, bool align8) const {
    return off <= arena_.bytes && len <= arena_.bytes - off && (!align8 || off % 8 == 0);
  }

  bool pd_compute(const PdCompute& q);

  bool compute(const Compute& q) {
    if (!arena_.p) { refuse(GKLHIP_ERR_INVALID_ARG, "call before any arena"); return false; }
    if (q.n_reads < 0 || q.n_haps < 0) { refuse(GKLHIP_ERR_INVALID_ARG, "negative read or haplotype count"); return false; }
    const uint64_t n_pairs = (uint64_t)q.n_reads * (uint64_t)q.n_haps;
    if (!inside(q.read_off, ((uint64_t)q.n_reads + 1) * 8, true) || !inside(q.hap_off, ((uint64_t)q.n_haps + 1) * 8, true) ||
        !inside(q.out, n_pairs * 8, true)) {
      refuse(GKLHIP_ERR_INVALID_ARG, "offset array or output outside the arena");
      return false;
    }
    // the offsets are copied out of the shared pages before they are checked: the client cannot change them under the call
    read_off_.resize((size_t)q.n_reads + 1);
    hap_off_.resize((size_t)q.n_haps + 1);
    memcpy(read_off_.data(), arena_.p + q.read_off, read_off_.size() * 8);
    memcpy(hap_off_.data(), arena_.p + q.hap_off, hap_off_.size() * 8);
    for (const std::vector<int64_t>* v : {&read_off_, &hap_off_}) {
      if ((*v)[0] != 0) { refuse(GKLHIP_ERR_INVALID_ARG, "offset arrays must start at 0"); return false; }
      for (size_t i = 1; i < v->size(); i++)
        if ((*v)[i] < (*v)[i - 1]) { refuse(GKLHIP_ERR_INVALID_ARG, "read_off / hap_off not monotone"); return false; }
    }
    const uint64_t rl = (uint64_t)read_off_.back(), hl = (uint64_t)hap_off_.back();
    const uint64_t rd[5] = {q.read_bases, q.read_quals, q.ins_gop, q.del_gop, q.gcp};
    for (uint64_t o : rd)
      if (!inside(o, rl, false)) { refuse(GKLHIP_ERR_INVALID_ARG, "a read array lies outside the arena"); return false; }
    if (!inside(q.hap_bases, hl, false)) { refuse(GKLHIP_ERR_INVALID_ARG, "haplotype bases outside the arena"); return false; }
    gklhip_batch b;
    b.n_reads = q.n_reads; b.n_haps = q.n_haps;
    b.read_off = read_off_.data(); b.hap_off = hap_off_.data();
    const uint8_t* a = arena_.p;
    if (arena_.registered) {
      b.read_bases = a + q.read_bases; b.read_quals = a + q.read_quals; b.ins_gop = a + q.ins_gop;
      b.del_gop = a + q.del_gop; b.gcp = a + q.gcp; b.hap_bases = a + q.hap_bases;
    } else {
      const size_t need = 5 * (size_t)rl + (size_t)hl + 1;
      if (need > stage_cap_) {
        if (stage_) gklhip_host_free(stage_);
        stage_cap_ = std::max(need, 2 * stage_cap_);
        stage_ = static_cast<uint8_t*>(gklhip_host_alloc(stage_cap_));
        if (!stage_) { stage_cap_ = 0; g_calls++; g_failed++; return reply(fd_, GKLHIP_ERR_OOM, "pinned staging allocation failed"); }
      }
      uint8_t* s = stage_;
      const uint8_t** dst[5] = {&b.read_bases, &b.read_quals, &b.ins_gop, &b.del_gop, &b.gcp};
      for (int i = 0; i < 5; i++) { memcpy(s, a + rd[i], (size_t)rl); *dst[i] = s; s += rl; }
      memcpy(s, a + q.hap_bases, (size_t)hl);
      b.hap_bases = s;
    }
    g_active++;
    const int st = gklhip_compute(ctx_, &b, reinterpret_cast<double*>(arena_.p + q.out));
    const char* e = st == GKLHIP_OK ? "" : gklhip_last_error();
    const std::string err = e ? e : "";
    g_active--;
    g_calls++;
    if (st != GKLHIP_OK) g_failed++;
    gklhip_stats stats;
    memset(&stats, 0, sizeof stats);
    (void)gklhip_get_stats(ctx_, &stats);
    return reply(fd_, st, err, &stats, sizeof stats);
  }
};

bool Session::pd_compute(const PdCompute& q) {
  auto bad = [&](const std::string& why) { refuse(GKLHIP_ERR_INVALID_ARG, why); return false; };
  if (!arena_.p) return bad("call before any arena");
  if (q.layout != 0 && q.layout != 1) return bad("unknown layout " + std::to_string(q.layout));
  if (q.n_read_items < 0 || q.n_hap_items < 0) return bad("negative read or haplotype count");
  if (q.max_hap_len <= 0 || q.max_read_len <= 0) return bad("row strides must be greater than 0");
  if (q.layout == 0 && q.n_read_items != q.n_hap_items) return bad("the paired layout wants as many reads as haplotypes");
  const uint64_t nr = (uint64_t)q.n_read_items, nh = (uint64_t)q.n_hap_items;
  const uint64_t n_pairs = q.layout == 0 ? nr : nr * nh;   // (two counts below 2^31: no overflow)
  if (n_pairs > 0x7fffffffull) return bad("more than 2^31 - 1 pairs");
  uint64_t hap_bytes, read_bytes;
  if (__builtin_mul_overflow(nh, (uint64_t)q.max_hap_len, &hap_bytes) || __builtin_mul_overflow(nr, (uint64_t)q.max_read_len, &read_bytes))
    return bad("array size overflows");
  if (!inside(q.hap_lengths, nh * 8, false) || !inside(q.read_lengths, nr * 8, false) || !inside(q.out, n_pairs * 8, true))
    return bad("length array or output outside the arena");
  const uint64_t hp[2] = {q.hap_bases, q.hap_pdbases};
  const uint64_t rd[5] = {q.read_bases, q.read_qual, q.read_ins_qual, q.read_del_qual, q.gcp};
  for (uint64_t o : hp) if (!inside(o, hap_bytes, false)) return bad("a haplotype array lies outside the arena");
  for (uint64_t o : rd) if (!inside(o, read_bytes, false)) return bad("a read array lies outside the arena");
  // the lengths are copied out of the shared pages before they are checked: the client cannot change them under the call
  pd_hap_len_.resize((size_t)nh);
  pd_read_len_.resize((size_t)nr);
  if (nh) memcpy(pd_hap_len_.data(), arena_.p + q.hap_lengths, (size_t)nh * 8);
  if (nr) memcpy(pd_read_len_.data(), arena_.p + q.read_lengths, (size_t)nr * 8);
  for (int64_t v : pd_hap_len_) if (v < 1 || v > q.max_hap_len) return bad("a haplotype length outside 1.." + std::to_string(q.max_hap_len));
  for (int64_t v : pd_read_len_) if (v < 1 || v > q.max_read_len) return bad("a read length outside 1.." + std::to_string(q.max_read_len));
  const uint8_t* a = arena_.p;
  const int8_t* arr[7];
  if (arena_.registered) {
    for (int i = 0; i < 2; i++) arr[i] = reinterpret_cast<const int8_t*>(a + hp[i]);
    for (int i = 0; i < 5; i++) arr[2 + i] = reinterpret_cast<const int8_t*>(a + rd[i]);
  } else {
    const size_t need = 2 * (size_t)hap_bytes + 5 * (size_t)read_bytes + 1;
    if (need > stage_cap_) {
      if (stage_) gklhip_host_free(stage_);
      stage_cap_ = std::max(need, 2 * stage_cap_);
      stage_ = static_cast<uint8_t*>(gklhip_host_alloc(stage_cap_));
      if (!stage_) { stage_cap_ = 0; g_pd_calls++; g_pd_failed++; return reply(fd_, GKLHIP_ERR_OOM, "pinned staging allocation failed"); }
    }
    uint8_t* s = stage_;
    for (int i = 0; i < 2; i++) { memcpy(s, a + hp[i], (size_t)hap_bytes); arr[i] = reinterpret_cast<const int8_t*>(s); s += hap_bytes; }
    for (int i = 0; i < 5; i++) { memcpy(s, a + rd[i], (size_t)read_bytes); arr[2 + i] = reinterpret_cast<const int8_t*>(s); s += read_bytes; }
  }
  double* out = reinterpret_cast<double*>(arena_.p + q.out);
  g_pd_active++;
  // fma_mode and tail_mode come with every call; the context is told only when one of them changes
  const int fma = q.flags & 1, tail = (q.flags >> 1) & 1;
  int st = GKLHIP_OK;
  if (fma != pd_fma_ && (st = g_pd.set_fma_mode(pd_ctx_, fma)) == GKLHIP_OK) pd_fma_ = fma;
  if (st == GKLHIP_OK && tail != pd_tail_ && (st = g_pd.set_tail_mode(pd_ctx_, tail)) == GKLHIP_OK) pd_tail_ = tail;
  if (st == GKLHIP_OK) {
    if (q.layout == 0) {
      const gklhip_pdhmm_batch b = {q.n_read_items, q.max_hap_len, q.max_read_len, arr[0], arr[1], arr[2], arr[3], arr[4], arr[5], arr[6],
                                    pd_hap_len_.data(), pd_read_len_.data()};
      st = g_pd.compute(pd_ctx_, &b, out);
    } else {
      const gklhip_pdhmm_cross x = {q.n_read_items, q.n_hap_items, q.max_hap_len, q.max_read_len, arr[0], arr[1], arr[2], arr[3], arr[4],
                                    arr[5], arr[6], pd_hap_len_.data(), pd_read_len_.data()};
      st = g_pd.compute_cross_batched(pd_ctx_, &x, q.ref_batch_pairs, out);
    }
  }
  // an error of the library goes back with its status and its exact text; the connection stays usable
  const char* e = st == GKLHIP_OK ? "" : g_pd.last_error();
  const std::string err = e ? e : "";
  g_pd_active--;
  g_pd_calls++;
  if (st != GKLHIP_OK) g_pd_failed++; else g_pd_pairs += (int64_t)n_pairs;
  PdComputeReply rep{};
  if (st == GKLHIP_OK) {
    rep.kernel_ms = g_pd.last_kernel_ms(pd_ctx_);
    (void)g_pd.last_routing(pd_ctx_, rep.routing);
  }
  return reply(fd_, st, err, &rep, sizeof rep);
}

void fill_info(gklhip_server_info* o) {
  memset(o, 0, sizeof *o);
  o->protocol = GKLHIP_SERVER_PROTOCOL;
  o->pid = (int32_t)getpid();
  o->calls_served = g_calls; o->calls_failed = g_failed; o->calls_active = g_active;
  o->live_connections = g_live; o->connections_total = g_conns_total;
  o->arenas_registered = g_registered; o->arenas_copied = g_copied; o->requests_refused = g_refused;
  std::lock_guard<std::mutex> l(g_mu);
  const std::vector<int32_t>& devs = g_devices.empty() ? g_used : g_devices;
  o->n_devices = (int32_t)std::min<size_t>(devs.size(), GKLHIP_SERVER_MAX_DEVICES);
  for (int i = 0; i < o->n_devices; i++) {
    o->device[i] = devs[(size_t)i];
    o->connections[i] = g_devices.empty() ? 0 : g_conn_per_entry[(size_t)i];
    (void)gklhip_small_call_counts(devs[(size_t)i], o->small_calls[i], 0);
  }
  if (g_devices.empty() && o->n_devices == 1) o->connections[0] = g_live;
}

void serve(int fd) {
  try {
    Session s(fd);
    s.run();
  } catch (...) {   // (bad_alloc of a huge client request: that connection ends, the server goes on)
  }
}

// The listening socket, mode 0600.  A stale socket file nobody listens on is replaced; a live one is an error.
int listen_on(const std::string& path) {
  sockaddr_un a{};
  a.sun_family = AF_UNIX;
  if (path.empty() || path.size() >= sizeof a.sun_path) { fprintf(stderr, "gklhip_server: bad socket path\n"); return -1; }
  memcpy(a.sun_path, path.c_str(), path.size() + 1);
  struct stat sb;
  if (lstat(path.c_str(), &sb) == 0) {
    if (!S_ISSOCK(sb.st_mode)) { fprintf(stderr, "gklhip_server: %s exists and is not a socket\n", path.c_str()); return -1; }
    const int probe = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    const bool live = probe >= 0 && connect(probe, reinterpret_cast<sockaddr*>(&a), sizeof a) == 0;
    if (probe >= 0) close(probe);
    if (live) { fprintf(stderr, "gklhip_server: another server listens on %s\n", path.c_str()); return -1; }
    unlink(path.c_str());
  }
  const int fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
  if (fd < 0) { perror("gklhip_server: socket"); return -1; }
  const mode_t old = umask(0177);
  const int rc = bind(fd, reinterpret_cast<sockaddr*>(&a), sizeof a);
  umask(old);
  if (rc != 0 || chmod(path.c_str(), 0600) != 0 || listen(fd, 128) != 0) {
    fprintf(stderr, "gklhip_server: cannot listen on %s: %s\n", path.c_str(), strerror(errno));
    close(fd);
    return -1;
  }
  return fd;
}

bool parse_devices(const char* s, std::vector<int32_t>* out) {
  while (*s) {
    char* end = nullptr;
    const long d = strtol(s, &end, 10);
    if (end == s || d < 0 || d > 1023) return false;
    out->push_back((int32_t)d);
    s = end;
    if (*s == ',') s++;
    else if (*s) return false;
  }
  return !out->empty() && out->size() <= GKLHIP_SERVER_MAX_DEVICES;
}

}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--socket") && i + 1 < argc) g_socket = argv[++i];
    else if (!strcmp(argv[i], "--devices") && i + 1 < argc) {
      if (!parse_devices(argv[++i], &g_devices)) { fprintf(stderr, "gklhip_server: --devices wants a list like 0,1,2\n"); return 2; }
    } else {
      fprintf(stderr, "usage: %s --socket PATH [--devices 0,1,...]\n", argv[0]);
      return 2;
    }
  }
  if (g_socket.empty()) { fprintf(stderr, "usage: %s --socket PATH [--devices 0,1,...]\n", argv[0]); return 2; }
  unsetenv("GKL_HIP_SERVER");   // the server's own contexts are local (it must never connect to itself)
  if (const char* v = getenv("GKL_HIP_SERVER_REGISTER")) g_try_register = atoi(v) != 0;
  g_conn_per_entry.assign(g_devices.size(), 0);
  g_pd_conn_per_entry.assign(g_devices.size(), 0);
  signal(SIGPIPE, SIG_IGN);
  if (pipe2(g_stop_pipe, O_CLOEXEC) != 0) { perror("gklhip_server: pipe"); return 1; }
  struct sigaction sa{};
  sa.sa_handler = on_signal;
  sigemptyset(&sa.sa_mask);
  sigaction(SIGTERM, &sa, nullptr);
  sigaction(SIGINT, &sa, nullptr);
  const int lfd = listen_on(g_socket);
  if (lfd < 0) return 1;
  printf("ready\n");
  fflush(stdout);
  const uid_t me = geteuid();
  std::list<std::unique_ptr<Conn>> conns;
  for (;;) {
    pollfd p[2] = {{lfd, POLLIN, 0}, {g_stop_pipe[0], POLLIN, 0}};
    const int n = poll(p, 2, 1000);
    for (auto it = conns.begin(); it != conns.end();) {   // reap finished connections
      if ((*it)->finished) { (*it)->th.join(); close((*it)->fd); it = conns.erase(it); }
      else ++it;
    }
    if (n < 0 && errno == EINTR) continue;
    if (n > 0 && p[1].revents) break;
    if (n <= 0 || !(p[0].revents & POLLIN)) continue;
    const int cfd = accept4(lfd, nullptr, nullptr, SOCK_CLOEXEC);
    if (cfd < 0) continue;
    ucred cr{};
    socklen_t len = sizeof cr;
    if (getsockopt(cfd, SOL_SOCKET, SO_PEERCRED, &cr, &len) != 0 || cr.uid != me) {
      g_refused++;
      (void)reply(cfd, GKLHIP_ERR_INVALID_ARG, "refused: the peer's uid is not the server's");
      close(cfd);
      continue;
    }
    std::unique_ptr<Conn> c(new Conn());
    c->fd = cfd;
    Conn* raw = c.get();
    try {
      c->th = std::thread([raw] { serve(raw->fd); raw->finished = true; });
    } catch (...) {
      close(cfd);
      continue;
    }
    conns.push_back(std::move(c));
  }
  // SIGTERM: no new connections; every connection finishes the call it is in, then sees end-of-file
  close(lfd);
  unlink(g_socket.c_str());
  for (auto& c : conns) shutdown(c->fd, SHUT_RD);
  for (auto& c : conns) { c->th.join(); close(c->fd); }
  fprintf(stderr, "gklhip_server: stopped after %lld calls\n", (long long)(g_calls.load() + g_pd_calls.load()));
  return 0;
}
