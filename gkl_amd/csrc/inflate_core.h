// RFC 1951 decoder, written once: the only copy of the dynamic-header parsing, the table construction, the symbol loop
// and the bounds rules.  inflate_kernel.h instantiates it for a wavefront (64 lanes), tests/native/inflate_core_check.cpp
// for one host thread under the address and undefined-behaviour sanitizers.  The two differ in the execution policy X
// only -- how a step is carried out (a lane-strided loop over 64 lanes or over one), never in what the step decides:
//   X::kLanes, X::lane()   the lanes that share one stream; every lane runs every statement below with the same
//                          wave-uniform state (bit reader, positions, status), lane-strided loops split the bulk work
//   X::sync()              everything the lanes stored before it (tables, output bytes) is visible to all of them after it
// Acceptance rules are zlib's inflate() with windowBits = -15; the status of a stream is the first condition met in
// stream order.  Nothing is written outside [dst, dst + cap) and nothing is read outside [src, src + src_len).
#pragma once
#include <stdint.h>

#ifndef GKL_INF_FN
#define GKL_INF_FN inline   // the kernel's translation unit defines it as __device__ __forceinline__
#endif

namespace gklinf {

enum Status : int32_t { ST_OK = 0, ST_INVALID_BLOCK = 1, ST_INVALID_SYMBOL = 2, ST_INVALID_LOOKBACK = 3, ST_END_INPUT = 4, ST_OUT_OVERFLOW = 5 };

constexpr int kFastBits = 10;             // codes up to this length decode with one table read
constexpr uint32_t kInvalidSym = 0x1FF;   // table entry of a bit pattern that no code of an incomplete set owns
constexpr int kCrcChunks = 64;            // the CRC is taken over this many contiguous chunks, then combined
enum TableKind { KIND_CODES = 0, KIND_LENS = 1, KIND_DISTS = 2 };

// One Huffman table: `fast` is indexed by the next kFastBits bits of the stream, an entry is (symbol << 4) | length and
// 0 sends a longer code to the canonical walk over `count` and `sorted`.
struct Huff {
  uint16_t fast[1 << kFastBits];
  uint16_t sorted[288];   // symbols in order of (length, symbol)
  uint16_t count[16];     // codes per length
  uint16_t next[16];      // next code to assign per length (lane 0, while it assigns)
  uint16_t offs[16];      // next slot of `sorted` per length
};

// Working memory of one stream at a time: LDS of the wavefront on the device (7.6 KB).
struct Scratch {
  Huff lit, dist;         // `dist` also holds the code-length code while a dynamic header is read
  uint8_t lens[320];      // code lengths: literal/length symbols, then the distance symbols
  uint16_t code[320];     // the canonical code of each symbol
  uint32_t crc_tab[256];
  uint32_t crc_part[kCrcChunks];
};

GKL_INF_FN uint32_t bit_reverse(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1u); v >>= 1; }
  return r;
}

// zlib's inflate_table(): 0 = usable, 1 = over-subscribed or (not allowed to be) incomplete.  An incomplete set passes
// only for literal/length or distance codes whose only code has length 1; a set with no code at all passes for every
// kind.  In both, the patterns that no code owns decode as (kInvalidSym, 1 bit).
template <class X>
GKL_INF_FN int build_table(Huff& h, const uint8_t* lens, uint16_t* code, int n, int kind) {
  const int lane = X::lane();
  for (int l = lane; l < 16; l += X::kLanes) {
    int c = 0;
    for (int s = 0; s < n; s++) c += lens[s] == l;
    h.count[l] = (uint16_t)c;
  }
  X::sync();
  int max = 0, left = 1;
  bool over = false;
  for (int l = 1; l <= 15; l++) {
    const int c = h.count[l];
    if (c) max = l;
    left = (left << 1) - c;
    if (left < 0) { over = true; break; }
  }
  if (over) return 1;
  if (max != 0 && left > 0 && (kind == KIND_CODES || max != 1)) return 1;
  const bool incomplete = max == 0 || left > 0;
  const uint16_t fill = incomplete ? (uint16_t)((kInvalidSym << 4) | 1u) : (uint16_t)0;
  for (int i = lane; i < (1 << kFastBits); i += X::kLanes) h.fast[i] = fill;
  if (lane == 0) {
    // the canonical codes, in symbol order
    uint32_t c = 0, off = 0;
    for (int l = 1; l <= 15; l++) {
      h.next[l] = (uint16_t)c;
      h.offs[l] = (uint16_t)off;
      c = (c + h.count[l]) << 1;
      off += h.count[l];
    }
    for (int s = 0; s < n; s++) {
      const int l = lens[s];
      if (l) { code[s] = h.next[l]++; h.sorted[h.offs[l]++] = (uint16_t)s; }
    }
  }
  X::sync();
  // each lane fills the entries of its own symbols
  for (int s = lane; s < n; s += X::kLanes) {
    const int l = lens[s];
    if (l == 0 || l > kFastBits) continue;
    const uint16_t e = (uint16_t)((s << 4) | l);
    for (uint32_t i = bit_reverse(code[s], l); i < (1u << kFastBits); i += 1u << l) h.fast[i] = e;
  }
  X::sync();
  return 0;
}

// `bits`: the next bits of the stream, zero beyond its end.  The caller compares *len with the bits it really has.
GKL_INF_FN void decode_symbol(const Huff& h, uint32_t bits, uint32_t* sym, uint32_t* len) {
  const uint32_t e = h.fast[bits & ((1u << kFastBits) - 1)];
  if (e) { *sym = e >> 4; *len = e & 15u; return; }
  // a code longer than kFastBits of a complete set: canonical walk, one bit at a time
  int32_t c = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; l++) {
    c |= (int32_t)((bits >> (l - 1)) & 1u);
    const int32_t cnt = h.count[l];
    if (c - cnt < first) { *sym = h.sorted[index + (c - first)]; *len = (uint32_t)l; return; }
    index += cnt;
    first = (first + cnt) << 1;
    c <<= 1;
  }
  *sym = kInvalidSym; *len = 1;   // not reached: a set with a 0 entry is complete
}

template <class X>
struct Inflater {
  Scratch& S;
  const uint8_t* src;
  uint32_t n;           // bytes of input
  uint8_t* dst;
  uint32_t cap;
  // bit reader: `hold` has `nbits` bits of the stream that are not consumed yet; src[ip] is the next byte to load
  uint64_t hold = 0;
  uint32_t nbits = 0, ip = 0;
  // output: bytes [0, pos) are stored, `npend` literals behind them wait in the lanes' `mylit`
  uint32_t pos = 0, npend = 0;
  uint8_t mylit = 0;

  GKL_INF_FN Inflater(Scratch& s, const uint8_t* src_, uint32_t n_, uint8_t* dst_, uint32_t cap_) : S(s), src(src_), n(n_), dst(dst_), cap(cap_) {}

  GKL_INF_FN void refill() {
    while (nbits <= 56 && ip < n) { hold |= (uint64_t)src[ip++] << nbits; nbits += 8; }
  }
  GKL_INF_FN uint32_t peek(uint32_t k) const { return (uint32_t)hold & ((1u << k) - 1u); }   // k <= 16
  GKL_INF_FN void drop(uint32_t k) { hold >>= k; nbits -= k; }
  GKL_INF_FN uint32_t take(uint32_t k) { const uint32_t v = peek(k); drop(k); return v; }

  GKL_INF_FN void flush_literals() {
    if ((uint32_t)X::lane() < npend) dst[pos + (uint32_t)X::lane()] = mylit;
    pos += npend;
    npend = 0;
  }

  GKL_INF_FN int stored_block() {
    drop(nbits & 7u);
    refill();
    if (nbits < 32) return ST_END_INPUT;
    const uint32_t len = take(16), nlen = take(16);
    if (len != (nlen ^ 0xFFFFu)) return ST_INVALID_BLOCK;
    ip -= nbits >> 3;   // whole bytes go back: the block's bytes are copied from src directly
    hold = 0; nbits = 0;
    flush_literals();
    const uint32_t avail = n - ip, room = cap - pos;
    uint32_t ncopy = len < avail ? len : avail;
    if (room < ncopy) ncopy = room;
    for (uint32_t i = (uint32_t)X::lane(); i < ncopy; i += X::kLanes) dst[pos + i] = src[ip + i];
    pos += ncopy; ip += ncopy;
    if (ncopy < len) return ncopy == avail ? ST_END_INPUT : ST_OUT_OVERFLOW;
    return ST_OK;
  }

  GKL_INF_FN int fixed_tables() {
    for (int s = X::lane(); s < 320; s += X::kLanes) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    X::sync();
    build_table<X>(S.lit, S.lens, S.code, 288, KIND_LENS);
    build_table<X>(S.dist, S.lens + 288, S.code + 288, 32, KIND_DISTS);
    return ST_OK;
  }

  GKL_INF_FN int dynamic_tables() {
    refill();
    if (nbits < 14) return ST_END_INPUT;
    const uint32_t hlit = take(5) + 257, hdist = take(5) + 1, hclen = take(4) + 4;
    if (hlit > 286 || hdist > 30) return ST_INVALID_BLOCK;
    for (int s = X::lane(); s < 19; s += X::kLanes) S.lens[s] = 0;
    X::sync();
    for (uint32_t i = 0; i < hclen; i++) {
      refill();
      if (nbits < 3) return ST_END_INPUT;
      const uint32_t v = take(3);
      // the order of the code-length code lengths (RFC 1951 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
      const uint32_t slot = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 8 - ((i - 3) >> 1) : 7 + ((i - 2) >> 1);
      if (X::lane() == 0) S.lens[slot] = (uint8_t)v;
    }
    X::sync();
    if (build_table<X>(S.dist, S.lens, S.code, 19, KIND_CODES)) return ST_INVALID_BLOCK;
    const uint32_t total = hlit + hdist;
    uint32_t have = 0, prev = 0;
    while (have < total) {
      refill();
      uint32_t sym, len;
      decode_symbol(S.dist, (uint32_t)hold, &sym, &len);
      if (len > nbits) return ST_END_INPUT;
      if (sym == kInvalidSym) sym = 0;   // zlib: with no code-length code at all, every pattern reads as length 0, one bit
      if (sym < 16) {
        drop(len);
        if (X::lane() == 0) S.lens[have] = (uint8_t)sym;
        have++;
        prev = sym;
        continue;
      }
      const uint32_t extra = sym == 16 ? 2 : sym == 17 ? 3 : 7;
      if (nbits < len + extra) return ST_END_INPUT;
      drop(len);
      uint32_t rep, v;
      if (sym == 16) {
        if (have == 0) return ST_INVALID_BLOCK;
        v = prev;
        rep = 3 + take(2);
      } else {
        v = 0;
        rep = (sym == 17 ? 3 : 11) + take(extra);
      }
      if (have + rep > total) return ST_INVALID_BLOCK;
      for (uint32_t i = (uint32_t)X::lane(); i < rep; i += X::kLanes) S.lens[have + i] = (uint8_t)v;
      have += rep;
      prev = v;
    }
    X::sync();
    if (S.lens[256] == 0) return ST_INVALID_BLOCK;   // no end-of-block code
    const int bad_lit = build_table<X>(S.lit, S.lens, S.code, (int)hlit, KIND_LENS);
    if (bad_lit) return ST_INVALID_BLOCK;
    if (build_table<X>(S.dist, S.lens + hlit, S.code + hlit, (int)hdist, KIND_DISTS)) return ST_INVALID_BLOCK;
    return ST_OK;
  }

  GKL_INF_FN int coded_block() {
    for (;;) {
      refill();   // 56 bits or the rest of the input: a whole token needs at most 15 + 5 + 15 + 13
      uint32_t sym, len;
      decode_symbol(S.lit, (uint32_t)hold, &sym, &len);
      if (len > nbits) return ST_END_INPUT;
      if (sym == kInvalidSym) return ST_INVALID_SYMBOL;
      drop(len);
      if (sym < 256) {
        if (pos + npend >= cap) return ST_OUT_OVERFLOW;
        if ((uint32_t)X::lane() == npend) mylit = (uint8_t)sym;
        if (++npend == (uint32_t)X::kLanes) flush_literals();
        continue;
      }
      if (sym == 256) return ST_OK;
      if (sym >= 286) return ST_INVALID_SYMBOL;
      const uint32_t li = sym - 257;
      const uint32_t lext = li < 8 || li == 28 ? 0 : (li - 4) >> 2;
      const uint32_t lbase = li < 8 ? 3 + li : li == 28 ? 258 : 3 + ((4 + (li & 3u)) << lext);
      if (nbits < lext) return ST_END_INPUT;
      const uint32_t length = lbase + take(lext);
      uint32_t ds, dl;
      decode_symbol(S.dist, (uint32_t)hold, &ds, &dl);
      if (dl > nbits) return ST_END_INPUT;
      if (ds >= 30) return ST_INVALID_SYMBOL;   // kInvalidSym too
      drop(dl);
      const uint32_t dext = ds < 4 ? 0 : (ds - 2) >> 1;
      const uint32_t dbase = ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1u)) << dext);
      if (nbits < dext) return ST_END_INPUT;
      const uint32_t dist = dbase + take(dext);
      if (dist > pos + npend) return ST_INVALID_LOOKBACK;
      flush_literals();
      X::sync();   // the run reads bytes that other lanes stored
      const uint32_t room = cap - pos;
      const uint32_t ncopy = length < room ? length : room;
      // lane i copies byte i of the run from pos - dist + (i mod dist): every source lies before pos
      for (uint32_t i = (uint32_t)X::lane(); i < ncopy; i += X::kLanes) dst[pos + i] = dst[pos - dist + (i % dist)];
      pos += ncopy;
      if (ncopy < length) return ST_OUT_OVERFLOW;
    }
  }

  GKL_INF_FN int blocks() {
    for (;;) {
      refill();
      if (nbits < 3) return ST_END_INPUT;
      const uint32_t bfinal = take(1), btype = take(2);
      int st;
      if (btype == 0) st = stored_block();
      else if (btype == 3) st = ST_INVALID_BLOCK;
      else {
        st = btype == 1 ? fixed_tables() : dynamic_tables();
        if (st == ST_OK) st = coded_block();
      }
      if (st != ST_OK) return st;
      if (bfinal) return ST_OK;
    }
  }

  GKL_INF_FN int run(int32_t* out_len, int32_t* consumed) {
    const int st = blocks();
    flush_literals();
    X::sync();
    *out_len = (int32_t)pos;
    *consumed = (int32_t)(st == ST_END_INPUT ? n : ip - (nbits >> 3));   // whole bytes that were loaded ahead go back
    return st;
  }
};

// One stream, 0 <= src_len, cap <= 2^31 - 1.  Every lane returns the same status, length and count.
template <class X>
GKL_INF_FN int inflate_stream(Scratch& S, const uint8_t* src, int32_t src_len, uint8_t* dst, int32_t cap, int32_t* out_len, int32_t* consumed) {
  Inflater<X> inf(S, src, (uint32_t)src_len, dst, (uint32_t)cap);
  return inf.run(out_len, consumed);
}

// ---- CRC-32 (the zlib / BGZF polynomial, reflected: x^0 is bit 31)
constexpr uint32_t kCrcPoly = 0xEDB88320u;

GKL_INF_FN uint32_t crc_mulmod(uint32_t a, uint32_t b) {   // a(x) * b(x) mod P
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
GKL_INF_FN uint32_t crc_xpow8(uint32_t len) {   // x^(8 * len) mod P
  uint32_t r = 0x80000000u, b = 0x00800000u;
  for (; len; len >>= 1) {
    if (len & 1u) r = crc_mulmod(r, b);
    b = crc_mulmod(b, b);
  }
  return r;
}

// CRC-32 of buf[0, len): kCrcChunks contiguous chunks, one per lane, through a byte table, then combined in order by the
// operator of zlib's crc32_combine: crc(A B) = crc(A) * x^(8 |B|) + crc(B).
template <class X>
GKL_INF_FN uint32_t crc32_stream(Scratch& S, const uint8_t* buf, uint32_t len) {
  for (uint32_t i = (uint32_t)X::lane(); i < 256; i += X::kLanes) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    S.crc_tab[i] = c;
  }
  X::sync();
  const uint32_t chunk = (uint32_t)(((uint64_t)len + kCrcChunks - 1) / kCrcChunks);
  for (uint32_t c = (uint32_t)X::lane(); c < (uint32_t)kCrcChunks; c += X::kLanes) {
    const uint64_t b64 = (uint64_t)c * chunk;
    const uint32_t beg = b64 < len ? (uint32_t)b64 : len;
    const uint32_t end = len - beg < chunk ? len : beg + chunk;
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = beg; i < end; i++) crc = S.crc_tab[(crc ^ buf[i]) & 0xFFu] ^ (crc >> 8);
    S.crc_part[c] = ~crc;
  }
  X::sync();
  const uint32_t xfull = crc_xpow8(chunk);
  uint32_t total = 0;
  for (uint32_t c = 0; c < (uint32_t)kCrcChunks; c++) {
    const uint64_t b64 = (uint64_t)c * chunk;
    if (b64 >= len) break;
    const uint32_t l = len - (uint32_t)b64 < chunk ? len - (uint32_t)b64 : chunk;
    total = crc_mulmod(l == chunk ? xfull : crc_xpow8(l), total) ^ S.crc_part[c];
  }
  X::sync();   // crc_part is free again
  return total;
}

}  // namespace gklinf
