// RFC 1951 encoder, written once: match search, greedy or lazy selection, histograms, length-limited code construction, the
// block-type decision by exact bit count and the bit packing.  deflate_kernel.h instantiates it for a wavefront
// (64 lanes), tests/native/deflate_core_check.cpp for one host thread and for four (under the sanitizers).  The execution
// policy X says how a step is carried out, never what it decides:
//   X::kLanes, X::lane()        the lanes that share one stream; wave-uniform state (positions, counts, bit offsets) is
//                               the same in every lane, lane-strided loops over 64 positions split the bulk work
//   X::sync()                   everything the lanes stored before it is visible to all of them after it
//   X::excl_scan64(a)           a[0..64) (shared) becomes its exclusive prefix sum, the total is returned to every lane;
//                               one lane: a serial loop.  Synchronises before and after
//   X::which64(a)               bit i of the result = a[i] != 0, for a shared uint16_t a[64] that is visible already;
//                               one lane: a loop
//   X::atomic_add(p, v), X::atomic_or(p, v) on a shared uint32_t, X::atomic_max16(p, v) on a shared uint16_t;
//                               one lane: the plain operation
// THE CONTRACT: the bytes of a stream are a function of the input bytes, level, strategy and block-type mask only.
// Every step is defined on a chunk of 64 positions whatever kLanes is: all table lookups of a chunk see the table as it
// was before the chunk, the inserts of a chunk resolve by "the highest position wins" (atomic_max16), sums are integer.
// Nothing is written outside [dst, dst + cap), nothing is read outside [src, src + src_len).
//
// A stream is cut into blocks of kBlockLen input bytes; positions are block-relative and matches never reach before the
// block, so a table entry is 16 bits (position + 1, 0 = empty).
//
// LEVELS 3-8 (tokenize_chains) search hash chains instead of the one-entry table, under the same contract.  The table
// holds the head of each chain (the latest position of a 3-byte hash), a ring of kRingLen 16-bit links behind the tokens
// in the lanes' own area holds prev[p & (kRingLen - 1)] = the previous position of p's hash (+ 1, 0 = none).  Unlike
// level 1, a lookup at p sees EVERY lower position of the block, its own chunk's included: the links come out as if the
// positions had been inserted one by one in ascending order.  Per chunk: the 64 hashes go to shared memory, every
// position takes as its link the nearest lower position of its chunk with the same hash, or else the head as before
// the chunk, and writes it to the ring; then the heads move ("the highest position wins") while every position walks
// its own chain: at most depth(level) candidates, nearest first, the longest match kept (on a tie the nearest), the
// walk over at nice(level) bytes, at the end of the input or at 258.  A walk checks, BEFORE it reads a candidate's link,
// that the candidate lies below the one before it and within kMaxDist: a ring slot that a position kRingLen higher has
// taken over may hold anything (of this block; a slot is never read before this block wrote it), and such a link ends
// the walk or leads to a lower position that is compared like any other -- so the loop runs at most depth times.  A
// 3-byte match farther than kFar3 is dropped.  Lazy selection (a match at p yields to a longer one at p + 1, p becomes
// a literal) looks at the chunk's candidates only: the last position of a chunk does not look ahead.
//     level   3    4    5    6    7    8
//     depth   4    8   16   32   64  128
//     nice   32   32   64  128  258  258
//     lazy   no  yes  yes  yes  yes  yes
// Huffman-only takes no search at any level, so its bytes are those of level 1.
#pragma once
#include <stdint.h>

#include "inflate_core.h"   // gklinf::Scratch + crc32_stream: the CRC-32 of the input

#ifndef GKL_DEF_FN
#define GKL_DEF_FN inline   // the kernel's translation unit defines it as __device__ __forceinline__
#endif

namespace gkldef {

enum Status : int32_t { ST_OK = 0, ST_OUT_OVERFLOW = 1 };
enum Strategy : int32_t { STRATEGY_DEFAULT = 0, STRATEGY_HUFFMAN_ONLY = 1 };
enum BlockType : int32_t { BT_STORED = 1, BT_FIXED = 2, BT_DYNAMIC = 4, BT_ALL = 7 };

constexpr uint32_t kBlockLen = 65535;        // input bytes per deflate block: a stored block is always possible
constexpr uint32_t kTokenWords = 65536;      // one token per input byte at the most, plus the end-of-block token
constexpr uint32_t kRingLen = 32768;         // levels 3-8: the 16-bit chain links of the last kMaxDist positions, 64 KB
constexpr uint32_t kTokensPerWave = kTokenWords + kRingLen / 2;   // words of a wavefront's own area: tokens, then the ring (320 KB)
constexpr int kHashBits = 13;                // 8192 slots, one entry each: 16 KB
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr uint32_t kFar3 = 4096;             // levels 3-8: a 3-byte match farther back than this is dropped (zlib's TOO_FAR)
constexpr uint32_t kTokMatch = 0x80000000u;  // token: a literal byte, 256 = end of block, or kTokMatch | (len - 3) << 16 | (dist - 1)

// the node arrays of one code construction (2 * 286 - 1 nodes at the most)
struct HuffWork {
  uint32_t weight[576];
  uint16_t parent[576];
  uint16_t sym[288];       // used symbols in order of (count, symbol)
  uint8_t depth[576];
};

struct Scratch {
  union {
    uint16_t table[1 << kHashBits];   // match search
    uint32_t table_words[(1 << kHashBits) / 2];   // the same, to clear it
    HuffWork hw;                      // code construction (the search of the block is over)
    gklinf::Scratch inf;              // CRC-32 of the input (before the first block)
    struct {                          // emission (the codes are built): the bits of 64 items,
      uint64_t ebits[64];
      uint32_t enb[64];               //   their lengths, then their bit offsets
    } emit;
  } u;
  uint32_t lhist[288], dhist[32], chist[20];
  uint16_t lcode[288], dcode[32], ccode[20];
  uint8_t llen[288], dlen[32], clen[20];
  uint16_t bl_count[16], next_code[16];
  uint16_t mlen[64], mdist[64];      // the chunk's candidates (levels 3-8: before them the chunk's links and hashes)
  uint32_t staging[104];             // 7 carried bits + 64 x 48 bits
  uint16_t hdr[320];                 // the dynamic header's code-length symbols: symbol | extra << 8
  uint32_t n_hdr, n_used, hlit, hdist;
};

GKL_DEF_FN uint32_t bit_reverse(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1u); v >>= 1; }
  return r;
}
GKL_DEF_FN uint32_t load4(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
GKL_DEF_FN uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }
GKL_DEF_FN uint32_t hash3(uint32_t v) { return ((v & 0xFFFFFFu) * 2654435761u) >> (32 - kHashBits); }
GKL_DEF_FN uint32_t floor_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

// levels 3-8: the candidates a walk may try, the length that ends it, lazy selection or greedy
struct LevelParams { uint16_t depth, nice, lazy; };
GKL_DEF_FN LevelParams level_params(int32_t level) {
  constexpr LevelParams table[6] = {{4, 32, 0}, {8, 32, 1}, {16, 64, 1}, {32, 128, 1}, {64, 258, 1}, {128, 258, 1}};
  return table[level < 3 ? 0 : level > 8 ? 5 : level - 3];
}

// the bytes in[c...] and in[p...] share, maxl at the most; c < p, p + maxl <= the end of the input.  (Level 1 keeps
// the loop it was built with: through this function its kernel takes 118 VGPRs instead of 114.)
GKL_DEF_FN uint32_t match_length(const uint8_t* in, uint32_t c, uint32_t p, uint32_t maxl) {
  uint32_t l = 0;
  while (l + 4 <= maxl) {   // four bytes a step
    const uint32_t x = load4(in + c + l) ^ load4(in + p + l);
    if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
    l += 4;
  }
  while (l < maxl && in[c + l] == in[p + l]) l++;
  return l;
}

// length 3..258 -> symbol 257..285, extra bits
GKL_DEF_FN void length_symbol(uint32_t len, uint32_t* sym, uint32_t* nextra, uint32_t* extra) {
  const uint32_t l = len - 3;
  if (l < 8) { *sym = 257 + l; *nextra = 0; *extra = 0; return; }
  if (len == 258) { *sym = 285; *nextra = 0; *extra = 0; return; }
  const uint32_t nb = floor_log2(l) - 2;
  *sym = 261 + 4 * nb + ((l >> nb) & 3u);
  *nextra = nb;
  *extra = l & ((1u << nb) - 1u);
}
// distance 1..32768 -> symbol 0..29, extra bits
GKL_DEF_FN void dist_symbol(uint32_t dist, uint32_t* sym, uint32_t* nextra, uint32_t* extra) {
  const uint32_t d = dist - 1;
  if (d < 4) { *sym = d; *nextra = 0; *extra = 0; return; }
  const uint32_t nb = floor_log2(d) - 1;
  *sym = 2 + 2 * nb + ((d >> nb) & 1u);
  *nextra = nb;
  *extra = d & ((1u << nb) - 1u);
}
GKL_DEF_FN uint32_t length_extra_bits(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
GKL_DEF_FN uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

// Length-limited code lengths for freq[0, n): plain Huffman (the two-queue construction over the symbols sorted by
// (count, symbol)), depths clamped to `limit`, then a repair of the Kraft sum on the counts per length, then the lengths
// handed out along the sorted order, longest first -- so a more frequent symbol never gets a longer code, and a tree that
// fits the limit keeps its cost.  One used symbol gets length 1; none, nothing.  Returns the number of used symbols.
template <class X>
GKL_DEF_FN uint32_t build_lengths(Scratch& S, const uint32_t* freq, uint32_t n, uint32_t limit, uint8_t* lens) {
  HuffWork& W = S.u.hw;
  const uint32_t lane = (uint32_t)X::lane();
  // rank sort: every lane places its own symbols
  for (uint32_t s = lane; s < n; s += X::kLanes) {
    lens[s] = 0;
    const uint32_t f = freq[s];
    if (f == 0) continue;
    uint32_t rank = 0;
    for (uint32_t t = 0; t < n; t++) {
      const uint32_t g = freq[t];
      rank += g != 0 && (g < f || (g == f && t < s));
    }
    W.sym[rank] = (uint16_t)s;
    W.weight[rank] = f;
  }
  if (lane == 0) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; s++) m += freq[s] != 0;
    S.n_used = m;
  }
  X::sync();
  const uint32_t m = S.n_used;
  if (m == 0) { X::sync(); return 0; }   // n_used is free again
  if (lane == 0) {
    if (m == 1) {
      lens[W.sym[0]] = 1;
    } else {
      // leaves 0..m-1 in ascending weight, internal nodes m..2m-2 in the order they are made (ascending too)
      uint32_t leaf = 0, node = m, made = m;
      for (; made < 2 * m - 1; made++) {
        uint32_t w = 0;
        for (int k = 0; k < 2; k++) {
          uint32_t pick;
          if (leaf < m && (node >= made || W.weight[leaf] <= W.weight[node])) pick = leaf++;
          else pick = node++;
          w += W.weight[pick];
          W.parent[pick] = (uint16_t)made;
        }
        W.weight[made] = w;
      }
      W.depth[2 * m - 2] = 0;
      for (uint32_t i = 2 * m - 2; i-- > 0;) {
        const uint32_t d = (uint32_t)W.depth[W.parent[i]] + 1u;
        W.depth[i] = (uint8_t)(d > 200 ? 200 : d);
      }
      for (uint32_t l = 0; l <= 15; l++) S.bl_count[l] = 0;
      for (uint32_t i = 0; i < m; i++) {
        const uint32_t d = W.depth[i];
        S.bl_count[d > limit ? limit : d]++;
      }
      // Kraft sum in units of 2^-limit
      uint32_t kraft = 0;
      for (uint32_t l = 1; l <= limit; l++) kraft += (uint32_t)S.bl_count[l] << (limit - l);
      const uint32_t one = 1u << limit;
      while (kraft > one) {   // lengthen one code of the longest length below the limit
        uint32_t l = limit - 1;
        while (S.bl_count[l] == 0) l--;
        S.bl_count[l]--; S.bl_count[l + 1]++;
        kraft -= 1u << (limit - l - 1);
      }
      while (kraft < one) {   // shorten the longest code whose gain still fits
        uint32_t l = limit;
        while (S.bl_count[l] == 0 || (1u << (limit - l)) > one - kraft) l--;
        S.bl_count[l]--; S.bl_count[l - 1]++;
        kraft += 1u << (limit - l);
      }
      uint32_t i = 0;
      for (uint32_t l = limit; l >= 1; l--)
        for (uint32_t c = S.bl_count[l]; c > 0; c--) lens[W.sym[i++]] = (uint8_t)l;
    }
  }
  X::sync();
  return m;
}

// canonical codes of lens[0, n), stored bit-reversed (deflate sends Huffman codes most significant bit first)
template <class X>
GKL_DEF_FN void assign_codes(Scratch& S, const uint8_t* lens, uint32_t n, uint16_t* code) {
  if (X::lane() == 0) {
    for (int l = 0; l < 16; l++) S.bl_count[l] = 0;
    for (uint32_t s = 0; s < n; s++) S.bl_count[lens[s]]++;
    uint32_t c = 0;
    S.bl_count[0] = 0;
    for (int l = 1; l < 16; l++) { c = (c + S.bl_count[l - 1]) << 1; S.next_code[l] = (uint16_t)c; }
    for (uint32_t s = 0; s < n; s++) {
      const int l = lens[s];
      code[s] = l ? (uint16_t)bit_reverse(S.next_code[l]++, l) : (uint16_t)0;
    }
  }
  X::sync();
}

// kSearches: which match searches an instantiation carries, so that a kernel for level 1 holds no code of levels 3-8
enum Searches : int { SEARCH_TABLE = 1, SEARCH_CHAINS = 2, SEARCH_BOTH = 3 };

template <class X, int kSearches = SEARCH_BOTH>
struct Deflater {
  Scratch& S;
  uint8_t* dst;
  uint32_t cap;
  uint32_t* toks;
  int32_t strategy, types;
  // output: bytes [0, outpos) are stored, `carry` bits (< 8) behind them wait in the low bits of staging[0]
  uint32_t outpos = 0, carry = 0;

  GKL_DEF_FN Deflater(Scratch& s, uint8_t* dst_, uint32_t cap_, uint32_t* toks_, int32_t strategy_, int32_t types_)
      : S(s), dst(dst_), cap(cap_), toks(toks_), strategy(strategy_), types(types_) {}

  // Sends m <= 64 items; item(i, &bits, &nb) gives the bits (at most 48, least significant first) of item i.  The
  // caller has checked that the bytes fit.
  template <class F>
  GKL_DEF_FN void put64(uint32_t m, F item) {
    const uint32_t lane = (uint32_t)X::lane();
    for (uint32_t i = lane; i < 64; i += X::kLanes) {
      uint64_t bits = 0;
      uint32_t nb = 0;
      if (i < m) item(i, &bits, &nb);
      S.u.emit.ebits[i] = bits;
      S.u.emit.enb[i] = nb;
    }
    const uint32_t total = X::excl_scan64(S.u.emit.enb) + carry;
    for (uint32_t i = lane; i < m; i += X::kLanes) {
      const uint64_t bits = S.u.emit.ebits[i];
      if (bits == 0) continue;
      const uint32_t off = carry + S.u.emit.enb[i], w = off >> 5, sh = off & 31u;
      const uint32_t lo = (uint32_t)bits;
      const uint64_t hi = (bits >> 32) << sh;
      X::atomic_or(&S.staging[w], lo << sh);
      const uint32_t mid = (sh ? lo >> (32 - sh) : 0u) | (uint32_t)hi;
      if (mid) X::atomic_or(&S.staging[w + 1], mid);
      if (hi >> 32) X::atomic_or(&S.staging[w + 2], (uint32_t)(hi >> 32));
    }
    X::sync();
    const uint32_t nbytes = total >> 3;
    for (uint32_t i = lane; i < nbytes; i += X::kLanes) dst[outpos + i] = (uint8_t)(S.staging[i >> 2] >> (8 * (i & 3u)));
    carry = total & 7u;
    const uint32_t left = (S.staging[nbytes >> 2] >> (8 * (nbytes & 3u))) & ((1u << carry) - 1u);
    outpos += nbytes;
    X::sync();
    for (uint32_t w = lane; w < 104; w += X::kLanes) S.staging[w] = w == 0 ? left : 0u;
    // the next put64 synchronises (excl_scan64) before it touches the staging words
  }

  // Match search and greedy selection of one block: tokens to toks[], counts to lhist / dhist.  Returns the token count.
  GKL_DEF_FN uint32_t tokenize(const uint8_t* in, uint32_t n, bool search) {
    const uint32_t lane = (uint32_t)X::lane();
    if (search)
      for (uint32_t i = lane; i < (1u << kHashBits) / 2; i += X::kLanes) S.u.table_words[i] = 0;
    for (uint32_t i = lane; i < 288; i += X::kLanes) S.lhist[i] = 0;
    for (uint32_t i = lane; i < 32; i += X::kLanes) S.dhist[i] = 0;
    X::sync();
    uint32_t ntok = 0, next = 0;   // next: the first position that no match covers yet
    for (uint32_t b = 0; b < n; b += 64) {
      // candidates: every lookup sees the table as it was before this chunk
      for (uint32_t i = lane; i < 64; i += X::kLanes) {
        const uint32_t p = b + i;
        uint32_t ml = 0, md = 0;
        if (search && p >= next && p + 4 <= n) {
          const uint32_t c1 = S.u.table[hash4(load4(in + p))];
          if (c1 != 0 && p - (c1 - 1) <= kMaxDist) {
            const uint32_t c = c1 - 1, maxl = n - p < kMaxMatch ? n - p : kMaxMatch;
            uint32_t l = 0;
            bool differ = false;
            while (l + 4 <= maxl) {   // four bytes a step: p + l + 3 < n
              const uint32_t x = load4(in + c + l) ^ load4(in + p + l);
              if (x) { l += (uint32_t)__builtin_ctz(x) >> 3; differ = true; break; }
              l += 4;
            }
            if (!differ)
              while (l < maxl && in[c + l] == in[p + l]) l++;
            if (l >= kMinMatch) { ml = l; md = p - c; }
          }
        }
        S.mlen[i] = (uint16_t)ml;
        S.mdist[i] = (uint16_t)(md - (md != 0));   // dist - 1: 32768 does not fit 16 bits
      }
      X::sync();
      // inserts: the highest position wins
      if (search)
        for (uint32_t i = lane; i < 64; i += X::kLanes) {
          const uint32_t p = b + i;
          if (p + 4 <= n) X::atomic_max16(&S.u.table[hash4(load4(in + p))], (uint16_t)(p + 1));
        }
      select64(in, b, n, false, &next, &ntok);
      X::sync();   // mlen / mdist are free again, the inserts are in the table
    }
    if (lane == 0) { toks[ntok] = 256; S.lhist[256] += 1; }
    X::sync();
    return ntok + 1;
  }

  // Selection over the candidates of the chunk at b (mlen / mdist, visible already) in position order, the same in
  // every lane, then the chunk's tokens and their counts.  Greedy: the first candidate that no match covers is taken.
  // Lazy: such a candidate yields to a longer one at the next position of the same chunk and becomes a literal.
  GKL_DEF_FN void select64(const uint8_t* in, uint32_t b, uint32_t n, bool lazy, uint32_t* next_io, uint32_t* ntok_io) {
    const uint32_t lane = (uint32_t)X::lane();
    uint32_t next = *next_io;
    const uint32_t ntok = *ntok_io;
    const uint32_t cnt = n - b < 64 ? n - b : 64;
    const uint64_t valid = cnt == 64 ? ~0ull : (1ull << cnt) - 1ull;
    const uint64_t cand = X::which64(S.mlen) & valid;
    const uint32_t first = next > b ? next - b : 0;   // < 64 or the whole chunk is covered
    uint64_t covered = first >= 64 ? ~0ull : (1ull << first) - 1ull;
    uint64_t starts = 0;
    uint64_t open = cand & ~covered;
    while (open) {
      const uint32_t i = (uint32_t)__builtin_ctzll(open);
      if (lazy && ((open >> i) & 2ull) && S.mlen[i + 1] > S.mlen[i]) {   // bit i + 1 of open: i < 63
        open &= ~(1ull << i);
        continue;
      }
      const uint32_t e = i + S.mlen[i];
      starts |= 1ull << i;
      const uint64_t upto = e >= 64 ? ~0ull : (1ull << e) - 1ull;
      covered |= upto & ~((2ull << i) - 1ull);
      next = b + e;
      open &= ~upto;
    }
    const uint64_t tokmask = valid & ~covered;   // literals and match starts
    for (uint32_t i = lane; i < cnt; i += X::kLanes) {
      if (!((tokmask >> i) & 1ull)) continue;
      const uint32_t idx = ntok + (uint32_t)__builtin_popcountll(tokmask & ((1ull << i) - 1ull));
      if ((starts >> i) & 1ull) {
        const uint32_t len = S.mlen[i], d1 = S.mdist[i];
        uint32_t ls, ds, nx, ex;
        length_symbol(len, &ls, &nx, &ex);
        dist_symbol(d1 + 1, &ds, &nx, &ex);
        toks[idx] = kTokMatch | ((len - 3) << 16) | d1;
        X::atomic_add(&S.lhist[ls], 1u);
        X::atomic_add(&S.dhist[ds], 1u);
      } else {
        const uint32_t byte = in[b + i];
        toks[idx] = byte;
        X::atomic_add(&S.lhist[byte], 1u);
      }
    }
    *next_io = next;
    *ntok_io = ntok + (uint32_t)__builtin_popcountll(tokmask);
  }

  // Levels 3-8: hash chains, bounded walks, lazy or greedy selection (see the head of the file).  Tokens to toks[],
  // counts to lhist / dhist, links to the ring behind the tokens.  Returns the token count.
  GKL_DEF_FN uint32_t tokenize_chains(const uint8_t* in, uint32_t n, const LevelParams lp) {
    const uint32_t lane = (uint32_t)X::lane();
    uint16_t* ring = reinterpret_cast<uint16_t*>(toks + kTokenWords);   // these words hold links only, never tokens
    for (uint32_t i = lane; i < (1u << kHashBits) / 2; i += X::kLanes) S.u.table_words[i] = 0;
    for (uint32_t i = lane; i < 288; i += X::kLanes) S.lhist[i] = 0;
    for (uint32_t i = lane; i < 32; i += X::kLanes) S.dhist[i] = 0;
    X::sync();
    constexpr uint32_t kNoHash = 0xFFFFu;   // a position with fewer than 3 bytes left: no hash, no link, no lookup
    uint32_t ntok = 0, next = 0;
    for (uint32_t b = 0; b < n; b += 64) {
      // the chunk's hashes (mdist holds them until the candidates take it back)
      for (uint32_t i = lane; i < 64; i += X::kLanes) {
        const uint32_t p = b + i;
        uint32_t h = kNoHash;
        if (p + 4 <= n) h = hash3(load4(in + p));
        else if (p + 3 == n) h = hash3((uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16));
        S.mdist[i] = (uint16_t)h;
      }
      X::sync();
      // links: the nearest lower position of the chunk with the same hash, else the head as before the chunk; mlen
      // keeps a position's own link for its walk
      for (uint32_t i = lane; i < 64; i += X::kLanes) {
        const uint32_t p = b + i, h = S.mdist[i];
        uint32_t c1 = 0;
        if (h != kNoHash) {
          uint32_t j = i;
          while (j > 0 && S.mdist[j - 1] != h) j--;
          c1 = j > 0 ? b + j : S.u.table[h];   // position b + j - 1, plus one
          ring[p & (kRingLen - 1)] = (uint16_t)c1;
        }
        S.mlen[i] = (uint16_t)c1;
      }
      X::sync();
      // heads: the highest position wins.  Walks: they read the ring, never the heads; mlen[i] and mdist[i] are read
      // and written by position i's own lane from here to the next sync
      for (uint32_t i = lane; i < 64; i += X::kLanes) {
        const uint32_t p = b + i, h = S.mdist[i];
        if (h != kNoHash) X::atomic_max16(&S.u.table[h], (uint16_t)(p + 1));
        uint32_t c1 = S.mlen[i];
        uint32_t best = 0, bdist = 0;
        if (p >= next && p + 3 <= n) {
          const uint32_t maxl = n - p < kMaxMatch ? n - p : kMaxMatch;
          const uint32_t enough = maxl < lp.nice ? maxl : lp.nice;
          uint32_t above = p;   // the candidate before this one: positions along a chain strictly decrease
          for (uint32_t k = 0; k < lp.depth; k++) {
            if (c1 == 0) break;
            const uint32_t c = c1 - 1;
            if (c >= above || p - c > kMaxDist) break;   // checked before c's link is read
            if (best == 0 || in[c + best] == in[p + best]) {   // best < maxl: only a longer match replaces the best
              const uint32_t l = match_length(in, c, p, maxl);
              if (l > best) { best = l; bdist = p - c; }
              if (l >= enough) break;
            }
            above = c;
            c1 = ring[c & (kRingLen - 1)];
          }
          if (best < 3 || (best == 3 && bdist > kFar3)) { best = 0; bdist = 0; }
        }
        S.mlen[i] = (uint16_t)best;
        S.mdist[i] = (uint16_t)(bdist - (bdist != 0));
      }
      X::sync();
      select64(in, b, n, lp.lazy != 0, &next, &ntok);
      X::sync();   // mlen / mdist are free again, the heads are in the table
    }
    if (lane == 0) { toks[ntok] = 256; S.lhist[256] += 1; }
    X::sync();
    return ntok + 1;
  }

  // Dynamic codes from the histograms: lengths, the header's run-length symbols and its code.  Returns the header's
  // bits behind the three block bits.
  GKL_DEF_FN uint32_t dynamic_codes(uint32_t* hlit_out, uint32_t* hdist_out, uint32_t* hclen_out) {
    build_lengths<X>(S, S.lhist, 286, 15, S.llen);
    const uint32_t nd = build_lengths<X>(S, S.dhist, 30, 15, S.dlen);
    if (X::lane() == 0) {
      if (nd == 0) S.dlen[0] = 1;   // no match in the block: one distance code of length 1, which zlib accepts
      uint32_t hlit = 286, hdist = 30;
      while (hlit > 257 && S.llen[hlit - 1] == 0) hlit--;
      while (hdist > 1 && S.dlen[hdist - 1] == 0) hdist--;
      for (int s = 0; s < 19; s++) S.chist[s] = 0;
      // the lengths of both alphabets as one sequence, run-length coded (RFC 1951 3.2.7)
      const uint32_t total = hlit + hdist;
      uint32_t k = 0, i = 0;
      while (i < total) {
        const uint32_t v = i < hlit ? S.llen[i] : S.dlen[i - hlit];
        uint32_t run = 1;
        while (i + run < total && (i + run < hlit ? S.llen[i + run] : S.dlen[i + run - hlit]) == v) run++;
        uint32_t left = run;
        if (v == 0) {
          while (left >= 11) { const uint32_t r = left < 138 ? left : 138; S.hdr[k++] = (uint16_t)(18 | ((r - 11) << 8)); S.chist[18]++; left -= r; }
          if (left >= 3) { S.hdr[k++] = (uint16_t)(17 | ((left - 3) << 8)); S.chist[17]++; left = 0; }
        } else {
          S.hdr[k++] = (uint16_t)v; S.chist[v]++; left--;
          while (left >= 3) { const uint32_t r = left < 6 ? left : 6; S.hdr[k++] = (uint16_t)(16 | ((r - 3) << 8)); S.chist[16]++; left -= r; }
        }
        for (; left > 0; left--) { S.hdr[k++] = (uint16_t)v; S.chist[v]++; }
        i += run;
      }
      S.n_hdr = k;
      // zlib refuses an incomplete code-length code: a lone symbol gets a partner
      uint32_t used = 0;
      for (int s = 0; s < 19; s++) used += S.chist[s] != 0;
      if (used == 1) S.chist[S.chist[0] ? 1 : 0] = 1;
      S.hlit = hlit; S.hdist = hdist;
    }
    X::sync();
    build_lengths<X>(S, S.chist, 19, 7, S.clen);
    assign_codes<X>(S, S.clen, 19, S.ccode);
    assign_codes<X>(S, S.llen, 286, S.lcode);
    assign_codes<X>(S, S.dlen, 30, S.dcode);
    uint32_t hclen = 19;
    while (hclen > 4 && S.clen[order(hclen - 1)] == 0) hclen--;
    uint32_t bits = 14 + 3 * hclen;
    const uint32_t nh = S.n_hdr;
    for (uint32_t i = 0; i < nh; i++) {   // over what is sent: a lone symbol's partner is in chist only
      const uint32_t s = S.hdr[i] & 0xFFu;
      bits += S.clen[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
    }
    *hlit_out = S.hlit; *hdist_out = S.hdist; *hclen_out = hclen;
    return bits;
  }

  // the order in which the code-length code's lengths are sent
  static GKL_DEF_FN uint32_t order(uint32_t i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 8 - ((i - 3) >> 1) : 7 + ((i - 2) >> 1); }

  GKL_DEF_FN void fixed_codes() {
    for (uint32_t s = (uint32_t)X::lane(); s < 288; s += X::kLanes) {
      const uint32_t l = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
      const uint32_t c = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xC0 + (s - 280);
      S.llen[s] = (uint8_t)l;
      S.lcode[s] = (uint16_t)bit_reverse(c, (int)l);
    }
    for (uint32_t s = (uint32_t)X::lane(); s < 32; s += X::kLanes) { S.dlen[s] = 5; S.dcode[s] = (uint16_t)bit_reverse(s, 5); }
    X::sync();
  }

  GKL_DEF_FN void put_tokens(uint32_t ntok) {
    for (uint32_t t0 = 0; t0 < ntok; t0 += 64) {
      const uint32_t m = ntok - t0 < 64 ? ntok - t0 : 64;
      put64(m, [&](uint32_t i, uint64_t* bits, uint32_t* nb) {
        const uint32_t t = toks[t0 + i];
        if (!(t & kTokMatch)) { *bits = S.lcode[t]; *nb = S.llen[t]; return; }
        uint32_t ls, lx, le, ds, dx, de;
        length_symbol(((t >> 16) & 0xFFu) + 3, &ls, &lx, &le);
        dist_symbol((t & 0xFFFFu) + 1, &ds, &dx, &de);
        uint64_t v = S.lcode[ls];
        uint32_t k = S.llen[ls];
        v |= (uint64_t)le << k; k += lx;
        v |= (uint64_t)S.dcode[ds] << k; k += S.dlen[ds];
        v |= (uint64_t)de << k; k += dx;
        *bits = v; *nb = k;
      });
    }
  }

  // One block.  Returns false when the stream no longer fits its capacity.
  GKL_DEF_FN bool block(const uint8_t* in, uint32_t n, bool final, int32_t level) {
    const bool stored_only = level == 0;
    const uint64_t at = (uint64_t)outpos * 8 + carry;
    const uint32_t pad = (uint32_t)((8 - ((at + 3) & 7u)) & 7u);
    const uint64_t stored_bits = 3 + pad + 32 + 8ull * n;
    uint32_t allow = stored_only ? (uint32_t)BT_STORED : (uint32_t)types;
    uint64_t dyn_bits = 0, fixed_bits = 0;
    uint32_t ntok = 0, hlit = 0, hdist = 0, hclen = 0;
    if (allow != BT_STORED) {
      const bool search = strategy == STRATEGY_DEFAULT;
      if ((kSearches & SEARCH_CHAINS) && search && level >= 3) ntok = tokenize_chains(in, n, level_params(level));
      else ntok = tokenize(in, n, search && (kSearches & SEARCH_TABLE));
      const uint32_t hdr_bits = dynamic_codes(&hlit, &hdist, &hclen);
      dyn_bits = 3 + hdr_bits;
      fixed_bits = 3;
      for (uint32_t s = 0; s < 286; s++) {
        const uint64_t f = S.lhist[s];
        const uint32_t x = s < 257 ? 0 : length_extra_bits(s);
        dyn_bits += f * (S.llen[s] + x);
        fixed_bits += f * ((s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u) + x);
      }
      for (uint32_t s = 0; s < 30; s++) {
        const uint64_t f = S.dhist[s];
        dyn_bits += f * (S.dlen[s] + dist_extra_bits(s));
        fixed_bits += f * (5 + dist_extra_bits(s));
      }
    }
    // the smallest of the allowed types; on a tie stored before fixed before dynamic
    uint32_t type = 0;
    uint64_t best = ~0ull;
    if ((allow & BT_DYNAMIC) && dyn_bits <= best) { type = BT_DYNAMIC; best = dyn_bits; }
    if ((allow & BT_FIXED) && fixed_bits <= best) { type = BT_FIXED; best = fixed_bits; }
    if ((allow & BT_STORED) && stored_bits <= best) { type = BT_STORED; best = stored_bits; }
    if ((at + best + 7) / 8 > cap) return false;
    const uint32_t bfinal = final ? 1u : 0u;
    if (type == BT_STORED) {
      put64(3, [&](uint32_t i, uint64_t* bits, uint32_t* nb) {
        if (i == 0) { *bits = bfinal; *nb = 3; }
        else if (i == 1) { *bits = 0; *nb = pad; }
        else { *bits = (uint64_t)n | ((uint64_t)(n ^ 0xFFFFu) << 16); *nb = 32; }
      });
      for (uint32_t i = (uint32_t)X::lane(); i < n; i += X::kLanes) dst[outpos + i] = in[i];
      outpos += n;
      return true;
    }
    if (type == BT_FIXED) {
      fixed_codes();
      put64(1, [&](uint32_t, uint64_t* bits, uint32_t* nb) { *bits = bfinal | 2u; *nb = 3; });
    } else {
      put64(1 + hclen, [&](uint32_t i, uint64_t* bits, uint32_t* nb) {
        if (i == 0) { *bits = bfinal | 4u | ((hlit - 257) << 3) | ((hdist - 1) << 8) | ((uint64_t)(hclen - 4) << 13); *nb = 17; }
        else { *bits = S.clen[order(i - 1)]; *nb = 3; }
      });
      const uint32_t nh = S.n_hdr;
      for (uint32_t h0 = 0; h0 < nh; h0 += 64) {
        const uint32_t m = nh - h0 < 64 ? nh - h0 : 64;
        put64(m, [&](uint32_t i, uint64_t* bits, uint32_t* nb) {
          const uint32_t e = S.hdr[h0 + i], s = e & 0xFFu, l = S.clen[s];
          *bits = S.ccode[s] | ((uint64_t)(e >> 8) << l);
          *nb = l + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u);
        });
      }
    }
    put_tokens(ntok);
    return true;
  }

  GKL_DEF_FN int run(const uint8_t* src, uint32_t len, int32_t level, int32_t* out_len) {
    for (uint32_t w = (uint32_t)X::lane(); w < 104; w += X::kLanes) S.staging[w] = 0;
    X::sync();
    *out_len = 0;
    uint32_t at = 0;
    do {
      const uint32_t n = len - at < kBlockLen ? len - at : kBlockLen;
      if (!block(src + at, n, at + n == len, level)) return ST_OUT_OVERFLOW;
      at += n;
    } while (at < len);
    if (carry) {   // the capacity check of the last block counted this byte
      X::sync();
      if (X::lane() == 0) dst[outpos] = (uint8_t)S.staging[0];
      outpos++;
    }
    X::sync();
    *out_len = (int32_t)outpos;
    return ST_OK;
  }
};

// the stored size: a stream given this capacity never overflows when stored blocks are allowed
constexpr int64_t deflate_bound(int64_t len) {
  const int64_t blocks = len <= 0 ? 1 : (len + kBlockLen - 1) / kBlockLen;
  return (len < 0 ? 0 : len) + 5 * blocks;
}

// One stream, 0 <= src_len, cap <= 2^31 - 1; level 0 (stored blocks only), 1 or 3..8 (the callers refuse the others);
// types: a mask of BlockType, 0 = all.  toks: kTokensPerWave words that only these lanes use; nothing is read from them
// that this call has not written.  Every lane returns the same status and length.  kSearches: an instantiation without
// SEARCH_CHAINS serves levels 0 and 1 only, one without SEARCH_TABLE levels 3..8 only.
template <class X, int kSearches = SEARCH_BOTH>
GKL_DEF_FN int deflate_stream(Scratch& S, const uint8_t* src, int32_t src_len, uint8_t* dst, int32_t cap, uint32_t* toks,
                              int32_t level, int32_t strategy, int32_t types, int32_t* out_len) {
  Deflater<X, kSearches> d(S, dst, (uint32_t)cap, toks, strategy, (types & BT_ALL) ? (types & BT_ALL) : BT_ALL);
  return d.run(src, (uint32_t)src_len, level, out_len);
}

}  // namespace gkldef
