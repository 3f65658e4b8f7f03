// lsmblk_keys.hpp -- the key order, once, with the vector types and buffer descriptors it reads through.
// Keys compare as byte strings (src/key.rs:77-81 via Vec<u8> Ord): a shorter key sorts before its
// extensions.  A key's leading 16 bytes, zero padded and read big-endian, are its "image": two
// images decide the order of their keys unless they tie; a tie with a key of at most 16 bytes is
// decided by the lengths (the pad is not a key byte: "a" < "a\0"), any other tie by the tails.
//
// Everything but the accessors is __host__ __device__ over a small accessor, so that
// tests/key_order_host.hip checks it exhaustively on a CPU.  An accessor ("KS") reads an arena by
// position and returns 0 past the arena's end:
//   dw(pos)          bytes [pos, pos + 4) as a little-endian dword
//   byte(pos)        one byte
//   fetch16(pos, v)  bytes [pos, pos + 16) as four little-endian dwords
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ rsrc_t make_rsrc(const void* p16, uint32_t nbytes) {
  const uint32_t n = nbytes >= 0xFFFFFFF0u ? 0xFFFFFFFFu : (nbytes + 15) & ~15u;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p16), (short)0, (int)n, 0x00020000);
}
// Store descriptor with an exact byte bound: an access reaching past nbytes is dropped.
__device__ __forceinline__ rsrc_t make_rsrc_exact(void* p16, uint32_t nbytes) {
  return __builtin_amdgcn_make_buffer_rsrc(p16, (short)0, (int)nbytes, 0x00020000);
}

// ---------------------------------------------------------------- accessors
// Global keys through a bounds-checked descriptor over the key arena (reads past it give 0):
// aligned dword loads, none straddles the bound, and alignbytes.
struct ArenaKeys {
  rsrc_t r;       // the key arena, base aligned down
  uint32_t lead;  // the bytes between that base and the keys pointer (0 in key_upto's view)
  ArenaKeys() = default;
  __device__ __forceinline__ ArenaKeys(const uint8_t* keys, uint32_t total) {
    lead = uint32_t(reinterpret_cast<uintptr_t>(keys) & 15);
    r = make_rsrc(keys - lead, lead + total);
  }
  __device__ __forceinline__ uint32_t dw(uint32_t pos) const {
    const uint32_t x = lead + pos, al = x & ~3u;
    const uint32_t w0 = __builtin_amdgcn_raw_buffer_load_b32(r, al, 0, 0);
    const uint32_t w1 = __builtin_amdgcn_raw_buffer_load_b32(r, al + 4, 0, 0);
    return __builtin_amdgcn_alignbyte(w1, w0, x & 3);
  }
  __device__ __forceinline__ uint32_t byte(uint32_t pos) const {
    return __builtin_amdgcn_raw_buffer_load_b8(r, lead + pos, 0, 0);
  }
  __device__ __forceinline__ void fetch16(uint32_t pos, uint32_t (&v)[4]) const {  // five loads, not eight
    const uint32_t x = lead + pos, al = x & ~3u;
    uint32_t w[5];
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) w[j] = __builtin_amdgcn_raw_buffer_load_b32(r, al + 4 * j, 0, 0);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) v[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], x & 3);
  }
};
// LDS key image (unaligned ds_read_b32: the gfx9 unaligned access mode)
struct LKeys {
  const uint8_t* base;
  __device__ __forceinline__ uint32_t dw(uint32_t pos) const { return *reinterpret_cast<const uint32_t*>(base + pos); }
  __device__ __forceinline__ uint32_t byte(uint32_t pos) const { return base[pos]; }
  __device__ __forceinline__ void fetch16(uint32_t pos, uint32_t (&v)[4]) const {
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) v[i] = dw(pos + 4 * i);
  }
};
// Host memory: n bytes at p, 0 past them as the descriptor gives.
struct CpuKeys {
  const uint8_t* p;
  uint32_t n;
  uint32_t byte(uint32_t pos) const { return pos < n ? p[pos] : 0u; }
  uint32_t dw(uint32_t pos) const {
    return byte(pos) | (byte(pos + 1) << 8) | (byte(pos + 2) << 16) | (byte(pos + 3) << 24);
  }
  void fetch16(uint32_t pos, uint32_t (&v)[4]) const {
    for (uint32_t i = 0; i < 4; ++i) v[i] = dw(pos + 4 * i);
  }
};
// One key inside an arena: fingerprint32's byte source and the byte compare's operand.
template <class KS>
struct KeyRef {
  KS S;
  uint32_t pos, len;
  __host__ __device__ __forceinline__ uint32_t fetch(uint32_t i) const { return S.dw(pos + i); }
  __host__ __device__ __forceinline__ uint32_t byte(uint32_t i) const { return S.byte(pos + i); }
  __host__ __device__ __forceinline__ KeyRef skip(uint32_t k) const { return KeyRef{S, pos + k, len - k}; }
};
// The key [k0, k1) of the arena at `keys` through a descriptor of its own, exact to the aligned dword
// that holds byte k1 - 1: a load past the key is dropped, not fetched.  The lead is folded into the
// view's position, so the view carries one scalar less (five SGPR spills in sst_get_kernel).
__device__ __forceinline__ KeyRef<ArenaKeys> key_upto(const uint8_t* keys, uint32_t k0, uint32_t k1) {
  const uint32_t lead = uint32_t(reinterpret_cast<uintptr_t>(keys) & 3);
  ArenaKeys K;
  K.r = make_rsrc_exact(const_cast<uint8_t*>(keys - lead), k1 ? (lead + k1 + 3) & ~3u : 0u);
  K.lead = 0;
  return KeyRef<ArenaKeys>{K, lead + k0, k1 - k0};
}
// len bytes behind a plain pointer (file bytes, range bounds): nothing is read past them.
struct KeyPtr {
  const uint8_t* p;
  uint32_t len;
  __host__ __device__ __forceinline__ uint32_t byte(uint32_t i) const { return p[i]; }
  __host__ __device__ __forceinline__ KeyPtr skip(uint32_t k) const { return KeyPtr{p + k, len - k}; }
};

__host__ __device__ __forceinline__ int order3(uint32_t x, uint32_t y) { return x < y ? -1 : (x > y ? 1 : 0); }

// 16 bytes at any alignment in one load
typedef u32x4 u32x4_u __attribute__((aligned(1)));
__host__ __device__ __forceinline__ u32x4 load16u(const uint8_t* p) { return *reinterpret_cast<const u32x4_u*>(p); }

// ---------------------------------------------------------------- the image
// Storage forms: big-endian words (k16, ck, cks); two native u64, most significant first -- the
// merge tiles' LDS words (u32x4 {w1, w0, w3, w2} of the big-endian words) and lsmblk_sst_index's
// img_hi / img_lo are both this.  The order is two 64-bit compares without a branch: a chain of
// word compares compiled to a divergent branch per word (exec-mask SALU around every step of every
// binary search in the merge tiles, PMC: SALU 5.9e8 against VALU 7.3e8).
struct KeyImage {
  uint64_t hi, lo;  // bytes 0..7 and 8..15
  __host__ __device__ __forceinline__ static KeyImage be(const u32x4& k) {
    return KeyImage{(uint64_t(k.x) << 32) | k.y, (uint64_t(k.z) << 32) | k.w};
  }
  __host__ __device__ __forceinline__ u32x4 be_words() const {
    return u32x4{uint32_t(hi >> 32), uint32_t(hi), uint32_t(lo >> 32), uint32_t(lo)};
  }
  __host__ __device__ __forceinline__ static KeyImage pair(const u32x4& k) {
    return KeyImage{(uint64_t(k.y) << 32) | k.x, (uint64_t(k.w) << 32) | k.z};
  }
  __host__ __device__ __forceinline__ u32x4 u64_pair() const {
    return u32x4{uint32_t(hi), uint32_t(hi >> 32), uint32_t(lo), uint32_t(lo >> 32)};
  }
  __host__ __device__ __forceinline__ bool operator<(const KeyImage& o) const { return hi < o.hi || (hi == o.hi && lo < o.lo); }
  __host__ __device__ __forceinline__ bool operator<=(const KeyImage& o) const { return hi < o.hi || (hi == o.hi && lo <= o.lo); }
  __host__ __device__ __forceinline__ bool operator==(const KeyImage& o) const { return hi == o.hi && lo == o.lo; }
  __host__ __device__ __forceinline__ int cmp(const KeyImage& o) const {
    const bool lt = *this < o;
    return hi != o.hi || lo != o.lo ? (lt ? -1 : 1) : 0;
  }
};

// ---------------------------------------------------------------- image builders
// Every builder masks the bytes past the key's end: a real trailing 0x00 is told from the pad by the
// lengths, never by the image.
// ... from bytes [0, 16) as little-endian dwords
__host__ __device__ __forceinline__ KeyImage image_of_dwords(const uint32_t (&v)[4], uint32_t len) {
  uint32_t o[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    uint32_t x = v[i];
    const int32_t keep = int32_t(len) - int32_t(4 * i);  // bytes of this word inside the key
    if (keep < 4) x &= keep <= 0 ? 0u : (1u << (8 * keep)) - 1;
    o[i] = __builtin_bswap32(x);
  }
  return KeyImage::be(u32x4{o[0], o[1], o[2], o[3]});
}
// ... of the key at arena position pos
template <class KS>
__host__ __device__ __forceinline__ KeyImage image_of(const KS& S, uint32_t pos, uint32_t len) {
  uint32_t v[4];
  S.fetch16(pos, v);
  return image_of_dwords(v, len);
}
template <class KS>
__host__ __device__ __forceinline__ KeyImage image_of(const KeyRef<KS>& k) { return image_of(k.S, k.pos, k.len); }
// ... of p[0 .. len): 16 independent guarded byte loads (one round trip), nothing read past the key
__host__ __device__ __forceinline__ KeyImage image_of_bytes(const uint8_t* p, uint32_t len) {
  KeyImage m{0, 0};
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    const uint64_t x = j < len ? p[j] : 0;
    if (j < 8) m.hi |= x << (56 - 8 * j);
    else m.lo |= x << (56 - 8 * (j - 8));
  }
  return m;
}
// ... of the key at position pos of the arena (keys, total bytes) behind a plain pointer: ONE 16-byte
// load at any alignment where 16 bytes from the key's start lie inside the arena (every key but the
// arena's last few), else the byte form
__host__ __device__ __forceinline__ KeyImage image_of_load16(const uint8_t* keys, uint64_t total, uint32_t pos, uint32_t len) {
  if (uint64_t(pos) + 16 > total) return image_of_bytes(keys + pos, len);
  const u32x4 v = load16u(keys + pos);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  return image_of_dwords(w, len);
}

// ---------------------------------------------------------------- whole-key compares
// The first difference of keys (a, la) and (b, lb) of one arena, a dword a step: their common
// prefix, their order in {-1, 0, 1} and the two dwords that hold the difference (0 when one key is
// a prefix of the other).
struct KeyDiff {
  uint32_t lcp;
  int order;
  uint32_t w0, w1;
};
// One loop in two shapes, each measured where it runs (profiles/key_order_ab.json): kMaskFirst masks
// the last partial dword before the compare (the merge kernels' tails: with the other shape
// merge_tile_kernel took 1.97 ms against 1.87 on config C); otherwise the difference's place is held
// against the shorter length afterwards (the plan walk: with the masks plan_walk_kernel lost a wave
// of occupancy).
template <bool kMaskFirst, class KS>
__host__ __device__ __forceinline__ KeyDiff key_diff_as(const KS& S, uint32_t a, uint32_t la, uint32_t b, uint32_t lb) {
  const uint32_t m = la < lb ? la : lb;
  for (uint32_t i = 0; i < m; i += 4) {
    uint32_t x = S.dw(a + i), y = S.dw(b + i);
    if (kMaskFirst && m - i < 4) {
      const uint32_t mk = (1u << (8 * (m - i))) - 1;
      x &= mk;
      y &= mk;
    }
    if (x != y) {
      const uint32_t sh = uint32_t(__builtin_ctz(x ^ y)) & ~7u, z = i + (sh >> 3);
      if (kMaskFirst || z < m) return KeyDiff{z, ((x >> sh) & 0xFF) < ((y >> sh) & 0xFF) ? -1 : 1, x, y};
      break;  // (the bytes past the shorter key's end)
    }
  }
  return KeyDiff{m, order3(la, lb), 0, 0};
}
template <class KS>
__host__ __device__ __forceinline__ KeyDiff key_diff(const KS& S, uint32_t a, uint32_t la, uint32_t b, uint32_t lb) {
  return key_diff_as<false>(S, a, la, b, lb);
}
template <class KS>
__host__ __device__ __forceinline__ int key_cmp(const KS& S, uint32_t a, uint32_t la, uint32_t b, uint32_t lb) {
  return key_diff_as<true>(S, a, la, b, lb).order;
}

// Byte order of x against y, a byte a step (KeyPtr, KeyRef): -1, 0, 1.
template <class X, class Y>
__host__ __device__ int byte_cmp(const X& x, const Y& y) {
  const uint32_t mn = x.len < y.len ? x.len : y.len;
  for (uint32_t i = 0; i < mn; ++i) {
    const uint32_t u = x.byte(i), v = y.byte(i);
    if (u != v) return u < v ? -1 : 1;
  }
  return order3(x.len, y.len);
}

// Image-first order of two keys: tail() orders the bytes past 16 and runs only on a tie of the
// images with both keys longer than 16 bytes.
template <class Tail>
__host__ __device__ __forceinline__ int image_cmp(const KeyImage& x, uint32_t xl, const KeyImage& y, uint32_t yl, Tail tail) {
  const bool lt = x < y;
  if (x.hi != y.hi || x.lo != y.lo) return lt ? -1 : 1;
  if (xl <= 16 || yl <= 16) return order3(xl, yl);
  return tail();
}
// The same order by one lane of the read kernels, whose operands are byte views: the images one
// half after the other, then the whole keys byte by byte (no length rule: the byte loop decides a
// short key too).  Through image_cmp and a tail past byte 16, lsm_get_kernel, lsm_scan_rank_kernel
// and lsm_scan_expand_kernel measured slower (profiles/key_order_ab.json).
template <class X, class Y>
__host__ __device__ __forceinline__ int image_byte_cmp(const KeyImage& xm, const X& x, const KeyImage& ym, const Y& y) {
  if (xm.hi != ym.hi) return xm.hi < ym.hi ? -1 : 1;
  if (xm.lo != ym.lo) return xm.lo < ym.lo ? -1 : 1;
  return byte_cmp(x, y);
}
// ... and their common prefix: tail(order) returns the tails' and sets their order.
template <class Tail>
__host__ __device__ __forceinline__ uint32_t image_lcp(const KeyImage& x, uint32_t xl, const KeyImage& y, uint32_t yl, int& order,
                                                       Tail tail) {
  const uint32_t m = xl < yl ? xl : yl;
  const u32x4 xw = x.be_words(), yw = y.be_words();
  const uint32_t xs[4] = {xw.x, xw.y, xw.z, xw.w}, ys[4] = {yw.x, yw.y, yw.z, yw.w};
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    if (xs[w] != ys[w]) {
      const uint32_t z = 4 * w + (uint32_t(__builtin_clz(xs[w] ^ ys[w])) >> 3);
      if (z < m) {
        const uint32_t sh = 24 - 8 * (z & 3);
        order = ((xs[w] >> sh) & 0xFF) < ((ys[w] >> sh) & 0xFF) ? -1 : 1;
        return z;
      }
      order = order3(xl, yl);  // (a zero pad against a key byte)
      return m;
    }
  }
  if (m <= 16) {
    order = order3(xl, yl);
    return m;
  }
  return 16 + tail(order);
}

// x == y: the lengths, then unaligned 16-byte compares, then bytes.
__host__ __device__ __forceinline__ bool key_equal(const KeyPtr& x, const KeyPtr& y) {
  if (x.len != y.len) return false;
  bool differ = false;
  uint32_t i = 0;
  for (; i + 16 <= x.len && !differ; i += 16) {
    const u32x4 p = load16u(x.p + i), q = load16u(y.p + i);
    differ = p.x != q.x || p.y != q.y || p.z != q.z || p.w != q.w;
  }
  for (; i < x.len && !differ; ++i) differ = x.p[i] != y.p[i];
  return !differ;
}
// key k starts with f
__host__ __device__ __forceinline__ bool has_prefix(const KeyPtr& k, const KeyPtr& f) {
  if (f.len > k.len) return false;
  bool m = true;
  for (uint32_t x = 0; x < f.len && m; ++x) m = f.p[x] == k.p[x];
  return m;
}
// ... with one of the npfx prefixes of (pfx, pfx_off) (CompactionFilter::Prefix, src/compact.rs:264-275)
__host__ __device__ __forceinline__ bool has_any_prefix(const KeyPtr& k, const uint8_t* pfx, const uint32_t* pfx_off, uint32_t npfx) {
  for (uint32_t f = 0; f < npfx; ++f)
    if (has_prefix(k, KeyPtr{pfx + pfx_off[f], pfx_off[f + 1] - pfx_off[f]})) return true;
  return false;
}

}  // namespace
