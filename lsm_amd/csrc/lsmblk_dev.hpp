// lsmblk_dev.hpp -- shared by the HIP translation units of liblsmblk.so: wave primitives,
// buffer-descriptor helpers, the key order (lsmblk_keys.hpp), look-back granules (device) and the
// context struct (host).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "lsmblk.h"
#include "lsmblk_keys.hpp"  // (u32x4, rsrc_t, make_rsrc and the key order)

namespace {

constexpr uint32_t kSpinLimit = 1u << 22;  // look-back bound (~seconds); never reached when correct

// Diagnostics build (lsm_amd/_build.py builds liblsmblk_diag.so with -DLSMBLK_DIAG_BUILD=1 next to the
// product liblsmblk.so with 0): only there do the kernels honour the ablation masks of
// LSMBLK_DEBUG_DECODE_SKIP, which make outputs wrong for timing experiments.  In the product
// library the masks fold to 0 at compile time and lsmblk_debug_set refuses the key.
constexpr bool kDiag = LSMBLK_DIAG_BUILD != 0;
__device__ __forceinline__ uint32_t diag_mask(uint32_t skip) { return kDiag ? skip : 0u; }

// ---------------------------------------------------------------- wave primitives
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t uni(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// XCD-aware tile order: workgroup b runs on XCD b mod 8 (dispatch is round-robin over the eight
// XCDs, each with its own L2); tile xcd_tile(b) gives XCD x the contiguous tiles
// [x q + min(x, r), ...) of the G = 8 q + r, so kernels whose tiles read their neighbours' data
// (windows, near gathers) find it in their own XCD's L2.  A bijection on [0, G).
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t G) {
  const uint32_t x = b & 7, i = b >> 3, q = G >> 3, r = G & 7;
  return x * q + (x < r ? x : r) + i;
}
__device__ __forceinline__ uint64_t uni64(uint64_t x) {
  return (uint64_t(uni(uint32_t(x >> 32))) << 32) | uni(uint32_t(x));
}
// lane j's x (readlane returns int: both halves go through uint32_t, no sign extension)
__device__ __forceinline__ uint64_t lane64(uint64_t x, uint32_t j) {
  return (uint64_t(uint32_t(__builtin_amdgcn_readlane(uint32_t(x >> 32), j))) << 32) |
         uint32_t(__builtin_amdgcn_readlane(uint32_t(x), j));
}
// Read-only views in the constant address space: a uniform-address load through one is a scalar
// load (s_load: SGPR result, waited by lgkmcnt, so it never queues behind the vector loads that
// vmcnt counts in order).  Only for data no kernel of the same launch writes.
typedef const __attribute__((address_space(4))) uint32_t cu32_t;
typedef const __attribute__((address_space(4))) uint64_t cu64_t;
__device__ __forceinline__ cu32_t* kconst(const uint32_t* p) { return (cu32_t*)p; }
__device__ __forceinline__ cu64_t* kconst(const uint64_t* p) { return (cu64_t*)p; }
// threadIdx.x / 64 through readfirstlane: the compiler does not know it is wave-uniform, and a
// loop bound or block index derived from it would compile to an exec-masked (divergent) loop
__device__ __forceinline__ uint32_t wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Wave64 inclusive scan / sum of u32 with DPP (row_shr 1,2,4,8 then row_bcast 15 / 31):
// pure VALU, no ds_bpermute traffic through the LDS crossbar.
// (the builtin returns int: without the cast, max(uint32_t, int) resolves to the double overload
// and every max-scan step became two v_cvt_f64 + v_max_f64)
#define LSM_DPP(v, ctrl, rmask) uint32_t(__builtin_amdgcn_update_dpp(0u, (v), (ctrl), (rmask), 0xF, false))
__device__ __forceinline__ uint32_t wave_incl_scan32(uint32_t v) {
  v += LSM_DPP(v, 0x111, 0xF);  // row_shr:1
  v += LSM_DPP(v, 0x112, 0xF);  // row_shr:2
  v += LSM_DPP(v, 0x114, 0xF);  // row_shr:4
  v += LSM_DPP(v, 0x118, 0xF);  // row_shr:8
  v += LSM_DPP(v, 0x142, 0xA);  // row_bcast:15 -> rows 1, 3
  v += LSM_DPP(v, 0x143, 0xC);  // row_bcast:31 -> rows 2, 3
  return v;
}
__device__ __forceinline__ uint32_t wave_incl_max32(uint32_t v) {
  v = max(v, LSM_DPP(v, 0x111, 0xF));
  v = max(v, LSM_DPP(v, 0x112, 0xF));
  v = max(v, LSM_DPP(v, 0x114, 0xF));
  v = max(v, LSM_DPP(v, 0x118, 0xF));
  v = max(v, LSM_DPP(v, 0x142, 0xA));
  v = max(v, LSM_DPP(v, 0x143, 0xC));
  return v;
}
// Inclusive min-scan of values <= 0x7FFFFFFF as the max-scan of 0x7FFFFFFF - v: DPP lanes
// shifted in from outside a row read 0, the max identity.  (Measured on gfx950: an
// update_dpp "old" of 0xFFFFFFFF does not reach those lanes, and ~max(~v) was folded away.)
__device__ __forceinline__ uint32_t wave_incl_min31(uint32_t v) { return 0x7FFFFFFFu - wave_incl_max32(0x7FFFFFFFu - v); }
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
  return __builtin_amdgcn_readlane(wave_incl_scan32(v), 63);
}
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  if constexpr (sizeof(T) == 4) {
    return T(wave_incl_scan32(uint32_t(v)));
  } else {
    const uint32_t l = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      T t = __shfl_up(v, d, 64);
      if (l >= d) v += t;
    }
    return v;
  }
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  if constexpr (sizeof(T) == 4) {
    return T(__builtin_amdgcn_readlane(wave_incl_scan32(uint32_t(v)), 63));
  } else {
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
  }
}
__device__ __forceinline__ uint32_t bswap16(uint32_t v) { return ((v & 0xFF) << 8) | ((v >> 8) & 0xFF); }

// ---------------------------------------------------------------- look-back granules
// 8-byte granule = value << 16 | epoch << 2 | flag  (flag 1 = aggregate, 2 = inclusive).
// Written by one relaxed agent-scope store (global_store sc1), read by relaxed agent-scope
// loads: the value and its tag travel in one naturally aligned 8-byte word, so no fence is
// needed (MI355X_MICROARCH.md, "granule" hand-off).
// Poll protocol (kernel argument `poll`): 0 = sc1 loads; 1 = sc1 loads + agent acquire
// fence between polls; 2 = agent-scope atomic RMW (fetch_or 0) polls and atomic-swap
// publishes, performed at the coherence point.
__device__ __forceinline__ uint64_t gload(const uint64_t* p, uint32_t poll) {
  if (poll == 2)
    return __hip_atomic_fetch_or(const_cast<uint64_t*>(p), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gstore(uint64_t* p, uint64_t v, uint32_t poll) {
  if (poll == 2)
    (void)__hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int NQ>
__device__ __forceinline__ void publish(uint64_t* arr, uint64_t idx, const uint64_t (&v)[NQ],
                                        uint32_t tag, uint32_t flag, uint32_t poll) {
  const uint32_t l = lane_id();
  if (l < NQ) {
    uint64_t x = v[0];
    if (NQ > 1 && l == 1) x = v[1 % NQ];
    if (NQ > 2 && l == 2) x = v[2 % NQ];
    gstore(arr + idx * NQ + l, (x << 16) | (uint64_t(tag) << 2) | flag, poll);
  }
}

// Wave-parallel decoupled look-back: lane j inspects predecessor (pred - j).  Returns false
// on timeout (then excl is garbage and the caller raises LSMBLK_ERR_TIMEOUT).
template <int NQ>
__device__ __forceinline__ bool lookback(const uint64_t* agg, const uint64_t* inc, uint64_t self, uint32_t tag,
                         uint32_t poll, uint64_t (&excl)[NQ]) {
  const uint32_t l = lane_id();
  const uint64_t want_agg = (uint64_t(tag) << 2) | 1, want_inc = (uint64_t(tag) << 2) | 2;
#pragma unroll
  for (int q = 0; q < NQ; ++q) excl[q] = 0;
  int64_t pred = int64_t(self) - 1;
  uint32_t spins = 0;
  while (pred >= 0) {
    const int64_t idx = pred - int64_t(l);
    uint64_t vi[NQ], va[NQ];
    bool li = idx < 0, la = false;  // lanes before block 0 read as "inclusive 0"
#pragma unroll
    for (int q = 0; q < NQ; ++q) vi[q] = va[q] = 0;
    uint32_t round = 0;
    for (;;) {
      // Only lanes still unresolved poll.  A granule carrying the current epoch tag is the
      // value its producer wrote (each is written once per epoch), so a ready observation
      // is final; only not-ready observations are re-polled (first round plain sc1 loads,
      // later rounds the protocol `poll`).
      const uint32_t pm = round == 0 ? 0u : poll;
      if (!li && !la) {
        bool ri = true;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          vi[q] = gload(inc + idx * NQ + q, pm);
          ri = ri && ((vi[q] & 0xFFFF) == want_inc);
        }
        li = ri;
        if (!ri) {
          bool ra = true;
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            va[q] = gload(agg + idx * NQ + q, pm);
            ra = ra && ((va[q] & 0xFFFF) == want_agg);
          }
          la = ra;
        }
      }
      const uint64_t im = __ballot(li);
      const uint64_t rm = __ballot(li || la);
      const uint32_t first = im ? uint32_t(__builtin_ctzll(im)) : 64u;
      const uint64_t need = first >= 63 ? ~0ull : ((2ull << first) - 1);
      if ((rm & need) == need) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const uint64_t c = l < first ? (va[q] >> 16) : (l == first ? (vi[q] >> 16) : 0);
          excl[q] += wave_sum(c);
        }
        if (first < 64) return true;
        pred -= 64;
        break;
      }
      ++round;
      if (++spins > kSpinLimit) return false;
      if (poll == 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __builtin_amdgcn_s_sleep(1);
    }
  }
  return true;
}

__device__ __forceinline__ uint32_t take_ticket(uint32_t* ctr) {
  uint32_t t = 0;
  if (lane_id() == 0) t = atomicAdd(ctr, 1u);
  return uni(__shfl(t, 0, 64));
}

// Error flags: or_word ORs err into one 64-bit status word by the calling thread (nothing when
// err is 0); a call's flags live in stats[3].  or_err is the per-thread entry point, raise_err the
// wave-wide one (every lane calls it with the wave's flags, lane 0 acts).
__device__ __forceinline__ void or_word(uint64_t* word, uint32_t err) {
  if (err) atomicOr(reinterpret_cast<unsigned long long*>(word), (unsigned long long)err);
}
__device__ __forceinline__ void or_err(uint64_t* stats, uint32_t err) { or_word(stats + 3, err); }
__device__ __forceinline__ void raise_err(uint64_t* stats, uint32_t err) {
  if (lane_id() == 0) or_err(stats, err);
}

// ---------------------------------------------------------------- one-workgroup scan
// The top-level scan of every batched call: one workgroup of kWgScan threads (16 waves) over n
// items, in one of two forms.
//   share form   thread t sums its contiguous share of the items (share1024), the 1024 sums are
//                scanned once (block_excl1024) and the thread walks its share again from its base:
//                for items whose values are re-read or recomputed, any n in two barriers.
//   rounds form  rounds of 1024 consecutive items, thread t item r + t (coalesced loads), each
//                round's scan on top of a carry (block_round1024): for items loaded once.
constexpr uint32_t kWgScan = 1024;

// thread t's contiguous share [x0, x1) of n items
__device__ __forceinline__ void share1024(uint64_t n, uint64_t& x0, uint64_t& x1) {
  const uint64_t per = (n + kWgScan - 1) / kWgScan, t = threadIdx.x;
  x0 = per * t < n ? per * t : n;
  x1 = x0 + per < n ? x0 + per : n;
}
// Exclusive prefixes of the NQ sums v over the workgroup's 1024 threads, and the totals (in every
// thread).  wsum: 16 x NQ words of LDS, free again after the call's second barrier.
template <int NQ>
__device__ __forceinline__ void block_excl1024(const uint64_t (&v)[NQ], uint64_t (*wsum)[NQ], uint64_t (&base)[NQ],
                                               uint64_t (&tot)[NQ]) {
  static_assert(kWgScan == 16 * 64, "16 wave sums");
  const uint32_t w = threadIdx.x >> 6;
  uint64_t inc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) inc[q] = wave_incl_scan<uint64_t>(v[q]);
  // (pinned after the wave scans: the compiler otherwise moves the barrier above them, so that
  // every round waits for its slowest wave before any wave scans: sst_layout_kernel 7.6 -> 8.4 us
  // at 2500 SSTs, profiles/top_scan_ab.json)
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();  // wsum's previous use is over
  if (lane_id() == 63) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) wsum[w][q] = inc[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    uint64_t b = 0, s = 0;
    for (uint32_t x = 0; x < 16; ++x) {
      if (x < w) b += wsum[x][q];
      s += wsum[x][q];
    }
    base[q] = b + inc[q] - v[q];
    tot[q] = s;
  }
}
__device__ __forceinline__ uint64_t block_excl1024(uint64_t v, uint64_t* wsum, uint64_t& tot) {
  const uint64_t v1[1] = {v};
  uint64_t b[1], s[1];
  block_excl1024<1>(v1, reinterpret_cast<uint64_t(*)[1]>(wsum), b, s);
  tot = s[0];
  return b[0];
}
// One round of the rounds form: base = carry + the round's exclusive prefixes, carry += its totals.
template <int NQ>
__device__ __forceinline__ void block_round1024(const uint64_t (&v)[NQ], uint64_t (*wsum)[NQ], uint64_t (&carry)[NQ],
                                                uint64_t (&base)[NQ]) {
  uint64_t tot[NQ];
  block_excl1024<NQ>(v, wsum, base, tot);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    base[q] += carry[q];
    carry[q] += tot[q];
  }
}
__device__ __forceinline__ uint64_t block_round1024(uint64_t v, uint64_t* wsum, uint64_t& carry) {
  uint64_t tot;
  const uint64_t base = carry + block_excl1024(v, wsum, tot);
  carry += tot;
  return base;
}

// The totals epilogue of a batched call, by exactly one thread: stats[0..2] = tot (entries, key
// bytes, value bytes), LSMBLK_ERR_OVERFLOW when the key or value bytes (with ovf_entries, the
// entries too) pass 2^32, LSMBLK_ERR_CAPACITY when a total passes its cap, the key_off[N] /
// val_off[N] sentinels, and err (seeded by the caller) ORed into stats[3].  The sentinels go out
// when the call is clean (kSentIfClean) or whenever N fits (kSentIfFits); never through null
// pointers (a call without outputs, which passes caps of ~0 as well).
enum SentinelRule { kSentIfClean, kSentIfFits };
struct TotalCaps {
  uint64_t entry, key, val;
};
__device__ __forceinline__ void publish_totals(uint64_t* stats, const uint64_t (&tot)[3], const TotalCaps& cap,
                                               uint32_t* okey_off, uint32_t* oval_off, SentinelRule rule,
                                               uint32_t err = 0, bool ovf_entries = false) {
  for (uint32_t q = 0; q < 3; ++q) stats[q] = tot[q];
  if ((ovf_entries && tot[0] > 0xFFFFFFFFull) || tot[1] > 0xFFFFFFFFull || tot[2] > 0xFFFFFFFFull) err |= LSMBLK_ERR_OVERFLOW;
  if (tot[0] > cap.entry || tot[1] > cap.key || tot[2] > cap.val) err |= LSMBLK_ERR_CAPACITY;
  if (okey_off && (rule == kSentIfFits ? tot[0] <= cap.entry : !err)) {
    okey_off[tot[0]] = uint32_t(tot[1]);
    oval_off[tot[0]] = uint32_t(tot[2]);
  }
  or_err(stats, err);
}

// len bytes src -> dst by the whole wave, any alignment (16-B pieces, 1 KiB per instruction).
__device__ __forceinline__ void wave_copy_bytes(uint8_t* dst, const uint8_t* src, uint64_t len) {
  for (uint64_t o = 16ull * lane_id(); o < len; o += 1024) {
    if (o + 16 <= len) {
      *reinterpret_cast<u32x4*>(dst + o) = *reinterpret_cast<const u32x4*>(src + o);
    } else {
      for (uint64_t x = o; x < len; ++x) dst[x] = src[x];
    }
  }
}

// ---------------------------------------------------------------- farmhash fingerprint32
// farmhash 1.1.5 fingerprint32 = farmhashmk::Hash32 of Google's FarmHash (a CityHash descendant):
// restated from the published algorithm (oracle/pyref.py has the same restatement; parity with
// the crate itself is unpinned here -- DESIGN.md).  Rotate is a right rotation; Fetch a
// little-endian u32 load at any byte offset.
constexpr uint32_t kF1 = 0xcc9e2d51u, kF2 = 0x1b873593u;

__host__ __device__ __forceinline__ uint32_t frot(uint32_t v, uint32_t s) { return s ? (v >> s) | (v << (32 - s)) : v; }
__host__ __device__ __forceinline__ uint32_t ffmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
__host__ __device__ __forceinline__ uint32_t fmur(uint32_t a, uint32_t h) {
  a *= kF1;
  a = frot(a, 17);
  a *= kF2;
  h ^= a;
  h = frot(h, 19);
  return h * 5 + 0xe6546b64u;
}

// Src: a byte source with u32 fetches at arbitrary offsets (bytes [i, i + 4), little-endian)
// and single bytes (KeyRef).
template <class Src>
__host__ __device__ uint32_t fingerprint32(const Src& S, uint32_t len) {
  if (len <= 4) {
    uint32_t b = 0, c = 9;
    for (uint32_t i = 0; i < len; ++i) {
      const int32_t v = int32_t(int8_t(S.byte(i)));  // signed char
      b = b * kF1 + uint32_t(v);
      c ^= b;
    }
    return ffmix(fmur(b, fmur(len, c)));
  }
  if (len <= 12) {
    uint32_t a = len, b = len * 5, c = 9, d = b;
    a += S.fetch(0);
    b += S.fetch(len - 4);
    c += S.fetch((len >> 1) & 4);
    return ffmix(fmur(c, fmur(b, fmur(a, d))));
  }
  if (len <= 24) {
    uint32_t a = S.fetch((len >> 1) - 4), b = S.fetch(4), c = S.fetch(len - 8), d = S.fetch(len >> 1);
    const uint32_t e = S.fetch(0), f = S.fetch(len - 4);
    uint32_t h = d * kF1 + len;
    a = frot(a, 12) + f;
    h = fmur(c, h) + a;
    a = frot(a, 3) + c;
    h = fmur(e, h) + a;
    a = frot(a + f, 12) + d;
    h = fmur(b, h) + a;
    return ffmix(h);
  }
  uint32_t h = len, g = kF1 * len, f = g;
  const uint32_t a0 = frot(S.fetch(len - 4) * kF1, 17) * kF2, a1 = frot(S.fetch(len - 8) * kF1, 17) * kF2;
  const uint32_t a2 = frot(S.fetch(len - 16) * kF1, 17) * kF2, a3 = frot(S.fetch(len - 12) * kF1, 17) * kF2;
  const uint32_t a4 = frot(S.fetch(len - 20) * kF1, 17) * kF2;
  h ^= a0;
  h = frot(h, 19);
  h = h * 5 + 0xe6546b64u;
  h ^= a2;
  h = frot(h, 19);
  h = h * 5 + 0xe6546b64u;
  g ^= a1;
  g = frot(g, 19);
  g = g * 5 + 0xe6546b64u;
  g ^= a3;
  g = frot(g, 19);
  g = g * 5 + 0xe6546b64u;
  f += a4;
  f = frot(f, 19) + 113;
  uint32_t iters = (len - 1) / 20, p = 0;
  do {
    const uint32_t a = S.fetch(p), b = S.fetch(p + 4), c = S.fetch(p + 8), d = S.fetch(p + 12), e = S.fetch(p + 16);
    h += a;
    g += b;
    f += c;
    h = fmur(d, h) + e;
    g = fmur(c, g) + a;
    f = fmur(b + e * kF1, f) + d;
    f += g;
    g += f;
    p += 20;
  } while (--iters != 0);
  g = frot(g, 11) * kF1;
  g = frot(g, 17) * kF1;
  f = frot(f, 11) * kF1;
  f = frot(f, 17) * kF1;
  h = frot(h + g, 19);
  h = h * 5 + 0xe6546b64u;
  h = frot(h, 17) * kF1;
  h = frot(h + f, 19);
  h = h * 5 + 0xe6546b64u;
  h = frot(h, 17) * kF1;
  return h;
}

// ---------------------------------------------------------------- byte sources
// An "image" is a block's bytes addressed block-relative; LdsImg reads the LDS staging copy,
// GlbImg reads global memory through a bounds-checked buffer descriptor (OOB reads = 0).
// Decode reads the (unswizzled) LDS image with unaligned ds_read_u16/b32/b64/b128 (the gfx9
// unaligned access mode): one instruction per field instead of one per byte.
#ifndef LSMBLK_XALIGNED_LDS
#define LSMBLK_XALIGNED_LDS 0
#endif
// 4 / 8 bytes at byte x of a 16-B-aligned LDS buffer (any alignment) from aligned dwords: the LDS
// array serves a misaligned access with extra passes (PMC SQ_LDS_UNALIGNED_STALL), two or three
// aligned dword reads + v_alignbyte do not stall.
__device__ __forceinline__ uint32_t lds_dw_al(const uint8_t* base, uint32_t x) {
  const uint32_t* d = reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(base, 16)) + (x >> 2);
  return __builtin_amdgcn_alignbyte(d[1], d[0], x & 3);
}
__device__ __forceinline__ u32x2 lds_qw_al(const uint8_t* base, uint32_t x) {
  const uint32_t* d = reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(base, 16)) + (x >> 2);
  const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], sh = x & 3;
  return u32x2{__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh)};
}
struct LdsImg {
  const uint8_t* base;  // LDS image; block byte 0 is image byte lead
  uint32_t lead;
  __device__ __forceinline__ uint32_t u8(uint32_t i) const { return base[lead + i]; }
  __device__ __forceinline__ uint32_t u16(uint32_t i) const {
    if constexpr (LSMBLK_XALIGNED_LDS) return bswap16(lds_dw_al(base, lead + i) & 0xFFFFu);
    return bswap16(*reinterpret_cast<const uint16_t*>(base + lead + i));
  }
  __device__ __forceinline__ uint32_t le32(uint32_t i) const {
    if constexpr (LSMBLK_XALIGNED_LDS) return lds_dw_al(base, lead + i);
    return *reinterpret_cast<const uint32_t*>(base + lead + i);
  }
  __device__ __forceinline__ uint64_t u64(uint32_t i) const {
    const u32x2 q = LSMBLK_XALIGNED_LDS ? lds_qw_al(base, lead + i) : *reinterpret_cast<const u32x2*>(base + lead + i);
    return __builtin_bswap64((uint64_t(q.y) << 32) | q.x);
  }
};
struct GlbImg {
  rsrc_t r;
  uint32_t lead;  // rsrc base = block start - lead
  __device__ __forceinline__ uint32_t u8(uint32_t i) const {
    return __builtin_amdgcn_raw_buffer_load_b8(r, lead + i, 0, 0);
  }
  // Wider fields as one unaligned buffer load each (the gfx9 unaligned access mode) instead of a
  // byte load per byte.  A load that reaches past the descriptor bound returns 0 as a whole
  // (byte loads would return the bytes before the bound): the parse rules reject every entry
  // whose fields reach past the block before using them, so the results agree on valid blocks
  // and the MALFORMED verdicts agree on all.
  __device__ __forceinline__ uint32_t u16(uint32_t i) const {
    return bswap16(__builtin_amdgcn_raw_buffer_load_b16(r, lead + i, 0, 0));
  }
  __device__ __forceinline__ uint32_t le32(uint32_t i) const {
    return __builtin_amdgcn_raw_buffer_load_b32(r, lead + i, 0, 0);
  }
  __device__ __forceinline__ uint64_t u64(uint32_t i) const {
    const u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(r, lead + i, 0, 0);
    return (uint64_t(__builtin_bswap32(q.x)) << 32) | __builtin_bswap32(q.y);
  }
};

// ---------------------------------------------------------------- the block parser
// The one definition of a well-formed block ("Validation rules"): the decode, its counts,
// crc_kernel<true>'s count_block and the scan kernels of lsmblk_get.hip parse through these two
// functions, and every read kernel takes its header from parse_hdr, so they give one MALFORMED
// verdict.  Two restatements of the entry rules remain, each load behind its check: seek_kernel
// (lsmblk_sst.hip: a raw pointer, a load must not leave the block) and block_lu (lsmblk_get.hip:
// the point read measured slower through parse_entry).  tests/test_gpu_block_rules.py holds all of
// them to every rule.
// Contract: parse_entry loads before it checks, so the image's out-of-range reads must not fault --
// GlbImg's descriptor returns 0 past its bound, an LDS read past the image returns other LDS bytes
// or 0 -- and whatever such a read returns, the entry fails a rule.  A failed entry's p, s and vl
// are 0.
struct BlockHdr {
  uint32_t len, n, data_end, fks;
  bool ok;
};

template <class Img>
__device__ __forceinline__ BlockHdr parse_hdr(const Img& im, uint32_t len) {
  BlockHdr h{len, 0, 0, 0, true};
  if (len < 2) { h.ok = false; return h; }
  h.n = im.u16(len - 2);
  if (2 + 2 * h.n > len) { h.ok = false; h.n = 0; return h; }
  h.data_end = len - 2 - 2 * h.n;
  if (h.n) {
    // get_first_key (iterator.rs:23-34) parses the entry at data position 0.
    if (h.data_end < 4) { h.ok = false; return h; }
    h.fks = im.u16(2);
    if (4 + h.fks + 8 > h.data_end) h.ok = false;
  }
  return h;
}

// Corrected seek_to_offset (iterator.rs:125-139) with the validation rules of DESIGN.md.
template <class Img>
__device__ __forceinline__ bool parse_entry(const Img& im, const BlockHdr& h, uint32_t k,
                                            uint32_t& off, uint32_t& p, uint32_t& s, uint32_t& vl) {
  off = im.u16(h.data_end + 2 * k);
  bool ok = off + 4 <= h.data_end;
  const uint32_t w = im.le32(off);  // BE16 p | BE16 s
  p = bswap16(w & 0xFFFF);
  s = bswap16(w >> 16);
  ok = ok && (off + 4 + s + 10 <= h.data_end) && (p <= h.fks) && (p + s > 0);
  vl = im.u16(off + 12 + s);
  ok = ok && (off + 14 + s + vl <= h.data_end);
  if (!ok) { p = s = vl = 0; }
  return ok;
}

// 4 bytes starting at byte offset x of a 4-byte-aligned LDS buffer.
__device__ __forceinline__ uint32_t lds_dword_at(const uint8_t* base, uint32_t x) {
  return *reinterpret_cast<const uint32_t*>(base + x);  // unaligned ds_read_b32
}

// Store bytes [lo, hi) (0 <= lo < hi <= 16) of a 16-B chunk at dst (16-aligned): one b128
// store when whole, else conditional whole-dword stores plus at most three bytes at each
// end (closed-form; a wave pays ~10 stores for its partial lanes, not 16 byte stores).
__device__ __forceinline__ void store_chunk(uint8_t* dst, const uint32_t (&v)[4], uint32_t lo, uint32_t hi) {
  if (lo == 0 && hi == 16) {
    // streamed: written once, read by a later pass (nt stores: U 735 against 722 GiB/s)
    __builtin_nontemporal_store(u32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<u32x4*>(dst));
    return;
  }
  const uint32_t lo4 = (lo + 3) >> 2, hi4 = hi >> 2;  // whole dwords [lo4, hi4)
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d)
    if (d >= lo4 && d < hi4) d32[d] = v[d];
  // head bytes [lo, min(hi, 4 lo4)) and tail bytes [max(lo, 4 hi4), hi); when the range lies
  // inside one dword both describe the same bytes: only the head copy writes them
  const uint32_t he = min(hi, 4 * lo4), ts = max(max(lo, 4 * hi4), he);
  const uint32_t hw = v[min(lo >> 2, 3u)], tw = v[min(hi4, 3u)];
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i) {
    const uint32_t x = lo + i;
    if (x < he) dst[x] = uint8_t(hw >> (8 * (x & 3)));
  }
#pragma unroll
  for (uint32_t i = 0; i < 3; ++i) {
    const uint32_t x = ts + i;
    if (x < hi) dst[x] = uint8_t(tw >> (8 * (x & 3)));
  }
}

// LDS image bytes [lo, lo + len) -> global memory, where image byte x mirrors global byte
// gdst_aligned + x (gdst_aligned 16-B aligned, lo < 16), by threads tid < nthr of the caller:
//   * every whole 16-B chunk with one aligned (nt) store, B chunks per thread per round (threads
//     past the last chunk masked off: repeating a chunk from many lanes serialised the stores);
//   * the at most two partial edge chunks (the head chunk when lo > 0 or the run ends inside it,
//     the tail chunk when lo + len is not 16-aligned) one byte per thread, threads 0..15 the head
//     and 16..31 the tail: one predicated byte store for both.
// (Per-lane byte-masked edge stores inside the chunk loop compiled to ~15 exec-mask branches per
// unrolled chunk, every round that held an edge: the scalar unit is the decode's busiest pipe.)
// Store policy of a whole-chunk flush store: 0 nt (keeps the line in the XCD's L2), 1 sc1
// (write-through: the line leaves L2, MI355X_MICROARCH.md), 2 plain.
#ifndef LSMBLK_XDEC_STORE
#define LSMBLK_XDEC_STORE 0
#endif
template <int POL>
__device__ __forceinline__ void st_chunk16(uint8_t* dst, const u32x4& q) {
  if constexpr (POL == 1)
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(q) : "memory");
  else if constexpr (POL == 2)
    *reinterpret_cast<u32x4*>(dst) = q;
  else
    __builtin_nontemporal_store(q, reinterpret_cast<u32x4*>(dst));
}
template <uint32_t B, int POL = 0>
__device__ __forceinline__ void flush_chunks(uint8_t* gdst_aligned, const uint8_t* lds, uint32_t lo, uint32_t len,
                                             uint32_t tid, uint32_t nthr) {
  if (len == 0) return;
  const uint32_t end = lo + len, nc = (end + 15) >> 4;
  const bool head_part = lo != 0 || end < 16, tail_part = (end & 15) != 0;
  const uint32_t cf = head_part ? 1u : 0u;                 // first whole chunk
  const uint32_t ce = tail_part ? nc - 1 : nc;             // one past the last whole chunk
  {
    const uint32_t x = tid < 16 ? tid : 16 * (nc - 1) + (tid - 16);  // the edge byte of this thread
    if (tid < 32 && (tid < 16 ? head_part : tail_part) && x >= lo && x < end) gdst_aligned[x] = lds[x];
  }
  if (ce > cf) {
    const uint32_t nw = ce - cf;
    for (uint32_t c0 = 0; c0 < nw; c0 += nthr * B) {
      u32x4 q[B];
#pragma unroll
      for (uint32_t j = 0; j < B; ++j)
        if (c0 + nthr * j + tid < nw) q[j] = *reinterpret_cast<const u32x4*>(lds + 16 * (cf + c0 + nthr * j + tid));
#pragma unroll
      for (uint32_t j = 0; j < B; ++j)
        if (c0 + nthr * j + tid < nw) st_chunk16<POL>(gdst_aligned + 16 * (cf + c0 + nthr * j + tid), q[j]);
    }
  }
}
}  // namespace


// ---------------------------------------------------------------- CRC-32 (crc32fast) tables
namespace {
constexpr uint32_t kCrcChunk = 4096;
// A chunk is cut into lane segments of kCrcSeg = 68 B (17 dwords, odd): lane l's dword i is
// then LDS bank (17 l + i) mod 32, so the 32 lanes of a ds_read_b32 group hit 32 distinct
// banks.  64-B segments put every lane of a group on 2 banks (a 16-way conflict per read).
constexpr uint32_t kCrcSeg = 68;
constexpr uint32_t kCrcMats = 7;  // Z(., kCrcSeg << j), j = 0..5, and j = 6: Z(., kCrcChunk)
// crc_chunk reads up to kCrcPad bytes before a chunk, which must hold zeros
constexpr uint32_t kCrcPad = 80;
constexpr uint32_t kCrcStage = kCrcPad + 5 * 1024;  // zero pad, five 1-KiB load pieces
struct alignas(16) CrcTabs {
  uint32_t fold[8][16];              // R_0 after xoring a dword into the register: by nibble
  uint32_t shift[kCrcMats][8][16];   // Z(., kCrcSeg << j), j < 6, Z(., kCrcChunk): by nibble
  uint32_t zinv[kCrcSeg];            // zinv[j]: the register that j zero bytes take to the init
  uint32_t unz[3][8][16];            // Z(., t)^-1, t = 1..3: undoes t appended zero bytes
  uint32_t z32[8][16];               // Z(., 32): joins a window's two fold chains
};
// crc_stream_kernel (the plain CRC pass): the stride step Z(., 256) as four byte tables (each
// workgroup replicates them 32 times in LDS), the joins as nibble maps.
struct alignas(16) CrcStreamTabs {
  uint32_t a256[4][256];             // a256[k][v] = Z(v << 8k, 256)
  uint32_t unz4[8][16];              // Z(., 4)^-1: a lane's four dword chains
  uint32_t unzl[4][8][16];           // Z(., 16 << b)^-1, b = 0..3: the lane tree of a 16-lane row
  uint32_t z4096[8][16];             // Z(., 4096): chunk after chunk
  uint32_t unzt[16][8][16];          // Z(., t)^-1: t tail zero bytes (t = 0 unused)
  uint32_t zinit[260];               // zinit[m] = Z(0xFFFFFFFF, 16 m), m = 0..256
};
struct alignas(16) CrcAllTabs {
  CrcTabs t;
  CrcStreamTabs s;
};

// 4 * (byte B of v & 15 << 2 ...): (byte B of v) & 0x3C as one SDWA instruction
template <int B>
__device__ __forceinline__ uint32_t sdwa_and(uint32_t v, uint32_t m) {
  uint32_t r;
  if constexpr (B == 0)
    asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(r) : "v"(v), "v"(m));
  else if constexpr (B == 1)
    asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(r) : "v"(v), "v"(m));
  else if constexpr (B == 2)
    asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(r) : "v"(v), "v"(m));
  else
    asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(r) : "v"(v), "v"(m));
  return r;
}
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

// m applied to x: the XOR of m[k][nibble k of x].  The LDS byte offsets 4 * nibble come from
// y = x << 2 (even nibbles: byte k/2 of y, bits 2..5) and z = x >> 2 (odd nibbles: byte
// (k-1)/2 of z), one SDWA AND with 0x3C each, so a map costs 2 + 8 + 4 VALU (xor3 tree).
__device__ __forceinline__ uint32_t crc_apply(const uint32_t (&m)[8][16], uint32_t x) {
  const uint32_t y = x << 2, z = x >> 2, k3c = 0x3C;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(&m[0][0]);
  auto at = [&](uint32_t k, uint32_t off) { return *reinterpret_cast<const uint32_t*>(b + 64 * k + off); };
  const uint32_t a0 = at(0, sdwa_and<0>(y, k3c)), a1 = at(1, sdwa_and<0>(z, k3c));
  const uint32_t a2 = at(2, sdwa_and<1>(y, k3c)), a3 = at(3, sdwa_and<1>(z, k3c));
  const uint32_t a4 = at(4, sdwa_and<2>(y, k3c)), a5 = at(5, sdwa_and<2>(z, k3c));
  const uint32_t a6 = at(6, sdwa_and<3>(y, k3c)), a7 = at(7, sdwa_and<3>(z, k3c));
  return xor3(xor3(xor3(a0, a1, a2), a3, a4), a5, a6) ^ a7;
}

// R over the chunk bytes p[0, sz) (LDS), 0 < sz + t <= 64 * kCrcSeg; the block's first chunk
// starts from the CRC init.  Every lane returns the chunk's register.
//
// The chunk is read as M || 0^t, t < 4 zero bytes the caller placed after it (so that p + sz + t
// is 4-aligned and every window read is an aligned dword); the register of M || 0^t is
// Z(R(M), t), undone by the map unz[t - 1] at the end.  Lane l >= l0 = 64 - ceil((sz + t) / 68)
// folds the 68-B window that ends 68 (63 - l) bytes before the end: 17 dword steps, fully
// unrolled, every load issued first.  Lane l0's window starts up to 67 bytes before p: the
// caller keeps p[-kCrcPad, 0) zero, and zero bytes leave a zero register unchanged, so the
// window's CRC is the chunk head's.  On a block's first chunk lane l0 starts from zinv[68 - r]
// instead, the register that the 68 - r leading zeros carry to the init 0xFFFFFFFF.
__device__ __forceinline__ uint32_t crc_chunk(const CrcTabs& T, const uint8_t* p, uint32_t sz, bool first,
                                              uint32_t t = 0) {
  const uint32_t l = lane_id(), sx = sz + t;
  const uint32_t nseg = (sx + kCrcSeg - 1) / kCrcSeg, l0 = 64 - nseg, r = sx - kCrcSeg * (nseg - 1);
  const bool live = l >= l0;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(live ? p + sx - kCrcSeg * (64 - l) : p - kCrcSeg);
  uint32_t d[kCrcSeg / 4];
#pragma unroll
  for (uint32_t i = 0; i < kCrcSeg / 4; ++i) d[i] = q[i];
  // two independent fold chains per lane (dwords 0..8 and 9..16, joined by Z(., 32)): the
  // dependent LDS round trips per window drop from 17 to 10
  uint32_t ca = first && l == l0 ? T.zinv[kCrcSeg - r] : 0u, cb = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    ca = crc_apply(T.fold, ca ^ d[i]);
    cb = crc_apply(T.fold, cb ^ d[9 + i]);
  }
  ca = crc_apply(T.fold, ca ^ d[8]);
  uint32_t crc = crc_apply(T.z32, ca) ^ cb;
  const uint32_t m = 63 - l;  // full windows after this one
#pragma unroll
  for (uint32_t j = 0; j < 6; ++j)
    if ((m >> j) & 1) crc = crc_apply(T.shift[j], crc);
  crc = live ? crc : 0u;
#pragma unroll
  for (uint32_t dd = 32; dd >= 1; dd >>= 1) crc ^= __shfl_xor(crc, dd, 64);
  if (t) crc = crc_apply(T.unz[t - 1], crc);
  return crc;
}

// Persistent waves, one block at a time, the next chunk's loads in flight while the current
// one is folded.  A block of len bytes has ceil(len / 4096) chunks; the first holds the
// len mod 4096 remainder (or a full 4096), so every later chunk is full.
}  // namespace
namespace {
// CRC tables (host).  Each linear map of the 32-bit register is tabulated by its columns
// (the images of the 32 unit vectors), then as eight nibble tables.
inline uint32_t crc_bit_step(uint32_t c) { return (c >> 1) ^ ((c & 1) ? 0xEDB88320u : 0u); }
inline void crc_nibble_tables(const uint32_t (&col)[32], uint32_t (&m)[8][16]) {
  for (uint32_t k = 0; k < 8; ++k)
    for (uint32_t v = 0; v < 16; ++v) {
      uint32_t y = 0;
      for (uint32_t bit = 0; bit < 4; ++bit)
        if ((v >> bit) & 1) y ^= col[4 * k + bit];
      m[k][v] = y;
    }
}
// inverse of one bit step: the top bit of c' says whether the polynomial was folded in
inline uint32_t crc_bit_unstep(uint32_t c) { return (c & 0x80000000u) ? ((c ^ 0xEDB88320u) << 1) | 1u : c << 1; }
inline void crc_host_tables(CrcTabs& T) {
  uint32_t z = 0xFFFFFFFFu;
  for (uint32_t j = 0; j < kCrcSeg; ++j) {
    T.zinv[j] = z;
    for (int s = 0; s < 8; ++s) z = crc_bit_unstep(z);
  }
  for (uint32_t t = 1; t <= 3; ++t) {  // Z(., t)^-1: 8 t inverse bit steps
    uint32_t col[32];
    for (uint32_t bit = 0; bit < 32; ++bit) {
      uint32_t x = 1u << bit;
      for (uint32_t s = 0; s < 8 * t; ++s) x = crc_bit_unstep(x);
      col[bit] = x;
    }
    crc_nibble_tables(col, T.unz[t - 1]);
  }
  uint32_t col[32];
  for (uint32_t bit = 0; bit < 32; ++bit) {  // fold: 32 bit steps (4 zero bytes after the xor)
    uint32_t x = 1u << bit;
    for (int s = 0; s < 32; ++s) x = crc_bit_step(x);
    col[bit] = x;
  }
  crc_nibble_tables(col, T.fold);
  for (uint32_t bit = 0; bit < 32; ++bit) {  // Z(., 32): 256 bit steps
    uint32_t x = 1u << bit;
    for (uint32_t s = 0; s < 256; ++s) x = crc_bit_step(x);
    col[bit] = x;
  }
  crc_nibble_tables(col, T.z32);
  for (uint32_t j = 0; j < kCrcMats; ++j) {  // Z(., n) = 8 n bit steps
    const uint32_t steps = 8u * (j < 6 ? kCrcSeg << j : kCrcChunk);
    for (uint32_t bit = 0; bit < 32; ++bit) {
      uint32_t x = 1u << bit;
      for (uint32_t s = 0; s < steps; ++s) x = crc_bit_step(x);
      col[bit] = x;
    }
    crc_nibble_tables(col, T.shift[j]);
  }
}
// columns of Z(., bytes) (bytes > 0) or Z(., -bytes)^-1 (bytes < 0)
inline void crc_shift_cols(int64_t bytes, uint32_t (&col)[32]) {
  for (uint32_t bit = 0; bit < 32; ++bit) {
    uint32_t x = 1u << bit;
    if (bytes >= 0)
      for (int64_t s = 0; s < 8 * bytes; ++s) x = crc_bit_step(x);
    else
      for (int64_t s = 0; s < -8 * bytes; ++s) x = crc_bit_unstep(x);
    col[bit] = x;
  }
}
inline void crc_stream_host_tables(CrcStreamTabs& T) {
  uint32_t col[32];
  crc_shift_cols(256, col);
  for (uint32_t k = 0; k < 4; ++k)
    for (uint32_t v = 0; v < 256; ++v) {
      uint32_t y = 0;
      for (uint32_t bit = 0; bit < 8; ++bit)
        if ((v >> bit) & 1) y ^= col[8 * k + bit];
      T.a256[k][v] = y;
    }
  crc_shift_cols(-4, col);
  crc_nibble_tables(col, T.unz4);
  for (uint32_t b = 0; b < 4; ++b) {
    crc_shift_cols(-(int64_t(16) << b), col);
    crc_nibble_tables(col, T.unzl[b]);
  }
  crc_shift_cols(4096, col);
  crc_nibble_tables(col, T.z4096);
  for (uint32_t t = 0; t < 16; ++t) {
    crc_shift_cols(-int64_t(t), col);
    crc_nibble_tables(col, T.unzt[t]);
  }
  uint32_t z = 0xFFFFFFFFu;
  for (uint32_t m = 0; m < 260; ++m) {
    T.zinit[m] = z;
    for (int s = 0; s < 128; ++s) z = crc_bit_step(z);
  }
}

}  // namespace

constexpr uint32_t kDecLagDefault = 10240;
constexpr uint64_t kDecLagBytesDefault = 10240ull * 4096;
constexpr uint32_t kScanUnitsDefault = 1u << 17;

// Look-back status granules live in uncached device memory: every poll and publish goes to
// the coherence point, so no XCD's L2 can hold a stale copy (MI355X L2s are per XCD and not
// coherent with each other).
constexpr unsigned kStatusFlags = hipDeviceMallocUncached;

// A workspace buffer of a context: grown on demand on the calling ABI call's stream, released
// with the context.  A context's buffers chain themselves (lsmblk_ctx::bufs, DevBufBase::next), so
// lsmblk_ctx_destroy releases them without naming them.
//
// Growth is ordered on the call's stream `st`:
//   * the new buffer is zeroed by hipMemsetAsync on st, so the fill precedes every kernel the call
//     launches on st (round 4's hang: a null-stream hipMemset, unordered with the caller's
//     non-blocking stream, wiped a fresh context's rotation levels after they were written);
//   * ordinary buffers come from the device's stream-ordered pool (hipMallocAsync) and the old one
//     is released by hipFreeAsync on st, after the work queued before it on st -- a context's
//     work is on its caller's stream, and every call that forks onto the context's second stream
//     joins it back into st before returning (CallGuard::join, also on its error paths);
//   * uncached status memory (hipExtMallocWithFlags) has no stream-ordered free: st is
//     synchronized and hipFree releases it (hipFree synchronizes the device, as HIP documents it;
//     status arrays grow only with the batch's block or segment count).
// Round 5 zeroed with hipMemset + hipDeviceSynchronize, which stalled every context and stream of
// the device whenever any context grew (ADVICE / VERDICT round 5).
struct DevBufBase {
  void* mem = nullptr;
  uint64_t cap = 0;    // elements the buffer holds (0: none)
  uint64_t bytes = 0;  // its size
  const bool status;   // uncached status memory (kStatusFlags)
  DevBufBase* next;
  DevBufBase(DevBufBase*& chain, bool status_) : status(status_), next(chain) { chain = this; }
  DevBufBase(const DevBufBase&) = delete;  // (a copy would not be on the chain)
  ~DevBufBase() { release(); }
  // Room for `need` elements of `elem` bytes (capacity need + need / 4 + 1024 when it grows).
  // *fresh is set when the memory is new (and so all zero); it is never cleared.
  int grow_bytes(hipStream_t st, uint64_t need, uint64_t elem, bool* fresh) {
    if (need <= cap) return LSMBLK_OK;
    const uint64_t nc = need + need / 4 + 1024, nb = nc * elem;
    if (mem) {
      if (status) {
        if (hipStreamSynchronize(st) != hipSuccess) return LSMBLK_E_HIP;
        (void)hipFree(mem);
      } else if (hipFreeAsync(mem, st) != hipSuccess) {
        return LSMBLK_E_HIP;
      }
      mem = nullptr;
      cap = bytes = 0;
    }
    const hipError_t e = status ? hipExtMallocWithFlags(&mem, nb, kStatusFlags) : hipMallocAsync(&mem, nb, st);
    if (e != hipSuccess) {
      mem = nullptr;
      return LSMBLK_E_NOMEM;
    }
    if (fresh) *fresh = true;
    if (hipMemsetAsync(mem, 0, nb, st) != hipSuccess) return LSMBLK_E_HIP;
    cap = nc;
    bytes = nb;
    return LSMBLK_OK;
  }
  // The whole buffer zeroed on st (nothing when there is none).
  bool zero(hipStream_t st) const { return !bytes || hipMemsetAsync(mem, 0, bytes, st) == hipSuccess; }
  // At context destruction (the device is synchronized by then; pool frees go to the null stream).
  void release() {
    if (!mem) return;
    if (status) (void)hipFree(mem);
    else (void)hipFreeAsync(mem, nullptr);
    mem = nullptr;
    cap = bytes = 0;
  }
};
template <typename T>
struct DevBuf : DevBufBase {
  using DevBufBase::DevBufBase;
  T* get() const { return static_cast<T*>(mem); }
  operator T*() const { return get(); }
  // `need` elements of `per` T each
  int grow(hipStream_t st, uint64_t need, uint64_t per, bool* fresh = nullptr) {
    return grow_bytes(st, need, per * sizeof(T), fresh);
  }
};

struct lsmblk_ctx {
  int device = 0;
  std::mutex mu;
  DevBufBase* bufs = nullptr;    // every DevBuf below
  uint32_t* counters = nullptr;  // [0] decode ticket, [1] plan ticket, [2] emit big-block count
  DevBuf<uint32_t> dec_agg{bufs, false};   // (entries, key bytes, value bytes) per block
  void* crc_tabs = nullptr;      // CrcTabs: CRC-32 slicing + zero-extension tables (first CRC call)
  DevBuf<uint64_t> tile_sum{bufs, false};  // 3 per 64-block tile
  DevBuf<uint64_t> tile_pre{bufs, false};
  DevBuf<uint64_t> seg_agg{bufs, true};    // 2 granules per segment
  DevBuf<uint64_t> seg_inc{bufs, true};
  DevBuf<uint32_t> rec_first{bufs, false}; // n+1
  DevBuf<uint32_t> blk_first{bufs, false};
  DevBuf<uint32_t> ent{bufs, false};       // per (segment-local) block: its encoded size (plan walk)
  DevBuf<uint32_t> big_list{bufs, false};  // n+1 u32: emit_big_kernel's per-block flags (bytes)
  DevBuf<uint32_t> blk_sz{bufs, false};    // n+1: every block's size (per-segment slot output)
  // fused walk + emit (encode_fused_kernel): 4 uncached granules per block record, R(w, i) < n +
  // walkers; per walker its block count (uncached granule, and plain); per record a big-block flag
  DevBuf<uint64_t> frec{bufs, true};
  DevBuf<uint64_t> fdone{bufs, true};
  DevBuf<uint32_t> fwnb{bufs, false};
  DevBuf<uint8_t> fbig{bufs, false};
  bool fuse_on = false;          // diagnostics: slot output through encode_fused_kernel (A/B)
  bool plan_pipe = false;        // the plan walk's helper pipelined over chunks (LSMBLK_DEBUG_PLAN_PIPE, A/B)
  uint32_t emit_mode = 0;        // LSMBLK_DEBUG_EMIT_MODE: 0 default, 1 emit_kernel, 2 emit_block_kernel (A/B)
  uint32_t emit_grid = 0;        // emit_block_kernel's grid clamp (0: kEmitGridMax; tests reach its block loop)
  DevBuf<uint64_t> lag_gran{bufs, true};   // lagged decode granules: 3 aggregate + 3 base per block,
  uint64_t lag_blk_cap = 0;      //   then 3 aggregate + 3 inclusive per 64-block tile; blocks covered
  uint32_t rot_poison = 0;       // diagnostics builds only: LSMBLK_DEBUG_ROT_POISON
  uint32_t emit_poison = 0;      // diagnostics builds only: LSMBLK_DEBUG_EMIT_POISON
  bool dec_two_pass = false;     // diagnostics: count + scan + decode instead of the lagged decode (A/B)
  uint32_t dec_lag = kDecLagDefault;  // blocks the lagged decode's counts run ahead of its decodes, at most;
  uint64_t dec_lag_bytes = kDecLagBytesDefault;  // that many bytes of blocks at the mean block size (0: exactly dec_lag)
  uint64_t* dbg = nullptr;       // debug cycle counters (LSMBLK_DEBUG_COUNTERS), 16 words
  bool dbg_on = false;
  uint32_t epoch = 0;            // 1..16383; 0 = status arrays need clearing
  uint32_t poll = 0;             // look-back poll protocol (see gload)
  uint32_t skip = 0;             // ablation mask (diagnostics builds only: kDiag)
  bool timing = false;           // dispatch start / stop events on every kernel launch (diagnostics)
  // kernel log (timing on): a ring of launches with their dispatch events; slot = the
  // lsmblk_ctx_kernel_times entry the launch counts towards (-1: none)
  struct KLog {
    const char* name;
    int slot;
    hipEvent_t e0, e1;
  };
  std::vector<KLog> klog;        // kKLogCap entries once timing is first switched on
  uint64_t klog_n = 0;           // launches logged since the last lsmblk_ctx_kernel_log
  uint64_t klog_total = 0;       // launches logged since timing was switched on
  uint64_t dec_log0 = 0, dec_log1 = 0, enc_log0 = 0, enc_log1 = 0;  // klog_total range of the last decode / encode
  // BlockMeta sections (lsmblk_block_meta_batch)
  DevBuf<uint32_t> meta_rec{bufs, false};   // nblk
  DevBuf<uint64_t> meta_pos{bufs, false};   // nblk + 1
  DevBuf<uint64_t> meta_tile{bufs, false};  // 2 per tile: sums, prefixes
  DevBuf<uint32_t> meta_crc{bufs, false};   // nseg
  uint64_t* meta_cstats = nullptr;  // crc_kernel stats of the section CRC pass
  // compaction filter (lsmblk_compact_filter_batch)
  DevBuf<uint32_t> filt_keep{bufs, false};  // n
  DevBuf<uint64_t> filt_tile{bufs, false};  // 6 per tile: sums, prefixes
  // merge / compaction pipeline (lsmblk_compact.hip): one arena, carved per call
  DevBuf<uint8_t> cws{bufs, false};
  // CRC-verified decode (lsmblk_decode_batch_ex): per-block CRCs
  DevBuf<uint32_t> vcrc{bufs, false};
  // lsmblk_compact_batch: a second stream for the SST rotation beside the kept stream's byte
  // gather, and the fork / join events (created on first use)
  hipStream_t aux = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  // SST files (lsmblk_sst.hip)
  DevBuf<uint8_t> sws{bufs, false};
  // range scans (lsmblk_sst_scan_batch): the work units a batch's blocks are spread over beyond
  // one per range (LSMBLK_DEBUG_SCAN_UNITS); the workspace is carved from sws
  uint32_t scan_units = kScanUnitsDefault;
  // key-range shard rotation (lsmblk_shard_*): its own arena, carved from the parameters of the
  // last lsmblk_shard_rotation_prepare, which the carry and encode calls replay
  DevBuf<uint8_t> rws{bufs, false};
  uint64_t shard_n = 0, shard_m = 0, shard_target = 0;
  uint32_t shard_block_size = 0, shard_flags = 0, shard_sst_cap = 0;
  bool shard_ready = false;
};

// The context whose ABI call is running on this thread (set by DeviceGuard under the context's
// lock): every kernel launch of the call goes through lsm_launch, which logs it when the
// context's kernel timing is on.
inline thread_local lsmblk_ctx* tl_launch_ctx = nullptr;
constexpr uint32_t kKLogCap = 16384;

namespace {
// Make `dev` current for one ABI call and restore the caller's device afterwards: the library
// never changes which device the calling thread's later allocations land on.
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  lsmblk_ctx* prev_ctx = nullptr;
  explicit DeviceGuard(int dev, lsmblk_ctx* c = nullptr) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = prev == dev || hipSetDevice(dev) == hipSuccess;
    prev_ctx = tl_launch_ctx;
    tl_launch_ctx = c;
  }
  ~DeviceGuard() {
    tl_launch_ctx = prev_ctx;
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// The compute units of the context's device, as the runtime reports them (256 when it cannot say).
inline int cu_count(const lsmblk_ctx* c) {
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
  return cus;
}

// The next kernel-log entry of c (events created on first use of a ring slot), nullptr when
// events cannot be created (the launch then runs untimed).
inline lsmblk_ctx::KLog* klog_next(lsmblk_ctx* c, const char* name, int slot) {
  if (c->klog.size() != kKLogCap) c->klog.assign(kKLogCap, lsmblk_ctx::KLog{nullptr, -1, nullptr, nullptr});
  lsmblk_ctx::KLog& e = c->klog[c->klog_total % kKLogCap];
  if (!e.e0 && hipEventCreate(&e.e0) != hipSuccess) return nullptr;
  if (!e.e1 && hipEventCreate(&e.e1) != hipSuccess) return nullptr;
  e.name = name;
  e.slot = slot;
  ++c->klog_n;
  ++c->klog_total;
  return &e;
}

// The launches of one ABI call (kernel log indices [*a, *b)), for lsmblk_ctx_kernel_times.
struct KLogRange {
  lsmblk_ctx* c;
  uint64_t* b;
  KLogRange(lsmblk_ctx* c_, uint64_t* a_, uint64_t* b_) : c(c_), b(b_) { *a_ = *b_ = c->klog_total; }
  ~KLogRange() { *b = c->klog_total; }
  KLogRange(const KLogRange&) = delete;
  KLogRange& operator=(const KLogRange&) = delete;
};

// Every kernel launch of the library: with the running call's context timing on, the dispatch
// itself fills the log entry's start / stop events (hipExtLaunchKernelGGL) -- the kernel's own
// begin and end, as rocprofv3 reports them (event markers recorded between launches added ~8 %).
template <typename K, typename... Args>
inline void lsm_launch(const char* name, int slot, K kern, dim3 grid, dim3 block, uint32_t shmem, hipStream_t st,
                       Args... args) {
  lsmblk_ctx* c = tl_launch_ctx;
  lsmblk_ctx::KLog* e = c && c->timing ? klog_next(c, name, slot) : nullptr;
  if (e)
    hipExtLaunchKernelGGL(kern, grid, block, shmem, st, e->e0, e->e1, 0, args...);
  else
    hipLaunchKernelGGL(kern, grid, block, shmem, st, args...);
}
}  // namespace
#define LSM_LAUNCH(kern, grid, block, shmem, st, ...) lsm_launch(#kern, -1, kern, grid, block, shmem, st, __VA_ARGS__)
#define LSM_LAUNCH_SLOT(slot, kern, grid, block, shmem, st, ...) \
  lsm_launch(#kern, slot, kern, grid, block, shmem, st, __VA_ARGS__)
// A kernel template with several arguments: #kern would stop at the first comma of its argument
// list, so the log name is given explicitly.
#define LSM_LAUNCH_NAMED(name, kern, grid, block, shmem, st, ...) lsm_launch(name, -1, kern, grid, block, shmem, st, __VA_ARGS__)

// Internal entry points shared between translation units (called with ctx->mu held).
namespace lsmblk_impl {
// lsmblk_encode_batch_ex's arguments, with optional device-side entry count (dn) and segment
// count (dnseg): in->n and nseg are then upper bounds that size the grids and the workspace.
// span: the segments cover [seg_start[0], seg_start[nseg]) of the stream (a key-range shard's part
// of a stream that also holds the previous rank's crossing block and the halo), not all of it.
struct EncodeReq {
  hipStream_t st = nullptr;
  const lsmblk_kv_stream* in = nullptr;
  const uint64_t* dn = nullptr;
  const uint32_t* seg_start = nullptr;
  const uint32_t* dnseg = nullptr;
  uint32_t nseg = 0;
  uint32_t block_size = 0;
  uint8_t* out = nullptr;
  uint64_t out_cap = 0;
  uint64_t* blk_off = nullptr;
  uint64_t blk_cap = 0;
  uint64_t* stats = nullptr;
  bool span = false;
  uint32_t flags = 0;
  uint64_t* seg_out = nullptr;
};
int encode_locked(lsmblk_ctx* c, const EncodeReq& q);
// lsmblk_encode_segment_blocks for the encode that just ran on this context.
int segment_blocks_locked(lsmblk_ctx* c, const uint32_t* seg_start, uint32_t nseg_max, const uint64_t* enc_stats,
                          uint32_t* seg_blk, hipStream_t st);
// CRC tables on the context (first use) and the CRC launch over [blk_off[b], blk_off[b+1] - tail):
// crc_stream_kernel, or crc_kernel<true> when agg takes the per-block counts as well, or
// crc_kernel<false> for a few long ranges (sections: a wave per range, its 4 KiB chunks one after
// another, keeps more waves busy than a 16-lane row per range).
int ensure_crc_tabs(lsmblk_ctx* c, hipStream_t st);
// The context's second stream and its fork / join events (created on first use): work launched
// on c->aux after fork_aux(c, st) runs beside st; join_aux(c, st) makes st wait for it.
int fork_aux(lsmblk_ctx* c, hipStream_t st);
int join_aux(lsmblk_ctx* c, hipStream_t st);
int launch_crc(lsmblk_ctx* c, const uint8_t* blocks, const uint64_t* blk_off, uint64_t nblk, uint32_t tail,
               uint32_t* crc, uint64_t* stats, hipStream_t st, uint32_t* agg = nullptr, bool sections = false);
// LSMBLK_ENCODE_FRAMED: every block's CRC written big-endian after it (the encode's block table;
// its count read on the device from stats[0], nothing after an encode error).
int launch_crc_frames(lsmblk_ctx* c, uint8_t* out, const uint64_t* blk_off, const uint32_t* blk_sz,
                      uint64_t nblk_max, uint64_t* stats, hipStream_t st);
// lsmblk_block_meta_batch with the context lock held.
int block_meta_locked(lsmblk_ctx* c, const uint8_t* blocks, const uint64_t* blk_off, uint64_t nblk, uint32_t tail,
                      const uint32_t* seg_blk, uint32_t nseg, uint8_t* meta, uint64_t meta_cap, uint64_t* meta_off,
                      uint64_t* stats, hipStream_t st);
}  // namespace lsmblk_impl

// ---------------------------------------------------------------- host: what the entry points share
namespace {
// A call's epilogue: whether every launch since the last look was accepted.
inline int launch_rc() { return hipGetLastError() == hipSuccess ? LSMBLK_OK : LSMBLK_E_HIP; }

// A call's prologue: the context's lock, its device made current, the caller's stream, the stats
// words (when given) zeroed on it.  rc != 0: the call returns it.  The arguments are validated
// before the guard is built, which dereferences c.  A call that forks onto the context's second
// stream does so through fork(): whatever path it then returns by, the caller's stream has waited
// for the work queued there (join(), at the latest when the guard goes).
struct CallGuard {
  std::lock_guard<std::mutex> lock;
  DeviceGuard dg;
  lsmblk_ctx* const c;
  hipStream_t st;
  int rc;
  bool forked = false;
  CallGuard(lsmblk_ctx* c_, void* stream, uint64_t* stats = nullptr, uint32_t words = 0)
      : lock(c_->mu), dg(c_->device, c_), c(c_), st(reinterpret_cast<hipStream_t>(stream)),
        rc(dg.ok && (!stats || !words || hipMemsetAsync(stats, 0, words * 8, st) == hipSuccess) ? LSMBLK_OK
                                                                                                  : LSMBLK_E_HIP) {}
  ~CallGuard() { (void)join(); }
  int fork() {
    const int r = lsmblk_impl::fork_aux(c, st);
    forked = r == LSMBLK_OK;
    return r;
  }
  int join() {
    if (!forked) return LSMBLK_OK;
    forked = false;
    return lsmblk_impl::join_aux(c, st);
  }
};

// Workspace regions of an arena one after another, each rounded up to 256 bytes; off: their total.
// A layout is a function of a Carve, run with a null base to measure and again on the arena to bind.
struct Carve {
  uint8_t* base;
  uint64_t off = 0;
  Carve(uint8_t* b, uint64_t o = 0) : base(b), off(o) {}
  template <typename T>
  T* take(uint64_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off = (off + count * sizeof(T) + 255) & ~uint64_t(255);
    return p;
  }
};

// Workgroups of `kern` (at `threads` threads, no dynamic LDS) resident at once on a device of `cus`
// compute units, `per_cu` a CU when the runtime cannot say: the grid of a persistent kernel.
template <typename K>
inline uint32_t resident_wgs(int cus, K kern, int threads, int per_cu) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, threads, 0) != hipSuccess || n < 1) n = per_cu;
  return uint32_t(cus > 0 ? cus : 256) * uint32_t(n);
}
}  // namespace
