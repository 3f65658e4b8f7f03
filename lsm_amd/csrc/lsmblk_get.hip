// lsmblk_get.hip -- batched SST point lookups of the batch C ABI (include/lsmblk.h), gfx950
// (key_within -> bloom.may_contain -> find_block_idx -> read_block ->
// BlockIterator::create_and_seek_to_key -> the visible version and its value):
//
//   lsmblk_sst_open_batch   SsTable::open (src/table.rs:162-186) for SST files resident in device
//                           memory: footers, section CRCs, BlockMeta walk -> descriptors + block index
//     sst_open_prep_kernel  one workgroup: footers of every SST range-checked, index slots reserved
//                           (exclusive scan of the claimed block counts), the CRC range table
//     crc_kernel<false>     the bloom and BlockMeta section CRCs (launch_crc, sections)
//     sst_open_walk_kernel  one workgroup per SST: CRCs compared, the BlockMeta records walked over
//                           chunks staged into LDS -> index records and the descriptor
//   lsmblk_sst_get_batch    the lookups
//     sst_get_kernel        one wave per lookup, grid-strided: key range, bloom probes from k lanes
//                           at once, k-ary block search over the first-key images, the landed block
//                           staged into LDS with 16-B loads, every entry compared by its own lane
//                           (equal range [L, U)), the reference's probe sequence replayed on L / U,
//                           the version walk
//     val_scan_kernel       value sizes of the FOUND lookups -> val_off (one workgroup)
//     val_gather_kernel     one wave per FOUND lookup copies its value
#include "lsmblk_dev.hpp"

namespace {

// A block of up to kGetLdsBlock bytes is staged into its wave's LDS image (one round trip of 16-B
// loads); a larger one (block_size > 4096, or one oversized entry) is read from global memory.
// 4098: BlockBuilder::add's size estimate counts an entry (2 - prefix) bytes short, so block_size
// 4096 yields blocks of up to 4098 bytes.  4 waves x (kGetLdsBlock + 32) B = 16.1 KiB per workgroup:
// 9 workgroups of a CU's 160 KiB, so LDS never caps the 8 waves per SIMD.
constexpr uint32_t kGetLdsBlock = 4098;
constexpr uint32_t kGetImg = kGetLdsBlock + 32;  // lead < 16 before the block, slack for 4-B reads after
constexpr uint32_t kGetWaves = 4;
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t be32_at(const uint8_t* p) {
  return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3];
}

// ---------------------------------------------------------------- open
constexpr uint32_t kOpenChunk = 8192;  // BlockMeta bytes staged per LDS window
constexpr uint32_t kMetaRecMin = 24;   // u32 offset | u16 | key | u64 | u16 | key | u64 with empty keys

struct OpenArgs {
  const uint8_t* files;
  const uint64_t* file_off;
  uint32_t nsst;
  lsmblk_sst_desc* desc;
  lsmblk_sst_index* index;
  uint64_t index_cap;
  uint64_t* tab;        // 4 nsst + 1: CRC ranges, SSTs in reverse order
  const uint32_t* crc;  // 4 nsst
  uint64_t* stats;
};

// Footers, range checks, slot reservation.  The CRC range table holds per SST, in REVERSE SST order,
// [BlockMeta body start, its CRC, bloom start, its CRC] (absolute): range 4r is the BlockMeta body,
// 4r + 2 the bloom filter | k; range 4r + 1 is the 8 bytes between the sections and range 4r + 3
// decreases (the next entry belongs to the file before), which the CRC pass skips.  A failed SST's
// four entries are its file's start: empty ranges.
__global__ __launch_bounds__(1024) void sst_open_prep_kernel(OpenArgs a) {
  const uint32_t t = threadIdx.x, w = t >> 6;
  __shared__ uint64_t wsum[16];
  int tb = 0;
  for (uint32_t s = t; s < a.nsst; s += 1024) tb |= a.file_off[s + 1] < a.file_off[s];
  const bool tbad = __syncthreads_or(tb) != 0;
  uint64_t carry = 0;
  for (uint32_t r = 0; r < a.nsst; r += 1024) {
    const uint32_t s = r + t;
    uint64_t cnt = 0;
    if (s < a.nsst) {
      const uint64_t fo = tbad ? 0 : a.file_off[s], flen = tbad ? 0 : a.file_off[s + 1] - fo;
      const uint8_t* F = a.files + fo;
      lsmblk_sst_desc d;
      memset(&d, 0, sizeof(d));
      uint64_t bo = 0, mo = 0;
      // file = data | meta (>= 16) | u32 meta_offset | filter | k | u32 crc | u32 bloom_offset
      bool ok = flen >= 16 + 4 + 5 + 4;
      if (ok) {
        bo = be32_at(F + flen - 4);
        ok = bo >= 20 && bo + 5 <= flen - 4 && flen - 4 - bo <= 0x7FFFFFF0ull;
      }
      if (ok) {
        mo = be32_at(F + bo - 4);
        ok = mo + 16 <= bo - 4 && bo - 4 - mo <= 0x7FFFFFF0ull;
      }
      uint32_t num = 0;
      if (ok) {
        num = be32_at(F + mo);
        ok = num >= 1 && uint64_t(num) * kMetaRecMin + 16 <= bo - 4 - mo;
      }
      if (ok) {
        cnt = num;
        d.meta_offset = uint32_t(mo);
        d.bloom_len = uint32_t(flen - 4 - bo - 5);
        d.bloom_pos = fo + bo;
        d.bloom_k = F[flen - 9];
      } else {
        d.err = LSMBLK_ERR_MALFORMED;
      }
      a.desc[s] = d;
      uint64_t* e = a.tab + 4ull * (a.nsst - 1 - s);
      e[0] = ok ? fo + mo + 4 : fo;
      e[1] = ok ? fo + bo - 8 : fo;
      e[2] = ok ? fo + bo : fo;
      e[3] = ok ? fo + flen - 8 : fo;
      if (s == 0) a.tab[4ull * a.nsst] = e[3];  // an empty last range
    }
    const uint64_t inc = wave_incl_scan<uint64_t>(cnt);
    if (lane_id() == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t base = carry, tot = carry;
    for (uint32_t x = 0; x < 16; ++x) {
      if (x < w) base += wsum[x];
      tot += wsum[x];
    }
    if (s < a.nsst) a.desc[s].blk0 = uint32_t(base + inc - cnt);
    carry = tot;
    __syncthreads();
  }
  if (t == 0) {
    uint32_t e = tbad ? LSMBLK_ERR_MALFORMED : 0u;
    a.stats[1] = carry;
    if (carry > 0xFFFFFFFFull) e |= LSMBLK_ERR_OVERFLOW;
    if (carry > a.index_cap) e |= LSMBLK_ERR_CAPACITY;
    if (e) atomicOr(reinterpret_cast<unsigned long long*>(a.stats + 3), (unsigned long long)e);
  }
}

// One workgroup (one wave) per SST.  The BlockMeta records are variable-length, so the walk is
// serial; it runs over an LDS window of kOpenChunk bytes that all lanes refill together (16-B loads)
// whenever a field lies outside it -- every lane walks the same positions, lane 0 writes.
__global__ __launch_bounds__(64) void sst_open_walk_kernel(OpenArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kOpenChunk];
  if (a.stats[3]) return;
  const uint32_t s = blockIdx.x, l = threadIdx.x;
  lsmblk_sst_desc d = a.desc[s];
  if (d.err) {
    if (l == 0) atomicOr(reinterpret_cast<unsigned long long*>(a.stats + 2), (unsigned long long)d.err);
    return;
  }
  const uint64_t fo = a.file_off[s], fend = a.file_off[s + 1];
  const uint8_t* F = a.files + fo;
  const uint64_t mo = d.meta_offset, bo = d.bloom_pos - fo;
  const uint32_t r = a.nsst - 1 - s;
  uint32_t err = 0;
  if (be32_at(F + bo - 8) != a.crc[4 * r] || be32_at(F + (fend - fo) - 8) != a.crc[4 * r + 2]) err = LSMBLK_ERR_CHECKSUM;
  const uint32_t num = be32_at(F + mo);
  const uint64_t rec_end = bo - 16;  // the records end where max_ts starts
  uint64_t wbase = ~0ull;            // absolute, 16-B aligned; no window yet
  // bytes [p, p + nb) of the file (nb <= 16) inside the window; p + nb <= bo - 4 by the callers' checks
  auto need = [&](uint64_t p, uint32_t nb) -> const uint8_t* {
    const uint64_t ap = fo + p;
    if (wbase == ~0ull || ap < wbase || ap + nb > wbase + kOpenChunk) {
      __syncthreads();
      wbase = ap & ~15ull;
      u32x4 q[kOpenChunk / 1024];
#pragma unroll
      for (uint32_t i = 0; i < kOpenChunk / 1024; ++i) {
        const uint64_t x = wbase + 16ull * (l + 64 * i);
        q[i] = u32x4{0, 0, 0, 0};
        if (x + 16 <= fend) {
          q[i] = *reinterpret_cast<const u32x4*>(a.files + x);
        } else if (x < fend) {  // the file's last, partial piece: never read past the file
          uint8_t* qb = reinterpret_cast<uint8_t*>(&q[i]);
          for (uint64_t y = x; y < fend; ++y) qb[y - x] = a.files[y];
        }
      }
#pragma unroll
      for (uint32_t i = 0; i < kOpenChunk / 1024; ++i) *reinterpret_cast<u32x4*>(win + 16 * (l + 64 * i)) = q[i];
      __syncthreads();
    }
    return win + (ap - wbase);
  };
  auto be16w = [&](uint64_t p) {
    const uint8_t* b = need(p, 2);
    return uni((uint32_t(b[0]) << 8) | b[1]);
  };
  lsmblk_sst_index* const ix = a.index + d.blk0;
  uint64_t pos = mo + 4, prev_off = 0, fk_pos = 0, lk_pos = 0;
  uint32_t fk_len = 0, lk_len = 0;
  bool bad = false;
  for (uint32_t i = 0; i < num && !bad; ++i) {
    if (pos + 6 > rec_end) {
      bad = true;
      break;
    }
    const uint8_t* b = need(pos, 6);
    const uint32_t off = uni(be32_at(b)), fl = uni((uint32_t(b[4]) << 8) | b[5]);
    const uint64_t kpos = pos + 6;
    if (kpos + fl + 8 + 2 > rec_end) {
      bad = true;
      break;
    }
    uint64_t hi = 0, lo = 0;
    if (fl) {
      const uint32_t m = fl < 16 ? fl : 16;
      const uint8_t* k = need(kpos, m);
      for (uint32_t j = 0; j < m; ++j) {
        if (j < 8) hi |= uint64_t(k[j]) << (56 - 8 * j);
        else lo |= uint64_t(k[j]) << (56 - 8 * (j - 8));
      }
    }
    const uint32_t ll = be16w(kpos + fl + 8);
    const uint64_t lpos = kpos + fl + 8 + 2;
    if (lpos + ll + 8 > rec_end) {
      bad = true;
      break;
    }
    // a framed block is at least its u16 entry count and the u32 CRC, inside the data section
    if ((i && off < prev_off + 6) || uint64_t(off) + 6 > mo) {
      bad = true;
      break;
    }
    if (l == 0) {
      lsmblk_sst_index rec;
      rec.img_hi = hi;
      rec.img_lo = lo;
      rec.off = off;
      rec.end = uint32_t(mo);  // the last block ends at the meta section; patched by the next record
      rec.key_pos = uint32_t(kpos);
      rec.key_len = fl;
      ix[i] = rec;
      if (i) ix[i - 1].end = off;
    }
    if (i == 0) {
      fk_pos = kpos;
      fk_len = fl;
    }
    lk_pos = lpos;
    lk_len = ll;
    prev_off = off;
    pos = lpos + ll + 8;
  }
  if (!bad && pos != rec_end) bad = true;
  if (bad) err |= LSMBLK_ERR_MALFORMED;
  if (l == 0) {
    if (!err) {
      d.nblk = num;
      d.first_key_pos = fo + fk_pos;
      d.first_key_len = fk_len;
      d.last_key_pos = fo + lk_pos;
      d.last_key_len = lk_len;
      uint64_t mt = 0;
      for (uint32_t j = 0; j < 8; ++j) mt = (mt << 8) | F[rec_end + j];
      d.max_ts = mt;
      atomicAdd(reinterpret_cast<unsigned long long*>(a.stats), 1ull);
    } else {
      atomicOr(reinterpret_cast<unsigned long long*>(a.stats + 2), (unsigned long long)err);
    }
    d.err = err;
    a.desc[s] = d;
  }
}

// ---------------------------------------------------------------- get
struct GetArgs {
  const uint8_t* files;
  const uint64_t* file_off;
  uint32_t nsst;
  const lsmblk_sst_desc* desc;
  const lsmblk_sst_index* index;
  const uint32_t* q_sst;
  const uint8_t* qkeys;
  const uint32_t* qkey_off;
  const uint64_t* q_ts;
  uint64_t nq;
  uint32_t flags;
  lsmblk_get_result* res;
  uint8_t* vals;
  uint64_t val_cap;
  uint32_t* val_off;
  uint64_t* stats;
};

// The query key through a bounds-checked descriptor over the arena up to the key's end (rounded up
// to the aligned dword that holds its last byte): aligned dword loads, past the bound they read 0.
struct QKey {
  rsrc_t r;
  uint32_t x;  // descriptor byte of the key's first byte
  uint32_t len;
  __device__ __forceinline__ uint32_t fetch(uint32_t i) const {
    const uint32_t y = x + i, al = y & ~3u;
    return __builtin_amdgcn_alignbyte(__builtin_amdgcn_raw_buffer_load_b32(r, al + 4, 0, 0),
                                      __builtin_amdgcn_raw_buffer_load_b32(r, al, 0, 0), y & 3);
  }
  __device__ __forceinline__ uint32_t byte(uint32_t i) const { return __builtin_amdgcn_raw_buffer_load_b8(r, x + i, 0, 0); }
};

// key order of the first nv (1..4) bytes of two little-endian dword loads
__device__ __forceinline__ int cmp_dw(uint32_t x, uint32_t y, uint32_t nv) {
  const uint32_t m = nv >= 4 ? ~0u : ~(~0u >> (8 * nv));
  x = __builtin_bswap32(x) & m;
  y = __builtin_bswap32(y) & m;
  return x < y ? -1 : (x > y ? 1 : 0);
}

// Key order of the bytes fa(0 .. la) against the query, by the whole wave (64 bytes a round, a byte
// per lane); lcp = their common prefix.  Every lane returns the same values.
template <class FA>
__device__ __forceinline__ int wave_cmp(FA fa, uint32_t la, const QKey& q, uint32_t& lcp) {
  const uint32_t l = lane_id(), mn = la < q.len ? la : q.len;
  for (uint32_t base = 0; base < mn; base += 64) {
    const uint32_t i = base + l;
    uint32_t x = 0, y = 0;
    if (i < mn) {
      x = fa(i);
      y = q.byte(i);
    }
    const uint64_t dm = __ballot(x != y);
    if (dm) {
      const uint32_t j = uint32_t(__builtin_ctzll(dm));
      lcp = base + j;
      return uint32_t(__builtin_amdgcn_readlane(x, j)) < uint32_t(__builtin_amdgcn_readlane(y, j)) ? -1 : 1;
    }
  }
  lcp = mn;
  return la < q.len ? -1 : (la > q.len ? 1 : 0);
}

// Key order of file bytes p[0 .. la) against the query by one lane (the block search's fallback
// among equal first-key images).
__device__ int lane_cmp(const uint8_t* p, uint32_t la, const QKey& q) {
  const uint32_t mn = la < q.len ? la : q.len;
  for (uint32_t i = 0; i < mn; ++i) {
    const uint32_t x = p[i], y = q.byte(i);
    if (x != y) return x < y ? -1 : 1;
  }
  return la < q.len ? -1 : (la > q.len ? 1 : 0);
}

// First index of [lo, hi) where pred turns false (hi: nowhere), pred true on a prefix of the range:
// 64 probes a step, one per lane, so a step cuts the range 65-fold for one round trip.
template <class Pred>
__device__ __forceinline__ uint32_t kary_first_false(uint32_t lo, uint32_t hi, Pred pred) {
  const uint32_t l = lane_id();
  while (hi - lo > 64) {
    const uint32_t stride = (hi - lo + 63) / 64;
    const uint32_t idx = lo + (l + 1) * stride - 1;  // < 2^32: hi - lo + 64 * stride stays far below
    const bool p = idx < hi && pred(idx);
    const uint32_t cnt = uint32_t(__builtin_popcountll(__ballot(p)));
    const uint32_t nhi = lo + (cnt + 1) * stride - 1;  // the first false probe (or past the range)
    lo = uni(lo + cnt * stride);
    hi = uni(nhi < hi ? nhi : hi);
  }
  const uint32_t idx = lo + l;
  const bool p = idx < hi && pred(idx);
  return uni(lo + uint32_t(__builtin_popcountll(__ballot(p))));
}

struct BlkHdr {
  uint32_t n, data_end, fks;
  bool ok;
};
// Block::decode's header with seek_kernel's checks (lsmblk_sst.hip).
template <class Img>
__device__ __forceinline__ BlkHdr get_hdr(const Img& im, uint32_t len) {
  BlkHdr h{0, 0, 0, false};
  if (len < 2) return h;
  h.n = uni(im.u16(len - 2));
  if (2 + 2 * h.n > len) return h;
  h.data_end = len - 2 - 2 * h.n;
  if (h.n) {
    if (h.data_end < 4) return h;
    h.fks = uni(im.u16(2));
    if (4 + h.fks + 8 > h.data_end) return h;
  }
  h.ok = true;
  return h;
}

// What one visited block decides.
struct Visit {
  bool done;      // the lookup is answered (else: go on with the next block)
  bool bad;       // the block breaks the decode rules
};

struct Look {     // a lookup's state across the blocks it visits (wave-uniform)
  uint32_t status, blk, ent, hit_blk, hit_ent, vlen;
  uint64_t ts, val_pos;
  bool landed;
};

// Block b of the SST (len bytes at absolute position bpos, read through im): `first` = the block the
// block search chose, else a block the iterator moved on to (its entry 0 is the next entry).
//   every lane compares its own entries with the query: L = entries below it, U = entries not above
//   it, so [L, U) is the equal range (the block is sorted);
//   first block: the landing is L (MVCC) or what the reference's binary search reaches, replayed
//   on L / U without touching memory (mid < L: less, mid >= U: greater, else equal and it stops);
//   then the first version of [landing, U) with ts <= read_ts.
template <class Img>
__device__ Visit visit_block(const Img& im, uint32_t len, uint64_t bpos, uint32_t b, bool first, bool mvcc,
                             const QKey& q, uint64_t read_ts, Look& k) {
  const uint32_t l = lane_id();
  const BlkHdr h = get_hdr(im, len);
  if (!h.ok) return Visit{true, true};
  // m = lcp(first key, query); an entry that shares more than m bytes with the first key orders
  // against the query as the first key does at byte m, one that shares at most m has its first
  // `prefix` bytes equal to the query's and is decided by its suffix
  uint32_t m = 0;
  int cfk = 0;
  if (h.n) cfk = wave_cmp([&](uint32_t i) { return im.u8(4 + i); }, h.fks, q, m);
  const int cbeyond = m == q.len ? 1 : cfk;
  uint32_t L = 0, U = 0;
  bool bad = false;
  for (uint32_t c = 0; c < h.n; c += 64) {
    const uint32_t e = c + l;
    int cm = 1;
    if (e < h.n) {
      const uint32_t off = im.u16(h.data_end + 2 * e);
      bool okk = off + 4 <= h.data_end;
      uint32_t pf = 0, sf = 0;
      if (okk) {
        pf = im.u16(off);
        sf = im.u16(off + 2);
        okk = off + 4 + sf + 10 <= h.data_end && pf <= h.fks && pf + sf > 0;
      }
      if (okk) okk = off + 14 + sf + im.u16(off + 12 + sf) <= h.data_end;
      if (!okk) {
        bad = true;
      } else if (pf > m) {
        cm = cbeyond;
      } else {
        const uint32_t rem = q.len - pf, mm = sf < rem ? sf : rem;
        cm = 0;
        for (uint32_t j = 0; j < mm && !cm; j += 4) cm = cmp_dw(im.le32(off + 4 + j), q.fetch(pf + j), mm - j);
        if (!cm) cm = sf < rem ? -1 : (sf > rem ? 1 : 0);
      }
    }
    L += uint32_t(__builtin_popcountll(__ballot(e < h.n && cm < 0)));
    U += uint32_t(__builtin_popcountll(__ballot(e < h.n && cm <= 0)));
  }
  if (__ballot(bad)) return Visit{true, true};
  L = uni(L);
  U = uni(U);
  uint32_t from = 0;  // the walk starts here
  if (first) {
    uint32_t land = L;
    if (!mvcc) {
      uint32_t lo = 0, hi = h.n;
      bool found = false;
      while (lo < hi && !found) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (mid < L) lo = mid + 1;
        else if (mid >= U) hi = mid;
        else {
          land = mid;
          found = true;
        }
      }
      if (!found) land = lo;
    }
    if (land >= h.n) return Visit{false, false};  // the block iterator ended invalid: spill
    k.landed = true;
    k.blk = b;
    k.ent = land;
    if (land < L || land >= U) return Visit{true, false};  // landed on another key
    from = land;
  } else {
    if (!k.landed) {
      k.landed = true;
      k.blk = b;
      k.ent = 0;
    }
    if (h.n == 0) return Visit{false, false};
    if (L != 0 || U == 0) return Visit{true, false};  // entry 0 is another key
  }
  for (uint32_t c = from; c < U; c += 64) {
    const uint32_t e = c + l;
    uint32_t off = 0, sf = 0;
    uint64_t ts = 0;
    bool hit = false;
    if (e < U) {
      off = im.u16(h.data_end + 2 * e);
      sf = im.u16(off + 2);
      ts = im.u64(off + 4 + sf);
      hit = ts <= read_ts;
    }
    const uint64_t hm = __ballot(hit);
    if (hm) {
      const uint32_t j = uint32_t(__builtin_ctzll(hm));
      const uint32_t vl = e < U ? im.u16(off + 12 + sf) : 0u;
      k.hit_blk = b;
      k.hit_ent = c + j;
      k.ts = lane64(ts, j);
      k.vlen = uint32_t(__builtin_amdgcn_readlane(vl, j));
      k.val_pos = bpos + uint32_t(__builtin_amdgcn_readlane(off + 14 + sf, j));
      k.status = k.vlen ? LSMBLK_GET_FOUND : LSMBLK_GET_TOMBSTONE;
      return Visit{true, false};
    }
  }
  // no visible version here: the key's versions may go on in the next block
  return Visit{U < h.n, false};
}

// 8 waves per SIMD (64 VGPRs): a lookup is a chain of dependent reads, so the lookups in flight hide
// each other's round trips; the compiler's free choice was 181 VGPRs (2 waves per SIMD).
__global__ __launch_bounds__(64 * kGetWaves) __attribute__((amdgpu_waves_per_eu(8))) void sst_get_kernel(GetArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t img[kGetWaves][kGetImg];
  const uint32_t l = lane_id();
  uint8_t* const S = img[wave_id()];
  const bool mvcc = (a.flags & LSMBLK_GET_MVCC) != 0, filter = !(a.flags & LSMBLK_GET_NO_FILTER);
  const uint32_t qlead = uint32_t(reinterpret_cast<uintptr_t>(a.qkeys) & 3);
  const uint8_t* const qbase = a.qkeys - qlead;
  uint32_t err = 0, nfound = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.stats[0] = a.nq;
  const uint64_t stride = uint64_t(gridDim.x) * kGetWaves;
  for (uint64_t qi = uint64_t(blockIdx.x) * kGetWaves + wave_id(); qi < a.nq; qi += stride) {
    Look k{LSMBLK_GET_ABSENT, kNone, kNone, kNone, kNone, 0, 0, 0, false};
    do {
      const uint32_t s = uni(a.q_sst[qi]);
      const uint32_t k0 = uni(a.qkey_off[qi]), k1 = uni(a.qkey_off[qi + 1]);
      if (s >= a.nsst) {
        err |= LSMBLK_ERR_SEGMENTS;
        break;
      }
      if (k1 <= k0) {
        err |= LSMBLK_ERR_EMPTY_KEY;
        break;
      }
      const QKey q{make_rsrc_exact(const_cast<uint8_t*>(qbase), (qlead + k1 + 3) & ~3u), qlead + k0, k1 - k0};
      const uint64_t read_ts = uni64(a.q_ts[qi]);
      const lsmblk_sst_desc* dp = a.desc + s;
      const uint32_t blk0 = uni(dp->blk0), nblk = uni(dp->nblk);
      const uint64_t fo = uni64(a.file_off[s]);
      const uint8_t* const F = a.files + fo;
      if (nblk == 0) {  // not opened: the iterator is invalid from the start
        k.blk = 0;
        k.ent = 0;
        break;
      }
      if (filter) {
        // key_within (lsm_storage.rs:136-138): first_key <= key <= last_key
        const uint8_t* fk = a.files + uni64(dp->first_key_pos);
        const uint8_t* lk = a.files + uni64(dp->last_key_pos);
        uint32_t lcp;
        if (wave_cmp([&](uint32_t i) { return uint32_t(fk[i]); }, uni(dp->first_key_len), q, lcp) > 0 ||
            wave_cmp([&](uint32_t i) { return uint32_t(lk[i]); }, uni(dp->last_key_len), q, lcp) < 0) {
          k.status = LSMBLK_GET_RANGE_OUT;
          break;
        }
        // Bloom::may_contain (bloom.rs:104-120): probe i tests bit (h + i delta) % (nbits as u32);
        // the k <= 30 probes are independent: lane i makes probe i, one round trip for all
        const uint32_t bk = uni(dp->bloom_k);
        if (bk <= 30) {
          const uint32_t nbits = uni(dp->bloom_len) * 8u;
          bool pass = false;
          if (nbits) {
            const uint32_t h = fingerprint32(q, q.len), delta = (h >> 17) | (h << 15);
            bool miss = false;
            if (l < bk) {
              const uint32_t bit = (h + l * delta) % nbits;
              miss = !((a.files[uni64(dp->bloom_pos) + (bit >> 3)] >> (bit & 7)) & 1);
            }
            pass = __ballot(miss) == 0;
          }
          if (!pass) {
            k.status = LSMBLK_GET_BLOOM_OUT;
            break;
          }
        }
      }
      // find_block_idx (table.rs:253-257): P = partition_point(first_key <= key) (MVCC: < key) over
      // the first-key images; blocks whose image equals the query's, [iL, iU), compare whole keys
      uint64_t qhi, qlo;
      {
        uint32_t w[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t nv = q.len > 4 * j ? q.len - 4 * j : 0u;
          const uint32_t v = __builtin_bswap32(q.fetch(4 * j));
          w[j] = nv >= 4 ? v : (nv ? v & ~(~0u >> (8 * nv)) : 0u);
        }
        qhi = (uint64_t(w[0]) << 32) | w[1];
        qlo = (uint64_t(w[2]) << 32) | w[3];
      }
      const lsmblk_sst_index* const ix = a.index + blk0;
      const uint32_t iL = kary_first_false(0, nblk, [&](uint32_t i) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ix + i);
        const uint64_t hi = (uint64_t(v.y) << 32) | v.x, lo = (uint64_t(v.w) << 32) | v.z;
        return hi < qhi || (hi == qhi && lo < qlo);
      });
      const uint32_t iU = kary_first_false(iL, nblk, [&](uint32_t i) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ix + i);
        const uint64_t hi = (uint64_t(v.y) << 32) | v.x, lo = (uint64_t(v.w) << 32) | v.z;
        return hi < qhi || (hi == qhi && lo <= qlo);
      });
      uint32_t P = iL;
      if (iU > iL)
        P = kary_first_false(iL, iU, [&](uint32_t i) {
          const int c = lane_cmp(F + ix[i].key_pos, ix[i].key_len, q);
          return mvcc ? c < 0 : c <= 0;
        });
      uint32_t b = P ? P - 1 : 0;
      bool first = true;
      for (;;) {
        if (b >= nblk) {  // the iterator ended invalid
          if (!k.landed) {
            k.blk = nblk;
            k.ent = 0;
          }
          break;
        }
        const uint32_t off = uni(ix[b].off), end = uni(ix[b].end);
        Visit v{true, true};
        if (end >= off + 4 + 2 && uint64_t(end) <= uni(dp->meta_offset)) {
          const uint32_t len = end - off - 4;
          const uint8_t* src = F + off;
          const uint32_t lead = uni(uint32_t(reinterpret_cast<uintptr_t>(src) & 15));
          if (len <= kGetLdsBlock) {
            // the block and up to 15 bytes on either side (inside the file: `files` is 16-B aligned
            // and the block's CRC and the sections follow it) in 16-B pieces, all loads first
            const uint32_t nch = (lead + len + 15) >> 4;
            u32x4 p[(kGetLdsBlock + 15 + 15) / 1024 + 1];
            wave_sync();  // the previous block's reads are done
#pragma unroll
            for (uint32_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i)
              if (l + 64 * i < nch) p[i] = *reinterpret_cast<const u32x4*>(src - lead + 16 * (l + 64 * i));
#pragma unroll
            for (uint32_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i)
              if (l + 64 * i < nch) *reinterpret_cast<u32x4*>(S + 16 * (l + 64 * i)) = p[i];
            wave_sync();
            v = visit_block(LdsImg{S, lead}, len, fo + off, b, first, mvcc, q, read_ts, k);
          } else {
            const rsrc_t R = make_rsrc(reinterpret_cast<const uint8_t*>(uni64(reinterpret_cast<uintptr_t>(src - lead))),
                                       uni(lead + len));
            v = visit_block(GlbImg{R, lead}, len, fo + off, b, first, mvcc, q, read_ts, k);
          }
        }
        if (v.bad) {
          err |= LSMBLK_ERR_MALFORMED;
          k.status = LSMBLK_GET_ABSENT;
          if (!k.landed) {
            k.blk = b;
            k.ent = 0;
          }
        }
        if (v.done) break;
        ++b;
        first = false;
      }
    } while (false);
    if (k.status == LSMBLK_GET_FOUND) ++nfound;
    if (l == 0) {
      lsmblk_get_result r;
      r.status = k.status;
      r.blk = k.blk;
      r.ent = k.ent;
      r.hit_blk = k.hit_blk;
      r.hit_ent = k.hit_ent;
      r.vlen = k.vlen;
      r.ts = k.ts;
      r.val_pos = k.val_pos;
      a.res[qi] = r;
    }
  }
  raise_err(a.stats, err);
  if (nfound && l == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats + 1), (unsigned long long)nfound);
}

// val_off = exclusive scan of the FOUND lookups' value sizes: thread t sums the contiguous share
// [t per, (t + 1) per) of the lookups, the shares are scanned across the workgroup (wave scan, then
// the wave totals), and every thread writes its share's offsets.
__global__ __launch_bounds__(1024) void val_scan_kernel(GetArgs a) {
  __shared__ uint64_t wsum[16];
  const uint32_t t = threadIdx.x, w = t >> 6;
  const uint64_t per = (a.nq + 1023) / 1024;
  const uint64_t q0 = per * t < a.nq ? per * t : a.nq, q1 = q0 + per < a.nq ? q0 + per : a.nq;
  uint64_t sum = 0;
  for (uint64_t q = q0; q < q1; ++q) sum += a.res[q].status == LSMBLK_GET_FOUND ? a.res[q].vlen : 0u;
  const uint64_t inc = wave_incl_scan<uint64_t>(sum);
  if (lane_id() == 63) wsum[w] = inc;
  __syncthreads();
  uint64_t base = 0, tot = 0;
  for (uint32_t x = 0; x < 16; ++x) {
    if (x < w) base += wsum[x];
    tot += wsum[x];
  }
  uint64_t o = base + inc - sum;
  for (uint64_t q = q0; q < q1; ++q) {
    a.val_off[q] = uint32_t(o);
    o += a.res[q].status == LSMBLK_GET_FOUND ? a.res[q].vlen : 0u;
  }
  if (t == 0) {
    a.val_off[a.nq] = uint32_t(tot);
    a.stats[2] = tot;
    uint32_t e = 0;
    if (tot > 0xFFFFFFFFull) e |= LSMBLK_ERR_OVERFLOW;
    if (tot > a.val_cap) e |= LSMBLK_ERR_CAPACITY;
    if (e) atomicOr(reinterpret_cast<unsigned long long*>(a.stats + 3), (unsigned long long)e);
  }
}

// One wave per lookup, grid-strided: a FOUND lookup's value bytes into its place.
__global__ __launch_bounds__(256) void val_gather_kernel(GetArgs a) {
  if (a.stats[3] & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW)) return;
  const uint64_t stride = uint64_t(gridDim.x) * 4;
  for (uint64_t q = uint64_t(blockIdx.x) * 4 + wave_id(); q < a.nq; q += stride) {
    if (uni(a.res[q].status) != LSMBLK_GET_FOUND) continue;
    const uint32_t vl = uni(a.res[q].vlen), o = uni(a.val_off[q]);
    if (uint64_t(o) + vl > a.val_cap) continue;
    wave_copy_bytes(a.vals + o, a.files + uni64(a.res[q].val_pos), vl);
  }
}

}  // namespace

extern "C" {

int lsmblk_sst_open_batch(lsmblk_ctx* c, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                          lsmblk_sst_desc* desc, lsmblk_sst_index* index, uint64_t index_cap, uint64_t* stats,
                          void* stream) {
  if (!c || !stats || (nsst && (!file_off || !desc || !files)) || (index_cap && !index)) return LSMBLK_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(files) & 15) || (reinterpret_cast<uintptr_t>(index) & 15) || nsst > 0x3FFFFFFFu)
    return LSMBLK_E_INVAL;
  std::lock_guard<std::mutex> g(c->mu);
  DeviceGuard dg(c->device, c);
  if (!dg.ok) return LSMBLK_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(stats, 0, LSMBLK_STATS_WORDS * 8, st) != hipSuccess) return LSMBLK_E_HIP;
  if (nsst == 0) return LSMBLK_OK;
  int rc;
  if ((rc = lsmblk_impl::ensure_crc_tabs(c, st))) return rc;
  // workspace: the CRC range table, the CRCs, the CRC pass's own stats
  const uint64_t tab_bytes = (8ull * (4ull * nsst + 1) + 255) & ~255ull, crc_bytes = (16ull * nsst + 255) & ~255ull;
  const uint64_t need = tab_bytes + crc_bytes + 256;
  if (need > c->sws_cap && (rc = grow(st, &c->sws, &c->sws_cap, need, 1))) return rc;
  OpenArgs a;
  a.files = files;
  a.file_off = file_off;
  a.nsst = nsst;
  a.desc = desc;
  a.index = index;
  a.index_cap = index_cap;
  a.tab = reinterpret_cast<uint64_t*>(c->sws);
  uint32_t* crc = reinterpret_cast<uint32_t*>(c->sws + tab_bytes);
  uint64_t* cstats = reinterpret_cast<uint64_t*>(c->sws + tab_bytes + crc_bytes);
  a.crc = crc;
  a.stats = stats;
  if (hipMemsetAsync(cstats, 0, 32, st) != hipSuccess) return LSMBLK_E_HIP;
  LSM_LAUNCH(sst_open_prep_kernel, dim3(1), dim3(1024), 0, st, a);
  // (the ranges between the sections are flagged in cstats, which nothing reads)
  if ((rc = lsmblk_impl::launch_crc(c, files, a.tab, 4ull * nsst, 0, crc, cstats, st, nullptr, true))) return rc;
  LSM_LAUNCH(sst_open_walk_kernel, dim3(nsst), dim3(64), 0, st, a);
  return hipGetLastError() == hipSuccess ? LSMBLK_OK : LSMBLK_E_HIP;
}

int lsmblk_sst_get_batch(lsmblk_ctx* c, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                         const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const uint32_t* q_sst,
                         const uint8_t* qkeys, const uint32_t* qkey_off, const uint64_t* q_ts, uint64_t nq,
                         uint32_t flags, lsmblk_get_result* res, uint8_t* vals, uint64_t val_cap, uint32_t* val_off,
                         uint64_t* stats, void* stream) {
  if (!c || !stats || (flags & ~(LSMBLK_GET_NO_FILTER | LSMBLK_GET_MVCC)) || (vals && !val_off)) return LSMBLK_E_INVAL;
  if (nq && (!q_sst || !qkey_off || !q_ts || !res || (nsst && (!files || !file_off || !desc)))) return LSMBLK_E_INVAL;
  if ((reinterpret_cast<uintptr_t>(files) & 15) || (reinterpret_cast<uintptr_t>(index) & 15) || nq >= 0xFFFFFFFFull)
    return LSMBLK_E_INVAL;
  std::lock_guard<std::mutex> g(c->mu);
  DeviceGuard dg(c->device, c);
  if (!dg.ok) return LSMBLK_E_HIP;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(stats, 0, LSMBLK_STATS_WORDS * 8, st) != hipSuccess) return LSMBLK_E_HIP;
  if (nq == 0) {
    if (vals && hipMemsetAsync(val_off, 0, 4, st) != hipSuccess) return LSMBLK_E_HIP;
    return LSMBLK_OK;
  }
  GetArgs a{files, file_off, nsst, desc, index, q_sst, qkeys, qkey_off, q_ts, nq, flags, res, vals, val_cap, val_off, stats};
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
  const uint64_t cap = uint64_t(cus > 0 ? cus : 256) * 8, want = (nq + kGetWaves - 1) / kGetWaves;
  LSM_LAUNCH(sst_get_kernel, dim3(uint32_t(want < cap ? want : cap)), dim3(64 * kGetWaves), 0, st, a);
  if (vals) {
    LSM_LAUNCH(val_scan_kernel, dim3(1), dim3(1024), 0, st, a);
    const uint64_t gw = (nq + 3) / 4;
    LSM_LAUNCH(val_gather_kernel, dim3(uint32_t(gw < cap ? gw : cap)), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? LSMBLK_OK : LSMBLK_E_HIP;
}

}  // extern "C"
