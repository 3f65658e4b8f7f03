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
//     sst_get_kernel        one wave per lookup, grid-strided (sst_lookup): key range, bloom probes from k lanes
//                           at once, k-ary block search over the first-key images, the landed block
//                           staged into LDS with 16-B loads, every entry compared by its own lane
//                           (equal range [L, U)), the reference's probe sequence replayed on L / U,
//                           the version walk
//     val_scan_kernel       value sizes of the FOUND lookups -> val_off (one workgroup)
//     val_gather_kernel     one wave per FOUND lookup copies its value
//   lsmblk_lsm_get_batch    get_with_ts (lsm_storage.rs:361-438) for a batch of keys over an LSM view of
//                           the opened set: memtable runs, L0 tables, levels, one answer per key
//     lsm_view_check_kernel one lane per view entry: ids, failed opens, level_start, check_sst_valid;
//                           mem_start
//     lsm_get_kernel        one wave per key: lane s holds source s's table (a level's by a search over
//                           its tables' first-key images), every lane runs keep_table for its own,
//                           the passing sources are read in priority order by sst_lookup -- the
//                           per-table read it shares with sst_get_kernel -- up to the decider
//   lsmblk_sst_scan_batch   raw range scans of one SST per query (scan_with_ts's SsTableIterator per
//                           table, lsm_storage.rs:474-502, run to its end bound); the end bound is
//                           tested on every entry, the landing included -- LsmIterator::new's untested
//                           first position (lsm_iterator.rs:29-43) belongs to the merged iterator and
//                           is not reproduced per SST.  Kernels: see "scan" below
//   lsmblk_lsm_scan_batch   scan_with_ts (lsm_storage.rs:446-550) for a batch of ranges over an LSM view:
//                           every passing memtable run sliced, every passing table scanned by the scan kernels, a
//                           segmented merge per range, the reader's view.  Kernels: see "the LSM range
//                           scan" below
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
  const uint32_t t = threadIdx.x;
  __shared__ uint64_t wsum[16];
  int tb = 0;
  for (uint32_t s = t; s < a.nsst; s += kWgScan) tb |= a.file_off[s + 1] < a.file_off[s];
  const bool tbad = __syncthreads_or(tb) != 0;
  uint64_t carry = 0;
  for (uint32_t r = 0; r < a.nsst; r += kWgScan) {  // the rounds form of the workgroup scan
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
    const uint64_t base = block_round1024(cnt, wsum, carry);
    if (s < a.nsst) a.desc[s].blk0 = uint32_t(base);
  }
  if (t == 0) {
    uint32_t e = tbad ? LSMBLK_ERR_MALFORMED : 0u;
    a.stats[1] = carry;
    if (carry > 0xFFFFFFFFull) e |= LSMBLK_ERR_OVERFLOW;
    if (carry > a.index_cap) e |= LSMBLK_ERR_CAPACITY;
    or_err(a.stats, e);
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
    if (l == 0) or_word(a.stats + 2, d.err);
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
    KeyImage fm{0, 0};
    if (fl) fm = image_of_bytes(need(kpos, fl < 16 ? fl : 16), fl);
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
      rec.img_hi = fm.hi;
      rec.img_lo = fm.lo;
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
      or_word(a.stats + 2, err);
    }
    d.err = err;
    a.desc[s] = d;
  }
}

// ---------------------------------------------------------------- the read calls' arguments
// The pieces the kernel argument structs of the four read calls are composed of: each field list is
// written here once.  A base struct's fields keep their spelling in the kernels (a.files, a.nl0).
struct OpenedSet {  // what lsmblk_sst_open_batch made of the resident files
  const uint8_t* files;
  const uint64_t* file_off;
  uint32_t nsst;
  const lsmblk_sst_desc* desc;
  const lsmblk_sst_index* index;
};
struct MemArgs {  // the memtable runs of a lsmblk_lsm_view: run r = entries [start[r], start[r + 1]) of the stream
  const uint8_t* keys;
  const uint32_t* key_off;
  const uint8_t* vals;
  const uint32_t* val_off;
  const uint64_t* ts;
  uint64_t n;
  const uint32_t* start;
  uint32_t nmem;       // <= kMaxMem: a run per lane
  uint32_t key_bytes;  // key_off[n], read by the kernels that compare keys (mem_keys): the arena's end
};
struct ViewArgs {  // lsmblk_lsm_view
  const uint32_t* l0;
  uint32_t nl0, nlevel;
  const uint32_t* level_sst;
  const uint32_t* level_start;
  MemArgs mem;
};
constexpr uint32_t kMaxMem = 64;
static_assert(sizeof(lsmblk_lsm_view) == 56, "lsmblk_lsm_view: the memtable runs are its last three fields");
struct PointArgs {  // a batch of point reads and where their values go
  const uint8_t* qkeys;
  const uint32_t* qkey_off;
  const uint64_t* q_ts;
  uint64_t nq;
  uint32_t flags;
  uint8_t* vals;
  uint64_t val_cap;
  uint32_t* val_off;
  uint64_t* stats;
};
struct BoundArgs {  // a batch of ranges: bound keys and kinds
  const uint8_t* lkeys;
  const uint32_t* lkey_off;
  const uint8_t* ukeys;
  const uint32_t* ukey_off;
  const uint32_t* q_bound;
};
struct DevStream {  // a lsmblk_kv_stream the kernels write (or read back); on: the caller gave one
  uint8_t* keys;
  uint32_t* key_off;
  uint8_t* vals;
  uint32_t* val_off;
  uint64_t* ts;
  uint64_t entry_cap, key_cap, val_cap;
  uint32_t on;
};
DevStream dev_stream(const lsmblk_kv_stream* s) {
  if (!s) return DevStream{};
  return DevStream{s->keys, s->key_off, s->vals, s->val_off, s->ts, s->entry_cap, s->key_cap, s->val_cap, 1u};
}

// ---------------------------------------------------------------- get
struct GetArgs : OpenedSet, PointArgs {
  const uint32_t* q_sst;
  lsmblk_get_result* res;
};

using QKey = KeyRef<ArenaKeys>;  // the query key, through key_upto (lsmblk_keys.hpp)

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

// partition_point of an SST's block first keys against the query: the blocks with first_key <= q
// (strict: < q), by the k-ary search over the first-key images; blocks whose image equals the
// query's, [iL, iU), compare whole keys.
__device__ __forceinline__ uint32_t index_partition(const lsmblk_sst_index* ix, const uint8_t* F, uint32_t nblk,
                                                    const QKey& q, bool strict) {
  const KeyImage qm = image_of(q);  // (the index records hold each first key's image: img_hi, img_lo)
  auto img = [&](uint32_t i) { return KeyImage::pair(*reinterpret_cast<const u32x4*>(ix + i)); };
  const uint32_t iL = kary_first_false(0, nblk, [&](uint32_t i) { return img(i) < qm; });
  const uint32_t iU = kary_first_false(iL, nblk, [&](uint32_t i) { return img(i) <= qm; });
  uint32_t P = iL;
  if (iU > iL)
    P = kary_first_false(iL, iU, [&](uint32_t i) {
      const int c = byte_cmp(KeyPtr{F + ix[i].key_pos, ix[i].key_len}, q);
      return strict ? c < 0 : c <= 0;
    });
  return P;
}

// The shared parse_hdr (lsmblk_dev.hpp) for a wave that reads one block: every lane loads the same
// header, so its fields are made wave-uniform.
template <class Img>
__device__ __forceinline__ BlockHdr get_hdr(const Img& im, uint32_t len) {
  BlockHdr h = parse_hdr(im, len);
  h.n = uni(h.n);
  h.data_end = uni(h.data_end);
  h.fks = uni(h.fks);
  return h;
}

// The block's entries against the query, every lane comparing its own: L = entries below it, U =
// entries not above it, so [L, U) is the equal range (the block is sorted).  Every entry is parsed
// and checked; false: the block breaks the decode rules.
template <class Img>
__device__ __forceinline__ bool block_lu(const Img& im, const BlockHdr& h, const QKey& q, uint32_t& L, uint32_t& U) {
  const uint32_t l = lane_id();
  // m = lcp(first key, query); an entry that shares more than m bytes with the first key orders
  // against the query as the first key does at byte m, one that shares at most m has its first
  // `prefix` bytes equal to the query's and is decided by its suffix
  uint32_t m = 0;
  int cfk = 0;
  if (h.n) cfk = wave_cmp([&](uint32_t i) { return im.u8(4 + i); }, h.fks, q, m);
  const int cbeyond = m == q.len ? 1 : cfk;
  L = 0;
  U = 0;
  bool bad = false;
  for (uint32_t c = 0; c < h.n; c += 64) {
    const uint32_t e = c + l;
    int cm = 1;
    if (e < h.n) {
      // parse_entry's rules (lsmblk_dev.hpp), every load behind its check as in seek_kernel: through
      // the shared load-then-check form a filtered lsmblk_sst_get_batch measured 3.8 % slower
      // ("One block parser ..."); tests/test_gpu_block_rules.py holds this copy to the rules
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
  if (__ballot(bad)) return false;
  L = uni(L);
  U = uni(U);
  return true;
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
  bool on_key;  // the landing entry's key equals the query
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
  const BlockHdr h = get_hdr(im, len);
  if (!h.ok) return Visit{true, true};
  uint32_t L = 0, U = 0;
  if (!block_lu(im, h, q, L, U)) return Visit{true, true};
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
    k.on_key = true;
    from = land;
  } else {
    if (!k.landed) {
      k.landed = true;
      k.blk = b;
      k.ent = 0;
    }
    if (h.n == 0) return Visit{false, false};
    if (L != 0 || U == 0) return Visit{true, false};  // entry 0 is another key
    k.on_key = true;  // (a spill's landing, or the walk goes on)
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

struct QHash {  // fingerprint32 of the query key, computed by the first bloom test that needs it
  uint32_t h;
  bool valid;
};

// One table's read of one key (wave-uniform): key_within, the bloom test, find_block_idx, the landed
// block and the blocks the iterator moves on to -> k (k.status also RANGE_OUT / BLOOM_OUT; k.on_key:
// the landing entry's key is the query).  True: a block on the path breaks the decode rules.
__device__ __forceinline__ bool sst_lookup(const OpenedSet& o, uint32_t s, const QKey& q, uint64_t read_ts, bool mvcc,
                                           bool filter, uint8_t* S, QHash& qh, Look& k) {
  const uint32_t l = lane_id();
  const lsmblk_sst_desc* dp = o.desc + s;
  const uint32_t blk0 = uni(dp->blk0), nblk = uni(dp->nblk);
  const uint64_t fo = uni64(o.file_off[s]);
  const uint8_t* const F = o.files + fo;
  if (nblk == 0) {  // not opened: the iterator is invalid from the start
    k.blk = 0;
    k.ent = 0;
    return false;
  }
  if (filter) {
    // key_within (lsm_storage.rs:136-138): first_key <= key <= last_key
    const uint8_t* fk = o.files + uni64(dp->first_key_pos);
    const uint8_t* lk = o.files + uni64(dp->last_key_pos);
    uint32_t lcp;
    if (wave_cmp([&](uint32_t i) { return uint32_t(fk[i]); }, uni(dp->first_key_len), q, lcp) > 0 ||
        wave_cmp([&](uint32_t i) { return uint32_t(lk[i]); }, uni(dp->last_key_len), q, lcp) < 0) {
      k.status = LSMBLK_GET_RANGE_OUT;
      return false;
    }
    // Bloom::may_contain (bloom.rs:104-120): probe i tests bit (h + i delta) % (nbits as u32);
    // the k <= 30 probes are independent: lane i makes probe i, one round trip for all
    const uint32_t bk = uni(dp->bloom_k);
    if (bk <= 30) {
      const uint32_t nbits = uni(dp->bloom_len) * 8u;
      bool pass = false;
      if (nbits) {
        if (!qh.valid) {
          qh.h = fingerprint32(q, q.len);
          qh.valid = true;
        }
        const uint32_t h = qh.h, delta = (h >> 17) | (h << 15);
        bool miss = false;
        if (l < bk) {
          const uint32_t bit = (h + l * delta) % nbits;
          miss = !((o.files[uni64(dp->bloom_pos) + (bit >> 3)] >> (bit & 7)) & 1);
        }
        pass = __ballot(miss) == 0;
      }
      if (!pass) {
        k.status = LSMBLK_GET_BLOOM_OUT;
        return false;
      }
    }
  }
  // find_block_idx (table.rs:253-257): P = partition_point(first_key <= key) (MVCC: < key)
  const lsmblk_sst_index* const ix = o.index + blk0;
  const uint32_t P = index_partition(ix, F, nblk, q, mvcc);
  uint32_t b = P ? P - 1 : 0;
  bool first = true, bad = false;
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
      bad = true;
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
  return bad;
}

// 8 waves per SIMD (64 VGPRs): a lookup is a chain of dependent reads, so the lookups in flight hide
// each other's round trips; the compiler's free choice was 181 VGPRs (2 waves per SIMD).
__global__ __launch_bounds__(64 * kGetWaves) __attribute__((amdgpu_waves_per_eu(8))) void sst_get_kernel(GetArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t img[kGetWaves][kGetImg];
  const uint32_t l = lane_id();
  uint8_t* const S = img[wave_id()];
  const bool mvcc = (a.flags & LSMBLK_GET_MVCC) != 0, filter = !(a.flags & LSMBLK_GET_NO_FILTER);
  const OpenedSet& o = a;
  uint32_t err = 0, nfound = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.stats[0] = a.nq;
  const uint64_t stride = uint64_t(gridDim.x) * kGetWaves;
  for (uint64_t qi = uint64_t(blockIdx.x) * kGetWaves + wave_id(); qi < a.nq; qi += stride) {
    Look k{LSMBLK_GET_ABSENT, kNone, kNone, kNone, kNone, 0, 0, 0, false, false};
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
      const QKey q = key_upto(a.qkeys, k0, k1);
      QHash qh{0, false};
      if (sst_lookup(o, s, q, uni64(a.q_ts[qi]), mvcc, filter, S, qh, k)) err |= LSMBLK_ERR_MALFORMED;
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

// ---------------------------------------------------------------- the LSM point read
// lsmblk_lsm_get_batch: the view check, then one wave per key over the view's sources.
struct ViewCheckArgs : OpenedSet, ViewArgs {
  uint64_t* stats;
  uint32_t* vflag;  // the view check's verdict (workspace): error flags, 0 = the reads run
};
struct LsmGetArgs : OpenedSet, ViewArgs, PointArgs {
  lsmblk_lsm_get_result* res;
  uint32_t* vflag;
};

// The view against the opened set, one lane per view entry (the L0 ids, then the level ids):
// level_start (and mem_start, which bounds every read of a memtable run, against mem->n) first, by
// every workgroup -- it bounds the reads of level_sst -- then per entry the id,
// its open, and for a level entry with a right neighbour check_sst_valid's order
// (concat_iterator.rs:82-93), last_key(i) < first_key(i + 1), through the descriptors' key positions.
__global__ __launch_bounds__(256) void lsm_view_check_kernel(ViewCheckArgs a) {
  int sb = 0;
  for (uint32_t i = threadIdx.x; i < a.nlevel; i += 256)
    sb |= (i == 0 && a.level_start[0] != 0) || a.level_start[i + 1] < a.level_start[i];
  // mem_start, the same shape over the memtable runs' entries: it bounds every read of a run
  if (const uint32_t i = threadIdx.x; i < a.mem.nmem)
    sb |= (i == 0 && a.mem.start[0] != 0) || a.mem.start[i + 1] < a.mem.start[i] ||
          (i + 1 == a.mem.nmem && a.mem.start[i + 1] != a.mem.n);
  uint32_t err = 0;
  if (__syncthreads_or(sb)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) err = LSMBLK_ERR_SEGMENTS;
  } else {
    const uint32_t nlv = a.nlevel ? a.level_start[a.nlevel] : 0u;
    const uint64_t total = uint64_t(a.nl0) + nlv, stride = uint64_t(gridDim.x) * 256;
    for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += stride) {
      const bool lv = i >= a.nl0;
      const uint32_t j = uint32_t(i - a.nl0);  // (a level entry's place in level_sst)
      const uint32_t t = lv ? a.level_sst[j] : a.l0[i];
      if (t >= a.nsst) {
        err |= LSMBLK_ERR_SEGMENTS;
        continue;
      }
      const lsmblk_sst_desc* d = a.desc + t;
      if (d->err || d->nblk == 0) {
        err |= LSMBLK_ERR_MALFORMED;
        continue;
      }
      if (!lv || j + 1 >= nlv) continue;
      // j + 1 starts a level (first l in [1, nlevel] with level_start[l] >= j + 1 equals it): no neighbour
      uint32_t lo = 1, hi = a.nlevel;
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.level_start[mid] >= j + 1) hi = mid;
        else lo = mid + 1;
      }
      if (a.level_start[lo] == j + 1) continue;
      const uint32_t u = a.level_sst[j + 1];
      if (u >= a.nsst || a.desc[u].err || a.desc[u].nblk == 0) continue;  // (flagged by its own lane)
      const lsmblk_sst_desc* e = a.desc + u;
      if (byte_cmp(KeyPtr{a.files + d->last_key_pos, d->last_key_len},
                   KeyPtr{a.files + e->first_key_pos, e->first_key_len}) >= 0)
        err |= LSMBLK_ERR_MALFORMED;
    }
  }
  if (err) {
    atomicOr(a.vflag, err);
    or_err(a.stats, err);
  }
}

// A level's source for the query: the tables [0, n) of ls (a level's ids, in key order) with
// first_key <= q, counted as index_partition counts blocks -- a table's first key is its first
// block's, so index[desc[t].blk0] holds its image; whole keys only inside the image tie range.
// Table t's image against the query's: 1 = below it, 2 = not above it.
__device__ __forceinline__ uint32_t table_img_le(const OpenedSet& o, uint32_t nsst, uint32_t t, const KeyImage& qm) {
  if (t >= nsst) return 0;  // (the view check refuses such a view)
  const KeyImage v = KeyImage::pair(*reinterpret_cast<const u32x4*>(o.index + o.desc[t].blk0));
  return (v < qm ? 1u : 0u) | (v <= qm ? 2u : 0u);
}
// ... and the partition point from the image bounds: whole keys inside [iL, iU)
__device__ __forceinline__ uint32_t level_tie(const OpenedSet& o, uint32_t nsst, const uint32_t* ls, uint32_t iL, uint32_t iU,
                                              const QKey& q) {
  if (iU <= iL) return iL;
  return kary_first_false(iL, iU, [&](uint32_t i) {
    const uint32_t t = ls[i];
    if (t >= nsst) return false;
    return byte_cmp(KeyPtr{o.files + o.desc[t].first_key_pos, o.desc[t].first_key_len}, q) <= 0;
  });
}
__device__ __forceinline__ uint32_t level_partition(const OpenedSet& o, uint32_t nsst, const uint32_t* ls, uint32_t n,
                                                    const QKey& q, const KeyImage& qm) {
  const uint32_t iL = kary_first_false(0, n, [&](uint32_t i) { return (table_img_le(o, nsst, ls[i], qm) & 1) != 0; });
  const uint32_t iU = kary_first_false(iL, n, [&](uint32_t i) { return (table_img_le(o, nsst, ls[i], qm) & 2) != 0; });
  return level_tie(o, nsst, ls, iL, iU, q);
}

// Key order of file bytes p[0 .. len) against the query (image qm) by one lane: their leading 16
// bytes as images (16 independent loads, one round trip) decide unless they tie.
__device__ __forceinline__ int lane_cmp_img(const uint8_t* p, uint32_t len, const QKey& q, const KeyImage& qm) {
  return image_byte_cmp(image_of_bytes(p, len), KeyPtr{p, len}, qm, q);
}

// keep_table (lsm_storage.rs:383-398) by one lane for its own table, in two steps so that the key
// is hashed only when some table's range holds it: key_within ...
__device__ __forceinline__ bool lane_key_within(const OpenedSet& o, uint32_t t, const QKey& q, const KeyImage& qm) {
  const lsmblk_sst_desc* d = o.desc + t;
  if (d->nblk == 0) return false;  // not opened (the view check refuses such a view)
  return lane_cmp_img(o.files + d->first_key_pos, d->first_key_len, q, qm) <= 0 &&
         lane_cmp_img(o.files + d->last_key_pos, d->last_key_len, q, qm) >= 0;
}
// ... and Bloom::may_contain (bloom.rs:104-120), every probe made (independent loads)
__device__ __forceinline__ bool lane_may_contain(const OpenedSet& o, uint32_t t, uint32_t h) {
  const lsmblk_sst_desc* d = o.desc + t;
  const uint32_t bk = d->bloom_k, nbits = d->bloom_len * 8u;
  if (bk > 30) return true;
  if (!nbits) return false;
  const uint8_t* B = o.files + d->bloom_pos;
  const uint32_t delta = (h >> 17) | (h << 15);
  bool miss = false;
  for (uint32_t i = 0; i < bk; ++i) {
    const uint32_t bit = (h + i * delta) % nbits;
    miss |= !((B[bit >> 3] >> (bit & 7)) & 1);
  }
  return !miss;
}

// The runs with key_bytes filled in (wave-uniform; only after the view check passed: n is mem_start's end).
__device__ __forceinline__ MemArgs mem_keys(MemArgs m) {
  m.key_bytes = uni(m.key_off[m.n]);
  return m;
}

// Entry i of the memtable runs' stream against the query by one lane, images first as lane_cmp_img:
// the key's leading 16 bytes come from ONE 16-byte load at any alignment wherever 16 bytes from the
// key's start lie inside the arena (every key but the last few) -- a probe is then three loads, not
// eighteen -- and the bytes past the key's end are masked off.
__device__ __forceinline__ int mem_cmp(const MemArgs& m, uint32_t i, const QKey& q, const KeyImage& qm) {
  const uint32_t k0 = m.key_off[i], len = m.key_off[i + 1] - k0;
  return image_byte_cmp(image_of_load16(m.keys, m.key_bytes, k0, len), KeyPtr{m.keys + k0, len}, qm, q);
}

// The wave's lanes over the memtable runs: the 64 lanes are split evenly into lane groups of g = 2^lg
// lanes, the largest power of two with nmem g <= 64, and run r is searched by lanes [r g, (r + 1) g):
// one run has the whole wave, four runs 16 lanes each, more than 32 runs a lane each.
struct MemGroups {
  uint32_t lg, run, sub;  // log2 g; the lane's run and its place in the group
  bool on;                // the lane's group has a run
  __device__ __forceinline__ uint32_t g() const { return 1u << lg; }
  __device__ __forceinline__ bool lead() const { return on && sub == 0; }
  // the ballot bits of the lane's own group, counted
  __device__ __forceinline__ uint32_t count(uint64_t ballot) const {
    const uint64_t m = lg == 6 ? ~0ull : (1ull << g()) - 1;
    return uint32_t(__builtin_popcountll((ballot >> (run << lg)) & m));
  }
};
__device__ __forceinline__ MemGroups mem_groups(uint32_t nmem) {
  const uint32_t lg = nmem > 1 ? uint32_t(__builtin_clz(nmem - 1)) - 26u : 6u;  // 6 - ceil(log2 nmem)
  const uint32_t l = lane_id();
  return MemGroups{lg, l >> lg, l & ((1u << lg) - 1), (l >> lg) < nmem};
}

// First index of [lo, hi) where pred turns false (hi: nowhere), pred true on a prefix of the range, by
// the lane's group for the group's own range (lo, hi and `on` are the same in every lane of a group;
// every lane of the wave calls this): kary_first_false's step with g probes, so a step cuts the range
// (g + 1)-fold -- g = 1: in halves -- for one round trip, the groups' round trips in flight together.
// Every step shrinks every live range, so the steps are bounded by the longest range.
template <class Pred>
__device__ __forceinline__ uint32_t group_first_false(const MemGroups& G, uint32_t lo, uint32_t hi, bool on, Pred pred) {
  const uint32_t sh = G.lg ? G.lg : 1u;
  while (__ballot(on && lo < hi)) {
    const uint32_t n = on && lo < hi ? hi - lo : 0u;
    const uint32_t stride = (n + (1u << sh) - 1) >> sh;
    const uint32_t idx = lo + (G.sub + 1) * stride - 1;  // (n <= g: stride 1, a probe per entry)
    const bool p = n && idx < hi && pred(idx);
    const uint32_t cnt = G.count(__ballot(p));
    const uint32_t nhi = lo + (cnt + 1) * stride - 1;  // the first false probe (all true: the range's end)
    if (n) {
      lo += cnt * stride;
      if (cnt < G.g() && nhi < hi) hi = nhi;
    }
  }
  return lo;
}

// A run's read of one key by its lane group: the landing is the first entry with key >= the query
// (SkipMap::range: the same in every mode); on the key, the group's first lane walks its versions
// forward while ts > read_ts.  Both loops are bounded by the run's entries.  The result is in the
// group's first lane.
struct MemLook {
  bool on_key;   // the landing entry's key is the query
  uint32_t hit;  // the visible version's index in the stream; kNone: none
  uint32_t vlen;
  uint64_t ts;
};
__device__ __forceinline__ MemLook mem_lookup(const MemArgs& m, const MemGroups& G, const QKey& q, const KeyImage& qm,
                                              uint64_t read_ts) {
  MemLook o{false, kNone, 0, 0};
  const uint32_t lo = G.on ? m.start[G.run] : 0u, end = G.on ? m.start[G.run + 1] : 0u;
  const uint32_t land = group_first_false(G, lo, end, G.on, [&](uint32_t i) { return mem_cmp(m, i, q, qm) < 0; });
  if (G.lead()) {
    for (uint32_t e = land; e < end && mem_cmp(m, e, q, qm) == 0; ++e) {
      o.on_key = true;
      const uint64_t t = m.ts[e];
      if (t <= read_ts) {
        o.hit = e;
        o.ts = t;
        o.vlen = m.val_off[e + 1] - m.val_off[e];
        break;
      }
    }
  }
  return o;
}

// One wave per key, grid-strided, over the sources in priority order, 64 at a time:
//   memtable runs  (a view with any) before every table: the lanes are split into a group per run
//            (mem_groups), every group searches its own run, so all runs' round trips are in flight
//            together; the landings are folded in ordinal order -- the first run on the key decides
//            and no table is touched, or (NEWEST) the newest visible version of any run is the answer
//            the tables have to beat.  Tables are sources nmem + ...
//   tables   lane s holds source s's table: an L0 id, or the level's table routed by the wave -- a
//            view of up to 64 level tables in all has every table's image probed by its own lane
//            at once and each level's bounds counted out of the two ballots; a larger one runs
//            level_partition per level
//   filters  every lane runs keep_table for its own table: the sources' descriptor, key and filter
//            reads are in flight together, one chain of round trips for all sources instead of one
//            per source
//   reads    the sources that passed, in priority order, each by sst_lookup (no filter) through the
//            wave's LDS image
// Decider rule: the reads end at the first source whose landing is on the key (or whose path is
// malformed); bloom_out counts the rejected sources before it.  NEWEST: every passing source is
// read, the best (ts, lower ordinal) kept.
// kMem: the view has memtable runs.  A view without any runs the <false> form, which holds nothing
// of the runs: what it cost callers without memtables was measured ("Memtable runs ...").
template <bool kMem>
__global__ __launch_bounds__(64 * kGetWaves) __attribute__((amdgpu_waves_per_eu(8))) void lsm_get_kernel(LsmGetArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t img[kGetWaves][kGetImg];
  const uint32_t l = lane_id();
  uint8_t* const S = img[wave_id()];
  const bool newest = (a.flags & LSMBLK_LSM_GET_NEWEST) != 0, mvcc = newest || (a.flags & LSMBLK_GET_MVCC) != 0;
  const OpenedSet& o = a;
  const bool run = uni(*a.vflag) == 0;
  const uint32_t nsrc = a.nl0 + a.nlevel;
  const uint32_t nmem = kMem ? a.mem.nmem : 0u;  // the tables' first ordinal
  const uint32_t nlv = run && a.nlevel ? uni(a.level_start[a.nlevel]) : 0u;  // level tables in all
  uint32_t err = 0, nfound = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.stats[0] = a.nq;
  const uint64_t stride = uint64_t(gridDim.x) * kGetWaves;
  for (uint64_t qi = uint64_t(blockIdx.x) * kGetWaves + wave_id(); qi < a.nq; qi += stride) {
    // (every per-key state starts here: the answer, the hash and the counters)
    Look ans{LSMBLK_GET_ABSENT, kNone, kNone, kNone, kNone, 0, 0, 0, false, false};
    uint32_t asrc = kNone, asst = kNone, seeks = 0, bout = 0;
    QHash qh{0, false};
    const uint32_t k0 = uni(a.qkey_off[qi]), k1 = uni(a.qkey_off[qi + 1]);
    if (run && k1 <= k0) err |= LSMBLK_ERR_EMPTY_KEY;
    if (run && k1 > k0) {
      const QKey q = key_upto(a.qkeys, k0, k1);
      const uint64_t read_ts = uni64(a.q_ts[qi]);
      const KeyImage qm = image_of(q);
      uint64_t ltm = 0, lem = 0;  // nlv <= 64: level table i's image below / not above the query's
      if (nlv && nlv <= 64) {
        const uint32_t c = l < nlv ? table_img_le(o, a.nsst, a.level_sst[l], qm) : 0u;
        ltm = __ballot((c & 1) != 0);
        lem = __ballot((c & 2) != 0);
      }
      bool decided = false;
      if constexpr (kMem) {
        const MemArgs mem = mem_keys(a.mem);
        const MemGroups G = mem_groups(mem.nmem);
        const MemLook ml = mem_lookup(mem, G, q, qm, read_ts);
        // (a run's result is in its group's first lane: lane order is ordinal order)
        const uint64_t onm = __ballot(ml.on_key), hitm = __ballot(ml.hit != kNone);
        uint32_t w = kNone;  // the lane that answers
        seeks = nmem;
        if (!newest) {
          if (onm) {  // the decider: the runs after it count as never consulted
            w = uint32_t(__builtin_ctzll(onm));
            seeks = (w >> G.lg) + 1;
            decided = true;
          }
        } else {
          uint64_t best = 0;
          for (uint64_t m = hitm; m; m &= m - 1) {  // ordinal order: an equal ts keeps the lower run
            const uint32_t j = uint32_t(__builtin_ctzll(m));
            const uint64_t t = lane64(ml.ts, j);
            if (w == kNone || t > best) {
              w = j;
              best = t;
            }
          }
        }
        if (w != kNone) {
          asrc = w >> G.lg;  // (sst and hit_blk stay 0xFFFFFFFF: no table)
          ans.landed = ans.on_key = true;
          if ((hitm >> w) & 1) {
            ans.hit_ent = uint32_t(__builtin_amdgcn_readlane(ml.hit, w));
            ans.vlen = uint32_t(__builtin_amdgcn_readlane(ml.vlen, w));
            ans.ts = lane64(ml.ts, w);
            ans.val_pos = uni(a.mem.val_off[ans.hit_ent]);
            ans.status = ans.vlen ? LSMBLK_GET_FOUND : LSMBLK_GET_TOMBSTONE;
          }
        }
      }
      for (uint32_t base = 0; base < nsrc && !decided; base += 64) {
        const uint32_t cnt = nsrc - base < 64 ? nsrc - base : 64;
        uint32_t myt = kNone;  // lane s: the table of source base + s
        if (l < cnt && base + l < a.nl0) myt = a.l0[base + l];
        for (uint32_t src = base > a.nl0 ? base : a.nl0; src < base + cnt; ++src) {
          const uint32_t lo = uni(a.level_start[src - a.nl0]), hi = uni(a.level_start[src - a.nl0 + 1]);
          if (hi <= lo) continue;  // an empty level
          uint32_t P;
          if (nlv <= 64) {
            const uint64_t m = (hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1) << lo;  // hi <= nlv
            P = level_tie(o, a.nsst, a.level_sst + lo, uint32_t(__builtin_popcountll(ltm & m)),
                          uint32_t(__builtin_popcountll(lem & m)), q);
          } else {
            P = level_partition(o, a.nsst, a.level_sst + lo, hi - lo, q, qm);
          }
          if (P == 0) continue;    // below the level's first table
          const uint32_t t = uni(a.level_sst[lo + P - 1]);
          if (l == src - base) myt = t;
        }
        // (a key above the table's last key: a gap of the level, or past it)
        const bool within = myt < a.nsst && lane_key_within(o, myt, q, qm);
        bool pass = false;
        if (__ballot(within)) {
          if (!qh.valid) {
            qh.h = fingerprint32(q, q.len);
            qh.valid = true;
          }
          pass = within && lane_may_contain(o, myt, qh.h);
        }
        uint64_t passm = __ballot(pass), consulted = ~0ull;
        const uint64_t boutm = __ballot(within && !pass);
        while (passm) {
          const uint32_t s = uint32_t(__builtin_ctzll(passm));
          passm &= passm - 1;
          const uint32_t t = uint32_t(__builtin_amdgcn_readlane(myt, s));
          Look k{LSMBLK_GET_ABSENT, kNone, kNone, kNone, kNone, 0, 0, 0, false, false};
          const bool bad = sst_lookup(o, t, q, read_ts, mvcc, false, S, qh, k);
          if (bad) err |= LSMBLK_ERR_MALFORMED;
          ++seeks;
          if (!newest) {
            if (k.on_key || bad) {
              ans = k;
              asrc = nmem + base + s;
              asst = t;
              decided = true;
              consulted = (2ull << s) - 1;  // the sources up to the decider
              break;
            }
          } else if (k.status != LSMBLK_GET_ABSENT && (asrc == kNone || k.ts > ans.ts)) {
            ans = k;
            asrc = nmem + base + s;
            asst = t;
          }
        }
        bout += uint32_t(__builtin_popcountll(boutm & consulted));
      }
    }
    if (ans.status == LSMBLK_GET_FOUND) ++nfound;
    if (l == 0) {
      lsmblk_lsm_get_result r;
      r.status = ans.status;
      r.src = asrc;
      r.sst = asst;
      r.hit_blk = ans.hit_blk;
      r.hit_ent = ans.hit_ent;
      r.vlen = ans.vlen;
      r.ts = ans.ts;
      r.val_pos = ans.val_pos;
      r.seeks = seeks;
      r.bloom_out = bout;
      a.res[qi] = r;
    }
  }
  raise_err(a.stats, err);
  if (nfound && l == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats + 1), (unsigned long long)nfound);
}

// val_off = exclusive scan of the FOUND lookups' value sizes: the share form of the workgroup
// scan (lsmblk_dev.hpp) over the lookups.
template <class Args>
__global__ __launch_bounds__(1024) void val_scan_kernel(Args a) {
  __shared__ uint64_t wsum[16];
  uint64_t q0, q1;
  share1024(a.nq, q0, q1);
  uint64_t sum = 0, tot;
  for (uint64_t q = q0; q < q1; ++q) sum += a.res[q].status == LSMBLK_GET_FOUND ? a.res[q].vlen : 0u;
  uint64_t o = block_excl1024(sum, wsum, tot);
  for (uint64_t q = q0; q < q1; ++q) {
    a.val_off[q] = uint32_t(o);
    o += a.res[q].status == LSMBLK_GET_FOUND ? a.res[q].vlen : 0u;
  }
  // (not publish_totals: one total, in stats[2], and val_off has one entry per lookup, found or
  // not, so its sentinel index is nq whatever the total)
  if (threadIdx.x == 0) {
    a.val_off[a.nq] = uint32_t(tot);
    a.stats[2] = tot;
    uint32_t e = 0;
    if (tot > 0xFFFFFFFFull) e |= LSMBLK_ERR_OVERFLOW;
    if (tot > a.val_cap) e |= LSMBLK_ERR_CAPACITY;
    or_err(a.stats, e);
  }
}

// The arena a FOUND lookup's val_pos points into: the files, or for a hit in a memtable run of the
// view (src < nmem) the runs' value arena.
__device__ __forceinline__ const uint8_t* value_arena(const GetArgs& a, uint64_t) { return a.files; }
__device__ __forceinline__ const uint8_t* value_arena(const LsmGetArgs& a, uint64_t q) {
  return uni(a.res[q].src) < a.mem.nmem ? a.mem.vals : a.files;
}

// One wave per lookup, grid-strided: a FOUND lookup's value bytes into its place.
template <class Args>
__global__ __launch_bounds__(256) void val_gather_kernel(Args a) {
  if (a.stats[3] & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW)) return;
  const uint64_t stride = uint64_t(gridDim.x) * 4;
  for (uint64_t q = uint64_t(blockIdx.x) * 4 + wave_id(); q < a.nq; q += stride) {
    if (uni(a.res[q].status) != LSMBLK_GET_FOUND) continue;
    const uint32_t vl = uni(a.res[q].vlen), o = uni(a.val_off[q]);
    if (uint64_t(o) + vl > a.val_cap) continue;
    wave_copy_bytes(a.vals + o, value_arena(a, q) + uni64(a.res[q].val_pos), vl);
  }
}

// ---------------------------------------------------------------- scan
// lsmblk_sst_scan_batch: five launches, no device-side waits.
//   scan_bounds_kernel   one wave per range: range_overlap, begin (the point read's landing, the
//                        Excluded skip), end (a second index search and one in-block count) ->
//                        positions and the blocks the range touches
//   scan_units_kernel    one workgroup: blocks per unit = ceil(touched blocks / unit budget), units
//                        per range, their exclusive scan.  A unit is (range, up to `bpu` consecutive
//                        blocks), so a batch has at most nq + budget units whatever it touches and
//                        the workspace is sized without reading anything back
//   scan_count_kernel    one wave per unit: its blocks parsed and checked, clipped to the range's
//                        entry window -> entries, key bytes, value bytes
//   scan_offsets_kernel  one workgroup: the three-component scan over units (a malformed range's
//                        units count nothing), totals, capacity / overflow, sentinels, seg_start,
//                        res[q].n and the final statuses
//   scan_emit_kernel     one wave per unit: offsets and ts by the entry lanes, key prefix, key suffix
//                        and value of four entries at a time copied in 16-B pieces by 16 lanes each
constexpr uint32_t kScanWg = 1024;  // threads of the two one-workgroup scans: each takes a contiguous share

struct ScanArgs : OpenedSet, BoundArgs {
  const uint32_t* q_sst;
  uint64_t nq;
  uint32_t flags;
  lsmblk_scan_result* res;
  DevStream out;
  uint32_t* seg_start;
  uint64_t* stats;
  // workspace
  uint32_t* ubase;   // nq + 1: first unit of every range
  uint32_t* qbad;    // nq: a block of the range is malformed
  uint64_t* hdr;     // [0] units, [1] blocks per unit
  uint64_t* ucnt;    // 3 per unit: counts, then their exclusive prefixes
  uint32_t budget;
  // lsmblk_lsm_scan_batch's table scans (the kernels' kSub form): their count, known on the device
  // only, and per scan the range whose bound keys and kinds it takes; q_sst, res, qbad and seg_start
  // are per scan
  const uint64_t* nq_dev;
  const uint32_t* parent;
  // ... and the view's memtable runs: table scan "table" nsst + r is the slice of run r (kSub only)
  MemArgs mem;
};
template <bool kSub>
__device__ __forceinline__ uint64_t scan_nq(const ScanArgs& a) {
  if constexpr (kSub) return uni64(*a.nq_dev);
  else return a.nq;
}

// Block b of the SST through its LDS image S (up to kGetLdsBlock bytes) or a bounds-checked
// descriptor: fn(image, block bytes) -> its verdict; false when the index record's range is not a
// framed block inside the data section.
template <class Fn>
__device__ __forceinline__ bool on_block(const uint8_t* F, const lsmblk_sst_index* ix, uint32_t b, uint32_t meta_offset,
                                         uint8_t* S, Fn fn) {
  const uint32_t l = lane_id();
  const uint32_t off = uni(ix[b].off), end = uni(ix[b].end);
  if (!(end >= off + 4 + 2 && end <= meta_offset)) return false;
  const uint32_t len = end - off - 4;
  const uint8_t* src = F + off;
  const uint32_t lead = uni(uint32_t(reinterpret_cast<uintptr_t>(src) & 15));
  if (len <= kGetLdsBlock) {
    const uint32_t nch = (lead + len + 15) >> 4;  // inside the file: see sst_get_kernel
    u32x4 p[(kGetLdsBlock + 15 + 15) / 1024 + 1];
    wave_sync();
#pragma unroll
    for (uint32_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i)
      if (l + 64 * i < nch) p[i] = *reinterpret_cast<const u32x4*>(src - lead + 16 * (l + 64 * i));
#pragma unroll
    for (uint32_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i)
      if (l + 64 * i < nch) *reinterpret_cast<u32x4*>(S + 16 * (l + 64 * i)) = p[i];
    wave_sync();
    return fn(LdsImg{S, lead}, len);
  }
  const rsrc_t R = make_rsrc(reinterpret_cast<const uint8_t*>(uni64(reinterpret_cast<uintptr_t>(src - lead))),
                             uni(lead + len));
  return fn(GlbImg{R, lead}, len);
}

// (entries below the key, entries not above it, entries) of block b; false: malformed
__device__ __forceinline__ bool scan_lu(const uint8_t* F, const lsmblk_sst_index* ix, uint32_t b, uint32_t meta_offset,
                                        uint8_t* S, const QKey& q, uint32_t& L, uint32_t& U, uint32_t& n) {
  return on_block(F, ix, b, meta_offset, S, [&](const auto& im, uint32_t len) {
    const BlockHdr h = get_hdr(im, len);
    if (!h.ok) return false;
    n = h.n;
    return block_lu(im, h, q, L, U);
  });
}

template <bool kSub>
__global__ __launch_bounds__(64 * kGetWaves) void scan_bounds_kernel(ScanArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t img[kGetWaves][kGetImg];
  const uint32_t l = lane_id();
  uint8_t* const S = img[wave_id()];
  const bool mvcc = (a.flags & LSMBLK_SCAN_MVCC) != 0, filter = !(a.flags & LSMBLK_SCAN_NO_FILTER);
  uint32_t err = 0;
  const uint64_t stride = uint64_t(gridDim.x) * kGetWaves;
  const uint64_t nq = scan_nq<kSub>(a);
  for (uint64_t qi = uint64_t(blockIdx.x) * kGetWaves + wave_id(); qi < nq; qi += stride) {
    uint32_t status = LSMBLK_SCAN_EMPTY, b0 = kNone, e0 = kNone, b1 = kNone, e1 = kNone, nb = 0;
    bool malformed = false, mem = false;
    do {
      uint64_t pq = qi;  // the range whose bounds this scan takes
      if constexpr (kSub) pq = uni(a.parent[qi]);
      const uint32_t s = uni(a.q_sst[qi]), bnd = uni(a.q_bound[pq]);
      const uint32_t lk = bnd & 3, uk = (bnd >> 2) & 3;
      if constexpr (kSub) {
        // a memtable run's slice: lsm_scan_expand_kernel searched the run and wrote the result
        mem = s >= a.nsst && s - a.nsst < a.mem.nmem;
        if (mem) break;
      }
      if (s >= a.nsst || lk == 3 || uk == 3) {
        err |= LSMBLK_ERR_SEGMENTS;
        break;
      }
      uint32_t l0 = 0, l1 = 0, u0 = 0, u1 = 0;
      if (lk) {
        l0 = uni(a.lkey_off[pq]);
        l1 = uni(a.lkey_off[pq + 1]);
      }
      if (uk) {
        u0 = uni(a.ukey_off[pq]);
        u1 = uni(a.ukey_off[pq + 1]);
      }
      if ((lk && l1 <= l0) || (uk && u1 <= u0)) {
        err |= LSMBLK_ERR_EMPTY_KEY;
        break;
      }
      // (an unbounded side: an empty descriptor, never read)
      const QKey lo = key_upto(a.lkeys, l0, l1), up = key_upto(a.ukeys, u0, u1);
      const lsmblk_sst_desc* dp = a.desc + s;
      const uint32_t nblk = uni(dp->nblk), mo = uni(dp->meta_offset);
      if (nblk == 0) break;  // not opened
      const uint8_t* const F = a.files + uni64(a.file_off[s]);
      const lsmblk_sst_index* const ix = a.index + uni(dp->blk0);
      if (filter) {  // range_overlap (lsm_storage.rs:142-167)
        uint32_t lcp;
        bool outside = false;
        if (uk) {
          const uint8_t* fk = a.files + uni64(dp->first_key_pos);
          const int c = wave_cmp([&](uint32_t i) { return uint32_t(fk[i]); }, uni(dp->first_key_len), up, lcp);
          outside = uk == LSMBLK_BOUND_EXCLUDED ? c >= 0 : c > 0;  // upper <= / < the table's first key
        }
        if (lk && !outside) {
          const uint8_t* lkp = a.files + uni64(dp->last_key_pos);
          const int c = wave_cmp([&](uint32_t i) { return uint32_t(lkp[i]); }, uni(dp->last_key_len), lo, lcp);
          outside = lk == LSMBLK_BOUND_EXCLUDED ? c <= 0 : c < 0;  // lower >= / > the table's last key
        }
        if (outside) {
          status = LSMBLK_SCAN_RANGE_OUT;
          break;
        }
      }
      bool bad = false;
      // begin
      uint32_t b = 0, e = 0;
      if (lk) {
        const uint32_t P = index_partition(ix, F, nblk, lo, mvcc);
        b = P ? P - 1 : 0;
        uint32_t L = 0, U = 0, n = 0;
        if (!scan_lu(F, ix, b, mo, S, lo, L, U, n)) bad = true;
        if (!bad) {
          e = L;
          if (!mvcc) {  // BlockIterator::seek_to_key's probe sequence replayed on L / U (visit_block)
            uint32_t x = 0, y = n;
            bool found = false;
            while (x < y && !found) {
              const uint32_t mid = x + (y - x) / 2;
              if (mid < L) x = mid + 1;
              else if (mid >= U) y = mid;
              else {
                e = mid;
                found = true;
              }
            }
            if (!found) e = x;
          }
          if (lk == LSMBLK_BOUND_INCLUDED) {
            if (e >= n) {  // the spill
              ++b;
              e = 0;
            }
          } else {
            // forward while the entry's key equals the bound: inside [L, U) to U, from a block's end
            // to the next block's entry 0 (at most nblk blocks)
            for (;;) {
              if (e >= L && e < U) e = U;
              if (e < n) break;
              ++b;
              e = 0;
              if (b >= nblk) break;
              if (!scan_lu(F, ix, b, mo, S, lo, L, U, n)) {
                bad = true;
                break;
              }
              if (n == 0) continue;
              if (!(L == 0 && U > 0)) break;
            }
          }
        }
      }
      // end: the first entry with key > upper (Included) / >= upper (Excluded), not before begin
      uint32_t eb = nblk, ee = 0;
      if (uk && !bad) {
        const bool strict = uk == LSMBLK_BOUND_EXCLUDED;
        const uint32_t P = index_partition(ix, F, nblk, up, strict);
        eb = P ? P - 1 : 0;
        uint32_t L = 0, U = 0, n = 0;
        if (!scan_lu(F, ix, eb, mo, S, up, L, U, n)) bad = true;
        ee = strict ? L : U;
        if (ee >= n) {
          ++eb;
          ee = 0;
        }
      }
      if (bad) {
        err |= LSMBLK_ERR_MALFORMED;
        malformed = true;
        break;
      }
      if (b > nblk) b = nblk;
      if (eb < b || (eb == b && ee < e)) {
        eb = b;
        ee = e;
      }
      b0 = b;
      e0 = e;
      b1 = eb;
      e1 = ee;
      nb = (b1 == b0 && e1 == e0) ? 0u : b1 - b0 + (e1 > 0 ? 1u : 0u);
    } while (false);
    if (l == 0) {
      lsmblk_scan_result r;
      r.status = status;
      r.blk0 = b0;
      r.ent0 = e0;
      r.blk1 = b1;
      r.ent1 = e1;
      r.blocks = nb;
      r.n = 0;
      if (!mem) a.res[qi] = r;
      // (a table scan of the LSM scan marks a malformed search as well: its range takes no partial merge)
      a.qbad[qi] = kSub && malformed ? 1u : 0u;
    }
  }
  raise_err(a.stats, err);
}

static_assert(kScanWg == kWgScan, "share1024 / block_excl1024 (lsmblk_dev.hpp) serve a workgroup of kWgScan threads");

template <bool kSub>
__global__ __launch_bounds__(kScanWg) void scan_units_kernel(ScanArgs a) {
  __shared__ uint64_t wsum[16];
  const uint64_t nq = scan_nq<kSub>(a);
  uint64_t q0, q1;
  share1024(nq, q0, q1);
  uint64_t sum = 0, tot;
  for (uint64_t q = q0; q < q1; ++q) sum += a.res[q].blocks;
  (void)block_excl1024(sum, wsum, tot);
  const uint64_t bpu = tot > a.budget ? (tot + a.budget - 1) / a.budget : 1;
  sum = 0;
  for (uint64_t q = q0; q < q1; ++q) sum += (a.res[q].blocks + bpu - 1) / bpu;
  uint64_t o = block_excl1024(sum, wsum, tot);
  for (uint64_t q = q0; q < q1; ++q) {
    a.ubase[q] = uint32_t(o);
    o += (a.res[q].blocks + bpu - 1) / bpu;
  }
  if (threadIdx.x == 0) {
    a.ubase[nq] = uint32_t(tot);  // <= nq + budget < 2^32
    a.hdr[0] = tot;
    a.hdr[1] = bpu;
  }
}

// the range of unit u: the last q with ubase[q] <= u (empty ranges share their successor's base)
__device__ __forceinline__ uint32_t unit_query(const uint32_t* ubase, uint64_t nq, uint32_t u) {
  return kary_first_false(0, uint32_t(nq) + 1, [&](uint32_t i) { return ubase[i] <= u; }) - 1;
}

// One unit's blocks: fn(image, header, block, first entry, end entry) per block, in order; false as
// soon as a block is malformed.
template <class Fn>
__device__ __forceinline__ bool unit_blocks(const ScanArgs& a, uint32_t q, uint32_t u, uint8_t* S, Fn fn) {
  const uint32_t s = uni(a.q_sst[q]);
  const lsmblk_sst_desc* dp = a.desc + s;
  const uint8_t* const F = a.files + uni64(a.file_off[s]);
  const lsmblk_sst_index* const ix = a.index + uni(dp->blk0);
  const uint32_t mo = uni(dp->meta_offset), nblk = uni(dp->nblk);
  const uint32_t b0 = uni(a.res[q].blk0), e0 = uni(a.res[q].ent0), b1 = uni(a.res[q].blk1), e1 = uni(a.res[q].ent1);
  const uint32_t nb = uni(a.res[q].blocks), bpu = uint32_t(uni64(a.hdr[1]));
  const uint64_t first = uint64_t(u - uni(a.ubase[q])) * bpu;
  for (uint64_t j = first; j < first + bpu && j < nb; ++j) {
    const uint32_t b = b0 + uint32_t(j);
    if (b >= nblk) return false;
    const bool ok = on_block(F, ix, b, mo, S, [&](const auto& im, uint32_t len) {
      const BlockHdr h = get_hdr(im, len);
      if (!h.ok) return false;
      const uint32_t w0 = b == b0 ? e0 : 0u, w1 = b == b1 ? e1 : h.n;
      return fn(im, h, w0, w1 < h.n ? w1 : h.n);
    });
    if (!ok) return false;
  }
  return true;
}

template <bool kSub>
__global__ __launch_bounds__(64 * kGetWaves) void scan_count_kernel(ScanArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t img[kGetWaves][kGetImg];
  const uint32_t l = lane_id();
  uint8_t* const S = img[wave_id()];
  const uint64_t nu = uni64(a.hdr[0]), stride = uint64_t(gridDim.x) * kGetWaves, nq = scan_nq<kSub>(a);
  uint32_t err = 0;
  for (uint64_t u = uint64_t(blockIdx.x) * kGetWaves + wave_id(); u < nu; u += stride) {
    const uint32_t q = unit_query(a.ubase, nq, uint32_t(u));
    uint64_t ne = 0, kb = 0, vb = 0;
    if constexpr (kSub) {
      if (uni(a.q_sst[q]) >= a.nsst) {  // a memtable run's slice: one unit, its sizes are offset differences
        const uint32_t b = uni(a.res[q].blk0), e = uni(a.res[q].blk1);
        if (l == 0) {
          const bool in = b <= e && e <= a.mem.n;
          a.ucnt[3 * u] = in ? e - b : 0u;
          a.ucnt[3 * u + 1] = in ? a.mem.key_off[e] - a.mem.key_off[b] : 0u;
          a.ucnt[3 * u + 2] = in ? a.mem.val_off[e] - a.mem.val_off[b] : 0u;
        }
        continue;
      }
    }
    const bool ok = unit_blocks(a, q, uint32_t(u), S, [&](const auto& im, const BlockHdr& h, uint32_t w0, uint32_t w1) {
      bool bad = false;
      for (uint32_t c = 0; c < h.n; c += 64) {  // every entry is checked, the window's are counted
        const uint32_t e = c + l;
        if (e < h.n) {
          uint32_t off = 0, pf = 0, sf = 0, vl = 0;
          if (!parse_entry(im, h, e, off, pf, sf, vl)) {
            bad = true;
          } else if (e >= w0 && e < w1) {
            ne += 1;
            kb += pf + sf;
            vb += vl;
          }
        }
      }
      return __ballot(bad) == 0;
    });
    if (!ok) {
      err |= LSMBLK_ERR_MALFORMED;
      if (l == 0) a.qbad[q] = 1;
    }
    ne = wave_sum<uint64_t>(ne);
    kb = wave_sum<uint64_t>(kb);
    vb = wave_sum<uint64_t>(vb);
    if (l == 0) {
      a.ucnt[3 * u] = ne;
      a.ucnt[3 * u + 1] = kb;
      a.ucnt[3 * u + 2] = vb;
    }
  }
  raise_err(a.stats, err);
}

template <bool kSub>
__global__ __launch_bounds__(kScanWg) void scan_offsets_kernel(ScanArgs a) {
  __shared__ uint64_t wsum[16][3];
  const uint64_t nu = a.hdr[0], nq = scan_nq<kSub>(a);
  uint64_t u0, u1;
  share1024(nu, u0, u1);
  // a share's first range by search, then forward with the units (ubase is non-decreasing)
  auto first_query = [&](uint64_t u) {
    uint64_t lo = 0, hi = nq;  // the last q with ubase[q] <= u
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) / 2;
      if (a.ubase[mid] <= u) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  };
  // only a batch with a malformed block follows the units' ranges (dependent loads per unit);
  // otherwise a share is a run of independent loads
  const bool masked = (a.stats[3] & LSMBLK_ERR_MALFORMED) != 0;
  uint64_t sum[3] = {0, 0, 0}, tot[3], base[3];
  if (u0 < u1 && masked) {
    uint64_t q = first_query(u0);
    for (uint64_t u = u0; u < u1; ++u) {
      while (q + 1 < nq && a.ubase[q + 1] <= u) ++q;
      if (!a.qbad[q])
        for (uint32_t k = 0; k < 3; ++k) sum[k] += a.ucnt[3 * u + k];
    }
  } else {
    for (uint64_t u = u0; u < u1; ++u)
      for (uint32_t k = 0; k < 3; ++k) sum[k] += a.ucnt[3 * u + k];
  }
  block_excl1024<3>(sum, wsum, base, tot);
  if (!masked) {
    for (uint64_t u = u0; u < u1; ++u)
      for (uint32_t k = 0; k < 3; ++k) {
        const uint64_t v = a.ucnt[3 * u + k];
        a.ucnt[3 * u + k] = base[k];
        base[k] += v;
      }
  } else if (u0 < u1) {
    uint64_t q = first_query(u0);
    for (uint64_t u = u0; u < u1; ++u) {
      while (q + 1 < nq && a.ubase[q + 1] <= u) ++q;
      const bool live = !a.qbad[q];
      for (uint32_t k = 0; k < 3; ++k) {
        const uint64_t v = a.ucnt[3 * u + k];
        a.ucnt[3 * u + k] = base[k];
        if (live) base[k] += v;
      }
    }
  }
  if (threadIdx.x == 0) {
    // the entry total is held to 2^32 as well (seg_start holds u32 positions in it); a counting
    // call (no outputs) has no caps and no sentinels
    const TotalCaps caps = a.out.on ? TotalCaps{a.out.entry_cap, a.out.key_cap, a.out.val_cap} : TotalCaps{~0ull, ~0ull, ~0ull};
    publish_totals(a.stats, tot, caps, a.out.on ? a.out.key_off : nullptr, a.out.on ? a.out.val_off : nullptr, kSentIfClean, 0,
                   /*ovf_entries=*/true);
  }
  __threadfence_block();
  __syncthreads();  // the unit prefixes are written
  for (uint64_t q = threadIdx.x; q <= nq; q += kScanWg) {
    const uint32_t ub = a.ubase[q];
    const uint64_t st = ub < nu ? a.ucnt[3 * uint64_t(ub)] : tot[0];
    a.seg_start[q] = uint32_t(st);
    if (q < nq) {
      const uint32_t ue = a.ubase[q + 1];
      const uint64_t n = (ue < nu ? a.ucnt[3 * uint64_t(ue)] : tot[0]) - st;
      lsmblk_scan_result r = a.res[q];
      if (a.qbad[q]) {
        r.blk0 = r.ent0 = r.blk1 = r.ent1 = kNone;
        r.blocks = 0;
      }
      r.n = n;
      if (r.status != LSMBLK_SCAN_RANGE_OUT) r.status = n ? LSMBLK_SCAN_OK : LSMBLK_SCAN_EMPTY;
      a.res[q] = r;
    }
  }
}

// len bytes of the image from src -> dst by the 16 lanes of a quarter wave (sub = lane & 15), any
// alignment: 16-B pieces, then the last partial piece one byte per lane (adjacent lanes, adjacent
// bytes: one store instruction; a serial byte loop in one lane cost a round trip per byte, and most
// keys' prefix and suffix are shorter than 16 bytes).
template <class Img>
__device__ __forceinline__ void quarter_copy(uint8_t* dst, const Img& im, uint32_t src, uint32_t len, uint32_t sub) {
  const uint32_t full = len & ~15u;
  for (uint32_t o = 16 * sub; o < full; o += 256) {
    const u32x4 v{im.le32(src + o), im.le32(src + o + 4), im.le32(src + o + 8), im.le32(src + o + 12)};
    *reinterpret_cast<u32x4*>(dst + o) = v;
  }
  const uint32_t x = full + sub;
  if (x < len) dst[x] = uint8_t(im.u8(src + x));
}

// Entries [b, e) of the memtable runs' stream -> out from entry ei, key byte ko, value byte vo, by the
// whole wave: the offsets rebased and the ts entry by entry, the key and the value bytes each as one
// contiguous copy at any alignment.
__device__ __forceinline__ void mem_emit(const MemArgs& m, const DevStream& out, uint32_t b, uint32_t e, uint64_t ei,
                                         uint64_t ko, uint64_t vo) {
  if (b >= e || e > m.n) return;
  const uint32_t k0 = uni(m.key_off[b]), v0 = uni(m.val_off[b]);
  const uint32_t kb = uni(m.key_off[e]) - k0, vb = uni(m.val_off[e]) - v0;
  // (the totals passed the capacity check; a slice past a capacity would be a stream that changed
  // since the count: it is not written)
  if (ei + (e - b) > out.entry_cap || ko + kb > out.key_cap || vo + vb > out.val_cap) return;
  for (uint32_t i = lane_id(); i < e - b; i += 64) {
    out.key_off[ei + i] = uint32_t(ko) + (m.key_off[b + i] - k0);
    out.val_off[ei + i] = uint32_t(vo) + (m.val_off[b + i] - v0);
    out.ts[ei + i] = m.ts[b + i];
  }
  wave_copy_bytes(out.keys + ko, m.keys + k0, kb);
  wave_copy_bytes(out.vals + vo, m.vals + v0, vb);
}

template <bool kSub>
__global__ __launch_bounds__(64 * kGetWaves) void scan_emit_kernel(ScanArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t img[kGetWaves][kGetImg];
  if (a.stats[3] & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW)) return;
  const uint32_t l = lane_id(), sub = l & 15, grp = l >> 4;
  uint8_t* const S = img[wave_id()];
  const uint64_t nu = uni64(a.hdr[0]), stride = uint64_t(gridDim.x) * kGetWaves, nq = scan_nq<kSub>(a);
  for (uint64_t u = uint64_t(blockIdx.x) * kGetWaves + wave_id(); u < nu; u += stride) {
    const uint32_t q = unit_query(a.ubase, nq, uint32_t(u));
    if (uni(a.qbad[q])) continue;
    uint64_t ei = uni64(a.ucnt[3 * u]), ko = uni64(a.ucnt[3 * u + 1]), vo = uni64(a.ucnt[3 * u + 2]);
    if constexpr (kSub) {
      if (uni(a.q_sst[q]) >= a.nsst) {
        mem_emit(a.mem, a.out, uni(a.res[q].blk0), uni(a.res[q].blk1), ei, ko, vo);
        continue;
      }
    }
    (void)unit_blocks(a, q, uint32_t(u), S, [&](const auto& im, const BlockHdr& h, uint32_t w0, uint32_t w1) {
      for (uint32_t c = w0; c < w1; c += 64) {
        const uint32_t e = c + l, cnt = w1 - c < 64 ? w1 - c : 64u;
        uint32_t off = 0, pf = 0, sf = 0, vl = 0;
        bool live = e < w1 && parse_entry(im, h, e, off, pf, sf, vl);
        const uint32_t kl = live ? pf + sf : 0u;
        if (!live) vl = 0;
        const uint32_t ik = wave_incl_scan32(kl), iv = wave_incl_scan32(vl);
        const uint64_t mk = ko + ik - kl, mv = vo + iv - vl;  // this entry's key / value place
        // (the totals passed the capacity check; a place past a capacity would be a block that
        // changed since the count: such an entry is not written)
        live = live && ei + l < a.out.entry_cap && mk + kl <= a.out.key_cap && mv + vl <= a.out.val_cap;
        if (live) {
          a.out.key_off[ei + l] = uint32_t(mk);
          a.out.val_off[ei + l] = uint32_t(mv);
          a.out.ts[ei + l] = im.u64(off + 4 + sf);
        }
        for (uint32_t r = 0; r < cnt; r += 4) {  // four entries a round, 16 lanes each
          const uint32_t t = r + grp;
          const bool on = __shfl(live ? 1 : 0, t, 64) != 0 && t < cnt;
          const uint32_t xoff = __shfl(off, t, 64), xpf = __shfl(pf, t, 64), xsf = __shfl(sf, t, 64);
          const uint32_t xvl = __shfl(vl, t, 64);
          const uint32_t xk = __shfl(uint32_t(mk), t, 64), xv = __shfl(uint32_t(mv), t, 64);
          if (on) {
            quarter_copy(a.out.keys + xk, im, 4, xpf, sub);  // first_key[..prefix]
            quarter_copy(a.out.keys + xk + xpf, im, xoff + 4, xsf, sub);
            quarter_copy(a.out.vals + xv, im, xoff + 14 + xsf, xvl, sub);
          }
        }
        ei += cnt;
        ko += uint32_t(__builtin_amdgcn_readlane(ik, 63));
        vo += uint32_t(__builtin_amdgcn_readlane(iv, 63));
      }
      return true;
    });
  }
}

// The five scan launches: lsmblk_sst_scan_batch's (kSub false) and, under their own names in the
// kernel log, the table scans of lsmblk_lsm_scan_batch (kSub true).
template <bool kSub>
void launch_scan(const ScanArgs& a, uint32_t qgrid, uint32_t ugrid, bool emit, hipStream_t st) {
  LSM_LAUNCH_NAMED(kSub ? "lsm_scan_sub_bounds_kernel" : "scan_bounds_kernel", scan_bounds_kernel<kSub>, dim3(qgrid),
                   dim3(64 * kGetWaves), 0, st, a);
  LSM_LAUNCH_NAMED(kSub ? "lsm_scan_sub_units_kernel" : "scan_units_kernel", scan_units_kernel<kSub>, dim3(1), dim3(kScanWg), 0,
                   st, a);
  LSM_LAUNCH_NAMED(kSub ? "lsm_scan_sub_count_kernel" : "scan_count_kernel", scan_count_kernel<kSub>, dim3(ugrid),
                   dim3(64 * kGetWaves), 0, st, a);
  LSM_LAUNCH_NAMED(kSub ? "lsm_scan_sub_offsets_kernel" : "scan_offsets_kernel", scan_offsets_kernel<kSub>, dim3(1),
                   dim3(kScanWg), 0, st, a);
  if (emit)
    LSM_LAUNCH_NAMED(kSub ? "lsm_scan_sub_emit_kernel" : "scan_emit_kernel", scan_emit_kernel<kSub>, dim3(ugrid),
                     dim3(64 * kGetWaves), 0, st, a);
}

// ---------------------------------------------------------------- the LSM range scan
// lsmblk_lsm_scan_batch: scan_with_ts for a batch of ranges over an LSM view.
//   lsm_view_check_kernel     the point read's, unchanged
//   lsm_scan_expand_kernel    <false> one wave per range: the tables that pass range_overlap, counted
//                             (L0: every table by its own lane; a level: the span between two k-ary
//                             searches, then every table of the span by its own lane).  <.., true>, a
//                             view with memtable runs: the runs first, each by its lane group, and the
//                             fill pass finds a passing run's slice and writes its scan's result
//   lsm_scan_subs_kernel      one workgroup: sbase = exclusive scan of the counts, the total against
//                             sub_cap -> nsub, the table scans that run (0: refused view, sub_cap short)
//   lsm_scan_expand_kernel    <true> the same walk, writing (range, table) of every table scan
//   lsm_scan_sub_*_kernel     the five scan kernels over the table scans -> the raw stream, run after
//                             run, and sseg = every run's first raw entry (a memtable run's slice: its
//                             bounds are skipped, its sizes are offset differences, its emit one copy)
//   lsm_scan_rank_kernel      the segmented merge: one raw entry per lane, its merge rank among the
//                             runs of its range by a search in every other run -> slot (<true>,
//                             LSMBLK_LSM_SCAN_NEWEST: the rank by (key, ts descending), no ownership)
//   lsm_scan_offsets_kernel   one workgroup: the three-component scan over the slots in merged order,
//                             totals, capacity / overflow, key_off / val_off, seg_start, res
//   lsm_scan_gather_kernel    16 lanes per kept entry: key, value, ts -> out
struct LsmScanArgs : OpenedSet, ViewArgs, BoundArgs {
  const uint64_t* q_ts;  // null: the merged stream itself
  uint64_t nq, sub_cap;
  lsmblk_lsm_scan_result* res;
  DevStream raw;  // the table scans' output, read by the merge
  DevStream out;
  uint32_t* seg_start;
  uint64_t* stats;
  // workspace
  uint32_t* vflag;        // the view check's verdict
  uint64_t* nsub;         // [0] table scans that run
  uint64_t* sstats;       // the table scans' stats (4 words)
  uint32_t* scnt;         // nq: tables per range
  uint32_t* sbase;        // nq + 1: first table scan of every range
  uint32_t* pbad;         // nq: a block on the range's path is malformed
  uint32_t* mcnt;         // nq: merged entries
  uint32_t* sub_q;        // sub_cap: the table scan's range ...
  uint32_t* sub_sst;      // ... and table (nsst + r: memtable run r)
  lsmblk_scan_result* sres;  // sub_cap: the table scans' results (a memtable run's slice is written by the expansion)
  uint32_t* sseg;         // sub_cap + 1: first raw entry of every run
  const uint32_t* sbad;   // sub_cap: the table scans' qbad
  uint32_t* slot;         // slot_cap: merged position -> raw entry + 1 (0: not kept)
  uint32_t* opre;         // slot_cap + 1: kept entries before the merged position
  uint64_t slot_cap;
};

// One wave per range, grid-strided, over the view's tables in priority order; every candidate table
// is tested by its own lane with range_overlap (lsm_storage.rs:142-167) against the descriptor's
// first and last key.  A level's tables are ordered and disjoint (the view check), so the tables
// whose last key lies before the lower bound are a prefix of the level and those whose first key
// lies within the upper bound are one too: a level of more than 64 tables is cut to that span by two
// k-ary searches first.  kFill false: scnt[q] = the passing tables; true: their (range, table) pairs
// from sbase[q] on.
template <bool kFill, bool kMem>
__global__ __launch_bounds__(64 * kGetWaves) void lsm_scan_expand_kernel(LsmScanArgs a) {
  const uint32_t l = lane_id();
  if constexpr (kFill) {
    if (uni64(a.nsub[0]) == 0) return;
  }
  const bool run = uni(*a.vflag) == 0;
  uint32_t err = 0;
  const uint64_t stride = uint64_t(gridDim.x) * kGetWaves;
  for (uint64_t qi = uint64_t(blockIdx.x) * kGetWaves + wave_id(); qi < a.nq; qi += stride) {
    uint32_t cnt = 0;
    const uint32_t base = kFill ? uni(a.sbase[qi]) : 0u;
    do {
      if (!run) break;
      const uint32_t bnd = uni(a.q_bound[qi]);
      const uint32_t lk = bnd & 3, uk = (bnd >> 2) & 3;
      if (lk == 3 || uk == 3) {
        err |= LSMBLK_ERR_SEGMENTS;
        break;
      }
      uint32_t l0 = 0, l1 = 0, u0 = 0, u1 = 0;
      if (lk) {
        l0 = uni(a.lkey_off[qi]);
        l1 = uni(a.lkey_off[qi + 1]);
      }
      if (uk) {
        u0 = uni(a.ukey_off[qi]);
        u1 = uni(a.ukey_off[qi + 1]);
      }
      if ((lk && l1 <= l0) || (uk && u1 <= u0)) {
        err |= LSMBLK_ERR_EMPTY_KEY;
        break;
      }
      const QKey lo = key_upto(a.lkeys, l0, l1), up = key_upto(a.ukeys, u0, u1);
      KeyImage lm{0, 0}, um{0, 0};
      if (lk) lm = image_of(lo);
      if (uk) um = image_of(up);
      // table t's first key against the upper bound, its last key against the lower bound
      auto first_in = [&](uint32_t t) {
        const lsmblk_sst_desc* d = a.desc + t;
        const int c = lane_cmp_img(a.files + d->first_key_pos, d->first_key_len, up, um);
        return uk == LSMBLK_BOUND_EXCLUDED ? c < 0 : c <= 0;
      };
      auto last_before = [&](uint32_t t) {
        const lsmblk_sst_desc* d = a.desc + t;
        const int c = lane_cmp_img(a.files + d->last_key_pos, d->last_key_len, lo, lm);
        return lk == LSMBLK_BOUND_EXCLUDED ? c <= 0 : c < 0;
      };
      // ids[i0 .. i1): each tested by its own lane, the passing ones taken in order
      auto take = [&](const uint32_t* ids, uint32_t i0, uint32_t i1) {
        for (uint32_t c = i0; c < i1; c += 64) {
          const uint32_t i = c + l, t = i < i1 ? ids[i] : kNone;
          bool ok = t < a.nsst && a.desc[t].nblk != 0;  // (the view check refuses any other)
          if (ok && uk) ok = first_in(t);
          if (ok && lk) ok = !last_before(t);
          const uint64_t m = __ballot(ok);
          if constexpr (kFill) {
            const uint64_t x = uint64_t(base) + cnt + uint32_t(__builtin_popcountll(m & ((1ull << l) - 1)));
            if (ok && x < a.sub_cap) {
              a.sub_q[x] = uint32_t(qi);
              a.sub_sst[x] = t;
            }
          }
          cnt += uint32_t(__builtin_popcountll(m));
        }
      };
      // the memtable runs first, each by its own lane group (mem_groups): a run that is not empty passes
      // as a table does, on its first and last key; its table scan is "table" nsst + r
      if constexpr (kMem) {
        const MemArgs mem = mem_keys(a.mem);
        const MemGroups G = mem_groups(mem.nmem);
        bool ok = false;
        uint32_t x0 = 0, x1 = 0;
        if (G.on) {
          x0 = a.mem.start[G.run];
          x1 = a.mem.start[G.run + 1];
          ok = x1 > x0;
          if (ok && uk) {
            const int c = mem_cmp(mem, x0, up, um);
            ok = uk == LSMBLK_BOUND_EXCLUDED ? c < 0 : c <= 0;
          }
          if (ok && lk) {
            const int c = mem_cmp(mem, x1 - 1, lo, lm);
            ok = !(lk == LSMBLK_BOUND_EXCLUDED ? c <= 0 : c < 0);
          }
        }
        const uint64_t m = __ballot(ok && G.sub == 0);  // a bit per passing run, in ordinal order
        if constexpr (kFill) {
          // The slice, as (blk0 = begin, blk1 = end) entry indices of the runs' stream in one "block":
          // two searches over the run by its lane group, the same in every mode.  begin: the first key
          // >= lower (Excluded: > lower, after all its versions); end: the first key at or after begin
          // > upper (Excluded: >= upper).
          const uint64_t x = uint64_t(base) + uint32_t(__builtin_popcountll(m & ((1ull << (G.run << G.lg)) - 1)));
          const bool on = ok && x < a.sub_cap;
          const bool excl = lk == LSMBLK_BOUND_EXCLUDED, strict = uk == LSMBLK_BOUND_EXCLUDED;
          uint32_t b = x0, e = x1;
          if (lk)
            b = group_first_false(G, x0, x1, on, [&](uint32_t i) {
              const int c = mem_cmp(mem, i, lo, lm);
              return excl ? c <= 0 : c < 0;
            });
          if (uk)
            e = group_first_false(G, b, x1, on, [&](uint32_t i) {
              const int c = mem_cmp(mem, i, up, um);
              return strict ? c < 0 : c <= 0;
            });
          if (on && G.sub == 0) {
            a.sub_q[x] = uint32_t(qi);
            a.sub_sst[x] = a.nsst + G.run;
            a.sres[x] = lsmblk_scan_result{LSMBLK_SCAN_EMPTY, b, 0, e, 0, e > b ? 1u : 0u, 0};
          }
        }
        cnt += uint32_t(__builtin_popcountll(m));
      }
      take(a.l0, 0, a.nl0);
      for (uint32_t lv = 0; lv < a.nlevel; ++lv) {
        const uint32_t t0 = uni(a.level_start[lv]), n = uni(a.level_start[lv + 1]) - t0;
        const uint32_t* ls = a.level_sst + t0;
        uint32_t s0 = 0, s1 = n;
        if (n > 64) {
          if (lk) s0 = kary_first_false(0, n, [&](uint32_t i) { return ls[i] < a.nsst && last_before(ls[i]); });
          if (uk) s1 = kary_first_false(s0, n, [&](uint32_t i) { return ls[i] < a.nsst && first_in(ls[i]); });
        }
        take(ls, s0, s1);
      }
    } while (false);
    if constexpr (!kFill) {
      if (l == 0) a.scnt[qi] = cnt;
    }
  }
  if constexpr (!kFill) raise_err(a.stats, err);
}

// sbase = exclusive scan of the ranges' table counts (the share form of the workgroup scan); the
// total is stats[7], and the table scans run only when it fits sub_cap.
__global__ __launch_bounds__(kScanWg) void lsm_scan_subs_kernel(LsmScanArgs a) {
  __shared__ uint64_t wsum[16];
  uint64_t q0, q1;
  share1024(a.nq, q0, q1);
  uint64_t sum = 0, tot;
  for (uint64_t q = q0; q < q1; ++q) sum += a.scnt[q];
  uint64_t o = block_excl1024(sum, wsum, tot);
  const bool fits = tot <= a.sub_cap;  // (sub_cap < 2^31: the positions fit u32)
  for (uint64_t q = q0; q < q1; ++q) {
    a.sbase[q] = fits ? uint32_t(o) : 0u;
    o += a.scnt[q];
  }
  if (threadIdx.x == 0) {
    a.sbase[a.nq] = fits ? uint32_t(tot) : 0u;
    a.nsub[0] = fits ? tot : 0;
    a.stats[7] = tot;
    if (!fits) or_err(a.stats, LSMBLK_ERR_CAPACITY);
  }
}

// The segmented merge.  Work items are 64-entry tiles of the raw stream, one entry per lane, so a
// huge range spreads over as many waves as a batch of small ones.  Entry e is entry i of run r of
// range q; for every other run r' of q a bytewise, ts-agnostic binary search (a shorter key is less)
// gives lb(r') = its entries below key(e) or ub(r') = its entries not above it, and
//   pos = i + sum over r' < r of ub(r') + sum over r' > r of lb(r')
// is e's rank in the stable merge of q's runs by key, a bijection onto q's [0, raw).  e is owned iff
// no r' < r holds its key (lb == ub there): MergeIterator yields exactly the owned entries, keys
// ascending, a key's versions in its owner's order.  The reader's rule needs merged entry pos - 1:
// a key's owned versions are contiguous at the head of its group in merged order (the owner is the
// lowest run holding the key, and ub places every lower run's entries before them), so the merged
// predecessor of an owned entry with the same key is the same run's entry i - 1, and one with
// another key changes nothing in the rule whoever owns it.
//
// kNewest (LSMBLK_LSM_SCAN_NEWEST): the merge by (key ascending, ts descending) instead.  The order
// of raw entry x against e is the key order and, on equal keys, x before e when ts[x] > ts[e]; an
// equal ts is the tie the run order resolves, as an equal key is above.  Every run is sorted by that
// order (the precondition), so lb / ub, the shortcut and the search carry over and pos is e's rank
// in the stable merge by (key, ts descending, run, position), a bijection onto q's [0, raw): every
// entry is merged, nothing is owned.  The reader's rule needs the merged predecessor: the
// entries of run r' before e in merged order are [x0, p), those with e's key are contiguous at the end,
// and p - 1 has the smallest ts of them; the predecessor is the latest of the runs' p - 1 (the own
// run's is e - 1), so it has e's key and a ts <= read_ts -- e is hidden -- iff some run's p - 1 has.
template <bool kNewest>
__global__ __launch_bounds__(256) void lsm_scan_rank_kernel(LsmScanArgs a) {
  const uint64_t nsub = uni64(a.nsub[0]);
  if (!nsub || (a.sstats[3] & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW))) return;
  const uint64_t nraw = uni(a.sseg[nsub]);
  if (nraw > a.slot_cap) return;  // (a raw stream that passed its capacity check fits the slots)
  const uint32_t l = lane_id();
  const uint64_t tiles = (nraw + 63) / 64, stride = uint64_t(gridDim.x) * 4;
  auto klen = [&](uint64_t x) { return a.raw.key_off[x + 1] - a.raw.key_off[x]; };
  for (uint64_t tile = uint64_t(blockIdx.x) * 4 + wave_id(); tile < tiles; tile += stride) {
    const uint64_t e = tile * 64 + l;
    const bool on = e < nraw;
    uint32_t q = kNone;
    bool owned = false;
    if (on) {
      uint64_t lo = 0, hi = nsub - 1;  // the run: the first r with sseg[r + 1] > e
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.sseg[mid + 1] <= e) lo = mid + 1;
        else hi = mid;
      }
      const uint32_t r = uint32_t(lo);
      q = a.sub_q[r];
      const uint32_t r0 = a.sbase[q], r1 = a.sbase[q + 1];
      const uint8_t* const kp = a.raw.keys + a.raw.key_off[e];
      const uint32_t kl = klen(e);
      // raw key x against the lane's own: images first (independent loads, one round trip)
      const KeyImage km = image_of_bytes(kp, kl);
      auto cmp_key = [&](uint64_t x) {
        const uint8_t* const xp = a.raw.keys + a.raw.key_off[x];
        const uint32_t xl = klen(x);
        return image_byte_cmp(image_of_bytes(xp, xl), KeyPtr{xp, xl}, km, KeyPtr{kp, kl});
      };
      // the reader's rule on e and its own run's predecessor
      auto own_rule = [&](uint64_t read_ts) {
        bool k = a.raw.ts[e] <= read_ts && a.raw.val_off[e + 1] > a.raw.val_off[e];
        if (k && e > a.sseg[r] && a.raw.ts[e - 1] <= read_ts)
          k = byte_cmp(KeyPtr{a.raw.keys + a.raw.key_off[e - 1], klen(e - 1)}, KeyPtr{kp, kl}) != 0;
        return k;
      };
      uint64_t ets = 0, snap_ts = 0;
      bool vis = true;  // kNewest: e passes the reader's rule as far as the runs seen tell
      if constexpr (kNewest) {
        ets = a.raw.ts[e];
        if (a.q_ts) {
          snap_ts = a.q_ts[q];
          vis = own_rule(snap_ts);
        }
      }
      auto cmp = [&](uint64_t x) {
        int c = cmp_key(x);
        if constexpr (kNewest) {
          if (c == 0) {
            const uint64_t tx = a.raw.ts[x];
            c = tx > ets ? -1 : (tx < ets ? 1 : 0);
          }
        }
        return c;
      };
      uint64_t pos = e - a.sseg[r];
      owned = true;
      for (uint32_t r2 = r0; r2 < r1; ++r2) {
        const uint64_t x0 = a.sseg[r2], x1 = a.sseg[r2 + 1];
        if (r2 == r || x1 <= x0) continue;
        const bool upper = r2 < r;  // ub for the runs before r, lb for those after
        uint64_t p;
        // the run's first and last key first: most runs of a range lie wholly on one side of a key
        const int cf = cmp(x0);
        if (cf > 0 || (cf == 0 && !upper)) {
          p = x0;
        } else {
          const int cl = x1 - x0 > 1 ? cmp(x1 - 1) : cf;
          if (cl < 0 || (cl == 0 && upper)) {
            p = x1;
          } else {  // the first x of (x0, x1 - 1] with key(x) > key(e) (ub) / >= key(e) (lb)
            uint64_t s = x0 + 1, t = x1 - 1;
            while (s < t) {
              const uint64_t mid = s + (t - s) / 2;
              const int c = cmp(mid);
              if (c < 0 || (c == 0 && upper)) s = mid + 1;
              else t = mid;
            }
            p = s;
          }
        }
        pos += p - x0;
        if constexpr (kNewest) {
          // (a key-only compare: the order above includes ts)
          if (vis && a.q_ts && p > x0 && cmp_key(p - 1) == 0 && a.raw.ts[p - 1] <= snap_ts) vis = false;
        } else {
          if (upper && p > x0 && cmp(p - 1) == 0) owned = false;
        }
      }
      bool keep = owned;
      if constexpr (kNewest) keep = vis;
      else if (keep && a.q_ts) keep = own_rule(a.q_ts[q]);
      const uint64_t at = uint64_t(a.sseg[r0]) + pos;
      if (at < nraw) a.slot[at] = keep ? uint32_t(e) + 1 : 0u;
    }
    // merged entries: a tile's lanes are in raw order, so a range's lanes are consecutive; its first
    // lane adds the range's owned lanes (kNewest: all of them)
    const uint64_t om = __ballot(on && owned);
    const uint32_t qp = __shfl_up(q, 1, 64);
    const bool head = on && (l == 0 || qp != q);
    const uint64_t hm = __ballot(head);
    if (head) {
      const uint64_t rest = l == 63 ? 0ull : hm >> (l + 1);
      const uint32_t nxt = rest ? l + 1 + uint32_t(__builtin_ctzll(rest)) : 64u;
      const uint64_t m = (nxt == 64 ? ~0ull : (1ull << nxt) - 1) & ~((1ull << l) - 1);
      const uint32_t c = uint32_t(__builtin_popcountll(om & m));
      if (c) atomicAdd(a.mcnt + q, c);
    }
  }
}

// One workgroup: the ranges' malformed marks, then the three-component exclusive scan (entries, key
// bytes, value bytes) over the slots in merged order in the share form of the workgroup scan, the
// totals and flags, the out offsets, and per range seg_start and res.
__global__ __launch_bounds__(kScanWg) void lsm_scan_offsets_kernel(LsmScanArgs a) {
  __shared__ uint64_t wsum[16][3];
  const uint64_t nsub = a.nsub[0];
  const uint32_t serr = uint32_t(a.sstats[3]);
  const uint64_t nraw = nsub ? a.sseg[nsub] : 0;
  // ranked: the raw stream was written and lsm_scan_rank_kernel ran over it
  const bool ranked = nsub && a.raw.on && !(serr & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW)) && nraw <= a.slot_cap;
  const bool masked = (serr & LSMBLK_ERR_MALFORMED) != 0;
  if (masked)
    for (uint64_t s = threadIdx.x; s < nsub; s += kScanWg)
      if (a.sbad[s]) a.pbad[a.sub_q[s]] = 1;
  __threadfence_block();
  __syncthreads();
  auto qstart = [&](uint64_t q) -> uint64_t { return a.sseg[a.sbase[q]]; };  // q <= nq: sbase[nq] = nsub
  auto first_query = [&](uint64_t i) {  // the last q with qstart(q) <= i
    uint64_t lo = 0, hi = a.nq - 1;
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) / 2;
      if (qstart(mid) <= i) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  };
  uint64_t i0, i1;
  share1024(ranked ? nraw : 0, i0, i1);
  // a slot's entry, 0 when it keeps none; a malformed range's slots are cleared on the way
  uint64_t q = masked && i0 < i1 ? first_query(i0) : 0;
  uint64_t sum[3] = {0, 0, 0}, tot[3], base[3];
  for (uint64_t i = i0; i < i1; ++i) {
    uint32_t s = a.slot[i];
    if (masked) {
      while (q + 1 < a.nq && qstart(q + 1) <= i) ++q;
      if (a.pbad[q]) s = 0;
    }
    if (s > nraw) s = 0;
    if (s != a.slot[i]) a.slot[i] = s;
    if (s) {
      sum[0] += 1;
      sum[1] += a.raw.key_off[s] - a.raw.key_off[s - 1];
      sum[2] += a.raw.val_off[s] - a.raw.val_off[s - 1];
    }
  }
  block_excl1024<3>(sum, wsum, base, tot);
  const bool fits = a.out.on && tot[0] <= a.out.entry_cap && tot[1] <= a.out.key_cap && tot[2] <= a.out.val_cap &&
                    tot[0] <= 0xFFFFFFFFull && tot[1] <= 0xFFFFFFFFull && tot[2] <= 0xFFFFFFFFull;
  for (uint64_t i = i0; i < i1; ++i) {
    const uint32_t s = a.slot[i];
    a.opre[i] = uint32_t(base[0]);
    if (s) {
      if (fits) {
        a.out.key_off[base[0]] = uint32_t(base[1]);
        a.out.val_off[base[0]] = uint32_t(base[2]);
      }
      base[0] += 1;
      base[1] += a.raw.key_off[s] - a.raw.key_off[s - 1];
      base[2] += a.raw.val_off[s] - a.raw.val_off[s - 1];
    }
  }
  if (threadIdx.x == 0) {
    if (ranked) a.opre[nraw] = uint32_t(tot[0]);
    const TotalCaps caps = a.out.on ? TotalCaps{a.out.entry_cap, a.out.key_cap, a.out.val_cap} : TotalCaps{~0ull, ~0ull, ~0ull};
    publish_totals(a.stats, tot, caps, a.out.on ? a.out.key_off : nullptr, a.out.on ? a.out.val_off : nullptr, kSentIfClean, 0,
                   /*ovf_entries=*/true);
    or_err(a.stats, serr);
    for (uint32_t k = 0; k < 3; ++k) a.stats[4 + k] = a.sstats[k];
  }
  __threadfence_block();
  __syncthreads();  // opre is written
  for (uint64_t p = threadIdx.x; p <= a.nq; p += kScanWg) {
    if (p == a.nq) {
      a.seg_start[p] = ranked ? uint32_t(tot[0]) : 0u;
      break;
    }
    lsmblk_lsm_scan_result r{LSMBLK_SCAN_EMPTY, 0, 0, 0, 0};
    uint32_t st = 0;
    if (nsub && !a.pbad[p]) {
      r.sources = a.sbase[p + 1] - a.sbase[p];
      r.raw = qstart(p + 1) - qstart(p);
    }
    if (ranked) {
      st = a.opre[qstart(p)];
      r.n = a.opre[qstart(p + 1)] - st;
      if (!a.pbad[p]) r.merged = a.mcnt[p];
      if (r.n) r.status = LSMBLK_SCAN_OK;
    }
    a.seg_start[p] = st;
    a.res[p] = r;
  }
}

// len bytes src -> dst by the 16 lanes of a quarter wave (sub = lane & 15), any alignment: 16-B
// pieces, then the last partial piece one byte per lane (quarter_copy's shape over global memory).
__device__ __forceinline__ void quarter_copy_glb(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t sub) {
  const uint32_t full = len & ~15u;
  for (uint32_t o = 16 * sub; o < full; o += 256) *reinterpret_cast<u32x4*>(dst + o) = *reinterpret_cast<const u32x4*>(src + o);
  const uint32_t x = full + sub;
  if (x < len) dst[x] = src[x];
}

// A quarter wave per merged position, grid-strided: a kept entry's key, value and ts to its place.
__global__ __launch_bounds__(256) void lsm_scan_gather_kernel(LsmScanArgs a) {
  if (a.stats[3] & (LSMBLK_ERR_CAPACITY | LSMBLK_ERR_OVERFLOW)) return;
  const uint64_t nsub = a.nsub[0];
  const uint64_t nraw = nsub ? a.sseg[nsub] : 0;
  if (nraw > a.slot_cap) return;
  const uint32_t sub = threadIdx.x & 15;
  const uint64_t stride = uint64_t(gridDim.x) * 16;
  for (uint64_t i = uint64_t(blockIdx.x) * 16 + (threadIdx.x >> 4); i < nraw; i += stride) {
    const uint32_t s = a.slot[i];
    if (!s || s > nraw) continue;
    const uint64_t e = s - 1, oi = a.opre[i];
    if (oi >= a.out.entry_cap) continue;
    const uint32_t kl = a.raw.key_off[e + 1] - a.raw.key_off[e], vl = a.raw.val_off[e + 1] - a.raw.val_off[e];
    const uint32_t ko = a.out.key_off[oi], vo = a.out.val_off[oi];
    // (the totals passed the capacity check: a place past a capacity is not written)
    if (uint64_t(ko) + kl > a.out.key_cap || uint64_t(vo) + vl > a.out.val_cap) continue;
    quarter_copy_glb(a.out.keys + ko, a.raw.keys + a.raw.key_off[e], kl, sub);
    quarter_copy_glb(a.out.vals + vo, a.raw.vals + a.raw.val_off[e], vl, sub);
    if (sub == 0) a.out.ts[oi] = a.raw.ts[e];
  }
}

// ---------------------------------------------------------------- host: what the entry points share
// The argument checks (true: LSMBLK_E_INVAL), made before the context is locked.  The opened set:
// files and index 16-B aligned, and its arrays given when the call reads them.
bool bad_opened(const OpenedSet& o, bool read) {
  return (read && o.nsst && (!o.files || !o.file_off || !o.desc)) || (reinterpret_cast<uintptr_t>(o.files) & 15) ||
         (reinterpret_cast<uintptr_t>(o.index) & 15);
}
bool bad_view(const lsmblk_lsm_view* v) {
  if (!v || (v->nl0 && !v->l0) || (v->nlevel && (!v->level_start || !v->level_sst)) ||
      uint64_t(v->nl0) + v->nlevel + v->nmem >= 0xFFFFFFFFull || v->nmem > kMaxMem)
    return true;
  const lsmblk_kv_stream* m = v->mem;
  return v->nmem && (!m || !v->mem_start || !m->keys || !m->key_off || !m->vals || !m->val_off || !m->ts);
}
bool bad_stream(const lsmblk_kv_stream* s) {  // (an absent stream is fine)
  return s && (!s->key_off || !s->val_off || (s->entry_cap && !s->ts) || (s->key_cap && !s->keys) || (s->val_cap && !s->vals));
}
ViewArgs view_args(const lsmblk_lsm_view* v) {
  ViewArgs a{v->l0, v->nl0, v->nlevel, v->level_sst, v->level_start, MemArgs{}};
  if (v->nmem) a.mem = MemArgs{v->mem->keys, v->mem->key_off, v->mem->vals, v->mem->val_off, v->mem->ts, v->mem->n, v->mem_start, v->nmem, 0};
  return a;
}

// The first entry of an offsets array (or of both of a stream's) zeroed: an empty batch's result.
bool zero_first(uint32_t* off, hipStream_t st) { return !off || hipMemsetAsync(off, 0, 4, st) == hipSuccess; }
bool zero_first(const lsmblk_kv_stream* s, hipStream_t st) { return !s || (zero_first(s->key_off, st) && zero_first(s->val_off, st)); }

// Grid of a grid-strided kernel that takes `per` items per workgroup: at most 8 workgroups per CU.
struct GridCap {
  uint64_t cap;
  explicit GridCap(const lsmblk_ctx* c) {
    const int cus = cu_count(c);
    cap = uint64_t(cus > 0 ? cus : 256) * 8;
  }
  uint32_t operator()(uint64_t items, uint64_t per) const {
    const uint64_t w = (items + per - 1) / per;
    return uint32_t(w < 1 ? 1 : (w < cap ? w : cap));
  }
};

// lsmblk_sst_open_batch's workspace: the CRC range table, the CRCs, the CRC pass's own stats.
struct OpenWs {
  uint64_t* tab;
  uint32_t* crc;
  uint64_t* cstats;
  uint64_t bytes;
};
OpenWs open_ws(uint8_t* base, uint64_t nsst) {
  Carve cv{base};
  OpenWs w;
  w.tab = cv.take<uint64_t>(4 * nsst + 1);
  w.crc = cv.take<uint32_t>(4 * nsst);
  w.cstats = cv.take<uint64_t>(32);
  w.bytes = cv.off;
  return w;
}

// The scan kernels' workspace for nq scans spread over nq + budget units: ubase | qbad | hdr | ucnt.
void scan_regions(Carve& cv, ScanArgs& a, uint64_t nq, uint64_t budget) {
  a.ubase = cv.take<uint32_t>(nq + 1);
  a.qbad = cv.take<uint32_t>(nq);
  a.hdr = cv.take<uint64_t>(32);
  a.ucnt = cv.take<uint64_t>(3 * (nq + budget));
  a.budget = uint32_t(budget);
}
// lsmblk_sst_scan_batch's workspace, sized by nq and the unit budget alone: a's regions; its size.
uint64_t scan_ws(uint8_t* base, ScanArgs& a, uint64_t nq, uint64_t budget) {
  Carve cv{base};
  scan_regions(cv, a, nq, budget);
  return cv.off;
}

// lsmblk_lsm_scan_batch's workspace, sized by nq, sub_cap, the unit budget and raw's entry capacity
// alone: the regions of a and of the table scans s (s.qbad is a.sbad), and
//   head (vflag, nsub, the table scans' stats) | pbad | mcnt | scnt | sbase | sub_q | sub_sst | sseg | table scan
//   results | the scan kernels' ubase | qbad | hdr | ucnt | slot | opre
struct LsmScanWs {
  uint64_t* head;
  lsmblk_scan_result* sres;
  uint64_t zero_end;  // head, pbad and mcnt start from zero
  uint64_t bytes;
};
LsmScanWs lsm_scan_ws(uint8_t* base, LsmScanArgs& a, ScanArgs& s, uint64_t budget) {
  Carve cv{base};
  LsmScanWs w;
  w.head = cv.take<uint64_t>(32);
  a.pbad = cv.take<uint32_t>(a.nq);
  a.mcnt = cv.take<uint32_t>(a.nq);
  w.zero_end = cv.off;
  a.scnt = cv.take<uint32_t>(a.nq);
  a.sbase = cv.take<uint32_t>(a.nq + 1);
  a.sub_q = cv.take<uint32_t>(a.sub_cap);
  a.sub_sst = cv.take<uint32_t>(a.sub_cap);
  a.sseg = cv.take<uint32_t>(a.sub_cap + 1);
  w.sres = a.sres = cv.take<lsmblk_scan_result>(a.sub_cap);
  scan_regions(cv, s, a.sub_cap, budget);
  a.sbad = s.qbad;
  a.slot = cv.take<uint32_t>(a.slot_cap);
  a.opre = cv.take<uint32_t>(a.slot_cap + 1);
  w.bytes = cv.off;
  return w;
}

// The values of a point-read call's FOUND lookups: their offsets, then the bytes.
template <class Args>
void launch_values(const Args& a, const GridCap& grid, hipStream_t st) {
  LSM_LAUNCH_NAMED("val_scan_kernel", val_scan_kernel<Args>, dim3(1), dim3(1024), 0, st, a);
  LSM_LAUNCH_NAMED("val_gather_kernel", val_gather_kernel<Args>, dim3(grid(a.nq, 4)), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

int lsmblk_sst_open_batch(lsmblk_ctx* c, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                          lsmblk_sst_desc* desc, lsmblk_sst_index* index, uint64_t index_cap, uint64_t* stats,
                          void* stream) {
  if (!c || !stats || bad_opened(OpenedSet{files, file_off, nsst, desc, index}, true) || (index_cap && !index) ||
      nsst > 0x3FFFFFFFu)
    return LSMBLK_E_INVAL;
  CallGuard call(c, stream, stats, LSMBLK_STATS_WORDS);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  if (nsst == 0) return LSMBLK_OK;
  int rc;
  if ((rc = lsmblk_impl::ensure_crc_tabs(c, st))) return rc;
  if ((rc = c->sws.grow(st, open_ws(nullptr, nsst).bytes, 1))) return rc;
  const OpenWs w = open_ws(c->sws, nsst);
  const OpenArgs a{files, file_off, nsst, desc, index, index_cap, w.tab, w.crc, stats};
  if (hipMemsetAsync(w.cstats, 0, 32, st) != hipSuccess) return LSMBLK_E_HIP;
  LSM_LAUNCH(sst_open_prep_kernel, dim3(1), dim3(1024), 0, st, a);
  // (the ranges between the sections are flagged in cstats, which nothing reads)
  if ((rc = lsmblk_impl::launch_crc(c, files, a.tab, 4ull * nsst, 0, w.crc, w.cstats, st, nullptr, true))) return rc;
  LSM_LAUNCH(sst_open_walk_kernel, dim3(nsst), dim3(64), 0, st, a);
  return launch_rc();
}

int lsmblk_sst_get_batch(lsmblk_ctx* c, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                         const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const uint32_t* q_sst,
                         const uint8_t* qkeys, const uint32_t* qkey_off, const uint64_t* q_ts, uint64_t nq,
                         uint32_t flags, lsmblk_get_result* res, uint8_t* vals, uint64_t val_cap, uint32_t* val_off,
                         uint64_t* stats, void* stream) {
  if (!c || !stats || (flags & ~(LSMBLK_GET_NO_FILTER | LSMBLK_GET_MVCC)) || (vals && !val_off)) return LSMBLK_E_INVAL;
  const OpenedSet o{files, file_off, nsst, desc, index};
  if (nq && (!q_sst || !qkey_off || !q_ts || !res)) return LSMBLK_E_INVAL;
  if (bad_opened(o, nq != 0) || nq >= 0xFFFFFFFFull) return LSMBLK_E_INVAL;
  CallGuard call(c, stream, stats, LSMBLK_STATS_WORDS);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  if (nq == 0) return !vals || zero_first(val_off, st) ? LSMBLK_OK : LSMBLK_E_HIP;
  const GetArgs a{o, {qkeys, qkey_off, q_ts, nq, flags, vals, val_cap, val_off, stats}, q_sst, res};
  const GridCap grid(c);
  LSM_LAUNCH(sst_get_kernel, dim3(grid(nq, kGetWaves)), dim3(64 * kGetWaves), 0, st, a);
  if (vals) launch_values(a, grid, st);
  return launch_rc();
}

int lsmblk_lsm_get_batch(lsmblk_ctx* c, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                         const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const lsmblk_lsm_view* view,
                         const uint8_t* qkeys, const uint32_t* qkey_off, const uint64_t* q_ts, uint64_t nq,
                         uint32_t flags, lsmblk_lsm_get_result* res, uint8_t* vals, uint64_t val_cap, uint32_t* val_off,
                         uint64_t* stats, void* stream) {
  if (!c || !stats || bad_view(view) || (flags & ~(LSMBLK_GET_MVCC | LSMBLK_LSM_GET_NEWEST)) || (vals && !val_off))
    return LSMBLK_E_INVAL;
  const OpenedSet o{files, file_off, nsst, desc, index};
  if (nq && (!qkey_off || !q_ts || !res)) return LSMBLK_E_INVAL;
  if (bad_opened(o, nq != 0) || nq >= 0xFFFFFFFFull) return LSMBLK_E_INVAL;
  CallGuard call(c, stream, stats, LSMBLK_STATS_WORDS);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  if (nq == 0) return !vals || zero_first(val_off, st) ? LSMBLK_OK : LSMBLK_E_HIP;
  int rc;
  if ((rc = c->sws.grow(st, 256, 1))) return rc;
  if (hipMemsetAsync(c->sws, 0, 256, st) != hipSuccess) return LSMBLK_E_HIP;
  const ViewArgs v = view_args(view);
  uint32_t* const vflag = Carve{c->sws}.take<uint32_t>(64);
  const LsmGetArgs a{o, v, {qkeys, qkey_off, q_ts, nq, flags, vals, val_cap, val_off, stats}, res, vflag};
  const ViewCheckArgs vc{o, v, stats, vflag};
  const GridCap grid(c);
  LSM_LAUNCH(lsm_view_check_kernel, dim3(32), dim3(256), 0, st, vc);
  if (v.mem.nmem)
    LSM_LAUNCH_NAMED("lsm_get_kernel", lsm_get_kernel<true>, dim3(grid(nq, kGetWaves)), dim3(64 * kGetWaves), 0, st, a);
  else
    LSM_LAUNCH_NAMED("lsm_get_kernel", lsm_get_kernel<false>, dim3(grid(nq, kGetWaves)), dim3(64 * kGetWaves), 0, st, a);
  if (vals) launch_values(a, grid, st);
  return launch_rc();
}

int lsmblk_sst_scan_batch(lsmblk_ctx* c, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                          const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const uint32_t* q_sst,
                          const uint8_t* lkeys, const uint32_t* lkey_off, const uint8_t* ukeys, const uint32_t* ukey_off,
                          const uint32_t* q_bound, uint64_t nq, uint32_t flags, lsmblk_scan_result* res,
                          const lsmblk_kv_stream* out, uint32_t* seg_start, uint64_t* stats, void* stream) {
  if (!c || !stats || !seg_start || (flags & ~(LSMBLK_SCAN_NO_FILTER | LSMBLK_SCAN_MVCC))) return LSMBLK_E_INVAL;
  const OpenedSet o{files, file_off, nsst, desc, index};
  if (nq && (!q_sst || !q_bound || !lkey_off || !ukey_off || !res)) return LSMBLK_E_INVAL;
  if (bad_stream(out) || bad_opened(o, nq != 0) || nq > 0x7FFFFFFFull) return LSMBLK_E_INVAL;
  CallGuard call(c, stream, stats, LSMBLK_STATS_WORDS);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  if (nq == 0) return zero_first(seg_start, st) && zero_first(out, st) ? LSMBLK_OK : LSMBLK_E_HIP;
  const uint64_t budget = c->scan_units;
  ScanArgs a{o, {lkeys, lkey_off, ukeys, ukey_off, q_bound}, q_sst, nq, flags, res, dev_stream(out), seg_start, stats};
  int rc;
  if ((rc = c->sws.grow(st, scan_ws(nullptr, a, nq, budget), 1))) return rc;
  scan_ws(c->sws, a, nq, budget);
  const GridCap grid(c);
  launch_scan<false>(a, grid(nq, kGetWaves), grid(nq + budget, kGetWaves), out != nullptr, st);
  return launch_rc();
}

int lsmblk_lsm_scan_batch(lsmblk_ctx* c, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                          const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const lsmblk_lsm_view* view,
                          const uint8_t* lkeys, const uint32_t* lkey_off, const uint8_t* ukeys, const uint32_t* ukey_off,
                          const uint32_t* q_bound, const uint64_t* q_ts, uint64_t nq, uint32_t flags, uint64_t sub_cap,
                          lsmblk_lsm_scan_result* res, const lsmblk_kv_stream* raw, const lsmblk_kv_stream* out,
                          uint32_t* seg_start, uint64_t* stats, void* stream) {
  if (!c || !stats || !seg_start || bad_view(view) || (flags & ~(LSMBLK_SCAN_MVCC | LSMBLK_LSM_SCAN_NEWEST)) || (out && !raw))
    return LSMBLK_E_INVAL;
  const bool newest = (flags & LSMBLK_LSM_SCAN_NEWEST) != 0;  // (implies the corrected landing)
  const OpenedSet o{files, file_off, nsst, desc, index};
  if (nq && (!q_bound || !lkey_off || !ukey_off || !res)) return LSMBLK_E_INVAL;
  if (bad_stream(raw) || bad_stream(out) || bad_opened(o, nq != 0) || nq > 0x7FFFFFFFull || sub_cap > 0x7FFFFFFFull)
    return LSMBLK_E_INVAL;
  CallGuard call(c, stream, stats, LSMBLK_LSM_SCAN_STATS_WORDS);
  if (call.rc) return call.rc;
  hipStream_t st = call.st;
  if (nq == 0) return zero_first(seg_start, st) && zero_first(raw, st) && zero_first(out, st) ? LSMBLK_OK : LSMBLK_E_HIP;
  const uint64_t budget = c->scan_units, units = sub_cap + budget;
  const uint64_t slot_cap = raw ? (raw->entry_cap < 0xFFFFFFFFull ? raw->entry_cap : 0xFFFFFFFFull) : 0;

  // the three argument structs, from the same opened set, view and bounds
  const ViewArgs v = view_args(view);
  const BoundArgs b{lkeys, lkey_off, ukeys, ukey_off, q_bound};
  LsmScanArgs a{o, v, b, q_ts, nq, sub_cap, res, dev_stream(raw), dev_stream(out), seg_start, stats};
  a.slot_cap = slot_cap;
  // the table scans: range_overlap already passed (NO_FILTER), bounds and kinds of the scan's range
  // (their count is on the device: nq_dev; the output stream is raw, its runs' starts sseg)
  ScanArgs s{o, b, nullptr, 0, (newest ? LSMBLK_SCAN_MVCC : flags) | LSMBLK_SCAN_NO_FILTER, nullptr, a.raw};

  int rc;
  if ((rc = c->sws.grow(st, lsm_scan_ws(nullptr, a, s, budget).bytes, 1))) return rc;
  const LsmScanWs w = lsm_scan_ws(c->sws, a, s, budget);
  if (hipMemsetAsync(c->sws, 0, w.zero_end, st) != hipSuccess) return LSMBLK_E_HIP;
  // (a slot no entry ranks to -- only files that are not in key order leave one -- keeps nothing)
  if (slot_cap && hipMemsetAsync(a.slot, 0, 4 * slot_cap, st) != hipSuccess) return LSMBLK_E_HIP;
  a.vflag = reinterpret_cast<uint32_t*>(w.head);
  a.nsub = w.head + 1;
  a.sstats = w.head + 4;
  const ViewCheckArgs vc{o, v, stats, a.vflag};
  s.q_sst = a.sub_sst;
  s.res = w.sres;
  s.seg_start = a.sseg;
  s.stats = a.sstats;
  s.nq_dev = a.nsub;
  s.parent = a.sub_q;
  s.mem = v.mem;

  const GridCap grid(c);
  LSM_LAUNCH(lsm_view_check_kernel, dim3(32), dim3(256), 0, st, vc);
  // (a view without memtable runs runs the forms that hold nothing of them, under the same names)
  if (v.mem.nmem)
    LSM_LAUNCH_NAMED("lsm_scan_expand_count_kernel", (lsm_scan_expand_kernel<false, true>), dim3(grid(nq, kGetWaves)),
                     dim3(64 * kGetWaves), 0, st, a);
  else
    LSM_LAUNCH_NAMED("lsm_scan_expand_count_kernel", (lsm_scan_expand_kernel<false, false>), dim3(grid(nq, kGetWaves)),
                     dim3(64 * kGetWaves), 0, st, a);
  LSM_LAUNCH(lsm_scan_subs_kernel, dim3(1), dim3(kScanWg), 0, st, a);
  if (v.mem.nmem)
    LSM_LAUNCH_NAMED("lsm_scan_expand_fill_kernel", (lsm_scan_expand_kernel<true, true>), dim3(grid(nq, kGetWaves)),
                     dim3(64 * kGetWaves), 0, st, a);
  else
    LSM_LAUNCH_NAMED("lsm_scan_expand_fill_kernel", (lsm_scan_expand_kernel<true, false>), dim3(grid(nq, kGetWaves)),
                     dim3(64 * kGetWaves), 0, st, a);
  launch_scan<true>(s, grid(sub_cap, kGetWaves), grid(units, kGetWaves), raw != nullptr, st);
  if (raw && newest)
    LSM_LAUNCH_NAMED("lsm_scan_rank_newest_kernel", lsm_scan_rank_kernel<true>, dim3(grid(slot_cap, 256)), dim3(256), 0, st, a);
  else if (raw)
    LSM_LAUNCH_NAMED("lsm_scan_rank_kernel", lsm_scan_rank_kernel<false>, dim3(grid(slot_cap, 256)), dim3(256), 0, st, a);
  LSM_LAUNCH(lsm_scan_offsets_kernel, dim3(1), dim3(kScanWg), 0, st, a);
  if (out) LSM_LAUNCH(lsm_scan_gather_kernel, dim3(grid(slot_cap, 16)), dim3(256), 0, st, a);
  return launch_rc();
}

}  // extern "C"
