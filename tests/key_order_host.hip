// key_order_host.hip -- the key order of lsmblk_keys.hpp, every template over the host accessor, on
// a CPU against a plain byte loop (tests/test_key_order_host.py builds it with the host sanitizers
// and runs it).  Prints one coverage line; exits 1 at the first mismatch, naming the function, the
// two keys and the lead.
#include "lsmblk_dev.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// ---------------------------------------------------------------- the key family
constexpr uint32_t kBaseLen = 36;                     // two dwords past the image
constexpr uint32_t kLeads = 16;                       // arena leads 0 .. 15
constexpr uint32_t kSlack = 16;                       // bytes after the second key (0 in the exact placement)
constexpr uint32_t kExactLead = 5;                    // the placement whose second key ends the arena
constexpr uint8_t kJunk = 0xA5;                       // lead and slack bytes: never a pad
constexpr uint8_t kSubst[2] = {0x00, 0xFF};           // with base[c] - 1 and base[c] + 1
__host__ uint8_t base_byte(uint32_t i) { return uint8_t(0x20 + 3 * i); }  // no byte repeats, none is 0x00 / 0xFF

typedef std::vector<uint8_t> Key;
Key head(const Key& k, uint32_t n) { return Key(k.begin(), k.begin() + n); }
void put(uint8_t* dst, const Key& k, size_t n) {  // (an empty vector's data() may be null)
  for (size_t i = 0; i < n; ++i) dst[i] = k[i];
}

std::vector<Key> family() {
  Key base;
  for (uint32_t i = 0; i < kBaseLen; ++i) base.push_back(base_byte(i));
  std::vector<Key> f;
  for (uint32_t n = 0; n <= kBaseLen; ++n) f.push_back(head(base, n));
  for (uint32_t c = 0; c < kBaseLen; ++c) {
    const uint8_t vs[4] = {kSubst[0], uint8_t(base[c] - 1), uint8_t(base[c] + 1), kSubst[1]};
    for (uint8_t v : vs) {
      Key k = base;
      k[c] = v;
      uint32_t last = 0;
      for (uint32_t n : {c + 1, c + 2, kBaseLen}) {
        if (n > kBaseLen || n == last) continue;
        f.push_back(head(k, n));
        last = n;
      }
    }
  }
  return f;
}

// ---------------------------------------------------------------- the reference: plain byte loops
int ref_cmp(const Key& x, const Key& y, uint32_t* lcp) {
  const size_t xl = x.size(), yl = y.size();
  uint32_t i = 0;
  while (i < xl && i < yl && x[i] == y[i]) ++i;
  *lcp = i;
  if (i < xl && i < yl) return x[i] < y[i] ? -1 : 1;
  return xl < yl ? -1 : (xl > yl ? 1 : 0);
}
void ref_image(const Key& k, uint64_t* hi, uint64_t* lo) {
  *hi = *lo = 0;
  for (uint32_t j = 0; j < 16; ++j) {
    const uint64_t b = j < k.size() ? k[j] : 0;
    if (j < 8) *hi = (*hi << 8) | b;
    else *lo = (*lo << 8) | b;
  }
}

std::string hex(const Key& k) {
  std::string s;
  char b[4];
  for (uint8_t c : k) {
    snprintf(b, sizeof b, "%02x", c);
    s += b;
  }
  return s.empty() ? "(empty)" : s;
}

struct Counts {
  uint64_t pairs = 0, placements = 0, len_ties = 0, tail_ties = 0, tail_calls = 0, fallback = 0, load16 = 0, past_bound = 0;
};

struct Check {
  const Key &x, &y;
  uint32_t lead;
  [[noreturn]] void fail(const char* fn, long long got, long long want) const {
    printf("MISMATCH %s: got %lld want %lld; x=%s y=%s lead=%u\n", fn, got, want, hex(x).c_str(), hex(y).c_str(), lead);
    exit(1);
  }
  void eq(const char* fn, long long got, long long want) const {
    if (got != want) fail(fn, got, want);
  }
};

// One pair in one arena: `lead` junk bytes, x, y, `slack` junk bytes, a heap allocation of exactly
// that size (the sanitizer sees any read past it).
void check_placement(const Key& x, const Key& y, uint32_t lead, uint32_t slack, Counts& n) {
  const Check C{x, y, lead};
  const uint32_t xl = uint32_t(x.size()), yl = uint32_t(y.size()), px = lead, py = lead + xl, total = lead + xl + yl + slack;
  uint8_t* const arena = static_cast<uint8_t*>(malloc(total ? total : 1));
  memset(arena, kJunk, total);
  put(arena + px, x, xl);
  put(arena + py, y, yl);
  const CpuKeys S{arena, total};
  const KeyRef<CpuKeys> rx{S, px, xl}, ry{S, py, yl};
  const KeyPtr kx{arena + px, xl}, ky{arena + py, yl};
  ++n.placements;

  uint32_t want_lcp;
  const int want = ref_cmp(x, y, &want_lcp);
  const uint32_t m = xl < yl ? xl : yl;

  // the accessor past its bound: zero, as the descriptor gives
  C.eq("CpuKeys::byte past the bound", S.byte(total), 0);
  C.eq("CpuKeys::dw past the bound", S.dw(total), 0);
  if (total) {
    C.eq("CpuKeys::dw across the bound", S.dw(total - 1), arena[total - 1]);
    ++n.past_bound;
  }

  // the difference finder
  const KeyDiff d = key_diff(S, px, xl, py, yl);
  C.eq("key_diff.lcp", d.lcp, want_lcp);
  C.eq("key_diff.order", d.order, want);
  if (want_lcp < m) {
    C.eq("key_diff.w0", (d.w0 >> (8 * (want_lcp & 3))) & 0xFF, x[want_lcp]);
    C.eq("key_diff.w1", (d.w1 >> (8 * (want_lcp & 3))) & 0xFF, y[want_lcp]);
  }
  C.eq("key_cmp", key_cmp(S, px, xl, py, yl), want);

  // the image, from every builder
  uint64_t xh, xo, yh, yo;
  ref_image(x, &xh, &xo);
  ref_image(y, &yh, &yo);
  const KeyImage ix = image_of(S, px, xl), iy = image_of(S, py, yl);
  C.eq("image_of(x).hi", ix.hi, xh), C.eq("image_of(x).lo", ix.lo, xo);
  C.eq("image_of(y).hi", iy.hi, yh), C.eq("image_of(y).lo", iy.lo, yo);
  C.eq("image_of(KeyRef)", image_of(ry) == iy, 1);
  C.eq("image_of_bytes(x)", image_of_bytes(kx.p, xl) == ix, 1);
  C.eq("image_of_bytes(y)", image_of_bytes(ky.p, yl) == iy, 1);
  C.eq("image_of_load16(x)", image_of_load16(arena, total, px, xl) == ix, 1);
  C.eq("image_of_load16(y)", image_of_load16(arena, total, py, yl) == iy, 1);
  for (uint32_t p : {px, py}) (uint64_t(p) + 16 > total ? n.fallback : n.load16) += 1;

  // its order and its storage forms
  uint8_t bx[16] = {0}, by[16] = {0};
  put(bx, x, xl < 16 ? xl : 16);
  put(by, y, yl < 16 ? yl : 16);
  const int mc = memcmp(bx, by, 16), wimg = mc < 0 ? -1 : (mc > 0 ? 1 : 0);
  C.eq("KeyImage::cmp", ix.cmp(iy), wimg);
  C.eq("KeyImage <", ix < iy, wimg < 0);
  C.eq("KeyImage <=", ix <= iy, wimg <= 0);
  C.eq("KeyImage ==", ix == iy, wimg == 0);
  const u32x4 be = ix.be_words(), pr = ix.u64_pair();
  C.eq("be_words", be.x, (uint32_t(bx[0]) << 24) | (bx[1] << 16) | (bx[2] << 8) | bx[3]);
  C.eq("be_words", be.w, (uint32_t(bx[12]) << 24) | (bx[13] << 16) | (bx[14] << 8) | bx[15]);
  C.eq("KeyImage::be round trip", KeyImage::be(be) == ix, 1);
  C.eq("KeyImage::pair round trip", KeyImage::pair(pr) == ix, 1);
  uint64_t mem[2];  // (lsmblk_sst_index: img_hi, img_lo)
  memcpy(mem, &pr, 16);
  C.eq("u64_pair in memory", mem[0] == ix.hi && mem[1] == ix.lo, 1);

  // the image-first compare and its LCP form, with each kind of tail
  const bool tie = wimg == 0, tails = tie && xl > 16 && yl > 16;
  if (tie) (tails ? n.tail_ties : n.len_ties) += 1;
  uint32_t calls = 0;
  C.eq("image_cmp / key_cmp tail", image_cmp(ix, xl, iy, yl, [&] {
         ++calls;
         return key_cmp(S, px + 16, xl - 16, py + 16, yl - 16);
       }), want);
  C.eq("image_cmp / byte_cmp(KeyPtr, KeyPtr) tail", image_cmp(ix, xl, iy, yl, [&] {
         ++calls;
         return byte_cmp(kx.skip(16), ky.skip(16));
       }), want);
  C.eq("image_cmp / byte_cmp(KeyPtr, KeyRef) tail", image_cmp(ix, xl, iy, yl, [&] {
         ++calls;
         return byte_cmp(kx.skip(16), ry.skip(16));
       }), want);
  C.eq("image_byte_cmp(KeyPtr, KeyPtr)", image_byte_cmp(ix, kx, iy, ky), want);
  C.eq("image_byte_cmp(KeyPtr, KeyRef)", image_byte_cmp(ix, kx, iy, ry), want);
  int ord = 7;
  C.eq("image_lcp", image_lcp(ix, xl, iy, yl, ord, [&](int& o) {
         ++calls;
         const KeyDiff t = key_diff(S, px + 16, xl - 16, py + 16, yl - 16);
         o = t.order;
         return t.lcp;
       }), want_lcp);
  C.eq("image_lcp order", ord, want);
  C.eq("tail calls", calls, tails ? 4 : 0);
  n.tail_calls += calls;

  // bytes, equality, prefixes
  C.eq("byte_cmp(KeyPtr, KeyPtr)", byte_cmp(kx, ky), want);
  C.eq("byte_cmp(KeyPtr, KeyRef)", byte_cmp(kx, ry), want);
  C.eq("byte_cmp(KeyRef, KeyRef)", byte_cmp(rx, ry), want);
  C.eq("key_equal", key_equal(kx, ky), want == 0);
  C.eq("has_prefix", has_prefix(kx, ky), want_lcp == yl);
  Key pf(kBaseLen + 1, kJunk);  // a prefix longer than any key, then y
  pf.insert(pf.end(), y.begin(), y.end());
  const uint32_t pfx_off[3] = {0, kBaseLen + 1, kBaseLen + 1 + yl};
  C.eq("has_any_prefix", has_any_prefix(kx, pf.data(), pfx_off, 2), want_lcp == yl);
  C.eq("has_any_prefix (too long only)", has_any_prefix(kx, pf.data(), pfx_off, 1), 0);
  C.eq("has_any_prefix (none)", has_any_prefix(kx, pf.data(), pfx_off, 0), 0);
  free(arena);
}

}  // namespace

int main() {
  const std::vector<Key> F = family();
  Counts n;
  for (const Key& x : F)
    for (const Key& y : F) {
      ++n.pairs;
      for (uint32_t lead = 0; lead < kLeads; ++lead) check_placement(x, y, lead, kSlack, n);
      check_placement(x, y, kExactLead, 0, n);  // y ends the arena
    }
  printf("key_order_host: keys=%zu pairs=%llu placements=%llu len_ties=%llu tail_ties=%llu tail_calls=%llu load16=%llu "
         "fallback=%llu past_bound=%llu skipped=0\n",
         F.size(), (unsigned long long)n.pairs, (unsigned long long)n.placements, (unsigned long long)n.len_ties,
         (unsigned long long)n.tail_ties, (unsigned long long)n.tail_calls, (unsigned long long)n.load16,
         (unsigned long long)n.fallback, (unsigned long long)n.past_bound);
  if (n.pairs != uint64_t(F.size()) * F.size() || n.placements != n.pairs * (kLeads + 1)) return 2;
  if (!n.len_ties || !n.tail_ties || !n.tail_calls || !n.fallback || !n.load16 || !n.past_bound) return 3;
  return 0;
}
