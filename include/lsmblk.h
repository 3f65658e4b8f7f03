/*
 * lsmblk.h -- C ABI of the MI355X-native SSTable block codec (liblsmblk.so).
 *
 * Drop-in boundary for the CrystalAnalyst/Lsm block path (paths relative to the reference
 * repository root).  Two halves:
 *
 *  1. Per-entry API, host-synchronous, mirroring the reference's Rust API one-to-one so that
 *     SsTableBuilder / SsTable / SsTableIterator keep their call shape:
 *       lsmblk_builder_*  <-  BlockBuilder          src/block/builder.rs:37-89
 *       lsmblk_block_*    <-  Block::encode/decode  src/block.rs:14-34
 *       lsmblk_iter_*     <-  BlockIterator         src/block/iterator.rs:37-139
 *     (the reference calls these at src/table/builder.rs:34,55,62,113-114, src/table.rs:232,
 *      src/table/iterator.rs:35,59,64,75-92).  `add` must answer "accepted?" synchronously,
 *     so this half runs on the host CPU inside liblsmblk.so; it is product code, not a
 *     fallback for the batch half.
 *
 *  2. Batch / device API (the HIP kernels, gfx950): whole flush / compaction batches.
 *       lsmblk_decode_batch  replaces the per-block loop  SsTable::read_block -> Block::decode
 *                            -> BlockIterator::next        (src/table.rs:213-233,
 *                                                           src/table/iterator.rs:86-97)
 *       lsmblk_encode_batch  replaces the per-entry loop  SsTableBuilder::add ->
 *                            BlockBuilder::add / finish_block  (src/table/builder.rs:48-65,
 *                                                           112-123), one segment per SST
 *       lsmblk_crc32_batch   the per-block framing checksum  (src/table/builder.rs:120-122,
 *                                                           src/table.rs:226-230)
 *       lsmblk_block_meta_batch  the SST BlockMeta section per segment  (src/table.rs:29-63,
 *                                                           src/table/builder.rs:68-77)
 *       lsmblk_compact_filter_batch  compaction's per-entry keep/drop rules  (src/compact.rs:234-299)
 *     All pointers are DEVICE pointers; calls are asynchronous on `stream` (a hipStream_t
 *     passed as void*; NULL = the default stream).  Concurrency: a context's calls are
 *     serialised by its lock (any host thread) and its device work is ordered on the stream each
 *     call is given; a context's workspace is reused by its next call, so work that must run
 *     concurrently (several streams, several host threads at once) takes one context each.
 *     Every device-side wait is bounded (LSMBLK_E_TIMEOUT) and every data-dependent walk is
 *     bounded by its progress (LSMBLK_E_INTERNAL), so no call can leave a kernel running forever.
 *
 * Errors: every function returns 0 (LSMBLK_OK) or a negative LSMBLK_E_* code.  Where the
 * reference panics (empty key builder.rs:55, empty build :82-83, malformed decode
 * block.rs:25-27) the ABI returns an error code instead.
 *
 * Block format (bit-exact with the reference builder):
 *   entry  = u16 prefix | u16 suffix_len | key[prefix..] | u64 ts | u16 value_len | value
 *   block  = entry* | u16 offset* | u16 num_entries          (all integers big-endian)
 *   prefix = LCP(key, first key of the block); fields use the reference's `as u16` wrap.
 */
#ifndef LSMBLK_H
#define LSMBLK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSMBLK_ABI_VERSION 1

enum {
  LSMBLK_OK = 0,
  LSMBLK_E_INVAL = -1,     /* bad argument: empty key, empty build, bad segment table, misaligned output */
  LSMBLK_E_MALFORMED = -2, /* a block does not parse (the reference would panic); an encode input's offsets decrease */
  LSMBLK_E_CAPACITY = -3,  /* an output buffer is too small; the stats hold the required sizes */
  LSMBLK_E_NOMEM = -4,     /* host or device allocation failed */
  LSMBLK_E_HIP = -5,       /* a HIP runtime call failed */
  LSMBLK_E_TIMEOUT = -6,   /* a device-side look-back wait exceeded its bound (must not happen) */
  LSMBLK_E_OVERFLOW = -7,  /* a batch total does not fit the u32 KV-stream offsets */
  LSMBLK_E_INTERNAL = -8,  /* device self-check failed */
  LSMBLK_E_CHECKSUM = -9,  /* a block's framing CRC does not match (read_block, src/table.rs:228-230) */
};

int lsmblk_abi_version(void);
const char* lsmblk_strerror(int status);

/* ------------------------------------------------------------------ per-entry (host) */
typedef struct lsmblk_builder lsmblk_builder;
typedef struct lsmblk_block lsmblk_block;
typedef struct lsmblk_iter lsmblk_iter;

/* BlockBuilder::new (builder.rs:37-44). NULL on allocation failure. */
lsmblk_builder* lsmblk_builder_new(size_t block_size);
void lsmblk_builder_free(lsmblk_builder* b);
/* BlockBuilder::add (builder.rs:54-73). *accepted = 0 means "block full" (the reference's
 * `false`); LSMBLK_E_INVAL for an empty key (the reference's assert!). */
int lsmblk_builder_add(lsmblk_builder* b, const uint8_t* key, size_t klen, uint64_t ts,
                       const uint8_t* val, size_t vlen, int* accepted);
/* BlockBuilder::is_empty (builder.rs:76-78). */
int lsmblk_builder_is_empty(const lsmblk_builder* b);
/* estimated_size (builder.rs:48-50) == the encoded length finish() will produce. */
size_t lsmblk_builder_estimated_size(const lsmblk_builder* b);
/* build() + Block::encode() (builder.rs:81-89 + block.rs:14-22); the builder is reset to
 * empty as SsTableBuilder::finish_block does (src/table/builder.rs:113). */
int lsmblk_builder_finish(lsmblk_builder* b, uint8_t* out, size_t cap, size_t* len);
/* build() without encode: hands the Block to the caller (refcount 1). */
int lsmblk_builder_build(lsmblk_builder* b, lsmblk_block** out);

/* Block::decode (block.rs:24-34). The returned block is reference counted (the reference
 * shares it as Arc<Block>); iterators hold a reference. */
int lsmblk_block_decode(const uint8_t* buf, size_t len, lsmblk_block** out);
/* Block::encode (block.rs:14-22). */
int lsmblk_block_encode(const lsmblk_block* blk, uint8_t* out, size_t cap, size_t* len);
size_t lsmblk_block_encoded_len(const lsmblk_block* blk);
/* Block { data, offsets } fields (block.rs:7-10). */
int lsmblk_block_data(const lsmblk_block* blk, const uint8_t** data, size_t* len);
int lsmblk_block_offsets(const lsmblk_block* blk, const uint16_t** offsets, size_t* n);
void lsmblk_block_free(lsmblk_block* blk); /* drops one reference */

/* BlockIterator (iterator.rs). seek_to_offset is the CORRECTED inverse of the builder: the
 * 8-byte ts after the key suffix is skipped and returned as the key's ts (the reference
 * reads value_len from the ts bytes, iterator.rs:133-134). */
int lsmblk_iter_create_and_seek_to_first(lsmblk_block* blk, lsmblk_iter** out); /* :66-70 */
int lsmblk_iter_create_and_seek_to_key(lsmblk_block* blk, const uint8_t* key, size_t klen,
                                       lsmblk_iter** out);                         /* :73-77 */
int lsmblk_iter_seek_to_first(lsmblk_iter* it);                                     /* :99-101 */
int lsmblk_iter_seek_to_key(lsmblk_iter* it, const uint8_t* key, size_t klen);      /* :80-94 */
int lsmblk_iter_next(lsmblk_iter* it);                                              /* :104-107 */
int lsmblk_iter_is_valid(const lsmblk_iter* it);                                    /* :59-61 */
/* key() (:51-53): pointer valid until the next seek/next; ts is the entry's timestamp. */
int lsmblk_iter_key(const lsmblk_iter* it, const uint8_t** key, size_t* klen, uint64_t* ts);
int lsmblk_iter_value(const lsmblk_iter* it, const uint8_t** val, size_t* vlen);    /* :55-57 */
void lsmblk_iter_free(lsmblk_iter* it);

/* ------------------------------------------------------------------ batch (device) */
/* SoA KV stream in device memory (the decoded form of a batch of blocks):
 *   keys[key_off[i] .. key_off[i+1]), vals[val_off[i] .. val_off[i+1]), ts[i],  i < n.
 * key_off / val_off hold n+1 entries; arenas are limited to 4 GiB each per batch. */
typedef struct {
  uint8_t* keys;
  uint32_t* key_off;
  uint8_t* vals;
  uint32_t* val_off;
  uint64_t* ts;
  uint64_t n;          /* encode input: number of entries. decode output: ignored */
  uint64_t entry_cap;  /* decode output capacities: entries (key_off/val_off hold cap+1) */
  uint64_t key_cap;    /*   bytes */
  uint64_t val_cap;    /*   bytes */
} lsmblk_kv_stream;

/* Device-side result words (u64[LSMBLK_STATS_WORDS], device memory, written by the call):
 *   decode: [0] entries  [1] key bytes  [2] value bytes  [3] error flags
 *   encode: [0] blocks   [1] out bytes  [2] 0            [3] error flags             */
#define LSMBLK_STATS_WORDS 4
#define LSMBLK_ERR_MALFORMED 1u
#define LSMBLK_ERR_CAPACITY 2u
#define LSMBLK_ERR_OVERFLOW 4u
#define LSMBLK_ERR_TIMEOUT 8u
#define LSMBLK_ERR_SEGMENTS 16u
#define LSMBLK_ERR_INTERNAL 32u
#define LSMBLK_ERR_EMPTY_KEY 64u
#define LSMBLK_ERR_CHECKSUM 128u
/* Map a stats[3] error-flag word (copied to the host) to an LSMBLK_E_* status. */
int lsmblk_stats_status(uint64_t error_flags);

typedef struct lsmblk_ctx lsmblk_ctx;
/* One context per (device, stream user). Holds the look-back / plan workspace. */
int lsmblk_ctx_create(int device, lsmblk_ctx** out);
void lsmblk_ctx_destroy(lsmblk_ctx* ctx);
/* Pre-size the workspace (optional; calls grow it on demand, which synchronizes). */
int lsmblk_ctx_reserve(lsmblk_ctx* ctx, uint64_t max_blocks, uint64_t max_entries,
                       uint64_t max_segments);

/* Diagnostics (timing experiments only; results are WRONG while a skip mask is set):
 *   LSMBLK_DEBUG_POLL_MODE    look-back poll protocol: 0 sc1 loads, 1 + agent acquire,
 *                             2 sc1 first then agent atomic-RMW re-polls (default)
 *   LSMBLK_DEBUG_DECODE_SKIP  decode ablation mask: 1 look-back, 2 keys, 4 values, 8 metadata */
#define LSMBLK_DEBUG_POLL_MODE 0
#define LSMBLK_DEBUG_DECODE_SKIP 1
#define LSMBLK_DEBUG_KERNEL_TIMING 2 /* 1: dispatch start/stop events on every kernel launch */
#define LSMBLK_DEBUG_TWO_PASS_DECODE 3 /* 1: count + tile scan + decode (three launches) instead of the lagged decode (A/B) */
#define LSMBLK_DEBUG_DECODE_LAG 4 /* blocks the lagged decode counts ahead of its decodes (>= 128; default: 40 MiB of
                                     blocks at the batch's mean block size, at most 10240); setting it fixes the lag, 0 restores the default */
#define LSMBLK_DEBUG_DECODE_LAG_BYTES 6 /* the lagged decode's lag in bytes of blocks (default 40 MiB; 0: the lag set by key 4) */
#define LSMBLK_DEBUG_COUNTERS 5 /* 1: the lagged decode records a realtime trace per tile (lsmblk_debug_counters) */
#define LSMBLK_DEBUG_ROT_POISON 7 /* diagnostics builds only (fault injection): 1 = the SST rotation's block-chain levels
                                     get links that do not advance (J(s) = s, S(s) = 0) over a third of the
                                     stream; the rotation must report LSMBLK_E_INTERNAL, never loop */
#define LSMBLK_DEBUG_ENCODE_FUSED 8 /* 1: LSMBLK_ENCODE_SEG_SLOTS with block_size <= 4096 through one launch
                                       that walks and emits at once (encode_fused_kernel; measured slower
                                       than the plan walk + emit launches) */
#define LSMBLK_DEBUG_PLAN_PIPE 9 /* 0: the plan walk's helper waits for each chunk's offsets, then its keys
                                    (two round trips per chunk, the default); 1: pipelined over batches */
#define LSMBLK_DEBUG_EMIT_POISON 10 /* diagnostics builds only (fault injection): 1 = after the plan walk,
                                       every fifth block's first entry is set past its end entry (a
                                       block table with e < s, and e > n at the end); emit must report
                                       LSMBLK_E_INTERNAL and read none of those entries */
#define LSMBLK_DEBUG_SCAN_UNITS 11 /* work units (waves' worth of blocks) lsmblk_sst_scan_batch spreads a batch's
                                      blocks over beyond one per range (default 131072; 0 restores it): with
                                      more blocks than units a unit takes several consecutive blocks */
#define LSMBLK_DEBUG_EMIT_MODE 12 /* bits 0-7, the emit launch of the encode calls: 0 the default, 1 emit_kernel
                                     (persistent waves striding over the blocks), 2 emit_block_kernel (one block
                                     per single-wave workgroup, in dispatch order); same bytes either way (A/B;
                                     environment LSMBLK_EMIT_MODE at context creation).  Bits 8-31: mode 2's
                                     grid clamp in workgroups (0: the default), so that a small batch reaches
                                     the loop over blocks j, j + grid, ... */
int lsmblk_debug_set(lsmblk_ctx* ctx, int key, uint32_t value);
/* The trace of the last lagged decode with LSMBLK_DEBUG_COUNTERS on (n <= 16 + 8 * 32768 words;
 * synchronizes).  Words 16 + 8 t + k, 100 MHz s_memrealtime stamps of 64-block tile t: k = 0 tile
 * finish starts, 1 the tile's bases are published, 2 / 3 its first decoder's base wait begins /
 * ends, 4 its first count starts, 5 its first decoder starts. */
int lsmblk_debug_counters(lsmblk_ctx* ctx, uint64_t* out, uint32_t n);
/* Durations (ms) of the kernels of the last timed decode / encode call on this context:
 * [0] dec_count [1] dec_scan [2] decode [3] plan [4] emit; -1 if not recorded.  Waits for
 * the recorded events. */
#define LSMBLK_KERNELS 5
int lsmblk_ctx_kernel_times(lsmblk_ctx* ctx, float* ms);
/* Every kernel launched on this context since the previous call (or since LSMBLK_DEBUG_KERNEL_TIMING
 * was switched on), summed by kernel name: out[0 .. *n).  The log holds the last 16384 launches;
 * LSMBLK_E_CAPACITY if more were made (or more than cap distinct kernels).  Waits for the events.
 * Diagnostics (bench.py's per-kernel roofline of every config); the log is cleared by the call. */
typedef struct {
  char name[56];
  uint32_t launches;
  float ms;
} lsmblk_kernel_stat;
int lsmblk_ctx_kernel_log(lsmblk_ctx* ctx, lsmblk_kernel_stat* out, uint32_t cap, uint32_t* n);

/* Decode nblk blocks (block b = blocks[blk_off[b] .. blk_off[b+1]), blk_off u64[nblk+1])
 * into the SoA stream `out` (outputs must be 16-byte aligned).  Asynchronous: completion
 * and error flags are in `stats` once the stream reaches this point. */
int lsmblk_decode_batch(lsmblk_ctx* ctx, const uint8_t* blocks, const uint64_t* blk_off,
                        uint64_t nblk, const lsmblk_kv_stream* out, uint64_t* stats,
                        void* stream);

/* Decode of an SST data section as SsTable::read_block reads it (src/table.rs:213-233): block b =
 * blocks[blk_off[b] .. blk_off[b+1] - tail) -- tail = 4 over a framed data section addressed by its
 * BlockMeta offsets (block_len = offset_end - offset - 4), 0 for packed blocks.  With
 * LSMBLK_DECODE_VERIFY_CRC (tail must be 4) the u32 BE after every block is checked against its
 * crc32fast; a mismatch sets LSMBLK_ERR_CHECKSUM ("block checksum mismatched").  blk_ent (device
 * u64[nblk+1], optional) receives every block's first entry index in `out` and then the total, e.g.
 * the run boundaries for lsmblk_merge_batch.  Otherwise as lsmblk_decode_batch. */
#define LSMBLK_DECODE_VERIFY_CRC 1u
int lsmblk_decode_batch_ex(lsmblk_ctx* ctx, const uint8_t* blocks, const uint64_t* blk_off, uint64_t nblk,
                           uint32_t tail, uint32_t flags, const lsmblk_kv_stream* out, uint64_t* blk_ent,
                           uint64_t* stats, void* stream);

/* Encode the SoA stream `in` greedily into blocks of `block_size`, restarting the block
 * packing at every segment start (seg_start u32[nseg+1], seg_start[0] = 0, seg_start[nseg]
 * = in->n, non-decreasing), exactly as one SsTableBuilder per segment would.  Blocks are
 * written tightly packed to `out` (16-byte aligned, out_cap bytes); blk_off (u64, room for
 * blk_cap values) receives nblk+1 offsets.  key_off / val_off must be non-decreasing: an entry whose
 * offsets decrease fails the call with LSMBLK_ERR_MALFORMED and nothing is written. */
int lsmblk_encode_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* seg_start,
                        uint32_t nseg, uint32_t block_size, uint8_t* out, uint64_t out_cap,
                        uint64_t* blk_off, uint64_t blk_cap, uint64_t* stats, void* stream);

/* lsmblk_encode_batch with flags.  LSMBLK_ENCODE_SEG_SLOTS writes every segment -- one SST's data
 * section, as its SsTableBuilder accumulates it (src/table/builder.rs:112-123, without the CRCs) --
 * back to back at its own slot instead of packing all segments together:
 *   slot(s) = (key_off[seg_start[s]] - key_off[seg_start[0]]) + (val_off[seg_start[s]] -
 *             val_off[seg_start[0]]) + 18 * (seg_start[s] - seg_start[0]),
 * an upper bound of the encoded size of the segments before s, so out_cap >= key bytes + value
 * bytes + 18 * n always suffices, and every SST's place is known before the encode runs.  The
 * block bytes are the same as lsmblk_encode_batch's.  seg_out (u64[2 * nseg], required): [2 s] = slot(s),
 * [2 s + 1] = segment s's encoded bytes.  blk_off[b] = where block b starts; a block ends where the
 * next starts unless it is its segment's last (then at seg_out[2 s] + seg_out[2 s + 1]);
 * blk_off[nblk] = the end of the last segment.  stats[1] = the encoded bytes (their sum). */
#define LSMBLK_ENCODE_SEG_SLOTS 1u
/* LSMBLK_ENCODE_FRAMED writes every block followed by its crc32fast as a big-endian u32 -- the SST
 * data section exactly as SsTableBuilder::finish_block builds it (src/table/builder.rs:112-123:
 * the encoded block, then put_u32(crc32(block))).  blk_off[b] = where block b starts; its CRC sits
 * at the block's end, and (without SEG_SLOTS) blk_off[b + 1] = blk_off[b] + block size + 4, so
 * lsmblk_decode_batch_ex(tail = 4, LSMBLK_DECODE_VERIFY_CRC) reads the output as read_block reads
 * the file.  stats[1] counts the CRC bytes too.  With SEG_SLOTS the slot bound is 22 bytes per
 * entry instead of 18 (4 more per block, at most one block per entry) and seg_out[2 s + 1] includes
 * the segment's CRCs.  The CRCs are a pass over the encoded blocks (the streaming CRC kernel of
 * lsmblk_crc32_batch) after emit. */
#define LSMBLK_ENCODE_FRAMED 2u
int lsmblk_encode_batch_ex(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* seg_start,
                           uint32_t nseg, uint32_t block_size, uint32_t flags, uint8_t* out,
                           uint64_t out_cap, uint64_t* blk_off, uint64_t blk_cap, uint64_t* seg_out,
                           uint64_t* stats, void* stream);

/* SST block framing (SURVEY.md §8 f, row 1): crc[b] = crc32fast::hash(block b) for block
 * b = blocks[blk_off[b] .. blk_off[b+1] - tail) -- the checksum SsTableBuilder::finish_block
 * appends after every encoded block as a big-endian u32 (src/table/builder.rs:120-122) and
 * SsTable::read_block verifies before Block::decode (src/table.rs:219-230).  tail = 0 for
 * tightly packed blocks (lsmblk_encode_batch output); tail = 4 over a framed SST data section
 * with blk_off = the BlockMeta offsets plus the meta-section offset (read_block's
 * block_len = offset_end - offset - 4).  CRC-32/ISO-HDLC (reflected 0xEDB88320, init and
 * xorout 0xFFFFFFFF); an empty block's CRC is 0.  stats: [0] blocks [1] bytes spanned
 * [3] error flags (LSMBLK_ERR_MALFORMED: a range is shorter than tail, decreasing, or over
 * 2 GiB; its crc is then 0).  Asynchronous like the calls above. */
int lsmblk_crc32_batch(lsmblk_ctx* ctx, const uint8_t* blocks, const uint64_t* blk_off,
                       uint64_t nblk, uint32_t tail, uint32_t* crc, uint64_t* stats, void* stream);

/* Segment -> block table after an encode: seg_blk[s] (u32[nseg+1]) = index of segment s's
 * first block in the lsmblk_encode_batch output (seg_blk[nseg] = nblk).  Must be called on the
 * same context and stream as that encode, before the next encode on the context; seg_start and
 * enc_stats are the encode's own arguments (device pointers).  After a failed encode every
 * entry is 0.  Asynchronous. */
int lsmblk_encode_segment_blocks(lsmblk_ctx* ctx, const uint32_t* seg_start, uint32_t nseg,
                                 const uint64_t* enc_stats, uint32_t* seg_blk, void* stream);

/* SST BlockMeta sections (SURVEY.md §8 f, row 1): for every segment s (an SST, blocks
 * seg_blk[s] .. seg_blk[s+1]) the bytes BlockMeta::encode_block_meta writes after the SST data
 * section (src/table.rs:29-63, called at src/table/builder.rs:77), as SsTableBuilder produces
 * them: offset = the block's position in the framed data section (every block followed by its
 * u32 CRC, builder.rs:118-122), first/last key = the block's first/last key with ts 0
 * (key.rs:166-169), max_ts = 0, CRC-32 of the section after its u32 count.  The keys are parsed
 * from the blocks themselves.  Block b = blocks[blk_off[b] .. blk_off[b+1] - tail): tail = 0 for
 * packed blocks (encode output), 4 over a framed data section.  Section s is written to
 * meta[meta_off[s] .. meta_off[s+1]) (meta_off u64[nseg+1]; meta_cap >= 16).  stats: [0] nseg
 * [1] bytes required [3] error flags (MALFORMED: a block without entries or whose first/last
 * entry does not parse; CAPACITY: meta_cap too small, stats[1] = required; SEGMENTS: bad
 * seg_blk).  A segment without blocks gets the 16-byte section of an empty meta list (the
 * reference would panic building an empty SST).  Asynchronous. */
int lsmblk_block_meta_batch(lsmblk_ctx* ctx, const uint8_t* blocks, const uint64_t* blk_off,
                            uint64_t nblk, uint32_t tail, const uint32_t* seg_blk, uint32_t nseg,
                            uint8_t* meta, uint64_t meta_cap, uint64_t* meta_off, uint64_t* stats,
                            void* stream);

/* Compaction filter (SURVEY.md §8 f, row 2 -- the per-entry rules of compact_generate_sst,
 * src/compact.rs:234-299) over a MERGED stream `in` (user keys ascending, versions newest
 * first, as MergeIterator yields them).  Keeps every version newer than `watermark` and, of
 * each key's versions at or below it, only the newest -- unless bottom_level and that version
 * is a tombstone (empty value) with no newer version (:244-254), or the key starts with one of
 * the nprefix prefixes (prefixes[prefix_off[f] .. prefix_off[f+1]), device memory;
 * CompactionFilter::Prefix, :264-275).  The kept entries are written in order to `out` (any
 * alignment).  stats: [0] kept entries [1] key bytes [2] value bytes [3] error flags
 * (CAPACITY: out's entry_cap / key_cap / val_cap too small, stats hold the required sizes,
 * nothing written).  SST rotation (:278-289) stays with the encode's segment table.
 * Asynchronous. */
int lsmblk_compact_filter_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, uint64_t watermark,
                                int bottom_level, const uint8_t* prefixes, const uint32_t* prefix_off,
                                uint32_t nprefix, const lsmblk_kv_stream* out, uint64_t* stats,
                                void* stream);

/* Merge modes (lsmblk_merge_batch_ex, lsmblk_compact_opts.merge_mode).  The reference's compact()
 * never merges its inputs with one MergeIterator: every task reads them through
 * TwoMergeIterator(a, b) with a = MergeIterator(L0 SSTs) or SstConcatIterator(upper level) and b =
 * SstConcatIterator(lower level) (src/compact.rs:170-173, 188-196, 206-215).
 *   LSMBLK_MERGE_RUNS       run-priority merge of all runs, the lower level as the LAST run: for every
 *                           user key, all versions of the lowest-index run holding it.  This is what
 *                           the reference's own TwoMergeIterator tests expect (src/tests/week1_day5.rs:
 *                           15-129: test_task1_merge_1..5) and what MergeIterator does
 *                           (merge_iterator.rs:59-184).  Default.
 *   LSMBLK_MERGE_TWO_LEVEL  two_merge_iterator.rs:19-93 exactly as written, with a = MergeIterator over
 *                           runs 0..nrun-2 and b = run nrun-1; it fails week1_day5's merge_3 / merge_4:
 *                           the stream ends with b (an empty b yields nothing; a's keys >= b's last key
 *                           are dropped), and for a key in both, skip_b drops b's 1st, 3rd, ... version
 *                           and the 2nd, 4th, ... come BEFORE a's versions.  Byte-identical to what the
 *                           reference binary's compaction writes for the same inputs.
 *   LSMBLK_MERGE_NEWEST     the snapshot-preserving merge, the write-side counterpart of
 *                           LSMBLK_LSM_GET_NEWEST / LSMBLK_LSM_SCAN_NEWEST: the stable merge of all runs by
 *                           (key ascending bytewise, a shorter key less; ts descending as u64; run index
 *                           ascending; position in the run ascending).  EVERY input entry is in the
 *                           output (stats[0] == in->n; lsmblk_compact_batch: stats[4] == in->n); two
 *                           entries with the same (key, ts) in two runs are both emitted, the lower run
 *                           first -- nothing is deduplicated.  Precondition: every run is in (key
 *                           ascending, ts descending) order, as a builder fed by a memtable flush or a
 *                           compaction writes it; it is checked on run-adjacent pairs (entry g against
 *                           g-1 of the same run), and a key that decreases or an equal key with a larger
 *                           ts reports LSMBLK_ERR_MALFORMED (the output is then unspecified).  The rules,
 *                           the SST rotation and the block packing are those of the other modes; over
 *                           this order "a key's versions newest first" holds across runs, so every
 *                           version above the watermark is kept from whichever run; of a key's versions
 *                           at or below it only the first in merged order (on an equal ts: the lower
 *                           run's); and with bottom_level a tombstone goes, with everything older, only
 *                           when it is at or below the watermark and the key's newest version over ALL
 *                           runs.  A snapshot read (newest = 1) at any read_ts >= watermark returns the
 *                           same rows before and after such a compaction without prefix filters; after a
 *                           LSMBLK_MERGE_RUNS one it need not (a key's versions in the other runs are
 *                           gone).  No reference counterpart: Key's Ord ignores the ts there.
 * DESIGN.md §3 tabulates the input classes on which the modes differ. */
#define LSMBLK_MERGE_RUNS 0u
#define LSMBLK_MERGE_TWO_LEVEL 1u
#define LSMBLK_MERGE_NEWEST 2u

/* k-way merge of sorted runs (SURVEY.md §8 f, row 2) with MergeIterator's semantics
 * (src/iterators/merge_iterator.rs:59-184) = LSMBLK_MERGE_RUNS: run r = entries [run_start[r], run_start[r+1]) of `in`
 * (run_start: device u32[nrun+1], [0] = 0, [nrun] = in->n; 1 <= nrun <= 64), run 0 the highest
 * priority (MergeIterator::create's index 0, e.g. the newest L0 SST).  Heads compare by user key
 * only (src/key.rs:63-81) with the run index breaking ties, and every step advances the other
 * runs' heads equal to the current key (:134-152): for every user key the output holds all the
 * versions of the lowest-index run containing it, in that run's order.  Each run must be sorted
 * by key (the reference's debug_assert :135-138); a merged order that is not reports
 * LSMBLK_ERR_MALFORMED.  The merged stream is written to `out` (any alignment; capacities as
 * for decode).  stats: [0] entries [1] key bytes [2] value bytes [3] error flags (CAPACITY with
 * the required sizes in [0..2]; SEGMENTS: bad run_start, or a key over 65 535 bytes -- the merge
 * tiles hold u16 key lengths, as the block format does).  Asynchronous. */
int lsmblk_merge_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* run_start, uint32_t nrun,
                       const lsmblk_kv_stream* out, uint64_t* stats, void* stream);
/* lsmblk_merge_batch in merge_mode LSMBLK_MERGE_RUNS, LSMBLK_MERGE_TWO_LEVEL (run nrun-1 = b) or
 * LSMBLK_MERGE_NEWEST (every entry, by key / ts descending / run); any other value: LSMBLK_E_INVAL. */
int lsmblk_merge_batch_ex(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* run_start, uint32_t nrun,
                          uint32_t merge_mode, const lsmblk_kv_stream* out, uint64_t* stats, void* stream);

/* SST rotation of compact_generate_sst (src/compact.rs:278-289) over `in`, the stream of entries
 * handed to SsTableBuilder::add (one key's versions newest first): a new SST starts before entry e
 * when the open SST's estimate_size() -- its finished blocks plus a 4-byte CRC each
 * (src/table/builder.rs:105-123) -- is >= target_sst_size and key(e) differs from key(e-1).  The
 * blocks are BlockBuilder's greedy packing of block_size restarted at every SST start, so this
 * is exactly the segment table under which lsmblk_encode_batch reproduces the compaction's SSTs.
 * sst_start (device u32[sst_cap]) receives the nsst SST first entries and then in->n.  stats: [0]
 * nsst [3] error flags (CAPACITY: sst_cap < nsst + 1).  Asynchronous. */
int lsmblk_sst_rotation_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, uint32_t block_size,
                              uint64_t target_sst_size, uint32_t* sst_start, uint32_t sst_cap, uint64_t* stats,
                              void* stream);

/* Options of lsmblk_compact_batch: the compaction rules (src/compact.rs:239-276) and the SST
 * layout (LsmStorageOptions::block_size / target_sst_size, src/lsm_storage.rs:68-94). */
typedef struct {
  uint64_t watermark;          /* LsmMvccInner::watermark() */
  int32_t bottom_level;        /* compact_to_bottom_level: drop tombstones at or below the watermark */
  uint32_t nprefix;            /* CompactionFilter::Prefix filters (device memory) */
  const uint8_t* prefixes;
  const uint32_t* prefix_off;  /* u32[nprefix+1] */
  uint32_t block_size;
  uint32_t merge_mode;         /* LSMBLK_MERGE_RUNS (0), LSMBLK_MERGE_TWO_LEVEL (run nrun-1 = the lower level) or
                                  LSMBLK_MERGE_NEWEST (the snapshot-preserving merge) */
  uint64_t target_sst_size;
} lsmblk_compact_opts;

#define LSMBLK_COMPACT_STATS_WORDS 8
/* compact_generate_sst (src/compact.rs:223-311) on the device for sorted runs already decoded
 * into `in` (run_start as for lsmblk_merge_batch): merge (opts->merge_mode: the run-priority merge,
 * the reference's TwoMergeIterator with the lower level as the last run, or the snapshot-preserving
 * LSMBLK_MERGE_NEWEST) -> keep/drop rules ->
 * SST rotation -> SsTableBuilder block packing.  `kept` receives the entries handed to
 * SsTableBuilder::add (capacities as for decode); the blocks of every SST are written packed to
 * `out` (16-byte aligned) with blk_off (u64[blk_cap], nblk+1 values), as lsmblk_encode_batch writes
 * them; sst_start / sst_blk (u32[sst_cap], sst_cap >= 2) receive each SST's first kept entry / first
 * block, then kept count / nblk.  Per-block CRCs and BlockMeta sections follow from
 * lsmblk_crc32_batch / lsmblk_block_meta_batch with seg_blk = sst_blk.  When nothing is kept the
 * result is zero SSTs (the reference panics building an empty SST).  stats (u64[8]): [0] blocks
 * [1] bytes [2] SSTs [3] error flags [4] merged entries [5] kept entries [6] kept key bytes
 * [7] kept value bytes.  Asynchronous; allocates workspace on the context (~45 B per input entry
 * plus 8 B per entry per rotation level). */
int lsmblk_compact_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* run_start, uint32_t nrun,
                         const lsmblk_compact_opts* opts, const lsmblk_kv_stream* kept, uint8_t* out,
                         uint64_t out_cap, uint64_t* blk_off, uint64_t blk_cap, uint32_t* sst_start,
                         uint32_t* sst_blk, uint32_t sst_cap, uint64_t* stats, void* stream);

/* ------------------------------------------------------------------ key-range sharded compaction (§8 e) */
/* One GPU's share of a compaction split by user-key range over W ranks (SURVEY.md §8 e): the
 * concatenation of every rank's output is byte-identical to the single-stream compact_generate_sst
 * (src/compact.rs:223-311) over all the input, SST boundaries included.  Per rank:
 *   1. lsmblk_compact_merge_batch: merge + rules over the decoded input blocks, keeping only the
 *      keys in [lo, hi) (blocks straddling a splitter are read by both neighbours);
 *   2. the caller appends the halo -- the first lsmblk_shard_halo_entries(block_size) kept entries
 *      of the ranks after this one -- to the kept stream (one small all-gather);
 *   3. lsmblk_shard_rotation_prepare: everything of the SST rotation that does not depend on the
 *      state entering the range (block chains, SST-end function, its powers);
 *   4. lsmblk_shard_rotation_carry: the boundary carry, rank after rank (send/recv of 16 bytes):
 *      carry = {p, D}: the open SST's next block starts at entry p of the receiving rank's range and
 *      the SST's data section (blocks + CRCs) holds D bytes there (D = 0: an SST starts at p);
 *      rank 0 receives {0, 0};
 *   5. lsmblk_shard_encode_batch: this rank's SST cut points and blocks. */
typedef struct {
  const uint8_t* lo;  /* device bytes; used when has_lo */
  const uint8_t* hi;  /* device bytes; used when has_hi (exclusive) */
  uint32_t lo_len, hi_len;
  uint32_t has_lo, has_hi;
} lsmblk_key_range;

/* Halo length: a block that starts before a range end can take at most block_size / 16 entries
 * after it, plus the entry it rejects. */
uint64_t lsmblk_shard_halo_entries(uint32_t block_size);

/* lsmblk_compact_batch's merge + rules + gather, restricted to keys in *range (NULL: all keys;
 * opts->merge_mode must be LSMBLK_MERGE_RUNS here; every mode: lsmblk_compact_merge_batch_ex):
 * kept receives this range's entries handed to SsTableBuilder::add.  stats: [0] kept entries [1] key
 * bytes [2] value bytes [3] error flags [4] merged entries.  Asynchronous. */
int lsmblk_compact_merge_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* run_start, uint32_t nrun,
                               const lsmblk_compact_opts* opts, const lsmblk_key_range* range,
                               const lsmblk_kv_stream* kept, uint64_t* stats, void* stream);

/* The same in every merge mode.  LSMBLK_MERGE_TWO_LEVEL (TwoMergeIterator as written, run nrun-1 = b):
 * the stream ends at b's last key kb over the WHOLE compaction (two_merge_iterator.rs:32-42,60-66), so
 * each range says where kb lies (the caller all-gathers every range's local b-run end):
 *   LSMBLK_TWO_END_IN_RANGE  kb is in this range (or range is NULL): b's local last key is kb;
 *   LSMBLK_TWO_END_ABOVE     the range lies wholly below kb: no cut-off in it;
 *   LSMBLK_TWO_END_BELOW     kb lies below the range, or b is empty everywhere: no a-entry survives;
 * and kept_same (device u8[kept->entry_cap]) receives every kept entry's same_as_last_key of the
 * compact_generate_sst loop (src/compact.rs:279; with the two-level order it is not "same key as the
 * previous kept entry"), which the rotation needs: lsmblk_shard_rotation_prepare_ex.  LSMBLK_MERGE_RUNS and
 * LSMBLK_MERGE_NEWEST: two_end is ignored and kept_same may be NULL. */
#define LSMBLK_TWO_END_IN_RANGE 0u
#define LSMBLK_TWO_END_ABOVE 1u
#define LSMBLK_TWO_END_BELOW 2u
int lsmblk_compact_merge_batch_ex(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* run_start,
                                  uint32_t nrun, const lsmblk_compact_opts* opts, const lsmblk_key_range* range,
                                  uint32_t two_end, const lsmblk_kv_stream* kept, uint8_t* kept_same, uint64_t* stats,
                                  void* stream);

/* Rotation state of one range over `ext` = its n_own kept entries followed by the halo (ext->n
 * entries in all).  flags: LSMBLK_SHARD_LAST when ext ends where the whole compaction's stream ends
 * (the last rank, or a halo that reached the end).  sst_cap bounds the SSTs that start in the range.
 * The state stays on the context until the next prepare: lsmblk_shard_rotation_carry and
 * lsmblk_shard_encode_batch may follow any number of times, each encode using the latest carry (same
 * context, no other compaction call on it in between).  Without LSMBLK_SHARD_LAST the halo must reach
 * the first block start or SST start at or after n_own: a shorter one, and no halo at all
 * (ext->n == n_own) under a carry_in.p below n_own, reports LSMBLK_ERR_SEGMENTS.  Asynchronous. */
#define LSMBLK_SHARD_LAST 1u
int lsmblk_shard_rotation_prepare(lsmblk_ctx* ctx, const lsmblk_kv_stream* ext, uint64_t n_own, uint32_t flags,
                                  uint32_t block_size, uint64_t target_sst_size, uint32_t sst_cap, void* stream);
/* The same with ext_same (device u8[ext->n], two-level merges): every ext entry's same_as_last_key,
 * the range's own from lsmblk_compact_merge_batch_ex's kept_same, the halo's from the ranks that
 * own it.  NULL: "same key as the previous entry" (LSMBLK_MERGE_RUNS, LSMBLK_MERGE_NEWEST: it holds over
 * a (key, ts descending) stream too). */
int lsmblk_shard_rotation_prepare_ex(lsmblk_ctx* ctx, const lsmblk_kv_stream* ext, const uint8_t* ext_same,
                                     uint64_t n_own, uint32_t flags, uint32_t block_size, uint64_t target_sst_size,
                                     uint32_t sst_cap, void* stream);

/* carry_in (device u64[2]) -> carry_out (device u64[2]) for the next rank.  Asynchronous. */
int lsmblk_shard_rotation_carry(lsmblk_ctx* ctx, const uint64_t* carry_in, uint64_t* carry_out, void* stream);

/* The range's segments -- [p, first SST end, ..., last SST start, end), SST cut points of the whole
 * compaction, the first segment continuing the previous rank's open SST when carry_in.D > 0 and the
 * last one continued by the next rank when carry_out.D > 0 -- into seg_start (device u32[seg_cap]:
 * nseg + 1 entry indices of ext) and their blocks, packed, into out / blk_off as lsmblk_encode_batch
 * writes them; seg_blk (u32[seg_cap]) receives every segment's first block.  stats (u64[8]): [0]
 * blocks [1] bytes [2] segments [3] error flags [4] first segment continues [5] last segment
 * continues [6] first entry (carry_in.p) [7] end entry (n_own + carry_out.p; a range wholly inside an
 * earlier rank's block, carry_in.p >= n_own, has no segments and reports the empty span [p, p)).
 * Asynchronous. */
int lsmblk_shard_encode_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* ext, uint8_t* out, uint64_t out_cap,
                              uint64_t* blk_off, uint64_t blk_cap, uint32_t* seg_start, uint32_t* seg_blk,
                              uint32_t seg_cap, uint64_t* stats, void* stream);

/* ------------------------------------------------------------------ memtable (§8 f row 4, host) */
/* MemTable (src/mem_table.rs:55-158): an ordered map keyed by the key bytes only (Key's Ord ignores
 * the ts, src/key.rs:63-81), so put() of a present key replaces the entry; flush() (:131-136) yields
 * the entries in key order -- the flush source the device encoder consumes (lsmblk_encode_batch,
 * then lsmblk_sst_files_batch).  Host memory; every call takes the memtable's lock (see _get). */
typedef struct lsmblk_memtable lsmblk_memtable;
lsmblk_memtable* lsmblk_memtable_new(void);
void lsmblk_memtable_free(lsmblk_memtable* m);
int lsmblk_memtable_put(lsmblk_memtable* m, const uint8_t* key, size_t klen, uint64_t ts, const uint8_t* val,
                        size_t vlen);                                                  /* :113-127 */
/* 1 = found, 0 = absent (:93-99).  *val points into the memtable: valid only while no put of the same
 * key can run (single-writer use); concurrent readers use lsmblk_memtable_get_copy. */
int lsmblk_memtable_get(lsmblk_memtable* m, const uint8_t* key, size_t klen, const uint8_t** val, size_t* vlen,
                        uint64_t* ts);
/* get() that copies the value into val[0 .. cap) under the memtable's lock (safe against concurrent
 * puts).  1 = found, 0 = absent, LSMBLK_E_CAPACITY = cap < *vlen (nothing copied; *vlen, *ts set). */
int lsmblk_memtable_get_copy(lsmblk_memtable* m, const uint8_t* key, size_t klen, uint8_t* val, size_t cap,
                             size_t* vlen, uint64_t* ts);
size_t lsmblk_memtable_len(lsmblk_memtable* m);
size_t lsmblk_memtable_approximate_size(lsmblk_memtable* m);                          /* :154-157 */
/* The entries in key order as a SoA KV stream in host buffers (flush, :131-136); *n / *kbytes /
 * *vbytes report the sizes (LSMBLK_E_CAPACITY when a buffer is too small). */
int lsmblk_memtable_flush(lsmblk_memtable* m, uint8_t* keys, uint32_t* key_off, uint8_t* vals, uint32_t* val_off,
                          uint64_t* ts, uint64_t entry_cap, uint64_t key_cap, uint64_t val_cap, uint64_t* n,
                          uint64_t* kbytes, uint64_t* vbytes);

/* ------------------------------------------------------------------ SST container (§8 f row 3) */
/* Whole SST files as SsTableBuilder::build writes them (src/table/builder.rs:68-98), for the nsst
 * SSTs of an encode or compaction: SST s = blocks [sst_blk[s], sst_blk[s+1]) of (blocks, blk_off)
 * (packed, as lsmblk_encode_batch / lsmblk_compact_batch write them), holding the entries
 * [sst_ent[s], sst_ent[s+1]) of `kv` -- the entries handed to SsTableBuilder::add, whose
 * fingerprint32 hashes fill the bloom filter (:53, src/table/bloom.rs:72-101).  File s =
 * files[file_off[s] .. file_off[s+1]) (file_off: device u64[nsst+1]):
 *   every block followed by its BE u32 crc32fast | BlockMeta section | BE u32 meta_offset |
 *   filter | k | BE u32 crc32fast(filter | k) | BE u32 bloom_offset.
 * sst_blk / sst_ent: device u32[nsst+1].  stats: [0] nsst [1] bytes (required on CAPACITY)
 * [3] error flags.  Synchronizes once (reads the key arena size to bound the workspace). */
int lsmblk_sst_files_batch(lsmblk_ctx* ctx, const uint8_t* blocks, const uint64_t* blk_off, uint64_t nblk,
                           const uint32_t* sst_blk, const uint32_t* sst_ent, uint32_t nsst,
                           const lsmblk_kv_stream* kv, uint8_t* files, uint64_t files_cap, uint64_t* file_off,
                           uint64_t* stats, void* stream);
/* BlockIterator::create_and_seek_to_key (src/block/iterator.rs:73-94) for a batch of point
 * lookups (§8 a row 13): lookup q seeks key qkeys[qkey_off[q] .. qkey_off[q+1]) in block q_blk[q]
 * of (blocks, blk_off, tail as for lsmblk_decode_batch_ex).  idx[q] = the entry index the
 * iterator lands on -- its binary search with ts-agnostic key order, stopping at the first probe
 * that compares equal -- or the block's entry count when the iterator ends invalid.  All device
 * pointers (qkey_off: u32[nq+1], q_blk, idx: u32[nq]).  stats[3]: MALFORMED for a block that does
 * not parse (idx = its entry count), SEGMENTS for a block index out of range.  Asynchronous. */
int lsmblk_seek_batch(lsmblk_ctx* ctx, const uint8_t* blocks, const uint64_t* blk_off, uint64_t nblk, uint32_t tail,
                      const uint8_t* qkeys, const uint32_t* qkey_off, const uint32_t* q_blk, uint64_t nq,
                      uint32_t* idx, uint64_t* stats, void* stream);
/* farmhash::fingerprint32 (the key hash of SsTableBuilder::add, src/table/builder.rs:53), host. */
uint32_t lsmblk_fingerprint32(const uint8_t* key, size_t klen);
/* Bloom::may_contain (src/table/bloom.rs:104-120) over a decoded filter, host. */
int lsmblk_bloom_may_contain(const uint8_t* filter, size_t nbytes, uint32_t k, uint32_t h);

/* ------------------------------------------------------------------ SST point lookups (device) */
/* The read side's point read: key_within -> bloom.may_contain(fingerprint32(key))
 * -> SsTable::find_block_idx -> read_block -> BlockIterator::create_and_seek_to_key, for batches of
 * (sst, key, read_ts) lookups over SST files resident in device memory, laid out as
 * lsmblk_sst_files_batch writes them: file s = files[file_off[s] .. file_off[s+1]).  `files` and
 * `index` must be 16-byte aligned (LSMBLK_E_INVAL otherwise).  The files are opened once (lsmblk_sst_open_batch: descriptors and a block
 * index in caller-provided device buffers), then any number of lookup batches run over them
 * (lsmblk_sst_get_batch).
 * Not part of these calls: the per-block CRC of read_block (src/table.rs:226-230) -- callers verify
 * a loaded file with lsmblk_crc32_batch or lsmblk_decode_batch_ex(LSMBLK_DECODE_VERIFY_CRC) -- and
 * merging results across SSTs or levels (the caller orders its candidate SSTs; lsmblk_lsm_get_batch
 * below is the read over a whole LSM view). */

/* One opened SST (64 bytes).  Positions are absolute byte offsets in `files` unless noted. */
typedef struct {
  uint32_t blk0;          /* index of the SST's first record in the block index (its slots are reserved
                             by the block count its BlockMeta section claims, also when the open fails) */
  uint32_t nblk;          /* blocks; 0 after a failed open (lookups then report LSMBLK_GET_ABSENT) */
  uint32_t meta_offset;   /* file-relative start of the BlockMeta section = end of the data section */
  uint32_t bloom_len;     /* bytes of the bloom filter's bit array (without k and the CRC) */
  uint64_t bloom_pos;     /* the bit array (= bloom_offset) */
  uint64_t first_key_pos; /* first key of the first block (SsTable::first_key), in the BlockMeta section */
  uint64_t last_key_pos;  /* last key of the last block (SsTable::last_key) */
  uint32_t first_key_len;
  uint32_t last_key_len;
  uint64_t max_ts;        /* the BlockMeta section's max_ts */
  uint32_t bloom_k;       /* probes per key (the byte after the bit array) */
  uint32_t err;           /* LSMBLK_ERR_* flags of this SST's open; 0 = opened */
} lsmblk_sst_desc;

/* One block of an opened SST (32 bytes; record blk0 + b is the SST's block b).  img_hi / img_lo are
 * the first key's leading 16 bytes as two big-endian integers (bytes 0..7, 8..15; a shorter key is
 * padded with zero bytes): img(a) < img(b) implies a < b in key order, equal images decide nothing. */
typedef struct {
  uint64_t img_hi, img_lo;
  uint32_t off;           /* file-relative start of the block */
  uint32_t end;           /* file-relative end of the framed block: the next block's offset, or meta_offset
                             (read_block, src/table.rs:215-220); the block's bytes are [off, end - 4) */
  uint32_t key_pos;       /* file-relative position of the block's first key in the BlockMeta section */
  uint32_t key_len;
} lsmblk_sst_index;

/* SsTable::open (src/table.rs:162-186) for nsst files: per SST the footer (bloom_offset = the last 4
 * bytes, meta_offset = the 4 bytes before the bloom section), the CRC of the bloom section
 * (bloom.rs:49-60) and of the BlockMeta section (table.rs:65-93), then the walk over the BlockMeta
 * records -> desc[s] and index[desc[s].blk0 ..).  Every offset read from a file is checked against
 * the file's bounds before it is used; per SST, desc[s].err holds
 *   LSMBLK_ERR_MALFORMED  a footer or record points outside its file or section, block offsets do
 *                         not increase, or the SST has no block (the reference unwrap()s and panics)
 *   LSMBLK_ERR_CHECKSUM   a section's CRC does not match
 * and the other SSTs of the batch still open.  stats: [0] SSTs opened  [1] index records reserved
 * (the required index_cap on CAPACITY)  [2] the OR of every desc[s].err  [3] error flags of the
 * call as a whole: CAPACITY (index_cap too small: no SST is opened; index may be NULL with
 * index_cap 0 to ask for the size), MALFORMED (file_off decreases), OVERFLOW (over 2^32 - 1
 * blocks).  desc: device lsmblk_sst_desc[nsst].  Asynchronous. */
int lsmblk_sst_open_batch(lsmblk_ctx* ctx, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                          lsmblk_sst_desc* desc, lsmblk_sst_index* index, uint64_t index_cap, uint64_t* stats,
                          void* stream);

/* Result of one lookup (40 bytes). */
typedef struct {
  uint32_t status;   /* LSMBLK_GET_* */
  uint32_t blk, ent; /* where SsTableIterator::seek_to_key_inner (src/table/iterator.rs:56-68) leaves the
                        iterator: SST-local block and entry; blk == nblk (ent 0): it ended invalid;
                        0xFFFFFFFF both: no seek was made */
  uint32_t hit_blk, hit_ent; /* the visible version (FOUND, TOMBSTONE); else 0xFFFFFFFF */
  uint32_t vlen;     /* its value's bytes */
  uint64_t ts;       /* its timestamp */
  uint64_t val_pos;  /* absolute offset of its value bytes in `files` */
} lsmblk_get_result;

#define LSMBLK_GET_ABSENT 0u    /* the iterator ended invalid, landed on another key, or the key has no
                                   version with ts <= read_ts from the landing on */
#define LSMBLK_GET_FOUND 1u
#define LSMBLK_GET_TOMBSTONE 2u /* the visible version's value is empty (get_with_ts returns None,
                                   src/lsm_storage.rs:435-438) */
#define LSMBLK_GET_RANGE_OUT 3u /* key_within is false (src/lsm_storage.rs:136-138); no seek */
#define LSMBLK_GET_BLOOM_OUT 4u /* Bloom::may_contain is false (src/table/bloom.rs:104-120, with its
                                   k > 30 -> true and h % (nbits as u32)); no seek */

/* flags.  Default: the reference as written -- block = max(partition_point(first_key <= key) - 1, 0)
 * (table.rs:253-257), BlockIterator::seek_to_key's binary search that stops at the first probe
 * comparing equal (the landing of lsmblk_seek_batch), the spill to entry 0 of the next block when
 * the block iterator ends invalid, then LsmIterator::move_to_key (lsm_iterator.rs:59-86) over that
 * iterator: forward while the key equals the query and ts > read_ts.  With several versions of a
 * key the landing may lie past newer versions, which are then never seen. */
#define LSMBLK_GET_NO_FILTER 1u /* skip key_within and the bloom test: SsTableIterator::create_and_seek_to_key alone */
#define LSMBLK_GET_MVCC 2u      /* the corrected read: land on the first entry in SST order whose key is >=
                                   the query (block found with first_key < key), then follow
                                   SsTableIterator::next to the first version with ts <= read_ts */

/* nq lookups: query q = (q_sst[q], qkeys[qkey_off[q] .. qkey_off[q+1]), q_ts[q]) over the opened set
 * (files, file_off, desc, index as lsmblk_sst_open_batch left them) -> res[q].  With vals != NULL the
 * values of the FOUND queries are gathered in query order: vals[val_off[q] .. val_off[q+1])
 * (val_off: u32[nq+1]; not FOUND: empty); when they exceed val_cap the stats carry CAPACITY, [2]
 * the required bytes, and vals is not written.  stats: [0] lookups  [1] FOUND  [2] value bytes
 * [3] error flags: SEGMENTS (a q_sst >= nsst), EMPTY_KEY (an empty query key), MALFORMED (a block
 * on a lookup's path breaks the decode rules of lsmblk_seek_batch, checked for every entry of the
 * block); those lookups report LSMBLK_GET_ABSENT.  Every walk is bounded by the block's entry count
 * and the SST's block count.  All device pointers (q_sst u32[nq], qkey_off u32[nq+1], q_ts
 * u64[nq]).  Asynchronous. */
int lsmblk_sst_get_batch(lsmblk_ctx* ctx, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                         const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const uint32_t* q_sst,
                         const uint8_t* qkeys, const uint32_t* qkey_off, const uint64_t* q_ts, uint64_t nq,
                         uint32_t flags, lsmblk_get_result* res, uint8_t* vals, uint64_t val_cap,
                         uint32_t* val_off, uint64_t* stats, void* stream);

/* ------------------------------------------------------------------ LSM point reads (device) */
/* LsmStorageInner::get_with_ts (src/lsm_storage.rs:361-439) for a batch of keys over an LSM view of
 * the opened set: the view's memtable runs (none, nmem == 0: the read below the memtables), every L0
 * table in order, per level the one table whose key range holds the key, keep_table (key_within, then
 * the bloom test) on each table, the merge, the reader's view at read_ts,
 * `key == query && !value.is_empty()`.
 *
 * Sources, in priority order (the ordinals below are the tables' with nmem == 0; the memtable runs go
 * first and shift them by nmem, see lsmblk_lsm_view): source i < nl0 is table l0[i] (l0_sstables order = MergeIterator::
 * create's index order); source nl0 + l is level l, whose tables are in key order and do not overlap
 * (SstConcatIterator::check_sst_valid, src/iterators/concat_iterator.rs:82-93).  A level's source
 * for a key is the last table of the level with first_key <= key, which must then pass
 * key <= last_key and the bloom test like an L0 table; a key below the level's first table, above
 * its last or in a gap between two tables has no source in that level.
 *
 * The merge is MergeIterator's (LSMBLK_MERGE_RUNS, the default everywhere in this library): Key's
 * Eq / Ord ignore the ts (src/key.rs:63-81), and when MergeIterator::next leaves a key it moves
 * every other source past all of that key's versions.  In closed form: the answer comes from the
 * first source in priority order whose landing entry's key equals the query (the decider); its
 * versions are walked from its landing exactly as lsmblk_sst_get_batch walks them (forward while
 * ts > read_ts), and the result is that lookup's FOUND / TOMBSTONE / ABSENT.  Sources after the
 * decider are never consulted, even when the decider holds no visible version and a later source
 * does; a source that lands on another key (a bloom false positive, a key inside the range that the
 * table does not hold) decides nothing; no source on the key: ABSENT.  The as-written
 * TwoMergeIterator nesting of get_with_ts (LSMBLK_MERGE_TWO_LEVEL) is NOT reproduced: it ends with
 * its second iterator, so it yields nothing whenever no level table passes the filter, and differs
 * from the above on about 15 % of random queries. */
typedef struct {            /* all device pointers */
  const uint32_t* l0;           /* u32[nl0]: SST ids, priority order */
  uint32_t nl0;
  uint32_t nlevel;
  const uint32_t* level_sst;    /* u32[level_start[nlevel]]: per level its SST ids in key order */
  const uint32_t* level_start;  /* u32[nlevel+1], [0] = 0, non-decreasing; an empty level is allowed */
  const lsmblk_kv_stream* mem;  /* host struct of device arrays: all memtable runs back to back; mem->n = their entries */
  const uint32_t* mem_start;    /* device u32[nmem+1], the run_start shape: run r = entries [mem_start[r], mem_start[r+1]) */
  uint32_t nmem;                /* 0 .. 64; 0: the view as it was */
} lsmblk_lsm_view;              /* 56 bytes (32 before the memtable runs were appended: LSMBLK_ABI_VERSION is
                                   unchanged, a caller built against the shorter struct must be rebuilt) */

/* The memtable runs of a view (LsmStorageState: memtable, imm_memtables, l0_sstables, levels): the
 * sources get_with_ts / scan_with_ts consult first (src/lsm_storage.rs:369-380, :460-471), as sorted
 * SoA streams in device memory -- what lsmblk_memtable_flush yields, uploaded.
 *   Order      run 0 is the mutable memtable, runs 1 .. the immutable memtables, newest first
 *              (MergeIterator::create's index order, :369-380).
 *   Ordinals   mem run r is source r, L0 table i is source nmem + i, level l is source nmem + nl0 + l.
 *   A run      entries in (key ascending bytewise with a shorter key less, ts descending) order, keys of
 *              1 .. 65535 bytes, values of at most 65535 bytes.  lsmblk_memtable_flush yields such runs
 *              with one entry per key; several versions per key are allowed.  This is NOT checked: for
 *              other runs the result is unspecified, every search and walk bounded by the run's entry count.
 *   Landing    in every mode (flags 0, MVCC, NEWEST) the first entry of the run whose key is >= the query
 *              or the bound: SkipMap::range has no binary-search quirk.  No key-range test, no bloom filter.
 *   Point read, decider rule (flags 0 / LSMBLK_GET_MVCC): the mem runs are consulted first, in order; a
 *              run whose landing is on the key is the decider: its versions are walked forward while
 *              ts > read_ts -> FOUND / TOMBSTONE / ABSENT, and no later source is consulted, even when
 *              the run holds no visible version and a table does.
 *   Point read, LSMBLK_LSM_GET_NEWEST: every mem run and every passing table is searched; the largest
 *              ts <= read_ts wins, the lower ordinal on an equal ts (a memtable beats a table).
 *   A mem hit  src = r, sst = hit_blk = 0xFFFFFFFF, hit_ent = the entry's index in mem, val_pos =
 *              mem->val_off[hit_ent] (an offset into mem->vals, not into files).  seeks counts every source
 *              searched, mem runs included: every mem run up to the decider (all of them when no mem run
 *              decides; NEWEST: all).  bloom_out counts tables only.  The value gather copies mem hits
 *              from mem->vals and table hits from files into one vals / val_off in query order; stats[1]
 *              and stats[2] count both kinds.
 *   Range scan a mem run is a source of range q iff it is not empty and passes range_overlap on its
 *              first and last key (the rule a table passes).  Mem sources come before the L0 tables and
 *              count in res[q].sources, in stats[7] and against sub_cap.  The run's slice: begin = the
 *              run's start (Unbounded), the first entry with key >= k (Included(k)) or with key > k,
 *              after all of k's versions (Excluded(k)); end = the first entry at or after begin with
 *              key > upper (Included) or >= upper (Excluded), the run's end for an unbounded upper.  The
 *              slices are copied into raw with the bytes they have in mem, ordered by range and then by
 *              source; the merge, the reader's view, NEWEST, the capacity contract, seg_start and every
 *              stats word are the ones described below, over those runs.
 *   View check (device, same call, before anything runs): SEGMENTS when mem_start[0] != 0, mem_start
 *              decreases or mem_start[nmem] != mem->n, reported as a bad level_start is: no lookup or
 *              scan runs.
 *   Host       nmem > 64, or nmem > 0 with mem == NULL, mem_start == NULL or a NULL array in mem
 *              (keys, key_off, vals, val_off, ts): LSMBLK_E_INVAL.
 *   No SST     with nmem > 0 and a view that names no table (nl0 == 0, nlevel == 0), nsst == 0 with NULL
 *              files / file_off / desc / index is valid.  With nmem == 0 every rule is what it was. */

/* Result of one key (48 bytes). */
typedef struct {
  uint32_t status;              /* LSMBLK_GET_ABSENT / FOUND / TOMBSTONE */
  uint32_t src, sst;            /* the deciding source's ordinal and SST id (NEWEST: the chosen version's);
                                   0xFFFFFFFF both: no source landed on the key (NEWEST: no visible version) */
  uint32_t hit_blk, hit_ent;    /* as lsmblk_get_result, SST-local; 0xFFFFFFFF unless FOUND / TOMBSTONE */
  uint32_t vlen;
  uint64_t ts, val_pos;
  uint32_t seeks;               /* sources searched (passed key_within and bloom), the decider included */
  uint32_t bloom_out;           /* sources consulted that the bloom test rejected */
} lsmblk_lsm_get_result;

/* flags: 0 = the reference landing per table (lsmblk_sst_get_batch's default) and the decider rule;
 * LSMBLK_GET_MVCC = the corrected landing per table and the decider rule; LSMBLK_GET_NO_FILTER has
 * no meaning across sources (LSMBLK_E_INVAL). */
#define LSMBLK_LSM_GET_NEWEST 4u /* implies the corrected landing; every source that passes its filters is
                                    searched and the result is the version with the largest ts <= read_ts
                                    over all of them (equal ts: the lower source ordinal), a tombstone
                                    giving TOMBSTONE: the snapshot read of a (key asc, ts desc) merge */

/* nq keys: query q = (qkeys[qkey_off[q] .. qkey_off[q+1]), q_ts[q]) over `view` (a host struct of
 * device pointers) of the opened set -> res[q].  vals / val_cap / val_off and stats follow
 * lsmblk_sst_get_batch: [0] lookups (= nq) [1] FOUND [2] value bytes [3] error flags; CAPACITY
 * carries the required bytes and nothing is written to vals; nq == 0 writes val_off[0].
 * With the decider rule, seeks and bloom_out count the sources up to and including the decider.
 * The view is checked on the device in the same call before any lookup runs:
 *   SEGMENTS   an id >= nsst; level_start[0] != 0 or level_start decreases
 *   MALFORMED  a table of the view whose open failed (desc.err != 0), or two neighbours of a level
 *              with last_key(i) >= first_key(i+1) (check_sst_valid)
 * and with either raised no lookup runs: every res[q] is ABSENT with src / sst / hit_* 0xFFFFFFFF,
 * val_off is all zero, stats[3] carries the flag.  EMPTY_KEY (that key: ABSENT, no source) and
 * MALFORMED (a block on a lookup's path breaks the decode rules, every entry of a visited block
 * being checked: that source decides ABSENT) are as in lsmblk_sst_get_batch.  Every walk is
 * bounded by entry, block, table and source counts.  Asynchronous; 256 B of context workspace. */
int lsmblk_lsm_get_batch(lsmblk_ctx* ctx, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                         const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const lsmblk_lsm_view* view,
                         const uint8_t* qkeys, const uint32_t* qkey_off, const uint64_t* q_ts, uint64_t nq,
                         uint32_t flags, lsmblk_lsm_get_result* res, uint8_t* vals, uint64_t val_cap,
                         uint32_t* val_off, uint64_t* stats, void* stream);

/* ------------------------------------------------------------------ SST range scans (device) */
/* The read side's range read (scan_with_ts, src/lsm_storage.rs:446-550) over the opened set of the
 * point lookups: per SST the raw range scan (lsmblk_sst_scan_batch), across SSTs lsmblk_merge_batch
 * with the scans' seg_start as run_start, then the reader's view at read_ts
 * (lsmblk_read_filter_batch).  A batch of ranges over a whole LSM view, with any number of tables
 * per range, is one call of lsmblk_lsm_scan_batch (below). */

/* Bound kinds of q_bound: bits 0-1 the lower bound, bits 2-3 the upper bound (std::ops::Bound). */
#define LSMBLK_BOUND_UNBOUNDED 0u
#define LSMBLK_BOUND_INCLUDED 1u
#define LSMBLK_BOUND_EXCLUDED 2u

/* Result of one range (32 bytes).  Positions are SST-local (block, entry); blk == nblk with ent 0 is
 * the SST's end; all four are 0xFFFFFFFF when no seek was made (RANGE_OUT, a failed open, a bad
 * query) or a block on the range's path is malformed. */
typedef struct {
  uint32_t status;     /* LSMBLK_SCAN_* */
  uint32_t blk0, ent0; /* begin */
  uint32_t blk1, ent1; /* end, exclusive */
  uint32_t blocks;     /* blocks holding an entry of [begin, end) */
  uint64_t n;          /* entries of [begin, end) */
} lsmblk_scan_result;

#define LSMBLK_SCAN_OK 0u        /* n > 0 */
#define LSMBLK_SCAN_EMPTY 1u     /* the range holds no entry */
#define LSMBLK_SCAN_RANGE_OUT 2u /* range_overlap is false (src/lsm_storage.rs:142-167); no seek */

/* flags (the values of LSMBLK_GET_NO_FILTER / LSMBLK_GET_MVCC) */
#define LSMBLK_SCAN_NO_FILTER 1u /* skip range_overlap */
#define LSMBLK_SCAN_MVCC 2u      /* an Included / Excluded lower bound lands on the first entry in SST order
                                    with key >= the bound instead of the reference's landing */

/* nq raw range scans, the SsTableIterator that scan_with_ts builds per table
 * (src/lsm_storage.rs:474-502) run to its end bound: query q = SST q_sst[q], lower key
 * lkeys[lkey_off[q] .. lkey_off[q+1]), upper key ukeys[ukey_off[q] .. ukey_off[q+1]), kinds q_bound[q]
 * (an unbounded side's key is ignored; an empty key with a bounded kind raises EMPTY_KEY and the
 * range is empty).
 *   range_overlap against the SST's first / last key fails: LSMBLK_SCAN_RANGE_OUT.
 *   begin: Unbounded (0, 0); Included(k) the landing of SsTableIterator::create_and_seek_to_key(k),
 *     the (blk, ent) of lsmblk_sst_get_batch with LSMBLK_GET_NO_FILTER in the same mode; Excluded(k)
 *     that landing, then forward while the entry's key equals k (:487-496), across block ends.
 *   end: the first entry at or after begin with key > upper (Included) or >= upper (Excluded); the
 *     SST's end for an unbounded upper.  The bound is tested on every entry, the landing included:
 *     LsmIterator::new does not test its first position (src/lsm_iterator.rs:29-43), a quirk of the
 *     merged iterator that is deliberately not reproduced per SST.
 *   The end comes from the index search and one in-block count (SST entries are in key order; for
 *   files that are not the result is unspecified, every walk bounded by entry and block counts).
 * res[q]: the positions and the entry count.  out (may be NULL: sizes only) receives every version
 * of every entry of [begin, end), range after range in query order, with the bytes
 * lsmblk_decode_batch_ex gives for them (any alignment); seg_start (u32[nq+1], required) = each
 * range's first entry in out, the run_start shape of lsmblk_merge_batch.  Overlapping and repeated
 * ranges are each written in full.
 * stats: [0] entries [1] key bytes [2] value bytes [3] error flags: CAPACITY (a capacity of out is
 * too small: [0..2] hold the required sizes, nothing is written to out; res and seg_start are),
 * OVERFLOW (a total does not fit u32), SEGMENTS (a q_sst >= nsst or a bound kind of 3), EMPTY_KEY,
 * MALFORMED (a visited block breaks the decode rules, every entry of every visited block being
 * checked: that range is empty, LSMBLK_SCAN_EMPTY).  A query on an SST whose open failed is EMPTY.
 * All device pointers.  Asynchronous; workspace on the context (32 B per query + 3 MiB). */
int lsmblk_sst_scan_batch(lsmblk_ctx* ctx, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                          const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const uint32_t* q_sst,
                          const uint8_t* lkeys, const uint32_t* lkey_off, const uint8_t* ukeys,
                          const uint32_t* ukey_off, const uint32_t* q_bound, uint64_t nq, uint32_t flags,
                          lsmblk_scan_result* res, const lsmblk_kv_stream* out, uint32_t* seg_start,
                          uint64_t* stats, void* stream);

/* What a reader at read_ts sees of each segment of `in` (segment s = entries [seg_start[s],
 * seg_start[s+1]), seg_start u32[nseg+1] non-decreasing with seg_start[nseg] <= in->n; read_ts =
 * seg_ts[s], u64[nseg]): LsmIterator::move_to_key / next (src/lsm_iterator.rs:45-86) over an inner
 * iterator yielding the segment.  Within a segment user keys must ascend with versions newest
 * first (a raw scan of a builder-written SST, which may begin in the middle of a key's versions,
 * or lsmblk_merge_batch's output); then entry i is kept iff ts[i] <= read_ts, its value is not
 * empty, and i is the segment's first entry or key[i-1] != key[i] or ts[i-1] > read_ts.  Nothing
 * is compared across a segment boundary; entries outside every segment are dropped.  The kept
 * entries go in order to `out` (any alignment); out_seg_start (u32[nseg+1]) = each segment's kept
 * range.  stats: [0] kept entries [1] key bytes [2] value bytes [3] error flags (CAPACITY: the
 * required sizes, nothing written to out's arenas; SEGMENTS: a bad seg_start).  Asynchronous. */
int lsmblk_read_filter_batch(lsmblk_ctx* ctx, const lsmblk_kv_stream* in, const uint32_t* seg_start,
                             const uint64_t* seg_ts, uint32_t nseg, const lsmblk_kv_stream* out,
                             uint32_t* out_seg_start, uint64_t* stats, void* stream);

/* ------------------------------------------------------------------ LSM range scans (device) */
/* LsmStorageInner::scan_with_ts (src/lsm_storage.rs:446-550) for a batch of ranges over an LSM view
 * of the opened set (the lsmblk_lsm_view of lsmblk_lsm_get_batch, checked on the device by the same
 * check before anything else runs).  The view's memtable runs are the first sources of every range
 * (lsmblk_lsm_view: their slices, their place in raw); with nmem == 0 this is the scan below the
 * memtables.
 *
 * Sources of a range, in priority order (MergeIterator::create's index order): every L0 table, in l0
 * order, that passes range_overlap(lower, upper, first_key, last_key) (:142-167, :474-502), then
 * level by level every table of the level, in table order, that passes it (:504-538).  A level's
 * tables are in key order and do not overlap (check_sst_valid, src/iterators/concat_iterator.rs:82-93),
 * so one run per passing table yields what the level's SstConcatIterator yields after
 * create_and_seek_to_key / the Excluded skip (concat_iterator.rs:50-80): the tables before the seek's
 * table hold nothing at or after the bound, and the tables after the last passing one nothing within
 * the upper bound.
 * Per table: the run is exactly that table's lsmblk_sst_scan_batch range for the same bounds and
 * kinds, begin and end rules included (flags 0: the reference landing; LSMBLK_SCAN_MVCC: the corrected
 * landing; LSMBLK_LSM_SCAN_NEWEST: below).  LSMBLK_SCAN_NO_FILTER has no meaning across sources, and it
 * and every other flag bit return LSMBLK_E_INVAL, with or without the flags above.
 * Merge: MergeIterator's (LSMBLK_MERGE_RUNS, src/iterators/merge_iterator.rs:59-184), as in
 * lsmblk_lsm_get_batch: for every user key, all versions of the lowest-priority-index run that holds
 * the key, in that run's order, keys ascending.  The as-written TwoMergeIterator nesting of
 * scan_with_ts (:541-542) is NOT reproduced, as in the point read.
 * Reader's view: with q_ts != NULL the merged range q is cut by the rule of lsmblk_read_filter_batch
 * at read_ts = q_ts[q]: merged entry i is kept iff ts[i] <= read_ts, its value is not empty, and i is
 * the range's first merged entry or key[i-1] != key[i] or ts[i-1] > read_ts.  So a key whose owning
 * run has no visible version yields nothing even when a later source holds one, and a tombstone in
 * the owning run hides the key.  LsmIterator::new's untested first position
 * (src/lsm_iterator.rs:29-43) is not reproduced: the end bound holds for every entry.  With
 * q_ts == NULL the output is the merged stream itself (res[q].n == res[q].merged).
 *
 * LSMBLK_LSM_SCAN_NEWEST (the value of LSMBLK_LSM_GET_NEWEST; with or without LSMBLK_SCAN_MVCC, which
 * it implies) is the snapshot scan, the range read that lsmblk_lsm_get_batch's NEWEST is for a key.
 * Sources, table scans, the view check, the sub_cap / raw / out capacity contract, the stats words and
 * every error report are those of the other modes.
 *   Landing: the corrected one per table.  An Included / Excluded lower bound begins at a key's first
 *     version or after its last, and the end rule holds for every entry, so every run holds whole
 *     version groups.
 *   Merge: the stable merge of the range's runs by (key ascending bytewise with a shorter key less, ts
 *     descending, source ordinal ascending, position in the run ascending).  Every raw entry of a
 *     healthy range is in it: res[q].merged == res[q].raw.  With q_ts == NULL out is that stream --
 *     every version of every key from every passing table, in snapshot order -- and res[q].n ==
 *     res[q].merged.
 *   Reader's view (q_ts != NULL): the rule above over that merged stream.  Per key the row is the
 *     newest version at or below read_ts over all sources, the lower source ordinal winning an equal
 *     ts, and a tombstone there hides the key whichever source holds it.
 *   Precondition: every table's entries are in (key ascending, ts descending) order, as a builder fed
 *     by a memtable flush or a compaction writes them.  For other files the result is unspecified;
 *     every walk and search stays bounded as in the other modes. */
#define LSMBLK_LSM_SCAN_NEWEST 4u
typedef struct {           /* 32 bytes */
  uint32_t status;         /* LSMBLK_SCAN_OK (n > 0) or LSMBLK_SCAN_EMPTY */
  uint32_t sources;        /* tables of the view that passed range_overlap and were scanned */
  uint64_t raw;            /* entries of all those tables' raw scans */
  uint64_t merged;         /* entries MergeIterator yields over them (all versions of every owned key);
                              LSMBLK_LSM_SCAN_NEWEST: = raw */
  uint64_t n;              /* entries written to out for this range */
} lsmblk_lsm_scan_result;

/* nq ranges: range q = lower key lkeys[lkey_off[q] .. lkey_off[q+1]), upper key
 * ukeys[ukey_off[q] .. ukey_off[q+1]), kinds q_bound[q] (as lsmblk_sst_scan_batch), read_ts q_ts[q].
 *   sub_cap    the most table scans the batch may expand into (< 2^31); the context workspace is sized
 *              from nq, sub_cap and raw->entry_cap alone, nothing is read back, the call is asynchronous
 *   raw        required when out is given (NULL with out: LSMBLK_E_INVAL): receives the per-table raw
 *              scans back to back, ordered by range and then by source -- the scratch the merge reads.
 *              NULL: only the table scans are sized
 *   out        NULL: sizes only.  Else the final entries range after range in query order, with the
 *              bytes lsmblk_decode_batch_ex gives for them (any alignment)
 *   seg_start  u32[nq+1], required: each range's first entry in out
 *   nq == 0    writes seg_start[0] and the first word of both offsets arrays of raw and out
 * stats (u64[LSMBLK_LSM_SCAN_STATS_WORDS]): [0] out entries [1] out key bytes [2] out value bytes
 * [3] error flags [4] raw entries [5] raw key bytes [6] raw value bytes [7] table scans expanded.
 * CAPACITY carries the required sizes and nothing is written to the stream that was too small:
 *   [7] > sub_cap          no scan runs: only [7] and [3] are meaningful, every res[q] is EMPTY with
 *                          zero counts, seg_start is all zero
 *   else [4..6] > raw's    (or raw == NULL) [4..7] are valid, [0..2] are zero; res[q].sources and
 *                          res[q].raw are valid, merged and n zero, seg_start all zero
 *   else [0..2] > out's    every word, res and seg_start are valid; out's sizes never exceed raw's
 * Other flags: SEGMENTS / MALFORMED from the view check (as lsmblk_lsm_get_batch: no scan runs, every
 * res[q] EMPTY with zero counts, seg_start all zero); SEGMENTS for a bound kind of 3 and EMPTY_KEY for
 * an empty key with a bounded kind (that range is empty, no source); MALFORMED when a visited block
 * breaks the decode rules: the whole range is empty with sources, raw, merged and n all zero -- never
 * a partial merge -- while raw and [4..6] still hold its healthy tables' scans; OVERFLOW when a total
 * does not fit u32.  Every walk and search is bounded by entry, block, table and run counts. */
#define LSMBLK_LSM_SCAN_STATS_WORDS 8
int lsmblk_lsm_scan_batch(lsmblk_ctx* ctx, const uint8_t* files, const uint64_t* file_off, uint32_t nsst,
                          const lsmblk_sst_desc* desc, const lsmblk_sst_index* index, const lsmblk_lsm_view* view,
                          const uint8_t* lkeys, const uint32_t* lkey_off, const uint8_t* ukeys,
                          const uint32_t* ukey_off, const uint32_t* q_bound, const uint64_t* q_ts, uint64_t nq,
                          uint32_t flags, uint64_t sub_cap, lsmblk_lsm_scan_result* res,
                          const lsmblk_kv_stream* raw, const lsmblk_kv_stream* out, uint32_t* seg_start,
                          uint64_t* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
