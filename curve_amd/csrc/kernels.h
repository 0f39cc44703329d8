// curve_amd/csrc/kernels.h -- internal launcher interface between engine.hip
// (C ABI, device contexts) and kernels.hip (gfx950 kernels).  Not exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cc {

// LDS image geometry of the page kernel (see DESIGN.md "LDS image").
constexpr uint32_t kLdsBytes = 163840;  // all 160 KiB of a CU's LDS
// The device image is the LDS image followed by the x^(-8t) * x^i product table
// (kXinvEntries x 32 words).
constexpr uint32_t kFinBase = 131072;   // per-lane final-shift nibble tables [128K, 160K)
constexpr uint32_t kWordsPerWaveStep = 64;  // one dword per lane per step
constexpr uint32_t kWaveBytes = 256;        // bytes consumed per wave step
constexpr int kWavesPerBlock = 8;  // waves per CU (one workgroup per CU: the LDS image fills it); 8 beat 16 by 4-5 %
constexpr int kBlockThreads = 64 * kWavesPerBlock;
constexpr uint32_t kDynHeads = 8;  // dynamic-tail counters of the page kernel: one per XCD
constexpr uint32_t kDynHeadStride = 16;  // 128 bytes between heads: one cache line each
constexpr uint32_t kDynCtrBytes = kDynHeads * kDynHeadStride * 8;
constexpr uint32_t kDynCtrWords64 = kDynHeads * kDynHeadStride;  // the heads as uint64 words
// A stream's tail-counter block: two slot sets of heads; a launch pulls from
// one and zeroes the other for the stream's next launch (engine.hip tail_block).
constexpr uint32_t kTailBlockWords64 = 2 * kDynCtrWords64;
constexpr uint32_t kTailBlockBytes = kTailBlockWords64 * 8;

// Host builder of the 160 KiB LDS image (engine.hip).
void build_lds_image(uint32_t* image /* kLdsBytes/4 words */);

// Verify outputs: mismatch count, first bad page, and (optional) the list of
// bad page indices (unordered, at most max_list kept; count may exceed it).
struct VerifySink {
    unsigned long long* bad_count;
    unsigned long long* first_bad;
    unsigned long long* list;
    unsigned long long max_list;
    // cc_scrub_dev with neither struct: a bad page also counts on its chunk,
    // per_chunk[2 * (page / pages_per_chunk)] += 1 (null: no per-chunk words)
    uint32_t* per_chunk;
    uint32_t pages_per_chunk;
};

struct PageLaunch {
    const uint32_t* pages;
    uint64_t n_pages;
    uint32_t words_per_lane;  // page_bytes / 256
    const void* image;        // device copy of the LDS image
    uint32_t kconst;          // V-domain correction for this page size
    uint32_t* out;            // compute: CRC per page
    const uint32_t* expected; // verify: expected CRC per page
    VerifySink sink;          // verify only
    int blocks;
    uint32_t tile_shift;      // 2^tile_shift consecutive pages per wave tile (0..6)
    // dynamic tail: null = every tile in the strided static walk; else tiles
    // [static_tiles, all) are handed out through this zeroed counter
    unsigned long long* dyn_ctr;  // kDynHeads counters, kDynHeadStride words apart (zeroed before the launch)
    uint64_t static_tiles;
    // non-null: dyn_ctr is one slot set of the stream's tail block and this the
    // other, which the launch zeroes for the stream's next launch
    unsigned long long* dyn_next;
    // fused metapages (cc_pool_scan_dev when metapage size == page size): n_meta
    // more pages of the same size, appended to the dynamic tail as chunks of their own
    const uint32_t* meta_pages;
    uint64_t n_meta;
    uint32_t* meta_out;
    // block 0 zeroes these word ranges before its walk (stream-ordered for the
    // kernels after it: the next launch's tail counter, a digest to XOR into)
    uint32_t* zero[2];
    uint64_t zero_words[2];
    // non-null: timing events carried by the kernel's own dispatch
    // (hipExtLaunchKernel), so timing it adds no marker packets to the stream
    hipEvent_t ev_begin, ev_end;
};

hipError_t launch_page_crc(const PageLaunch& a, hipStream_t s);
// engine.hip, for cc_pool_scan_dev: metapage launch (clears the data launch's
// tail counter and the digest) then the data launch, bracketed by the events
int pool_page_launches(const void* d_data, uint64_t n_data_pages, uint32_t page_bytes, uint32_t* d_page_crcs,
                       const void* d_meta, uint64_t n_meta, uint32_t meta_bytes, uint32_t* d_meta_crcs,
                       uint32_t* d_digest, uint64_t digest_words, hipStream_t s, void* ev_begin, void* ev_end);
hipError_t launch_read_probe(const void* buf, uint64_t bytes, uint32_t* sink, int blocks, hipStream_t s);
hipError_t launch_page_verify(const PageLaunch& a, hipStream_t s);
// the page kernel with its CRC arithmetic replaced by a rotate-XOR (4 KiB pages):
// the same schedule, loads and stores -- the ceiling the real kernel is held to
hipError_t launch_page_load_probe(const PageLaunch& a, hipStream_t s);
// the scan step's metapage pass (a separate instantiation, same code as compute)
hipError_t launch_page_meta(const PageLaunch& a, hipStream_t s);

struct FoldLaunch {
    const uint32_t* crcs;
    uint64_t n_groups;
    uint32_t per_group;
    uint32_t m_unit;      // x^(8*unit_bytes) mod P
    uint32_t m_tree[7];   // x^(8*unit_bytes*q*2^t), t=0..5 (fast path, q = per_group/64)
    uint32_t* out;
};
hipError_t launch_fold(const FoldLaunch& a, hipStream_t s);

// x^(2^k) mod P table for the shift kernel, uploaded once per device.
hipError_t upload_x2k(const uint32_t* t64);

hipError_t launch_shift(const uint32_t* crcs, const uint64_t* shift_bytes, uint64_t n,
                        uint32_t* out, hipStream_t s);

struct UpdateDesc {
    uint64_t dst, src;
    uint32_t len, reserved;
};

// Write-log path (cc_apply_log_dev): every update of an ORDERED log becomes
// `slots` pieces, one per page it touches; an open-addressing table keyed by
// page groups them (each entry heads a linked list of the page's pieces) with
// no sort; one wave per touched page (balanced over the grid) then applies its
// pieces in log order in registers, stores the changed rows and rehashes it.
// A page with more than 64 pieces is finished by its wave replaying the log.
constexpr uint32_t kNoPiece = 0xFFFFFFFFu;
constexpr uint32_t kInsertThreads = 512;   // pieces per insert chunk, one a thread (512: every CU busy; profiles/write_log_insert_threads_ab_r04.txt)
constexpr uint32_t kInsertBlocks = 256;    // insert blocks at most (grid-stride over chunks): head segments
constexpr int kLogWaves = 12;  // waves per CU of the write-log page kernel at 8 KiB pages (A/B at 4 KiB, round 1: 12 beats 8 by ~6 %)
constexpr int kLogWavesFull = 16;   // full mode, pages <= 4 KiB: 103 VGPRs since the row offsets went into the offset field
constexpr int kLogWavesDelta = 16;  // delta mode, pages <= 4 KiB: 120 VGPRs at 16 waves (was 12 waves: 129 would spill)
// waves per workgroup of log_pages_kernel<M, Delta>
constexpr int log_waves(int m, bool delta) { return m > 16 ? kLogWaves : (delta ? kLogWavesDelta : kLogWavesFull); }
// waves per workgroup of log_small_kernel<M, Delta>
constexpr int log_small_waves(int m, bool delta) { return (!delta && m <= 16) ? kLogWavesFull : kLogWaves; }
// The NEXT batch's grouping, done by the page kernel of the current one
// (cc_apply_logs_dev): its pieces go into its own table and head segments, in
// the kernel's tail -- a workgroup done with its pages takes chunks of the next
// batch (one counter) while the slower ones finish -- so the kernel boundary
// before the next page kernel is the only barrier the next batch needs.  The
// fields insert_piece reads, for that batch; n_pieces = 0: nothing to insert.
// chunks a workgroup claims per take of the tail grouping's counter (A/B: 2 beats
// 1 by ~0.6 %: half as many, earlier-finishing workgroups do the inserts); a
// compile-time knob for the A/B builds
#ifndef CC_GROUP_TAKE
#define CC_GROUP_TAKE 2
#endif
constexpr uint32_t kGroupTake = CC_GROUP_TAKE;
struct LogInsert {
    const UpdateDesc* upd;
    uint64_t n_pieces;
    uint64_t pool_bytes;
    uint32_t page_bytes, max_len, slots, table_mask;
    uint64_t* table;
    uint32_t* next;
    uint32_t* heads;            // one segment of seg_cap records per block of the inserting kernel
    uint32_t* seg_count;        // [gridDim.x of the inserting kernel]
    uint32_t seg_cap;           // >= rounds x the block's threads
    uint32_t rounds;            // chunks (of the block's threads) one workgroup may take: a multiple of kGroupTake
    unsigned long long* take;   // the chunk counter, zero at launch (the grouping kernel before zeroed it)
    unsigned long long* zero;   // the counter the grouping kernel after next takes from: zeroed here
};
struct LogLaunch {
    unsigned char* pool;
    uint64_t pool_bytes;
    const unsigned char* src;
    const UpdateDesc* upd;
    uint64_t n_updates;
    uint32_t page_bytes;
    uint32_t max_len;
    uint32_t slots;             // pieces per update: (max_len - 1) / page_bytes + 2
    uint64_t n_pieces;          // n_updates * slots
    uint64_t* table;            // [table_mask + 1] {page + 1, piece + 1} of the page's list head (0 = empty)
    uint32_t table_mask;
    uint32_t* next;             // [n_pieces] next piece of the same page (kNoPiece = end)
    // head records {table slot, claiming piece} of the touched pages (uint2), in
    // one segment of seg_cap records per insert block: block b's at b * seg_cap,
    // seg_count[b] of them (written by the insert, no clearing needed)
    uint32_t* heads;
    uint32_t* seg_count;        // [n_segs]
    uint32_t seg_cap;
    uint32_t n_segs;            // insert blocks (<= kInsertBlocks)
    int clear_table;            // the table is the engine's per-stream one: the page kernel leaves it zero
    const void* image;
    uint32_t kconst;
    uint32_t* page_crcs;        // out; in delta mode also in (the CRCs before the batch)
    int blocks;
    int delta;                  // 1: update the stored CRCs through linearity (reads touched rows only)
    LogInsert nx;               // the next batch's grouping, in this batch's page kernel (launch_log_pages)
    unsigned long long* zero_ctrs;  // log_insert_kernel zeroes these 3 words (the queue's chunk counters) or null
};
hipError_t launch_log_insert(const LogLaunch& a, hipStream_t s);
hipError_t launch_log_pages(const LogLaunch& a, hipStream_t s);
// <= 64 writes of <= 2 pieces each in one launch (no table, no insert)
hipError_t launch_log_small(const LogLaunch& a, hipStream_t s);
// Copy on write (cc_apply_log_cow_dev): between launch_log_insert and
// launch_log_pages, one wave per head record copies the page's old bytes and
// its stored CRC into its chunk's snapshot slot unless the slot's bitmap
// already holds the page.  Reads the table and the head records only.
constexpr int kCowWaves = 16;  // waves per workgroup of log_cow_kernel<M, Verify>
struct LogCowLaunch {
    const unsigned char* pool;
    const uint64_t* table;      // LogLaunch::table after the insert: page = entry >> 32, minus 1
    const uint32_t* heads;      // LogLaunch::heads / seg_count / seg_cap / n_segs
    const uint32_t* seg_count;
    uint32_t seg_cap;
    uint32_t n_segs;
    uint32_t n_pages;           // pool pages
    uint32_t page_bytes;
    uint32_t pages_per_chunk;
    uint32_t words_per_slot;    // bitmap words a slot: ceil(pages_per_chunk / 32)
    uint32_t n_slots;
    const uint32_t* snap_slot;  // [chunks] slot of the chunk's open snapshot (>= n_slots: none)
    unsigned char* snap;        // n_slots x chunk
    uint32_t* snap_crcs;        // n_slots x pages_per_chunk
    uint32_t* snap_bitmap;      // n_slots x words_per_slot
    const uint32_t* page_crcs;  // the pool's CRC table before the batch
    unsigned long long* copied; // += pages copied, or null
    unsigned long long* stale;  // += copied pages whose bytes mismatch page_crcs (null: no rehash, no LDS image)
    const void* image;
    uint32_t kconst;
    int blocks;
};
hipError_t launch_log_cow(const LogCowLaunch& a, hipStream_t s);
// diagnostic: the write log's page traffic alone (4 KiB pages; kernels.hip log_probe_kernel)
struct LogProbeDesc {
    uint64_t page;      // touched page
    uint64_t src_off;   // source byte of page byte 0 (mod 2^64) when covered != 0
    uint32_t covered;   // rows read from the source (the page's only piece covers them whole)
    uint32_t dirty;     // rows stored back
};
struct LogProbeLaunch {
    unsigned char* pool;
    uint64_t pool_pages;  // a descriptor naming a page >= this touches nothing (reads page 0, stores none)
    const unsigned char* src;
    const LogProbeDesc* desc;
    uint64_t n;
    uint32_t* out;  // [n]
    int blocks;
};
hipError_t launch_log_probe(const LogProbeLaunch& a, hipStream_t s);
// diagnostic: the read traffic of a page list alone (4 KiB pages; kernels.hip page_list_probe_kernel)
struct PageListProbeLaunch {
    const uint32_t* pool;
    uint64_t pool_pages;  // an index >= this reads page 0 instead (never outside the pool)
    const uint64_t* pages;
    uint64_t n;
    uint32_t* out;  // [n]
    int blocks;
    // dynamic tail, as verify-on-read's: the last 1/16 of the list in 32-page
    // chunks through *dyn_ctr (zero at launch); the launch zeroes *dyn_next (the
    // stream's other slot set) for the next one.  Null: a static split only.
    unsigned long long* dyn_ctr;
    unsigned long long* dyn_next;
};
hipError_t launch_page_list_probe(const PageListProbeLaunch& a, hipStream_t s);

struct RangeDesc {
    uint64_t off, len;
};

// Verify-on-read for a batch of reads (cc_verify_reads_dev): every page a read
// touches is a "slot"; the batch's slots are read 0's pages, then read 1's, ...;
// ONE launch on the range kernel's schedule: the waves count kRangeTiles tiles
// of reads themselves (epoch-tagged words in the stream's range scratch) and
// each rehashes an equal share of the slots, the last 1/16 dynamically.
struct ReadVerifyLaunch {
    const uint32_t* pool;
    uint64_t pool_bytes;
    uint32_t page_bytes;
    uint32_t page_shift;        // log2(page_bytes)
    const RangeDesc* reads;
    uint64_t n_reads;
    const uint32_t* page_crcs;  // stored CRC per pool page
    uint32_t* bad_per_read;     // [n_reads] += mismatching pages; UINT32_MAX for a read beyond the pool
    unsigned long long* bad_total;
    uint64_t* tiles;            // [kReadTiles] epoch << 40 | pages of the tile
    unsigned long long* tail;   // dynamic-tail counter slots (epoch % 2: this call's; the other zeroed for the next)
    uint32_t epoch;
    const void* image;
    uint32_t kconst;
    int blocks;
};
hipError_t launch_read_verify(const ReadVerifyLaunch& a, hipStream_t s);
// <= 64 reads in one launch (no tiles; pages split over waves)
hipError_t launch_read_verify_small(const ReadVerifyLaunch& a, hipStream_t s);
// Snapshot reads (cc_read_snap_dev): verify-on-read's schedule over page-aligned
// reads, every page slot resolved to its snapshot-view source first -- the
// chunk's slot page and its CRC in snap_crcs when the slot's bitmap holds the
// page, the live page and page_crcs otherwise -- rehashed against that CRC and,
// with `out`, stored at out + out_off[read] + (page's position in the read).
// n_slots == 0: no snapshot (cow == NULL), every page is live and the snapshot
// fields are not read.
struct SnapReadLaunch {
    ReadVerifyLaunch rv;         // pool, reads, page_crcs, counters, tiles, tail, epoch, image, grid
    uint32_t pages_per_chunk;
    uint32_t words_per_slot;     // bitmap words a slot: ceil(pages_per_chunk / 32)
    uint32_t n_slots;
    uint32_t ppc_mlo, ppc_mhi;   // ceil(2^64 / pages_per_chunk): page / pages_per_chunk for pages < 2^32 (snap_recip)
    const uint32_t* snap_slot;   // [chunks] slot of the chunk's open snapshot (>= n_slots: none)
    const unsigned char* snap;   // n_slots x chunk
    const uint32_t* snap_crcs;   // n_slots x pages_per_chunk
    const uint32_t* snap_bitmap; // n_slots x words_per_slot
    unsigned char* out;          // null: verify only
    const uint64_t* out_off;     // [n_reads] byte offset of read i's bytes in out
    uint64_t out_bytes;
};
// the reciprocal the kernels divide by: ceil(2^64 / d), exact for n < 2^32 (d >= 2; the kernels divide otherwise)
inline uint64_t snap_recip(uint32_t d) { return d > 1 ? ~0ull / d + 1 : 0; }
hipError_t launch_snap_read(const SnapReadLaunch& a, hipStream_t s);
// <= 64 reads in one launch (no tiles, no scratch)
hipError_t launch_snap_read_small(const SnapReadLaunch& a, hipStream_t s);
// Clone chunks (cc_paste_dev, cc_clone_mark_dev, cc_clone_check_reads_dev): the
// written-page bitmaps of cc_clone.  Chunk c's bitmap is slot clone_slot[c]
// (>= n_slots: not a clone chunk); page q of a slot is bit q % 32 of word q / 32.
struct CloneGeo {
    uint32_t pages_per_chunk;
    uint32_t words_per_slot;     // bitmap words a slot: ceil(pages_per_chunk / 32)
    uint32_t n_slots;
    uint32_t ppc_mlo, ppc_mhi;   // snap_recip(pages_per_chunk)
    const uint32_t* clone_slot;  // [chunks]
    uint32_t* bitmap;            // n_slots x words_per_slot
    uint32_t* claim;             // n_slots x pages_per_chunk, all 0xFFFFFFFF between calls (paste only)
};
// cc_paste_dev: an ORDERED batch of Paste requests in two launches.  The claim
// launch leaves in claim[s * pages_per_chunk + q] the lowest index of the valid
// entries covering a clone page whose bit is clear (and marks the invalid
// entries); the paste launch walks the batch's (entry, page) slots on
// verify-on-read's schedule, and the slot that finds its own index in the claim
// word copies its source page into the pool, hashing it on the way, writes the
// CRC, sets the bit, counts, and resets the claim word.
struct PasteLaunch {
    uint32_t* pool;
    uint64_t pool_bytes;
    uint32_t page_bytes;
    uint32_t page_shift;         // log2(page_bytes)
    const unsigned char* src;
    uint64_t src_bytes;
    const UpdateDesc* pastes;
    uint64_t n;
    uint32_t* page_crcs;
    CloneGeo geo;
    unsigned long long* pasted;  // += pages pasted, or null
    uint32_t* pasted_per_entry;  // [n] += pages entry i pasted; UINT32_MAX for an invalid entry
    uint64_t* tiles;             // the stream's range scratch, as ReadVerifyLaunch
    unsigned long long* tail;
    uint32_t epoch;
    const void* image;
    uint32_t kconst;
    int blocks;                  // CUs
};
hipError_t launch_paste_claim(const PasteLaunch& a, hipStream_t s);
hipError_t launch_paste(const PasteLaunch& a, hipStream_t s);
// cc_clone_mark_dev: the bits of the pages a write log covered whole (one launch; reads no page)
struct CloneMarkLaunch {
    CloneGeo geo;
    uint64_t pool_bytes;
    uint32_t page_bytes;
    uint32_t page_shift;
    uint32_t max_len;
    const UpdateDesc* log;
    uint64_t n;
    int blocks;                  // CUs
};
hipError_t launch_clone_mark(const CloneMarkLaunch& a, hipStream_t s);
// cc_apply_logs_cow_dev: the copy-on-write pass and the clone marks of a whole
// QUEUE of write logs in one launch BEFORE the queue's own kernels (a snapshot
// keeps a page's first version, and the first batch that touches a page finds
// it as it stood before the queue).  Up to kPrepassBatches batch descriptors
// ride in the kernel argument: no host-to-device copy, no allocation.  One lane
// is one (entry, page slot) pair, `slots` pairs an entry as the insert kernel
// counts its pieces; pair0 is the batch's first pair in the launch.
constexpr int kPrepassBatches = 32;
constexpr int kPrepassWaves = 16;  // waves per workgroup of logs_prepass_kernel<M, Verify>
struct LogsPrepassBatch {
    const UpdateDesc* upd;
    uint64_t n_pairs;  // n_updates x slots (< 2^31: log_work)
    uint64_t pair0;    // pairs of the launch's earlier batches
};
struct LogsPrepassLaunch {
    LogsPrepassBatch b[kPrepassBatches];  // 768 bytes
    uint32_t n_batches;
    uint64_t n_pairs;            // of all n_batches
    const unsigned char* pool;
    uint64_t pool_bytes;
    uint32_t page_bytes;
    uint32_t page_shift;
    uint32_t max_len;
    uint32_t slots;
    // the snapshot side (LogCowLaunch's fields); snap_slot null: no cc_cow
    uint32_t pages_per_chunk;
    uint32_t words_per_slot;
    uint32_t n_slots;
    const uint32_t* snap_slot;
    unsigned char* snap;
    uint32_t* snap_crcs;
    uint32_t* snap_bitmap;
    const uint32_t* page_crcs;   // the pool's CRC table before the queue
    unsigned long long* copied;  // += pages copied, or null
    unsigned long long* stale;   // += copied pages whose bytes mismatch page_crcs (null: no rehash, no LDS image)
    // the clone side; clone.clone_slot null: no cc_clone (claim is never used)
    CloneGeo clone;
    const void* image;
    uint32_t kconst;
    int blocks;
};
hipError_t launch_logs_prepass(const LogsPrepassLaunch& a, hipStream_t s);
// cc_apply_ops_dev: a queue of write logs AND paste batches.  Three pass kinds
// run before the queue's own launches, each over (entry, page slot) pairs with
// a lane per pair, the batch descriptors in the kernel argument as above:
//   BID      batches 0 .. the last paste batch: a paste pair, and a write pair
//            that covers its page whole, bids for a clone page whose bit is clear
//            with atomicMin(claim, 2 x ordinal + kind); marks invalid paste entries
//   RESOLVE  the write batches among them: a pair that finds its own key puts
//            all-ones back; a pair covering its page partly that finds the key of
//            a LATER paste counts one contested pair
//   PASTE    the paste batches: the pair that finds its own key copies and hashes
//            its source page, writes the CRC, sets the bit, counts and resets
// An entry's ordinal is its position in the queue (ord0 of its batch + its index).
constexpr int kOpsBatches = 32;
constexpr int kOpsWaves = 16;  // waves per workgroup of the three kernels
constexpr uint32_t kOpWrite = 0, kOpPaste = 1;  // CC_OP_WRITE, CC_OP_PASTE
struct OpsBatch {
    const UpdateDesc* recs;
    const unsigned char* src;    // paste: the batch's origin buffer
    uint64_t src_bytes;          // paste: its size
    uint32_t* pasted_per_entry;  // paste: [n] += pages entry i pasted; UINT32_MAX for an invalid entry
    uint64_t pair0;              // pairs of the launch's earlier batches
    uint32_t ord0;               // ordinal of the batch's entry 0
    uint32_t kind;               // kOpWrite | kOpPaste
};
struct OpsLaunch {
    OpsBatch b[kOpsBatches];     // 1536 bytes
    uint32_t n_batches;
    uint64_t n_pairs;            // of all n_batches
    uint32_t* pool;
    uint64_t pool_bytes;
    uint32_t page_bytes;
    uint32_t page_shift;
    uint32_t max_len;            // write entries: the write log's rule
    uint32_t max_paste_len;      // paste entries: a multiple of page_bytes
    uint32_t slots;              // pairs a write entry (log_slots)
    uint32_t paste_slots;        // pairs a paste entry: max_paste_len / page_bytes
    uint32_t* page_crcs;
    CloneGeo geo;
    unsigned long long* pasted;     // += pages pasted, or null
    unsigned long long* contested;  // += contested (write entry, page) pairs, or null
    const void* image;
    uint32_t kconst;
    int blocks;
};
hipError_t launch_ops_bid(const OpsLaunch& a, hipStream_t s);
hipError_t launch_ops_resolve(const OpsLaunch& a, hipStream_t s);
hipError_t launch_ops_paste(const OpsLaunch& a, hipStream_t s);
// cc_clone_check_reads_dev: per read, the touched pages of clone chunks whose bit is clear (one launch)
struct CloneCheckLaunch {
    CloneGeo geo;
    uint64_t pool_bytes;
    uint32_t page_shift;
    const RangeDesc* reads;
    uint64_t n;
    uint32_t* unwritten_per_read;   // [n] += ; UINT32_MAX for a read past the pool
    unsigned long long* unwritten_total;
    int blocks;                  // CUs
};
hipError_t launch_clone_check(const CloneCheckLaunch& a, hipStream_t s);
// Clone reads (cc_read_merge_dev): snapshot reads' schedule over page-aligned
// reads of a pool with clone chunks, every page slot resolved against its
// chunk's written-page bitmap first.  A written page (no clone chunk, or its
// bit set) is the live pool page: rehashed against page_crcs and stored at
// out + out_off[read] + (page's position in the read).  A never-written page
// (clone chunk, bit clear) counts on its read; when the read has an origin
// (origin != null and origin_off[read] != kNoOrigin) the page's bytes are
// origin + origin_off[read] + (page's position in the read), stored unhashed,
// otherwise nothing of the page moves.  geo.claim is not used; geo.bitmap is
// only read.  geo.n_slots == 0: every page is written and the tables are not read.
constexpr uint64_t kNoOrigin = ~0ull;
struct MergeReadLaunch {
    ReadVerifyLaunch rv;            // pool, reads, page_crcs, bad counters, tiles, tail, epoch, image, grid
    CloneGeo geo;
    const unsigned char* origin;    // the fetched origin buffers, or null
    const uint64_t* origin_off;     // [n_reads] byte offset of read i's origin bytes (kNoOrigin: none); null with origin
    uint64_t origin_bytes;
    unsigned char* out;
    const uint64_t* out_off;        // [n_reads] byte offset of read i's bytes in out
    uint64_t out_bytes;
    uint32_t* unwritten_per_read;   // [n_reads] += never-written pages; UINT32_MAX for an invalid read
    unsigned long long* unwritten_total;
};
hipError_t launch_merge_read(const MergeReadLaunch& a, hipStream_t s);
// <= 64 reads in one launch (no tiles, no scratch)
hipError_t launch_merge_read_small(const MergeReadLaunch& a, hipStream_t s);
// Page repair (cc_repair_dev): an ORDERED batch of candidate ranges in two
// launches, as cc_paste_dev.  The claim launch leaves in claim[p] the lowest
// index of the valid entries naming pool page p (and marks the invalid
// entries); the repair launch walks the batch's (entry, page) slots on
// verify-on-read's schedule.  The slot that finds its own index in claim[p]
// handles the page: it hashes the live page against e = expect ? expect[p] :
// page_crcs[p]; when that misses it loads and hashes the candidate and stores
// it when it hits; it counts the page on its entry by class and resets the
// claim word.  Every other slot
// is shadowed: no page traffic, no hash, one count a run.
constexpr uint32_t kRepairClean = 0, kRepairRepaired = 1, kRepairFailed = 2, kRepairShadowed = 3;
struct RepairLaunch {
    uint32_t* pool;
    uint64_t pool_bytes;
    uint32_t page_bytes;
    uint32_t page_shift;         // log2(page_bytes)
    const unsigned char* src;
    uint64_t src_bytes;
    const UpdateDesc* reqs;
    uint64_t n;
    uint32_t* page_crcs;
    const uint32_t* expect;      // [pool pages] the authority's CRCs, or null: page_crcs is the record
    uint32_t* claim;             // [pool pages], all 0xFFFFFFFF between calls
    uint32_t* per_entry;         // [n][4] += entry i's pages by class; all four UINT32_MAX for an invalid entry
    unsigned long long* totals;  // [4] += the four sums, or null
    uint64_t* tiles;             // the stream's range scratch, as ReadVerifyLaunch
    unsigned long long* tail;
    uint32_t epoch;
    const void* image;
    uint32_t kconst;
    int blocks;                  // CUs
};
hipError_t launch_repair_claim(const RepairLaunch& a, hipStream_t s);
hipError_t launch_repair(const RepairLaunch& a, hipStream_t s);
// Scrub (cc_scrub_dev): the integrity pass over the pages that EXIST.  The
// domain is the live pages [0, n_pages) and, with a snapshot side, their
// snapshot copies [n_pages, 2 n_pages), in groups of 64 indices on
// verify-on-read's schedule (groups for reads).  A live page exists unless its
// chunk is a clone chunk whose bit is clear (counted, never read); a snapshot
// page exists when its chunk names a slot whose bit is set.  Every page that
// exists is hashed against its table's word; nothing else moves.
struct ScrubLaunch {
    const uint32_t* pool;
    uint64_t n_pages;            // pool pages (< 2^32)
    uint64_t n_index;            // the domain: n_pages, or 2 n_pages with a snapshot side
    uint64_t n_groups;           // ceil(n_index / 64)
    uint32_t page_shift;         // log2(page_bytes)
    uint32_t words_per_lane;     // page_bytes / 256
    uint32_t pages_per_chunk;
    uint32_t words_per_slot;     // bitmap words a slot: ceil(pages_per_chunk / 32)
    uint32_t ppc_mlo, ppc_mhi;   // snap_recip(pages_per_chunk)
    const uint32_t* page_crcs;
    // the snapshot side (cc_cow); snap_slot null: none
    uint32_t snap_n_slots;
    const uint32_t* snap_slot;
    const unsigned char* snap;
    const uint32_t* snap_crcs;
    const uint32_t* snap_bitmap;
    // the clone side (cc_clone); clone_slot null: none
    uint32_t clone_n_slots;
    const uint32_t* clone_slot;
    const uint32_t* clone_bitmap;
    unsigned long long* counts;  // cc_scrub_counts: live_checked, live_bad, snap_checked, snap_bad, unwritten, listed
    unsigned long long* list;    // [max_list] entries: page, or 2^63 | page for a snapshot copy
    uint64_t max_list;
    uint32_t* per_chunk;         // cc_scrub_chunk [chunks] {live_bad, snap_bad}, or null
    uint64_t* tiles;             // the stream's range scratch, as ReadVerifyLaunch
    unsigned long long* tail;
    uint32_t epoch;
    const void* image;
    uint32_t kconst;
    int blocks;                  // CUs
};
hipError_t launch_scrub(const ScrubLaunch& a, hipStream_t s);
// the one-thread kernels around the page kernel when cc_scrub_dev has neither struct (kernels.hip scrub_plain_kernel)
hipError_t launch_scrub_plain(unsigned long long* counts, uint64_t n_pages, int post, hipStream_t s);
// CRC32C (butil Value) of arbitrary byte ranges of one device buffer, on the
// flat block schedule, ONE launch: range_flat_kernel counts the
// 4 KiB blocks of kRangeTiles contiguous tiles of the batch itself (epoch-tagged
// words in `tiles`), gives every wave an equal share of the blocks, and ranges
// cut by a share boundary meet in their accumulator pair (acc[2r], acc[2r+1]).
// The per-stream scratch (engine.hip range_work) is zero on first use and left
// so by every launch: tiles are overwritten each call (the epoch tells this
// call's words), the accumulators self-reset and each call zeroes the tail
// counter slot the next call uses.
constexpr uint32_t kRangeTiles = 1024;
// verify on read counts its reads in fewer tiles (half the words every wave
// polls; A/B round 6, profiles/range_tiles_ab_r06.txt); the scratch holds kRangeTiles
constexpr uint32_t kReadTiles = 512;
static_assert(kReadTiles <= kRangeTiles && kReadTiles % 64 == 0, "read tiles share the range scratch");
struct RangeLaunch {
    const unsigned char* buf;
    const RangeDesc* ranges;
    uint64_t n;
    uint64_t* tiles;             // [kRangeTiles] epoch << 40 | blocks of the tile
    unsigned long long* tail;    // dynamic-tail counter slots (epoch % 2: this call's; the other zeroed for the next)
    uint32_t* acc;               // [2 n] split-range XOR / block-count pairs, zero at rest
    uint32_t epoch;              // 1 .. 2^24 - 1, the next one (parity alternating) per call on the scratch
    const void* image;
    uint32_t* out;
    int blocks;
};
hipError_t launch_range_flat(const RangeLaunch& a, hipStream_t s);
// x^(-8t) mod P for t = 0..kXinvEntries-1 (undoing the zero pad after a range in its last 4 KiB block)
constexpr uint32_t kXinvEntries = 4100;  // x^(-8t), t < 4096 + 4: the zero pad after a range in its last 4 KiB block

// Fused scan epilogue: one 256-thread block per chunk.
struct EpilogueLaunch {
    const uint32_t* page_crcs;  // [n_chunks * pages_per_chunk]
    const uint32_t* meta_crcs;  // [n_chunks]
    uint64_t n_chunks;
    uint32_t pages_per_chunk;   // 256 * q
    uint32_t q;                 // pages per thread
    uint32_t slice_shift;       // log2(threads per slice)
    const uint32_t* mtab;       // product tables [10][4][256]: 0 = x^(8 page), 1..8 = level k-1, 9 = chunk
    uint32_t* slice_crcs;       // [n_chunks * 256 >> slice_shift]
    uint32_t* file_crcs;        // [n_chunks] (may be null)
    const uint32_t* after_mult; // digest inputs x^(8 * after_bytes) (all three null = no digest)
    const uint32_t* group;
    uint32_t* digest;
};
hipError_t launch_epilogue(const EpilogueLaunch& a, hipStream_t s);
hipError_t launch_xpow8(const uint64_t* nbytes, uint64_t n, uint32_t* out, hipStream_t s);

hipError_t launch_combine(const uint32_t* a, const uint32_t* b, uint32_t m_len_b, uint64_t n, uint32_t* out,
                          hipStream_t s);

hipError_t launch_digest(const uint32_t* crcs, const uint64_t* after_bytes, const uint32_t* group, uint64_t n,
                         uint32_t* digest, hipStream_t s);

// out[i] = XOR_r gathered[r*n + i]  (digest fold after the RCCL all-gather)
hipError_t launch_xor_fold(const uint32_t* gathered, uint32_t nranks, uint64_t n, uint32_t* out, hipStream_t s);

}  // namespace cc
