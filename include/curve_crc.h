/*
 * include/curve_crc.h -- C ABI of libcurvecrc, the MI355X-native chunk-checksum
 * engine for Curve's per-page CRC32C integrity path.
 *
 * Plain C: no C++ or torch types cross this boundary; pointers + sizes only.
 * Every entry point cites the reference interface it replaces (paths relative
 * to the opencurve/curve tree).
 *
 * Conventions
 *   - CRC values are CRC-32C (Castagnoli, reflected poly 0x82F63B78) with
 *     butil semantics: crc32c_extend(c, A||B) == crc32c_extend(crc32c_extend(c, A), B),
 *     crc32c_value(p, n) == crc32c_extend(0, p, n), value of the empty buffer = 0.
 *   - Functions returning `int` return CC_OK (0) or a negative CC_E* code.
 *   - `*_dev` calls take caller-owned device memory on the calling thread's
 *     current HIP device, enqueue on `stream` (a hipStream_t, NULL = default
 *     stream) and return without synchronising.  They never fall back to the
 *     CPU: with no usable GPU they return CC_ENODEV.
 */
#ifndef CURVE_CRC_H_
#define CURVE_CRC_H_

#include <stddef.h>
#include <stdint.h>
#include <sys/uio.h> /* struct iovec */

#ifdef __cplusplus
extern "C" {
#endif

#define CC_OK 0
#define CC_EINVAL (-22)   /* bad argument (size, alignment, null pointer) */
#define CC_ENODEV (-19)   /* no HIP device / device code unavailable */
#define CC_ENOMEM (-12)   /* device or pinned-host allocation failed */
#define CC_EHIP (-5)      /* a HIP runtime call failed */
#define CC_ECORRUPT (-74) /* verify found mismatching pages (host verify) */
#define CC_EIO (-5001)    /* reading or writing a file failed (errno is kept where the call says so) */
#define CC_ESTALE (-116)  /* a per-page CRC table no longer describes its chunk (sn / write generation) */
#define CC_ETIMEDOUT (-110) /* a bounded wait expired (communicator init whose peers never joined) */
#define CC_EFORMAT (-5002) /* a chunk file's size is not metapage + chunk (CSErrorCode::FileFormatError,
                              chunkserver_chunkfile.cpp:233-238) */

/* ------------------------------------------------------------------------
 * CPU primitive -- drop-in for the inline header src/common/crc32.h
 * ------------------------------------------------------------------------ */

/* Replaces curve::common::CRC32(const char*, size_t)  (src/common/crc32.h:40-42)
 * = butil::crc32c::Value.  Also nebd::common::CRC32 (nebd/src/common/crc32.h). */
uint32_t crc32c_value(const void* p, size_t n);

/* Replaces curve::common::CRC32(uint32_t, const char*, size_t) (src/common/crc32.h:53-55)
 * = butil::crc32c::Extend.  Pure, reentrant, any length/alignment. */
uint32_t crc32c_extend(uint32_t crc, const void* p, size_t n);

/* GF(2) algebra (new; needed to derive the reference digests from page CRCs).
 * crc32c_combine(V(A), V(B), |B|) == V(A||B)  (zlib crc32_combine identity).
 * crc32c_shift(c, n) multiplies the 32-bit register by x^(8n) mod P. */
uint32_t crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
uint32_t crc32c_shift(uint32_t crc, uint64_t nbytes);
/* V(n zero bytes); e.g. crc32c_zeros(4096) == 0x98F94189, the CRC of every page
 * of a freshly formatted pool chunk (src/tools/curve_format_main.cpp:132). */
uint32_t crc32c_zeros(uint64_t nbytes);

/* CRC32C over a scattered buffer: crc32c_extend(crc, iov[0] || iov[1] || ...).
 * Replaces braft::crc32(const butil::IOBuf&) -- the checksum CurveSegment::append
 * takes over every WAL entry's data IOBuf (src/chunkserver/raftlog/curve_segment.cpp:405,
 * get_checksum :283-288) -- which walks the IOBuf's blocks and extends one CRC
 * across them.  Fragments of any length/alignment (0 allowed). */
uint32_t crc32c_extend_iov(uint32_t crc, const struct iovec* iov, size_t n);

/* Fold n page CRCs (each over page_bytes) into the CRC of their concatenation. */
uint32_t cc_fold_host(const uint32_t* page_crcs, uint64_t n, uint64_t page_bytes);

/* Batched host fold: out[s] = CRC of pages s*pages_per_slice ..
 * (s+1)*pages_per_slice - 1, for n_pages / pages_per_slice slices; e.g. the
 * 1024 page CRCs of a 4 MiB scan slice -> its ScanMap.crc (proto/scan.proto:28,
 * op_request.cpp:794).  n_pages must be a multiple of pages_per_slice. */
int cc_slice_fold(const uint32_t* page_crcs, uint64_t n_pages, uint32_t pages_per_slice, uint32_t page_bytes,
                  uint32_t* out);

/* ------------------------------------------------------------------------
 * Engine lifetime -- created next to ScanManager::Init and torn down at
 * ChunkServer::Fini (src/chunkserver/chunkserver.cpp:298-303, :455).
 * Optional: device calls initialise per-device state lazily.
 * ------------------------------------------------------------------------ */
typedef struct cc_opts {
    uint32_t page_bytes;     /* default 4096 (conf/chunkserver.conf:22 blocksize) */
    uint32_t slice_bytes;    /* default 4 MiB (copyset.scan_size_byte, conf/chunkserver.conf:114) */
    uint64_t staging_bytes;  /* pinned host staging per device for *_host calls, default 256 MiB */
} cc_opts;

int cc_engine_init(const cc_opts* opts);  /* NULL = defaults */
int cc_engine_fini(void);
/* Free the device memory the engine caches per stream on the calling thread's
 * device: the write log's hash tables (cc_apply_log_dev) and the range /
 * verify-on-read scratch (cc_crc_ranges_dev, cc_verify_reads_dev); the next
 * call re-creates what it needs.  The entries are detached under the engine's
 * locks, then the call waits for the device to be idle WITHOUT holding them
 * (other threads' calls proceed meanwhile) and frees them.  Entries of
 * hipStreamPerThread are also dropped when their thread exits. */
int cc_engine_trim(void);
/* Diagnostic: the per-stream entries (tail blocks, write-log tables, range
 * scratch) the engine holds on the calling thread's device right now. */
uint64_t cc_engine_stream_entries(void);
int cc_device_count(void);
const char* cc_strerror(int code);
const char* cc_version(void);

/* ------------------------------------------------------------------------
 * Device batch calls -- the hot path (replace the CRC32() loops of the scan
 * hasher, op_request.cpp:794/:847, and of the chunk/copyset hashers,
 * chunkserver_chunkfile.cpp:805, copyset_node.cpp:964).
 * ------------------------------------------------------------------------ */

/* d_out[i] = crc32c_value(d_pages + i*page_bytes, page_bytes).
 * page_bytes: multiple of 256, 256..1 MiB.  d_pages 4-byte aligned. */
int cc_page_crc_dev(const void* d_pages, uint64_t n_pages, uint32_t page_bytes,
                    uint32_t* d_out, void* stream);

/* Recompute and compare against d_expected.  *d_bad_count += mismatches;
 * *d_first_bad = min(*d_first_bad, first mismatching page index).  The caller
 * zeroes d_bad_count and sets d_first_bad to UINT64_MAX before the call. */
int cc_page_verify_dev(const void* d_pages, uint64_t n_pages, uint32_t page_bytes,
                       const uint32_t* d_expected, uint64_t* d_bad_count,
                       uint64_t* d_first_bad, void* stream);

/* cc_page_verify_dev plus the indices of the mismatching pages: the first
 * min(count, max_bad_pages) of them land in d_bad_pages[*d_bad_count_before ..]
 * in no particular order (the caller sorts).  Lets a scan report every bad page
 * (SURVEY §8d C1 "verify must flag exactly those") without a second pass.
 * d_bad_pages may be NULL only when max_bad_pages == 0. */
int cc_page_verify_list_dev(const void* d_pages, uint64_t n_pages, uint32_t page_bytes,
                            const uint32_t* d_expected, uint64_t* d_bad_count,
                            uint64_t* d_first_bad, uint64_t* d_bad_pages,
                            uint64_t max_bad_pages, void* stream);

/* Group fold: d_out[g] = CRC of the concatenation of units g*per_group ..
 * g*per_group+per_group-1, each unit_bytes long, from their CRCs d_crcs.
 * E.g. 1024 page CRCs -> one 4 MiB ScanMap.crc (proto/scan.proto:28). */
int cc_fold_dev(const uint32_t* d_crcs, uint64_t n_groups, uint32_t per_group,
                uint64_t unit_bytes, uint32_t* d_out, void* stream);

/* A byte range of a device buffer. */
typedef struct cc_range {
    uint64_t off;
    uint64_t len;
} cc_range;

/* d_out[i] = crc32c_value(d_buf + off_i, len_i) for arbitrary offsets,
 * alignments and lengths (0 allowed), e.g. raft WAL entries on replay -- the
 * data and header checksums CurveSegment::_load_entry verifies with
 * braft::crc32 (= butil::crc32c::Value), src/chunkserver/raftlog/curve_segment.cpp:307-371 --
 * or GetChunkHash's raw-file range (chunkserver_chunkfile.cpp:785-811).  The
 * batch is one stream of 4 KiB blocks split evenly over the device whatever
 * the range sizes (a range cut between waves is hashed in segments and
 * recombined), the last 1/32 handed out dynamically: ranges of any size mix
 * freely.  ONE launch: the waves count the batch's tiles themselves.  The
 * engine keeps scratch per stream for it (tile words, tail counters and the
 * split ranges' accumulator pairs: 8 B x the next power of two >= n, at least
 * 64 Ki pairs, plus ~9 KiB; at most 32 MiB + 9 KiB a stream -- a batch of more
 * than 4 Mi ranges takes scratch of its own for the call -- for at most 256
 * streams; shared with cc_verify_reads_dev; cc_engine_trim releases it).  The
 * scratch is left zero by every launch that completes; after a device fault
 * the context is unusable anyway (HIP errors are sticky) -- call
 * cc_engine_fini, or cc_engine_trim, before using the engine again. */
int cc_crc_ranges_dev(const void* d_buf, const cc_range* d_ranges, uint64_t n, uint32_t* d_out,
                      void* stream);

/* Host-resident variant for many separate buffers (e.g. the data of a batch
 * of WAL entries read from a segment file, CurveSegment::_load_entry,
 * curve_segment.cpp:307-371): h_out[i] = crc32c_value(h_bufs[i], h_lens[i]).
 * Buffers are packed into the pinned staging ring and hashed on the device by
 * the range kernel; a buffer larger than a staging slot is hashed in pieces
 * combined on the host.  Blocking, thread-safe. */
int cc_crc_bufs_host(const void* const* h_bufs, const uint64_t* h_lens, uint64_t n, uint32_t* h_out);

/* d_out[i] = x^(8 * d_nbytes[i]) mod P: the multiplier that shifts a CRC by
 * d_nbytes[i] bytes (precompute once per static pool layout for the epilogue's
 * digest). */
int cc_xpow8_dev(const uint64_t* d_nbytes, uint64_t n, uint32_t* d_out, void* stream);

/* Fused scan epilogue for whole chunks, ONE launch (replaces fold + fold +
 * combine + digest): from the page CRCs of n_chunks chunks (pages_per_chunk
 * each, contiguous) and their metapage CRCs produce
 *   d_slice_crcs[c*S + k]  S = pages_per_chunk / pages_per_slice   (ScanMap.crc)
 *   d_file_crcs[c]         CRC of metapage || data  (NULL = skip)
 *   d_digest[d_group[c]] ^= file CRC * d_after_mult[c]             (all three NULL = skip)
 * with d_after_mult[c] = x^(8 * bytes after file c in its copyset's sorted-name
 * chain) from cc_xpow8_dev.  Geometry: pages_per_chunk = 256*q; pages_per_slice
 * = q * 2^j, j in [0, 8] (16 MiB chunks, 4 KiB pages, 4 MiB slices: q = 16,
 * j = 6); CC_EINVAL otherwise. */
int cc_scan_epilogue_dev(const uint32_t* d_page_crcs, const uint32_t* d_meta_crcs, uint64_t n_chunks,
                         uint32_t pages_per_chunk, uint32_t page_bytes, uint32_t pages_per_slice,
                         uint32_t* d_slice_crcs, uint32_t* d_file_crcs, const uint32_t* d_after_mult,
                         const uint32_t* d_group, uint32_t* d_digest, void* stream);

/* Linear-domain digest contributions (per-copyset digest):
 * d_out[i] = crc32c_shift(d_crcs[i], d_shift_bytes[i]).  XOR of contributions
 * plus a length-only constant reproduces CopysetNode::GetHash's chain. */
int cc_shift_dev(const uint32_t* d_crcs, const uint64_t* d_shift_bytes, uint64_t n,
                 uint32_t* d_out, void* stream);

/* d_out[i] = crc32c_combine(d_a[i], d_b[i], len_b): e.g. a chunk FILE's CRC from
 * its metapage CRC and its 16 MiB data CRC (the file is metapage || data,
 * chunkserver_chunkfile.cpp:497-536 reads data at offset + metaPageSize). */
int cc_combine_dev(const uint32_t* d_a, const uint32_t* d_b, uint64_t len_b, uint64_t n,
                   uint32_t* d_out, void* stream);

/* Per-copyset digest partials: for each file i,
 *   d_digest[d_group[i]] ^= crc32c_shift(d_file_crcs[i], d_after_bytes[i])
 * where d_after_bytes[i] = bytes of the copyset's files that sort after file i
 * (CopysetNode::GetHash chains files in std::sort name order, copyset_node.cpp:938).
 * The XOR is order-free, so ranks holding disjoint file sets produce partials
 * whose XOR is exactly the reference's chained copyset hash.  d_digest is
 * caller-zeroed. */
int cc_digest_dev(const uint32_t* d_file_crcs, const uint64_t* d_after_bytes,
                  const uint32_t* d_group, uint64_t n_files, uint32_t* d_digest,
                  void* stream);

/* Device XOR fold of gathered digest partials: d_digest[i] = XOR over r <
 * nranks of d_gathered[r * n + i].  The local half of the per-copyset digest
 * exchange for callers that move the partials themselves (any
 * transport: RCCL all-gather, the MDS, a TCP store); cc_digest_allreduce_dev
 * runs it after its own RCCL all-gather. */
int cc_digest_fold_dev(const uint32_t* d_gathered, uint32_t nranks, uint64_t n, uint32_t* d_digest, void* stream);

/* ------------------------------------------------------------------------
 * Host-in / host-out convenience (blocking; thread-safe).  Starts and ends in
 * host memory like the reference's datastore read path (chunkserver_chunkfile.cpp:497-536).
 * ------------------------------------------------------------------------ */
/* h_out[i] = crc32c_value(h_pages + i*page_bytes, page_bytes).  A call of at
 * most 16 MiB (the scan op's shape: one 4 MiB slice or the 4 KiB metapage per
 * ScanChunkRequest, op_request.cpp:776-794, from up to wconcurrentapply.size =
 * 10 apply threads) runs on a LANE of its own -- device buffer, stream,
 * completion signal; up to 16 lanes per device, made on first demand, a caller
 * finding none idle waits -- so concurrent callers overlap their copies and
 * kernels.  A larger call takes the device's two-slot pinned staging ring,
 * held for the whole call.  Pinned input is DMA'd directly; pageable input is
 * copied through pinned staging.  The caller sleeps until done: a lane call on
 * a word its stream writes after the kernel (no HIP wait, so no thread spins
 * for it: ~10 us of process CPU for a 4 KiB call, ~40 us for 4 MiB), a large
 * call on a condition variable. */
int cc_page_crc_host(const void* h_pages, uint64_t n_pages, uint32_t page_bytes,
                     uint32_t* h_out);

/* One byte-range write into a device-resident pool (client partial write). */
typedef struct cc_update {
    uint64_t dst; /* byte offset in the pool */
    uint64_t src; /* byte offset in the source buffer */
    uint32_t len; /* bytes, >= 1 */
    uint32_t reserved;
} cc_update;

/* Client partial-write path (BASELINE config 3), the drop-in for the write
 * loop of WriteChunkRequest::OnApply -> CSChunkFile::Write (op_request.cpp:429-481,
 * chunkserver_chunkfile.cpp:287-427, which applies writes in raft-log order);
 * the per-page CRC table is new.  d_log[0..n) is the ORDERED write
 * log: entries may overlap, have any alignment and straddle pages; later
 * entries win.  Every entry becomes one piece per page it touches; the pieces
 * are grouped by page in a device hash table (one 64-bit CAS per piece: no
 * sort, no host planning), and one wave per touched page applies that page's
 * pieces in log order in registers, stores the changed 256-byte rows and
 * writes the page's new CRC to d_page_crcs (untouched pages keep theirs).
 * Two launches (insert, pages); a log of <= 64 entries no longer than a page
 * takes one.  The hash table is the engine's, one per stream, created (and
 * grown) on the stream on first use and left clear by every call, so no call
 * clears it; calls sharing a stream are serialised by the engine while they
 * enqueue.  Retained device memory: 8 B x the next power of two >= 8 x the
 * pieces (n_updates x ((max_len - 1) / page_bytes + 2)) per stream, at most
 * 64 MiB a stream (a log needing more takes a table for that call only), for
 * at most 256 streams; the null stream and hipStreamLegacy are one stream,
 * hipStreamPerThread counts once per calling thread (its entry is dropped when
 * the thread exits).  cc_engine_trim releases them.  Contract per entry: 1 <= len <= max_len and
 * dst + len <= pool_bytes -- an entry that breaks it is skipped whole (never
 * half-applied); d_src must not alias d_pool.  page_bytes = 256 * 2^k
 * (k = 0..5).  d_work: >= cc_apply_log_work_bytes(n, max_len, page_bytes) bytes
 * (the pieces' list links and the touched-page list; no clearing needed;
 * 0 = unsupported sizes: a table of more than 2^32 slots). */
uint64_t cc_apply_log_work_bytes(uint64_t n_updates, uint32_t max_len, uint32_t page_bytes);
int cc_apply_log_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const void* d_src,
                     const cc_update* d_log, uint64_t n_updates, uint32_t max_len, uint32_t* d_page_crcs,
                     void* d_work, uint64_t work_bytes, void* stream);

/* The same write log, with d_page_crcs[p] taken as the CRC of page p BEFORE
 * the batch and updated incrementally: V(new) = V(old) ^ raw(old ^ new) for
 * equal-length pages, so only the 256-byte rows the writes touch are read
 * (a page with several writes reads whole).  Identical output to
 * cc_apply_log_dev whenever the stored CRCs matched the pages; a page whose
 * stored CRC did not match (latent corruption) keeps mismatching after the
 * write instead of receiving a fresh CRC over the corrupt bytes.  Same
 * contract and work size as cc_apply_log_dev. */
int cc_apply_log_delta_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const void* d_src,
                           const cc_update* d_log, uint64_t n_updates, uint32_t max_len, uint32_t* d_page_crcs,
                           void* d_work, uint64_t work_bytes, void* stream);

/* Copy on write for chunks with an open snapshot: the step CSChunkFile::Write
 * runs between its sn update and writeData (needCow(sn), then
 * copy2Snapshot(offset, length): chunkserver_chunkfile.cpp:381-396, :848-884,
 * :912-963), one page being one block.  Before the batch's writes land, every
 * page the log touches (a page that gets at least one piece: an entry that
 * breaks the contract gets none and copies nothing) whose chunk has a snapshot
 * slot below n_slots and whose bit in that slot's bitmap is clear has its old
 * bytes copied into the slot at the same chunk offset, d_page_crcs[p] MOVED
 * (not recomputed) to d_snap_crcs, and its bit set.  A page whose bit is set is
 * left alone: the snapshot keeps the first version, as Divide(...,
 * &uncopiedRange, nullptr) does.  A slot index >= n_slots is CC_NO_SNAPSHOT:
 * nothing is ever written outside d_snap.  Then the batch is applied exactly as
 * cc_apply_log_dev (delta = 0) or cc_apply_log_delta_dev (delta != 0) applies
 * it: the pool bytes and d_page_crcs are theirs, bit for bit; cow == NULL IS
 * that call.  One more launch between the two (three in all; a log of <= 64
 * entries takes them too: the one-launch path keeps no touched-page list).
 *
 * The struct is a HOST struct of device pointers, like cc_pool_shard.  In full
 * mode too, d_page_crcs is an INPUT for the copied pages (as it always is in
 * delta mode): it must hold the CRCs of the pages before the batch.
 *
 * needCow is decided per request in the reference; here per chunk per CALL:
 * d_snap_slot is read once, before any write of the batch.  The caller splits
 * a batch at the request that creates a snapshot (a rare event: one per chunk
 * per volume snapshot).
 *
 * d_stale, when non-NULL, is the optional check: the pass also rehashes every
 * page it copies and counts those whose bytes disagree with their stored CRC.
 * Such a page is still copied with its stored CRC, so the mismatch survives in
 * the snapshot (delta mode's rule for latent corruption).  With d_stale NULL
 * the pass does no CRC work at all.
 *
 * Checked before a device is needed (CC_EINVAL): chunk_bytes a multiple of
 * page_bytes that divides pool_bytes; every pointer but the two counters
 * non-NULL; d_snap 4-byte aligned.
 *
 * Not covered by this call: a queue of batches (that is cc_apply_logs_cow_dev:
 * one pass before the whole queue, then cc_apply_logs_dev's launches, so a
 * pool with open snapshots keeps the pipelined queue); clone chunks and Paste
 * (cc_paste_dev, cc_clone_mark_dev).  (Reading a snapshot back:
 * cc_read_snap_dev.) */
#define CC_NO_SNAPSHOT 0xFFFFFFFFu
typedef struct cc_cow {
    uint32_t chunk_bytes;         /* a multiple of page_bytes; pool_bytes a multiple of it */
    uint32_t n_slots;             /* snapshot slots behind d_snap */
    const uint32_t* d_snap_slot;  /* [pool_bytes / chunk_bytes] slot of chunk c's open snapshot, or
                                     CC_NO_SNAPSHOT (needCow false: written in place) */
    void* d_snap;                 /* n_slots x chunk_bytes; slot s holds the copied pages at their chunk offsets */
    uint32_t* d_snap_crcs;        /* n_slots x pages_per_chunk */
    uint32_t* d_snap_bitmap;      /* n_slots x ceil(pages_per_chunk / 32) words; page q of a slot is bit q % 32 of
                                     word q / 32 = bit q % 8 of byte q / 8 (common/bitmap.h:196-199): the bytes
                                     of a slot ARE SnapshotMetaPage's bitmap (cc_snap_meta_encode) */
    uint64_t* d_copied;           /* optional: += pages copied by the call */
    uint64_t* d_stale;            /* optional: += copied pages whose bytes did not match d_page_crcs */
} cc_cow;
int cc_apply_log_cow_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const void* d_src,
                         const cc_update* d_log, uint64_t n_updates, uint32_t max_len, uint32_t* d_page_crcs,
                         void* d_work, uint64_t work_bytes, void* stream, int delta, const cc_cow* cow);

/* A QUEUE of write logs applied in order, as n_batches cc_apply_log_dev calls
 * (delta = 0) or cc_apply_log_delta_dev calls (delta = 1) would be on `stream`:
 * the same pool bytes and page CRCs, bit for bit.  Pipelined: the page kernel
 * of batch k also groups batch k+1's pieces in its tail (workgroups done with
 * their pages insert them into the other half of the stream's engine table,
 * which is kept at twice the single-batch size, and the other of two work
 * regions), so only the first batch (and one after a <= 64-write batch, which
 * takes the one-launch path) pays the separate grouping launch and the kernel
 * boundary behind it.  `batches` is a
 * HOST array (its device pointers: as for cc_apply_log_dev, valid until the
 * stream has run the call's work); empty batches are skipped.  d_work: >=
 * cc_apply_logs_work_bytes(largest batch's n_updates, max_len, page_bytes).
 * A stream without an engine table (more than 256 streams hold one) takes one
 * call per batch.  Replaces a chunkserver's apply loop over its queued write
 * requests (ChunkOpRequest::OnApply per write, op_request.cpp:429-481). */
typedef struct cc_log_batch {
    const void* d_src;        /* device: the batch's data (its records' src offsets) */
    const cc_update* d_log;   /* device: the batch's records, log order */
    uint64_t n_updates;
} cc_log_batch;
uint64_t cc_apply_logs_work_bytes(uint64_t max_updates, uint32_t max_len, uint32_t page_bytes);
int cc_apply_logs_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const cc_log_batch* batches,
                      uint32_t n_batches, uint32_t max_len, uint32_t* d_page_crcs, int delta, void* d_work,
                      uint64_t work_bytes, void* stream);

/* Verify-on-read for a batch of datastore reads (the read path of
 * CSChunkFile::Read, chunkserver_chunkfile.cpp:497-536, which today returns the
 * bytes unchecked): every page that read i = d_reads[i] (pool byte range, any
 * offset/length; a partly covered page is verified whole) touches is rehashed
 * and compared with its stored CRC in d_page_crcs.  d_bad_per_read[i] += the
 * mismatching pages of read i (caller zeroes it; UINT32_MAX marks a read that
 * runs past the pool); *d_bad_total += all mismatches.  Every touched page is
 * one work slot and the slots are split evenly over the device, so reads of
 * any size mix freely.  page_bytes = 256 * 2^k (k = 0..5).  ONE launch on the
 * range kernel's schedule, using the stream's range scratch the engine keeps
 * (see cc_crc_ranges_dev).  d_work / work_bytes are kept for ABI stability
 * only: cc_verify_reads_work_bytes returns a constant 256 and d_work must be
 * non-NULL, but the engine does not touch it. */
uint64_t cc_verify_reads_work_bytes(uint64_t n_reads);
int cc_verify_reads_dev(const void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const cc_range* d_reads,
                        uint64_t n_reads, const uint32_t* d_page_crcs, uint32_t* d_bad_per_read,
                        uint64_t* d_bad_total, void* d_work, uint64_t work_bytes, void* stream);

/* Snapshot reads: a batch of reads of chunks AS THEY WERE when their snapshot
 * was taken, verified and gathered on the device.  Replaces the host loop of
 * CSChunkFile::ReadSpecifiedChunk (chunkserver_chunkfile.cpp:550-636:
 * Divide(begin, end, &uncopied, &copied), then readData for the uncopied
 * ranges and snapshot_->Read for the copied ones), which returns the bytes
 * unchecked; with cow == NULL it is a verified, gathering CSChunkFile::Read
 * (:497-536, the sn == metaPage_.sn branch).
 *
 * Reads are pool byte ranges as for cc_verify_reads_dev, but off and len must
 * be multiples of page_bytes (one page is one block, the COW call's
 * convention; CheckOffsetAndLength, chunkserver_chunkfile.h:386-394).  A read
 * may cross chunk boundaries: every page is resolved on its own.  For pool
 * page p, chunk c = p / pages_per_chunk, page in chunk q = p % pages_per_chunk
 * and slot s = cow->d_snap_slot[c]: when cow != NULL, s < cow->n_slots and bit
 * q of slot s's bitmap is set, the page's bytes are d_snap + (s *
 * pages_per_chunk + q) * page_bytes and its expected CRC d_snap_crcs[s *
 * pages_per_chunk + q]; otherwise (CC_NO_SNAPSHOT, any slot >= n_slots, a
 * clear bit, cow == NULL) they are the live pool page and d_page_crcs[p].  A
 * live page under a set bit is not part of the view: it is neither read nor
 * checked.  `cow` is the struct cc_apply_log_cow_dev takes; d_copied and
 * d_stale are ignored and everything is read only.  The caller must not run a
 * COW batch over the same slots on another stream at the same time.
 *
 * Every page of every valid read is rehashed whole and compared with its
 * expected CRC: d_bad_per_read[i] += the mismatching pages of read i (the
 * caller zeroes it), *d_bad_total += all mismatches.  With d_out != NULL the
 * page's bytes are also stored at d_out + d_out_off[i] + (page start - off_i),
 * whether or not the page matched (the reference returns bytes unchecked; the
 * counts tell the caller what to do with them).  d_out == NULL verifies only:
 * d_out_off may be NULL and out_bytes is ignored.  Overlapping output ranges
 * are the caller's business.
 *
 * A read is INVALID -- d_bad_per_read[i] = UINT32_MAX, not hashed, nothing
 * written -- when its off or len is misaligned, when it runs past the pool
 * (off >= pool_bytes or len > pool_bytes - off) or, with d_out, when
 * d_out_off[i] is not 4-byte aligned or d_out_off[i] + len > out_bytes.
 * Nothing is ever written outside [d_out, d_out + out_bytes).  len == 0 is
 * valid whatever its off: it touches nothing and leaves its word alone.
 *
 * Checked before a device is needed (CC_EINVAL): page_bytes = 256 * 2^k
 * (k = 0..5); pool_bytes whole pages; d_pool 4-byte aligned; d_pool, d_reads,
 * d_page_crcs, d_bad_per_read, d_bad_total non-NULL; d_out non-NULL with a
 * NULL d_out_off or not 4-byte aligned; with cow, chunk_bytes a multiple of
 * page_bytes that divides pool_bytes, its slot, snap, CRC and bitmap pointers
 * non-NULL and d_snap 4-byte aligned; n_reads < 2^31.  n_reads == 0 is CC_OK.
 * No GPU: CC_ENODEV, never a CPU fallback.
 *
 * ONE launch on verify-on-read's schedule (every touched page one slot, the
 * slots split evenly over the device, the last 1/16 dynamically), using the
 * stream's range scratch the engine keeps (see cc_crc_ranges_dev; shared with
 * cc_verify_reads_dev, no caller work buffer); a batch of <= 64 reads on a
 * pool of < 2^26 pages takes one launch with no scratch at all. */
int cc_read_snap_dev(const void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const cc_range* d_reads,
                     uint64_t n_reads, const uint32_t* d_page_crcs, const cc_cow* cow, void* d_out,
                     const uint64_t* d_out_off, uint64_t out_bytes, uint32_t* d_bad_per_read, uint64_t* d_bad_total,
                     void* stream);

/* Clone chunks: the written-page bitmap on the device.  A clone chunk is
 * allocated lazily (clone, or recover from a snapshot in S3 or another volume)
 * and carries, in its metapage, one bit per page that has been written; the
 * first three calls below are the three places where CSChunkFile looks at or
 * changes that bitmap, for a pool some of whose chunks are clones, and
 * cc_read_merge_dev is CloneCore's read of such a chunk.  A clone chunk can
 * never open a snapshot (Write returns StatusConflictError,
 * chunkserver_chunkfile.cpp:329-336), so these calls and cc_apply_log_cow_dev
 * never meet on one chunk.
 *
 * The struct is a HOST struct of device pointers, like cc_cow, and follows its
 * slot and bitmap conventions: chunk c's bitmap is slot d_clone_slot[c]; any
 * value >= n_slots (CC_NOT_CLONE) says the chunk is not a clone, and nothing of
 * it is ever looked up behind d_bitmap or d_claim.  d_claim is cc_paste_dev's
 * scratch, kept by the caller beside the bitmaps: all 0xFFFFFFFF before the
 * first call, and every call that completes leaves it so. */
#define CC_NOT_CLONE 0xFFFFFFFFu
typedef struct cc_clone {
    uint32_t chunk_bytes;            /* a multiple of page_bytes that divides pool_bytes */
    uint32_t n_slots;                /* clone bitmaps behind d_bitmap */
    const uint32_t* d_clone_slot;    /* [pool_bytes / chunk_bytes]: chunk c's bitmap index; any value >= n_slots
                                        (CC_NOT_CLONE) = not a clone chunk */
    uint32_t* d_bitmap;              /* n_slots x ceil(pages_per_chunk / 32) words; bit q % 32 of word q / 32 =
                                        bit q % 8 of byte q / 8: a slot's bytes ARE ChunkFileMetaPage's bitmap */
    uint32_t* d_claim;               /* n_slots x pages_per_chunk words, all 0xFFFFFFFF on entry; every call that
                                        completes leaves them so (the engine tables' convention) */
    uint64_t* d_pasted;              /* optional: += pages pasted by cc_paste_dev */
} cc_clone;

/* Paste: origin data lands only where nothing was written yet.  Replaces the
 * host loop of CSChunkFile::Paste (chunkserver_chunkfile.cpp:440-495:
 * Divide(begin, end, &uncopied, nullptr), writeData per uncopied range, then
 * flush() sets the bits; Success and nothing written on a non-clone chunk),
 * which PasteChunkInternalRequest::OnApply runs for CloneCore::PasteCloneData
 * (op_request.cpp:725-747, clone_core.cpp:418-460).  d_pastes[0..n) is an
 * ORDERED batch, applied as n Paste calls in that order would be: concurrent
 * reads of one unwritten region each fetch the origin and each paste, and the
 * first paste applied wins every page.
 *
 * Per pool page, by its chunk and bit as they stood BEFORE the call: a page of
 * a clone chunk whose bit is clear is written exactly once, from the
 * LOWEST-indexed valid entry covering it -- its bytes are d_src + src_i +
 * (page start - dst_i), its bit is set (an atomic OR on its word) and
 * d_page_crcs[p] becomes the CRC of the new bytes, hashed as the page passes
 * through registers; a page whose bit is set, and any page of a chunk that is
 * not a clone, keeps its bytes and its CRC.  An entry may cross chunk
 * boundaries: every page is resolved on its own, as in cc_read_snap_dev.
 * d_pasted_per_entry[i] += the pages entry i pasted (the caller zeroes it),
 * *clone->d_pasted += all of them.  With the lowest-index rule the pool, the
 * CRC table, the bitmaps and both counts are deterministic.
 *
 * An entry is INVALID -- d_pasted_per_entry[i] = UINT32_MAX, nothing written,
 * nothing claimed -- when dst or len is not a multiple of page_bytes
 * (CheckOffsetAndLength, chunkserver_chunkfile.h:386-394), when it runs past
 * the pool (dst >= pool_bytes or len > pool_bytes - dst), when src is not
 * 4-byte aligned or when src + len > src_bytes.  len == 0 is valid: it touches
 * nothing and leaves its word alone.  d_src must not alias d_pool.
 *
 * Checked before a device is needed (CC_EINVAL): page_bytes = 256 * 2^k
 * (k = 0..5); pool_bytes whole pages; d_pool and d_src 4-byte aligned; d_pool,
 * d_src, d_pastes, d_page_crcs, d_pasted_per_entry, clone and clone's
 * d_clone_slot, d_bitmap, d_claim non-NULL; chunk_bytes a multiple of
 * page_bytes that divides pool_bytes; n < 2^31 (entry indices live in d_claim,
 * all-ones reserved).  n == 0 is CC_OK.  No GPU: CC_ENODEV, never a CPU
 * fallback.
 *
 * Two launches on `stream`.  CLAIM: one lane per (valid entry, page), no page
 * traffic; where the page's chunk is a clone and its bit is clear,
 * atomicMin(d_claim[s * pages_per_chunk + q], i); it also marks the invalid
 * entries.  PASTE: every (entry, page) pair is one slot on verify-on-read's
 * schedule (the slots split evenly over the device, the last 1/16 dynamically,
 * using the stream's range scratch the engine keeps: no caller work buffer);
 * the slot whose claim word equals its entry index copies and hashes the page,
 * writes the CRC, sets the bit, counts and puts 0xFFFFFFFF back; every other
 * slot loads no page.  The bitmap is only read in the first launch and only
 * written in the second.  The caller must not run another call over the same
 * bitmaps on another stream at the same time. */
int cc_paste_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const void* d_src, uint64_t src_bytes,
                 const cc_update* d_pastes, uint64_t n, uint32_t* d_page_crcs, const cc_clone* clone,
                 uint32_t* d_pasted_per_entry, void* stream);

/* The flush() half of CSChunkFile::Write on clone chunks
 * (chunkserver_chunkfile.cpp:405-406, :965-1000: the bits of the pages the
 * write covered are set, so that a later Paste does not bury a user write
 * under origin data).  Enqueue it after the cc_apply_log*_dev call for the
 * same log on the same stream.  For every entry that keeps the write log's
 * contract (1 <= len <= max_len, dst + len <= pool_bytes; any other entry is
 * skipped, as the log call skips it), every page the entry covers WHOLE whose
 * chunk is a clone gets its bit set.  A partly covered page keeps its bit --
 * the reference only accepts block-aligned writes, and declaring a page
 * written while part of it was never filled would let a read return garbage
 * silently -- and two partial entries that together cover a page do not count.
 * One launch; it touches neither d_claim nor any page.  The checks are
 * cc_paste_dev's where they apply: page_bytes, pool_bytes whole pages, d_log
 * and clone (with its three pointers) non-NULL, chunk_bytes, max_len >= 1,
 * n_updates < 2^31; n_updates == 0 is CC_OK; no GPU: CC_ENODEV.  When the last
 * bit of a chunk is set the chunk has become an ordinary one (:972-996): the
 * caller sees that in the bitmap it reads back for the metapage. */
int cc_clone_mark_dev(uint64_t pool_bytes, uint32_t page_bytes, const cc_update* d_log, uint64_t n_updates,
                      uint32_t max_len, const cc_clone* clone, void* stream);

/* The QUEUE of write logs (cc_apply_logs_dev) for a pool with open snapshots
 * and/or clone chunks: the pipelined queue, with the copy-on-write pass and the
 * clone marks of ALL its batches done in one pass before its first write.
 *
 * Equivalence: for every non-empty batch k in order, take
 * cc_apply_log_cow_dev(batch k, delta, cow) followed, when clone != NULL, by
 * cc_clone_mark_dev(batch k's log, max_len, clone), all on `stream`.  This call
 * leaves the pool, d_page_crcs, d_snap (copied pages only; every other slot
 * byte untouched), d_snap_crcs, d_snap_bitmap, *d_copied, *d_stale and the
 * clone d_bitmap bit for bit as that sequence leaves them.  Why one pass up
 * front is enough: d_snap_slot is read once per call; a snapshot keeps a page's
 * FIRST version; and the first batch of the queue that touches page p finds p
 * and d_page_crcs[p] exactly as they stood before the queue.  The clone marks
 * are idempotent ORs that no log kernel reads.  d_claim is not touched.
 * Nothing is written outside d_snap for a slot >= n_slots, or behind d_bitmap
 * for a CC_NOT_CLONE chunk.
 *
 * cow == NULL && clone == NULL IS cc_apply_logs_dev: same code path, same
 * launches.  Either struct alone is allowed.  A chunk that carries both a
 * snapshot slot and a clone slot is a caller error in the reference; here each
 * struct is applied on its own terms and nothing is undefined.
 *
 * Per entry the write log's rule holds: 1 <= len <= max_len, dst < pool_bytes,
 * len <= pool_bytes - dst; an entry that breaks it copies nothing, marks
 * nothing and writes nothing.  A page is copied when a valid entry touches it
 * (cc_apply_log_cow_dev's rule); a clone bit is set only for a page that one
 * entry covers WHOLE (cc_clone_mark_dev's rule: a partly covered page keeps its
 * bit, and two partial entries that together cover a page do not count).
 * d_stale, when non-NULL, makes the pass rehash every page it copies, as in
 * cc_apply_log_cow_dev.  In full mode too d_page_crcs must hold the CRCs of
 * the pages before the queue.
 *
 * d_work / work_bytes: as for cc_apply_logs_dev (cc_apply_logs_work_bytes);
 * the pass needs no caller memory, makes no host-to-device copy and allocates
 * nothing: the batch descriptors ride in the kernel argument, 32 a launch.
 *
 * Checked before a device is needed (CC_EINVAL): cc_apply_logs_dev's checks;
 * cc_apply_log_cow_dev's checks on cow; cc_clone_mark_dev's checks on clone,
 * every batch's n_updates < 2^31 among them.  A malformed cow or clone is
 * refused even for an empty queue.  n_batches == 0, or only empty batches:
 * CC_OK.  No GPU: CC_ENODEV, never a CPU fallback.
 *
 * Launches: ceil(non-empty batches / 32) for the pass, then exactly those of
 * cc_apply_logs_dev: batches of <= 64 entries no longer than a page keep the
 * one-launch path, and a stream without an engine table takes the pass and
 * then one plain cc_apply_log*_dev per batch.  needCow is decided per chunk per
 * CALL, as in cc_apply_log_cow_dev: the caller splits a queue at the request
 * that creates a snapshot.  The caller must not run another call over the same
 * slots or bitmaps on another stream at the same time.  Paste inside the queue:
 * cc_apply_ops_dev. */
int cc_apply_logs_cow_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const cc_log_batch* batches,
                          uint32_t n_batches, uint32_t max_len, uint32_t* d_page_crcs, int delta, void* d_work,
                          uint64_t work_bytes, void* stream, const cc_cow* cow, const cc_clone* clone);

/* The queue with PASTE BATCHES in it: a chunkserver's whole apply loop in one
 * call.  In the reference a paste is a raft op like a write
 * (PasteChunkInternalRequest::OnApply, op_request.cpp:725-747) and sits in the
 * same apply queue, in log order; a lazily cloned volume produces them all the
 * time (every clone read of a never-written region pastes what it fetched, and
 * CHUNK_OP_RECOVER does nothing else).  ops[0..n_ops) is a HOST array (device
 * pointers valid until the stream has run the call's work) of batches in queue
 * order, each a write log (CC_OP_WRITE: d_src, d_recs, n as cc_log_batch) or a
 * paste batch (CC_OP_PASTE: d_src, src_bytes, d_recs, n, d_pasted_per_entry as
 * cc_paste_dev's arguments); empty batches are skipped.
 *
 * THE SEQUENCE this call stands for: per batch, in order, on `stream` --
 *   write:  cc_apply_log_cow_dev(batch, delta, cow), then cc_clone_mark_dev(batch's log, max_len, clone);
 *   paste:  cc_paste_dev(batch).
 *
 * THE MODEL this call computes.  Number the entries of all batches 0, 1, 2, ...
 * in queue order: an entry's ORDINAL.  For a page p of a clone chunk whose bit is
 * clear before the call, p's FIRST SETTER is the lowest-ordinal entry that is a
 * valid paste entry covering p or a valid write entry covering p WHOLE.
 *   1. Every page whose first setter is a paste entry is pasted as cc_paste_dev
 *      pastes it: that entry's bytes, a fresh CRC in d_page_crcs, the bit set,
 *      +1 on the entry's d_pasted_per_entry word and on *clone->d_pasted.
 *   2. Then the write batches run, in order, as cc_apply_logs_cow_dev(write
 *      batches, delta, cow, clone) runs them.
 * The call leaves the pool, d_page_crcs, the snapshot arrays, the clone bitmaps,
 * every d_pasted_per_entry, *clone->d_pasted and *d_contested exactly so.
 *
 * Relation to the sequence.  Which entry pastes a page is the same in both (the
 * pre-queue bits and the records decide it, never bytes), so the bitmaps, every
 * d_pasted_per_entry word and *d_pasted are ALWAYS those of the sequence.  A
 * (write entry, page) pair is CONTESTED when the valid write entry touches p
 * without covering it whole and p's first setter is a paste entry of a higher
 * ordinal.  *d_contested += the number of such pairs (d_contested may be NULL).
 * With no contested pair the result equals the sequence's bit for bit, in full
 * and in delta mode: nothing reads or writes p, its CRC word or its bit before
 * its paste, and the pasted page gets a fresh CRC before any delta touches it.
 * On a contested page the bytes and the CRC word differ, and nothing else: the
 * sequence lets the later paste bury the partial write; here the partial write
 * lands on top of the origin data (origin bytes with the queue's writes applied
 * in order), which is what a lazy clone should hold.  The reference accepts only
 * block-aligned writes, so it has no contested pair.
 *
 * Per entry.  Write: the write log's rule, unchanged (1 <= len <= max_len, dst <
 * pool_bytes, len <= pool_bytes - dst; else skipped whole).  Paste:
 * cc_paste_dev's four rules (dst and len page multiples; inside the pool; src
 * 4-byte aligned; src + len <= src_bytes) and len <= max_paste_len, a multiple of
 * page_bytes, which makes a paste batch's (entry, page) pair space static as
 * max_len does for writes.  An invalid paste entry gets UINT32_MAX in its word,
 * bids for nothing and writes nothing; len == 0 is valid and inert.
 *
 * d_claim: all 0xFFFFFFFF on entry, and left so by every completed call.
 *
 * Reductions.  A queue with no non-empty paste batch IS cc_apply_logs_cow_dev
 * over its write batches: same code path, same launches (clone and
 * max_paste_len are then not needed).  With paste batches, the launches after
 * the new passes are exactly those of cc_apply_logs_cow_dev over the write
 * batches.  The passes, all on `stream`, each kind finished over all its
 * launches before the next begins, 32 batch descriptors a launch riding in the
 * kernel argument (no caller memory, no host-to-device copy, no allocation):
 *   BID      a lane per (entry, page) pair of batches 0 .. the last paste batch:
 *            a paste pair, and a write pair that covers its page whole, bids with
 *            atomicMin(d_claim[page], 2 x ordinal + kind) where the page's chunk
 *            is a clone and its bit is clear; marks invalid paste entries; reads
 *            bitmaps, writes none.  (Later writes cannot change a winner.)
 *   RESOLVE  the write pairs of those batches: a pair that finds its own key
 *            puts all-ones back; a partial cover that finds the key of a paste of
 *            a higher ordinal counts one contested pair.
 *   PASTE    the pairs of all paste batches: the pair that finds its own key
 *            loads its source page, hashes it in registers, stores it, writes
 *            the CRC, ORs the bit, counts and resets the claim word.
 * d_work / work_bytes: as for cc_apply_logs_dev, sized by the largest WRITE
 * batch (not needed without write entries).  Measured: what the call
 * saves is per paste batch, so it pays for the small, frequent paste batches of
 * clone reads; PASTE moves pages about 7 % slower than cc_paste_dev's second
 * launch, so a paste batch as large as a write batch is as well served by its
 * own cc_paste_dev call between two queues.
 *
 * A chunk that carries both a snapshot slot and a clone slot is a caller error
 * (cc_apply_logs_cow_dev).  Here the paste passes run first and the queue's
 * copy-on-write pass after them, so such a chunk's snapshot would hold pasted
 * pages; every access stays inside the arrays either way.
 *
 * Checked before a device is needed (CC_EINVAL): cc_apply_logs_cow_dev's checks
 * on the write batches, cow and clone; per non-empty paste batch cc_paste_dev's
 * (d_src, d_recs, d_pasted_per_entry non-NULL, d_src 4-byte aligned), and with
 * one such batch: d_pool and d_page_crcs non-NULL, d_pool 4-byte aligned,
 * pool_bytes whole pages, clone required (cc_paste_dev's checks on it),
 * max_paste_len a non-zero multiple of page_bytes, and n x (max_paste_len /
 * page_bytes) < 2^32 per paste batch (a batch's pairs are indexed in 32 bits);
 * a kind other than the two; reserved != 0; ops NULL with n_ops > 0; the entries
 * of all batches together >= 2^31 - 1 (ordinals live in d_claim).  n_ops == 0,
 * or only empty batches: CC_OK.  No GPU: CC_ENODEV, never a CPU fallback.  The
 * caller must not run another call over the same bitmaps on another stream at
 * the same time, nor enqueue one on the same stream from another thread while
 * this call enqueues (its passes and the queue's launches must reach the stream
 * as one group, as a cc_paste_dev call's two launches must).  Not covered:
 * sequence-exact bytes on contested pages. */
#define CC_OP_WRITE 0u
#define CC_OP_PASTE 1u
typedef struct cc_op_batch {
    uint32_t kind;                 /* CC_OP_WRITE | CC_OP_PASTE */
    uint32_t reserved;             /* 0 */
    const void* d_src;             /* the batch's data / origin buffer */
    uint64_t src_bytes;            /* paste: bounds of d_src (cc_paste_dev's rule); write: ignored */
    const cc_update* d_recs;       /* records, in order */
    uint64_t n;
    uint32_t* d_pasted_per_entry;  /* paste: [n], zeroed by the caller; write: ignored */
} cc_op_batch;
int cc_apply_ops_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const cc_op_batch* ops, uint32_t n_ops,
                     uint32_t max_len, uint32_t max_paste_len, uint32_t* d_page_crcs, int delta, void* d_work,
                     uint64_t work_bytes, void* stream, const cc_cow* cow, const cc_clone* clone,
                     uint64_t* d_contested /* optional */);

/* The NextClearBit test of CSChunkFile::Read on a clone chunk
 * (chunkserver_chunkfile.cpp:510-526: a range with any clear bit is refused
 * with PageNerverWrittenError) and of CloneCore::HandleReadRequest
 * (clone_core.cpp:166: must the origin be fetched at all), for a batch.  Reads
 * are pool byte ranges of any offset and length, as for cc_verify_reads_dev; a
 * partly covered page counts.  d_unwritten_per_read[i] += the pages of read i
 * that lie in a clone chunk with a clear bit (the caller zeroes it),
 * *d_unwritten_total += their sum; UINT32_MAX marks a read that runs past the
 * pool; len == 0 touches nothing.  A non-zero count is the reference's
 * PageNerverWrittenError, or "fetch the origin, answer with cc_read_merge_dev
 * and cc_paste_dev it"; a read with count 0 may go to cc_verify_reads_dev,
 * cc_read_snap_dev or cc_read_merge_dev.  It reads
 * bitmap words only, in one launch.  Checks as cc_paste_dev's where they
 * apply, with d_reads and both counters non-NULL and n_reads < 2^31. */
int cc_clone_check_reads_dev(uint64_t pool_bytes, uint32_t page_bytes, const cc_range* d_reads, uint64_t n_reads,
                             const cc_clone* clone, uint32_t* d_unwritten_per_read, uint64_t* d_unwritten_total,
                             void* stream);

/* Clone reads: a batch of CloneCore::ReadThenMerge calls (clone_core.cpp:352-416:
 * Divide() the request's blocks into copied and uncopied ranges, ReadChunk per
 * copied range, cloneData->copy_to per uncopied one), fed as
 * SetReadChunkResponse feeds them -- the read of a clone chunk answered from
 * the written pages of the pool and the unwritten pages of the fetched origin
 * buffer, in ONE gathered, verified call.  It sits between
 * cc_clone_check_reads_dev (which reads must fetch their origin) and
 * cc_paste_dev (the optional, asynchronous PasteCloneData): the answer never
 * waits for the paste.
 *
 * Reads follow cc_read_snap_dev's conventions: pool byte ranges whose off and
 * len are multiples of page_bytes (CloneReadByLocalInfo refuses anything else,
 * clone_core.cpp:145-157); a read may cross chunk boundaries, and every page is
 * resolved on its own.  `clone` is cc_paste_dev's struct; the call reads
 * d_clone_slot and d_bitmap only, never touches d_claim or d_pasted (both may
 * be NULL) and writes no bitmap.  For pool page p of read i, chunk c = p /
 * pages_per_chunk, q = p % pages_per_chunk and s = d_clone_slot[c]:
 *
 * WRITTEN -- s >= n_slots (not a clone, out-of-range values included) or bit q
 * of slot s set: the bytes are the live pool page, rehashed whole and compared
 * with d_page_crcs[p]; a mismatch adds 1 to d_bad_per_read[i] and to
 * *d_bad_total; the bytes go to d_out + d_out_off[i] + (page start - off_i)
 * whether or not they matched (cc_read_snap_dev's rule).
 *
 * NEVER WRITTEN -- s < n_slots and bit q clear: the pool page and its CRC word
 * are not read; d_unwritten_per_read[i] and *d_unwritten_total each get +1
 * (the caller zeroes them).  If the read has an origin (d_origin != NULL and
 * d_origin_off[i] != CC_NO_ORIGIN) the page's bytes are d_origin +
 * d_origin_off[i] + (page start - off_i), stored at the same output position
 * UNHASHED: the origin has no stored CRC to check against, and the reference
 * returns it as downloaded.  If the read has no origin the output bytes of
 * that page are left untouched; a non-zero count on such a read is the
 * reference's PageNerverWrittenError.
 *
 * Every page is judged by the bitmaps as they stood before the call (the call
 * writes none), so the result does not depend on the schedule.  d_out must not
 * alias d_pool or d_origin, and no cc_paste_dev, cc_clone_mark_dev or write
 * log may run over the same chunks and bitmaps on another stream at the same
 * time.  Overlapping output ranges are the caller's business.
 *
 * A read is INVALID -- both of its words = UINT32_MAX, nothing hashed, nothing
 * written -- when its off or len is misaligned, when it runs past the pool,
 * when d_out_off[i] is not 4-byte aligned or d_out_off[i] + len > out_bytes,
 * or, for a read with an origin, when d_origin_off[i] is not 4-byte aligned or
 * d_origin_off[i] + len > origin_bytes (a read with CC_NO_ORIGIN never looks
 * at the origin buffer, whatever its size).  Nothing is ever written outside
 * [d_out, d_out + out_bytes).  len == 0 is valid: it touches nothing and
 * leaves its words alone.
 *
 * Checked before a device is needed (CC_EINVAL): cc_read_snap_dev's checks on
 * page_bytes, pool_bytes, d_pool, d_reads, d_page_crcs, d_bad_per_read,
 * d_bad_total and n_reads; d_out and d_out_off non-NULL and d_out 4-byte
 * aligned (there is no verify-only mode: cc_verify_reads_dev and
 * cc_read_snap_dev cover it); both unwritten counters non-NULL; clone, its
 * d_clone_slot and its d_bitmap non-NULL, chunk_bytes a multiple of page_bytes
 * that divides pool_bytes; d_origin non-NULL with a NULL d_origin_off, or not
 * 4-byte aligned.  n_reads == 0 is CC_OK.  No GPU: CC_ENODEV, never a CPU
 * fallback.
 *
 * ONE launch on cc_read_snap_dev's schedule and scratch; a batch of <= 64
 * reads on a pool of < 2^26 pages takes one launch with no scratch at all.
 * The unwritten pages of one read that fall to one wave are counted with one
 * atomic. */
#define CC_NO_ORIGIN 0xFFFFFFFFFFFFFFFFull
int cc_read_merge_dev(const void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const cc_range* d_reads,
                      uint64_t n_reads, const uint32_t* d_page_crcs, const cc_clone* clone, const void* d_origin,
                      const uint64_t* d_origin_off, uint64_t origin_bytes, void* d_out, const uint64_t* d_out_off,
                      uint64_t out_bytes, uint32_t* d_bad_per_read, uint64_t* d_bad_total,
                      uint32_t* d_unwritten_per_read, uint64_t* d_unwritten_total, void* stream);

/* Page repair: a peer's copy of a page enters the pool ONLY if it hashes to the
 * CRC on record.  The reference detects and stops: ScanManager::CompareMap puts
 * the failed maps into failedScanMaps_ (scan_manager.cpp:397) and the heartbeat
 * reports them (heartbeat.cpp:158); the integrity calls here name the bad page
 * (cc_page_verify_list_dev, cc_integrity_check).  This call closes the loop for
 * two situations.  SCRUB REPAIR: a page's bytes no longer match
 * d_page_crcs[p]; a peer's copy is fetched and accepted only when it hashes to
 * the stored CRC (d_expect == NULL).  REPLICA RESYNC: a follower's CRC table
 * differs from the authority's (the leader's, or the majority's) in some pages;
 * those pages are fetched from the authority, each is accepted only when it
 * hashes to the AUTHORITY's CRC, and the local table word is brought to that
 * value (d_expect = the authority's table).
 *
 * d_reqs[0..n) is an ORDERED batch of cc_update entries: entry i offers
 * d_src + src_i + (page start - dst_i) as the candidate for every pool page in
 * [dst_i, dst_i + len_i).  A pool page named by several valid entries is
 * handled by the LOWEST-indexed one; every other (entry, page) pair is
 * SHADOWED: it moves no bytes and hashes nothing.  (A second peer for a page
 * that failed is tried by sending the page again in a later call.)
 *
 * For the handling entry, with e = d_expect ? d_expect[p] : d_page_crcs[p] and
 * the pool as it stood BEFORE the call (only the handler reads or writes the
 * page and its CRC word):
 *   CLEAN     the live page hashes to e.  No pool byte is written; with
 *             d_expect, d_page_crcs[p] becomes e (a stale table word is mended).
 *   REPAIRED  otherwise, when the candidate hashes to e: the candidate's bytes
 *             are stored to the pool page and d_page_crcs[p] = e.
 *   FAILED    neither hashes to e: neither the page nor its CRC word is written.
 * So afterwards every clean or repaired page hashes to e and d_page_crcs[p] ==
 * e, and a failed or shadowed-only page is bit for bit what it was.  The pool,
 * the table, the counts and the claim table do not depend on the schedule.
 *
 * d_per_entry[i] gets += 1 in the word of its class for each of entry i's
 * pages (the caller zeroes it): for a valid entry the four words sum to
 * len_i / page_bytes, and for an entry of one page they are a status.
 * d_totals, when non-NULL, gets += the four sums in the struct's order.
 *
 * An entry is INVALID -- all four of its words = UINT32_MAX, nothing claimed,
 * hashed or written -- when dst or len is not a multiple of page_bytes, when
 * it runs past the pool (dst >= pool_bytes or len > pool_bytes - dst), when src
 * is not 4-byte aligned or when src + len > src_bytes.  len == 0 is valid: it
 * touches nothing and leaves its words alone.  d_src must not alias d_pool.
 *
 * Checked before a device is needed (CC_EINVAL): page_bytes = 256 * 2^k
 * (k = 0..5); pool_bytes whole pages; d_pool and d_src 4-byte aligned; d_pool,
 * d_src, d_reqs, d_page_crcs, d_claim and d_per_entry non-NULL; n < 2^31 (entry
 * indices live in d_claim, all-ones reserved).  n == 0 is CC_OK.  No GPU:
 * CC_ENODEV, never a CPU fallback.
 *
 * d_claim is the call's scratch, one word per POOL PAGE, kept by the caller:
 * all 0xFFFFFFFF before the first call, and every call that completes leaves
 * it so.  Two launches on `stream`, as cc_paste_dev.  CLAIM: one lane per
 * (valid entry, page) does atomicMin(d_claim[p], i); it moves no page traffic
 * and also marks the invalid entries.  REPAIR: every (entry, page) pair is one
 * slot on verify-on-read's schedule (the slots split evenly over the device,
 * the last 1/16 dynamically, using the stream's range scratch the engine keeps:
 * no caller work buffer); the slot that finds its own index in d_claim[p] loads
 * and hashes the live page; only when that misses e does it load and hash the
 * candidate, and store it when it hits; it counts and puts 0xFFFFFFFF back.  A
 * shadowed slot reads either the handler's index or all-ones, never its own, so
 * no third launch is needed; shadowed slots are counted a run at a time.  The
 * caller must not run another call that writes the same pages, table words or
 * claim words on another stream at the same time. */
typedef struct cc_repair_counts {
    uint32_t clean, repaired, failed, shadowed;
} cc_repair_counts;
int cc_repair_dev(void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, const void* d_src, uint64_t src_bytes,
                  const cc_update* d_reqs, uint64_t n, uint32_t* d_page_crcs, const uint32_t* d_expect,
                  uint32_t* d_claim, cc_repair_counts* d_per_entry, uint64_t* d_totals, void* stream);

/* Scrub: the bulk integrity pass over a device pool AS THE DATASTORE SEES IT.
 * cc_page_verify_list_dev hashes every pool page against d_page_crcs; a pool
 * with clone chunks has pages that were never written (no meaningful bytes or
 * CRC word: the datastore refuses to read them, PageNerverWrittenError,
 * chunkserver_chunkfile.cpp:510-526), and a pool with open snapshots has pages
 * in its snapshot slots that no bulk pass ever looks at.  This call checks the
 * pages that EXIST, each against the table that describes it, and counts the
 * rest.  It answers the ScanManager's pass (scan_manager.cpp:210-296) for a
 * device-resident pool, snapshot copies included.
 *
 * Geometry: ppc = chunk_bytes / page_bytes; pool page p is chunk c = p / ppc,
 * page q = p % ppc.
 *
 * LIVE pass, over every pool page p.  Let cs = clone ? d_clone_slot[c] :
 * CC_NOT_CLONE.  If cs < clone->n_slots and bit q of slot cs is clear the page
 * was NEVER WRITTEN: neither the page nor d_page_crcs[p] is read, unwritten
 * += 1.  Otherwise the page is hashed whole against d_page_crcs[p]:
 * live_checked += 1, and on a mismatch live_bad += 1,
 * d_bad_per_chunk[c].live_bad += 1 and the list gets p.  A live page whose
 * snapshot bit is set is still a live page and is checked: this call audits
 * storage, it is not cc_read_snap_dev's snapshot view.
 *
 * SNAP pass, only with cow.  For every pool page p let s = d_snap_slot[c]; when
 * s < cow->n_slots and bit q of slot s is set, the bytes at d_snap +
 * (s * ppc + q) * page_bytes are hashed against d_snap_crcs[s * ppc + q]:
 * snap_checked += 1, and on a mismatch snap_bad += 1,
 * d_bad_per_chunk[c].snap_bad += 1 and the list gets CC_SCRUB_SNAP | p.  Nothing
 * else of a slot is read: not a page whose bit is clear, not a slot that no
 * chunk names, not a slot value >= n_slots.  Bits at positions >= ppc of a
 * slot's last bitmap word are ignored, in both structs.  Two chunks naming one
 * slot (a caller error in the datastore) are each scrubbed on their own terms.
 *
 * List: every mismatch does k = listed++ (the value before the call counts: a
 * second call on the same counters continues the cursor) and stores its entry
 * at d_bad_list[k] when k < max_list.  The entries come in no particular order,
 * as cc_page_verify_list_dev's; listed may exceed max_list, and nothing is
 * written at or past d_bad_list + max_list.  d_bad_list may be NULL only when
 * max_list == 0.  When the mismatches fit, the SET of entries is deterministic;
 * the six counts and the per-chunk words always are.  All counts are += (the
 * caller zeroes them).
 *
 * Read-only: the call writes d_counts, d_bad_list and d_bad_per_chunk and
 * nothing else -- not the pool, a CRC table, a bitmap, d_claim, d_copied,
 * d_stale or d_pasted; d_claim and the counters of both structs may be NULL.
 * The caller must not run a write log, a paste or a repair over the same pool
 * on another stream at the same time.
 *
 * Checked before a device is needed (CC_EINVAL): page_bytes = 256 * 2^k
 * (k = 0..5); chunk_bytes a non-zero multiple of page_bytes that divides
 * pool_bytes; pool_bytes / page_bytes < 2^32; d_pool, d_page_crcs and d_counts
 * non-NULL, d_pool 4-byte aligned; a non-zero max_list with a NULL list; with
 * cow: its chunk_bytes == chunk_bytes, its slot, snap, CRC and bitmap pointers
 * non-NULL, d_snap 4-byte aligned; with clone: its chunk_bytes == chunk_bytes,
 * d_clone_slot and d_bitmap non-NULL.  pool_bytes == 0 is CC_OK.  No GPU:
 * CC_ENODEV, never a CPU fallback.
 *
 * cow == NULL && clone == NULL IS cc_page_verify_list_dev: the page kernel, the
 * same launch, its rate (the kernel's list cursor is `listed`, its mismatch
 * path also counts the chunk's word; two one-thread launches around it fill
 * live_checked and live_bad).  Otherwise ONE launch on verify-on-read's
 * schedule with groups of 64 domain indices (the live pages, then their
 * snapshot copies) in the place of reads: the kernel counts the pages that
 * exist per tile of groups from the bitmap words, every wave hashes an equal
 * share of them, the last 1/16 handed out dynamically, so the balance does not
 * depend on where the sparse parts lie and a page that does not exist moves no
 * bytes.  Uses the stream's range scratch the engine keeps: no caller work
 * buffer. */
#define CC_SCRUB_SNAP (1ull << 63) /* list entry: the SNAPSHOT copy of pool page (entry & ~CC_SCRUB_SNAP) */
typedef struct cc_scrub_counts {   /* device memory, all += ; the caller zeroes */
    uint64_t live_checked, live_bad, snap_checked, snap_bad, unwritten, listed;
} cc_scrub_counts;
typedef struct cc_scrub_chunk {
    uint32_t live_bad, snap_bad;
} cc_scrub_chunk;
int cc_scrub_dev(const void* d_pool, uint64_t pool_bytes, uint32_t page_bytes, uint32_t chunk_bytes,
                 const uint32_t* d_page_crcs, const cc_cow* cow, const cc_clone* clone, cc_scrub_counts* d_counts,
                 uint64_t* d_bad_list, uint64_t max_list,
                 cc_scrub_chunk* d_bad_per_chunk /* [pool_bytes / chunk_bytes], += , or NULL */, void* stream);

/* One chunk file as the datastore holds it: metapage + data
 * (file = metapage || data, chunkserver_chunkfile.cpp:497-536). */
typedef struct cc_chunk_src {
    const void* meta; /* meta_bytes of host memory */
    const void* data; /* chunk_bytes of host memory */
} cc_chunk_src;

/* Streaming scan of host-resident chunk files (BASELINE config 4; the scan
 * hasher ScanChunkRequest::OnApply, op_request.cpp:769-820, for every scan op
 * of every chunk in ScanManager::ScanJobProcess order, scan_manager.cpp:250-283).
 * Per chunk c:
 *   h_meta_crcs[c]                          = CRC32(metapage)          (the readMetaPage op)
 *   h_slice_crcs[c*S + k], S = chunk/slice  = CRC32(data[k*slice, +slice))
 *   h_file_crcs[c]                          = CRC32(metapage || data)  (chunk-file CRC for
 *                                             the copyset chain, copyset_node.cpp:964)
 * Pipelined over two pinned staging slots and two HIP streams: the H2D copy of
 * batch i+1 overlaps the hashing of batch i.  Pinned (hipHostMalloc'ed or
 * registered) sources are DMA'd directly; pageable ones are staged by memcpy
 * (decided per buffer).  Any output pointer may be NULL.  Every chunk pointer
 * is checked before any work starts; on an error no batch of the call is left
 * in flight.  Blocking; thread-safe (per-device lock). */
int cc_scan_host(const cc_chunk_src* chunks, uint64_t n_chunks, uint32_t chunk_bytes,
                 uint32_t meta_bytes, uint32_t page_bytes, uint32_t slice_bytes,
                 uint32_t* h_meta_crcs, uint32_t* h_slice_crcs, uint32_t* h_file_crcs);

/* Per-copyset digest of a streamed scan (BASELINE config 4: "per-copyset
 * digest", CopysetNode::GetHash, copyset_node.cpp:925-975). */
typedef struct cc_scan_digest {
    const uint64_t* h_after_bytes; /* [n_chunks] bytes of the chunk's copyset that sort after its file */
    const uint32_t* h_group;       /* [n_chunks] copyset index of the chunk, < n_groups */
    uint64_t n_groups;
    uint32_t* h_digest;            /* [n_groups] out: XOR_c shift(file CRC of c, after bytes of c) over the
                                      call's chunks -- the copyset's GetHash value when all its files are in
                                      the call, else this call's partial (XOR partials of disjoint calls) */
} cc_scan_digest;

/* cc_scan_host plus the per-copyset digest, computed on the device by the
 * fused epilogue of every batch (no host pass over the file CRCs).  The chunk
 * list may mix pinned and pageable buffers.  dg NULL = cc_scan_host. */
int cc_scan_host_digest(const cc_chunk_src* chunks, uint64_t n_chunks, uint32_t chunk_bytes,
                        uint32_t meta_bytes, uint32_t page_bytes, uint32_t slice_bytes,
                        uint32_t* h_meta_crcs, uint32_t* h_slice_crcs, uint32_t* h_file_crcs,
                        const cc_scan_digest* dg);

/* Per-file outcome of cc_scan_files. */
typedef struct cc_file_result {
    int32_t status;    /* 0 ok; -errno from open/fstat/pread; CC_EFORMAT: size != meta+chunk
                          (CSChunkFile::Open's FileFormatError, chunkserver_chunkfile.cpp:233-238) */
    uint32_t meta_crc; /* CRC32(metapage) */
    uint32_t file_crc; /* CRC32(metapage || data) == CopysetNode::GetHash's per-file chain step */
    uint32_t reserved;
} cc_file_result;

/* Native datastore read path + scan: open/fstat/pread every chunk FILE (the
 * whole-file read of CopysetNode::GetHash, copyset_node.cpp:942-962, and the
 * metapage + data reads of the scan ops, chunkserver_chunkfile.cpp:497-548)
 * with `io_threads` reader threads (0 = cc_default_io_threads(); the caller is
 * one of them) into pinned staging, overlapping the reads of batch i+1 with the
 * H2D copy + kernels of batch i.  The readers are persistent: created once per
 * device on first use, parked between batches.  Outputs as cc_scan_host (slice
 * CRCs may be NULL); a file whose size is not meta_bytes + chunk_bytes gets
 * CC_EFORMAT, one that cannot be read -errno, and neither gets CRCs (the caller
 * chains such files on the CPU).  Blocking, thread-safe. */
int cc_scan_files(const char* const* paths, uint64_t n_files, uint32_t chunk_bytes, uint32_t meta_bytes,
                  uint32_t page_bytes, uint32_t slice_bytes, uint32_t io_threads, uint32_t* h_slice_crcs,
                  cc_file_result* h_results);
/* The reader count io_threads = 0 selects: half the CPUs this process may use
 * (its affinity mask, capped by the cgroup v2 cpu.max quota), in [2, 8]. */
uint32_t cc_default_io_threads(void);

/* ------------------------------------------------------------------------
 * Full-pool integrity scan sharded over the GPUs of a node (BASELINE config 5,
 * SURVEY §8e).  One process per GPU; each rank scans the chunk-index range it
 * owns with no data-path collective.  The only exchange is the per-copyset
 * digest of CopysetNode::GetHash (copyset_node.cpp:925-975): order-free XOR
 * partials, all-gathered over RCCL (xGMI) and XOR-folded on the device (XOR is
 * not an RCCL reduction op).  Per-chunk work is the scan hasher's
 * (ScanChunkRequest::OnApply, op_request.cpp:769-820, for every op that
 * ScanManager::ScanJobProcess schedules, scan_manager.cpp:210-296).
 * ------------------------------------------------------------------------ */
#define CC_ECOMM (-71) /* an RCCL call failed */
#define CC_COMM_ID_BYTES 128

typedef struct cc_comm cc_comm; /* opaque: an RCCL communicator + gather scratch */

/* Rank 0 creates the id and hands its CC_COMM_ID_BYTES bytes to every rank
 * out of band (the MDS, a TCP store, ...). */
int cc_comm_unique_id(void* id, size_t bytes);
/* Collective: every rank calls it with the same id, on the HIP device it owns
 * (the calling thread's current device).  Returns once all ranks joined, or
 * after `timeout_ms` (0 = $CC_COMM_INIT_TIMEOUT_MS, else 120 s) with
 * CC_ETIMEDOUT and the half-built communicator aborted: a rank whose peers
 * never arrive (one failed before reaching RCCL) is never blocked forever.
 * The communicator is RCCL non-blocking (ncclConfig_t.blocking = 0); every
 * call below waits for its own enqueue to settle.  The reference's exchange
 * (FollowScanMap, chunk_closure.cpp:82-104) is likewise bounded (retry x
 * timeout, scan_manager.cpp:285-289).  Ranks that disagree on whether their
 * init succeeded must all fall back together (bench.py / pool.agreed_comm
 * reduce a success flag before the first collective). */
int cc_comm_init_timeout(cc_comm** comm, int nranks, int rank, const void* id, size_t bytes, uint32_t timeout_ms);
int cc_comm_init(cc_comm** comm, int nranks, int rank, const void* id, size_t bytes); /* default timeout */
/* destroy: finalize (flush this rank's work) + free.  abort: free without
 * waiting for the peers (a rank leaving a communicator its peers gave up on). */
int cc_comm_destroy(cc_comm* comm);
int cc_comm_abort(cc_comm* comm);
int cc_comm_size(const cc_comm* comm);
int cc_comm_rank(const cc_comm* comm);

/* d_digest[0..n) <- XOR over all ranks of their d_digest[0..n) (in place;
 * collective, stream-ordered, enqueue only): ncclAllGather of the partials,
 * then cc_digest_fold_dev.  Calls on one communicator must be issued in the
 * same order on every rank, from one stream at a time. */
int cc_digest_allreduce_dev(cc_comm* comm, uint32_t* d_digest, uint64_t n, void* stream);

/* Bounded wait for everything enqueued on `stream` so far -- the digest
 * exchanges of cc_pool_scan_dev / cc_digest_allreduce_dev included -- with the
 * communicator's health polled meanwhile (ncclCommGetAsyncError).  CC_OK once
 * the stream has reached this point; if a peer stopped participating after
 * init the collective never completes: after `timeout_ms` (0 =
 * $CC_COMM_WAIT_TIMEOUT_MS, else 60 s) the communicator is aborted (its
 * kernels released, the stream drains) and CC_ETIMEDOUT is returned; an RCCL
 * async error aborts it at once with CC_ECOMM.  An aborted communicator
 * answers CC_ECOMM to every later exchange; free it with cc_comm_abort.  The
 * reference bounds its exchange the same way (FollowScanMap retry x timeout,
 * chunk_closure.cpp:82-104).  Blocking (sleep-polls, never spins a core). */
int cc_comm_wait(cc_comm* comm, void* stream, uint32_t timeout_ms);

/* One rank's shard of the pool and the outputs of one scan pass over it. */
typedef struct cc_pool_shard {
    const void* d_data;       /* n_chunks x chunk_bytes, chunk c's data at c*chunk_bytes */
    const void* d_meta;       /* n_chunks x meta_bytes metapages (file = metapage || data) */
    uint64_t n_chunks;
    uint32_t chunk_bytes;     /* 16 MiB (conf/chunkserver.conf chunksize) */
    uint32_t meta_bytes;      /* 4 KiB metapage */
    uint32_t page_bytes;      /* 4 KiB */
    uint32_t slice_bytes;     /* 4 MiB scan slice (copyset.scan_size_byte) */
    const uint32_t* d_after_mult; /* [n_chunks] x^(8*bytes after the file in its copyset chain), cc_xpow8_dev */
    const uint32_t* d_group;      /* [n_chunks] copyset index of each file */
    uint64_t n_groups;            /* copysets in the WHOLE pool (same on every rank) */
    /* outputs (device) */
    uint32_t* d_page_crcs;    /* [n_chunks * chunk_bytes/page_bytes] */
    uint32_t* d_meta_crcs;    /* [n_chunks]  ScanMap.crc of the readMetaPage op */
    uint32_t* d_slice_crcs;   /* [n_chunks * chunk_bytes/slice_bytes]  ScanMap.crc of the data ops */
    uint32_t* d_file_crcs;    /* [n_chunks]  CRC32(metapage || data), may be NULL */
    uint32_t* d_digest;       /* [n_groups]  full per-copyset digests after the call */
    /* optional hipEvent_t recorded on `stream` right before / after the page
     * kernel over the data (NULL = none): lets a bench time the hot kernel
     * inside the one call */
    void* ev_pages_begin;
    void* ev_pages_end;
    /* optional hipEvent_t recorded on `stream` right before the digest
     * exchange's all-gather and right after its XOR fold (comm non-NULL only;
     * NULL = none): the exchange's own share of a scan step at N > 1 */
    void* ev_exchange_begin;
    void* ev_exchange_end;
} cc_pool_shard;

/* One integrity scan pass over the shard: page CRCs of every data page and
 * metapage, slice CRCs (ScanMap.crc), file CRCs, digest partials, then (comm
 * non-NULL) the digest all-reduce, after which d_digest[g] on every rank is
 * copyset g's CopysetNode::GetHash value over the WHOLE pool
 * (V(f1||..||fn) = XOR_i shift(V(fi), bytes after fi): exact, no constant).
 * Enqueue only; comm NULL = single-rank pool.  Needs chunk_bytes = 256*q
 * pages with slice_bytes = q*2^j pages (the fused epilogue's geometry). */
int cc_pool_scan_dev(const cc_pool_shard* shard, cc_comm* comm, void* stream);

/* ------------------------------------------------------------------------
 * Per-page CRC persistence -- the table verify-on-read and
 * the integrity jobs of proto/integrity.proto (IntegrityService, :55-61;
 * declared and compiled in the reference, never implemented) check against.
 * The reference keeps no data CRC anywhere: the metapage holds a CRC of its own
 * header only (chunkserver_chunkfile.cpp:64-130), so the table is a NEW sidecar
 * file per chunk, kept OUTSIDE the copyset data directory (CopysetNode::GetHash
 * chains every file listed there, copyset_node.cpp:931-970).  It records the
 * chunk's sn (metapage) and the chunk file's mtime and size when it was
 * written: a table whose chunk changed since is STALE and never condemns data.
 * (mtime comes from the kernel's coarse clock: a write path that changes a
 * chunk must store its table -- cc_pcrc_store after the write, e.g. from the
 * CRCs cc_apply_log_delta_dev keeps current -- staleness is the safety net.)
 * ------------------------------------------------------------------------ */
#define CC_PCRC_HEADER_BYTES 64

typedef struct cc_pcrc_header {
    uint32_t page_bytes;
    uint32_t n_pages;
    uint64_t chunk_sn;      /* metapage sn when the table was written */
    int64_t data_mtime_ns;  /* the chunk file's st_mtim then */
    uint64_t data_size;     /* the chunk file's size then */
    int64_t stamp_ns;       /* CLOCK_REALTIME when the CRCs' bytes were known current: a check's
                               time just before it read the chunk; cc_pcrc_store_expect's
                               expect->stamp_ns (or the mtime); cc_pcrc_store's call time */
} cc_pcrc_header;

/* Racy tables (git's "racily clean" index entries).  File mtimes come from a
 * coarse clock: a write landing in the same clock tick as data_mtime_ns leaves
 * the identity unchanged.  A table is trusted to condemn data only when that
 * cannot have happened after its CRCs were taken, i.e. when
 *     data_mtime_ns + tick < stamp_ns      (tick = clock_getres(CLOCK_REALTIME_COARSE);
 *                                           1 s -- 2 s on an even second -- when the mtime
 *                                           has no sub-second part: a filesystem keeping
 *                                           whole seconds, or FAT's 2 s)
 * Otherwise it is RACY: its pages are still compared, a match re-stamps it
 * (the table is rewritten with a later stamp), and a mismatch is reported as
 * STALE -- refreshed by policy -- never as bad pages. */
int cc_pcrc_is_racy(const cc_pcrc_header* h);

/* In-memory codec.  decode: CC_ECORRUPT for a bad magic / version / header CRC
 * / table CRC / length; page_crcs may be NULL (header only). */
uint64_t cc_pcrc_encoded_bytes(uint32_t n_pages);
int cc_pcrc_encode(const cc_pcrc_header* h, const uint32_t* page_crcs, void* out, uint64_t out_bytes);
int cc_pcrc_decode(const void* buf, uint64_t bytes, cc_pcrc_header* h, uint32_t* page_crcs, uint32_t max_pages);

/* sn of a chunk metapage, after ChunkFileMetaPage::decode's checks
 * (chunkserver_chunkfile.cpp:90-130: header CRC, version 1 or 2), bounds-checked;
 * CC_ECORRUPT otherwise. */
int cc_chunk_meta_sn(const void* metapage, uint32_t bytes, uint64_t* sn);

/* The snapshot file's metapage, byte for byte SnapshotMetaPage::encode/decode
 * (datastore/chunkserver_snapshot.cpp:30-82): version u8 = FORMAT_VERSION (1) |
 * damaged u8 | sn u64 | bits u32 | bitmap (bits + 7) / 8 bytes | CRC32C of
 * everything before it, u32 | the rest of the page zero.  `bitmap` is a slot of
 * cc_cow::d_snap_bitmap copied to the host, unchanged (bit q of the slot = bit
 * q % 8 of byte q / 8).  Bounds-checked: 14 + (bits + 7) / 8 + 4 must fit the
 * page -- CC_EINVAL on encode, CC_ECORRUPT on decode, as are a bad CRC or
 * version.  decode: sn / damaged / bits / bitmap may each be NULL; a non-NULL
 * bitmap of fewer than (bits + 7) / 8 bytes is CC_EINVAL. */
int cc_snap_meta_encode(uint64_t sn, int damaged, uint32_t bits, const void* bitmap, void* out, uint32_t out_bytes);
int cc_snap_meta_decode(const void* buf, uint32_t bytes, uint64_t* sn, int* damaged, uint32_t* bits,
                        void* bitmap, uint32_t bitmap_cap_bytes);

/* Write the table of chunk file `chunk_path` (metapage of meta_bytes, then
 * n_pages data pages) to `table_path`, atomically (temp file + fsync + rename),
 * recording the chunk's current sn, mtime and size.  Call it after the data
 * write it describes (the write path's CSChunkFile::Write, chunkserver_chunkfile.cpp:287-427),
 * under the chunk's write lock (CSChunkFile::rwLock_) so no other write lands
 * between the two.  CC_EFORMAT when the file's size is not meta_bytes +
 * n_pages x page_bytes (FileFormatError). */
int cc_pcrc_store(const char* chunk_path, uint32_t meta_bytes, const char* table_path, const uint32_t* page_crcs,
                  uint32_t n_pages, uint32_t page_bytes);
/* The same, but only if the chunk's identity is still `expect` (its sn,
 * data_mtime_ns and data_size; the caller stats the file right after its
 * pwrite): CC_ESTALE and nothing written otherwise, so a store that runs after
 * a LATER write cannot pair the newer identity with the older CRCs.  The table
 * is stamped with expect->stamp_ns -- the caller's CLOCK_REALTIME taken BEFORE
 * its pwrite -- or, when that is 0, with data_mtime_ns (racy until a check
 * re-stamps it); never with the store's own clock, which could clear a table
 * whose chunk took a second same-size write within the mtime's tick. */
int cc_pcrc_store_expect(const char* chunk_path, uint32_t meta_bytes, const char* table_path,
                         const uint32_t* page_crcs, uint32_t n_pages, uint32_t page_bytes,
                         const cc_pcrc_header* expect);
/* Read + decode a table file (-errno if it cannot be read, -ENOENT if absent).
 * With page_crcs, a file larger than a table of max_pages pages is CC_ECORRUPT
 * before anything is allocated; without, only the 64-byte header is read. */
int cc_pcrc_load(const char* table_path, cc_pcrc_header* h, uint32_t* page_crcs, uint32_t max_pages);

/* Table state of one chunk after a check. */
#define CC_TABLE_OK 0        /* table describes the chunk; bad_pages counted against it */
#define CC_TABLE_CREATED 1   /* no table: one was written from the current bytes */
#define CC_TABLE_CORRUPT 2   /* table unreadable (CRC / geometry): reported, not used */
#define CC_TABLE_STALE 3     /* chunk changed since the table was written: not used */
#define CC_TABLE_REFRESHED 4 /* stale, and rewritten from the current bytes */
#define CC_TABLE_MISSING 5   /* no table, none written */
#define CC_TABLE_REBUILT 6   /* corrupt, and rewritten from the current bytes */

typedef struct cc_integrity_opts {
    uint32_t chunk_bytes;    /* 16 MiB */
    uint32_t meta_bytes;     /* 4 KiB */
    uint32_t page_bytes;     /* 4 KiB */
    uint32_t io_threads;     /* readers of cc_scan_files (0 = cc_default_io_threads()) */
    uint32_t create_missing; /* write a table for a chunk that has none */
    uint32_t refresh_stale;  /* rewrite stale / corrupt tables from the current bytes */
} cc_integrity_opts;

typedef struct cc_integrity_result {
    int32_t status;       /* 0; -errno; CC_EFORMAT (file size != metapage + chunk, checked first as
                             CSChunkFile::Open does); CC_ECORRUPT (metapage header) */
    uint32_t table_state; /* CC_TABLE_* */
    uint32_t n_pages;
    uint32_t bad_pages;   /* pages whose bytes no longer match the (valid, current) table */
    int64_t first_bad;    /* -1: none */
} cc_integrity_result;

/* The integrity check of a batch of chunk files (the work of one
 * IntegrityService job step): every data page rehashed on the device (native
 * pread into pinned staging, cc_scan_files) and compared with the chunk's
 * table; a file that changes while it is read counts as stale.  Bad pages are
 * listed as (file index << 32 | page) in bad_list (the first bad_cap of them;
 * *n_bad = all).  Blocking, thread-safe. */
int cc_integrity_check(const char* const* chunk_paths, const char* const* table_paths, uint64_t n,
                       const cc_integrity_opts* opts, cc_integrity_result* res, uint64_t* bad_list, uint64_t bad_cap,
                       uint64_t* n_bad);

/* ------------------------------------------------------------------------
 * Diagnostics (new; no reference counterpart)
 * ------------------------------------------------------------------------ */
/* Copy the 163840-byte LDS image the page kernel loads into every CU (G tables
 * + per-lane final maps, DESIGN.md "LDS image") so host tests can replay the
 * kernel's arithmetic on the CPU.  Needs no GPU. */
int cc_lds_image(void* out, size_t bytes);

/* Read-only HBM probe: streams `bytes` (multiple of 4096, 16-byte aligned) from
 * d_buf with the page kernel's access style (nontemporal, grid-stride,
 * persistent blocks) and XOR-reduces into d_sink[0 .. 2*CUs*16).  What a pure
 * read achieves on THIS device: bench.py reports the page kernel against it
 * beside the 8 TB/s spec.  Enqueue only. */
int cc_hbm_read_probe_dev(const void* d_buf, uint64_t bytes, uint32_t* d_sink, void* stream);

/* Diagnostic (no reference counterpart): the page kernel over n_pages 4 KiB
 * pages with its CRC arithmetic replaced by a rotate-XOR -- the same schedule
 * (tiles, prefetch ring, dynamic tail), loads and 4-byte-per-page stores into
 * d_out, so its time is the ceiling cc_page_crc_dev is held to on this device.
 * d_out receives meaningless words.  Enqueue only. */
int cc_page_load_probe_dev(const void* d_pages, uint64_t n_pages, uint32_t* d_out, void* stream);

/* Diagnostic (no reference counterpart): the write log's page traffic alone,
 * the ceiling cc_apply_log_dev is held to on its access pattern.  One
 * descriptor per touched 4 KiB page of a log (host-built, e.g.
 * curve_amd.crc.log_probe_descs): the rows read from the source (covered by the
 * page's only piece; src_off = the source byte of page byte 0, mod 2^64) -- the
 * others from the page -- and the rows stored back.  Same grid and occupancy
 * as the write log's page pass, no table, no CRC.  It stores back the bytes it
 * loaded: run right after the log it describes was applied, it changes no
 * byte.  d_out[i] = an XOR of page i's words.  A descriptor naming a page past
 * the pool touches nothing (page 0 read, no store); source offsets are the
 * caller's to keep inside d_src.  Enqueue only. */
typedef struct cc_log_probe_desc {
    uint64_t page;
    uint64_t src_off;
    uint32_t covered_rows;
    uint32_t dirty_rows;
} cc_log_probe_desc;
int cc_apply_log_probe_dev(void* d_pool, uint64_t pool_bytes, const void* d_src, const cc_log_probe_desc* d_desc,
                           uint64_t n, uint32_t* d_out, void* stream);

/* Diagnostic (no reference counterpart): the read traffic of a list of 4 KiB
 * pages alone -- d_pages[i] = a page index of the pool, in list order (for a
 * batch of reads: each read's pages in turn) -- the ceiling cc_verify_reads_dev
 * is held to on its access pattern.  Verify-on-read's grid, occupancy and
 * schedule (a workgroup of 8 waves per CU, LDS unused; each wave an equal
 * contiguous share of the first 15/16 of the list, the rest in 32-page chunks
 * to whichever waves finish first), two pages in flight, no CRC, no stored-CRC
 * loads.  d_out[i] = an
 * XOR of page i's words.  An index past the pool reads page 0 instead (never
 * outside the pool).  Enqueue only. */
int cc_page_list_probe_dev(const void* d_pool, uint64_t pool_bytes, const uint64_t* d_pages, uint64_t n,
                           uint32_t* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CURVE_CRC_H_ */
