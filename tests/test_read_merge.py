"""Clone reads on the device (cc_read_merge_dev): everything that needs no GPU.

The numpy model of the call (read_merge_model, page by page) lives here and is
checked against a request-by-request restatement of CloneCore::ReadThenMerge
(clone_core.cpp:352-416: Divide() the request's blocks into copied and
uncopied ranges, ReadChunk per copied range, cloneData->copy_to per uncopied
one); clone_read's composition (check -> fetch -> merge -> paste) is checked,
with the three device calls replaced by their models, against a sequential
replay of HandleReadRequest -> ReadThenMerge -> Paste.  The GPU tests
(test_read_merge_gpu.py) lean on the models, never on the code under test.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_clone import NOT_CLONE, U32_MAX, bit, check_reads_model, paste_model, replay_paste, set_bit
from test_snap_read import bit_runs, cut_per_chunk, packed_offsets

NO_ORIGIN = 0xFFFFFFFFFFFFFFFF
OUT_SENT = 0x3C   # what the output buffers hold before a call


# --------------------------------------------------------------------------- model
def merge_valid(off, ln, oo, go, pool_bytes, out_bytes, origin_bytes, pb):
    """cc_read_merge_dev's contract per read (include/curve_crc.h).  go None: the read has no origin."""
    if ln == 0:
        return True
    if off % pb or ln % pb:
        return False
    if off >= pool_bytes or ln > pool_bytes - off:
        return False
    if oo % 4 or oo > out_bytes or ln > out_bytes - oo:
        return False
    if go is not None and (go % 4 or go > origin_bytes or ln > origin_bytes - go):
        return False
    return True


def origin_of(origin, origin_off, i):
    """Read i's origin offset, or None when it has none (d_origin NULL or CC_NO_ORIGIN)."""
    if origin is None or int(origin_off[i]) == NO_ORIGIN:
        return None
    return int(origin_off[i])


def read_merge_model(pool, page_crcs, slot, n_slots, bm, reads, origin, origin_off, out_off, out, pb, cb, crc_fn=None):
    """One cc_read_merge_dev call on host arrays, page by page; `out` (the
    buffer as it was before the call) is filled in place.  origin None:
    d_origin == NULL.  crc_fn None: nothing is hashed (bytes only).  Returns
    (bad_per_read, bad_total, unwritten_per_read, unwritten_total)."""
    ppc = cb // pb
    n = len(reads)
    bad, unw = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    bad_total = unw_total = 0
    mism = {}
    for i, (off, ln) in enumerate(reads):
        off, ln, oo = int(off), int(ln), int(out_off[i])
        go = origin_of(origin, origin_off, i)
        if not merge_valid(off, ln, oo, go, pool.size, out.size, 0 if origin is None else origin.size, pb):
            bad[i] = unw[i] = U32_MAX
            continue
        for p in range(off // pb, (off + ln) // pb):
            c, q = divmod(p, ppc)
            s = int(slot[c])
            at = oo + p * pb - off
            if s < n_slots and not bit(bm, s, q):          # never written
                unw[i] += 1
                unw_total += 1
                if go is not None:
                    out[at:at + pb] = origin[go + p * pb - off:go + (p + 1) * pb - off]
                continue
            data = pool[p * pb:(p + 1) * pb]
            if crc_fn is not None:
                if p not in mism:
                    mism[p] = crc_fn(data) != int(page_crcs[p])
                if mism[p]:
                    bad[i] += 1
                    bad_total += 1
            out[at:at + pb] = data
    return bad, bad_total, unw, unw_total


def replay_read_then_merge(pool, slot, n_slots, bm, chunk, off, ln, clone_data, pb, cb):
    """CloneCore::ReadThenMerge for one request on chunk `chunk` (offset and
    length relative to the chunk, block-aligned; clone_data = the downloaded
    [offset, offset + length) of the origin): Divide(beginIndex, endIndex,
    &uncopied, &copied) on a clone chunk, else one copied range; loop 1 reads
    every copied range from the chunk, loop 2 copies every uncopied range out of
    clone_data, each at chunkData + (range start - offset).  Returns chunkData."""
    assert off % pb == 0 and ln % pb == 0 and ln > 0 and off + ln <= cb   # CloneReadByLocalInfo, :145-157
    buf = np.full(ln, OUT_SENT, np.uint8)
    begin, end = off // pb, (off + ln - 1) // pb
    s = int(slot[chunk])
    if s < n_slots:                                        # chunkInfo.isClone
        uncopied, copied = bit_runs(bm[s], begin, end)
    else:
        uncopied, copied = [], [(begin, end)]
    for b, e in copied:                                    # 1. Read
        ro, rs = b * pb, (e - b + 1) * pb
        buf[ro - off:ro - off + rs] = pool[chunk * cb + ro:chunk * cb + ro + rs]
    for b, e in uncopied:                                  # 2. Merge
        ro, rs = b * pb, (e - b + 1) * pb
        buf[ro - off:ro - off + rs] = clone_data[ro - off:ro - off + rs]
    return buf


# --------------------------------------------------------------------------- model against the replay
def geometry(ppc, pb=256, n_slots=3):
    slot = np.array([0, NOT_CLONE, 2, 7, 1, NOT_CLONE], np.uint32)   # 7: out of range for n_slots = 3
    return slot, n_slots, ppc * pb


def bitmaps(kind, n_slots, ppc, rng):
    bm = np.zeros((n_slots, (ppc + 31) // 32), np.uint32)
    for s in range(n_slots):
        for q in range(ppc):
            if {"random": rng.integers(0, 2), "all_set": 1, "all_clear": 0, "alternating": (q + s) & 1}[kind]:
                set_bit(bm, s, q)
    return bm


@pytest.mark.parametrize("kind", ["random", "all_set", "all_clear", "alternating"])
@pytest.mark.parametrize("ppc", [40, 32, 5])
def test_model_equals_request_by_request_read_then_merge(kind, ppc):
    """Reads inside one chunk and reads crossing chunks with different slots
    (clone, not a clone, out of range), pages_per_chunk = 40 with a partial
    last bitmap word, all-set and all-clear bitmaps: the model's bytes are
    ReadThenMerge's, request by request, and nothing else is written."""
    pb = 256
    slot, n_slots, cb = geometry(ppc, pb)
    rng = np.random.default_rng(ppc * 7 + len(kind))
    pool = rng.integers(0, 256, slot.size * cb, dtype=np.uint8)
    bm = bitmaps(kind, n_slots, ppc, rng)
    n_pages = pool.size // pb
    reads = []
    for _ in range(80):                                    # anywhere, crossing chunks
        p0 = int(rng.integers(0, n_pages))
        reads.append((p0 * pb, int(rng.integers(1, min(2 * ppc, n_pages - p0) + 1)) * pb))
    for _ in range(40):                                    # inside one chunk
        c, q0 = int(rng.integers(0, slot.size)), int(rng.integers(0, ppc))
        reads.append(((c * ppc + q0) * pb, int(rng.integers(1, ppc - q0 + 1)) * pb))
    reads.append((0, pool.size))                           # the whole pool in one read
    lens = [ln for _, ln in reads]
    out_off, out_bytes = packed_offsets(lens, gap=8)
    origin_off, origin_bytes = packed_offsets(lens, gap=4)
    origin = rng.integers(0, 256, origin_bytes, dtype=np.uint8)
    out = np.full(out_bytes, OUT_SENT, np.uint8)
    bad, bad_total, unw, unw_total = read_merge_model(pool, None, slot, n_slots, bm, reads, origin, origin_off, out_off,
                                                      out, pb, cb)
    assert bad_total == 0 and not bad.any()
    covered = np.zeros(out_bytes, bool)
    clear = np.zeros(len(reads), np.uint32)
    for i, c, off, ln, at in cut_per_chunk(reads, cb):
        go = int(origin_off[i]) + at
        want = replay_read_then_merge(pool, slot, n_slots, bm, c, off, ln, origin[go:go + ln], pb, cb)
        o = int(out_off[i]) + at
        assert (out[o:o + ln] == want).all(), (i, c, off, ln)
        covered[o:o + ln] = True
        s = int(slot[c])
        if s < n_slots:
            clear[i] += sum(1 - bit(bm, s, q) for q in range(off // pb, (off + ln) // pb))
    assert (out[~covered] == OUT_SENT).all() and covered.sum() == sum(lens)
    assert (unw == clear).all() and unw_total == int(clear.sum())
    if kind == "all_set":
        assert unw_total == 0
    if kind == "all_clear":
        assert unw[-1] == 3 * ppc                          # the three clone chunks, whole
    # for aligned reads the unwritten counts are cc_clone_check_reads_dev's
    chk, chk_total = check_reads_model(reads, pool.size, slot, n_slots, bm, pb, cb)
    assert (chk == unw).all() and chk_total == unw_total


def test_model_cases_by_hand(oracle):
    pb, ppc = 256, 5
    cb = ppc * pb
    slot = np.array([0, NOT_CLONE], np.uint32)
    crc_fn = lambda b: oracle.crc32c(b.tobytes())
    rng = np.random.default_rng(4)
    pool = rng.integers(0, 256, 2 * cb, dtype=np.uint8)
    crcs = oracle.page_crcs(pool, pb)
    origin = rng.integers(0, 256, 8 * pb, dtype=np.uint8)
    bm = np.zeros((1, 1), np.uint32)
    bm[0, 0] = 0b11011                                     # page 2 of chunk 0 never written
    # a read whose only unwritten page has no origin: that page stays at the sentinel and counts 1
    out = np.full(4 * pb, OUT_SENT, np.uint8)
    bad, bt, unw, ut = read_merge_model(pool, crcs, slot, 1, bm, [(pb, 3 * pb)], origin, [NO_ORIGIN], [0], out, pb, cb,
                                        crc_fn)
    assert unw.tolist() == [1] and ut == 1 and bt == 0 and bad.tolist() == [0]
    assert (out[:pb] == pool[pb:2 * pb]).all() and (out[pb:2 * pb] == OUT_SENT).all()
    assert (out[2 * pb:3 * pb] == pool[3 * pb:4 * pb]).all() and (out[3 * pb:] == OUT_SENT).all()
    # ... and the same with d_origin == NULL
    out2 = np.full(4 * pb, OUT_SENT, np.uint8)
    res = read_merge_model(pool, crcs, slot, 1, bm, [(pb, 3 * pb)], None, None, [0], out2, pb, cb, crc_fn)
    assert (out2 == out).all() and res[2].tolist() == [1]
    # a corrupt pool page under a clear bit is neither counted nor delivered
    dirty = pool.copy()
    dirty[2 * pb + 7] ^= 0x40
    out = np.full(4 * pb, OUT_SENT, np.uint8)
    bad, bt, unw, ut = read_merge_model(dirty, crcs, slot, 1, bm, [(pb, 3 * pb)], origin, [2 * pb], [0], out, pb, cb,
                                        crc_fn)
    assert bt == 0 and not bad.any() and unw.tolist() == [1]
    assert (out[pb:2 * pb] == origin[3 * pb:4 * pb]).all()
    # a corrupt origin byte under a set bit is not delivered
    org = origin.copy()
    org[2 * pb + 5] ^= 0x01                                # origin bytes of the read's first page (written)
    out3 = np.full(4 * pb, OUT_SENT, np.uint8)
    read_merge_model(pool, crcs, slot, 1, bm, [(pb, 3 * pb)], org, [2 * pb], [0], out3, pb, cb, crc_fn)
    assert (out3[:3 * pb] == np.concatenate([pool[pb:2 * pb], org[3 * pb:4 * pb], pool[3 * pb:4 * pb]])).all()
    assert (out3[:pb] != org[2 * pb:3 * pb]).any()
    # a corrupt WRITTEN page is counted and still delivered; the other chunk is no clone
    dirty = pool.copy()
    dirty[3 * pb] ^= 1
    dirty[6 * pb] ^= 1
    out = np.full(10 * pb, OUT_SENT, np.uint8)
    bad, bt, unw, ut = read_merge_model(dirty, crcs, slot, 1, bm, [(0, 2 * cb)], origin, [NO_ORIGIN], [0], out, pb, cb,
                                        crc_fn)
    assert bad.tolist() == [2] and bt == 2 and unw.tolist() == [1]
    assert (out[3 * pb:4 * pb] == dirty[3 * pb:4 * pb]).all() and (out[2 * pb:3 * pb] == OUT_SENT).all()
    # invalid reads: both words UINT32_MAX, nothing written; an origin overrun on a read with no origin is valid
    reads = [(128, pb), (0, 100), (2 * cb, pb), (2 * cb - pb, 2 * pb), (0, pb), (0, pb), (0, pb), (0, pb), (0, pb),
             (pb, 0)]
    out_off = [0, 0, 0, 0, 2, 4 * pb - 4, 0, 0, 0, 0]
    origin_off = [0, 0, 0, 0, 0, 0, 6, 8 * pb - 4, NO_ORIGIN, 1 << 50]
    out = np.full(4 * pb, OUT_SENT, np.uint8)
    bad, bt, unw, ut = read_merge_model(pool, crcs, slot, 1, bm, reads, origin[:8 * pb], origin_off, out_off, out, pb,
                                        cb, crc_fn)
    assert bad.tolist() == [U32_MAX] * 8 + [0, 0] and unw.tolist() == [U32_MAX] * 8 + [0, 0]
    assert (out[:pb] == pool[:pb]).all() and (out[pb:] == OUT_SENT).all()


# --------------------------------------------------------------------------- clone_read's composition
class Host:
    """A host array where crc.clone_read expects a device tensor it reads back (.cpu().numpy())."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def clone_read_model(monkeypatch, pool, crcs, image, slot, n_slots, bm, reads, pb, cb, crc_fn, paste=True):
    """crc.clone_read ITSELF, with its three device calls replaced by their
    models on host arrays (clone_check_reads -> check_reads_model, read_merge ->
    read_merge_model with the outputs packed back to back, paste ->
    paste_model); `fetch` hands out each read's slice of the origin image, one
    buffer, packed.  Returns (out, out_off, bad, unwritten, the index lists
    fetch was called with, pasted total)."""
    from curve_amd import crc as C
    fetched, pasted = [], []

    def as_reads(off, ln):
        return [(int(o), int(n)) for o, n in zip(off, ln)]

    def fake_check(pool_, off, ln, clone, page_bytes, stream=None):
        counts, total = check_reads_model(as_reads(off, ln), pool_.size, slot, n_slots, bm, page_bytes, cb)
        return Host(counts.view(np.int32)), total           # as the device call: int32, -1 = past the pool

    def fake_read_merge(pool_, crcs_, off, ln, clone, origin=None, origin_off=None, page_bytes=pb, stream=None):
        rd = as_reads(off, ln)
        out_off, out_bytes = packed_offsets([n for _, n in rd])
        out = np.full(out_bytes, OUT_SENT, np.uint8)
        bad, bt, unw, ut = read_merge_model(pool_, crcs_, slot, n_slots, bm, rd, origin, origin_off, out_off, out,
                                            page_bytes, cb, crc_fn)
        return out, out_off, bad, bt, unw, ut

    def fake_paste(pool_, crcs_, origin, dst, src, lens, clone, page_bytes=pb, stream=None):
        entries = [(int(d), int(o), int(n)) for d, o, n in zip(dst, src, lens)]
        per, total = paste_model(pool_, crcs_, origin, entries, slot, n_slots, bm, page_bytes, cb, crc_fn)
        pasted.append(total)
        return per

    def fetch(idx):
        idx = [int(i) for i in idx]
        fetched.append(idx)
        offs, total = packed_offsets([reads[i][1] for i in idx])
        origin = np.concatenate([image[reads[i][0]:reads[i][0] + reads[i][1]] for i in idx])
        assert origin.size == total
        return origin, offs

    monkeypatch.setattr(C, "clone_check_reads", fake_check)
    monkeypatch.setattr(C, "read_merge", fake_read_merge)
    monkeypatch.setattr(C, "paste", fake_paste)
    out, out_off, bad, _, unw, _ = C.clone_read(pool, crcs, [r[0] for r in reads], [r[1] for r in reads], None, fetch,
                                                paste=paste, page_bytes=pb)
    assert len(fetched) <= 1 and len(pasted) <= len(fetched)
    return out, out_off, bad, unw, fetched, sum(pasted)


def replay_handle_read_requests(pool, crcs, image, slot, n_slots, bm, reads, pb, cb, crc_fn, paste=True):
    """The same batch as len(reads) CloneCore::HandleReadRequest calls in
    order, each cut per chunk as the client cuts it: needClone = isClone &&
    NextClearBit(begin, end) != NO_POS; without it ReadChunk; with it the
    download of [offset, offset + length), ReadThenMerge into the response, then
    (enablePaste_) PasteCloneData -> CSChunkFile::Paste.  Returns the responses."""
    out = []
    for i, c, off, ln, _ in cut_per_chunk(reads, cb):
        s = int(slot[c])
        clear = s < n_slots and any(not bit(bm, s, q) for q in range(off // pb, (off + ln) // pb))
        base = c * cb + off
        if not clear:
            out.append((i, pool[base:base + ln].copy()))
            continue
        clone_data = image[base:base + ln]
        out.append((i, replay_read_then_merge(pool, slot, n_slots, bm, c, off, ln, clone_data, pb, cb)))
        if paste:
            replay_paste(pool, crcs, clone_data, [(base, 0, ln)], slot, n_slots, bm, pb, cb, crc_fn)
    return out


@pytest.mark.parametrize("paste", [True, False])
def test_clone_read_composition_equals_the_sequential_replay(oracle, monkeypatch, paste):
    """crc.clone_read, its device calls replaced by their models.  The origin is ONE immutable image the size of the pool and every fetched
    buffer a slice of it, so whichever request pastes a page first pastes the
    same bytes: the batch's outputs, final pool, CRC table and bitmaps equal the
    request-by-request replay, overlapping reads included.  (The batch judges
    every page by the bitmaps before the call and delivers the origin's bytes;
    the replay's later request finds the page pasted and reads the pool -- the
    same bytes.  The lowest-index paste rule picks among identical sources.)"""
    pb, ppc = 256, 40
    slot, n_slots, cb = geometry(ppc, pb)
    crc_fn = lambda b: oracle.crc32c(b.tobytes())
    rng = np.random.default_rng(17)
    pool = rng.integers(0, 256, slot.size * cb, dtype=np.uint8)
    image = rng.integers(0, 256, pool.size, dtype=np.uint8)
    bm = np.zeros((n_slots, 2), np.uint32)
    for s in range(n_slots):
        for q in range(ppc):
            if rng.random() < 0.3:
                set_bit(bm, s, q)
    crcs = oracle.page_crcs(pool, pb)
    n_pages = pool.size // pb
    reads = []
    for _ in range(60):
        k = int(rng.integers(1, 9))
        reads.append((int(rng.integers(0, n_pages - k + 1)) * pb, k * pb))
    reads += [(3 * pb, 6 * pb), (5 * pb, 6 * pb), (3 * pb, 6 * pb), (38 * pb, 5 * pb), (39 * pb, 3 * pb)]  # overlapping
    r_pool, r_crcs, r_bm = pool.copy(), crcs.copy(), bm.copy()
    bm0 = bm.copy()
    out, out_off, bad, unw, fetched, pasted = clone_read_model(monkeypatch, pool, crcs, image, slot, n_slots, bm, reads,
                                                               pb, cb, crc_fn, paste)
    assert len(fetched) == 1
    need = fetched[0]
    responses = replay_handle_read_requests(r_pool, r_crcs, image, slot, n_slots, r_bm, reads, pb, cb, crc_fn, paste)
    at = {}
    for i, data in responses:
        o = int(out_off[i]) + at.get(i, 0)
        assert (out[o:o + data.size] == data).all(), i
        at[i] = at.get(i, 0) + data.size
    assert (out != OUT_SENT).any() and not bad.any()
    assert (pool == r_pool).all() and (crcs == r_crcs).all() and (bm == r_bm).all()
    assert (crcs == oracle.page_crcs(pool, pb)).all()
    assert len(need) >= 20 and len(need) < len(reads) and (unw[need] > 0).all()
    if paste:
        assert pasted > 0 and (bm != bm0).any()
        again = clone_read_model(monkeypatch, pool, crcs, image, slot, n_slots, bm, reads, pb, cb, crc_fn, paste)
        assert (again[0] == out).all() and not again[3].any() and again[4] == [] and again[5] == 0
    else:
        assert pasted == 0 and (bm == bm0).all()


def test_clone_read_without_unwritten_pages_fetches_nothing(oracle, monkeypatch):
    pb, ppc = 256, 5
    slot, n_slots, cb = geometry(ppc, pb)
    rng = np.random.default_rng(3)
    pool = rng.integers(0, 256, slot.size * cb, dtype=np.uint8)
    bm = bitmaps("all_set", n_slots, ppc, rng)
    crcs = oracle.page_crcs(pool, pb)
    reads = [(0, 3 * pb), (4 * pb, 4 * pb), (0, pool.size)]
    before = pool.copy()
    out, out_off, bad, unw, need, pasted = clone_read_model(monkeypatch, pool, crcs, None, slot, n_slots, bm, reads, pb,
                                                            cb, lambda b: oracle.crc32c(b.tobytes()))
    assert need == [] and pasted == 0 and not unw.any() and not bad.any() and (pool == before).all()
    for i, (off, ln) in enumerate(reads):
        assert (out[int(out_off[i]):int(out_off[i]) + ln] == pool[off:off + ln]).all()


def test_clone_read_never_fetches_a_misaligned_read(oracle, monkeypatch):
    """CloneReadByLocalInfo refuses a misaligned request before any download:
    such a read is not fetched and not pasted even where it touches
    never-written pages; read_merge marks it invalid."""
    pb, ppc = 256, 5
    slot, n_slots, cb = geometry(ppc, pb)
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 256, slot.size * cb, dtype=np.uint8)
    image = rng.integers(0, 256, pool.size, dtype=np.uint8)
    bm = bitmaps("all_clear", n_slots, ppc, rng)
    crcs = oracle.page_crcs(pool, pb)
    reads = [(pb + 128, pb), (0, 2 * pb), (3 * pb, pb + 4), (5 * pb, pb)]   # chunk 0: a clone; chunk 1: none
    out, out_off, bad, unw, fetched, pasted = clone_read_model(monkeypatch, pool, crcs, image, slot, n_slots, bm, reads,
                                                               pb, cb, lambda b: oracle.crc32c(b.tobytes()))
    assert fetched == [[1]] and pasted == 2
    assert bad.tolist() == [U32_MAX, 0, U32_MAX, 0] and unw.tolist() == [U32_MAX, 2, U32_MAX, 0]
    assert int(bm[0, 0]) == 0b00011 and (pool[:2 * pb] == image[:2 * pb]).all()
    assert (out[int(out_off[1]):int(out_off[1]) + 2 * pb] == image[:2 * pb]).all()
    assert (out[int(out_off[0]):int(out_off[0]) + pb] == OUT_SENT).all()


# --------------------------------------------------------------------------- the GPU file's inputs
PPC, N_SLOTS = 40, 4
SLOTS = [0, NOT_CLONE, 2, NOT_CLONE, 1, 7, NOT_CLONE, 3]     # test_clone_gpu's rig
N_PAGES = len(SLOTS) * PPC
GPU_SEEDS = {256: 50, 512: 51, 1024: 52, 2048: 53, 4096: 54, 8192: 55}


def rig_bitmaps(rng, density):
    """test_clone_gpu.random_bitmaps, restated (that module needs torch)."""
    bm = np.zeros((N_SLOTS, (PPC + 31) // 32), np.uint32)
    for s in range(N_SLOTS):
        for q in range(PPC):
            if rng.random() < density:
                set_bit(bm, s, q)
    return bm


def gpu_reads(rng, n, pb, lo=1, hi=8):
    """test_snap_read_gpu.random_reads, restated (that module needs torch): n
    page-aligned reads of lo..hi pages; the first four cross chunk boundaries
    between chunks with different slots and end on the pool's last page."""
    reads = []
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        reads.append((int(rng.integers(0, N_PAGES - k + 1)) * pb, k * pb))
    fixed = [(PPC - 2, 4), (2 * PPC - 3, 5), (5 * PPC - 1, 2), (N_PAGES - 3, 3)]
    for i, (p0, k) in enumerate(fixed[:n]):
        reads[i] = (p0 * pb, k * pb)
    return reads


SRC_PAGES = 512                                              # test_clone_gpu's source buffer: the origin here


def gpu_batch(seed, n, pb, lo=1, hi=8):
    """Test 1's batch: the reads, and for about a quarter of them no origin;
    the others' origin bytes start at a 4-byte-aligned place of their own in the
    SRC_PAGES-page origin buffer.  Returns (reads, origin_off)."""
    rng = np.random.default_rng(seed * 1000 + n)
    reads = gpu_reads(rng, n, pb, lo, hi)
    none = rng.random(n) < 0.25
    at = np.array([int(rng.integers(0, (SRC_PAGES * pb - ln) // 4 + 1)) * 4 for _, ln in reads], np.uint64)
    return reads, np.where(none, np.uint64(NO_ORIGIN), at)


def page_classes(reads, origin_off, slots, n_slots, bm, pb, ppc=PPC):
    """The page slots of a batch of valid reads by what becomes of them: (plain
    chunk, out-of-range slot, clone page with its bit set, unwritten with an
    origin, unwritten without)."""
    plain = oor = held = with_o = without = 0
    for i, (off, ln) in enumerate(reads):
        for p in range(off // pb, (off + ln) // pb):
            c, q = divmod(p, ppc)
            s = int(slots[c])
            if s == NOT_CLONE:
                plain += 1
            elif s >= n_slots:
                oor += 1
            elif bit(bm, s, q):
                held += 1
            elif int(origin_off[i]) != NO_ORIGIN:
                with_o += 1
            else:
                without += 1
    return plain, oor, held, with_o, without


@pytest.mark.parametrize("n", [65, 3000])
@pytest.mark.parametrize("pb", sorted(GPU_SEEDS))
def test_gpu_seeds_meet_the_class_count_condition(pb, n):
    """The inputs test_read_merge_gpu.py's first test uses, as that test draws
    them (the rig's generator draws pool, bitmaps, then the source): for n >= 65
    every class has at least 10 page slots."""
    rng = np.random.default_rng(GPU_SEEDS[pb])
    rng.integers(0, 256, N_PAGES * pb, dtype=np.uint8)     # the rig's pool comes first
    bm = rig_bitmaps(rng, 0.3)
    reads, origin_off = gpu_batch(GPU_SEEDS[pb], n, pb)
    counts = page_classes(reads, origin_off, np.array(SLOTS, np.uint32), N_SLOTS, bm, pb)
    assert min(counts) >= 10, counts


# --------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_new_symbol():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    assert re.search(r"^int cc_read_merge_dev\(", hdr, re.M)
    assert hasattr(_lib.lib(), "cc_read_merge_dev") and "cc_read_merge_dev" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cc_read_merge_dev"][1]) == 18
    assert re.search(r"^#define CC_NO_ORIGIN 0xFFFFFFFFFFFFFFFFull", hdr, re.M)
    assert _lib.CC_NO_ORIGIN == NO_ORIGIN
    decl = hdr[hdr.index("Clone reads: a batch of CloneCore::ReadThenMerge"):hdr.index("int cc_read_merge_dev(")]
    decl = re.sub(r"[\s*]+", " ", decl)
    assert "d_out must not alias d_pool or d_origin" in decl and "on another stream at the same time" in decl


FAKE = 1 << 20  # a fake device pointer: never dereferenced (the checks come first, and no device is present)


def _good_clone():
    from curve_amd import _lib
    c = _lib.CcClone()
    c.chunk_bytes, c.n_slots = 64 << 10, 2
    c.d_clone_slot = c.d_bitmap = FAKE
    c.d_claim = c.d_pasted = None                           # never touched by this call
    return c


def _call(L, clone="good", pool=FAKE, pool_bytes=1 << 20, page_bytes=4096, reads=FAKE, n=3, crcs=FAKE, origin=FAKE,
          origin_off=FAKE, origin_bytes=1 << 20, out=FAKE, out_off=FAKE, out_bytes=1 << 20, bad=FAKE, total=FAKE,
          unw=FAKE, unw_total=FAKE):
    vp = ctypes.c_void_p
    clone = _good_clone() if isinstance(clone, str) else clone
    return L.cc_read_merge_dev(vp(pool), pool_bytes, page_bytes, vp(reads), n, vp(crcs),
                               ctypes.byref(clone) if clone is not None else None, vp(origin), vp(origin_off),
                               origin_bytes, vp(out), vp(out_off), out_bytes, vp(bad), vp(total), vp(unw),
                               vp(unw_total), None)


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    E = _lib.CC_EINVAL
    for pb in (0, 100, 128, 1000, 3 * 256, 16384):           # not 256 * 2^k, k = 0..5
        assert _call(L, page_bytes=pb) == E, pb
    assert _call(L, pool_bytes=(1 << 20) + 256) == E         # not whole 4 KiB pages
    assert _call(L, pool=FAKE + 2) == E                      # misaligned pool
    for name in ("pool", "reads", "crcs", "bad", "total"):
        assert _call(L, **{name: None}) == E, name
    assert _call(L, n=1 << 31) == E
    assert _call(L, out=None) == E and _call(L, out_off=None) == E   # no verify-only mode
    assert _call(L, out=None, out_off=None) == E
    assert _call(L, out=FAKE + 1) == E                       # misaligned output
    assert _call(L, unw=None) == E and _call(L, unw_total=None) == E
    assert _call(L, None) == E                               # no clone
    for field in ("d_clone_slot", "d_bitmap"):
        c = _good_clone()
        setattr(c, field, None)
        assert _call(L, c) == E, field
    for cb in (96 << 10, (64 << 10) + 256, 0):               # does not divide the pool; no page multiple; zero
        c = _good_clone()
        c.chunk_bytes = cb
        assert _call(L, c) == E, cb
    assert _call(L, origin_off=None) == E                    # an origin without its offsets
    assert _call(L, origin=FAKE + 2) == E                    # misaligned origin
    # an empty batch is a no-op, with or without anything else
    assert _call(L, n=0) == _lib.CC_OK
    assert _call(L, None, n=0, out=None, out_off=None, origin=None, origin_off=None) == _lib.CC_OK


def test_well_formed_call_needs_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    N = _lib.CC_ENODEV
    assert _call(L) == N
    assert _call(L, origin=None, origin_off=None, origin_bytes=0) == N   # no origin at all
    assert _call(L, origin=None) == N                        # offsets without a buffer: ignored
    assert _call(L, n=(1 << 31) - 1) == N
    for pb in (256, 512, 1024, 2048, 4096, 8192):
        assert _call(L, page_bytes=pb) == N, pb
    c = _good_clone()
    c.n_slots = 0                                            # no clone chunk anywhere
    assert _call(L, c) == N
    c = _good_clone()
    c.d_claim = c.d_pasted = FAKE
    assert _call(L, c) == N
    assert _call(L, out_bytes=0, origin_bytes=0) == N        # every read invalid: still a device call
