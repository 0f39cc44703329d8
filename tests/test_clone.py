"""Clone chunks on the device (cc_paste_dev, cc_clone_mark_dev,
cc_clone_check_reads_dev): everything that needs no GPU.

The numpy models of the three calls live here (paste_model: lowest-index claim,
then write, mark and count; mark_model; check_reads_model) and are checked
against request-by-request restatements of the reference: CSChunkFile::Paste
(chunkserver_chunkfile.cpp:440-495: per chunk, Divide() the request's blocks,
writeData per uncopied run, flush() sets the bits), Write ... flush() on a clone
chunk (:405-406, :965-1000) and Read's NextClearBit test (:510-526).  The GPU
tests (test_clone_gpu.py) lean on the models, never on the code under test.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_snap_read import bit_runs, cut_per_chunk

U32_MAX = 0xFFFFFFFF
NOT_CLONE = 0xFFFFFFFF


# --------------------------------------------------------------------------- models
def bit(bm, s, q):
    return (int(bm[s, q // 32]) >> (q % 32)) & 1


def set_bit(bm, s, q):
    bm[s, q // 32] |= np.uint32(1 << (q % 32))


def paste_valid(dst, so, ln, pool_bytes, src_bytes, pb):
    """cc_paste_dev's contract per entry (include/curve_crc.h)."""
    if ln == 0:
        return True
    if dst % pb or ln % pb:
        return False
    if dst >= pool_bytes or ln > pool_bytes - dst:
        return False
    return not (so % 4 or so > src_bytes or ln > src_bytes - so)


def paste_model(pool, crcs, src, entries, slot, n_slots, bm, pb, cb, crc_fn):
    """One cc_paste_dev call on host arrays, in place: every page of a clone
    chunk whose bit is clear goes to the LOWEST-indexed valid entry covering it
    (the claim), then each claimed page is written, hashed, marked and counted.
    entries = [(dst, src, len)].  Returns (pasted_per_entry uint32, total)."""
    ppc = cb // pb
    per = np.zeros(len(entries), np.uint32)
    claim = {}
    for i, (dst, so, ln) in enumerate(entries):
        if not paste_valid(dst, so, ln, pool.size, src.size, pb):
            per[i] = U32_MAX
            continue
        for p in range(dst // pb, (dst + ln) // pb):
            c, q = divmod(p, ppc)
            s = int(slot[c])
            if s < n_slots and not bit(bm, s, q):
                claim.setdefault(p, i)  # entries come in index order: the first to bid is the lowest
    for p, i in claim.items():
        dst, so, _ = entries[i]
        at = so + p * pb - dst
        pool[p * pb:(p + 1) * pb] = src[at:at + pb]
        crcs[p] = crc_fn(pool[p * pb:(p + 1) * pb])
        c, q = divmod(p, ppc)
        set_bit(bm, int(slot[c]), q)
        per[i] += 1
    return per, len(claim)


def replay_paste(pool, crcs, src, entries, slot, n_slots, bm, pb, cb, crc_fn):
    """The same batch as len(entries) CSChunkFile::Paste calls, one after the
    other: the entry is cut per chunk it spans; a chunk that is no clone returns
    Success and writes nothing; otherwise Divide(beginIndex, endIndex, &uncopied,
    nullptr), writeData per uncopied run, and flush() sets the runs' bits.  The
    CRC table follows every writeData."""
    per = np.zeros(len(entries), np.uint32)
    total = 0
    for i, (dst, so, ln) in enumerate(entries):
        if not paste_valid(dst, so, ln, pool.size, src.size, pb):  # CheckOffsetAndLength / the call's contract
            per[i] = U32_MAX
            continue
        for _, c, off, n, at in cut_per_chunk([(dst, ln)], cb):
            s = int(slot[c])
            if s >= n_slots:
                continue
            uncopied, _ = bit_runs(bm[s], off // pb, (off + n - 1) // pb)
            for b, e in uncopied:
                ro, rs = b * pb, (e - b + 1) * pb
                pool[c * cb + ro:c * cb + ro + rs] = src[so + at + ro - off:so + at + ro - off + rs]
                for q in range(b, e + 1):
                    p = c * (cb // pb) + q
                    crcs[p] = crc_fn(pool[p * pb:(p + 1) * pb])
            for b, e in uncopied:  # flush()
                for q in range(b, e + 1):
                    set_bit(bm, s, q)
                per[i] += e - b + 1
                total += e - b + 1
    return per, total


def write_valid(dst, ln, max_len, pool_bytes):
    return 1 <= ln <= max_len and dst < pool_bytes and ln <= pool_bytes - dst


def write_model(pool, src, log, max_len):
    """The write log's bytes (cc_apply_log_dev): valid entries in order, later ones win.  log = [(dst, src, len)]."""
    for dst, so, ln in log:
        if write_valid(dst, ln, max_len, pool.size):
            pool[dst:dst + ln] = src[so:so + ln]


def mark_model(log, max_len, pool_bytes, slot, n_slots, bm, pb, cb):
    """One cc_clone_mark_dev call: the bit of every page a valid entry covers WHOLE, in clone chunks."""
    ppc = cb // pb
    for dst, _, ln in log:
        if not write_valid(dst, ln, max_len, pool_bytes):
            continue
        for p in range(-(-dst // pb), (dst + ln) // pb):
            c, q = divmod(p, ppc)
            if int(slot[c]) < n_slots:
                set_bit(bm, int(slot[c]), q)


def replay_write_flush(pool, src, log, slot, n_slots, bm, pb, cb):
    """Block-aligned CSChunkFile::Write requests, one after the other, per chunk:
    writeData, then on a clone chunk flush() sets bits [beginIndex, endIndex]."""
    for dst, so, ln in log:
        assert dst % pb == 0 and ln % pb == 0 and ln > 0  # CheckOffsetAndLength
        for _, c, off, n, at in cut_per_chunk([(dst, ln)], cb):
            pool[c * cb + off:c * cb + off + n] = src[so + at:so + at + n]
            s = int(slot[c])
            if s < n_slots:
                for q in range(off // pb, (off + n - 1) // pb + 1):
                    set_bit(bm, s, q)


def check_reads_model(reads, pool_bytes, slot, n_slots, bm, pb, cb):
    """One cc_clone_check_reads_dev call.  Returns (unwritten_per_read uint32, total)."""
    ppc = cb // pb
    out = np.zeros(len(reads), np.uint32)
    total = 0
    for i, (off, ln) in enumerate(reads):
        if ln == 0:
            continue
        if off >= pool_bytes or ln > pool_bytes - off:
            out[i] = U32_MAX
            continue
        for p in range(off // pb, (off + ln - 1) // pb + 1):
            c, q = divmod(p, ppc)
            s = int(slot[c])
            if s < n_slots and not bit(bm, s, q):
                out[i] += 1
                total += 1
    return out, total


NO_POS = 0xFFFFFFFF


def next_clear_bit(row, begin, end):
    """Bitmap::NextClearBit(begin, end): the first clear bit in [begin, end], or NO_POS."""
    for q in range(begin, end + 1):
        if not (int(row[q // 32]) >> (q % 32)) & 1:
            return q
    return NO_POS


# --------------------------------------------------------------------------- the hand-made geometry
PB, PPC, N_SLOTS = 256, 5, 2
CB = PB * PPC
SLOT = np.array([0, NOT_CLONE, 7, 1], np.uint32)   # chunk 2: out of range for n_slots = 2
POOL_BYTES = SLOT.size * CB
SRC_BYTES = 64 * PB


def fresh(preset, seed=0):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, POOL_BYTES, dtype=np.uint8)
    src = rng.integers(0, 256, SRC_BYTES, dtype=np.uint8)
    bm = np.zeros((N_SLOTS, (PPC + 31) // 32), np.uint32)
    for s, q in preset:
        set_bit(bm, s, q)
    return pool, src, bm


def P(page, src_page, pages):
    return (page * PB, src_page * PB, pages * PB)


BATCHES = {
    # many entries over the same pages of chunk 0 (and chunk 3), each from another source
    "same_pages": [P(1, 10, 3), P(0, 20, 5), P(1, 30, 3), P(2, 40, 1), P(15, 5, 5), P(16, 50, 2), P(1, 0, 4)],
    # entries crossing clone | non-clone (0 | 1), non-clone | out of range (1 | 2), out of range | clone (2 | 3)
    "crossing": [P(3, 0, 4), P(8, 8, 4), P(13, 16, 4), P(0, 24, 20)],
    # every kind of invalid entry among valid ones
    "invalid": [P(0, 0, 1), (PB + 128, 0, PB), (2 * PB, 0, PB + 4), (POOL_BYTES - PB, 0, 2 * PB), (POOL_BYTES, 0, PB),
                (1 << 40, 0, PB), (3 * PB, 2, PB), (3 * PB, SRC_BYTES - PB + 4, PB), (3 * PB, SRC_BYTES, PB),
                (3 * PB, 1 << 40, PB), P(3, 63, 1), P(4, 62, 2)],
    # chunk 0 filled completely, by pieces out of order
    "fill_chunk0": [P(3, 3, 2), P(0, 10, 2), P(2, 7, 1), P(0, 30, 5)],
    # an empty entry: valid whatever its offsets
    "empty": [P(0, 0, 2), (1, 3, 0), (1 << 50, 1 << 50, 0), P(1, 5, 2)],
}
PRESETS = {"clear": [], "preset": [(0, 2), (1, 0), (1, 4)]}


@pytest.mark.parametrize("preset", sorted(PRESETS))
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_paste_model_equals_request_by_request_replay(oracle, batch, preset):
    crc_fn = lambda b: oracle.crc32c(b.tobytes())
    entries = BATCHES[batch]
    pool, src, bm = fresh(PRESETS[preset], seed=len(batch))
    crcs = oracle.page_crcs(pool, PB)
    before, bm0 = pool.copy(), bm.copy()
    r_pool, r_crcs, r_bm = pool.copy(), crcs.copy(), bm.copy()
    per, total = paste_model(pool, crcs, src, entries, SLOT, N_SLOTS, bm, PB, CB, crc_fn)
    r_per, r_total = replay_paste(r_pool, r_crcs, src, entries, SLOT, N_SLOTS, r_bm, PB, CB, crc_fn)
    assert (pool == r_pool).all() and (crcs == r_crcs).all() and (bm == r_bm).all()
    assert per.tolist() == r_per.tolist() and total == r_total
    assert (crcs == oracle.page_crcs(pool, PB)).all()
    # chunks 1 and 2 are no clones, and a page whose bit was set keeps its bytes
    assert (pool[CB:3 * CB] == before[CB:3 * CB]).all()
    for s, q in PRESETS[preset]:
        c = int(np.nonzero(SLOT == s)[0][0])
        assert (pool[c * CB + q * PB:c * CB + (q + 1) * PB] == before[c * CB + q * PB:c * CB + (q + 1) * PB]).all()
    assert total == sum(bin(int(w)).count("1") for w in bm.ravel()) - sum(bin(int(w)).count("1") for w in bm0.ravel())


def test_paste_model_cases_by_hand(oracle):
    """The batches' answers, written down: who wins, what is invalid, what fills."""
    crc_fn = lambda b: oracle.crc32c(b.tobytes())
    pool, src, bm = fresh([], seed=1)
    crcs = oracle.page_crcs(pool, PB)
    per, total = paste_model(pool, crcs, src, BATCHES["same_pages"], SLOT, N_SLOTS, bm, PB, CB, crc_fn)
    assert per.tolist() == [3, 2, 0, 0, 5, 0, 0] and total == 10
    assert (pool[PB:4 * PB] == src[10 * PB:13 * PB]).all() and (pool[:PB] == src[20 * PB:21 * PB]).all()
    assert (pool[4 * PB:5 * PB] == src[24 * PB:25 * PB]).all()
    assert int(bm[0, 0]) == 0b11111 and int(bm[1, 0]) == 0b11111
    pool, src, bm = fresh([], seed=2)
    crcs = oracle.page_crcs(pool, PB)
    before = pool.copy()
    per, total = paste_model(pool, crcs, src, BATCHES["invalid"], SLOT, N_SLOTS, bm, PB, CB, crc_fn)
    assert per.tolist() == [1] + [U32_MAX] * 9 + [1, 1] and total == 3  # the last entry crosses into chunk 1
    assert (pool[PB:3 * PB] == before[PB:3 * PB]).all() and (pool[5 * PB:] == before[5 * PB:]).all()
    pool, src, bm = fresh([(0, 2)], seed=3)
    crcs = oracle.page_crcs(pool, PB)
    per, total = paste_model(pool, crcs, src, BATCHES["fill_chunk0"], SLOT, N_SLOTS, bm, PB, CB, crc_fn)
    assert per.tolist() == [2, 2, 0, 0] and total == 4 and int(bm[0, 0]) == 0b11111
    pool, src, bm = fresh([], seed=4)
    crcs = oracle.page_crcs(pool, PB)
    per, total = paste_model(pool, crcs, src, BATCHES["empty"], SLOT, N_SLOTS, bm, PB, CB, crc_fn)
    assert per.tolist() == [2, 0, 0, 1] and total == 3


def aligned_writes(rng, n):
    log = []
    for _ in range(n):
        k = int(rng.integers(1, 5))
        p0 = int(rng.integers(0, POOL_BYTES // PB - k + 1))
        log.append((p0 * PB, int(rng.integers(0, 60 - k)) * PB, k * PB))
    return log


def test_mark_model_equals_write_flush_replay_and_marks_whole_pages_only():
    rng = np.random.default_rng(7)
    log = aligned_writes(rng, 6)
    _, src, bm = fresh([(1, 3)])
    pool = np.zeros(POOL_BYTES, np.uint8)
    r_bm = bm.copy()
    mark_model(log, 4 * PB, POOL_BYTES, SLOT, N_SLOTS, bm, PB, CB)
    replay_write_flush(pool, src, log, SLOT, N_SLOTS, r_bm, PB, CB)
    assert (bm == r_bm).all() and bm.any()
    # unaligned entries: only the pages covered whole
    bm[:] = 0
    log = [(100, 0, PB),                    # straddles pages 0 | 1: neither whole
           (PB + 1, 0, 2 * PB - 1),          # page 1 partly, page 2 whole
           (3 * PB, 0, PB - 1),              # page 3 less its last byte
           (3 * PB + PB - 1, 0, 1),          # ... and that byte alone: two partial entries do not count
           (15 * PB + 8, 0, 3 * PB),         # chunk 3: pages 16, 17 whole, 15 and 18 partly
           (4 * PB + 200, 0, 3 * PB),        # crosses into chunk 1 (no clone): nothing whole in chunk 0
           (19 * PB, 0, PB)]                 # the pool's last page
    mark_model(log, 4 * PB, POOL_BYTES, SLOT, N_SLOTS, bm, PB, CB)
    assert int(bm[0, 0]) == 0b00100 and int(bm[1, 0]) == 0b10110
    # contract breakers mark nothing
    bm[:] = 0
    log = [(0, 0, 0), (0, 0, 4 * PB + 1), (POOL_BYTES - PB, 0, 2 * PB), (POOL_BYTES, 0, PB), (1 << 40, 0, PB)]
    mark_model(log, 4 * PB, POOL_BYTES, SLOT, N_SLOTS, bm, PB, CB)
    assert not bm.any()


@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_check_reads_model_equals_next_clear_bit(preset):
    rng = np.random.default_rng(11)
    _, _, bm = fresh(PRESETS[preset] + [(0, 0), (0, 1), (1, 2)])
    reads = [(int(rng.integers(0, POOL_BYTES)), int(rng.integers(1, 3 * PB))) for _ in range(150)]
    reads = [(o, min(n, POOL_BYTES - o)) for o, n in reads]
    # ... the whole pool, chunk crossings, and chunk 3's page 16 (never set) beside page 17 (set)
    reads += [(0, POOL_BYTES), (4 * PB + 10, 2 * PB), (14 * PB + 255, 2), (17 * PB, 1), (17 * PB - 1, 2), (5, 0)]
    got, total = check_reads_model(reads, POOL_BYTES, SLOT, N_SLOTS, bm, PB, CB)
    for i, (off, ln) in enumerate(reads):
        refused = clear = 0
        for _, c, o, n, _ in cut_per_chunk([(off, ln)], CB):
            s = int(SLOT[c])
            if s >= N_SLOTS:
                continue
            b, e = o // PB, (o + n - 1) // PB
            refused += next_clear_bit(bm[s], b, e) != NO_POS   # Read: PageNerverWrittenError
            clear += sum(1 - bit(bm, s, q) for q in range(b, e + 1))
        assert (got[i] != 0) == bool(refused) and got[i] == clear, (i, off, ln)
    assert total == int(got.sum()) and got[-2] == 1 and got[-1] == 0
    past, _ = check_reads_model([(POOL_BYTES - 1, 2), (POOL_BYTES, 1), (1 << 40, 5), (POOL_BYTES - 1, 1)], POOL_BYTES,
                                SLOT, N_SLOTS, bm, PB, CB)
    assert past.tolist()[:3] == [U32_MAX] * 3 and past[3] != U32_MAX


@pytest.mark.parametrize("order", ["write_then_paste", "paste_then_write"])
def test_write_with_mark_and_paste_equal_the_interleaved_replay(oracle, order):
    """A write batch with its mark call, then a paste batch (and the other way
    round) == the same requests replayed one by one: a paste never overwrites a
    written page, and a write lands over pasted data."""
    crc_fn = lambda b: oracle.crc32c(b.tobytes())
    rng = np.random.default_rng(13)
    writes = aligned_writes(rng, 5)
    pastes = [P(0, 30, 5), P(3, 40, 9), P(14, 50, 6), P(16, 0, 2)]
    pool, src, bm = fresh([(1, 1)], seed=5)
    wsrc = np.random.default_rng(6).integers(0, 256, SRC_BYTES, dtype=np.uint8)
    crcs = oracle.page_crcs(pool, PB)
    r_pool, r_crcs, r_bm = pool.copy(), crcs.copy(), bm.copy()

    def write_batch():
        write_model(pool, wsrc, writes, 4 * PB)
        crcs[:] = oracle.page_crcs(pool, PB)             # what cc_apply_log_dev leaves
        mark_model(writes, 4 * PB, POOL_BYTES, SLOT, N_SLOTS, bm, PB, CB)

    def paste_batch():
        return paste_model(pool, crcs, src, pastes, SLOT, N_SLOTS, bm, PB, CB, crc_fn)

    def replay_writes():
        replay_write_flush(r_pool, wsrc, writes, SLOT, N_SLOTS, r_bm, PB, CB)
        r_crcs[:] = oracle.page_crcs(r_pool, PB)

    if order == "write_then_paste":
        write_batch()
        written = pool.copy()
        per, total = paste_batch()
        replay_writes()
        r_per, r_total = replay_paste(r_pool, r_crcs, src, pastes, SLOT, N_SLOTS, r_bm, PB, CB, crc_fn)
        for dst, _, ln in writes:                         # every written byte survived the paste
            assert (pool[dst:dst + ln] == written[dst:dst + ln]).all()
    else:
        per, total = paste_batch()
        write_batch()
        r_per, r_total = replay_paste(r_pool, r_crcs, src, pastes, SLOT, N_SLOTS, r_bm, PB, CB, crc_fn)
        replay_writes()
    assert (pool == r_pool).all() and (crcs == r_crcs).all() and (bm == r_bm).all()
    assert per.tolist() == r_per.tolist() and total == r_total and total > 0


# --------------------------------------------------------------------------- metapage
def test_clone_metapage_after():
    from curve_amd import _lib
    from curve_amd.chunkfile import ChunkFileMetaPage, CSErrorCode, clone_metapage_after
    L = _lib.lib()
    loc = b"/clone/origin@cs"
    meta = ChunkFileMetaPage(sn=9, correctedSn=3, location=loc, bitmap_bits=40, bitmap=bytes(5))
    # a bitmap as the device holds it (two words a slot) round-trips through encode / decode
    words = np.array([0x80000001, 0x0000007F], np.uint32)
    m1 = clone_metapage_after(meta, words.tobytes()[:5])
    assert meta.bitmap == bytes(5)                                # a copy: the argument is untouched
    rc, back = ChunkFileMetaPage.decode(m1.encode())
    assert rc == CSErrorCode.Success and back.location == loc and back.bitmap_bits == 40
    assert back.bitmap == words.tobytes()[:5] and back.sn == 9 and back.correctedSn == 3
    # 39 of 40: still a clone
    almost = bytearray(b"\xff" * 5)
    almost[4] = 0x7F
    m39 = clone_metapage_after(meta, bytes(almost))
    rc, back = ChunkFileMetaPage.decode(m39.encode())
    assert rc == CSErrorCode.Success and back.location == loc and back.bitmap == bytes(almost)
    # 40 of 40 (bits past the 40th in the device word are not part of it): an ordinary chunk
    full = clone_metapage_after(meta, b"\xff" * 8)
    assert full.location == b"" and full.bitmap_bits == 0 and full.bitmap == b""
    page = full.encode()
    rc, back = ChunkFileMetaPage.decode(page)
    assert rc == CSErrorCode.Success and back.location == b"" and back.sn == 9 and back.correctedSn == 3
    assert page[25:29] == ChunkFileMetaPage(sn=9, correctedSn=3).encode()[25:29]   # the CRC sits at byte 25
    assert page == ChunkFileMetaPage(sn=9, correctedSn=3).encode()
    sn = ctypes.c_uint64(0)
    assert L.cc_chunk_meta_sn(page, 4096, ctypes.byref(sn)) == 0 and sn.value == 9
    assert L.cc_chunk_meta_sn(m39.encode(), 4096, ctypes.byref(sn)) == 0 and sn.value == 9
    # 33 bits: the partial last byte counts its low bit only
    m33 = ChunkFileMetaPage(sn=1, location=loc, bitmap_bits=33, bitmap=bytes(5))
    assert clone_metapage_after(m33, b"\xff\xff\xff\xff\x01").location == b""
    assert clone_metapage_after(m33, b"\xff\xff\xff\xff\xfe").location == loc
    # no clone: unchanged
    plain = ChunkFileMetaPage(sn=4)
    assert clone_metapage_after(plain, b"\xff") == plain


# --------------------------------------------------------------------------- ABI
NEW = ("cc_paste_dev", "cc_clone_mark_dev", "cc_clone_check_reads_dev")


def test_header_declares_and_library_exports_the_new_symbols():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    for name, nargs in zip(NEW, (11, 7, 8)):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"^#define CC_NOT_CLONE 0xFFFFFFFFu", hdr, re.M) and _lib.CC_NOT_CLONE == 0xFFFFFFFF
    assert "typedef struct cc_clone {" in hdr


def test_cc_clone_has_the_headers_layout():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    body = hdr[hdr.index("typedef struct cc_clone {"):hdr.index("} cc_clone;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+);", body)
    assert names == ["chunk_bytes", "n_slots", "d_clone_slot", "d_bitmap", "d_claim", "d_pasted"]
    assert [f[0] for f in _lib.CcClone._fields_] == names
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.CcClone) == 8 + 4 * ptr          # two u32, four pointers
    assert _lib.CcClone.chunk_bytes.offset == 0 and _lib.CcClone.n_slots.offset == 4
    for k, name in enumerate(names[2:]):
        assert getattr(_lib.CcClone, name).offset == 8 + k * ptr


FAKE = 1 << 20  # a fake device pointer: never dereferenced (the checks come first, and no device is present)


def _good_clone():
    from curve_amd import _lib
    c = _lib.CcClone()
    c.chunk_bytes, c.n_slots = 64 << 10, 2
    c.d_clone_slot = c.d_bitmap = c.d_claim = c.d_pasted = FAKE
    return c


def _paste(L, clone="good", pool=FAKE, pool_bytes=1 << 20, page_bytes=4096, src=FAKE, src_bytes=1 << 20, pastes=FAKE,
           n=3, crcs=FAKE, per_entry=FAKE):
    vp = ctypes.c_void_p
    clone = _good_clone() if isinstance(clone, str) else clone
    return L.cc_paste_dev(vp(pool), pool_bytes, page_bytes, vp(src), src_bytes, vp(pastes), n, vp(crcs),
                          ctypes.byref(clone) if clone is not None else None, vp(per_entry), None)


def _mark(L, clone="good", pool_bytes=1 << 20, page_bytes=4096, log=FAKE, n=3, max_len=4096):
    clone = _good_clone() if isinstance(clone, str) else clone
    return L.cc_clone_mark_dev(pool_bytes, page_bytes, ctypes.c_void_p(log), n, max_len,
                               ctypes.byref(clone) if clone is not None else None, None)


def _check(L, clone="good", pool_bytes=1 << 20, page_bytes=4096, reads=FAKE, n=3, per_read=FAKE, total=FAKE):
    vp = ctypes.c_void_p
    clone = _good_clone() if isinstance(clone, str) else clone
    return L.cc_clone_check_reads_dev(pool_bytes, page_bytes, vp(reads), n,
                                      ctypes.byref(clone) if clone is not None else None, vp(per_read), vp(total),
                                      None)


def _bad_clones():
    out = [None]
    for field in ("d_clone_slot", "d_bitmap", "d_claim"):
        c = _good_clone()
        setattr(c, field, None)
        out.append(c)
    for cb in (96 << 10, (64 << 10) + 256, 0):                  # does not divide the pool; no page multiple; zero
        c = _good_clone()
        c.chunk_bytes = cb
        out.append(c)
    return out


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    E = _lib.CC_EINVAL
    for call in (_paste, _mark, _check):
        for pb in (0, 100, 128, 1000, 3 * 256, 16384):           # not 256 * 2^k, k = 0..5
            assert call(L, page_bytes=pb) == E, (call.__name__, pb)
        assert call(L, pool_bytes=(1 << 20) + 256) == E          # not whole 4 KiB pages
        assert call(L, n=1 << 31) == E
        for k, c in enumerate(_bad_clones()):
            assert call(L, c) == E, (call.__name__, k)
        assert call(L, n=0) == _lib.CC_OK                        # an empty batch is a no-op
    assert _paste(L, pool=FAKE + 2) == E and _paste(L, src=FAKE + 1) == E   # misaligned pool / source
    for name in ("pool", "src", "pastes", "crcs", "per_entry"):
        assert _paste(L, **{name: None}) == E, name
    assert _mark(L, log=None) == E and _mark(L, max_len=0) == E
    for name in ("reads", "per_read", "total"):
        assert _check(L, **{name: None}) == E, name
    c = _good_clone()
    c.d_pasted = None                                            # optional
    assert _paste(L, c, n=0) == _lib.CC_OK


def test_well_formed_calls_need_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    N = _lib.CC_ENODEV
    for call in (_paste, _mark, _check):
        assert call(L) == N
        assert call(L, n=(1 << 31) - 1) == N
        for pb in (256, 512, 1024, 2048, 4096, 8192):
            assert call(L, page_bytes=pb) == N, (call.__name__, pb)
        c = _good_clone()
        c.n_slots = 0
        assert call(L, c) == N
    c = _good_clone()
    c.d_pasted = None
    assert _paste(L, c) == N
    assert _paste(L, src_bytes=0) == N                           # every entry invalid: still a device call
