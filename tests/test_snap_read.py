"""Snapshot reads on the device (cc_read_snap_dev): everything that needs no GPU.

The numpy model of the call (snap_read_model, page by page) lives here and is
checked against a per-request restatement of CSChunkFile::ReadSpecifiedChunk
(chunkserver_chunkfile.cpp:550-636: Divide() the request's blocks into maximal
copied and uncopied runs, read the uncopied runs from the chunk, then the
copied runs from the snapshot); the GPU tests (test_snap_read_gpu.py) lean on
the model, never on the code under test.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_log_cow import NO_SNAPSHOT, SENT_BYTE, cow_model, fresh_slots

U32_MAX = 0xFFFFFFFF


# --------------------------------------------------------------------------- model
def read_valid(off, ln, oo, pool_bytes, out_bytes, page_bytes):
    """The call's contract per read (include/curve_crc.h).  out_bytes None: verify only."""
    if ln == 0:
        return True
    if off % page_bytes or ln % page_bytes:
        return False
    if off >= pool_bytes or ln > pool_bytes - off:
        return False
    if out_bytes is not None and (oo % 4 or oo > out_bytes or ln > out_bytes - oo):
        return False
    return True


def page_source(p, snap_slot, n_slots, bitmap, ppc):
    """(slot, page in chunk) when pool page p is read from its chunk's snapshot slot, else None."""
    c, q = divmod(p, ppc)
    if snap_slot is None:
        return None
    s = int(snap_slot[c])
    if s < n_slots and (int(bitmap[s, q // 32]) >> (q % 32)) & 1:
        return s, q
    return None


def snap_read_model(pool, page_crcs, snap, snap_crcs, bitmap, snap_slot, n_slots, reads, out_off, out_bytes,
                    page_bytes, chunk_bytes, crc_fn=None, out=None):
    """One cc_read_snap_dev call on host arrays, page by page.  reads = [(off,
    len)]; out_off None (with out_bytes None): verify only.  snap_slot None:
    cow == NULL.  crc_fn(bytes) -> CRC32C; None: nothing is counted (bytes
    only).  `out`: the output buffer as it was before the call (default:
    SENT_BYTE everywhere).  Returns (out or None, bad_per_read uint32, total)."""
    pb = page_bytes
    ppc = chunk_bytes // pb if chunk_bytes else 1
    n = len(reads)
    bad = np.zeros(n, np.uint32)
    if out_bytes is not None and out is None:
        out = np.full(out_bytes, SENT_BYTE, np.uint8)
    total = 0
    mism = {}  # source page -> its bytes disagree with its stored CRC (hashed once per source page)
    for i, (off, ln) in enumerate(reads):
        off, ln = int(off), int(ln)
        oo = int(out_off[i]) if out_off is not None else 0
        if not read_valid(off, ln, oo, pool.size, out_bytes, pb):
            bad[i] = U32_MAX
            continue
        for p in range(off // pb, (off + ln) // pb):
            src = page_source(p, snap_slot, n_slots, bitmap, ppc)
            if src is None:
                data, want = pool[p * pb:(p + 1) * pb], page_crcs[p]
            else:
                s, q = src
                data, want = snap[s, q * pb:(q + 1) * pb], snap_crcs[s, q]
            key = p if src is None else ("snap", src)
            if crc_fn is not None and key not in mism:
                mism[key] = crc_fn(data) != int(want)
            if crc_fn is not None and mism[key]:
                bad[i] += 1
                total += 1
            if out is not None:
                at = oo + p * pb - off
                out[at:at + pb] = data
    return out, bad, total


def bit_runs(bitmap_row, begin, end):
    """Bitmap::Divide(begin, end, &clear, &set): the maximal runs of clear and of
    set bits in [begin, end], each as inclusive (first, last)."""
    clear, held = [], []
    k = begin
    while k <= end:
        v = (int(bitmap_row[k // 32]) >> (k % 32)) & 1
        j = k
        while j + 1 <= end and ((int(bitmap_row[(j + 1) // 32]) >> ((j + 1) % 32)) & 1) == v:
            j += 1
        (held if v else clear).append((k, j))
        k = j + 1
    return clear, held


def replay_reference(pool, snap, bitmap, snap_slot, n_slots, chunk, off, ln, page_bytes, chunk_bytes):
    """CSChunkFile::ReadSpecifiedChunk(sn, buf, offset, length) for one request
    on chunk `chunk` (offset / length relative to the chunk, block-aligned):
    without a snapshot (sn == the chunk's sn) readData; with one, Divide the
    blocks [offset / blockSize, (offset + length - 1) / blockSize], read every
    uncopied run from the chunk and then every copied run from the snapshot, each
    at buf + (run start - offset).  Returns buf."""
    pb = page_bytes
    assert off % pb == 0 and ln % pb == 0 and ln > 0 and off + ln <= chunk_bytes  # CheckOffsetAndLength
    buf = np.zeros(ln, np.uint8)
    base = chunk * chunk_bytes
    s = int(snap_slot[chunk])
    if s >= n_slots:
        buf[:] = pool[base + off:base + off + ln]
        return buf
    uncopied, copied = bit_runs(bitmap[s], off // pb, (off + ln - 1) // pb)
    for b, e in uncopied:
        ro, rs = b * pb, (e - b + 1) * pb
        buf[ro - off:ro - off + rs] = pool[base + ro:base + ro + rs]
    for b, e in copied:
        ro, rs = b * pb, (e - b + 1) * pb
        buf[ro - off:ro - off + rs] = snap[s, ro:ro + rs]
    return buf


def cut_per_chunk(reads, chunk_bytes):
    """Pool reads cut at chunk boundaries: [(read index, chunk, off in chunk, len, offset in the read)]."""
    out = []
    for i, (off, ln) in enumerate(reads):
        pos = off
        while pos < off + ln:
            c = pos // chunk_bytes
            end = min(off + ln, (c + 1) * chunk_bytes)
            out.append((i, c, pos - c * chunk_bytes, end - pos, pos - off))
            pos = end
    return out


def packed_offsets(lens, gap=0):
    offs, at = [], 0
    for ln in lens:
        offs.append(at)
        at += int(ln) + gap
    return np.array(offs, np.uint64), at


BITMAP_CASES = ["random", "all_set", "all_clear", "alternating", "last_word_only"]


def make_bitmaps(kind, n_slots, ppc, rng):
    bm = np.zeros((n_slots, (ppc + 31) // 32), np.uint32)
    for s in range(n_slots):
        for q in range(ppc):
            on = {"random": rng.integers(0, 2), "all_set": 1, "all_clear": 0, "alternating": (q + s) & 1,
                  "last_word_only": q >= 32}[kind]
            if on:
                bm[s, q // 32] |= np.uint32(1 << (q % 32))
    return bm


@pytest.mark.parametrize("kind", BITMAP_CASES)
@pytest.mark.parametrize("ppc", [40, 32, 5])
def test_model_equals_per_request_replay(kind, ppc):
    """snap_read_model's bytes == ReadSpecifiedChunk's, request by request, on
    random page-aligned reads cut per chunk: random, all-set, all-clear and
    alternating bitmaps, and pages_per_chunk = 40 (the second bitmap word
    partial), with slotted, unslotted and out-of-range chunks."""
    pb, n_slots = 256, 3
    cb = ppc * pb
    slot = np.array([0, NO_SNAPSHOT, 2, 7, 1, NO_SNAPSHOT], np.uint32)
    rng = np.random.default_rng(ppc * 10 + len(kind))
    pool = rng.integers(0, 256, slot.size * cb, dtype=np.uint8)
    snap = rng.integers(0, 256, (n_slots, cb), dtype=np.uint8)
    bm = make_bitmaps(kind, n_slots, ppc, rng)
    n_pages = pool.size // pb
    reads = []
    for _ in range(120):
        p0 = int(rng.integers(0, n_pages))
        reads.append((p0 * pb, int(rng.integers(1, min(2 * ppc, n_pages - p0) + 1)) * pb))
    reads.append((0, pool.size))  # the whole pool in one read
    lens = [ln for _, ln in reads]
    out_off, out_bytes = packed_offsets(lens, gap=8)
    no_crcs, no_scrc = np.zeros(n_pages, np.uint32), np.zeros((n_slots, ppc), np.uint32)  # bytes only: not looked at
    out, bad, total = snap_read_model(pool, no_crcs, snap, no_scrc, bm, slot, n_slots, reads, out_off, out_bytes, pb,
                                      cb)
    assert total == 0 and not bad.any()
    covered = np.zeros(out_bytes, bool)
    for i, c, off, ln, at in cut_per_chunk(reads, cb):
        want = replay_reference(pool, snap, bm, slot, n_slots, c, off, ln, pb, cb)
        o = int(out_off[i]) + at
        assert (out[o:o + ln] == want).all(), (i, c, off, ln)
        covered[o:o + ln] = True
    assert (out[~covered] == SENT_BYTE).all() and covered.sum() == sum(lens)


def test_model_view_after_cow_batches_is_the_chunk_before_them(oracle):
    """Three cow_model batches, then the model's view of every chunk: the bytes
    from before the first batch for a slotted chunk, the live bytes for the
    others; every CRC the view checks matches (bad counts 0)."""
    pb, ppc, n_slots = 256, 40, 4
    cb = ppc * pb
    slot = np.array([0, NO_SNAPSHOT, 2, NO_SNAPSHOT, 1, 9, NO_SNAPSHOT, 3], np.uint32)
    rng = np.random.default_rng(3)
    pool = rng.integers(0, 256, slot.size * cb, dtype=np.uint8)
    orig = pool.copy()
    crcs = oracle.page_crcs(pool, pb)
    snap, scrc, bm = fresh_slots(n_slots, cb, pb)
    for n in (30, 200, 800):
        lens = rng.integers(1, 301, n).astype(np.uint32)
        dst = rng.integers(0, pool.size - 300, n).astype(np.uint64)
        src = rng.integers(0, 256, 4096, dtype=np.uint8)
        src_off = rng.integers(0, 4096 - 300, n).astype(np.uint64)
        cow_model(pool, crcs, src, dst, src_off, lens, 300, pb, cb, slot, n_slots, snap, scrc, bm)
        crcs = oracle.page_crcs(pool, pb)
    reads = [(c * cb, cb) for c in range(slot.size)]
    out_off, out_bytes = packed_offsets([cb] * slot.size)
    out, bad, total = snap_read_model(pool, crcs, snap, scrc, bm, slot, n_slots, reads, out_off, out_bytes, pb, cb,
                                      crc_fn=lambda b: oracle.crc32c(b.tobytes()))
    assert total == 0 and not bad.any()
    for c, s in enumerate(slot):
        want = orig if s < n_slots else pool
        assert (out[c * cb:(c + 1) * cb] == want[c * cb:(c + 1) * cb]).all(), c
    assert (pool != orig).any()
    # cow == NULL: the live bytes, whatever the slots hold
    out, bad, total = snap_read_model(pool, crcs, snap, scrc, bm, None, 0, reads, out_off, out_bytes, pb, cb,
                                      crc_fn=lambda b: oracle.crc32c(b.tobytes()))
    assert (out == pool).all() and total == 0


def test_model_marks_invalid_reads_and_counts_mismatches(oracle):
    pb, ppc = 256, 5
    cb = ppc * pb
    slot = np.array([0, NO_SNAPSHOT], np.uint32)
    rng = np.random.default_rng(4)
    pool = rng.integers(0, 256, 2 * cb, dtype=np.uint8)
    crcs = oracle.page_crcs(pool, pb)
    snap, scrc, bm = fresh_slots(1, cb, pb)
    bm[0, 0] = 0b00100
    snap[0, 2 * pb:3 * pb] = 7
    scrc[0, 2] = oracle.crc32c(bytes([7]) * pb) ^ 1          # a wrong stored snapshot CRC
    pool[2 * pb + 9] ^= 1                                    # the shadowed live page: not part of the view
    pool[7 * pb] ^= 1                                        # a live page of the unslotted chunk
    reads = [(0, cb), (cb, cb), (128, pb), (0, 100), (2 * cb, pb), (1 << 40, pb), (0, pb), (pb, pb), (pb, 0)]
    out_off = np.array([0, cb, 2 * cb, 2 * cb, 2 * cb, 2 * cb, 2 * cb + 2, 2 * cb + pb, 0], np.uint64)
    out_bytes = 2 * cb + pb + 4                              # the last but one: 4 bytes short
    out, bad, total = snap_read_model(pool, crcs, snap, scrc, bm, slot, 1, reads, out_off, out_bytes, pb, cb,
                                      crc_fn=lambda b: oracle.crc32c(b.tobytes()))
    assert bad.tolist() == [1, 1, U32_MAX, U32_MAX, U32_MAX, U32_MAX, U32_MAX, U32_MAX, 0] and total == 2
    assert (out[2 * pb:3 * pb] == 7).all() and (out[2 * cb:] == SENT_BYTE).all()


# --------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_new_symbol():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    assert re.search(r"^int cc_read_snap_dev\(", hdr, re.M)
    assert hasattr(_lib.lib(), "cc_read_snap_dev") and "cc_read_snap_dev" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cc_read_snap_dev"][1]) == 13
    # the COW comment no longer lists snapshot reads as missing
    cow = hdr[hdr.index("Copy on write for chunks with an open snapshot"):hdr.index("#define CC_NO_SNAPSHOT")]
    not_covered = cow[cow.index("Not covered"):]
    assert "verify-on-read of snapshot reads" not in not_covered
    assert "clone chunks and Paste" in not_covered


P = 1 << 20  # a fake device pointer: never dereferenced (the checks come first, and no device is present)


def _good_cow():
    from curve_amd import _lib
    c = _lib.CcCow()
    c.chunk_bytes, c.n_slots = 64 << 10, 2
    c.d_snap_slot = c.d_snap = c.d_snap_crcs = c.d_snap_bitmap = P
    return c


def _call(L, cow=None, pool=P, pool_bytes=1 << 20, page_bytes=4096, reads=P, n=3, crcs=P, out=P, out_off=P,
          out_bytes=1 << 20, bad=P, total=P):
    vp = ctypes.c_void_p
    return L.cc_read_snap_dev(vp(pool), pool_bytes, page_bytes, vp(reads), n, vp(crcs),
                              ctypes.byref(cow) if cow is not None else None, vp(out), vp(out_off), out_bytes,
                              vp(bad), vp(total), None)


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    E = _lib.CC_EINVAL
    for pb in (0, 100, 128, 1000, 3 * 256, 16384):           # not 256 * 2^k, k = 0..5
        assert _call(L, page_bytes=pb) == E, pb
    assert _call(L, pool_bytes=(1 << 20) + 256) == E         # not whole 4 KiB pages
    assert _call(L, pool=P + 2) == E                         # misaligned pool
    for name in ("pool", "reads", "crcs", "bad", "total"):
        assert _call(L, **{name: None}) == E, name
    assert _call(L, out_off=None) == E                       # an output without its offsets
    assert _call(L, out=P + 1) == E                          # misaligned output
    assert _call(L, n=1 << 31) == E
    c = _good_cow()
    c.chunk_bytes = 96 << 10                                 # a page multiple that does not divide the pool
    assert _call(L, c) == E
    c.chunk_bytes = (64 << 10) + 256                         # not a multiple of the page
    assert _call(L, c) == E
    c.chunk_bytes = 0
    assert _call(L, c) == E
    for field in ("d_snap_slot", "d_snap", "d_snap_crcs", "d_snap_bitmap"):
        c = _good_cow()
        setattr(c, field, None)
        assert _call(L, c) == E, field
    # an empty batch is a no-op, with or without anything else
    assert _call(L, n=0) == _lib.CC_OK
    assert _call(L, _good_cow(), n=0, out=None, out_off=None) == _lib.CC_OK


def test_well_formed_call_needs_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    N = _lib.CC_ENODEV
    assert _call(L, _good_cow()) == N
    assert _call(L) == N                                     # cow == NULL
    assert _call(L, out=None, out_off=None, out_bytes=0) == N  # verify only
    assert _call(L, _good_cow(), out=None, out_off=None, n=(1 << 31) - 1) == N
    for pb in (256, 512, 1024, 2048, 4096, 8192):
        assert _call(L, page_bytes=pb) == N, pb
    c = _good_cow()
    c.d_copied = c.d_stale = None                            # ignored here
    assert _call(L, c) == N
