"""Copy on write for the device write log (cc_apply_log_cow_dev) and the snapshot
metapage codec (cc_snap_meta_encode / cc_snap_meta_decode): everything that
needs no GPU.

The numpy model of the copy-on-write pass (cow_model) lives here and is checked
against a literal per-request replay of CSChunkFile::Write's copy2Snapshot +
writeData (chunkserver_chunkfile.cpp:381-396, :912-963); the GPU tests
(test_log_cow_gpu.py) lean on the model, never on the code under test.
"""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT

SENT_BYTE = 0xA5          # what the tests fill d_snap with
SENT_CRC = 0x5EA15EA1     # and d_snap_crcs
NO_SNAPSHOT = 0xFFFFFFFF


# --------------------------------------------------------------------------- model
def entry_ok(dst, ln, max_len, pool_bytes):
    """The write log's contract per entry (include/curve_crc.h): an entry that
    breaks it gets no piece and is skipped whole."""
    return 1 <= ln <= max_len and dst < pool_bytes and ln <= pool_bytes - dst


def cow_model(pool, page_crcs, src, dst, src_off, lens, max_len, page_bytes, chunk_bytes, snap_slot, n_slots,
              snap, snap_crcs, bitmap):
    """One cc_apply_log_cow_dev call on host arrays, in place.  pool uint8;
    page_crcs uint32 (the CRCs before the batch; NOT updated here: the tests
    take the CRCs after the batch from the oracle); snap uint8 [n_slots,
    chunk_bytes]; snap_crcs uint32 [n_slots, pages_per_chunk]; bitmap uint32
    [n_slots, ceil(pages_per_chunk / 32)].  Returns the pages copied.

    Per CALL, not per request: every page a valid entry touches whose chunk has
    a slot < n_slots and whose bit is clear is copied (old bytes, stored CRC)
    and marked BEFORE any write of the batch lands; then the log in order."""
    pool_bytes = pool.size
    ppc = chunk_bytes // page_bytes
    touched = set()
    for d, ln in zip(dst, lens):
        d, ln = int(d), int(ln)
        if entry_ok(d, ln, max_len, pool_bytes):
            touched.update(range(d // page_bytes, (d + ln - 1) // page_bytes + 1))
    copied = 0
    for p in sorted(touched):
        c, q = divmod(p, ppc)
        s = int(snap_slot[c])
        if s >= n_slots or (int(bitmap[s, q // 32]) >> (q % 32)) & 1:
            continue
        snap[s, q * page_bytes:(q + 1) * page_bytes] = pool[p * page_bytes:(p + 1) * page_bytes]
        snap_crcs[s, q] = page_crcs[p]
        bitmap[s, q // 32] |= np.uint32(1 << (q % 32))
        copied += 1
    for d, so, ln in zip(dst, src_off, lens):
        d, so, ln = int(d), int(so), int(ln)
        if entry_ok(d, ln, max_len, pool_bytes):
            pool[d:d + ln] = src[so:so + ln]
    return copied


def replay_reference(pool, page_crcs, src, dst, src_off, lens, max_len, page_bytes, chunk_bytes, snap_slot, n_slots,
                     snap, snap_crcs, bitmap, crc_fn):
    """The reference's order, literally: request by request, per chunk the
    request falls in -- needCow, then copy2Snapshot(offset, length) over the
    blocks [offset / blockSize, (offset + length - 1) / blockSize] the snapshot
    bitmap does not hold yet (read the block from the chunk as it is NOW, write
    it to the snapshot, set the bit), then writeData.  The per-page CRC table
    (ours, not the reference's) is kept current after every request, so the CRC
    a block carries into the snapshot is the one stored when it is copied."""
    ppc = chunk_bytes // page_bytes
    copied = 0
    for d, so, ln in zip(dst, src_off, lens):
        d, so, ln = int(d), int(so), int(ln)
        if not entry_ok(d, ln, max_len, pool.size):
            continue
        pos = d
        while pos < d + ln:  # one CSChunkFile::Write per chunk the entry spans
            c = pos // chunk_bytes
            end = min(d + ln, (c + 1) * chunk_bytes)
            off, length = pos - c * chunk_bytes, end - pos
            s = int(snap_slot[c])
            if s < n_slots:  # needCow
                for q in range(off // page_bytes, (off + length - 1) // page_bytes + 1):
                    if (int(bitmap[s, q // 32]) >> (q % 32)) & 1:
                        continue
                    p = c * ppc + q
                    snap[s, q * page_bytes:(q + 1) * page_bytes] = pool[p * page_bytes:(p + 1) * page_bytes]
                    snap_crcs[s, q] = page_crcs[p]
                    bitmap[s, q // 32] |= np.uint32(1 << (q % 32))
                    copied += 1
            pool[pos:end] = src[so + (pos - d):so + (end - d)]  # writeData
            for p in range(pos // page_bytes, (end - 1) // page_bytes + 1):
                page_crcs[p] = crc_fn(pool[p * page_bytes:(p + 1) * page_bytes])
            pos = end
    return copied


def fresh_slots(n_slots, chunk_bytes, page_bytes):
    ppc = chunk_bytes // page_bytes
    return (np.full((n_slots, chunk_bytes), SENT_BYTE, np.uint8), np.full((n_slots, ppc), SENT_CRC, np.uint32),
            np.zeros((n_slots, (ppc + 31) // 32), np.uint32))


def bitmap_bytes(words, bits):
    """A slot's bitmap words as the bytes SnapshotMetaPage holds."""
    return np.ascontiguousarray(words).astype("<u4").tobytes()[:(bits + 7) // 8]


HAND_LOGS = {
    # (dst, len) lists; page 256 B, 5 pages a chunk, 4 chunks: slots [0, none, out of range, 1], n_slots 2
    "overlap_and_straddle": [(10, 100), (200, 100), (250, 20), (0, 256), (1270, 20), (3900, 200), (3850, 30)],
    "same_page_many_times": [(300, 10)] * 5 + [(290, 40), (511, 2)],
    "contract_breakers": [(0, 0), (10, 257), (5110, 20), (1 << 40, 4), (600, 50)],
    "chunk_boundary": [(1279, 2), (3839, 2), (2559, 3)],
    "whole_pool": [(0, 256)] + [(256 * k, 256) for k in range(1, 20)],
}


@pytest.mark.parametrize("name", sorted(HAND_LOGS))
@pytest.mark.parametrize("preset", [False, True])
def test_model_equals_per_request_replay(oracle, name, preset):
    """cow_model (copy every touched page first, then the log) == the reference's
    request-by-request copy2Snapshot + writeData: bytes, carried CRCs, bitmaps,
    count and the pool -- on hand-made logs with overlaps, pages written many
    times, chunk-straddling entries, contract breakers and pre-set bits."""
    pb, cb, n_slots, max_len = 256, 5 * 256, 2, 256
    slot = np.array([0, NO_SNAPSHOT, 7, 1], np.uint32)
    rng = np.random.default_rng(len(name))
    pool0 = rng.integers(0, 256, 4 * cb, dtype=np.uint8)
    crcs0 = oracle.page_crcs(pool0, pb)
    log = HAND_LOGS[name]
    dst = np.array([d for d, _ in log], np.uint64)
    lens = np.array([n for _, n in log], np.uint32)
    src = rng.integers(0, 256, 4096, dtype=np.uint8)
    src_off = rng.integers(0, 4096 - 300, len(log)).astype(np.uint64)
    out = []
    for fn in (cow_model, replay_reference):
        pool, crcs = pool0.copy(), crcs0.copy()
        snap, scrc, bm = fresh_slots(n_slots, cb, pb)
        if preset:
            bm[0, 0] |= np.uint32(0b00011)   # chunk 0 pages 0, 1
            bm[1, 0] |= np.uint32(0b10000)   # chunk 3 page 4
        extra = (lambda b: oracle.crc32c(b.tobytes()),) if fn is replay_reference else ()
        n = fn(pool, crcs, src, dst, src_off, lens, max_len, pb, cb, slot, n_slots, snap, scrc, bm, *extra)
        out.append((n, pool, snap, scrc, bm))
    (n_a, pool_a, snap_a, scrc_a, bm_a), (n_b, pool_b, snap_b, scrc_b, bm_b) = out
    assert n_a == n_b
    assert (pool_a == pool_b).all() and (snap_a == snap_b).all()
    assert (scrc_a == scrc_b).all() and (bm_a == bm_b).all()
    # and the properties the GPU tests check, on the model itself
    for c, s in ((0, 0), (3, 1)):
        for q in range(5):
            p = c * 5 + q
            held = (int(bm_a[s, 0]) >> q) & 1
            was_preset = preset and ((s == 0 and q < 2) or (s == 1 and q == 4))
            if held and not was_preset:
                assert (snap_a[s, q * pb:(q + 1) * pb] == pool0[p * pb:(p + 1) * pb]).all()
                assert scrc_a[s, q] == crcs0[p]
            else:
                assert (snap_a[s, q * pb:(q + 1) * pb] == SENT_BYTE).all() and scrc_a[s, q] == SENT_CRC
                if not held:
                    assert (pool_a[p * pb:(p + 1) * pb] == pool0[p * pb:(p + 1) * pb]).all()
    if name == "contract_breakers":
        assert n_a == 1  # only (600, 50) is applied: chunk 0 page 2
        assert int(bm_a[0, 0]) == (0b100 | (0b11 if preset else 0))


# --------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_new_symbols():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    L = _lib.lib()
    for name in ("cc_apply_log_cow_dev", "cc_snap_meta_encode", "cc_snap_meta_decode"):
        assert re.search(r"^int %s\(" % name, hdr, re.M), name
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert re.search(r"#define CC_NO_SNAPSHOT 0xFFFFFFFFu", hdr)
    assert "typedef struct cc_cow" in hdr
    # the ctypes mirror has the header's layout: two u32 then six pointers
    assert ctypes.sizeof(_lib.CcCow) == 8 + 6 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.CcCow.d_snap_slot.offset == 8 and _lib.CcCow.d_stale.offset == 48
    assert _lib.CC_NO_SNAPSHOT == NO_SNAPSHOT


def _cow_call(L, cow, pool_bytes=1 << 20, page_bytes=4096, n=3):
    buf = ctypes.c_void_p(1 << 20)  # never dereferenced: the checks come first, and no device is present
    return L.cc_apply_log_cow_dev(buf, pool_bytes, page_bytes, buf, buf, n, 4096, buf, buf, 1 << 30, None, 0,
                                  ctypes.byref(cow) if cow is not None else None)


def _good_cow():
    from curve_amd import _lib
    c = _lib.CcCow()
    c.chunk_bytes, c.n_slots = 64 << 10, 2
    c.d_snap_slot = c.d_snap = c.d_snap_crcs = c.d_snap_bitmap = 1 << 20
    return c


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    c = _good_cow()
    c.chunk_bytes = 96 << 10                       # a page multiple that does not divide the 1 MiB pool
    assert _cow_call(L, c) == _lib.CC_EINVAL
    c.chunk_bytes = (64 << 10) + 256               # not a multiple of the 4 KiB page
    assert _cow_call(L, c) == _lib.CC_EINVAL
    c.chunk_bytes = 0
    assert _cow_call(L, c) == _lib.CC_EINVAL
    for field in ("d_snap_slot", "d_snap", "d_snap_crcs", "d_snap_bitmap"):
        c = _good_cow()
        setattr(c, field, None)
        assert _cow_call(L, c) == _lib.CC_EINVAL, field
    c = _good_cow()
    c.d_snap = (1 << 20) + 2                       # misaligned
    assert _cow_call(L, c) == _lib.CC_EINVAL
    assert _cow_call(L, _good_cow(), page_bytes=1000) == _lib.CC_EINVAL
    # the counters are optional, and an empty log is a no-op
    assert _cow_call(L, _good_cow(), n=0) == _lib.CC_OK


def test_well_formed_call_needs_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert _cow_call(L, _good_cow()) == _lib.CC_ENODEV
    assert _cow_call(L, None) == _lib.CC_ENODEV    # cow == NULL: cc_apply_log_dev


# --------------------------------------------------------------------------- codec
CODEC_CASES = [(1, 4096), (7, 4096), (8, 4096), (9, 4096), (128, 4096), (4096, 4096), (32768, 8192)]


@pytest.mark.parametrize("bits,page", CODEC_CASES)
def test_snap_meta_round_trip_and_layout(oracle, bits, page):
    """encode == a hand-assembled SnapshotMetaPage (version 1 | damaged | sn |
    bits | bitmap | CRC32C of those | zeros), CRC by the oracle; decode returns
    what went in."""
    from curve_amd import crc as C
    rng = np.random.default_rng(bits)
    nb = (bits + 7) // 8
    bm = rng.integers(0, 256, nb, dtype=np.uint8).tobytes()
    sn = 0x1122334455667788 ^ bits
    for damaged in (False, True):
        page_buf = C.snap_meta_encode(sn, bm, bits, page, damaged=damaged)
        head = struct.pack("<BBQI", 1, int(damaged), sn, bits) + bm
        assert len(head) == 14 + nb
        want = head + struct.pack("<I", oracle.crc32c(head))
        assert len(page_buf) == page
        assert page_buf[:len(want)] == want          # the CRC sits right behind the bitmap
        assert page_buf[len(want):] == bytes(page - len(want))
        assert C.snap_meta_decode(page_buf) == (sn, damaged, bits, bm)


def test_snap_meta_rejects_corruption_and_bad_sizes():
    from curve_amd import _lib
    from curve_amd import crc as C
    L = _lib.lib()
    bits = 4096
    bm = bytes(range(256)) * 2
    good = C.snap_meta_encode(9, bm, bits, 4096)
    for byte in (0, 1, 5, 12, 14, 14 + 511, 14 + 512, 14 + 515):  # version .. bitmap .. the CRC itself
        bad = bytearray(good)
        bad[byte] ^= 0x10
        with pytest.raises(C.CurveCrcError) as e:
            C.snap_meta_decode(bytes(bad))
        assert e.value.code == _lib.CC_ECORRUPT, byte
    # a valid CRC over another version is still refused
    v2 = bytearray(good[:14 + 512])
    v2[0] = 2
    v2 += struct.pack("<I", C.CRC32(bytes(v2)))
    with pytest.raises(C.CurveCrcError) as e:
        C.snap_meta_decode(bytes(v2) + bytes(4096 - len(v2)))
    assert e.value.code == _lib.CC_ECORRUPT
    # bits too large for the page: both ways (4096 B hold 14 + 4 + 4078 bytes of bitmap)
    out = ctypes.create_string_buffer(4096)
    big = bytes(8192)
    assert L.cc_snap_meta_encode(1, 0, 4078 * 8, big, out, 4096) == _lib.CC_OK
    assert L.cc_snap_meta_encode(1, 0, 4078 * 8 + 1, big, out, 4096) == _lib.CC_EINVAL
    assert L.cc_snap_meta_encode(1, 0, 0xFFFFFFFF, big, out, 4096) == _lib.CC_EINVAL
    huge = bytearray(good)
    huge[10:14] = struct.pack("<I", 0xFFFFFFFF)
    assert L.cc_snap_meta_decode(bytes(huge), 4096, None, None, None, None, 0) == _lib.CC_ECORRUPT
    huge[10:14] = struct.pack("<I", 4078 * 8 + 1)
    assert L.cc_snap_meta_decode(bytes(huge), 4096, None, None, None, None, 0) == _lib.CC_ECORRUPT
    # truncated buffers: shorter than the header, and cut inside the bitmap / the CRC
    for cut in (0, 13, 17, 14 + 100, 14 + 512 + 3):
        assert L.cc_snap_meta_decode(good[:cut], cut, None, None, None, None, 0) == _lib.CC_ECORRUPT, cut
    assert L.cc_snap_meta_decode(good[:14 + 512 + 4], 14 + 512 + 4, None, None, None, None, 0) == _lib.CC_OK
    # NULLs and a bitmap buffer too small for the decoded bits
    assert L.cc_snap_meta_encode(1, 0, 8, None, out, 4096) == _lib.CC_EINVAL
    assert L.cc_snap_meta_encode(1, 0, 8, big, None, 4096) == _lib.CC_EINVAL
    assert L.cc_snap_meta_decode(None, 4096, None, None, None, None, 0) == _lib.CC_EINVAL
    small = ctypes.create_string_buffer(16)
    assert L.cc_snap_meta_decode(good, 4096, None, None, None, small, 16) == _lib.CC_EINVAL


def test_snap_meta_codec_on_exact_size_buffers_under_sanitizers(tmp_path):
    """tests/native/snap_meta_bounds.cpp, a stand-alone program over integrity.cpp
    and the CPU primitive built from source with ASan/UBSan: encode into a page
    the bitmap fills to the last byte, decode of every truncation and of bits
    fields claiming more than the buffer holds -- no access past a buffer."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "snap_meta_bounds")
    csrc = os.path.join(ROOT, "curve_amd", "csrc")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-msse4.2", "-mpclmul", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(csrc, "integrity.cpp"), os.path.join(csrc, "crc32c_cpu.cpp"),
                        os.path.join(ROOT, "tests", "native", "snap_meta_bounds.cpp"), "-lpthread"],
                       capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("no AddressSanitizer runtime")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snap_meta_bounds: ok" in r.stdout


def test_slot_bitmap_words_are_the_metapage_bitmap():
    """Page q of a slot is bit q % 32 of word q / 32, which is bit q % 8 of byte
    q / 8 of the same memory (common/bitmap.h:196-199): a slot's words go into
    the metapage unchanged."""
    from curve_amd import crc as C
    ppc = 40
    words = np.zeros(2, np.uint32)
    held = [0, 7, 8, 31, 32, 39]
    for q in held:
        words[q // 32] |= np.uint32(1 << (q % 32))
    raw = bitmap_bytes(words, ppc)
    assert len(raw) == 5
    for q in range(ppc):
        assert ((raw[q // 8] >> (q % 8)) & 1) == (q in held)
    sn, damaged, bits, bm = C.snap_meta_decode(C.snap_meta_encode(3, raw, ppc))
    assert (sn, damaged, bits, bm) == (3, False, ppc, raw)
