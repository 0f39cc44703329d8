"""Scrub (cc_scrub_dev): the numpy model of the call and what can be checked
without a GPU -- the model against the models the suite already trusts
(read_merge_model for the live half, snap_read_model for the snapshot half),
hand-written cases, the argument checks through the real library, the struct
sizes, and the Python wrappers with the library faked.  test_scrub_gpu.py
runs the device against the same model."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_clone import NOT_CLONE, bit
from test_log_cow import NO_SNAPSHOT
from test_read_merge import read_merge_model
from test_snap_read import page_source, snap_read_model

SNAP = 1 << 63            # CC_SCRUB_SNAP
CRC_SENT = 0xDEADBEEF     # a table word that describes nothing: never-written pages, clear snapshot bits
BYTE_SENT = 0x5A          # the bytes of a snapshot page that does not exist
COUNTS = ("live_checked", "live_bad", "snap_checked", "snap_bad", "unwritten", "listed")


def crc_of(page):
    return zlib.crc32(bytes(page)) & 0xFFFFFFFF


# --------------------------------------------------------------------------- model
class CowState:
    """cc_cow on the host: snap_slot uint32 [chunks], snap uint8 [n_slots, chunk_bytes],
    snap_crcs uint32 [n_slots, ppc], bitmap uint32 [n_slots, words]."""

    def __init__(self, snap_slot, n_slots, snap, snap_crcs, bitmap):
        self.snap_slot, self.n_slots, self.snap, self.snap_crcs, self.bitmap = snap_slot, n_slots, snap, snap_crcs, bitmap


class CloneState:
    """cc_clone on the host: clone_slot uint32 [chunks], bitmap uint32 [n_slots, words]."""

    def __init__(self, clone_slot, n_slots, bitmap):
        self.clone_slot, self.n_slots, self.bitmap = clone_slot, n_slots, bitmap


def scrub_model(pool, page_crcs, cb, pb, cow_state, clone_state, max_list, crc_fn, counts=None):
    """One cc_scrub_dev call on host arrays, page by page (include/curve_crc.h).
    Returns (counts dict, the set of list entries of ALL mismatches -- the call
    stores the first max_list - listed-before of them in some order --, the
    per-chunk array uint32 [chunks, 2]).  `counts`: the counters before the call."""
    ppc = cb // pb
    n_pages = pool.size // pb
    n_chunks = pool.size // cb
    c = dict.fromkeys(COUNTS, 0) if counts is None else dict(counts)
    entries = set()
    per = np.zeros((n_chunks, 2), np.uint32)
    for p in range(n_pages):
        ch, q = divmod(p, ppc)
        cs = int(clone_state.clone_slot[ch]) if clone_state is not None else NOT_CLONE
        if clone_state is not None and cs < clone_state.n_slots and not bit(clone_state.bitmap, cs, q):
            c["unwritten"] += 1
            continue
        c["live_checked"] += 1
        if crc_fn(pool[p * pb:(p + 1) * pb]) != int(page_crcs[p]):
            c["live_bad"] += 1
            c["listed"] += 1
            per[ch, 0] += 1
            entries.add(p)
    if cow_state is not None:
        for p in range(n_pages):
            ch, q = divmod(p, ppc)
            s = int(cow_state.snap_slot[ch])
            if s >= cow_state.n_slots or not bit(cow_state.bitmap, s, q):
                continue
            c["snap_checked"] += 1
            if crc_fn(cow_state.snap[s, q * pb:(q + 1) * pb]) != int(cow_state.snap_crcs[s, q]):
                c["snap_bad"] += 1
                c["listed"] += 1
                per[ch, 1] += 1
                entries.add(SNAP | p)
    return c, entries, per


# --------------------------------------------------------------------------- the rig
PPC = 40                                                          # two bitmap words a slot, the second partial
CLONE_SLOTS = [0, NOT_CLONE, 2, NOT_CLONE, 1, 7, NOT_CLONE, 3]    # the suite's small rig; 7 is out of range
N_CLONE = 4
SNAP_SLOTS = [NO_SNAPSHOT, 2, NO_SNAPSHOT, 0, NO_SNAPSHOT, NO_SNAPSHOT, 9, NO_SNAPSHOT]  # 9 is out of range
N_SNAP = 3                                                        # slot 1: no chunk names it
PAGE_SIZES = [256, 512, 1024, 2048, 4096, 8192]


def random_bitmaps(rng, n_slots, ppc, density, garbage=True):
    """n_slots bitmaps with about `density` of the valid bits set; garbage in the unused bits of the last word."""
    wps = (ppc + 31) // 32
    bm = np.zeros((n_slots, wps), np.uint32)
    for s in range(n_slots):
        for q in range(ppc):
            if rng.random() < density:
                bm[s, q // 32] |= np.uint32(1 << (q % 32))
        if garbage and ppc % 32:
            bm[s, -1] |= np.uint32((int(rng.integers(1, 1 << 32)) << (ppc % 32)) & 0xFFFFFFFF)
    return bm


class HostRig:
    """A pool with clone chunks and snapshot slots whose every existing page
    matches its table word, and whose every table word and snapshot byte that
    describes nothing holds a sentinel."""

    def __init__(self, pb, seed, page_crcs_fn, ppc=PPC, clone_slots=CLONE_SLOTS, n_clone=N_CLONE,
                 snap_slots=SNAP_SLOTS, n_snap=N_SNAP, clone_density=0.3, snap_density=0.25):
        rng = np.random.default_rng(seed)
        self.pb, self.ppc, self.cb = pb, ppc, ppc * pb
        self.n_chunks = len(clone_slots)
        self.n_pages = self.n_chunks * ppc
        self.pool = rng.integers(0, 256, self.n_pages * pb, dtype=np.uint8)
        self.crcs = np.asarray(page_crcs_fn(self.pool, pb), dtype=np.uint32).copy()
        self.clone = CloneState(np.array(clone_slots, np.uint32), n_clone,
                                random_bitmaps(rng, max(n_clone, 1), ppc, clone_density))
        snap = np.full((max(n_snap, 1), self.cb), BYTE_SENT, np.uint8)
        scrc = np.full((max(n_snap, 1), ppc), CRC_SENT, np.uint32)
        sbm = random_bitmaps(rng, max(n_snap, 1), ppc, snap_density)
        self.cow = CowState(np.array(snap_slots, np.uint32), n_snap, snap, scrc, sbm)
        for ch in range(self.n_chunks):
            cs, s = int(clone_slots[ch]), int(snap_slots[ch])
            for q in range(ppc):
                if cs < n_clone and not bit(self.clone.bitmap, cs, q):
                    self.crcs[ch * ppc + q] = CRC_SENT                # never written: no CRC word
                if s < n_snap and bit(sbm, s, q):
                    snap[s, q * pb:(q + 1) * pb] = rng.integers(0, 256, pb, dtype=np.uint8)
        for s in range(n_snap):
            words = np.asarray(page_crcs_fn(snap[s], pb), dtype=np.uint32)
            for q in range(ppc):
                if bit(sbm, s, q) and s in [int(v) for v in snap_slots]:
                    scrc[s, q] = words[q]

    def model(self, crc_fn, cow=True, clone=True, max_list=1 << 20, counts=None):
        return scrub_model(self.pool, self.crcs, self.cb, self.pb, self.cow if cow else None,
                           self.clone if clone else None, max_list, crc_fn, counts=counts)

    # the page classes of the issue's table, as lists of pool pages (snapshot classes: (slot, page in chunk))
    def classes(self):
        out = {"ordinary": [], "written": [], "unwritten": [], "snap_set": [], "snap_clear": [], "unnamed": []}
        for p in range(self.n_pages):
            ch, q = divmod(p, self.ppc)
            cs, s = int(self.clone.clone_slot[ch]), int(self.cow.snap_slot[ch])
            if cs >= self.clone.n_slots:
                out["ordinary"].append(p)
            elif bit(self.clone.bitmap, cs, q):
                out["written"].append(p)
            else:
                out["unwritten"].append(p)
            if s < self.cow.n_slots:
                out["snap_set" if bit(self.cow.bitmap, s, q) else "snap_clear"].append((s, q, p))
        named = {int(v) for v in self.cow.snap_slot}
        for s in range(self.cow.n_slots):
            if s not in named:
                out["unnamed"] += [(s, q, None) for q in range(self.ppc)]
        return out


def zlib_page_crcs(buf, pb):
    return np.array([crc_of(buf[i:i + pb]) for i in range(0, buf.size, pb)], np.uint32)


def popcount_valid(bm, s, ppc):
    return sum(bit(bm, s, q) for q in range(ppc))


# --------------------------------------------------------------------------- the model against trusted models
def corrupt_some(rig, rng, n=30):
    """Flip a byte or a table word in n random places of every class, reported or not."""
    cls = rig.classes()
    for _ in range(n):
        kind = list(cls)[int(rng.integers(len(cls)))]
        if not cls[kind]:
            continue
        item = cls[kind][int(rng.integers(len(cls[kind])))]
        word = bool(rng.integers(2))
        if kind in ("ordinary", "written", "unwritten"):
            if word:
                rig.crcs[item] ^= np.uint32(1 << int(rng.integers(32)))
            else:
                rig.pool[item * rig.pb + int(rng.integers(rig.pb))] ^= np.uint8(1 << int(rng.integers(8)))
        else:
            s, q, _ = item
            if word:
                rig.cow.snap_crcs[s, q] ^= np.uint32(1 << int(rng.integers(32)))
            else:
                rig.cow.snap[s, q * rig.pb + int(rng.integers(rig.pb))] ^= np.uint8(1 << int(rng.integers(8)))


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("with_cow,with_clone", [(True, True), (True, False), (False, True), (False, False)])
def test_model_equals_the_trusted_models(seed, with_cow, with_clone):
    rig = HostRig(256, seed, zlib_page_crcs)
    corrupt_some(rig, np.random.default_rng(100 + seed))
    counts, entries, per = rig.model(crc_of, cow=with_cow, clone=with_clone)
    pb, cb, ppc = rig.pb, rig.cb, rig.ppc
    # live half: one whole-chunk read a chunk through read_merge_model, no origin
    slot = rig.clone.clone_slot if with_clone else np.full(rig.n_chunks, NOT_CLONE, np.uint32)
    reads = [(c * cb, cb) for c in range(rig.n_chunks)]
    out = np.zeros(rig.pool.size, np.uint8)
    bad, bad_total, unw, unw_total = read_merge_model(rig.pool, rig.crcs, slot, rig.clone.n_slots if with_clone else 0,
                                                      rig.clone.bitmap, reads, None, None,
                                                      [c * cb for c in range(rig.n_chunks)], out, pb, cb, crc_of)
    assert (counts["live_bad"], counts["unwritten"]) == (bad_total, unw_total)
    assert (per[:, 0] == bad).all()
    assert counts["live_checked"] + counts["unwritten"] == rig.n_pages
    assert sorted(e for e in entries if not e & SNAP) == sorted(
        p for p in range(rig.n_pages)
        if not (with_clone and int(slot[p // ppc]) < rig.clone.n_slots and not bit(rig.clone.bitmap, int(slot[p // ppc]), p % ppc))
        and crc_of(rig.pool[p * pb:(p + 1) * pb]) != int(rig.crcs[p]))
    # snapshot half: snap_read_model's verdict on every page it reads from a slot
    if not with_cow:
        assert counts["snap_checked"] == counts["snap_bad"] == 0 and not any(e & SNAP for e in entries)
        assert (per[:, 1] == 0).all()
        return
    cow = rig.cow
    one = [(p * pb, pb) for p in range(rig.n_pages)]
    _, sbad, _ = snap_read_model(rig.pool, rig.crcs, cow.snap, cow.snap_crcs, cow.bitmap, cow.snap_slot, cow.n_slots, one,
                                 None, None, pb, cb, crc_of)
    from_slot = [p for p in range(rig.n_pages) if page_source(p, cow.snap_slot, cow.n_slots, cow.bitmap, ppc)]
    assert counts["snap_checked"] == len(from_slot)
    assert {e & (SNAP - 1) for e in entries if e & SNAP} == {p for p in from_slot if sbad[p]}
    assert counts["snap_bad"] == sum(int(sbad[p]) for p in from_slot)
    assert [int(v) for v in per[:, 1]] == [sum(int(sbad[p]) for p in from_slot if p // ppc == c)
                                            for c in range(rig.n_chunks)]
    assert counts["listed"] == counts["live_bad"] + counts["snap_bad"] == len(entries)
    assert counts["live_bad"] > 0 and counts["snap_bad"] > 0           # the corruption did reach both halves


def small_case(ppc=40, n_chunks=2, pb=256):
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 256, n_chunks * ppc * pb, dtype=np.uint8)
    return pool, zlib_page_crcs(pool, pb), ppc * pb, pb


def test_model_cases_by_hand():
    pool, crcs, cb, pb = small_case()
    ppc, wps = 40, 2
    # a garbage bit at position >= ppc in the last bitmap word: clone chunk 0 with bits 0..39 clear, 40..63 set
    bm = np.zeros((1, wps), np.uint32)
    bm[0, 1] = 0xFFFFFF00
    clone = CloneState(np.array([0, NOT_CLONE], np.uint32), 1, bm)
    c, ent, per = scrub_model(pool, crcs, cb, pb, None, clone, 16, crc_of)
    assert (c["unwritten"], c["live_checked"], c["live_bad"]) == (40, 40, 0) and not ent
    # ... and in a snapshot slot: nothing is checked
    snap = np.full((2, cb), BYTE_SENT, np.uint8)
    scrc = np.full((2, ppc), CRC_SENT, np.uint32)
    sbm = np.zeros((2, wps), np.uint32)
    sbm[0, 1] = 0xFFFFFF00
    cow = CowState(np.array([0, NO_SNAPSHOT], np.uint32), 2, snap, scrc, sbm)
    c, ent, per = scrub_model(pool, crcs, cb, pb, cow, None, 16, crc_of)
    assert (c["snap_checked"], c["snap_bad"], c["live_checked"]) == (0, 0, 80) and not ent
    # a slot value >= n_slots, in both structs: an ordinary chunk with no snapshot
    sbm[:] = 0xFFFFFFFF
    cow = CowState(np.array([2, 0xFFFFFFFE], np.uint32), 2, snap, scrc, sbm)
    clone = CloneState(np.array([1, 5], np.uint32), 1, np.zeros((1, wps), np.uint32))
    c, ent, per = scrub_model(pool, crcs, cb, pb, cow, clone, 16, crc_of)
    assert (c["live_checked"], c["unwritten"], c["snap_checked"], c["listed"]) == (80, 0, 0, 0)
    # a slot no chunk names is never read, whatever its bits say: slot 1 is all sentinels, all bits set
    cow = CowState(np.array([NO_SNAPSHOT, NO_SNAPSHOT], np.uint32), 2, snap, scrc, sbm)
    c, ent, per = scrub_model(pool, crcs, cb, pb, cow, None, 16, crc_of)
    assert (c["snap_checked"], c["snap_bad"]) == (0, 0)
    # two chunks naming one slot: each is scrubbed on its own terms
    sbm[:] = 0
    sbm[0, 0] = 0b101
    for q in (0, 2):
        snap[0, q * pb:(q + 1) * pb] = pool[(ppc + q) * pb:(ppc + q + 1) * pb]
        scrc[0, q] = crcs[ppc + q]
    snap[0, 2 * pb] ^= 1
    cow = CowState(np.array([0, 0], np.uint32), 2, snap, scrc, sbm)
    c, ent, per = scrub_model(pool, crcs, cb, pb, cow, None, 16, crc_of)
    assert (c["snap_checked"], c["snap_bad"], c["listed"]) == (4, 2, 2)
    assert ent == {SNAP | 2, SNAP | (ppc + 2)} and per.tolist() == [[0, 1], [0, 1]]
    # a chunk with both a snapshot slot and a clone slot: the live pass follows the clone bitmap, the
    # snapshot pass the snapshot bitmap, independently (a never-written live page may have a snapshot copy)
    cbm = np.zeros((1, wps), np.uint32)
    cbm[0, 0] = 0b110                                    # live pages 1, 2 written; 0 and 3.. never
    clone = CloneState(np.array([0, NOT_CLONE], np.uint32), 1, cbm)
    cow = CowState(np.array([0, NO_SNAPSHOT], np.uint32), 2, snap, scrc, sbm)
    bad_pool = pool.copy()
    bad_pool[0] ^= 1                                     # never written: ignored
    bad_pool[pb] ^= 1                                    # written: reported
    c, ent, per = scrub_model(bad_pool, crcs, cb, pb, cow, clone, 16, crc_of)
    assert (c["live_checked"], c["unwritten"], c["live_bad"], c["snap_checked"], c["snap_bad"]) == (42, 38, 1, 2, 1)
    assert ent == {1, SNAP | 2} and per.tolist() == [[1, 1], [0, 0]]
    # the counters are += : a second call continues the cursor
    c2, ent2, _ = scrub_model(bad_pool, crcs, cb, pb, cow, clone, 16, crc_of, counts=c)
    assert c2["listed"] == 4 and c2["live_checked"] == 84 and ent2 == ent


def test_rig_has_every_class_at_every_named_position():
    rig = HostRig(256, 11, zlib_page_crcs)
    cls = rig.classes()
    assert all(len(v) >= 4 for v in cls.values()), {k: len(v) for k, v in cls.items()}
    c, ent, per = rig.model(crc_of)
    assert c["live_bad"] == c["snap_bad"] == c["listed"] == 0 and not ent
    assert c["live_checked"] + c["unwritten"] == rig.n_pages and c["unwritten"] == len(cls["unwritten"])
    assert c["snap_checked"] == sum(popcount_valid(rig.cow.bitmap, s, rig.ppc) for s in (0, 2))
    assert (rig.cow.bitmap[:, -1] >> np.uint32(PPC % 32)).all() and (rig.clone.bitmap[:, -1] >> np.uint32(PPC % 32)).all()


# --------------------------------------------------------------------------- ABI
def test_header_declares_library_exports_and_struct_sizes():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    L = _lib.lib()
    assert re.search(r"^int cc_scrub_dev\(", hdr, re.M)
    assert hasattr(L, "cc_scrub_dev") and "cc_scrub_dev" in _lib.SIGNATURES
    m = re.search(r"^int cc_scrub_dev\((.*?)\);", hdr, re.M | re.S)
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert args.count(",") == len(_lib.SIGNATURES["cc_scrub_dev"][1]) - 1
    assert ctypes.sizeof(_lib.CcScrubCounts) == 48 and ctypes.sizeof(_lib.CcScrubChunk) == 8
    assert [f[0] for f in _lib.CcScrubCounts._fields_] == list(COUNTS)
    assert re.search(r"#define CC_SCRUB_SNAP \(1ull << 63\)", hdr) and _lib.CC_SCRUB_SNAP == SNAP


FAKE = 1 << 20  # a fake device pointer: never dereferenced (the checks come first, and no device is present)
CB = 64 << 10


def _good_cow():
    from curve_amd import _lib
    c = _lib.CcCow()
    c.chunk_bytes, c.n_slots = CB, 2
    c.d_snap_slot = c.d_snap = c.d_snap_crcs = c.d_snap_bitmap = FAKE
    return c                                                      # d_copied, d_stale NULL: optional


def _good_clone():
    from curve_amd import _lib
    c = _lib.CcClone()
    c.chunk_bytes, c.n_slots = CB, 2
    c.d_clone_slot = c.d_bitmap = FAKE
    return c                                                      # d_claim, d_pasted NULL: never needed here


def _call(L, cow="good", clone="good", pool=FAKE, pool_bytes=1 << 20, page_bytes=4096, chunk_bytes=CB, crcs=FAKE,
          counts=FAKE, lst=FAKE, max_list=16, per=FAKE):
    vp = ctypes.c_void_p
    cow = _good_cow() if isinstance(cow, str) else cow
    clone = _good_clone() if isinstance(clone, str) else clone
    return L.cc_scrub_dev(vp(pool), pool_bytes, page_bytes, chunk_bytes, vp(crcs),
                          ctypes.byref(cow) if cow is not None else None,
                          ctypes.byref(clone) if clone is not None else None, vp(counts), vp(lst), max_list, vp(per),
                          None)


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    E, OK = _lib.CC_EINVAL, _lib.CC_OK
    structs = [("good", "good"), ("good", None), (None, "good"), (None, None)]
    for cow, clone in structs:
        for pb in (0, 100, 128, 1000, 3 * 256, 16384):            # not 256 * 2^k, k = 0..5
            assert _call(L, cow, clone, page_bytes=pb) == E, pb
        for cb in (0, CB + 256, 96 << 10):                        # zero; no page multiple; does not divide the pool
            assert _call(L, None, None, chunk_bytes=cb) == E, cb
        assert _call(L, cow, clone, pool_bytes=(1 << 20) + 4096) == E      # not whole chunks
        for name in ("pool", "crcs", "counts"):
            assert _call(L, cow, clone, **{name: None}) == E, name
        assert _call(L, cow, clone, pool=FAKE + 2) == E           # misaligned pool
        assert _call(L, cow, clone, lst=None) == E                # a non-zero max_list with a NULL list
        assert _call(L, cow, clone, lst=None, max_list=0, pool_bytes=0) == OK
        assert _call(L, cow, clone, pool_bytes=0) == OK           # an empty pool is a no-op
        assert _call(L, cow, clone, pool_bytes=0, per=None) == OK
    # pool pages must fit 32 bits
    assert _call(L, None, None, page_bytes=256, chunk_bytes=256, pool_bytes=256 << 32) == E
    assert _call(L, None, None, page_bytes=256, chunk_bytes=256, pool_bytes=0) == OK
    # the structs: a chunk size that differs, NULL pointers, a misaligned snapshot buffer
    for field in ("d_snap_slot", "d_snap", "d_snap_crcs", "d_snap_bitmap"):
        c = _good_cow()
        setattr(c, field, None)
        assert _call(L, cow=c) == E and _call(L, cow=c, clone=None) == E and _call(L, cow=c, pool_bytes=0) == E, field
    c = _good_cow()
    c.d_snap = FAKE + 2
    assert _call(L, cow=c) == E
    c = _good_cow()
    c.chunk_bytes = CB // 2                                       # a valid geometry, but not this call's
    assert _call(L, cow=c) == E and _call(L, cow=c, clone=None) == E
    for field in ("d_clone_slot", "d_bitmap"):
        c = _good_clone()
        setattr(c, field, None)
        assert _call(L, clone=c) == E and _call(L, cow=None, clone=c) == E and _call(L, clone=c, pool_bytes=0) == E, field
    c = _good_clone()
    c.chunk_bytes = CB * 2
    assert _call(L, clone=c) == E and _call(L, cow=None, clone=c) == E


def test_well_formed_call_needs_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    N = _lib.CC_ENODEV
    for cow in ("good", None):
        for clone in ("good", None):
            assert _call(L, cow, clone) == N
            assert _call(L, cow, clone, lst=None, max_list=0, per=None) == N
    for pb in (256, 512, 1024, 2048, 4096, 8192):
        assert _call(L, page_bytes=pb) == N, pb


# --------------------------------------------------------------------------- Python, the library faked
class _FakeLib:
    """A library whose cc_scrub_dev records its arguments."""

    def __init__(self):
        self.calls = []

    def cc_scrub_dev(self, *a):
        self.calls.append(a)
        return 0


class _Stub:
    """Replaces crc.scrub's device work: hands out the canned ScrubResults in order."""

    def __init__(self, results):
        self.results, self.calls = list(results), []

    def __call__(self, pool, table, chunk_bytes, cow=None, clone=None, max_bad=4096, page_bytes=4096, stream=None):
        self.calls.append((table, chunk_bytes, cow, clone, max_bad, page_bytes))
        return self.results.pop(0)


def _result(C, live=(), snap=(), unwritten=0, n_pages=80, chunks=2):
    per = np.zeros((chunks, 2), np.int32)
    for c, _ in live:
        per[c, 0] += 1
    for c, _ in snap:
        per[c, 1] += 1
    counts = (n_pages - unwritten, len(live), len(snap) + 3, len(snap), unwritten, len(live) + len(snap))
    return C.ScrubResult(counts, sorted(live), sorted(snap), per)


def _device_pool():
    """A DevicePool with nothing behind it but its geometry."""
    from curve_amd.scan import DevicePool
    p = DevicePool.__new__(DevicePool)
    p.chunk_size, p.page_bytes, p.data, p.page_crcs = 40 * 256, 256, "pool-data", "pool-crcs"
    return p


def test_scrub_raises_when_the_list_cannot_name_every_bad_page(monkeypatch):
    torch = pytest.importorskip("torch")
    from curve_amd import crc as C

    def fake_records(pool, page_crcs, chunk_bytes, counts, bad_list, bad_per_chunk=None, **kw):
        assert bad_list.numel() == 3 and counts.numel() == 6 and tuple(bad_per_chunk.shape) == (2, 2)
        counts += torch.tensor([78, 4, 5, 1, 2, 5])
        bad_list[:3] = torch.tensor([3, 41, (SNAP | 7) - (1 << 64)])
        bad_per_chunk += torch.tensor([[1, 1], [3, 0]], dtype=torch.int32)

    class CpuPool:
        device = torch.device("cpu")

        def numel(self):
            return 80 * 256

        def element_size(self):
            return 1

    monkeypatch.setattr(C, "scrub_records", fake_records)
    with pytest.raises(C.CurveCrcError) as e:
        C.scrub(CpuPool(), None, 40 * 256, max_bad=3, page_bytes=256)
    assert e.value.code == -74 and "5 bad pages" in str(e.value)     # CC_ECORRUPT, as DevicePool.bad_pages

    def fits(pool, page_crcs, chunk_bytes, counts, bad_list, bad_per_chunk=None, **kw):
        counts += torch.tensor([78, 2, 5, 1, 2, 3])
        bad_list[:3] = torch.tensor([41, (SNAP | 47) - (1 << 64), 3])
        bad_per_chunk += torch.tensor([[1, 0], [1, 1]], dtype=torch.int32)

    monkeypatch.setattr(C, "scrub_records", fits)
    r = C.scrub(CpuPool(), None, 40 * 256, max_bad=3, page_bytes=256)
    assert [getattr(r, n) for n in COUNTS] == [78, 2, 5, 1, 2, 3]
    assert r.live_bad_pages == [(0, 3), (1, 1)] and r.snap_bad_pages == [(1, 7)]
    assert r.per_chunk.tolist() == [[1, 0], [1, 1]] and not r.clean


def test_scrub_repair_sends_exactly_the_live_bad_pages(monkeypatch):
    from curve_amd import crc as C
    pool = _device_pool()
    live, snap = [(0, 3), (1, 1), (1, 39)], [(1, 7)]
    stub = _Stub([_result(C, live, snap, unwritten=9), _result(C, [(1, 39)], snap, unwritten=9)])
    sent = {}

    def fake_repair_pages(data, crcs, pages, fetchers, claim, expect=None, page_bytes=4096, stream=None):
        sent.update(pages=list(pages), fetchers=fetchers, claim=claim, expect=expect, page_bytes=page_bytes, crcs=crcs)
        return (np.array(sorted(pages), np.int64), np.array([C.REPAIR_REPAIRED, C.REPAIR_REPAIRED, C.REPAIR_FAILED], np.int8),
                np.array([0, 1, -1], np.int64))

    monkeypatch.setattr(C, "scrub", stub)
    monkeypatch.setattr(C, "repair_pages", fake_repair_pages)
    repaired, still, snap_bad = pool.scrub_repair(["f0", "f1"], cow="cow", clone="clone", claim="claim")
    assert sent["pages"] == [3, 41, 79] and sent["fetchers"] == ["f0", "f1"] and sent["claim"] == "claim"
    assert sent["expect"] == "pool-crcs" and sent["crcs"] == "pool-crcs" and sent["page_bytes"] == 256
    assert repaired == [(0, 3, 0), (1, 1, 1)] and still == [(1, 39)] and snap_bad == snap
    assert len(stub.calls) == 2 and all(c == ("pool-crcs", 40 * 256, "cow", "clone", 4096, 256) for c in stub.calls)
    # an authority's table goes to both scrubs and to the repair as `expect`
    stub = _Stub([_result(C, live, snap), _result(C, [(1, 39)], snap)])
    monkeypatch.setattr(C, "scrub", stub)
    pool.scrub_repair(["f0"], expected_page_crcs="authority", claim="claim")
    assert sent["expect"] == "authority" and sent["crcs"] == "pool-crcs" and [c[0] for c in stub.calls] == ["authority"] * 2
    # nothing live is bad: no repair, one scrub, the snapshot pages still reported
    sent.clear()
    stub = _Stub([_result(C, [], snap)])
    monkeypatch.setattr(C, "scrub", stub)
    assert pool.scrub_repair(["f0"], claim="claim") == ([], [], snap) and not sent and len(stub.calls) == 1


def test_scrub_repair_raises_when_the_second_scrub_disagrees(monkeypatch):
    from curve_amd import crc as C
    pool = _device_pool()
    live, snap = [(0, 3), (1, 1)], [(1, 7)]

    def fake_repair_pages(data, crcs, pages, *a, **kw):
        return (np.array(sorted(pages), np.int64), np.array([C.REPAIR_REPAIRED, C.REPAIR_FAILED], np.int8),
                np.array([0, -1], np.int64))

    monkeypatch.setattr(C, "repair_pages", fake_repair_pages)
    for second in (_result(C, [], snap), _result(C, live, snap), _result(C, [(1, 1)], [])):
        monkeypatch.setattr(C, "scrub", _Stub([_result(C, live, snap), second]))
        with pytest.raises(C.CurveCrcError):
            pool.scrub_repair(["f0"], claim="claim")
    monkeypatch.setattr(C, "scrub", _Stub([_result(C, live, snap), _result(C, [(1, 1)], snap)]))
    assert pool.scrub_repair(["f0"], claim="claim") == ([(0, 3, 0)], [(1, 1)], snap)


def test_scrub_records_passes_the_structs_and_the_list_size(monkeypatch):
    """crc.scrub_records reaches cc_scrub_dev with NULL for an absent struct, list or per-chunk array."""
    from curve_amd import crc as C
    from test_log_queue_cow import _FakeStruct, _FakeTensor, _FakeTorch
    fake = _FakeLib()
    monkeypatch.setattr(C, "lib", lambda: fake)
    monkeypatch.setattr(C, "_torch", lambda: _FakeTorch)
    monkeypatch.setattr(C, "_stream_handle", lambda stream: None)

    class T(_FakeTensor):
        def __init__(self, n, size):
            self.n, self.size = n, size

        def element_size(self):
            return self.size

    pool, crcs, counts, lst, per = T(1 << 20, 1), T(256, 4), T(6, 8), T(7, 8), T(32, 4)
    C.scrub_records(pool, crcs, CB, counts, lst, per, cow=_FakeStruct(_good_cow()), clone=_FakeStruct(_good_clone()),
                    page_bytes=4096)
    C.scrub_records(pool, crcs, CB, counts, None, None, page_bytes=4096)
    a, b = fake.calls
    assert len(a) == 12 and a[1:4] == (1 << 20, 4096, CB) and a[9] == 7
    assert a[5] is not None and a[6] is not None and a[8] is not None and a[10] is not None
    assert b[5] is None and b[6] is None and b[8] is None and b[9] == 0 and b[10] is None
    with pytest.raises(C.CurveCrcError):
        C.scrub_records(pool, T(255, 4), CB, counts, lst, per, page_bytes=4096)     # a short CRC table
    with pytest.raises(C.CurveCrcError):
        C.scrub_records(pool, crcs, CB, T(5, 8), lst, per, page_bytes=4096)         # five counters
    with pytest.raises(C.CurveCrcError):
        C.scrub_records(pool, crcs, CB, counts, lst, T(31, 4), page_bytes=4096)     # a short per-chunk array
