"""Paste batches inside the write-log queue (cc_apply_ops_dev): everything that
needs no GPU.

The call's contract is a model -- every page whose FIRST SETTER in the queue is
a paste entry is pasted up front, then the write batches run as
cc_apply_logs_cow_dev runs them -- and a claim about that model: it leaves what
the per-batch sequence (cc_apply_log*_dev + cc_clone_mark_dev, or cc_paste_dev)
leaves, except for the bytes and the CRC word of CONTESTED pages (a partial
write before the page's paste).  ops_model restates the contract on the host,
sequence_model is built on test_clone's models of the existing calls, and the
first two tests check the claim.  The GPU tests (test_apply_ops_gpu.py) lean on
these models, never on the code under test.
"""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_clone import NOT_CLONE, U32_MAX, bit, mark_model, paste_model, paste_valid, set_bit, write_model, write_valid
from test_log_queue_cow import (FAKE, _bad_clones, _bad_cows, _FakeLib, _FakeStruct, _FakeTensor, _FakeTorch, _good_clone,
                                _good_cow)

PB = 256


def crc_of(page):
    """A stand-in page CRC: the equivalence only needs SOME function of the bytes."""
    return zlib.crc32(page.tobytes())


# --------------------------------------------------------------------------- models
# A queue is a list of (kind, src, entries): kind "write" or "paste", src the batch's
# data / origin buffer (uint8), entries = [(dst, src offset, len)].
def ops_paste_valid(dst, so, ln, pool_bytes, src_bytes, pb, max_paste_len):
    """cc_apply_ops_dev's rule for a paste entry: cc_paste_dev's four, and len <= max_paste_len."""
    return paste_valid(dst, so, ln, pool_bytes, src_bytes, pb) and ln <= max_paste_len


def touched(entries, max_len, pool_bytes, pb):
    out = set()
    for d, _, ln in entries:
        if write_valid(d, ln, max_len, pool_bytes):
            out.update(range(d // pb, (d + ln - 1) // pb + 1))
    return out


def sequence_model(pool, crcs, queue, max_len, max_paste_len, slot, n_slots, bm, pb, cb, crc_fn=crc_of):
    """The per-batch sequence, in place: cc_apply_log_dev + cc_clone_mark_dev for a write
    batch, cc_paste_dev for a paste batch (an entry longer than max_paste_len is handed to
    it as an invalid one: the queue refuses it).  Returns (per-paste-batch counts, pasted)."""
    counts, total = [], 0
    for kind, src, entries in queue:
        if kind == "write":
            write_model(pool, src, entries, max_len)
            for p in touched(entries, max_len, pool.size, pb):
                crcs[p] = crc_fn(pool[p * pb:(p + 1) * pb])
            mark_model(entries, max_len, pool.size, slot, n_slots, bm, pb, cb)
        else:
            ent = [(d, s, ln) if ln <= max_paste_len else (1, s, ln) for d, s, ln in entries]   # dst 1: misaligned
            per, n = paste_model(pool, crcs, src, ent, slot, n_slots, bm, pb, cb, crc_fn)
            counts.append(per)
            total += n
    return counts, total


def ops_model(pool, crcs, queue, max_len, max_paste_len, slot, n_slots, bm, pb, cb, crc_fn=crc_of):
    """cc_apply_ops_dev's contract (include/curve_crc.h), in place.  Returns (per-paste-batch
    counts, pasted, contested pairs, contested pages)."""
    ppc = cb // pb

    def open_page(p):                        # a page of a clone chunk whose bit is clear BEFORE the queue
        c, q = divmod(p, ppc)
        s = int(slot[c])
        return s < n_slots and not bit(bm0, s, q)

    bm0 = bm.copy()
    first = {}                               # page -> (ordinal, batch, entry) of its first setter; entry None: a write
    ordinal = 0
    for b, (kind, src, entries) in enumerate(queue):
        for i, (d, so, ln) in enumerate(entries):
            if kind == "paste":
                if ops_paste_valid(d, so, ln, pool.size, src.size, pb, max_paste_len):
                    for p in range(d // pb, (d + ln) // pb):
                        if open_page(p):
                            first.setdefault(p, (ordinal, b, i))
            elif write_valid(d, ln, max_len, pool.size):
                for p in range(-(-d // pb), (d + ln) // pb):          # covered whole
                    if open_page(p):
                        first.setdefault(p, (ordinal, b, None))
            ordinal += 1
    counts = []
    for kind, src, entries in queue:
        if kind == "paste":
            counts.append(np.array([0 if ops_paste_valid(d, so, ln, pool.size, src.size, pb, max_paste_len) else U32_MAX
                                    for d, so, ln in entries], np.uint32))
    which = {}                               # paste batch -> its index among the paste batches
    for b, (kind, _, _) in enumerate(queue):
        if kind == "paste":
            which[b] = len(which)
    pasted = 0
    for p, (_, b, i) in first.items():       # 1. the pastes, before the queue's first write
        if i is None:
            continue
        _, src, entries = queue[b]
        d, so, _ = entries[i]
        at = so + p * pb - d
        pool[p * pb:(p + 1) * pb] = src[at:at + pb]
        crcs[p] = crc_fn(pool[p * pb:(p + 1) * pb])
        c, q = divmod(p, ppc)
        set_bit(bm, int(slot[c]), q)
        counts[which[b]][i] += 1
        pasted += 1
    contested, pages = 0, set()
    ordinal = 0
    for kind, src, entries in queue:
        for d, so, ln in entries:
            if kind == "write" and write_valid(d, ln, max_len, pool.size):
                for p in range(d // pb, (d + ln - 1) // pb + 1):
                    whole = p * pb >= d and (p + 1) * pb <= d + ln
                    f = first.get(p)
                    if not whole and f is not None and f[2] is not None and f[0] > ordinal:
                        contested += 1
                        pages.add(p)
            ordinal += 1
    for kind, src, entries in queue:         # 2. the write batches, as cc_apply_logs_cow_dev(clone) runs them
        if kind == "write":
            write_model(pool, src, entries, max_len)
            for p in touched(entries, max_len, pool.size, pb):
                crcs[p] = crc_fn(pool[p * pb:(p + 1) * pb])
            mark_model(entries, max_len, pool.size, slot, n_slots, bm, pb, cb)
    return counts, pasted, contested, pages


def lazy_clone_page(p, pool0, queue, max_len, max_paste_len, slot, n_slots, bm0, pb, cb):
    """Page p as a lazy clone should hold it, worked out from the records alone: the origin
    bytes of the first valid paste entry covering it, with every valid write of the queue
    applied on top in order."""
    page = None
    for kind, src, entries in queue:
        for d, so, ln in entries:
            if kind == "paste" and page is None and ln and d <= p * pb < d + ln and \
                    ops_paste_valid(d, so, ln, pool0.size, src.size, pb, max_paste_len):
                page = src[so + p * pb - d:so + p * pb - d + pb].copy()
    assert page is not None
    for kind, src, entries in queue:
        for d, so, ln in entries:
            if kind == "write" and write_valid(d, ln, max_len, pool0.size):
                lo, hi = max(d, p * pb), min(d + ln, (p + 1) * pb)
                if lo < hi:
                    page[lo - p * pb:hi - p * pb] = src[so + lo - d:so + hi - d]
    return page


SLOT = np.array([0, NOT_CLONE, 7, 1], np.uint32)   # chunk 1: no clone; chunk 2: out of range for n_slots = 2
N_SLOTS = 2
SRC_BYTES = 96 * PB


def make_queue(rng, ppc, aligned, max_len, max_paste_len):
    """Four chunks (clone, not a clone, out-of-range slot, clone).  Every queue holds: a whole
    write of a page BEFORE a paste of it and a whole write AFTER a paste of another; pastes
    overlapping within a batch and across batches; entries crossing chunk boundaries; every
    kind of invalid entry; random batches of both kinds around them."""
    cb = ppc * PB
    pool_bytes = SLOT.size * cb
    n_pages = pool_bytes // PB

    def src():
        return rng.integers(0, 256, SRC_BYTES, dtype=np.uint8)

    def write_entry():
        if aligned:
            ln = int(rng.integers(1, max_len // PB + 1)) * PB
            d = int(rng.integers(0, n_pages - ln // PB + 1)) * PB
        else:
            ln = int(rng.integers(1, max_len + 1))
            d = int(rng.integers(0, pool_bytes - ln + 1))
        return (d, int(rng.integers(0, SRC_BYTES - max_len)), ln)

    def paste_entry():
        n = int(rng.integers(0, max_paste_len // PB + 1))
        d = int(rng.integers(0, n_pages - n + 1)) * PB
        return (d, int(rng.integers(0, SRC_BYTES // 4 - n * PB // 4 + 1)) * 4, n * PB)

    h1, h2 = 3 * ppc + 1, 3 * ppc + 3                 # two pages of chunk 3 (slot 1)
    bad_w = [(5 * PB, 0, 0), (PB, 0, max_len + 1), (pool_bytes - PB, 0, 2 * PB), (1 << 40, 0, PB), (pool_bytes, 0, 1)]
    bad_p = [(PB + 128, 0, PB), (2 * PB, 0, PB + 4), (pool_bytes - PB, 0, 2 * PB), (pool_bytes, 0, PB), (0, 2, PB),
             (0, SRC_BYTES - PB + 4, PB), (0, SRC_BYTES + 4, PB), (0, 0, max_paste_len + PB)]
    core = [
        ("write", src(), [(h1 * PB, 0, PB)] + bad_w[:2]),
        ("paste", src(), [(h1 * PB, 0, 3 * PB), (h2 * PB, 8 * PB, PB), (h1 * PB, 16 * PB, 2 * PB)] + bad_p[:3]),
        ("write", src(), [(h2 * PB, PB, PB), (cb - PB, 0, 2 * PB if max_len >= 2 * PB else PB)] + bad_w[2:4]),
        # crossing clone | non-clone (0 | 1), non-clone | out of range (1 | 2), out of range | clone (2 | 3)
        ("paste", src(), [(cb - 2 * PB, 0, 4 * PB), (2 * cb - PB, 4 * PB, 2 * PB), (3 * cb - 2 * PB, 8 * PB, 4 * PB),
                          (h1 * PB, 24 * PB, 3 * PB)] + bad_p[3:6]),
        ("paste", src(), [(0, 0, 0), (3 * cb, 32 * PB, 4 * PB)] + bad_p[6:]),
        ("write", src(), [bad_w[4]]),
    ]
    queue = []
    for item in core:
        for _ in range(int(rng.integers(0, 2))):      # 0 or 1 random batches before each fixed one
            kind = "write" if rng.integers(0, 2) else "paste"
            n = int(rng.integers(0, 8))
            queue.append((kind, src(), [write_entry() if kind == "write" else paste_entry() for _ in range(n)]))
        kind, s, entries = item
        extra = [write_entry() if kind == "write" else paste_entry() for _ in range(int(rng.integers(0, 5)))]
        queue.append((kind, s, extra + entries))
    return queue, pool_bytes, cb


def fresh_state(rng, ppc, pool_bytes):
    pool = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
    crcs = np.array([crc_of(pool[p * PB:(p + 1) * PB]) for p in range(pool_bytes // PB)], np.uint32)
    bm = np.zeros((N_SLOTS, (ppc + 31) // 32), np.uint32)
    for s in range(N_SLOTS):                          # preset bits, inside the slot's pages only
        for q in rng.choice(ppc, size=ppc // 3, replace=False):
            set_bit(bm, s, int(q))
    return pool, crcs, bm


def run_both(seed, ppc, aligned):
    rng = np.random.default_rng(7919 * ppc + seed + (0 if aligned else 10 ** 6))
    max_len = int(rng.choice([PB, 3 * PB])) if aligned else int(rng.choice([PB, 3 * PB + 7, 40]))
    max_paste_len = 6 * PB
    queue, pool_bytes, cb = make_queue(rng, ppc, aligned, max_len, max_paste_len)
    pool0, crcs0, bm0 = fresh_state(rng, ppc, pool_bytes)
    a = [x.copy() for x in (pool0, crcs0, bm0)]
    b = [x.copy() for x in (pool0, crcs0, bm0)]
    seq = sequence_model(a[0], a[1], queue, max_len, max_paste_len, SLOT, N_SLOTS, a[2], PB, cb)
    ops = ops_model(b[0], b[1], queue, max_len, max_paste_len, SLOT, N_SLOTS, b[2], PB, cb)
    return queue, (pool0, crcs0, bm0), a, b, seq, ops, (max_len, max_paste_len, cb)


@pytest.mark.parametrize("ppc", [5, 8, 40])
def test_aligned_queues_equal_the_sequence_bit_for_bit(ppc):
    """70 seeded queues a chunk size (210 in all) of page-aligned writes: pool, CRC table,
    bitmaps, every per-entry count and the total equal the per-batch sequence's; no
    contested pair."""
    pasted = invalid = 0
    for seed in range(70):
        queue, _, a, b, (cnt_a, tot_a), (cnt_b, tot_b, contested, pages), _ = run_both(seed, ppc, True)
        assert contested == 0 and not pages, seed
        for name, x, y in zip(("pool", "crcs", "bitmap"), a, b):
            assert (x == y).all(), (seed, name)
        assert tot_a == tot_b and len(cnt_a) == len(cnt_b), seed
        for x, y in zip(cnt_a, cnt_b):
            assert (x == y).all(), seed
        if ppc % 32:                                  # no bit past the chunk's pages
            assert not (b[2][:, -1] >> np.uint32(ppc % 32)).any()
        pasted += tot_b
        invalid += sum(int((c == U32_MAX).sum()) for c in cnt_b)
    assert pasted > 200 and invalid >= 8 * 70         # the queues did paste, and held every invalid kind


@pytest.mark.parametrize("ppc", [5, 8, 40])
def test_unaligned_queues_differ_on_contested_pages_only(ppc):
    """70 seeded queues a chunk size (210 in all) of writes of any alignment: bitmaps and
    counts always equal the sequence's; pool and CRC table differ on contested pages at
    most; every contested page holds its origin bytes with the queue's writes on top."""
    n_contested = n_differ = 0
    for seed in range(70):
        queue, (pool0, _, bm0), a, b, (cnt_a, tot_a), (cnt_b, tot_b, contested, pages), (max_len, mpl, cb) = \
            run_both(seed, ppc, False)
        assert (a[2] == b[2]).all(), seed
        assert tot_a == tot_b and all((x == y).all() for x, y in zip(cnt_a, cnt_b)), seed
        assert (contested == 0) == (not pages) and contested >= len(pages), seed
        differ = {int(p) for p in np.nonzero((a[0] != b[0]).reshape(-1, PB).any(axis=1))[0]}
        differ |= {int(p) for p in np.nonzero(a[1] != b[1])[0]}
        assert differ <= pages, (seed, sorted(differ - pages))
        for p in pages:
            want = lazy_clone_page(p, pool0, queue, max_len, mpl, SLOT, N_SLOTS, bm0, PB, cb)
            assert (b[0][p * PB:(p + 1) * PB] == want).all(), (seed, p)
            assert int(b[1][p]) == crc_of(want), (seed, p)
        n_contested += contested
        n_differ += len(differ)
    assert n_contested > 10 and n_differ > 5          # the case did occur, and did change bytes


def test_hand_made_contested_queue():
    """One page, by hand: a partial write (ordinal 0), then a paste of the page (ordinal 1),
    then another partial write.  The sequence buries the first write under the paste; the
    model keeps it on the origin bytes; one contested pair; bit and count agree."""
    cb, ppc = 5 * PB, 5
    slot = np.array([0], np.uint32)
    ws, ps = np.full(64, 0xAA, np.uint8), np.arange(PB, dtype=np.uint8)
    queue = [("write", ws, [(PB + 10, 0, 20)]), ("paste", ps, [(PB, 0, PB)]), ("write", ws, [(PB + 100, 0, 8)])]
    out = []
    for fn in (sequence_model, ops_model):
        pool, bm = np.zeros(cb, np.uint8), np.zeros((1, 1), np.uint32)
        crcs = np.array([crc_of(pool[p * PB:(p + 1) * PB]) for p in range(ppc)], np.uint32)
        out.append((fn(pool, crcs, queue, 64, PB, slot, 1, bm, PB, cb), pool, crcs, bm))
    (seq, pool_a, _, bm_a), (ops, pool_b, crcs_b, bm_b) = out
    assert int(bm_a[0, 0]) == int(bm_b[0, 0]) == 2 and seq[1] == ops[1] == 1 and int(ops[0][0][0]) == 1
    assert ops[2] == 1 and ops[3] == {1}
    want = ps.copy()
    want[100:108] = 0xAA
    assert (pool_a[PB:2 * PB] == want).all()          # the sequence: the first write is gone
    want[10:30] = 0xAA
    assert (pool_b[PB:2 * PB] == want).all() and int(crcs_b[1]) == crc_of(want)


# --------------------------------------------------------------------------- ABI
def test_header_declares_library_exports_and_lib_has_the_prototype():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    L = _lib.lib()
    name = "cc_apply_ops_dev"
    assert re.search(r"^int %s\(" % name, hdr, re.M)
    assert hasattr(L, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    assert res is ctypes.c_int
    assert args == [vp, u64, u32, vp, u32, u32, u32, vp, ctypes.c_int, vp, u64, vp, ctypes.POINTER(_lib.CcCow),
                    ctypes.POINTER(_lib.CcClone), vp]
    m = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S)
    assert re.sub(r"/\*.*?\*/", "", m.group(1)).count(",") == len(args) - 1
    assert re.search(r"const cc_cow\* cow, const cc_clone\* clone,\s*uint64_t\* d_contested", m.group(1))
    # the struct: the header's fields, in order, at C's offsets
    body = re.search(r"typedef struct cc_op_batch \{(.*?)\} cc_op_batch;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.CcOpBatch._fields_]
    assert fields == ["kind", "reserved", "d_src", "src_bytes", "d_recs", "n", "d_pasted_per_entry"]
    assert ctypes.sizeof(_lib.CcOpBatch) == 48
    assert [getattr(_lib.CcOpBatch, f).offset for f in fields] == [0, 4, 8, 16, 24, 32, 40]
    assert re.search(r"#define CC_OP_WRITE 0u", hdr) and re.search(r"#define CC_OP_PASTE 1u", hdr)
    assert (_lib.CC_OP_WRITE, _lib.CC_OP_PASTE) == (0, 1)


W, P = 0, 1


def _ops(items=((W, 3), (P, 5), (W, 0), (P, 0), (W, 70)), src=FAKE, recs=FAKE, per=FAKE, src_bytes=1 << 20):
    from curve_amd import _lib
    arr = (_lib.CcOpBatch * max(len(items), 1))()
    for k, (kind, n) in enumerate(items):
        arr[k].kind, arr[k].n = kind, n
        arr[k].d_src, arr[k].d_recs, arr[k].src_bytes = src, recs, src_bytes
        arr[k].d_pasted_per_entry = per if kind == P else None
    return arr


def _call(L, cow="good", clone="good", ops=None, n_ops=None, pool=FAKE, pool_bytes=1 << 20, page_bytes=4096,
          max_len=4096, max_paste_len=128 << 10, crcs=FAKE, work=FAKE, work_bytes=1 << 40, null_ops=False,
          contested=FAKE):
    vp = ctypes.c_void_p
    cow = _good_cow() if isinstance(cow, str) else cow
    clone = _good_clone() if isinstance(clone, str) else clone
    ops = _ops() if ops is None else ops
    n_ops = len(ops) if n_ops is None else n_ops
    return L.cc_apply_ops_dev(vp(pool), pool_bytes, page_bytes, None if null_ops else ctypes.cast(ops, vp), n_ops,
                              max_len, max_paste_len, vp(crcs), 0, vp(work), work_bytes, None,
                              ctypes.byref(cow) if cow is not None else None,
                              ctypes.byref(clone) if clone is not None else None, vp(contested))


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    E, OK = _lib.CC_EINVAL, _lib.CC_OK
    # cc_apply_logs_cow_dev's checks on the write side
    for pb in (0, 100, 128, 1000, 3 * 256, 16384):
        assert _call(L, page_bytes=pb) == E, pb
    assert _call(L, null_ops=True) == E
    for name in ("pool", "crcs", "work"):
        assert _call(L, **{name: None}) == E, name
    assert _call(L, max_len=0) == E
    assert _call(L, pool_bytes=(1 << 20) + 256) == E
    assert _call(L, pool=FAKE + 2) == E
    assert _call(L, page_bytes=256, max_len=256, max_paste_len=256, pool_bytes=256 << 32) == E
    need = int(L.cc_apply_logs_work_bytes(70, 4096, 4096))
    assert need > 0 and _call(L, work_bytes=need - 1) == E
    for k, c in enumerate(_bad_cows()):
        assert _call(L, cow=c) == E, k
        assert _call(L, cow=c, n_ops=0) == E, k
        assert _call(L, cow=c, ops=_ops(((W, 0), (P, 0)))) == E, k
    for k, c in enumerate(_bad_clones()):
        assert _call(L, clone=c) == E, k
        assert _call(L, clone=c, n_ops=0) == E, k
        assert _call(L, clone=c, ops=_ops(((P, 4),))) == E, k
    # the batch pointers: a write batch's, a paste batch's (cc_paste_dev's checks)
    for items in (((W, 3),), ((P, 3),), ((W, 3), (P, 3))):
        assert _call(L, ops=_ops(items, recs=None)) == E, items
        assert _call(L, ops=_ops(items, src=None)) == E, items
        assert _call(L, ops=_ops(items, src=FAKE + 1)) == E, items
    assert _call(L, ops=_ops(((P, 3),), per=None)) == E
    for name in ("pool", "crcs"):                                # also with nothing but pastes
        assert _call(L, ops=_ops(((P, 3),)), **{name: None}) == E, name
    assert _call(L, ops=_ops(((P, 3),)), pool=FAKE + 2) == E
    assert _call(L, ops=_ops(((P, 3),)), pool_bytes=(1 << 20) + 256) == E
    # clone is required as soon as one paste batch is non-empty
    assert _call(L, clone=None) == E
    assert _call(L, clone=None, ops=_ops(((P, 1),))) == E
    assert _call(L, cow=None, clone=None, ops=_ops(((W, 3), (P, 0))), n_ops=0) == OK
    # kind and reserved
    for kind in (2, 7, 0xFFFFFFFF):
        assert _call(L, ops=_ops(((W, 3), (kind, 3)))) == E, kind
        assert _call(L, ops=_ops(((kind, 0),))) == E, kind       # an empty batch of no kind too
    bad = _ops()
    bad[1].reserved = 1
    assert _call(L, ops=bad) == E
    bad = _ops(((W, 0),))
    bad[0].reserved = 1
    assert _call(L, ops=bad) == E
    # max_paste_len: non-zero and whole pages, when a paste batch is non-empty
    for mpl in (0, 100, 4096 + 256, 0xFFFFFFFF):
        assert _call(L, max_paste_len=mpl) == E, mpl
    # ordinals live in d_claim: all entries together below 2^31 - 1
    assert _call(L, ops=_ops(((W, 70), (P, (1 << 31) - 1 - 70)))) == E
    assert _call(L, ops=_ops(((P, 1 << 31),))) == E
    assert _call(L, ops=_ops(((P, 1 << 30), (P, 1 << 30)))) == E
    assert _call(L, ops=_ops(((P, 1 << 27),)), max_paste_len=128 << 10) == E   # 2^27 x 32 pairs: not in 32 bits
    # empty queues are no-ops, with any struct or none
    for cow in ("good", None):
        for clone in ("good", None):
            assert _call(L, cow, clone, n_ops=0) == OK
            assert _call(L, cow, clone, n_ops=0, null_ops=True) == OK
            assert _call(L, cow, clone, ops=_ops(((W, 0), (P, 0), (W, 0)))) == OK
            assert _call(L, cow, clone, ops=_ops(((P, 0),)), max_paste_len=0, pool=None, crcs=None, work=None) == OK


def test_well_formed_call_needs_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    N = _lib.CC_ENODEV
    for cow in ("good", None):
        assert _call(L, cow) == N
        assert _call(L, cow, contested=None) == N                # the counter is optional
    for pb in (256, 512, 1024, 2048, 4096, 8192):
        assert _call(L, page_bytes=pb, max_len=3 * pb + 7, max_paste_len=5 * pb) == N, pb
    assert _call(L, ops=_ops(((P, 5),)), max_len=0, work=None, work_bytes=0) == N     # pastes only: no write side
    assert _call(L, ops=_ops(((P, (1 << 27) - 1),)), max_paste_len=128 << 10) == N
    # no non-empty paste batch: cc_apply_logs_cow_dev's path, which needs neither clone nor max_paste_len
    for clone in ("good", None):
        assert _call(L, clone=clone, ops=_ops(((W, 3), (P, 0), (W, 70))), max_paste_len=0) == N
    d = _good_clone()
    d.n_slots = 0                                                # nothing slotted: still a device call
    d.d_pasted = None
    assert _call(L, clone=d) == N


# --------------------------------------------------------------------------- Python
class _FakeOpsLib(_FakeLib):
    def cc_apply_ops_dev(self, *a):
        self.calls.append(("cc_apply_ops_dev", a))
        return 0


def test_python_apply_ops_without_a_paste_item_is_apply_logs(monkeypatch):
    """crc.apply_ops with write items only reaches the symbols apply_logs reaches, with
    apply_logs' arguments: cc_apply_logs_dev without cow and clone, cc_apply_logs_cow_dev
    with either.  With a paste item it reaches cc_apply_ops_dev, one CcOpBatch an item."""
    from curve_amd import _lib
    from curve_amd import crc as C
    fake = _FakeOpsLib()
    monkeypatch.setattr(C, "lib", lambda: fake)
    monkeypatch.setattr(C, "_torch", lambda: _FakeTorch)
    monkeypatch.setattr(C, "_stream_key", lambda device, stream: (device, 0))
    monkeypatch.setattr(C, "_stream_handle", lambda stream: None)
    monkeypatch.setattr(C, "_log_work", {})
    pool, crcs, t = _FakeTensor(), _FakeTensor(1024), _FakeTensor(4096)
    writes = [("write", t, t, 70), ("write", t, t, 0), ("write", t, t, 3)]
    clone = _FakeStruct(_good_clone())
    assert C.apply_ops(pool, crcs, writes, 4096, 8192) == []
    assert C.apply_ops(pool, crcs, writes, 4096, 8192, delta=True, clone=clone) == []
    assert [c[0] for c in fake.calls] == ["cc_apply_logs_dev", "cc_apply_logs_cow_dev"]
    ref = _FakeOpsLib()
    monkeypatch.setattr(C, "lib", lambda: ref)
    C.apply_logs(pool, crcs, [w[1:] for w in writes], 4096)
    C.apply_logs(pool, crcs, [w[1:] for w in writes], 4096, delta=True, clone=clone)
    for (name_a, a), (name_b, b) in zip(fake.calls, ref.calls):
        assert name_a == name_b and len(a) == len(b)
        assert [x for x in a if isinstance(x, int)] == [x for x in b if isinstance(x, int)]
    with pytest.raises(C.CurveCrcError):
        C.apply_ops(pool, crcs, [("trim", t, t, 1)], 4096, 8192)
    assert _lib.SIGNATURES["cc_apply_ops_dev"][1][-3:-1] == [ctypes.POINTER(_lib.CcCow), ctypes.POINTER(_lib.CcClone)]


# --------------------------------------------------------------------------- code object
def test_the_built_library_holds_the_ops_kernels_for_gfx950_without_scratch(tmp_path):
    """The code object inside libcurvecrc.so, as the build left it: ops_bid_kernel,
    ops_resolve_kernel and the six ops_paste_kernel<M> are there for gfx950, none with a
    private segment (scratch) or a spilled register; only the paste kernel holds the LDS
    image.  (Resource figures only.)"""
    import shutil
    import subprocess
    from curve_amd import _lib
    llvm = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin")
    so = shutil.copy(_lib.LIB_PATH, str(tmp_path / "libcurvecrc.so"))
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], check=True, capture_output=True)
    kernels = {}
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        assert f.endswith("gfx950"), f
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", str(tmp_path / f)], check=True,
                               capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            kernels[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|"
                                                              r"vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)",
                                                              entry)}
    assert any("logs_prepass_kernel" in k for k in kernels)       # the parse sees the kernels that were there before
    new = {}
    for k, v in kernels.items():
        m = re.search(r"ops_(bid|resolve)_kernel|ops_paste_kernelILi(\d+)E", k)
        if m:
            new[m.group(1) or "paste%s" % m.group(2)] = v
    assert sorted(new) == sorted(["bid", "resolve"] + ["paste%d" % m for m in (1, 2, 4, 8, 16, 32)]), sorted(new)
    for name, v in new.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0 and \
            v.get("sgpr_spill_count", 0) == 0, (name, v)
        assert v["vgpr_count"] <= 128, (name, v)                   # 16 waves a workgroup: four a SIMD
        # the paste kernels hold the LDS image; RESOLVE one word (its workgroup's contested count)
        assert v["group_segment_fixed_size"] == (163840 if name.startswith("paste") else 4 if name == "resolve" else 0), \
            (name, v)
