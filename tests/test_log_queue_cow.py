"""The write-log queue for pools with open snapshots and clone chunks
(cc_apply_logs_cow_dev): everything that needs no GPU.

The call's contract is an equivalence: one pass BEFORE the queue must leave
what cc_apply_log_cow_dev + cc_clone_mark_dev per batch leave.  The first test
checks that claim on host models alone -- the per-batch sequence is built on
cow_model (test_log_cow.py) and mark_model (test_clone.py), the up-front pass is
restated here -- and the GPU tests (test_log_queue_cow_gpu.py) check the code.
"""
import contextlib
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_clone import mark_model, write_valid
from test_log_cow import NO_SNAPSHOT, cow_model, entry_ok, fresh_slots

PB = 256


# --------------------------------------------------------------------------- models
def crc_of(page):
    """A stand-in page CRC: the equivalence only needs SOME function of the bytes."""
    return zlib.crc32(page.tobytes())


def touched_pages(batch, max_len, pool_bytes, pb):
    out = set()
    for d, _, ln in batch:
        if entry_ok(d, ln, max_len, pool_bytes):
            out.update(range(d // pb, (d + ln - 1) // pb + 1))
    return out


def sequence_model(pool, crcs, src, queue, max_len, pb, cb, snap_slot, n_slots, snap, scrc, bm, clone_slot, n_clone,
                   cbm):
    """cc_apply_log_cow_dev (full mode) + cc_clone_mark_dev, batch after batch, in place.
    Returns (copied, stale): stale = copies whose bytes did not match the CRC they carried."""
    copied = stale = 0
    for batch in queue:
        if not batch:
            continue
        dst = np.array([d for d, _, _ in batch], np.uint64)
        so = np.array([s for _, s, _ in batch], np.uint64)
        ln = np.array([n for _, _, n in batch], np.uint32)
        before = bm.copy()
        copied += cow_model(pool, crcs, src, dst, so, ln, max_len, pb, cb, snap_slot, n_slots, snap, scrc, bm)
        for s, w in zip(*np.nonzero(before != bm)):
            for b in range(32):
                if (int(bm[s, w]) ^ int(before[s, w])) >> b & 1:
                    q = int(w) * 32 + b
                    stale += crc_of(snap[s, q * pb:(q + 1) * pb]) != int(scrc[s, q])
        for p in touched_pages(batch, max_len, pool.size, pb):  # the page kernel: a fresh CRC per touched page
            crcs[p] = crc_of(pool[p * pb:(p + 1) * pb])
        mark_model(batch, max_len, pool.size, clone_slot, n_clone, cbm, pb, cb)
    return copied, stale


def prepass_model(pool, crcs, src, queue, max_len, pb, cb, snap_slot, n_slots, snap, scrc, bm, clone_slot, n_clone, cbm):
    """cc_apply_logs_cow_dev: ONE pass over the pairs of every batch against the pool and the
    CRC table as they stand before the queue, then the plain queue."""
    ppc = cb // pb
    copied = stale = 0
    for batch in queue:                      # pair order; any order gives the same arrays (first bid wins, same source)
        for d, _, ln in batch:
            if not write_valid(d, ln, max_len, pool.size):
                continue
            for p in range(d // pb, (d + ln - 1) // pb + 1):
                c, q = divmod(p, ppc)
                s = int(snap_slot[c])
                if s < n_slots and not (int(bm[s, q // 32]) >> (q % 32)) & 1:
                    bm[s, q // 32] |= np.uint32(1 << (q % 32))
                    snap[s, q * pb:(q + 1) * pb] = pool[p * pb:(p + 1) * pb]
                    scrc[s, q] = crcs[p]
                    copied += 1
                    stale += crc_of(pool[p * pb:(p + 1) * pb]) != int(crcs[p])
                t = int(clone_slot[c])
                if t < n_clone and p * pb >= d and (p + 1) * pb <= d + ln:
                    cbm[t, q // 32] |= np.uint32(1 << (q % 32))
    for batch in queue:
        for d, so, ln in batch:
            if write_valid(d, ln, max_len, pool.size):
                pool[d:d + ln] = src[so:so + ln]
        for p in touched_pages(batch, max_len, pool.size, pb):
            crcs[p] = crc_of(pool[p * pb:(p + 1) * pb])
    return copied, stale


def make_queue(rng, ppc, max_len):
    """Six chunks: snapshot slots {0, none, out of range, 1, none, none}, clone slots {none,
    0, none, none, out of range, 1}.  Every queue holds pages shared across and within
    batches, invalid entries of each kind, an entry crossing from the slotted chunk 0 into
    the unslotted chunk 1 and one crossing into the out-of-range chunk 2."""
    cb = ppc * PB
    pool_bytes = 6 * cb
    n_batches = int(rng.integers(2, 7))
    hot = int(rng.integers(0, ppc)) * PB + 3 * cb            # a page of chunk 3 (slot 1) every batch touches
    queue = []
    for k in range(n_batches):
        n = int(rng.integers(0, 12)) if k else int(rng.integers(4, 12))
        batch = []
        for _ in range(n):
            ln = int(rng.integers(1, max_len + 1))
            whole = rng.integers(0, 3) == 0                  # page-aligned entries, so clone bits do get set
            d = int(rng.integers(0, pool_bytes - ln))
            if whole:
                d, ln = d // PB * PB, max(PB, ln // PB * PB)
                d = min(d, pool_bytes - ln)
            batch.append((d, int(rng.integers(0, 4096)), ln))
        if n or k == 0:
            batch.append((hot + int(rng.integers(0, PB - 8)), 7, 8))
            batch.append((hot + int(rng.integers(0, PB - 8)), 9, 8))      # the same page twice in one batch
        queue.append(batch)
    queue[0] += [(cb - 10, 1, 20), (2 * cb - 10, 2, 20)]     # chunk 0 | 1 and chunk 1 | 2
    bad = [(5 * PB, 3, 0), (4 * cb + PB, 4, max_len + 1), (pool_bytes - 4, 5, 8), (1 << 40, 6, 4), (pool_bytes, 8, 1)]
    for j, e in enumerate(bad):                              # first, middle and last batch
        queue[(0, n_batches // 2, n_batches - 1)[j % 3]].append(e)
    return queue, pool_bytes, cb


@pytest.mark.parametrize("ppc", [5, 8, 40])
def test_one_pass_before_the_queue_equals_the_per_batch_sequence(ppc):
    """120 seeded queues (40 per chunk size: a partial bitmap word, a sub-word one and two
    words): slots, carried CRCs, snapshot bitmaps, clone bitmaps, both counts, the pool and
    the CRC table of the up-front pass equal those of apply_log_cow + clone_mark per batch,
    with preset bits, stale CRC words and out-of-range slots."""
    snap_slot = np.array([0, NO_SNAPSHOT, 7, 1, NO_SNAPSHOT, NO_SNAPSHOT], np.uint32)
    clone_slot = np.array([NO_SNAPSHOT, 0, NO_SNAPSHOT, NO_SNAPSHOT, 5, 1], np.uint32)
    total_copied = total_stale = total_marks = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 * ppc + seed)
        max_len = int(rng.choice([PB, 3 * PB + 7, 40]))
        queue, pool_bytes, cb = make_queue(rng, ppc, max_len)
        pool0 = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
        crcs0 = np.array([crc_of(pool0[p * PB:(p + 1) * PB]) for p in range(pool_bytes // PB)], np.uint32)
        wrong = rng.choice(crcs0.size, size=crcs0.size // 4, replace=False)
        crcs0[wrong] ^= np.uint32(0x10)                      # stale CRC words: they must be MOVED as they are
        src = rng.integers(0, 256, 4096 + max_len, dtype=np.uint8)
        snap0, scrc0, bm0 = fresh_slots(2, cb, PB)
        cbm0 = np.zeros((2, (ppc + 31) // 32), np.uint32)
        for arr in (bm0, cbm0):                              # preset bits, inside the slot's pages only
            for s in range(2):
                for q in rng.choice(ppc, size=ppc // 3, replace=False):
                    arr[s, q // 32] |= np.uint32(1 << (q % 32))
        out = []
        for fn in (sequence_model, prepass_model):
            st = [a.copy() for a in (pool0, crcs0, snap0, scrc0, bm0, cbm0)]
            pool, crcs, snap, scrc, bm, cbm = st
            counts = fn(pool, crcs, src, queue, max_len, PB, cb, snap_slot, 2, snap, scrc, bm, clone_slot, 2, cbm)
            out.append((counts, st))
        (cnt_a, st_a), (cnt_b, st_b) = out
        assert cnt_a == cnt_b, seed
        for name, a, b in zip(("pool", "crcs", "snap", "snap_crcs", "bitmap", "clone bitmap"), st_a, st_b):
            assert (a == b).all(), (seed, name)
        total_copied += cnt_a[0]
        total_stale += cnt_a[1]
        total_marks += int(sum(bin(int(w)).count("1") for w in (st_a[5] ^ cbm0).ravel()))
        if ppc % 32:                                         # no bit past the chunk's pages
            assert not (st_b[4][:, -1] >> np.uint32(ppc % 32)).any() and not (st_b[5][:, -1] >> np.uint32(ppc % 32)).any()
    assert total_copied > 40 and total_stale > 5 and total_marks > 5          # the queues did exercise all three


# --------------------------------------------------------------------------- ABI
def test_header_declares_library_exports_and_lib_has_the_prototype():
    from curve_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    L = _lib.lib()
    name = "cc_apply_logs_cow_dev"
    assert re.search(r"^int %s\(" % name, hdr, re.M)
    assert hasattr(L, name) and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    base_res, base_args = _lib.SIGNATURES["cc_apply_logs_dev"]
    assert res is base_res and args[:len(base_args)] == base_args
    assert args[len(base_args):] == [ctypes.POINTER(_lib.CcCow), ctypes.POINTER(_lib.CcClone)]
    m = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S)
    assert m.group(1).count(",") == len(args) - 1
    assert re.search(r"const cc_cow\* cow, const cc_clone\* clone\s*$", m.group(1))


FAKE = 1 << 20  # a fake device pointer: never dereferenced (the checks come first, and no device is present)


def _good_cow():
    from curve_amd import _lib
    c = _lib.CcCow()
    c.chunk_bytes, c.n_slots = 64 << 10, 2
    c.d_snap_slot = c.d_snap = c.d_snap_crcs = c.d_snap_bitmap = FAKE
    return c


def _good_clone():
    from curve_amd import _lib
    c = _lib.CcClone()
    c.chunk_bytes, c.n_slots = 64 << 10, 2
    c.d_clone_slot = c.d_bitmap = c.d_claim = c.d_pasted = FAKE
    return c


def _queue(n=(3, 0, 70), src=FAKE, log=FAKE):
    from curve_amd import _lib
    arr = (_lib.CcLogBatch * max(len(n), 1))()
    for k, nk in enumerate(n):
        arr[k].d_src, arr[k].d_log, arr[k].n_updates = src, log, nk
    return arr


def _call(L, cow="good", clone="good", queue=None, n_batches=None, pool=FAKE, pool_bytes=1 << 20, page_bytes=4096,
          max_len=4096, crcs=FAKE, work=FAKE, work_bytes=1 << 40, null_batches=False):
    vp = ctypes.c_void_p
    cow = _good_cow() if isinstance(cow, str) else cow
    clone = _good_clone() if isinstance(clone, str) else clone
    queue = _queue() if queue is None else queue
    n_batches = len(queue) if n_batches is None else n_batches
    return L.cc_apply_logs_cow_dev(vp(pool), pool_bytes, page_bytes,
                                   None if null_batches else ctypes.cast(queue, vp), n_batches, max_len, vp(crcs), 0,
                                   vp(work), work_bytes, None, ctypes.byref(cow) if cow is not None else None,
                                   ctypes.byref(clone) if clone is not None else None)


def _bad_cows():
    out = []
    for cb in (96 << 10, (64 << 10) + 256, 0):                  # does not divide the pool; no page multiple; zero
        c = _good_cow()
        c.chunk_bytes = cb
        out.append(c)
    for field in ("d_snap_slot", "d_snap", "d_snap_crcs", "d_snap_bitmap"):
        c = _good_cow()
        setattr(c, field, None)
        out.append(c)
    c = _good_cow()
    c.d_snap = FAKE + 2                                          # misaligned
    out.append(c)
    return out


def _bad_clones():
    out = []
    for field in ("d_clone_slot", "d_bitmap", "d_claim"):
        c = _good_clone()
        setattr(c, field, None)
        out.append(c)
    for cb in (96 << 10, (64 << 10) + 256, 0):
        c = _good_clone()
        c.chunk_bytes = cb
        out.append(c)
    return out


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    E, OK = _lib.CC_EINVAL, _lib.CC_OK
    # cc_apply_logs_dev's checks, one argument at a time
    for pb in (0, 100, 128, 1000, 3 * 256, 16384):               # not 256 * 2^k, k = 0..5
        assert _call(L, page_bytes=pb) == E, pb
    assert _call(L, null_batches=True) == E
    for name in ("pool", "crcs", "work"):
        assert _call(L, **{name: None}) == E, name
    assert _call(L, max_len=0) == E
    assert _call(L, None, None, pool_bytes=(1 << 20) + 256) == E  # not whole 4 KiB pages
    assert _call(L, pool_bytes=(1 << 20) + 256) == E
    assert _call(L, pool=FAKE + 2) == E                          # misaligned pool
    assert _call(L, page_bytes=256, max_len=256, pool_bytes=256 << 32) == E   # page + 1 must fit 32 bits
    assert _call(L, queue=_queue(log=None)) == E                 # records without a log
    assert _call(L, queue=_queue(src=None)) == E
    assert _call(L, queue=_queue(src=FAKE + 1)) == E             # misaligned source
    need = int(L.cc_apply_logs_work_bytes(70, 4096, 4096))
    assert need > 0 and _call(L, work_bytes=need - 1) == E
    # cc_apply_log_cow_dev's checks on cow, cc_clone_mark_dev's on clone -- also for an empty queue
    for k, c in enumerate(_bad_cows()):
        assert _call(L, cow=c) == E, k
        assert _call(L, cow=c, clone=None) == E, k
        assert _call(L, cow=c, n_batches=0) == E, k
        assert _call(L, cow=c, queue=_queue((0, 0))) == E, k
    for k, c in enumerate(_bad_clones()):
        assert _call(L, clone=c) == E, k
        assert _call(L, cow=None, clone=c) == E, k
        assert _call(L, clone=c, n_batches=0) == E, k
        assert _call(L, clone=c, queue=_queue((0, 0))) == E, k
    assert _call(L, queue=_queue((3, 1 << 31))) == E             # entry counts of the marks: below 2^31
    assert _call(L, cow=None, queue=_queue((1 << 31,))) == E
    # empty queues are no-ops, with either struct, both or none
    for cow in ("good", None):
        for clone in ("good", None):
            assert _call(L, cow, clone, n_batches=0) == OK
            assert _call(L, cow, clone, n_batches=0, null_batches=True) == OK
            assert _call(L, cow, clone, queue=_queue((0, 0, 0))) == OK
    c = _good_cow()                                              # the counters are optional
    c.d_copied = c.d_stale = None
    d = _good_clone()
    d.d_pasted = None
    assert _call(L, c, d, n_batches=0) == OK


def test_well_formed_call_needs_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    N = _lib.CC_ENODEV
    for cow in ("good", None):
        for clone in ("good", None):
            assert _call(L, cow, clone) == N
    for pb in (256, 512, 1024, 2048, 4096, 8192):
        assert _call(L, page_bytes=pb, max_len=3 * pb + 7) == N, pb
    assert _call(L, queue=_queue((3, (1 << 20)))) == N
    c, d = _good_cow(), _good_clone()
    c.n_slots = d.n_slots = 0                                    # nothing slotted: still a device call
    assert _call(L, c, d) == N


# --------------------------------------------------------------------------- Python
class _FakeTensor:
    is_cuda = True
    device = "dev0"

    def __init__(self, n=1 << 20):
        self.n = n

    def numel(self):
        return self.n

    def element_size(self):
        return 1

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return FAKE


class _FakeLib:
    def __init__(self):
        self.calls = []

    def cc_apply_logs_work_bytes(self, *a):
        return 4096

    def cc_apply_logs_dev(self, *a):
        self.calls.append(("cc_apply_logs_dev", a))
        return 0

    def cc_apply_logs_cow_dev(self, *a):
        self.calls.append(("cc_apply_logs_cow_dev", a))
        return 0


class _FakeTorch:
    class cuda:
        @staticmethod
        def device(_):
            return contextlib.nullcontext()

    uint8 = "u8"

    @staticmethod
    def empty(n, dtype=None, device=None):
        return _FakeTensor(n)


class _FakeStruct:
    def __init__(self, s):
        self._s = s

    def struct(self):
        return self._s


def test_python_apply_logs_takes_the_plain_symbol_without_cow_and_clone(monkeypatch):
    """crc.apply_logs(cow=None, clone=None) reaches cc_apply_logs_dev with the arguments it
    has always passed; with either struct it reaches cc_apply_logs_cow_dev, the structs last."""
    from curve_amd import crc as C
    fake = _FakeLib()
    monkeypatch.setattr(C, "lib", lambda: fake)
    monkeypatch.setattr(C, "_torch", lambda: _FakeTorch)
    monkeypatch.setattr(C, "_stream_key", lambda device, stream: (device, 0))
    monkeypatch.setattr(C, "_stream_handle", lambda stream: None)
    monkeypatch.setattr(C, "_log_work", {})
    pool, crcs, t = _FakeTensor(), _FakeTensor(1024), _FakeTensor(4096)
    batches = [(t, t, 70), (t, t, 0), (t, t, 3)]
    assert C.apply_logs(pool, crcs, batches, 4096, 4096) == 1
    assert C.apply_logs(pool, crcs, batches, 4096, 4096, delta=True, cow=None, clone=None) == 1
    assert [c[0] for c in fake.calls] == ["cc_apply_logs_dev"] * 2
    for (_, a), delta in zip(fake.calls, (0, 1)):
        assert len(a) == 11 and a[1:3] == (1 << 20, 4096) and a[4:6] == (3, 4096) and a[7] == delta and a[9] == 4096
    fake.calls.clear()
    from curve_amd import _lib
    cow, clone = _FakeStruct(_good_cow()), _FakeStruct(_good_clone())
    for kw in ({"cow": cow}, {"clone": clone}, {"cow": cow, "clone": clone}):
        assert C.apply_logs(pool, crcs, batches, 4096, 4096, **kw) == 1
    assert [c[0] for c in fake.calls] == ["cc_apply_logs_cow_dev"] * 3
    for (_, a), (has_cow, has_clone) in zip(fake.calls, ((1, 0), (0, 1), (1, 1))):
        assert len(a) == 13 and a[4:6] == (3, 4096)
        assert (a[11] is not None) == bool(has_cow) and (a[12] is not None) == bool(has_clone)
    assert _lib.SIGNATURES["cc_apply_logs_cow_dev"][1][-2:] == [ctypes.POINTER(_lib.CcCow), ctypes.POINTER(_lib.CcClone)]


# --------------------------------------------------------------------------- code object
def test_the_built_library_holds_the_prepass_kernels_for_gfx950_without_scratch(tmp_path):
    """The code object inside libcurvecrc.so, as the build left it: the twelve
    logs_prepass_kernel<M, Verify> are there for gfx950, none with a private segment
    (scratch) or a spilled register; without Verify the kernel holds no LDS image."""
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
    assert any("log_cow_kernel" in k for k in kernels)            # the parse sees the kernels that were there before
    new = {re.search(r"logs_prepass_kernelILi(\d+)ELb([01])E", k).groups(): v for k, v in kernels.items()
           if "logs_prepass_kernel" in k}
    assert sorted(new) == sorted((str(m), v) for m in (1, 2, 4, 8, 16, 32) for v in "01"), sorted(new)
    for (m, verify), v in new.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0 and \
            v.get("sgpr_spill_count", 0) == 0, (m, verify, v)
        assert v["vgpr_count"] <= 128, (m, verify, v)             # 16 waves a workgroup: four a SIMD
        assert v["group_segment_fixed_size"] == (163840 if verify == "1" else 0), (m, verify, v)
