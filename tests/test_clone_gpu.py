"""cc_paste_dev, cc_clone_mark_dev and cc_clone_check_reads_dev on the GPU,
checked bit for bit against the numpy models of test_clone.py (themselves
checked against request-by-request restatements of CSChunkFile::Paste, Write ...
flush() and Read's NextClearBit test) and the oracle's CRCs.

The rig: 8 chunks of 40 pages (two bitmap words a slot, the second partial; 40
is no power of two), clone slots {0, none, 2, none, 1, out of range, none, 3},
n_slots = 4, about 30 % of the bits set before the first call.  Pool, CRC table,
bitmaps and claim table are mirrored on the host and compared in full after
every call.
"""
import threading

import numpy as np
import pytest

from test_clone import (NOT_CLONE, U32_MAX, bit, check_reads_model, mark_model, paste_model, paste_valid,
                        replay_paste, set_bit, write_model)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PPC = 40
SLOTS = [0, NOT_CLONE, 2, NOT_CLONE, 1, 7, NOT_CLONE, 3]     # 7: out of range for n_slots = 4
N_SLOTS = 4
N_CHUNKS = len(SLOTS)
N_PAGES = N_CHUNKS * PPC
SRC_PAGES = 512
PAGE_SIZES = [256, 512, 1024, 2048, 4096, 8192]
SEEDS = {256: 50, 512: 51, 1024: 52, 2048: 53, 4096: 54, 8192: 55}  # each passes the class-count condition below


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from curve_amd import crc as C
    C.engine_init()
    return torch.device("cuda", 0)


def u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def random_bitmaps(rng, density, ppc=PPC):
    bm = np.zeros((N_SLOTS, (ppc + 31) // 32), np.uint32)
    for s in range(N_SLOTS):
        for q in range(ppc):
            if rng.random() < density:
                set_bit(bm, s, q)
    return bm


def random_pastes(rng, n=200, lo=1, hi=8):
    """n page-aligned pastes of lo..hi pages anywhere in the pool, each from a place of its own in the source,
    as [(first page, first source page, pages)]."""
    out = []
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        out.append((int(rng.integers(0, N_PAGES - k + 1)), int(rng.integers(0, SRC_PAGES - k + 1)), k))
    return out


def classes(entries, slots, bm, pb, pool_bytes, src_bytes, ppc=PPC):
    """The (entry, page) slots of a batch by what becomes of them, from the bitmaps BEFORE the call:
    (pasted, bit already set, lost to an earlier entry, chunk is no clone)."""
    pasted = held = lost = plain = 0
    taken = set()
    for dst, so, ln in entries:
        if not paste_valid(dst, so, ln, pool_bytes, src_bytes, pb):
            continue
        for p in range(dst // pb, (dst + ln) // pb):
            c, q = divmod(p, ppc)
            s = int(slots[c])
            if s >= N_SLOTS:
                plain += 1
            elif bit(bm, s, q):
                held += 1
            elif p in taken:
                lost += 1
            else:
                taken.add(p)
                pasted += 1
    return pasted, held, lost, plain


class Rig:
    """A pool with clone chunks on the device and its host mirror, advanced together one call at a time."""

    def __init__(self, dev, oracle, pb, seed=1, density=0.3, stream=None, ppc=PPC, src_pages=SRC_PAGES):
        from curve_amd import crc as C
        self.C, self.dev, self.stream = C, dev, stream
        self.host_init(oracle, pb, seed, density, ppc, src_pages)
        with C._on_stream(stream):
            self.d_pool = to_dev(self.host, dev)
            self.crcs = to_dev(i32(self.stored), dev)
            self.d_src = to_dev(self.src, dev)
            self.clone = C.Clone(N_CHUNKS, self.cb, pb, N_SLOTS, device=dev)
            self.clone.clone_slot.copy_(to_dev(i32(self.slots), dev))
            self.clone.bitmap.copy_(to_dev(i32(self.bm), dev))

    def host_init(self, oracle, pb, seed, density, ppc=PPC, src_pages=SRC_PAGES):
        self.oracle, self.pb = oracle, pb
        self.cb = ppc * pb
        self.slots = np.array(SLOTS, np.uint32)
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.host = rng.integers(0, 256, N_CHUNKS * self.cb, dtype=np.uint8)
        self.stored = oracle.page_crcs(self.host, pb)
        self.bm = random_bitmaps(rng, density, ppc)
        self.src = rng.integers(0, 256, src_pages * pb, dtype=np.uint8)
        self.total = 0

    def crc_fn(self, b):
        return self.oracle.crc32c(b.tobytes())

    def sync(self):
        if self.stream is not None:
            self.stream.synchronize()
        else:
            torch.cuda.synchronize()

    def entries(self, pastes):
        return [(p * self.pb, sp * self.pb, k * self.pb) for p, sp, k in pastes]

    def paste(self, entries, src=None, d_src=None):
        """One cc_paste_dev call and the model's answer to it: (per entry, model's per entry)."""
        C = self.C
        src = self.src if src is None else src
        d_src = self.d_src if d_src is None else d_src
        n = len(entries)
        rec = C.log_records([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries])
        with C._on_stream(self.stream):
            d_rec = to_dev(rec.view(np.uint8), self.dev)
            per = torch.zeros(n, dtype=torch.int32, device=self.dev)
        C.paste_records(self.d_pool, self.crcs, d_src, d_rec, n, self.clone, per, page_bytes=self.pb,
                        stream=self.stream)
        want, total = paste_model(self.host, self.stored, src, entries, self.slots, N_SLOTS, self.bm, self.pb, self.cb,
                                  self.crc_fn)
        self.total += total
        self.sync()
        return u32(per), want

    def check(self):
        """Pool, CRC table (against the model and against the oracle's CRCs of the
        resulting pool), bitmaps, the running total, and the claim table all-ones."""
        self.sync()
        got = self.d_pool.cpu().numpy()
        assert (got == self.host).all(), np.nonzero(got != self.host)[0][:10] // self.pb
        crcs = u32(self.crcs)
        assert (crcs == self.stored).all(), np.nonzero(crcs != self.stored)[0][:10]
        assert (crcs == self.oracle.page_crcs(got, self.pb)).all()
        bm = u32(self.clone.bitmap)
        assert (bm == self.bm).all(), (bm, self.bm)
        assert (u32(self.clone.claim) == U32_MAX).all()
        assert int(self.clone.pasted.item()) == self.total


def run_random_batch(rig, seed):
    """Test 1's batch on a rig: the input condition on the model's answer, then the device against the model."""
    pb = rig.pb
    entries = rig.entries(random_pastes(np.random.default_rng(seed)))
    pasted, held, lost, plain = classes(entries, rig.slots, rig.bm, pb, rig.host.size, rig.src.size)
    assert min(pasted, held, lost, plain) >= 50, (pasted, held, lost, plain)
    before, crcs_before, bm_before = rig.host.copy(), rig.stored.copy(), rig.bm.copy()
    got, want = rig.paste(entries)
    clear_left = sum(1 - bit(rig.bm, s, q) for s in (0, 1, 2, 3) for q in range(PPC))
    assert clear_left >= 1 and int(want.sum()) == pasted
    assert got.tolist() == want.tolist()
    rig.check()
    # every page the model did not paste keeps its bytes and its CRC
    untouched = np.ones(N_PAGES, bool)
    for c, s in enumerate(rig.slots):
        for q in range(PPC):
            if s < N_SLOTS and bit(rig.bm, s, q) and not bit(bm_before, s, q):
                untouched[c * PPC + q] = False
    assert (~untouched).sum() == pasted
    now = rig.d_pool.cpu().numpy().reshape(N_PAGES, pb)
    assert (now[untouched] == before.reshape(N_PAGES, pb)[untouched]).all()
    assert (u32(rig.crcs)[untouched] == crcs_before[untouched]).all()
    return entries, got


# --------------------------------------------------------------------------- 1, 3
@pytest.mark.parametrize("pb", PAGE_SIZES)
def test_paste_every_page_size(dev, oracle, pb):
    """M = 1 .. 32: 200 random page-aligned pastes of 1-8 pages, at least 50
    page slots in each class (pasted, bit already set, lost to an earlier entry,
    chunk is no clone).  Then the same batch again: nothing changes."""
    rig = Rig(dev, oracle, pb, seed=SEEDS[pb])
    entries, first = run_random_batch(rig, SEEDS[pb])
    got, want = rig.paste(entries)
    assert not got.any() and not want.any()
    rig.check()
    assert rig.total == int(first.sum())


# --------------------------------------------------------------------------- 2
def test_lowest_index_wins(dev, oracle):
    """130 entries over the same 3 clear pages of a clone chunk, each with a
    source pattern of its own: the pages hold entry 0's bytes."""
    pb = 1024
    rig = Rig(dev, oracle, pb, seed=2, density=0.0)
    n, p0 = 130, 2 * PPC + 31                                   # chunk 2 (slot 2), across its two bitmap words
    src = np.repeat(np.arange(n, dtype=np.uint8) + 1, 3 * pb)   # entry i's pages hold i + 1
    d_src = to_dev(src, dev)
    entries = [(p0 * pb, i * 3 * pb, 3 * pb) for i in range(n)]
    per = rig.C.paste(rig.d_pool, rig.crcs, d_src, [e[0] for e in entries], [e[1] for e in entries],
                      [e[2] for e in entries], rig.clone, pb)
    want, total = paste_model(rig.host, rig.stored, src, entries, rig.slots, N_SLOTS, rig.bm, pb, rig.cb, rig.crc_fn)
    rig.total += total
    torch.cuda.synchronize()
    assert u32(per).tolist() == [3] + [0] * (n - 1) == want.tolist() and total == 3
    rig.check()
    assert (rig.d_pool.cpu().numpy()[p0 * pb:(p0 + 3) * pb] == 1).all()
    assert int(rig.clone.pasted.item()) == 3
    assert int(rig.bm[2, 0]) == 1 << 31 and int(rig.bm[2, 1]) == 0b11


# --------------------------------------------------------------------------- schedule edges
def pastes_with_slots(rng, total):
    """Pastes of 1-8 pages, each from a place of its own in the source, whose page counts sum to `total` exactly."""
    out, left = [], total
    while left:
        k = min(int(rng.integers(1, 9)), left)
        out.append((int(rng.integers(0, N_PAGES - k + 1)), int(rng.integers(0, SRC_PAGES - k + 1)), k))
        left -= k
    return out


@pytest.mark.parametrize("pb", [1024, 4096])
@pytest.mark.parametrize("total", [1, 63, 64, 65, 1023])
def test_slot_totals_at_the_schedules_edges(dev, oracle, pb, total):
    """The paste launch's shares at its edges: one slot, one short of a group of
    64, a whole group, one over, and a total that leaves a dynamic tail with a
    short last chunk; every bit clear, so every first slot of a clone page pastes."""
    rig = Rig(dev, oracle, pb, seed=7 + total, density=0.0)
    entries = rig.entries(pastes_with_slots(np.random.default_rng(total), total))
    assert sum(e[2] for e in entries) == total * pb
    pasted, held, lost, plain = classes(entries, rig.slots, rig.bm, pb, rig.host.size, rig.src.size)
    assert held == 0 and pasted + lost + plain == total
    got, want = rig.paste(entries)
    assert got.tolist() == want.tolist() and int(got.sum()) == pasted == rig.total
    rig.check()


# --------------------------------------------------------------------------- 4
def test_invalid_entries_write_nothing(dev, oracle):
    pb = 512
    rig = Rig(dev, oracle, pb, seed=4, density=0.0)
    pool_bytes, src_bytes = rig.host.size, rig.src.size
    good = rig.entries(random_pastes(np.random.default_rng(40), n=90, lo=1, hi=4))
    # where each invalid entry would have landed there is a clear page of a clone chunk that no valid entry covers
    spare = [p for p in range(4 * PPC, 5 * PPC)]                # chunk 4 (slot 1)
    good = [e for e in good if not (e[0] < 5 * PPC * pb and e[0] + e[2] > 4 * PPC * pb)]
    good = [e for e in good if e[0] + e[2] <= pool_bytes - pb]   # ... nor the pool's last page
    bad = {
        3: (spare[0] * pb + 256, 0, pb),                        # misaligned dst
        7: (spare[2] * pb, 0, pb + 4),                          # misaligned len
        11: (pool_bytes - pb, 0, 2 * pb),                       # runs past the pool
        12: (pool_bytes, 0, pb),                                # starts at its end
        20: (1 << 40, 0, pb),                                   # dst = 2^40
        33: (spare[4] * pb, 6, pb),                             # src unaligned
        41: (spare[6] * pb, src_bytes - pb, 2 * pb),            # src past src_bytes by one page
        42: (spare[8] * pb, 1 << 40, pb),                       # src far outside
    }
    entries = list(good)
    for at in sorted(bad):
        entries.insert(at, bad[at])
    entries.insert(50, (spare[10] * pb, 0, 0))                  # empty: valid, touches nothing
    entries.append((spare[12] * pb, src_bytes - pb, pb))        # ends exactly at the source's end: valid
    empty_at = 50
    before = rig.host.copy()
    got, want = rig.paste(entries)
    assert got.tolist() == want.tolist()
    invalid = [i for i, e in enumerate(entries) if not paste_valid(*e, pool_bytes, src_bytes, pb)]
    assert sorted(invalid) == sorted(i for i, e in enumerate(entries) if e in bad.values()) and len(invalid) == 8
    assert (got[invalid] == U32_MAX).all() and (np.delete(got, invalid) != U32_MAX).all()
    assert got[empty_at] == 0 and got[-1] == 1
    rig.check()
    now = rig.d_pool.cpu().numpy()
    lo, hi = spare[0] * pb, spare[11] * pb                      # nothing of an invalid (or the empty) entry was written
    assert (now[lo:hi] == before[lo:hi]).all() and int(rig.bm[1, 0]) == 1 << 12 and int(rig.bm[1, 1]) == 0
    assert (now[-pb:] == before[-pb:]).all()


# --------------------------------------------------------------------------- 5, 7
def test_whole_chunk_paste_check_reads_and_read_back(dev, oracle):
    """A paste covering a whole clone chunk sets its 40 bits and no other; the
    metapage becomes an ordinary chunk's.  cc_clone_check_reads_dev before and
    after, against the model; reads it clears verify clean through
    cc_verify_reads_dev, and cc_read_snap_dev (cow = NULL) returns the pasted bytes."""
    from curve_amd.chunkfile import ChunkFileMetaPage, CSErrorCode, clone_metapage_after
    pb = 2048
    rig = Rig(dev, oracle, pb, seed=5)
    C, cb = rig.C, rig.cb
    rng = np.random.default_rng(57)
    reads = []
    for _ in range(200):
        off = int(rng.integers(0, rig.host.size))
        reads.append((off, int(rng.integers(1, min(6 * pb, rig.host.size - off) + 1))))
    reads[0] = (cb - 100, 200)                                  # slot 0 | none
    reads[1] = (2 * cb - pb - 1, 3 * pb)                        # none | slot 2
    reads[2] = (5 * cb - 1, 2)                                  # slot 1 | out of range
    reads[3] = (rig.host.size - 10, 11)                         # past the pool by one byte
    reads[4] = (rig.host.size, 1)
    reads[5] = (1 << 40, pb)
    reads[6] = (3 * pb, 0)                                      # empty
    reads[7] = (rig.host.size - 1, 1)                           # the pool's last byte
    inside = [(2 * cb + int(rng.integers(0, cb - 4 * pb)), int(rng.integers(1, 4 * pb))) for _ in range(20)]
    reads += inside                                             # all inside chunk 2 (slot 2)

    def check_reads():
        got, total = C.clone_check_reads(rig.d_pool, [r[0] for r in reads], [r[1] for r in reads], rig.clone, pb)
        torch.cuda.synchronize()
        want, w_total = check_reads_model(reads, rig.host.size, rig.slots, N_SLOTS, rig.bm, pb, cb)
        assert u32(got).tolist() == want.tolist() and int(total.item()) == w_total
        return want

    first = check_reads()
    assert (first[[3, 4, 5]] == U32_MAX).all() and first[6] == 0 and first[7] != U32_MAX
    assert first[-20:].any() and w_some(first)
    slot2_before = [bit(rig.bm, 2, q) for q in range(PPC)]
    assert 0 < sum(slot2_before) < PPC
    before = rig.host.copy()
    got, want = rig.paste([(2 * cb, 7 * pb, cb)])               # chunk 2, whole
    assert got.tolist() == want.tolist() == [PPC - sum(slot2_before)]
    rig.check()
    words = u32(rig.clone.bitmap)
    assert int(words[2, 0]) == 0xFFFFFFFF and int(words[2, 1]) == 0xFF   # bits 40-63 stay clear
    for q in range(PPC):                                        # set before: the old bytes; pasted: the source's
        exp = before[2 * cb + q * pb:2 * cb + (q + 1) * pb] if slot2_before[q] else rig.src[(7 + q) * pb:(8 + q) * pb]
        assert (rig.host[2 * cb + q * pb:2 * cb + (q + 1) * pb] == exp).all()
    meta = ChunkFileMetaPage(sn=3, location=b"/origin/vol@7", bitmap_bits=PPC, bitmap=bytes(5))
    after = clone_metapage_after(meta, rig.clone.slot_bitmap_bytes(2))
    assert after.location == b"" and after.encode() == ChunkFileMetaPage(sn=3).encode()
    rc, back = ChunkFileMetaPage.decode(after.encode())
    assert rc == CSErrorCode.Success and back.location == b""
    still = clone_metapage_after(meta, rig.clone.slot_bitmap_bytes(0))
    assert still.location == meta.location and still.bitmap == rig.bm[0].tobytes()[:5]
    second = check_reads()
    assert not second[-20:].any()                               # the reads inside that chunk all report 0
    # every read the check clears verifies clean through the existing verify-on-read
    ok = [r for r, cnt in zip(reads, second) if cnt == 0]
    assert len(ok) >= 20
    bad, total = C.verify_reads(rig.d_pool, rig.crcs, [r[0] for r in ok], [r[1] for r in ok], pb)
    torch.cuda.synchronize()
    assert not u32(bad).any() and int(total.item()) == 0
    # the pasted bytes come back through the existing snapshot-read path, with the new CRCs
    out, bad, total = C.read_snap(rig.d_pool, rig.crcs, [2 * cb, 2 * cb + 5 * pb], [cb, 3 * pb], None, pb)
    torch.cuda.synchronize()
    assert not u32(bad).any() and int(total.item()) == 0
    out = out.cpu().numpy()
    assert (out[:cb] == rig.host[2 * cb:3 * cb]).all() and (out[cb:] == rig.host[2 * cb + 5 * pb:2 * cb + 8 * pb]).all()


def w_some(counts):
    """The batch has reads that may be served and reads that may not."""
    ok = counts[counts != U32_MAX]
    return (ok == 0).any() and (ok != 0).any()


# --------------------------------------------------------------------------- 6
def mixed_log(rng, pb, n=150):
    """Whole-page, straddling and partial writes (max_len = 3 pages), and two contract breakers."""
    log = []
    pool_bytes = N_PAGES * pb
    for i in range(n):
        kind = i % 3
        if kind == 0:                                           # whole pages
            k = int(rng.integers(1, 4))
            dst = int(rng.integers(0, N_PAGES - k + 1)) * pb
            ln = k * pb
        elif kind == 1:                                         # straddling: one to three pages from mid-page
            k = int(rng.integers(1, 4))
            dst = int(rng.integers(0, N_PAGES - k)) * pb + int(rng.integers(1, pb))
            ln = k * pb
        else:                                                   # partial: inside one page
            ln = int(rng.integers(1, pb))
            dst = int(rng.integers(0, N_PAGES)) * pb + int(rng.integers(0, pb - ln + 1))
        log.append((dst, int(rng.integers(0, (SRC_PAGES - 3) * pb)), ln))
    log[10] = (pool_bytes - pb, 0, 2 * pb)                      # runs past the pool: skipped whole
    log[20] = (5 * pb, 0, 3 * pb + 1)                           # longer than max_len: skipped whole
    return log


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("pb", [512, 4096])
def test_mark_after_write_log_then_paste(dev, oracle, pb, delta):
    """apply_log (full and delta) -> clone_mark against mark_model; then a paste
    over the whole pool: every marked page keeps the bytes the write left, and
    the whole sequence equals the request-by-request replay on the CPU."""
    rig = Rig(dev, oracle, pb, seed=60 + delta, density=0.1)
    C = rig.C
    log = mixed_log(np.random.default_rng(pb + delta), pb)
    max_len = 3 * pb
    wsrc = np.random.default_rng(6).integers(0, 256, SRC_PAGES * pb, dtype=np.uint8)
    # the replay's own state: one request at a time
    r_pool, r_bm = rig.host.copy(), rig.bm.copy()
    for e in log:
        write_model(r_pool, wsrc, [e], max_len)
        mark_model([e], max_len, r_pool.size, rig.slots, N_SLOTS, r_bm, pb, rig.cb)
    r_crcs = oracle.page_crcs(r_pool, pb)
    rec = C.log_records([e[0] for e in log], [e[1] for e in log], [e[2] for e in log])
    d_log, d_wsrc = to_dev(rec.view(np.uint8), dev), to_dev(wsrc, dev)
    C.apply_log(rig.d_pool, rig.crcs, d_wsrc, d_log, len(log), max_len, pb, delta=delta)
    C.clone_mark(rig.d_pool, d_log, len(log), max_len, rig.clone, pb)
    bm_before = rig.bm.copy()
    write_model(rig.host, wsrc, log, max_len)
    rig.stored = oracle.page_crcs(rig.host, pb)
    mark_model(log, max_len, rig.host.size, rig.slots, N_SLOTS, rig.bm, pb, rig.cb)
    assert (rig.bm != bm_before).any()
    rig.check()
    assert (rig.bm == r_bm).all() and (rig.host == r_pool).all()
    written = rig.host.copy()
    marked = [(c, q) for c, s in enumerate(rig.slots) if s < N_SLOTS for q in range(PPC) if bit(rig.bm, s, q)]
    pastes = [(c * rig.cb, (3 * c + 1) * pb, rig.cb) for c in range(N_CHUNKS)] + [(0, 0, 2 * rig.cb)]
    got, want = rig.paste(pastes)
    assert got.tolist() == want.tolist() and want[-1] == 0 and int(want.sum()) == 4 * PPC - len(marked)
    rig.check()
    now = rig.d_pool.cpu().numpy()
    for c, q in marked:
        p = c * PPC + q
        assert (now[p * pb:(p + 1) * pb] == written[p * pb:(p + 1) * pb]).all(), (c, q)
    r_per, r_total = replay_paste(r_pool, r_crcs, rig.src, pastes, rig.slots, N_SLOTS, r_bm, pb, rig.cb, rig.crc_fn)
    assert (now == r_pool).all() and (u32(rig.crcs) == r_crcs).all() and (u32(rig.clone.bitmap) == r_bm).all()
    assert got.tolist() == r_per.tolist() and r_total == int(want.sum())


# --------------------------------------------------------------------------- 8
def test_streams_and_threads(dev, oracle):
    """Two threads, each with a stream, a rig and a Clone of its own, each running test 1's batch at 512 B and 4 KiB."""
    errs = []

    def work(i):
        try:
            s = torch.cuda.Stream(device=dev)
            for pb in (512, 4096):
                rig = Rig(dev, oracle, pb, seed=SEEDS[pb], stream=s)
                run_random_batch(rig, SEEDS[pb])
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append((i, e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
