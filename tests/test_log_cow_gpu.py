"""cc_apply_log_cow_dev on the GPU: copy on write for chunks with an open
snapshot, checked against the numpy model of test_log_cow.py (itself checked
against a per-request replay of the reference) and the oracle.

Every case checks
  * the pool bytes and page CRCs equal those of the non-COW call on a twin pool
    (and the model's bytes / the oracle's CRCs);
  * the snapshot view of every slotted chunk (slot page where the bit is set,
    live page otherwise) equals the chunk's bytes from before the first batch;
  * set bits: d_snap_crcs == the oracle CRC of those old bytes;
  * clear bits (and bits set before the call): slot bytes and CRCs still hold
    the sentinel they were filled with;
  * the bitmaps equal the model's, and d_copied the model's count.
"""
import threading

import numpy as np
import pytest

from test_log_cow import NO_SNAPSHOT, SENT_BYTE, SENT_CRC, bitmap_bytes, cow_model, fresh_slots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PPC = 40                                                     # two bitmap words a slot, the second partial
SLOTS = [0, NO_SNAPSHOT, 2, NO_SNAPSHOT, 1, 9, NO_SNAPSHOT, 3]  # 9: out of range for n_slots = 4
N_SLOTS = 4
PRESET = [(0, 4), (2, 33), (3, 39), (1, 0)]                  # (slot, page of the chunk) held before the first call


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from curve_amd import crc as C
    C.engine_init()
    return torch.device("cuda", 0)


def u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


class Rig:
    """A pool of len(slots) chunks with its twin (non-COW calls), the device
    slots and the host model, advanced together one batch at a time."""

    def __init__(self, dev, oracle, pb, ppc=PPC, slots=SLOTS, n_slots=N_SLOTS, preset=PRESET, seed=1, verify=False,
                 stream=None):
        from curve_amd import crc as C
        self.C, self.dev, self.oracle, self.pb, self.ppc, self.n_slots = C, dev, oracle, pb, ppc, n_slots
        self.stream = stream
        self.cb = ppc * pb
        self.slots = np.array(slots, np.uint32)
        rng = np.random.default_rng(seed)
        self.orig = rng.integers(0, 256, len(slots) * self.cb, dtype=np.uint8)
        self.orig_crcs = oracle.page_crcs(self.orig, pb)
        self.host = self.orig.copy()
        self.stored = self.orig_crcs.copy()  # the CRC table before the next batch
        self.snap, self.scrc, self.bm = fresh_slots(n_slots, self.cb, pb)
        for s, q in preset:
            self.bm[s, q // 32] |= np.uint32(1 << (q % 32))
        self.preset = set(preset)
        self.copied = 0
        with C._on_stream(stream):
            self.d_pool, self.d_twin = to_dev(self.orig, dev), to_dev(self.orig, dev)
            self.crcs, self.twin_crcs = to_dev(i32(self.orig_crcs), dev), to_dev(i32(self.orig_crcs), dev)
            self.cow = C.Cow(len(slots), self.cb, pb, n_slots, device=dev, verify=verify, fill=SENT_BYTE,
                             crc_fill=int(np.uint32(SENT_CRC).view(np.int32)))
            self.cow.snap_slot.copy_(to_dev(i32(self.slots), dev))
            self.cow.bitmap.copy_(to_dev(i32(self.bm), dev))

    def corrupt(self, pages):
        """Flip a byte of these pages behind the CRC table's back (pool, twin, model)."""
        for p in pages:
            off = p * self.pb + 17 + (p % 100)
            self.host[off] ^= 0x40
            self.orig[off] ^= 0x40  # the bytes a snapshot must show ARE the corrupt ones
            for t in (self.d_pool, self.d_twin):
                t[off] ^= 0x40

    def batch(self, dst, src_off, lens, src, max_len, delta, cow=True):
        C = self.C
        dst, src_off, lens = np.asarray(dst, np.uint64), np.asarray(src_off, np.uint64), np.asarray(lens, np.uint32)
        n = dst.size
        with C._on_stream(self.stream):
            d_log = torch.from_numpy(C.log_records(dst, src_off, lens).view(np.uint8)).to(self.dev)
            d_src = to_dev(src, self.dev)
        C.apply_log_cow(self.d_pool, self.crcs, d_src, d_log, n, max_len, self.cow if cow else None, self.pb,
                        stream=self.stream, delta=delta)
        C.apply_log(self.d_twin, self.twin_crcs, d_src, d_log, n, max_len, self.pb, stream=self.stream, delta=delta)
        if cow:
            self.copied += cow_model(self.host, self.stored, src, dst, src_off, lens, max_len, self.pb, self.cb,
                                     self.slots, self.n_slots, self.snap, self.scrc, self.bm)
        else:
            nobody = np.full_like(self.slots, NO_SNAPSHOT)
            cow_model(self.host, self.stored, src, dst, src_off, lens, max_len, self.pb, self.cb, nobody,
                      self.n_slots, self.snap, self.scrc, self.bm)
        self.stored = None  # (set by check(): the CRCs after this batch)

    def check(self, clean=True, view=True):
        """All the properties of the module docstring.  clean=False: some pages
        were corrupted behind the table, so the CRCs are compared with the
        twin's only, and the carried CRCs with the table from before.
        view=False: the batches went in with cow == NULL (written in place, as
        without a snapshot), so there is no snapshot view to hold."""
        if self.stream is not None:
            self.stream.synchronize()
        else:
            torch.cuda.synchronize()
        pb, ppc = self.pb, self.ppc
        got, twin = self.d_pool.cpu().numpy(), self.d_twin.cpu().numpy()
        assert (got == twin).all() and (got == self.host).all()
        crcs = u32(self.crcs)
        assert (crcs == u32(self.twin_crcs)).all()
        if clean:
            assert (crcs == self.oracle.page_crcs(self.host, pb)).all()
        self.stored = crcs.copy()
        snap = self.cow.snap.cpu().numpy()
        scrc, bm = u32(self.cow.snap_crcs), u32(self.cow.bitmap)
        assert (bm == self.bm).all()
        assert int(self.cow.copied.item()) == self.copied
        assert (snap == self.snap).all() and (scrc == self.scrc).all()  # sentinels included
        # ... and independently of the model:
        owner = {int(s): c for c, s in enumerate(self.slots) if s < self.n_slots}
        copied = 0
        for s in range(self.n_slots):
            held = np.array([(int(bm[s, q // 32]) >> (q % 32)) & 1 for q in range(ppc)], bool)
            mine = np.array([(s, q) in self.preset for q in range(ppc)], bool)
            pages = snap[s].reshape(ppc, pb)
            sent = ~held | mine
            assert (pages[sent] == SENT_BYTE).all() and (scrc[s][sent] == SENT_CRC).all()
            if s not in owner:
                assert not (held & ~mine).any()
                continue
            c = owner[s]
            old = self.orig[c * self.cb:(c + 1) * self.cb].reshape(ppc, pb)
            live = got[c * self.cb:(c + 1) * self.cb].reshape(ppc, pb)
            seen = np.where((held & ~mine)[:, None], pages, live)
            assert not view or (seen[~mine] == old[~mine]).all()
            taken = held & ~mine
            assert (scrc[s][taken] == self.orig_crcs[c * ppc:(c + 1) * ppc][taken]).all()
            if clean and taken.any():
                assert (scrc[s][taken] == self.oracle.page_crcs(pages[taken], pb)).all()
            copied += int(taken.sum())
        assert copied == self.copied
        return copied


def random_log(rng, n, pool_bytes, max_len, pb):
    lens = rng.integers(1, max_len + 1, n).astype(np.uint32)
    dst = rng.integers(0, pool_bytes - max_len, n).astype(np.uint64)
    # the first write straddles pages 3 | 4 of chunk 0 (slot 0; page 4 is held already)
    dst[0], lens[0] = 3 * pb + pb // 2, min(max_len, pb)
    src = rng.integers(0, 256, (1 << 16) + max_len, dtype=np.uint8)
    src_off = rng.integers(0, 1 << 16, n).astype(np.uint64)
    return dst, src_off, lens, src


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65, 3000])
@pytest.mark.parametrize("pb", [256, 512, 2048, 4096, 8192])
def test_cow_page_sizes_and_log_sizes(dev, oracle, pb, n, delta):
    """Every M family (1, 2, 8, 16, 32 dwords a lane) x logs of 1 / 64 (would take
    the one-launch path without cow) / 65 / 3,000 writes (several head segments)
    x full and delta mode, on 8 chunks of 40 pages with slots {0, none, 2, none,
    1, out of range, none, 3} and four bits held before the call."""
    rig = Rig(dev, oracle, pb, seed=pb + n)
    rng = np.random.default_rng(n * 7 + pb + delta)
    max_len = pb + 300 if n == 3000 else pb  # 3 pieces a write / 2
    rig.batch(*random_log(rng, n, rig.orig.size, max_len, pb), max_len, delta)
    copied = rig.check()
    assert copied == (1 if n == 1 else copied) and copied >= 1  # page 3 of chunk 0; page 4 was held
    if n == 3000:
        assert copied == 4 * PPC - len(PRESET)  # every page of the four slotted chunks is touched


@pytest.mark.parametrize("delta", [False, True])
def test_cow_three_batches_keep_the_first_version(dev, oracle, delta):
    """A second and a third batch over overlapping pages: pages copied by an
    earlier batch keep their first version (bytes and CRC), new pages join."""
    pb = 4096
    rig = Rig(dev, oracle, pb, seed=5)
    rng = np.random.default_rng(50 + delta)
    seen = []
    for k, n in enumerate((40, 200, 2000)):
        rig.batch(*random_log(rng, n, rig.orig.size, pb, pb), pb, delta)
        seen.append(rig.check())
    assert seen[0] < seen[1] < seen[2] == 4 * PPC - len(PRESET)


@pytest.mark.parametrize("delta", [False, True])
def test_cow_grid_stride_insert(dev, oracle, delta):
    """More pieces than kInsertThreads * kInsertBlocks = 131,072 (66,000 writes
    of 2 pieces): the insert blocks take several chunks each, so every head
    segment holds records of several rounds."""
    pb = 512
    rig = Rig(dev, oracle, pb, seed=6)
    rng = np.random.default_rng(60 + delta)
    n = 66000
    lens = rng.integers(1, 65, n).astype(np.uint32)
    dst = rng.integers(0, rig.orig.size - 64, n).astype(np.uint64)
    src = rng.integers(0, 256, (1 << 16) + 64, dtype=np.uint8)
    src_off = rng.integers(0, 1 << 16, n).astype(np.uint64)
    rig.batch(dst, src_off, lens, src, 64, delta)
    assert rig.check() == 4 * PPC - len(PRESET)


@pytest.mark.parametrize("delta", [False, True])
def test_cow_hot_pages_and_contract_breakers(dev, oracle, delta):
    """700 writes piled on four pages (piece lists longer than 64: each page is
    still copied once, before any of them lands) and entries that break the
    contract (len 0, len > max_len, past the pool, far beyond it), aimed at
    slotted pages nothing else touches: they copy nothing."""
    pb = 4096
    rig = Rig(dev, oracle, pb, seed=7, preset=[])
    rng = np.random.default_rng(70 + delta)
    n = 704
    cb, total = rig.cb, rig.orig.size
    lens = rng.integers(1, 3000, n).astype(np.uint32)
    dst = (rng.integers(0, 3 * pb, n) + 4 * cb + 5 * pb).astype(np.uint64)  # chunk 4 (slot 1) pages 5..8
    lens[dst + lens > 4 * cb + 9 * pb] = 100
    src = rng.integers(0, 256, (1 << 16) + 4096, dtype=np.uint8)
    src_off = rng.integers(0, 1 << 16, n).astype(np.uint64)
    dst[3], lens[3] = 2 * cb + 10 * pb, 0                  # empty, on chunk 2 (slot 2)
    dst[100], lens[100] = 2 * cb + 12 * pb, 3500           # > max_len
    dst[101], lens[101] = total - 10, 20                   # runs past the pool (chunk 7, slot 3)
    dst[650], lens[650] = 1 << 40, 8                       # far beyond
    rig.batch(dst, src_off, lens, src, 3000, delta)
    copied = rig.check()
    assert 1 <= copied <= 4
    bm = u32(rig.cow.bitmap)
    assert int(bm[1, 0]) & ~0b111100000 == 0 and not bm[[0, 2, 3]].any() and int(bm[1, 1]) == 0


@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("pb", [256, 2048, 4096, 8192])
def test_cow_stale_pages(dev, oracle, pb, delta, verify):
    """Three pages the batch touches and two it does not are corrupted behind
    the CRC table: d_stale comes back 3, the three copies keep mismatching the
    CRC they carry (the stored one, moved), everything else is as without the
    count; d_stale = NULL gives the same results without it."""
    rig = Rig(dev, oracle, pb, seed=8, preset=[], verify=verify)
    cb, ppc = rig.cb, PPC
    hit = [0 * ppc + 3, 2 * ppc + 33, 7 * ppc + 39]        # slots 0, 2, 3
    miss = [0 * ppc + 20, 4 * ppc + 1]                     # slotted chunks, untouched pages
    rig.corrupt(hit + miss)
    rng = np.random.default_rng(80 + delta)
    n = 90
    pages = rng.integers(0, 8 * ppc, n)
    pages = pages[~np.isin(pages, miss)]
    pages[:3] = hit
    n = pages.size
    lens = rng.integers(1, pb // 2, n).astype(np.uint32)
    dst = (pages * pb + rng.integers(0, pb // 2, n)).astype(np.uint64)
    src = rng.integers(0, 256, (1 << 16) + pb, dtype=np.uint8)
    src_off = rng.integers(0, 1 << 16, n).astype(np.uint64)
    rig.batch(dst, src_off, lens, src, pb, delta)
    copied = rig.check(clean=False)
    assert copied >= 3
    if verify:
        assert int(rig.cow.stale.item()) == 3
    else:
        assert rig.cow.stale is None
    snap, scrc = rig.cow.snap.cpu().numpy(), u32(rig.cow.snap_crcs)
    bad = 0
    for c, s in ((0, 0), (2, 2), (4, 1), (7, 3)):
        bm = u32(rig.cow.bitmap)[s]
        for q in range(ppc):
            if (int(bm[q // 32]) >> (q % 32)) & 1:
                mism = oracle.crc32c(snap[s, q * pb:(q + 1) * pb].tobytes()) != int(scrc[s, q])
                assert mism == (c * ppc + q in hit)
                bad += mism
    assert bad == 3


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("n", [64, 3000])
def test_cow_null_is_the_plain_call(dev, oracle, n, delta):
    """cow == NULL: cc_apply_log_dev / cc_apply_log_delta_dev, one-launch path included."""
    pb = 4096
    rig = Rig(dev, oracle, pb, seed=9)
    rng = np.random.default_rng(90 + n + delta)
    rig.batch(*random_log(rng, n, rig.orig.size, pb, pb), pb, delta, cow=False)
    assert rig.check(view=False) == 0


def test_cow_slot_bitmap_through_the_metapage_codec(dev, oracle):
    """A slot's bitmap, copied to the host and encoded with cc_snap_meta_encode,
    decodes to the model's bitmap for that slot."""
    from curve_amd import crc as C
    pb = 512
    rig = Rig(dev, oracle, pb, seed=10)
    rng = np.random.default_rng(100)
    rig.batch(*random_log(rng, 70, rig.orig.size, pb, pb), pb, False)
    rig.check()
    for s in range(N_SLOTS):
        raw = rig.cow.slot_bitmap_bytes(s)
        assert raw == bitmap_bytes(rig.bm[s], PPC)
        page = C.snap_meta_encode(1000 + s, raw, PPC, 4096)
        assert C.snap_meta_decode(page) == (1000 + s, False, PPC, bitmap_bytes(rig.bm[s], PPC))


def test_cow_streams_and_threads(dev, oracle):
    """A non-default stream, then two streams from two threads on disjoint
    pools, each with slots of its own."""
    pb = 4096
    s0 = torch.cuda.Stream(device=dev)
    rig = Rig(dev, oracle, pb, seed=11, stream=s0)
    rng = np.random.default_rng(110)
    rig.batch(*random_log(rng, 500, rig.orig.size, pb, pb), pb, True)
    rig.check()
    errs = []

    def work(i):
        try:
            s = torch.cuda.Stream(device=dev)
            r = Rig(dev, oracle, pb, seed=20 + i, stream=s)
            g = np.random.default_rng(120 + i)
            for n in (300, 65, 900):
                r.batch(*random_log(g, n, r.orig.size, pb, pb), pb, bool(i))
                r.check()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
