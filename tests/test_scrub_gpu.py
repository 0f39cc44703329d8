"""Scrub on the device (cc_scrub_dev): every case compared with test_scrub's
numpy model and the oracle's CRCs, never with the code under test.  The rig is
the suite's small one (8 chunks of 40 pages, clone slots {0, -, 2, -, 1, out of
range, -, 3}) with snapshot slots on three of the non-clone chunks, a sentinel
in every table word and snapshot byte that describes nothing, and the list and
the per-chunk array between guard bands."""
import numpy as np
import pytest

from test_clone import NOT_CLONE, bit
from test_log_cow import NO_SNAPSHOT
from test_repair_gpu import Guarded
from test_scrub import COUNTS, CRC_SENT, PAGE_SIZES, PPC, SNAP, HostRig, popcount_valid

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LIST_SENT = -7            # what the list holds where nothing was stored


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from curve_amd import crc as C
    C.engine_init()
    return torch.device("cuda", 0)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class DevRig:
    """A HostRig on the device: the pool, its table, a C.Cow and a C.Clone filled from the host arrays."""

    def __init__(self, dev, oracle, pb, seed, stream=None, max_list=64, **kw):
        from curve_amd import crc as C
        self.C, self.dev, self.oracle, self.stream, self.max_list = C, dev, oracle, stream, max_list
        self.h = HostRig(pb, seed, oracle.page_crcs, **kw)
        self.upload()

    def upload(self):
        C, h, dev = self.C, self.h, self.dev
        with C._on_stream(self.stream):
            self.pool = to_dev(h.pool, dev)
            self.crcs = to_dev(i32(h.crcs), dev)
            self.cow = C.Cow(h.n_chunks, h.cb, h.pb, h.cow.n_slots, device=dev, verify=True)
            self.cow.snap_slot = to_dev(i32(h.cow.snap_slot), dev)
            self.cow.snap = to_dev(h.cow.snap[:max(h.cow.n_slots, 1)], dev)
            self.cow.snap_crcs = to_dev(i32(h.cow.snap_crcs), dev)
            self.cow.bitmap = to_dev(i32(h.cow.bitmap), dev)
            self.clone = C.Clone(h.n_chunks, h.cb, h.pb, h.clone.n_slots, device=dev)
            self.clone.clone_slot = to_dev(i32(h.clone.clone_slot), dev)
            self.clone.bitmap = to_dev(i32(h.clone.bitmap), dev)
            self.counts = torch.zeros(6, dtype=torch.int64, device=dev)
            self.list = Guarded(np.full(max(self.max_list, 1), LIST_SENT, np.int64), dev, 16)
            self.per = Guarded(np.zeros(h.n_chunks * 2, np.int32), dev, 16)

    def crc_fn(self, b):
        return self.oracle.crc32c(b.tobytes())

    def model(self, cow=True, clone=True, counts=None):
        return self.h.model(self.crc_fn, cow=cow, clone=clone, counts=counts)

    def frozen(self):
        """Everything the call may not write."""
        ts = [self.pool, self.crcs, self.cow.snap_slot, self.cow.snap, self.cow.snap_crcs, self.cow.bitmap,
              self.cow.copied, self.cow.stale, self.clone.clone_slot, self.clone.bitmap, self.clone.claim,
              self.clone.pasted]
        return [t.cpu().numpy().copy() for t in ts]

    def scrub(self, cow=True, clone=True, max_list=None):
        """One cc_scrub_dev call on the rig's running counters (no host sync)."""
        n = self.max_list if max_list is None else max_list
        self.C.scrub_records(self.pool, self.crcs, self.h.cb, self.counts, self.list.t[:n] if n else None, self.per.t,
                             cow=self.cow if cow else None, clone=self.clone if clone else None,
                             page_bytes=self.h.pb, stream=self.stream)

    def results(self, max_list=None):
        """(counts dict, the entries stored, the per-chunk array) after a sync."""
        if self.stream is not None:
            self.stream.synchronize()
        n = self.max_list if max_list is None else max_list
        cnt = dict(zip(COUNTS, (int(v) for v in self.counts.cpu().numpy())))
        lst = self.list.t.cpu().numpy()
        stored = min(cnt["listed"], n)
        assert (lst[stored:] == LIST_SENT).all(), "an entry at or past max_list, or past the cursor"
        assert self.list.guards_ok() and self.per.guards_ok()
        return cnt, [int(v) for v in lst[:stored].view(np.uint64)], self.per.t.cpu().numpy().view(np.uint32).reshape(-1, 2)

    def check(self, cow=True, clone=True):
        """A fresh call against the model; the read-only state compared around it."""
        self.counts.zero_()
        self.per.t.zero_()
        self.list.t.fill_(LIST_SENT)
        before = self.frozen()
        self.scrub(cow=cow, clone=clone)
        cnt, ent, per = self.results()
        want, went, wper = self.model(cow=cow, clone=clone)
        print("scrub:", cnt, "model:", want)
        assert cnt == want
        assert len(set(ent)) == len(ent) and set(ent) == went
        assert (per == wper).all()
        for a, b in zip(before, self.frozen()):
            assert (a == b).all(), "the call wrote something it may only read"
        return cnt, ent, per

    def flip_byte(self, p, at=0):
        self.h.pool[p * self.h.pb + at] ^= 0x10

    def flip_crc(self, p):
        self.h.crcs[p] ^= np.uint32(0x400)

    def flip_snap_byte(self, s, q, at=0):
        self.h.cow.snap[s, q * self.h.pb + at] ^= 0x01

    def flip_snap_crc(self, s, q):
        self.h.cow.snap_crcs[s, q] ^= np.uint32(0x80000000)


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("pb", PAGE_SIZES)
def test_clean_rig_every_page_size(dev, oracle, pb):
    from curve_amd.scan import DevicePool
    rig = DevRig(dev, oracle, pb, 70 + pb // 256)
    cnt, ent, per = rig.check()
    h = rig.h
    assert cnt["live_bad"] == cnt["snap_bad"] == cnt["listed"] == 0 and not ent and not per.any()
    assert cnt["live_checked"] + cnt["unwritten"] == h.n_pages and cnt["unwritten"] > 0
    assert cnt["snap_checked"] == sum(popcount_valid(h.cow.bitmap, s, h.ppc) for s in (0, 2)) > 0
    # the gap this closes: the plain page pass against the same table reports every never-written page
    pool = DevicePool.__new__(DevicePool)
    pool.data, pool.page_crcs, pool.page_bytes, pool.chunk_size = rig.pool, rig.crcs, pb, h.cb
    plain = pool.bad_pages(rig.crcs, max_bad=h.n_pages)
    assert sorted(c * h.ppc + q for c, q in plain) == h.classes()["unwritten"]
    res = pool.scrub(cow=rig.cow, clone=rig.clone)
    assert res.clean and res.unwritten == len(plain) and res.live_bad_pages == [] and res.snap_bad_pages == []


# --------------------------------------------------------------------------- 2
def positions(h):
    """The named positions by class: the pool's first and last page, a chunk's first and last page, the pages at
    bits 31, 32 and 39 of a slot."""
    return [0, h.n_pages - 1] + [c * h.ppc + q for c in range(h.n_chunks) for q in (0, 31, 32, h.ppc - 1)]


@pytest.mark.parametrize("what", ["byte", "crc"])
@pytest.mark.parametrize("pb", [256, 4096])
def test_one_flip_in_every_page_class(dev, oracle, pb, what):
    rig = DevRig(dev, oracle, pb, 81)
    h = rig.h
    # the bits at the named positions are forced so that every class has a page at each of them
    for s in range(h.clone.n_slots):
        for q, v in ((0, 1), (31, s & 1), (32, 1 - (s & 1)), (39, 1), (1, 0), (38, 0)):
            w = np.uint32(1 << (q % 32))
            h.clone.bitmap[s, q // 32] = (h.clone.bitmap[s, q // 32] & ~w) | (w if v else np.uint32(0))
    for s in range(h.cow.n_slots):
        for q, v in ((0, 1), (31, 1), (32, 1), (39, 1), (1, 0), (30, 0), (33, 0), (38, 0)):
            w = np.uint32(1 << (q % 32))
            h.cow.bitmap[s, q // 32] = (h.cow.bitmap[s, q // 32] & ~w) | (w if v else np.uint32(0))
    # the tables again for the forced bits: written pages get their CRC back, set snapshot bits get bytes and a CRC
    true = oracle.page_crcs(h.pool, pb)
    rng = np.random.default_rng(5)
    for c in range(h.n_chunks):
        cs, s = int(h.clone.clone_slot[c]), int(h.cow.snap_slot[c])
        for q in range(h.ppc):
            never = cs < h.clone.n_slots and not bit(h.clone.bitmap, cs, q)
            h.crcs[c * h.ppc + q] = CRC_SENT if never else true[c * h.ppc + q]
            if s < h.cow.n_slots:
                if bit(h.cow.bitmap, s, q):
                    h.cow.snap[s, q * pb:(q + 1) * pb] = rng.integers(0, 256, pb, dtype=np.uint8)
                    h.cow.snap_crcs[s, q] = oracle.crc32c(h.cow.snap[s, q * pb:(q + 1) * pb].tobytes())
                else:
                    h.cow.snap_crcs[s, q] = CRC_SENT
    cls = h.classes()
    named = set(positions(h))
    expect_live, expect_snap = set(), set()
    for kind in ("ordinary", "written", "unwritten"):
        hit = [p for p in cls[kind] if p in named]
        assert len(hit) >= 3, kind
        for p in hit:
            rig.flip_byte(p, at=(p * 7) % pb) if what == "byte" else rig.flip_crc(p)
            if kind != "unwritten":
                expect_live.add(p)
    for kind in ("snap_set", "snap_clear"):
        hit = [(s, q, p) for s, q, p in cls[kind] if q in (0, 1, 30, 31, 32, 33, 38, 39)]
        assert len(hit) >= 6, kind
        for s, q, p in hit:
            rig.flip_snap_byte(s, q, at=(q * 5) % pb) if what == "byte" else rig.flip_snap_crc(s, q)
            if kind == "snap_set":
                expect_snap.add(SNAP | p)
    for s, q, _ in cls["unnamed"]:
        rig.flip_snap_byte(s, q) if what == "byte" else rig.flip_snap_crc(s, q)
    assert {0, h.n_pages - 1} <= expect_live | set(cls["unwritten"])
    rig.upload()
    cnt, ent, per = rig.check()
    assert set(ent) == expect_live | expect_snap
    assert cnt["live_bad"] == len(expect_live) and cnt["snap_bad"] == len(expect_snap)


# --------------------------------------------------------------------------- 3
def test_thirty_corruptions_and_a_list_of_seven(dev, oracle):
    from test_scrub import corrupt_some
    rig = DevRig(dev, oracle, 512, 83, max_list=7)
    corrupt_some(rig.h, np.random.default_rng(9), n=30)
    rig.upload()
    want, went, wper = rig.model()
    assert want["listed"] > 7 and want["live_bad"] and want["snap_bad"]
    rig.scrub()
    cnt, ent, per = rig.results()
    print("scrub:", cnt, "model:", want)
    assert cnt == want and (per == wper).all()
    assert len(ent) == 7 and len(set(ent)) == 7 and set(ent) <= went
    # a second call on the same counters continues the cursor: += everywhere, nothing more stored
    rig.scrub()
    cnt2, ent2, per2 = rig.results()
    assert cnt2 == {k: 2 * v for k, v in want.items()} and ent2 == ent and (per2 == 2 * wper).all()


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("cow,clone", [(False, True), (True, False), (False, False)])
def test_either_struct_alone_and_neither(dev, oracle, cow, clone):
    from test_scrub import corrupt_some
    rig = DevRig(dev, oracle, 1024, 84, max_list=512)
    corrupt_some(rig.h, np.random.default_rng(10), n=30)
    rig.upload()
    cnt, ent, per = rig.check(cow=cow, clone=clone)
    if not clone:
        assert cnt["unwritten"] == 0 and cnt["live_checked"] == rig.h.n_pages
        assert cnt["live_bad"] >= len(rig.h.classes()["unwritten"])       # their table words are sentinels
    if not cow:
        assert cnt["snap_checked"] == 0
    if not cow and not clone:
        # the plain call IS cc_page_verify_list_dev: the same count and the same set
        c2, lst = rig.C.page_verify_list(rig.pool, rig.crcs, rig.h.pb, max_bad=512)
        n = int(c2[0])
        assert n == cnt["live_bad"] == cnt["listed"] and sorted(lst[:n].cpu().tolist()) == sorted(ent)
        # ... also when the list overflows: the counts and the per-chunk words stay exact
        rig.counts.zero_()
        rig.per.t.zero_()
        rig.list.t.fill_(LIST_SENT)
        rig.scrub(cow=False, clone=False, max_list=5)
        cnt5, ent5, per5 = rig.results(max_list=5)
        assert cnt5 == cnt and (per5 == per).all() and len(set(ent5)) == 5 and set(ent5) <= set(ent)


# --------------------------------------------------------------------------- 5
def shape_rig(dev, oracle, n_chunks, ppc, pb=256, seed=90, snap_density=0.25, clone_density=0.3, all_clone=False,
              snaps=True):
    clone_slots = list(range(n_chunks)) if all_clone else [NOT_CLONE if c % 3 else c // 3 for c in range(n_chunks)]
    n_clone = n_chunks if all_clone else (n_chunks + 2) // 3
    snap_slots = [n_chunks - 1 - c for c in range(n_chunks)] if snaps else [NO_SNAPSHOT] * n_chunks
    return DevRig(dev, oracle, pb, seed, max_list=256, ppc=ppc, clone_slots=clone_slots, n_clone=n_clone,
                  snap_slots=snap_slots, n_snap=n_chunks, clone_density=clone_density, snap_density=snap_density)


@pytest.mark.parametrize("n_chunks,ppc", [(1, 1), (3, 33), (3, 64), (16, 256)])
def test_shapes_where_the_schedule_can_go_wrong(dev, oracle, n_chunks, ppc):
    from test_scrub import corrupt_some
    rig = shape_rig(dev, oracle, n_chunks, ppc)
    corrupt_some(rig.h, np.random.default_rng(n_chunks * ppc), n=40 if ppc > 1 else 4)
    rig.upload()
    cnt, ent, per = rig.check()
    assert cnt["live_checked"] + cnt["unwritten"] == n_chunks * ppc
    if ppc > 1:
        assert cnt["live_bad"] and cnt["snap_bad"]


@pytest.mark.parametrize("snap_density", [0.0, 1.0])
def test_a_large_pool_with_the_snapshot_half_empty_and_full(dev, oracle, snap_density):
    from test_scrub import corrupt_some
    rig = shape_rig(dev, oracle, 16, 256, seed=91, snap_density=snap_density)
    corrupt_some(rig.h, np.random.default_rng(3), n=40)
    rig.upload()
    cnt, ent, per = rig.check()
    assert cnt["snap_checked"] == (4096 if snap_density else 0)
    assert cnt["live_bad"] and bool(cnt["snap_bad"]) == bool(snap_density)


def test_an_all_clone_pool_with_every_bit_clear_hashes_nothing(dev, oracle):
    rig = shape_rig(dev, oracle, 16, 256, seed=92, clone_density=0.0, all_clone=True, snaps=False)
    rig.h.pool[:] = 0x33                                          # every page disagrees with its (sentinel) table word
    rig.upload()
    cnt, ent, per = rig.check()
    assert cnt == dict(zip(COUNTS, (0, 0, 0, 0, 4096, 0))) and not ent
    cnt, ent, per = rig.check(cow=False)
    assert cnt["unwritten"] == 4096 and cnt["live_checked"] == 0


# --------------------------------------------------------------------------- 6
def test_agrees_with_the_read_calls(dev, oracle):
    from test_scrub import corrupt_some
    rig = DevRig(dev, oracle, 2048, 85, max_list=512)
    corrupt_some(rig.h, np.random.default_rng(12), n=40)
    rig.upload()
    h, C = rig.h, rig.C
    cnt, ent, per = rig.check()
    # cc_read_merge_dev over one read a chunk: the same live_bad and unwritten, per chunk too
    offs = [c * h.cb for c in range(h.n_chunks)]
    _, _, bad, total, unw, unw_total = C.read_merge(rig.pool, rig.crcs, offs, [h.cb] * h.n_chunks, rig.clone,
                                                    page_bytes=h.pb)
    assert (int(total[0]), int(unw_total[0])) == (cnt["live_bad"], cnt["unwritten"])
    assert (bad.cpu().numpy().view(np.uint32) == per[:, 0]).all()
    # cc_read_snap_dev, verify only, over the set-bit pages of the mapped chunks: the same snap_bad
    pages = [p for _, _, p in h.classes()["snap_set"]]
    _, sbad, stotal = C.read_snap(rig.pool, rig.crcs, [p * h.pb for p in pages], [h.pb] * len(pages), rig.cow,
                                  page_bytes=h.pb, copy=False)
    assert int(stotal[0]) == cnt["snap_bad"] == len([e for e in ent if e & SNAP])
    assert {SNAP | p for p, b in zip(pages, sbad.cpu().tolist()) if b} == {e for e in ent if e & SNAP}


# --------------------------------------------------------------------------- 7
def test_two_streams_scrub_two_rigs_at_once(dev, oracle):
    from test_scrub import corrupt_some
    rigs = []
    for k in range(2):
        s = torch.cuda.Stream(device=dev)
        rig = shape_rig(dev, oracle, 16, 256, seed=93 + k, snap_density=0.1 + 0.5 * k)
        corrupt_some(rig.h, np.random.default_rng(20 + k), n=40)
        rig.stream = s
        rig.upload()
        rigs.append(rig)
    for _ in range(3):
        for rig in rigs:
            rig.scrub()
    for rig in rigs:
        cnt, ent, per = rig.results()
        want, went, wper = rig.model()
        assert cnt == {k: 3 * v for k, v in want.items()} and (per == 3 * wper).all()
        assert set(ent) == went and len(ent) == 3 * len(went)


def test_a_scrub_enqueued_behind_a_queue_sees_its_result(dev, oracle):
    pb = 1024
    s = torch.cuda.Stream(device=dev)
    rig = DevRig(dev, oracle, pb, 86, stream=s)
    h, C = rig.h, rig.C
    cls = h.classes()
    never = [p for p in cls["unwritten"] if p // h.ppc == 0][:5]  # five never-written pages of clone chunk 0
    broken = cls["ordinary"][3]                                   # an ordinary page, corrupt before the queue
    rig.flip_byte(broken, at=17)
    rig.upload()
    before, _, _ = rig.model()
    assert before["live_bad"] == 1
    src = np.random.default_rng(4).integers(0, 256, 8 * pb, dtype=np.uint8)
    with C._on_stream(s):
        d_src = to_dev(src, dev)
        pastes = C.log_records([p * pb for p in never], [k * pb for k in range(5)], [pb] * 5)
        writes = C.log_records([broken * pb], [6 * pb], [pb])
        d_pastes = to_dev(pastes.view(np.uint8), dev)
        d_writes = to_dev(writes.view(np.uint8), dev)
    C.apply_ops(rig.pool, rig.crcs, [("paste", d_src, d_pastes, 5), ("write", d_src, d_writes, 1)], pb, pb,
                page_bytes=pb, stream=s, clone=rig.clone)
    rig.scrub()                                                   # no host sync between the two
    cnt, ent, per = rig.results()
    # the host mirror of the queue: five pages pasted (bytes, CRC word, bit), one page overwritten whole
    for k, p in enumerate(never):
        h.pool[p * pb:(p + 1) * pb] = src[k * pb:(k + 1) * pb]
        h.crcs[p] = oracle.crc32c(src[k * pb:(k + 1) * pb].tobytes())
        h.clone.bitmap[int(h.clone.clone_slot[0]), (p % h.ppc) // 32] |= np.uint32(1 << (p % h.ppc % 32))
    h.pool[broken * pb:(broken + 1) * pb] = src[6 * pb:7 * pb]
    h.crcs[broken] = oracle.crc32c(src[6 * pb:7 * pb].tobytes())
    want, went, wper = rig.model()
    assert cnt == want and not ent and not per.any()
    assert want["unwritten"] == before["unwritten"] - 5 and want["live_bad"] == 0


# --------------------------------------------------------------------------- 8
def test_scrub_repair_on_a_pool_with_clone_chunks(dev, oracle):
    from curve_amd.scan import DevicePool
    pb = 4096
    rig = DevRig(dev, oracle, pb, 87)
    h, C = rig.h, rig.C
    cls = h.classes()
    good = h.pool.copy()                                          # the peer's copy
    mend = [cls["written"][0], cls["written"][-1], cls["ordinary"][5]]
    for p in mend:
        rig.flip_byte(p, at=p % pb)
    ignored = cls["unwritten"][2]
    rig.flip_byte(ignored)
    s, q, sp = cls["snap_set"][1]
    rig.flip_snap_byte(s, q, at=9)
    rig.upload()
    pool = DevicePool.__new__(DevicePool)
    pool.data, pool.page_crcs, pool.page_bytes, pool.chunk_size = rig.pool, rig.crcs, pb, h.cb
    peer = to_dev(good, dev)
    asked = []

    def fetch(pages):
        asked.append([int(p) for p in pages])
        return peer, [int(p) * pb for p in pages]

    repaired, still, snap_bad = pool.scrub_repair([fetch], cow=rig.cow, clone=rig.clone)
    ppc = h.ppc
    assert asked == [sorted(mend)]
    assert repaired == [(p // ppc, p % ppc, 0) for p in sorted(mend)] and still == []
    assert snap_bad == [(sp // ppc, sp % ppc)]
    got = rig.pool.cpu().numpy()
    for p in mend:
        assert (got[p * pb:(p + 1) * pb] == good[p * pb:(p + 1) * pb]).all()
        h.pool[p * pb:(p + 1) * pb] = good[p * pb:(p + 1) * pb]
    assert (got == h.pool).all()                                  # the never-written page was left as it was
    assert (rig.cow.snap.cpu().numpy() == h.cow.snap[:h.cow.n_slots]).all()     # and the snapshot page too
    cnt, ent, per = rig.check()
    assert ent == [SNAP | sp] and cnt["live_bad"] == 0 and cnt["snap_bad"] == 1
