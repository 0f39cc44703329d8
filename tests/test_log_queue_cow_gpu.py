"""cc_apply_logs_cow_dev on the GPU: the write-log queue for a pool with open
snapshots and clone chunks.

Every case runs on TWIN state.  State A takes the new call.  State B takes the
sequence the header defines it by: apply_log_cow + clone_mark per non-empty
batch.  Everything is compared in full -- pool, CRC table, snap, snap_crcs, both
bitmaps, copied, stale -- and the claim table must still be all ones.  Beside
the twin, the pool and the table are checked against in-order host application
with the oracle's CRCs, and the slots, bitmaps and counts against what follows
from the pre-queue pool alone (a held page = the page before the queue, every
other slot byte = the sentinel it was filled with, so a stray write shows).
"""
import ctypes

import numpy as np
import pytest

from test_clone import mark_model
from test_log_cow import NO_SNAPSHOT, SENT_BYTE, SENT_CRC, entry_ok

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_CHUNKS = 16
#            0  1           2  3           4  5  6           7 .. 13                     14 15
SNAP_SLOT = [0, NO_SNAPSHOT, 2, NO_SNAPSHOT, 1, 9] + [NO_SNAPSHOT] * 8 + [3, NO_SNAPSHOT]  # 9: out of range
N_SLOTS = 4
CLONE_SLOT = [NO_SNAPSHOT] * 8 + [0, NO_SNAPSHOT, 1, 7] + [NO_SNAPSHOT] * 3 + [2]          # 7: out of range
N_CLONE = 3
PAGE_SIZES = [256, 512, 1024, 2048, 4096, 8192]
MIXED = [70, 0, 5, 300, 64, 65, 1]   # table path, one-launch path, an empty batch, the 64 / 65 boundary


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


# --------------------------------------------------------------------------- queues
def random_batch(rng, n, pb, max_len, span):
    """n entries below `span`: any alignment and length, a third of them whole pages (so
    clone bits get set)."""
    lens = rng.integers(1, max_len + 1, n).astype(np.uint32)
    dst = rng.integers(0, span - max_len, n).astype(np.uint64)
    whole = rng.integers(0, 3, n) == 0
    k = rng.integers(1, max_len // pb + 1, n).astype(np.uint32)
    lens[whole] = k[whole] * pb
    dst[whole] = dst[whole] // pb * pb
    src = rng.integers(0, 256, (1 << 16) + max_len, dtype=np.uint8)
    src_off = rng.integers(0, 1 << 16, n).astype(np.uint64)
    return [dst, src_off, lens, src]


def random_queue(rng, sizes, pb, ppc, max_len, span=None):
    pool_bytes = N_CHUNKS * ppc * pb
    return [random_batch(rng, n, pb, max_len, span or pool_bytes) for n in sizes]


def host_apply(host, queue, max_len):
    for dst, so, ln, src in queue:
        for d, s, n in zip(dst, so, ln):
            d, s, n = int(d), int(s), int(n)
            if entry_ok(d, n, max_len, host.size):
                host[d:d + n] = src[s:s + n]


def touched(queue, max_len, pool_bytes, pb):
    out = set()
    for dst, _, ln, _ in queue:
        for d, n in zip(dst, ln):
            d, n = int(d), int(n)
            if entry_ok(d, n, max_len, pool_bytes):
                out.update(range(d // pb, (d + n - 1) // pb + 1))
    return out


# --------------------------------------------------------------------------- twin state
class State:
    def __init__(self, dev, orig, crcs, pb, ppc, bm, cbm, verify, stream):
        from curve_amd import crc as C
        cb = ppc * pb
        with C._on_stream(stream):
            self.pool, self.crcs = to_dev(orig, dev), to_dev(i32(crcs), dev)
            self.cow = C.Cow(N_CHUNKS, cb, pb, N_SLOTS, device=dev, verify=verify, fill=SENT_BYTE,
                             crc_fill=int(np.uint32(SENT_CRC).view(np.int32)))
            self.cow.snap_slot.copy_(to_dev(i32(SNAP_SLOT), dev))
            self.cow.bitmap.copy_(to_dev(i32(bm), dev))
            self.clone = C.Clone(N_CHUNKS, cb, pb, N_CLONE, device=dev)
            self.clone.clone_slot.copy_(to_dev(i32(CLONE_SLOT), dev))
            self.clone.bitmap.copy_(to_dev(i32(cbm), dev))

    def arrays(self):
        out = {"pool": self.pool.cpu().numpy(), "crcs": u32(self.crcs), "snap": self.cow.snap.cpu().numpy(),
               "snap_crcs": u32(self.cow.snap_crcs), "bitmap": u32(self.cow.bitmap),
               "copied": self.cow.copied.cpu().numpy(), "clone_bitmap": u32(self.clone.bitmap),
               "claim": u32(self.clone.claim), "pasted": self.clone.pasted.cpu().numpy()}
        if self.cow.stale is not None:
            out["stale"] = self.cow.stale.cpu().numpy()
        return out


def raw_logs_cow(pool, crcs, dev_q, max_len, pb, delta, cow=None, clone=None, stream=None):
    """cc_apply_logs_cow_dev itself (crc.apply_logs takes the plain symbol when both structs are None)."""
    from curve_amd import _lib
    from curve_amd import crc as C
    L = _lib.lib()
    need = int(L.cc_apply_logs_work_bytes(max(max(n for _, _, n in dev_q), 1), max_len, pb))
    assert need > 0
    with C._on_stream(stream):
        work = torch.empty(need, dtype=torch.uint8, device=pool.device)
    arr = (_lib.CcLogBatch * len(dev_q))()
    for i, (src, d_log, n) in enumerate(dev_q):
        arr[i].d_src, arr[i].d_log, arr[i].n_updates = (src.data_ptr(), d_log.data_ptr(), n) if n else (None, None, 0)
    ws = cow.struct() if cow is not None else None
    ls = clone.struct() if clone is not None else None
    rc = L.cc_apply_logs_cow_dev(C._dev_ptr(pool, "pool"), C._nbytes(pool), pb, ctypes.cast(arr, ctypes.c_void_p),
                                 len(dev_q), max_len, C._dev_ptr(crcs, "crcs"), 1 if delta else 0,
                                 C._dev_ptr(work, "work"), work.numel(), C._stream_handle(stream),
                                 ctypes.byref(ws) if ws is not None else None,
                                 ctypes.byref(ls) if ls is not None else None)
    assert rc == _lib.CC_OK, rc
    torch.cuda.synchronize()


class Twin:
    """Pre-queue pool, CRC table and bitmaps; state A and state B on the device."""

    def __init__(self, dev, oracle, pb, ppc=40, preset="random", seed=1, verify=False, stream=None, corrupt=()):
        self.dev, self.oracle, self.pb, self.ppc, self.stream = dev, oracle, pb, ppc, stream
        self.cb = ppc * pb
        rng = np.random.default_rng(seed)
        self.orig = rng.integers(0, 256, N_CHUNKS * self.cb, dtype=np.uint8)
        self.orig_crcs = oracle.page_crcs(self.orig, pb)
        for p in corrupt:                      # behind the table's back: the stored CRC no longer matches
            self.orig[p * pb + 17 + p % 100] ^= 0x40
        words = (ppc + 31) // 32
        full = np.zeros(words, np.uint32)
        for q in range(ppc):
            full[q // 32] |= np.uint32(1 << (q % 32))
        self.bm0, self.cbm0 = np.zeros((N_SLOTS, words), np.uint32), np.zeros((N_CLONE, words), np.uint32)
        if preset == "all":
            self.bm0[:], self.cbm0[:] = full, full
        elif preset == "random":
            self.bm0 = rng.integers(0, 1 << 32, self.bm0.shape, dtype=np.uint64).astype(np.uint32) & full
            self.cbm0 = rng.integers(0, 1 << 32, self.cbm0.shape, dtype=np.uint64).astype(np.uint32) & full
        self.A = State(dev, self.orig, self.orig_crcs, pb, ppc, self.bm0, self.cbm0, verify, stream)
        self.B = State(dev, self.orig, self.orig_crcs, pb, ppc, self.bm0, self.cbm0, verify, stream)
        self.host = self.orig.copy()
        self.queues = []

    def upload(self, queue):
        from curve_amd import crc as C
        with C._on_stream(self.stream):
            return [(to_dev(src, self.dev), torch.from_numpy(C.log_records(d, so, ln).view(np.uint8)).to(self.dev),
                     len(ln)) for d, so, ln, src in queue]

    def run(self, queue, max_len, delta, mode="both", model=True):
        """mode: which structs the calls get -- both, cow, clone or none.  model=False: no
        entry-by-entry host application (a log too long for it; check(model=False) then)."""
        from curve_amd import crc as C
        self.max_len, self.mode = max_len, mode
        dev_q = self.upload(queue)
        cow = lambda st: st.cow if mode in ("both", "cow") else None      # noqa: E731
        clone = lambda st: st.clone if mode in ("both", "clone") else None  # noqa: E731
        if mode == "none":
            raw_logs_cow(self.A.pool, self.A.crcs, dev_q, max_len, self.pb, delta, stream=self.stream)
            C.apply_logs(self.B.pool, self.B.crcs, dev_q, max_len, self.pb, stream=self.stream, delta=delta)
        else:
            C.apply_logs(self.A.pool, self.A.crcs, dev_q, max_len, self.pb, stream=self.stream, delta=delta,
                         cow=cow(self.A), clone=clone(self.A))
            for src, d_log, n in dev_q:
                if n == 0:
                    continue
                C.apply_log_cow(self.B.pool, self.B.crcs, src, d_log, n, max_len, cow(self.B), self.pb,
                                stream=self.stream, delta=delta)
                if clone(self.B) is not None:
                    C.clone_mark(self.B.pool, d_log, n, max_len, self.B.clone, self.pb, stream=self.stream)
        if model:
            host_apply(self.host, queue, max_len)
        self.queues.append(queue)

    def check(self, clean=True, model=True):
        """Twin equality in full, then the host's own expectations.  Returns state A's arrays."""
        if self.stream is not None:
            self.stream.synchronize()
        else:
            torch.cuda.synchronize()
        pb, ppc = self.pb, self.ppc
        a, b = self.A.arrays(), self.B.arrays()
        assert sorted(a) == sorted(b)
        for k in a:
            assert (a[k] == b[k]).all(), k
        assert (a["claim"] == 0xFFFFFFFF).all() and int(a["pasted"][0]) == 0
        if not model:
            return a
        assert (a["pool"] == self.host).all()
        if clean:
            assert (a["crcs"] == self.oracle.page_crcs(self.host, pb)).all()
        everything = [b for q in self.queues for b in q]
        tp = touched(everything, self.max_len, self.orig.size, pb)
        want_bm, copied = self.bm0.copy(), 0
        snap = a["snap"].reshape(N_SLOTS, ppc, pb)
        for c, s in enumerate(SNAP_SLOT):
            if s >= N_SLOTS:
                continue
            for q in range(ppc):
                p = c * ppc + q
                held = (int(self.bm0[s, q // 32]) >> (q % 32)) & 1
                if self.mode in ("both", "cow") and p in tp and not held:
                    want_bm[s, q // 32] |= np.uint32(1 << (q % 32))
                    copied += 1
                    assert (snap[s, q] == self.orig[p * pb:(p + 1) * pb]).all(), (c, q)   # the page before the queue
                    assert a["snap_crcs"][s, q] == self.orig_crcs[p], (c, q)               # and its stored CRC, moved
                else:
                    assert (snap[s, q] == SENT_BYTE).all() and a["snap_crcs"][s, q] == SENT_CRC, (c, q)
        assert (a["bitmap"] == want_bm).all() and int(a["copied"][0]) == copied
        want_cbm = self.cbm0.copy()
        if self.mode in ("both", "clone"):
            for dst, so, ln, _ in everything:
                mark_model([(int(d), 0, int(n)) for d, n in zip(dst, ln)], self.max_len, self.orig.size,
                           np.array(CLONE_SLOT, np.uint32), N_CLONE, want_cbm, pb, self.cb)
        assert (a["clone_bitmap"] == want_cbm).all()
        a["copied_n"] = copied
        return a


# --------------------------------------------------------------------------- cases
def add_fixed_entries(queue, pb, cb):
    """An entry from chunk 0 (slot 0) into chunk 1 (no snapshot), one inside chunk 5 (slot out of
    range), one from clone chunk 8 into chunk 9 (not a clone), one inside chunk 11 (clone slot out
    of range): into the first batch."""
    b = queue[0]
    for i, (d, n) in enumerate(((cb - 10, 20), (5 * cb + 3 * pb + 5, 30), (9 * cb - pb, pb), (11 * cb + pb, pb))):
        b[0][i], b[2][i] = d, n


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("pb", PAGE_SIZES)
def test_mixed_queue_all_page_sizes(dev, oracle, pb, long, delta):
    """Batches of [70, 0, 5, 300, 64, 65, 1] entries, writes of up to one page or up to 3 pages + 7
    bytes, 16 chunks of 40 pages, random bits held before the call, both structs."""
    max_len = 3 * pb + 7 if long else pb
    tw = Twin(dev, oracle, pb, seed=pb + long)
    rng = np.random.default_rng(pb * 4 + long * 2 + delta)
    queue = random_queue(rng, MIXED, pb, 40, max_len)
    add_fixed_entries(queue, pb, tw.cb)
    tw.run(queue, max_len, delta)
    a = tw.check()
    assert a["copied_n"] > 20


@pytest.mark.parametrize("pb,ppc", [(4096, 8), (512, 64)])
def test_chunks_of_8_and_64_pages(dev, oracle, pb, ppc):
    """A sub-word bitmap and exactly two words a slot."""
    tw = Twin(dev, oracle, pb, ppc=ppc, seed=ppc)
    rng = np.random.default_rng(ppc)
    queue = random_queue(rng, MIXED, pb, ppc, pb)
    add_fixed_entries(queue, pb, tw.cb)
    tw.run(queue, pb, True)
    tw.check()


@pytest.mark.parametrize("delta", [False, True])
def test_forty_one_entry_batches(dev, oracle, delta):
    """More batches than one pre-pass launch holds (32): two launches, every batch one entry."""
    pb = 4096
    tw = Twin(dev, oracle, pb, preset="none", seed=40)
    rng = np.random.default_rng(400 + delta)
    queue = random_queue(rng, [1] * 40, pb, 40, pb)
    for k, b in enumerate(queue):             # slotted chunks 0, 2, 4, 14 and clone chunks 8, 10, 15 in turn
        c = (0, 2, 4, 14, 8, 10, 15)[k % 7]
        b[0][0], b[2][0] = c * tw.cb + (k % 40) * pb, pb
    tw.run(queue, pb, delta)
    a = tw.check()
    assert a["copied_n"] == len([k for k in range(40) if k % 7 < 4])


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("mode", ["cow", "clone", "both", "none"])
def test_either_struct_both_or_neither(dev, oracle, mode, delta):
    """cow only, clone only, both (on different chunks) and neither; with neither, state B is
    apply_logs on the same queue and nothing but the pool and the table may change."""
    pb = 2048
    tw = Twin(dev, oracle, pb, seed=7)
    rng = np.random.default_rng(70 + delta)
    queue = random_queue(rng, MIXED, pb, 40, pb + 300)
    add_fixed_entries(queue, pb, tw.cb)
    tw.run(queue, pb + 300, delta, mode=mode)
    a = tw.check()
    assert (a["copied_n"] > 0) == (mode in ("cow", "both"))
    if mode in ("clone", "none"):
        assert (a["bitmap"] == tw.bm0).all()
    if mode in ("cow", "none"):
        assert (a["clone_bitmap"] == tw.cbm0).all()


@pytest.mark.parametrize("delta", [False, True])
def test_one_page_touched_by_four_batches_and_twice_in_one(dev, oracle, delta):
    """The slot holds the page as it stood before the queue, with the CRC from before the queue."""
    pb = 4096
    tw = Twin(dev, oracle, pb, preset="none", seed=9)
    rng = np.random.default_rng(90 + delta)
    queue = random_queue(rng, [70, 66, 5, 0, 100], pb, 40, pb, span=tw.cb)     # everything else in chunk 0 ...
    page = 2 * tw.cb // pb + 17                                                # ... the page: 17 of chunk 2 (slot 2)
    for k in (0, 1, 2, 4):
        queue[k][0][3], queue[k][2][3] = page * pb + 100 * k, 900
    queue[1][0][50], queue[1][2][50] = page * pb + 2000, 2000                  # twice inside batch 1
    tw.run(queue, pb, delta)
    a = tw.check()
    assert (a["snap"][2].reshape(40, pb)[17] == tw.orig[page * pb:(page + 1) * pb]).all()
    assert a["snap_crcs"][2, 17] == tw.orig_crcs[page] != a["crcs"][page]
    assert int(a["bitmap"][2, 0]) == 1 << 17 and int(a["bitmap"][2, 1]) == 0


@pytest.mark.parametrize("preset", ["none", "all", "random"])
def test_bits_held_before_the_call(dev, oracle, preset):
    pb = 1024
    tw = Twin(dev, oracle, pb, preset=preset, seed=11)
    rng = np.random.default_rng(110)
    queue = random_queue(rng, [300, 70, 64], pb, 40, pb)
    tw.run(queue, pb, True)
    a = tw.check()
    if preset == "all":
        assert a["copied_n"] == 0 and (a["snap"] == SENT_BYTE).all()


@pytest.mark.parametrize("pb", [256, 4096, 8192])
def test_stale_counts_two_corrupted_pages(dev, oracle, pb):
    """Two pages the queue touches (in different batches) and one it does not were corrupted
    behind the table: d_stale is 2, both sit in their slots with the stored CRC."""
    ppc = 40
    hit, miss = [0 * ppc + 3, 14 * ppc + 39], 4 * ppc + 1
    tw = Twin(dev, oracle, pb, preset="none", seed=13, verify=True, corrupt=hit + [miss])
    rng = np.random.default_rng(130)
    queue = random_queue(rng, [70, 5, 90], pb, ppc, pb, span=4 * tw.cb)        # chunks 0..3; chunk 4 stays untouched
    queue[0][0][0], queue[0][2][0] = hit[0] * pb + 9, 100
    queue[2][0][0], queue[2][2][0] = hit[1] * pb, pb
    tw.run(queue, pb, True)
    a = tw.check(clean=False)
    assert int(a["stale"][0]) == 2
    for p, s in ((hit[0], 0), (hit[1], 3)):
        q = p % ppc
        got = a["snap"][s].reshape(ppc, pb)[q]
        assert (got == tw.orig[p * pb:(p + 1) * pb]).all() and a["snap_crcs"][s, q] == tw.orig_crcs[p]
        assert oracle.crc32c(got.tobytes()) != int(a["snap_crcs"][s, q])


@pytest.mark.parametrize("delta", [False, True])
def test_invalid_entries_in_first_middle_and_last_batch(dev, oracle, delta):
    """len 0, len > max_len, past the pool's end and far beyond it, aimed at a slotted chunk (14)
    and a clone chunk (15) nothing else touches: nothing copied, nothing marked there."""
    pb = 4096
    tw = Twin(dev, oracle, pb, preset="none", seed=15)
    rng = np.random.default_rng(150 + delta)
    max_len = 2 * pb
    queue = random_queue(rng, [80, 70, 5, 64], pb, 40, max_len, span=14 * tw.cb)
    total = tw.orig.size
    bad = [(14 * tw.cb + 3 * pb, 0), (14 * tw.cb + 5 * pb, max_len + 1), (15 * tw.cb + 2 * pb, 3 * pb),
           (total - pb, pb + 1), (total, 1), (1 << 40, 8), ((1 << 64) - 4, 8)]
    for k in (0, 1, 3):
        for i, (d, n) in enumerate(bad[:4] if k == 1 else bad):
            queue[k][0][10 + i], queue[k][2][10 + i] = d, n
    tw.run(queue, max_len, delta)
    a = tw.check()
    assert not a["bitmap"][3].any() and not a["clone_bitmap"][2].any() and a["copied_n"] > 0


def test_clone_marks_need_whole_page_coverage(dev, oracle):
    """Whole-page coverage sets the bit; a partly covered page keeps its bit; two partial entries
    that together cover a page do not set it -- whichever batches they sit in."""
    pb = 512
    tw = Twin(dev, oracle, pb, preset="none", seed=17)
    rng = np.random.default_rng(170)
    queue = random_queue(rng, [66, 70], pb, 40, 3 * pb + 7, span=8 * tw.cb)    # random entries: no clone chunk
    base = 8 * tw.cb                                                           # chunk 8: clone slot 0
    for k, i, d, n in ((0, 0, base + 2 * pb, pb),                  # page 2 whole
                       (0, 1, base + 5 * pb - 1, pb + 2),          # page 5 whole, 4 and 6 by one byte
                       (1, 0, base + 10 * pb + 1, 3 * pb + 6),     # pages 11, 12 whole, 10 and 13 partly
                       (0, 2, base + 20 * pb, pb // 2),            # page 20: two halves, one a batch
                       (1, 1, base + 20 * pb + pb // 2, pb // 2),
                       (1, 2, base + 30 * pb, pb - 1)):            # page 30 but its last byte
        queue[k][0][i], queue[k][2][i] = d, n
    tw.run(queue, 3 * pb + 7, False)
    a = tw.check()
    want = sum(1 << q for q in (2, 5, 11, 12))
    assert int(a["clone_bitmap"][0, 0]) == want and int(a["clone_bitmap"][0, 1]) == 0


def test_reads_after_the_call(dev, oracle):
    """read_snap through the slots returns the chunks as they were before the queue, with 0 bad
    pages; verify_reads of the live pool reports 0 bad pages."""
    from curve_amd import crc as C
    pb = 4096
    tw = Twin(dev, oracle, pb, preset="none", seed=19)
    rng = np.random.default_rng(190)
    queue = random_queue(rng, MIXED, pb, 40, pb)
    tw.run(queue, pb, True)
    tw.check()
    slotted = [c for c, s in enumerate(SNAP_SLOT) if s < N_SLOTS]
    offs, lens = [c * tw.cb for c in slotted], [tw.cb] * len(slotted)
    out, bad, total = C.read_snap(tw.A.pool, tw.A.crcs, offs, lens, tw.A.cow, pb)
    vbad, vtotal = C.verify_reads(tw.A.pool, tw.A.crcs, [0], [tw.orig.size], pb)
    torch.cuda.synchronize()
    assert int(total.item()) == 0 and not bad.cpu().numpy().any()
    want = np.concatenate([tw.orig[c * tw.cb:(c + 1) * tw.cb] for c in slotted])
    assert (out.cpu().numpy() == want).all()
    assert int(vtotal.item()) == 0


def test_twice_in_a_row_and_on_a_side_stream(dev, oracle):
    """A second queue right behind the first (the engine table was left clean; held pages keep
    their first version), then the same on a stream of its own."""
    pb = 4096
    for stream in (None, torch.cuda.Stream(device=dev)):
        tw = Twin(dev, oracle, pb, seed=21, stream=stream)
        rng = np.random.default_rng(210)
        first = random_queue(rng, [70, 300, 5], pb, 40, pb)
        second = random_queue(rng, [65, 0, 64, 200], pb, 40, pb)
        tw.run(first, pb, True)
        tw.run(second, pb, True)
        tw.check()


def test_a_batch_too_large_for_the_engine_table_takes_the_pass_then_one_call_a_batch(dev, oracle):
    """A 300,000-entry batch needs more table than the engine keeps for a stream twice over, so
    the queue falls back to one plain call a batch -- behind the same pass.  Twin equality in
    full; the bitmaps and the count also against the touched pages, computed vectorised."""
    pb, ppc = 256, 40
    tw = Twin(dev, oracle, pb, seed=25)
    rng = np.random.default_rng(250)
    queue = random_queue(rng, [300000, 70, 64], pb, ppc, pb)
    tw.run(queue, pb, True, model=False)
    a = tw.check(model=False)
    dst = np.concatenate([b[0] for b in queue]).astype(np.int64)
    end = dst + np.concatenate([b[2] for b in queue]).astype(np.int64) - 1       # every entry is valid
    hit = np.zeros(N_CHUNKS * ppc, bool)
    hit[dst // pb] = True
    hit[end // pb] = True                                                        # at most two pages an entry
    want_bm, copied = tw.bm0.copy(), 0
    for c, s in enumerate(SNAP_SLOT):
        if s < N_SLOTS:
            for q in np.nonzero(hit[c * ppc:(c + 1) * ppc])[0]:
                copied += not (int(tw.bm0[s, q // 32]) >> (q % 32)) & 1
                want_bm[s, q // 32] |= np.uint32(1 << (q % 32))
    assert (a["bitmap"] == want_bm).all() and int(a["copied"][0]) == copied > 0


def test_skew_every_copy_in_the_first_64_entries(dev, oracle):
    """All of batch 0's first 64 entries hit clear slotted pages, nothing else does: one wave of
    the pass does every copy (correctness only)."""
    pb = 4096
    tw = Twin(dev, oracle, pb, preset="none", seed=23)
    rng = np.random.default_rng(230)
    queue = random_queue(rng, [400, 300, 70], pb, 40, pb, span=tw.cb)          # chunk 0 only ...
    for b in queue:
        b[0][:] += np.uint64(tw.cb)                                             # ... moved to chunk 1: no snapshot
    for i in range(64):
        c = (0, 2, 4, 14)[i % 4]
        queue[0][0][i], queue[0][2][i] = c * tw.cb + (i // 4) * pb + 7 * i, 64
    tw.run(queue, pb, True)
    a = tw.check()
    assert a["copied_n"] == 64
