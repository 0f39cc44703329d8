"""cc_apply_ops_dev on the GPU: paste batches inside the write-log queue.

Every case runs on TWIN state.  State A takes the new call.  State B takes the
sequence the header defines it by: per batch, apply_log_cow + clone_mark for a
write log, paste for a paste batch.  Everything is compared in full -- pool, CRC
table, clone bitmaps, every per-entry count, the pasted total, the snapshot
arrays -- and the claim table must be all ones afterwards.  Beside the twin,
state A is checked against the host model of the contract (test_apply_ops.py's
ops_model, with the oracle's CRCs), the contested count included; a queue WITH
contested pairs is checked against the model alone, since there the sequence
differs by definition.
"""
import numpy as np
import pytest

from test_apply_ops import ops_model
from test_clone import NOT_CLONE
from test_log_cow import NO_SNAPSHOT, SENT_BYTE, SENT_CRC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

#             0  1          2  3  4          5
CLONE_SLOT = [0, NOT_CLONE, 1, 7, NOT_CLONE, 2]   # chunk 1 and 4: no clones; 3: out of range
N_CLONE = 3
SNAP_SLOT = [NO_SNAPSHOT] * 4 + [0, NO_SNAPSHOT]  # chunk 4 has an open snapshot
N_SNAP = 1
N_CHUNKS = 6
PAGE_SIZES = [256, 512, 1024, 2048, 4096, 8192]
SRC_PAGES = 160


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
# (kind, src, entries) with entries = [(dst, src offset, len)], as test_apply_ops.py's models take them
class Gen:
    def __init__(self, seed, pb, ppc, max_len, mpl):
        self.rng = np.random.default_rng(seed)
        self.pb, self.ppc, self.max_len, self.mpl = pb, ppc, max_len, mpl
        self.cb = ppc * pb
        self.pool_bytes = N_CHUNKS * self.cb
        self.n_pages = N_CHUNKS * ppc
        self.src_bytes = SRC_PAGES * pb

    def src(self):
        return self.rng.integers(0, 256, self.src_bytes, dtype=np.uint8)

    def whole_write(self, pages=None):
        """A page-aligned write of 1 .. max_len / pb pages, anywhere."""
        rng, pb = self.rng, self.pb
        n = int(rng.integers(1, max(self.max_len // pb, 1) + 1)) if pages is None else pages
        return (int(rng.integers(0, self.n_pages - n + 1)) * pb, int(rng.integers(0, self.src_bytes - self.max_len)), n * pb)

    def any_write(self, chunks=None):
        """Any alignment and length; chunks: confined to these (never crossing out of them)."""
        rng = self.rng
        ln = int(rng.integers(1, self.max_len + 1))
        if chunks is None:
            d = int(rng.integers(0, self.pool_bytes - ln + 1))
        else:
            c = int(rng.choice(chunks))
            ln = min(ln, self.cb)
            d = c * self.cb + int(rng.integers(0, self.cb - ln + 1))
        return (d, int(rng.integers(0, self.src_bytes - self.max_len)), ln)

    def paste(self, pages=None, at=None):
        rng, pb = self.rng, self.pb
        n = int(rng.integers(0, self.mpl // pb + 1)) if pages is None else pages
        p = int(rng.integers(0, self.n_pages - n + 1)) if at is None else at
        return (p * pb, int(rng.integers(0, (self.src_bytes - n * pb) // 4 + 1)) * 4, n * pb)

    def bad_writes(self):
        return [(5 * self.pb, 0, 0), (self.pb, 0, self.max_len + 1), (self.pool_bytes - 4, 0, 8), (1 << 40, 0, 4),
                (self.pool_bytes, 0, 1)]

    def bad_pastes(self):
        pb, S = self.pb, self.src_bytes
        return [(pb + 128, 0, pb), (2 * pb, 0, pb + 4), (self.pool_bytes - pb, 0, 2 * pb), (self.pool_bytes, 0, pb),
                (0, 2, pb), (0, S - pb + 4, pb), (0, S + 4, pb), (0, 0, self.mpl + pb)]

    def safe_writes(self, n):
        """n writes that cannot be contested whatever follows: whole pages anywhere, partial ones
        only in the chunks without a clone bitmap (1, 3, 4)."""
        return [self.whole_write() if self.rng.integers(0, 2) else self.any_write([1, 3, 4]) for _ in range(n)]

    def mixed(self, sizes=(64, 33, 40, 0, 25, 0, 55, 51)):
        """W P W P(empty) P W(empty) P W: duplicate pastes of one page within a batch and across
        batches, a whole write before a paste of its page and after one, a partial write after a
        paste, entries crossing chunks, every invalid rule in the first, a middle and the last
        batch of its kind, empty batches of both kinds."""
        pb, ppc = self.pb, self.ppc
        h = [5 * ppc + 1, 5 * ppc + 2, 5 * ppc + 4, 2 * ppc + 3]   # hot pages: chunks 5 and 2
        bw, bp = self.bad_writes(), self.bad_pastes()
        w0 = [(h[0] * pb, 0, pb)] + self.safe_writes(sizes[0]) + bw
        p1 = [self.paste(3, h[0]), self.paste(1, h[1]), self.paste(2, h[0]), self.paste(1, h[3])] + \
            [self.paste() for _ in range(sizes[1])] + bp
        w2 = [(h[1] * pb, pb, pb)] + self.safe_writes(sizes[2]) + bw
        p3 = []
        p4 = [self.paste(3, h[0]), self.paste(2, h[3]), self.paste(min(ppc, self.mpl // pb), ppc - 2),
              self.paste(min(4, self.mpl // pb), 3 * ppc - 2)] + [self.paste() for _ in range(sizes[4])] + bp
        w5 = []
        p6 = [self.paste(1, h[2]), self.paste(1, h[2]), self.paste(0, 0)] + [self.paste() for _ in range(sizes[6])] + bp
        # the last write batch: nothing pastes after it, so partial writes may go anywhere
        w7 = [(h[2] * pb + 7, 3, min(40, self.max_len)), (h[3] * pb + pb // 2, 9, min(pb // 2, self.max_len))] + \
            [self.any_write() for _ in range(sizes[7])] + bw
        return [("write", self.src(), w0), ("paste", self.src(), p1), ("write", self.src(), w2), ("paste", self.src(), p3),
                ("paste", self.src(), p4), ("write", self.src(), w5), ("paste", self.src(), p6), ("write", self.src(), w7)]


# --------------------------------------------------------------------------- twin state
class State:
    def __init__(self, dev, orig, crcs, pb, ppc, cbm, cow, stream):
        from curve_amd import crc as C
        cb = ppc * pb
        with C._on_stream(stream):
            self.pool, self.crcs = to_dev(orig, dev), to_dev(i32(crcs), dev)
            self.clone = C.Clone(N_CHUNKS, cb, pb, N_CLONE, device=dev)
            self.clone.clone_slot.copy_(to_dev(i32(CLONE_SLOT), dev))
            self.clone.bitmap.copy_(to_dev(i32(cbm), dev))
            self.cow = None
            if cow:
                self.cow = C.Cow(N_CHUNKS, cb, pb, N_SNAP, device=dev, verify=cow == "stale", fill=SENT_BYTE,
                                 crc_fill=int(np.uint32(SENT_CRC).view(np.int32)))
                self.cow.snap_slot.copy_(to_dev(i32(SNAP_SLOT), dev))
            self.contested = torch.zeros(1, dtype=torch.int64, device=dev)
        self.counts = []

    def arrays(self):
        out = {"pool": self.pool.cpu().numpy(), "crcs": u32(self.crcs), "clone_bitmap": u32(self.clone.bitmap),
               "claim": u32(self.clone.claim), "pasted": self.clone.pasted.cpu().numpy()}
        for k, t in enumerate(self.counts):
            out["counts%d" % k] = u32(t)
        if self.cow is not None:
            out.update({"snap": self.cow.snap.cpu().numpy(), "snap_crcs": u32(self.cow.snap_crcs),
                        "snap_bitmap": u32(self.cow.bitmap), "copied": self.cow.copied.cpu().numpy()})
            if self.cow.stale is not None:
                out["stale"] = self.cow.stale.cpu().numpy()
        return out


class Twin:
    def __init__(self, dev, oracle, pb, ppc, max_len, mpl, preset="random", seed=1, cow=None, stream=None):
        self.dev, self.oracle, self.pb, self.ppc, self.stream = dev, oracle, pb, ppc, stream
        self.max_len, self.mpl, self.cb = max_len, mpl, ppc * pb
        rng = np.random.default_rng(seed)
        self.orig = rng.integers(0, 256, N_CHUNKS * self.cb, dtype=np.uint8)
        self.orig_crcs = oracle.page_crcs(self.orig, pb)
        words = (ppc + 31) // 32
        full = np.zeros(words, np.uint32)
        for q in range(ppc):
            full[q // 32] |= np.uint32(1 << (q % 32))
        self.cbm0 = np.zeros((N_CLONE, words), np.uint32)
        if preset == "all":
            self.cbm0[:] = full
        elif preset == "random":
            self.cbm0 = rng.integers(0, 1 << 32, self.cbm0.shape, dtype=np.uint64).astype(np.uint32) & full
        elif preset != "none":
            self.cbm0[:] = preset                              # an explicit bitmap
        self.A = State(dev, self.orig, self.orig_crcs, pb, ppc, self.cbm0, cow, stream)
        self.B = State(dev, self.orig, self.orig_crcs, pb, ppc, self.cbm0, cow, stream)
        # the host model's state
        self.h_pool, self.h_crcs, self.h_bm = self.orig.copy(), self.orig_crcs.copy(), self.cbm0.copy()
        self.h_counts, self.h_pasted, self.h_contested = [], 0, 0

    def upload(self, queue):
        from curve_amd import crc as C
        out = []
        with C._on_stream(self.stream):
            for kind, src, entries in queue:
                e = np.array(entries, dtype=np.uint64).reshape(-1, 3)
                rec = C.log_records(e[:, 0], e[:, 1], e[:, 2].astype(np.uint32))
                d_rec = torch.from_numpy(rec.view(np.uint8)).to(self.dev) if len(entries) else to_dev(np.zeros(24, np.uint8), self.dev)
                out.append((kind, to_dev(src, self.dev), d_rec, len(entries)))
        return out

    def run(self, queue, delta=False, sequence=True, contested=True):
        """State A: one apply_ops.  State B (sequence=True): the per-batch sequence.  The host model follows."""
        from curve_amd import crc as C
        A, B, pb = self.A, self.B, self.pb
        ops = self.upload(queue)
        got = C.apply_ops(A.pool, A.crcs, ops, self.max_len, self.mpl, pb, stream=self.stream, delta=delta, cow=A.cow,
                          clone=A.clone, contested=A.contested if contested else None)
        assert len(got) == sum(1 for kind, _, _ in queue if kind == "paste")
        A.counts += got
        if sequence:
            for (kind, src, d_rec, n), (_, _, entries) in zip(ops, queue):
                if kind == "write":
                    if n:
                        C.apply_log_cow(B.pool, B.crcs, src, d_rec, n, self.max_len, B.cow, pb, stream=self.stream,
                                        delta=delta)
                        C.clone_mark(B.pool, d_rec, n, self.max_len, B.clone, pb, stream=self.stream)
                    continue
                # cc_paste_dev knows no max_paste_len: an entry the queue refuses for it goes in as an invalid one
                ent = [(d, s, ln) if ln <= self.mpl else (1, s, ln) for d, s, ln in entries]
                e = np.array(ent, dtype=np.uint64).reshape(-1, 3)
                with C._on_stream(self.stream):
                    per = torch.zeros(max(n, 1), dtype=torch.int32, device=self.dev)
                    d_p = torch.from_numpy(C.log_records(e[:, 0], e[:, 1], e[:, 2].astype(np.uint32)).view(np.uint8)).to(
                        self.dev) if n else None
                if n:
                    C.paste_records(B.pool, B.crcs, src, d_p, n, B.clone, per, pb, stream=self.stream)
                    if self.stream is not None:
                        d_p.record_stream(self.stream)
                B.counts.append(per[:n])
        crc_fn = lambda page: int(self.oracle.page_crcs(np.ascontiguousarray(page), pb)[0])  # noqa: E731
        counts, pasted, cont, pages = ops_model(self.h_pool, self.h_crcs, queue, self.max_len, self.mpl,
                                                np.array(CLONE_SLOT, np.uint32), N_CLONE, self.h_bm, pb, self.cb, crc_fn)
        self.h_counts += counts
        self.h_pasted += pasted
        self.h_contested += cont if contested else 0
        self._keep = ops                                       # the device buffers, until check() has synchronised
        return cont, pages

    def check(self, sequence=True):
        if self.stream is not None:
            self.stream.synchronize()
        else:
            torch.cuda.synchronize()
        a = self.A.arrays()
        if sequence:
            b = self.B.arrays()
            assert sorted(a) == sorted(b)
            for k in a:
                assert (a[k] == b[k]).all(), k
        assert (a["claim"] == 0xFFFFFFFF).all()
        assert (a["pool"] == self.h_pool).all()
        assert (a["crcs"] == self.h_crcs).all()
        assert (a["crcs"] == self.oracle.page_crcs(self.h_pool, self.pb)).all()
        assert (a["clone_bitmap"] == self.h_bm).all()
        assert int(a["pasted"][0]) == self.h_pasted
        assert len(self.A.counts) == len(self.h_counts)
        for k, want in enumerate(self.h_counts):
            assert (a["counts%d" % k] == want).all(), k
        assert int(self.A.contested.cpu()[0]) == self.h_contested
        return a


# --------------------------------------------------------------------------- cases
@pytest.mark.parametrize("delta", [False, True], ids=["full", "delta"])
@pytest.mark.parametrize("pb", PAGE_SIZES)
def test_mixed_queue_equals_the_sequence(dev, oracle, pb, delta):
    """W P W P P W P W at every page size: in full mode on chunks of 40 pages (a bitmap word
    and a part) with random preset bits, in delta mode on chunks of 8 with none."""
    ppc = 8 if delta else 40
    max_len, mpl = 3 * pb + 7, 6 * pb
    g = Gen(100 + pb, pb, ppc, max_len, mpl)
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset="none" if delta else "random", seed=pb)
    cont, _ = t.run(g.mixed(), delta=delta)
    assert cont == 0                                           # the generator's promise: the twin must agree
    a = t.check()
    assert int(a["pasted"][0]) > 3                             # (the seeded queue does paste: 5 .. 39 pages)


@pytest.mark.parametrize("preset", ["none", "all", "random"])
def test_preset_bits(dev, oracle, preset):
    pb, ppc, max_len, mpl = 512, 40, 2 * 512, 8 * 512
    g = Gen(7, pb, ppc, max_len, mpl)
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset=preset, seed=3)
    cont, _ = t.run(g.mixed())
    assert cont == 0
    a = t.check()
    assert (int(a["pasted"][0]) == 0) == (preset == "all")     # every bit set: every paste loses


def alternating_35(g, pb, ppc, max_len, mpl):
    X = 5 * ppc + 1
    Y = X + 2

    def low_paste():
        n = int(g.rng.integers(0, mpl // pb + 1))
        return g.paste(n, int(g.rng.integers(0, 5 * ppc - n + 1)))

    def low_write():
        if g.rng.integers(0, 2):
            return g.any_write([1, 3, 4])
        n = int(g.rng.integers(1, max_len // pb + 1))
        return (int(g.rng.integers(0, 5 * ppc - n + 1)) * pb, int(g.rng.integers(0, 64)) * 4, n * pb)

    queue = []
    for k in range(35):
        if k % 2 == 0:
            ent = [low_paste() for _ in range(3 + k % 5)]
            if k == 0:
                ent.append(g.paste(1, X))
            if k == 34:
                ent.append(g.paste(3, X))                      # X, X + 1, Y: only X + 1 is still open
            queue.append(("paste", g.src(), ent))
        else:
            ent = [low_write() for _ in range(2 + k % 7)]
            if k == 1:
                ent.append((Y * pb, 0, pb))
            if k == 33:
                ent.append((X * pb, pb, pb))
            queue.append(("write", g.src(), ent))
    return queue, X, Y


def test_35_alternating_batches_cross_the_descriptor_boundary(dev, oracle):
    """35 non-empty batches, P W P W ... P: more than 32 descriptors in BID, and the first
    setters sit a launch away from the bidders they must beat.  The random entries keep to
    chunks 0-4; in chunk 5, page X is pasted by batch 0 (which beats the whole write of batch
    33 and the paste of batch 34), page Y = X + 2 is written whole by batch 1 (which beats
    the paste of batch 34), and X + 1 is left to batch 34."""
    pb, ppc, max_len, mpl = 256, 8, 2 * 256, 4 * 256
    g = Gen(35, pb, ppc, max_len, mpl)
    queue, X, Y = alternating_35(g, pb, ppc, max_len, mpl)
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset="none", seed=35)
    cont, _ = t.run(queue)
    assert cont == 0
    a = t.check()
    assert int(a["counts0"][-1]) == 1                          # batch 0's paste of X landed
    assert int(a["counts17"][-1]) == 1                         # batch 34: X + 1 alone of its three pages
    assert (a["pool"][(X + 1) * pb:(X + 2) * pb] == queue[34][1][queue[34][2][-1][1] + pb:][:pb]).all()
    assert (a["pool"][X * pb:(X + 1) * pb] == queue[33][1][pb:2 * pb]).all()   # batch 33's write, on batch 0's paste
    assert (a["pool"][Y * pb:(Y + 1) * pb] == queue[1][1][:pb]).all()          # Y: the user's write, never buried


def test_small_write_batches_between_pastes(dev, oracle):
    """Write batches of <= 64 one-page writes take the queue's one-launch path; paste batches
    sit between them."""
    pb, ppc, max_len, mpl = 1024, 8, 1024, 4 * 1024
    g = Gen(64, pb, ppc, max_len, mpl)
    queue = []
    for k, n in enumerate((64, 20, 1, 64, 33)):
        queue.append(("write", g.src(), [g.whole_write(1) for _ in range(n)]))
        queue.append(("paste", g.src(), [g.paste() for _ in range(30 + k)]))
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset="none", seed=64)
    cont, _ = t.run(queue, delta=True)
    assert cont == 0
    t.check()


@pytest.mark.parametrize("cow", ["cow", "stale"])
def test_open_snapshot_on_another_chunk(dev, oracle, cow):
    """Chunk 4 has an open snapshot (with and without the rehash of d_stale); the clone chunks
    beside it take pastes in the same queue."""
    pb, ppc, max_len, mpl = 2048, 8, 2 * 2048 + 5, 4 * 2048
    g = Gen(44, pb, ppc, max_len, mpl)
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, seed=44, cow=cow)
    cont, _ = t.run(g.mixed((40, 20, 40, 0, 20, 0, 20, 40)))
    assert cont == 0
    a = t.check()
    assert int(a["copied"][0]) > 0 and int(a["pasted"][0]) > 0
    if cow == "stale":
        assert int(a["stale"][0]) == 0


def test_pastes_only_and_writes_only(dev, oracle):
    """A queue of paste batches alone (no write side at all), then one of write logs alone,
    which must be cc_apply_logs_cow_dev: state B takes apply_logs(clone=) for it."""
    from curve_amd import crc as C
    pb, ppc, max_len, mpl = 4096, 8, 4096 + 9, 3 * 4096
    g = Gen(5, pb, ppc, max_len, mpl)
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset="random", seed=5)
    pastes = [("paste", g.src(), [g.paste() for _ in range(n)] + g.bad_pastes()) for n in (50, 0, 70)]
    t.run(pastes)
    t.check()
    writes = [("write", g.src(), [g.any_write() for _ in range(n)] + g.bad_writes()) for n in (70, 0, 30, 64)]
    ops = t.upload(writes)
    assert C.apply_ops(t.A.pool, t.A.crcs, ops, max_len, mpl, pb, clone=t.A.clone, contested=t.A.contested) == []
    C.apply_logs(t.B.pool, t.B.crcs, [o[1:] for o in ops], max_len, pb, clone=t.B.clone)
    ops_model(t.h_pool, t.h_crcs, writes, max_len, mpl, np.array(CLONE_SLOT, np.uint32), N_CLONE, t.h_bm, pb, t.cb,
              lambda page: int(oracle.page_crcs(np.ascontiguousarray(page), pb)[0]))
    t.check()


def test_twice_in_a_row_on_a_side_stream(dev, oracle):
    """Two queues back to back on a side stream, no synchronisation between them: the second
    finds the bits and the claim words as the first left them."""
    pb, ppc, max_len, mpl = 256, 40, 3 * 256 + 1, 5 * 256
    s = torch.cuda.Stream(device=dev)
    g = Gen(22, pb, ppc, max_len, mpl)
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset="none", seed=22, stream=s)
    q1, q2 = g.mixed((30, 20, 30, 0, 10, 0, 10, 0)), g.mixed((20, 30, 20, 0, 30, 0, 30, 40))
    keep = []                                                  # (q1's partial writes precede q2's pastes: another call,
    #                                                            so no contested pair, and the sequence agrees)
    for q in (q1, q2):
        cont, _ = t.run(q, delta=True)
        assert cont == 0
        keep.append(t._keep)
    t.check()


@pytest.mark.parametrize("counter", [True, False], ids=["counted", "null"])
def test_contested_queue_follows_the_model(dev, oracle, counter):
    """Unaligned writes BEFORE pastes of the same pages: the sequence would bury them, the call
    lays them on the origin bytes.  Pool, CRC table, bitmaps, counts and *d_contested equal the
    host model; with d_contested NULL everything else is the same."""
    pb, ppc, max_len, mpl = 512, 8, 3 * 512 + 7, 6 * 512
    g = Gen(77, pb, ppc, max_len, mpl)
    queue = [("write", g.src(), [g.any_write([0, 2, 5]) for _ in range(60)] + [g.whole_write() for _ in range(10)]),
             ("paste", g.src(), [g.paste() for _ in range(40)]),
             ("write", g.src(), [g.any_write() for _ in range(70)]),
             ("paste", g.src(), [g.paste() for _ in range(40)] + [g.paste(ppc, 5 * ppc)]),
             ("write", g.src(), [g.any_write() for _ in range(30)])]
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset="none", seed=77)
    cont, pages = t.run(queue, sequence=False, contested=counter)
    assert cont > 20 and len(pages) > 5                        # the case is there
    t.check(sequence=False)
    assert int(t.A.contested.cpu()[0]) == (cont if counter else 0)


def test_skew_all_winners_in_the_first_64_entries(dev, oracle):
    """Every winning page lies in the first 64 entries of the first paste batch; the rest of
    that batch and all of the next are losers (duplicates of the same pages)."""
    pb, ppc, max_len, mpl = 4096, 40, 4096, 4 * 4096
    g = Gen(9, pb, ppc, max_len, mpl)
    first = [g.paste(4, (0, 2 * ppc, 5 * ppc)[k % 3] + 4 * (k // 3 % 10)) for k in range(64)]
    losers = [g.paste(int(g.rng.integers(1, 5)), (0, 2 * ppc, 5 * ppc)[k % 3] + int(g.rng.integers(0, 36))) for k in range(70)]
    queue = [("write", g.src(), g.safe_writes(10)), ("paste", g.src(), first + losers),
             ("paste", g.src(), losers[::-1]), ("write", g.src(), [g.any_write() for _ in range(20)])]
    t = Twin(dev, oracle, pb, ppc, max_len, mpl, preset="none", seed=9)
    cont, _ = t.run(queue)
    assert cont == 0
    a = t.check()
    assert int(a["counts0"][64:].astype(np.int64).sum()) == 0 and int(a["counts1"].astype(np.int64).sum()) == 0
    assert int(a["counts0"][:64].sum()) == int(a["pasted"][0]) > 60
