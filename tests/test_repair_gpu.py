"""cc_repair_dev, crc.repair_pages and DevicePool.repair_bad_pages on the GPU,
checked bit for bit against repair_model of test_repair.py (itself checked
against a page-by-page restatement of the header comment) and the oracle's CRCs.

The rig: a pool of 320 pages and a source of 512 pages, each between two guard
bands of known bytes, as are the CRC table, the claim table and the counts.
Source page s is a copy for pool page s % 320: good, one bit off, or the bad
live bytes.  Everything is mirrored on the host and compared IN FULL after
every call; the claim table must be all-ones again.
"""
import threading

import numpy as np
import pytest

from test_repair import CLEAN, FAILED, REPAIRED, SHADOWED, U32_MAX, flip, repair_model, repair_valid

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_PAGES = 320
SRC_PAGES = 512
PAGE_SIZES = [256, 512, 1024, 2048, 4096, 8192]
SEEDS = {256: 60, 512: 61, 1024: 62, 2048: 63, 4096: 64, 8192: 65}  # each passes the class-count condition below
GUARD_BYTE, GUARD_WORD = 0xA5, 0x5AA5C33C


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from curve_amd import crc as C
    C.engine_init()
    return torch.device("cuda", 0)


def u32(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint32)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Guarded:
    """A device tensor between two guard bands of known values."""

    def __init__(self, host, dev, guard):
        fill = GUARD_BYTE if host.dtype == np.uint8 else np.uint32(GUARD_WORD).view(np.int32)
        self.g, self.fill = guard, fill
        band = np.full(guard, fill, host.dtype)
        self.buf = to_dev(np.concatenate([band, host.reshape(-1), band]), dev)
        self.t = self.buf[guard:guard + host.size]

    def guards_ok(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.g] == self.fill).all() and (b[-self.g:] == self.fill).all())


def make_case(oracle, pb, seed, n=200, hi=8, with_expect=False, n_pages=N_PAGES, src_pages=SRC_PAGES, invalid=10):
    """(pool, crcs, expect, src, entries): ~40 % of the pool pages corrupted by
    one bit (first dword, last dword, or a random one); source page s a copy
    for pool page s % n_pages (60 % good, 20 % one bit off, 20 % the bad live
    bytes); n entries of 1..hi pages whose source lines up with one of the
    copies (70 %) or lies anywhere (30 %); `invalid` invalid entries and an
    empty one among them.  With with_expect the authority's table differs from
    the local one in about a third of the pages: half of those because the
    authority holds other bytes, half because only the local WORD is stale (the
    live bytes already match the authority)."""
    rng = np.random.default_rng(seed)
    good = rng.integers(0, 256, n_pages * pb, dtype=np.uint8)
    crcs = oracle.page_crcs(good, pb)
    pool = good.copy()
    for p in np.nonzero(rng.random(n_pages) < 0.4)[0]:
        at = [0, pb - 4, 4 * int(rng.integers(0, pb // 4))][int(rng.integers(0, 3))]
        flip(pool, p * pb + at + int(rng.integers(0, 4)), int(rng.integers(0, 8)))
    expect = None
    if with_expect:
        expect = crcs.copy()
        for p in np.nonzero(rng.random(n_pages) < 0.33)[0]:
            if rng.random() < 0.5:
                crcs[p] ^= np.uint32(1 << int(rng.integers(0, 32)))
            else:
                good[p * pb:(p + 1) * pb] = rng.integers(0, 256, pb, dtype=np.uint8)
                expect[p] = oracle.crc32c(good[p * pb:(p + 1) * pb].tobytes())
    src = np.empty(src_pages * pb, np.uint8)
    for s in range(src_pages):
        p, kind = s % n_pages, rng.random()
        page = src[s * pb:(s + 1) * pb]
        page[:] = (good if kind < 0.8 else pool)[p * pb:(p + 1) * pb]
        if 0.6 <= kind < 0.8:
            flip(page, int(rng.integers(0, pb)), int(rng.integers(0, 8)))
    entries = []
    for _ in range(n):
        k = int(rng.integers(1, hi + 1))
        p0 = int(rng.integers(0, n_pages - k + 1))
        where = rng.random()
        if where < 0.25 and n_pages + p0 + k <= src_pages:
            s0 = n_pages + p0                                   # the second copy
        elif where < 0.7 and p0 + k <= src_pages:
            s0 = p0                                             # the first copy
        else:
            s0 = int(rng.integers(0, src_pages - k + 1))        # anywhere: unrelated bytes
        entries.append((p0 * pb, s0 * pb, k * pb))
    pool_bytes, src_bytes = pool.size, src.size
    bad = [(pb // 2, 0, pb), (2 * pb, 0, pb + 4), (pool_bytes - pb, 0, 2 * pb), (pool_bytes, 0, pb), (1 << 40, 0, pb),
           (4 * pb, 6, pb), (6 * pb, src_bytes - pb, 2 * pb), (8 * pb, 1 << 40, pb), (pb + 128, 0, 3 * pb),
           (0, src_bytes, pb)]
    for e in bad[:invalid]:
        entries.insert(int(rng.integers(0, len(entries) + 1)), e)
    if invalid:
        entries.insert(int(rng.integers(0, len(entries) + 1)), (3 * pb, 0, 0))
    return pool, crcs, expect, src, entries


class Rig:
    """Pool, tables and source on the device between guards, and their host mirror, advanced together."""

    def __init__(self, dev, oracle, pb, pool, crcs, expect, src, stream=None):
        from curve_amd import crc as C
        self.C, self.dev, self.oracle, self.pb, self.stream = C, dev, oracle, pb, stream
        self.host, self.stored, self.expect, self.src = pool, crcs, expect, src
        with C._on_stream(stream):
            self.g_pool = Guarded(pool, dev, 2 * pb)
            self.g_src = Guarded(src, dev, 2 * pb)
            self.g_crcs = Guarded(i32(crcs), dev, 64)
            self.g_claim = Guarded(np.full(pool.size // pb, -1, np.int32), dev, 64)
            self.g_expect = Guarded(i32(expect), dev, 64) if expect is not None else None
        self.guarded = [self.g_pool, self.g_src, self.g_crcs, self.g_claim] + ([self.g_expect] if self.g_expect else [])

    def sync(self):
        if self.stream is not None:
            self.stream.synchronize()
        else:
            torch.cuda.synchronize()

    def call(self, entries):
        """One cc_repair_dev call and the model's answer to it, everything compared in full.
        Returns (per_entry uint32 [n, 4], totals)."""
        C, n = self.C, len(entries)
        rec = C.log_records([e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries])
        with C._on_stream(self.stream):
            d_rec = to_dev(rec.view(np.uint8), self.dev)
            g_per = Guarded(np.zeros(4 * n, np.int32), self.dev, 64)
            g_tot = Guarded(np.zeros(4, np.int64), self.dev, 8)
        C.repair_records(self.g_pool.t, self.g_crcs.t, self.g_src.t, d_rec, n, self.g_claim.t, g_per.t,
                         expect=self.g_expect.t if self.g_expect else None, totals=g_tot.t, page_bytes=self.pb,
                         stream=self.stream)
        want, w_tot, w_claim = repair_model(self.host, self.stored, self.expect, self.src, entries, self.pb,
                                            lambda b: self.oracle.crc32c(b.tobytes()))
        self.sync()
        got = u32(g_per.t).reshape(n, 4)
        assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:10]
        assert g_tot.t.cpu().numpy().tolist() == w_tot.tolist()
        assert g_per.guards_ok() and (g_tot.buf.cpu().numpy()[[0, -1]] == GUARD_WORD).all()
        assert (w_claim == U32_MAX).all()
        self.check()
        return got, w_tot

    def check(self):
        """Pool, CRC table, the untouched source and expectation, the claim table all-ones, every guard."""
        self.sync()
        got = self.g_pool.t.cpu().numpy()
        assert (got == self.host).all(), np.nonzero(got != self.host)[0][:10] // self.pb
        crcs = u32(self.g_crcs.t)
        assert (crcs == self.stored).all(), np.nonzero(crcs != self.stored)[0][:10]
        assert (u32(self.g_claim.t) == U32_MAX).all()
        assert (self.g_src.t.cpu().numpy() == self.src).all()
        if self.g_expect:
            assert (u32(self.g_expect.t) == self.expect).all()
        assert all(g.guards_ok() for g in self.guarded)


def rig_for(dev, oracle, pb, seed, stream=None, **kw):
    pool, crcs, expect, src, entries = make_case(oracle, pb, seed, **kw)
    return Rig(dev, oracle, pb, pool, crcs, expect, src, stream=stream), entries


def postcondition(rig, entries, pool0, crcs0):
    """The header's postcondition, page by page, on the device's own outputs."""
    pb, n_pages = rig.pb, rig.host.size // rig.pb
    pool = rig.g_pool.t.cpu().numpy()
    crcs = u32(rig.g_crcs.t)
    rec = rig.expect if rig.expect is not None else crcs0
    now = rig.oracle.page_crcs(pool, pb)
    named = np.zeros(n_pages, bool)
    for dst, so, ln in entries:
        if ln and repair_valid(dst, so, ln, pool.size, rig.src.size, pb):
            named[dst // pb:(dst + ln) // pb] = True
    fine = named & (now == rec)                                 # clean or repaired: hashes to e, and the word is e
    assert (crcs[fine] == rec[fine]).all()
    rest = ~fine                                                # failed, or named by no valid entry: bit for bit
    assert (pool.reshape(-1, pb)[rest] == pool0.reshape(-1, pb)[rest]).all() and (crcs[rest] == crcs0[rest]).all()
    return int(fine.sum()), int((named & rest).sum())


# --------------------------------------------------------------------------- all six page sizes
@pytest.mark.parametrize("with_expect", [False, True])
@pytest.mark.parametrize("pb", PAGE_SIZES)
def test_repair_every_page_size(dev, oracle, pb, with_expect):
    """M = 1 .. 32: 200 entries of 1-8 pages plus invalid ones (the tiled path:
    more than 64 entries), every class at least 8 times.  With the authority's
    table: a third of the pages differ from the local table, stale words
    included.  Then the same batch again: what was repaired is clean now."""
    rig, entries = rig_for(dev, oracle, pb, SEEDS[pb] + (100 if with_expect else 0), with_expect=with_expect)
    pool0, crcs0 = rig.host.copy(), rig.stored.copy()
    got, totals = rig.call(entries)
    invalid = int((got[:, 0] == U32_MAX).sum())
    assert min(int(t) for t in totals) >= 8 and invalid >= 8, (totals, invalid)
    ok = got[:, 0] != U32_MAX
    assert (got[ok].sum(axis=1) == np.array([e[2] // pb for e in entries])[ok]).all()
    fine, failed = postcondition(rig, entries, pool0, crcs0)
    assert fine == int(totals[CLEAN] + totals[REPAIRED]) and failed == int(totals[FAILED])
    if with_expect:
        stale = (crcs0 != rig.expect) & (oracle.page_crcs(pool0, pb) == rig.expect)
        assert stale.sum() >= 8 and (rig.stored[stale] == rig.expect[stale]).sum() >= 8      # stale words mended
    again, t2 = rig.call(entries)
    assert int(t2[REPAIRED]) == 0 and int(t2[CLEAN]) == fine and int(t2[FAILED]) == failed
    assert (again[:, SHADOWED] == got[:, SHADOWED]).all()


# --------------------------------------------------------------------------- schedule edges
def entries_with_slots(rng, pb, total, n_pages=N_PAGES):
    """Entries of 1-8 pages (first copy of the source) whose page counts sum to `total` exactly."""
    out, left = [], total
    while left:
        k = min(int(rng.integers(1, 9)), left)
        p0 = int(rng.integers(0, n_pages - k + 1))
        out.append((p0 * pb, p0 * pb, k * pb))
        left -= k
    return out


@pytest.mark.parametrize("pb", [1024, 4096])                    # three register sets / two
@pytest.mark.parametrize("total", [1, 63, 64, 65, 1023])
def test_slot_totals_at_the_schedules_edges(dev, oracle, pb, total):
    rig, _ = rig_for(dev, oracle, pb, 7 + total)
    entries = entries_with_slots(np.random.default_rng(total), pb, total)
    got, totals = rig.call(entries)
    assert int(sum(totals)) == total == int(got.sum())


def test_one_entry_over_the_whole_pool(dev, oracle):
    pb = 2048
    rig, _ = rig_for(dev, oracle, pb, 11)
    pool0, crcs0 = rig.host.copy(), rig.stored.copy()
    entries = [(0, 0, N_PAGES * pb)]
    got, totals = rig.call(entries)
    assert int(got.sum()) == N_PAGES and int(totals[SHADOWED]) == 0 and min(int(t) for t in totals[:3]) >= 8
    postcondition(rig, entries, pool0, crcs0)


def test_4096_one_page_entries_with_long_shadowed_runs(dev, oracle):
    """An 8 MiB pool of 4 KiB pages; 4096 one-page entries over 64 of its pages,
    so that 4032 pairs are shadowed, in runs far longer than a wave's 64 entries."""
    pb, n_pages = 4096, 2048
    rig, _ = rig_for(dev, oracle, pb, 12, n_pages=n_pages, src_pages=n_pages, n=0, invalid=0)
    rng = np.random.default_rng(13)
    some = rng.choice(n_pages, 64, replace=False)
    pages = np.concatenate([some, rng.choice(some, 4096 - 64)])  # the first 64 entries take every page there is
    entries = [(int(p) * pb, int(p) * pb, pb) for p in pages]
    got, totals = rig.call(entries)
    assert int(totals[SHADOWED]) == 4032 and int(sum(totals[:3])) == 64
    assert (got[64:, SHADOWED] == 1).all() and (got[:64, SHADOWED] == 0).all()
    rng.shuffle(pages)                                           # handlers scattered among the shadowed
    entries = [(int(p) * pb, int(p) * pb, pb) for p in pages]
    got, totals = rig.call(entries)
    assert int(totals[SHADOWED]) == 4032 and int(totals[REPAIRED]) == 0


def test_a_batch_of_at_most_64_entries(dev, oracle):
    for pb, n in ((256, 1), (512, 40), (8192, 64)):
        rig, entries = rig_for(dev, oracle, pb, 14 + n, n=n, invalid=0)
        assert len(entries) == n
        got, totals = rig.call(entries)
        assert int(sum(totals)) == sum(e[2] // pb for e in entries)


# --------------------------------------------------------------------------- invalid entries
def test_invalid_entries_among_valid_ones_write_nothing(dev, oracle):
    pb = 512
    rig, entries = rig_for(dev, oracle, pb, 15, n=90, hi=4, invalid=10)
    pool_bytes, src_bytes = rig.host.size, rig.src.size
    entries.append((pool_bytes - pb, src_bytes - pb, pb))        # both ends exactly: valid
    invalid = [i for i, e in enumerate(entries) if not repair_valid(*e, pool_bytes, src_bytes, pb)]
    empty = [i for i, e in enumerate(entries) if e[2] == 0]
    assert len(invalid) == 10 and len(empty) == 1
    # the pages only invalid entries name stay as they are: keep the valid ones off pages 0 .. 9
    entries = [e for i, e in enumerate(entries) if i in invalid or i in empty or e[0] >= 10 * pb]
    invalid = [i for i, e in enumerate(entries) if not repair_valid(*e, pool_bytes, src_bytes, pb)]
    before = rig.host.copy()
    got, totals = rig.call(entries)                              # guards, pool and tables in full
    assert (got[invalid] == U32_MAX).all() and (np.delete(got, invalid, axis=0) != U32_MAX).all()
    empty = [i for i, e in enumerate(entries) if e[2] == 0]
    assert not got[empty].any() and int(got[-1].sum()) == 1
    assert (rig.g_pool.t.cpu().numpy()[:10 * pb] == before[:10 * pb]).all()


# --------------------------------------------------------------------------- the loop closed
def test_detect_repair_verify(dev, oracle):
    """page_verify_list, repair_pages with two peers of which the first is
    itself corrupt in some pages, page_verify: zero.  Then the same through
    DevicePool.repair_bad_pages against an authority's table."""
    from curve_amd import crc as C
    from curve_amd.scan import ChunkPool
    pb, n_chunks, ppc = 4096, 4, 64
    n_pages = n_chunks * ppc
    rng = np.random.default_rng(21)
    good = rng.integers(0, 256, n_pages * pb, dtype=np.uint8)
    table = oracle.page_crcs(good, pb)
    bad = np.sort(rng.choice(n_pages, 40, replace=False))
    peer0_bad = bad[::3]
    first = good.copy()
    for p in peer0_bad:
        flip(first, int(p) * pb + 5, 1)
    d_peers = [to_dev(first, dev), to_dev(good, dev)]
    asked = []

    def fetcher(who):
        def fetch(pages):
            asked.append((who, [int(p) for p in pages]))
            return d_peers[who], np.asarray(pages, np.uint64) * np.uint64(pb)   # the peer's image: page p at p * pb
        return fetch

    def corrupted():
        pool = good.copy()
        for p in bad:
            flip(pool, int(p) * pb + int(rng.integers(0, pb)), int(rng.integers(0, 8)))
        return to_dev(pool, dev)

    d_pool, d_table = corrupted(), to_dev(i32(table), dev)
    cnt, lst = C.page_verify_list(d_pool, d_table, pb)
    assert int(cnt[0]) == bad.size
    found = lst[:int(cnt[0])].cpu().numpy()
    claim = C.repair_claim(d_pool, pb)
    pages, cls, by = C.repair_pages(d_pool, d_table, found, [fetcher(0), fetcher(1)], claim, page_bytes=pb)
    assert pages.tolist() == bad.tolist() and (cls == REPAIRED).all()
    assert (by == np.isin(bad, peer0_bad).astype(np.int64)).all()
    assert asked == [(0, bad.tolist()), (1, peer0_bad.tolist())]
    cnt = C.page_verify(d_pool, d_table, pb)
    torch.cuda.synchronize()
    assert int(cnt[0]) == 0 and (d_pool.cpu().numpy() == good).all()
    assert (u32(claim) == U32_MAX).all() and (u32(d_table) == table).all()
    # the same through the pool object, on a side stream, its local table all stale
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        dp = ChunkPool(corrupted().reshape(n_chunks, ppc * pb), torch.zeros((n_chunks, pb), dtype=torch.uint8, device=dev),
                       list(range(n_chunks)), page_bytes=pb, scan_size=ppc * pb)
        dp.page_crcs.zero_()
    s.synchronize()
    repaired, still = dp.repair_bad_pages(d_table, [fetcher(0), fetcher(1)], stream=s)
    assert still == [] and [(c * ppc + q) for c, q, _ in repaired] == bad.tolist()
    assert [f for _, _, f in repaired] == np.isin(bad, peer0_bad).astype(int).tolist()
    assert (dp.data.cpu().numpy().reshape(-1) == good).all() and (u32(dp.page_crcs)[bad] == table[bad]).all()
    only_first = dp.repair_bad_pages(d_table, [fetcher(0)], stream=s)
    assert only_first == ([], [])


# --------------------------------------------------------------------------- streams and threads
def test_a_side_stream_with_a_second_thread_on_another_pool(dev, oracle):
    """Two threads, each with a stream and a rig of its own, each running the
    same batch twice from the same start: identical outputs, both equal to the model's."""
    errs, outs = [], {}

    def work(i):
        try:
            s = torch.cuda.Stream(device=dev)
            for pb in (512, 4096):
                runs = []
                for _ in range(2):
                    rig, entries = rig_for(dev, oracle, pb, SEEDS[pb], stream=s, with_expect=bool(i))
                    got, totals = rig.call(entries)
                    runs.append((got.tobytes(), tuple(int(t) for t in totals), rig.g_pool.t.cpu().numpy().tobytes(),
                                 u32(rig.g_crcs.t).tobytes()))
                assert runs[0] == runs[1]
                outs[(i, pb)] = runs[0][1]
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append((i, e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert len(outs) == 4
