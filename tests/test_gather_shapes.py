"""The batch shapes of gather_shapes.py, without a GPU: every shape is what
its docstring says at every grid the GPU suite runs at, and on the "all rotten"
inputs of test_gather_grids_gpu.py (every table word XOR 1, so a call that
handles every slot exactly once reports every page of every entry) the numpy
models of the six calls report exactly the generators' own page counts.  That
pins what the device is compared with before a device is asked.

The host states here restate the GPU files' rigs (those modules need torch):
8 chunks, snapshot slots {0, -, 2, -, 1, out of range, -, 3}, clone slots the
same, four slots each.
"""
import numpy as np
import pytest

import gather_shapes as G
from test_clone import NOT_CLONE, bit, paste_model, paste_valid, set_bit
from test_log_cow import NO_SNAPSHOT, fresh_slots
from test_read_merge import OUT_SENT, read_merge_model
from test_repair import repair_model
from test_scrub import HostRig
from test_snap_read import U32_MAX, packed_offsets, read_valid, snap_read_model

GRIDS = [8, 24, 504, 2048, 2432]                             # Wg at 1, 3, 63, 256 and 304 workgroups
N_CHUNKS, N_SLOTS = 8, 4
SNAP_SLOTS = [0, NO_SNAPSHOT, 2, NO_SNAPSHOT, 1, 9, NO_SNAPSHOT, 3]
CLONE_SLOTS = [0, NOT_CLONE, 2, NOT_CLONE, 1, 7, NOT_CLONE, 3]
PB = 256                                                     # the models' answers do not depend on the page size


# --------------------------------------------------------------------------- 1: the shapes
@pytest.mark.parametrize("Wg", GRIDS)
@pytest.mark.parametrize("name", G.SHAPE_NAMES)
def test_shape_is_what_its_docstring_says(name, Wg):
    shape = G.make(name, Wg)
    n_pool = G.pool_pages(name)
    kinds = [k for _, _, k in shape]
    assert len(shape) >= G.MIN_ENTRIES
    for p0, k, kind in shape:
        if kind == G.VALID:
            assert k >= 1 and 0 <= p0 and p0 + k <= n_pool
        elif kind == G.EMPTY:
            assert k == 0 and 0 <= p0 < n_pool
        else:
            assert kind == G.INVALID and k >= 1 and p0 + k > n_pool
    total = int(G.slots(shape).sum())
    assert shape == G.make(name, Wg)                         # seeded: the same batch in every process
    what, _, arg = name.partition("-")
    if what == "exact":
        want = G.edge_total(arg, Wg)
        assert want in G.EDGES(Wg) and total == want
        assert all(1 <= k <= 8 for _, k, kind in shape if kind == G.VALID)
        if want == 0:
            assert kinds == [G.EMPTY, G.INVALID] * 32 + [G.EMPTY]
        else:
            assert G.INVALID not in kinds
            assert (G.EMPTY in kinds) == (kinds.count(G.VALID) < G.MIN_ENTRIES)
    elif what == "sparse":
        assert len(shape) == 2000 == 31 * 64 + 16
        for i, (_, k, kind) in enumerate(shape):
            assert kind == (G.VALID if i in G.SPARSE_AT else G.INVALID if 200 <= i < 500 else G.EMPTY)
            assert kind != G.VALID or 1 <= k <= 40
    elif what == "few":
        assert len(shape) == int(arg) < 512 and set(kinds) == {G.VALID}
        assert all(1 <= k <= 3 for _, k, _ in shape)
    elif what == "giant":
        assert len(shape) == 300 and set(kinds) == {G.VALID}
        assert [k for _, k, _ in shape] == [n_pool if i == int(arg) else 1 for i in range(300)]
        assert shape[int(arg)][0] == 0 and total == 299 + n_pool
    else:
        assert name == "long" and len(shape) == 130 and n_pool == 3000 and set(kinds) == {G.VALID}
        assert all(500 <= k <= 3000 for _, k, _ in shape)
        assert total // 2432 > 64                            # more than 64 slots a wave at the widest grid


def test_edges_and_names_agree():
    for Wg in GRIDS:
        assert sorted({G.edge_total(e, Wg) for e in G.EDGE_NAMES}) == G.EDGES(Wg)
    assert len(G.EDGES(8)) == 11 and len(G.EDGES(2048)) == 14   # at 8 waves 8 Wg - 1 .. 8 Wg + 1 are 63 .. 65 again
    assert len(G.SHAPE_NAMES) == len(set(G.SHAPE_NAMES)) == 22


# --------------------------------------------------------------------------- 2: the models on all-rotten inputs
def rot(words):
    """Every word XOR 1: no page matches its word any more (in place; its own inverse)."""
    words ^= np.uint32(1)


def verify_model(pool, stored, reads, pb, page_crcs_fn):
    """cc_verify_reads_dev on page-aligned reads: the pages of each read whose bytes disagree with their word."""
    mism = np.asarray(page_crcs_fn(pool, pb), np.uint32) != stored
    return np.array([int(mism[off // pb:(off + ln) // pb].sum()) if read_valid(off, ln, 0, pool.size, None, pb)
                     else U32_MAX for off, ln in reads], np.uint32)


def unwritten_mask(slots, bm, ppc):
    """Per pool page: a never-written page of a clone chunk."""
    return np.array([int(s) < N_SLOTS and not bit(bm, int(s), q) for s in slots for q in range(ppc)], bool)


def written_per_entry(shape, unwritten):
    """The pages of each VALID entry that exist in the pool (not never-written), 0 for the other kinds."""
    return np.array([int((~unwritten[p0:p0 + k]).sum()) if kind == G.VALID else 0 for p0, k, kind in shape], np.int64)


def random_bits(rng, ppc, density):
    bm = np.zeros((N_SLOTS, (ppc + 31) // 32), np.uint32)
    for s in range(N_SLOTS):
        for q in range(ppc):
            if rng.random() < density:
                set_bit(bm, s, q)
    return bm


class Pool:
    """A pool of 8 chunks with a clean CRC table."""

    def __init__(self, oracle, n_pool, seed=3):
        self.oracle, self.ppc, self.cb = oracle, n_pool // N_CHUNKS, n_pool // N_CHUNKS * PB
        self.rng = np.random.default_rng(seed)
        self.pool = self.rng.integers(0, 256, n_pool * PB, dtype=np.uint8)
        self.stored = np.asarray(oracle.page_crcs(self.pool, PB), np.uint32).copy()

    def crc_fn(self, b):
        return self.oracle.crc32c(b.tobytes())


def shape_at(name):
    """The shape at 24 waves, whatever the machine: `long` and the three totals at the grid's edge included."""
    shape = G.make(name, 24)
    return shape, G.pool_pages(name), int(G.slots(shape).sum()), G.expected(shape)


@pytest.mark.parametrize("name", G.SHAPE_NAMES)
def test_verify_and_snapshot_read_models_report_every_page(oracle, name):
    shape, n_pool, T, want = shape_at(name)
    h = Pool(oracle, n_pool)
    reads = G.byte_ranges(shape, PB)
    rot(h.stored)
    got = verify_model(h.pool, h.stored, reads, PB, oracle.page_crcs)
    assert (got == want).all() and int(got[got != U32_MAX].sum()) == T
    # through snapshot slots with about a third of their bits set, both tables rotten
    snap, scrc, bm = fresh_slots(N_SLOTS, h.cb, PB)
    for s in range(N_SLOTS):
        for q in range(h.ppc):
            if h.rng.random() < 0.3:
                set_bit(bm, s, q)
                snap[s, q * PB:(q + 1) * PB] = h.rng.integers(0, 256, PB, dtype=np.uint8)
                scrc[s, q] = h.crc_fn(snap[s, q * PB:(q + 1) * PB])
    rot(scrc)
    _, bad, total = snap_read_model(h.pool, h.stored, snap, scrc, bm, np.array(SNAP_SLOTS, np.uint32), N_SLOTS, reads,
                                    None, None, PB, h.cb, crc_fn=h.crc_fn)
    assert (bad == want).all() and total == T


@pytest.mark.parametrize("name", G.SHAPE_NAMES)
def test_merged_read_model_reports_every_written_page(oracle, name):
    shape, n_pool, T, want = shape_at(name)
    h = Pool(oracle, n_pool)
    slots, bm = np.array(CLONE_SLOTS, np.uint32), random_bits(h.rng, h.ppc, 0.5)
    reads = G.byte_ranges(shape, PB)
    out_off, out_bytes = packed_offsets([ln for _, ln in reads])
    rot(h.stored)
    bad, bt, unw, ut = read_merge_model(h.pool, h.stored, slots, N_SLOTS, bm, reads, None, None, out_off,
                                        np.full(out_bytes, OUT_SENT, np.uint8), PB, h.cb, crc_fn=h.crc_fn)
    written = written_per_entry(shape, unwritten_mask(slots, bm, h.ppc))
    ok = want != U32_MAX
    assert (bad[~ok] == U32_MAX).all() and (unw[~ok] == U32_MAX).all()
    assert (bad[ok] == written[ok]).all() and (bad[ok].astype(np.int64) + unw[ok] == want[ok]).all()
    assert bt + ut == T and bt == int(written.sum())
    assert T < 100 or 0 < bt < T


def paste_classes(entries, slots, bm, pb, ppc, pool_bytes, src_bytes):
    """test_clone_gpu.classes, restated (that module needs torch): the (entry,
    page) slots of a batch by what becomes of them, from the bitmaps BEFORE the
    call: (pasted, bit already set, lost to an earlier entry, chunk is no clone)."""
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


def paste_entries(shape, pb):
    """(dst, src, len): each entry's source bytes start at its own first page's place in the source."""
    return [(p0 * pb, p0 * pb if kind == G.VALID else 0, k * pb) for p0, k, kind in shape]


@pytest.mark.parametrize("name", G.SHAPE_NAMES)
def test_paste_and_repair_models_account_for_every_slot(oracle, name):
    shape, n_pool, T, want = shape_at(name)
    h = Pool(oracle, n_pool)
    slots, bm = np.array(CLONE_SLOTS, np.uint32), random_bits(h.rng, h.ppc, 0.0)
    src = h.rng.integers(0, 256, n_pool * PB, dtype=np.uint8)
    entries = paste_entries(shape, PB)
    pasted, held, lost, plain = paste_classes(entries, slots, bm, PB, h.ppc, h.pool.size, src.size)
    assert held == 0 and pasted + lost + plain == T
    pool, crcs = h.pool.copy(), h.stored.copy()
    per, total = paste_model(pool, crcs, src, entries, slots, N_SLOTS, bm, PB, h.cb, h.crc_fn)
    ok = want != U32_MAX
    assert (per[~ok] == U32_MAX).all() and (per[ok] <= want[ok]).all()
    assert int(per[ok].sum()) == total == pasted
    assert (crcs == oracle.page_crcs(pool, PB)).all()
    # repair: every (entry, page) pair is counted in exactly one class
    rot(h.stored)                                            # every named page is bad, every candidate too
    per, totals, claim = repair_model(h.pool.copy(), h.stored, None, src, entries, PB, h.crc_fn)
    assert (per[~ok] == U32_MAX).all() and (per[ok].sum(axis=1) == want[ok]).all()
    assert int(totals.sum()) == T and (claim == U32_MAX).all()


# --------------------------------------------------------------------------- scrub: geometries, not entries
SCRUB_GEOMETRIES = [(1, 1), (3, 33), (3, 64), (16, 256)]


def scrub_kwargs(n_chunks, ppc, clone_density=0.3, snap_density=0.25):
    """test_scrub_gpu.shape_rig's arguments: every third chunk a clone, every chunk with a snapshot slot."""
    return dict(ppc=ppc, clone_slots=[NOT_CLONE if c % 3 else c // 3 for c in range(n_chunks)],
                n_clone=(n_chunks + 2) // 3, snap_slots=[n_chunks - 1 - c for c in range(n_chunks)], n_snap=n_chunks,
                clone_density=clone_density, snap_density=snap_density)


def present(h):
    """(live pages that exist, snapshot pages that exist) per chunk, uint32 [chunks, 2], from the bitmaps alone."""
    per = np.zeros((h.n_chunks, 2), np.uint32)
    cls = h.classes()
    for p in cls["ordinary"] + cls["written"]:
        per[p // h.ppc, 0] += 1
    for _, _, p in cls["snap_set"]:
        per[p // h.ppc, 1] += 1
    return per


def total_geometry(total):
    """(n_chunks, ppc) of the pool trim_to_total cuts down to `total` present pages: about total / 0.9 pages, of
    which ~77 % exist live and ~25 % in a snapshot."""
    n_chunks = 8 if total < 4096 else 16
    return n_chunks, -(-(total * 10 // 9 + n_chunks) // n_chunks)


def trim_to_total(h, total):
    """Clear set snapshot bits (then, if the live pages alone are too many, the
    set bits of clone chunks) from the pool's end until exactly `total` pages
    exist.  A cleared bit's page stops existing; its bytes and table word stay
    behind as the garbage such places may hold."""
    have = int(present(h).sum())
    assert have >= total, (have, total)
    for s, q, _ in reversed(h.classes()["snap_set"]):
        if have == total:
            break
        h.cow.bitmap[s, q // 32] &= ~np.uint32(1 << (q % 32))
        have -= 1
    for p in reversed(h.classes()["written"]):
        if have == total:
            break
        ch, q = divmod(p, h.ppc)
        h.clone.bitmap[int(h.clone.clone_slot[ch]), q // 32] &= ~np.uint32(1 << (q % 32))
        have -= 1
    assert int(present(h).sum()) == total


def rot_scrub(h):
    rot(h.crcs)
    rot(h.cow.snap_crcs)


def scrub_expectation(h, cnt, entries, per):
    """All rotten: the model's (or the device's) counts, list and per-chunk words name every page that exists."""
    exist = present(h)
    live, snap = int(exist[:, 0].sum()), int(exist[:, 1].sum())
    assert cnt["live_checked"] == cnt["live_bad"] == live and cnt["snap_checked"] == cnt["snap_bad"] == snap
    assert cnt["listed"] == live + snap == len(entries) and cnt["unwritten"] == h.n_pages - live
    assert (per == exist).all()


@pytest.mark.parametrize("n_chunks,ppc", SCRUB_GEOMETRIES)
def test_scrub_model_lists_every_page_that_exists(oracle, n_chunks, ppc):
    h = HostRig(PB, 90, oracle.page_crcs, **scrub_kwargs(n_chunks, ppc))
    rot_scrub(h)
    cnt, entries, per = h.model(lambda b: oracle.crc32c(b.tobytes()))
    scrub_expectation(h, cnt, entries, per)


@pytest.mark.parametrize("Wg", GRIDS)
def test_scrub_pool_with_a_total_at_the_grids_edge(oracle, Wg):
    total = 8 * Wg + 1
    h = HostRig(PB, 94, oracle.page_crcs, **scrub_kwargs(*total_geometry(total)))
    trim_to_total(h, total)
    rot_scrub(h)
    cnt, entries, per = h.model(lambda b: oracle.crc32c(b.tobytes()))
    scrub_expectation(h, cnt, entries, per)
    assert cnt["listed"] == total and cnt["snap_checked"] > 0 and cnt["unwritten"] > 0
