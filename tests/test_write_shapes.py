"""tests/write_shapes.py on the CPU: the piece classes that exist (by brute
force over every piece of a 256, 512 and 1,024-byte page), that the single-piece
matrix reaches every one of them at all six page sizes, and that every builder
tests/test_write_shapes_gpu.py uses contains what its name says.  These are
conditions, not measurements: a generator that drifts fails here."""
import numpy as np
import pytest

import write_shapes as W


def distinct(*cols):
    """The distinct tuples of small non-negative integer columns."""
    key = np.zeros(cols[0].shape, np.int64)
    for c in cols:
        key = key * 8 + c
    out = []
    for k in np.unique(key).tolist():
        t = []
        for _ in cols:
            t.append(k % 8)
            k //= 8
        out.append(tuple(reversed(t)))
    return out


def brute_force(pb):
    """(byte classes, row classes, flag tuples) over every 0 <= rlo < rhi <= pb
    and sh in 0..3, written on whole arrays, independently of W.classify."""
    lo, hi = np.meshgrid(np.arange(pb + 1), np.arange(pb + 1), indexing="ij")
    keep = lo < hi
    lo, hi = lo[keep], hi[keep]
    n = hi - lo
    first, last = lo // 4, (hi - 1) // 4  # the piece's first and last dword
    part_first = (lo % 4 != 0) | (n < 4)
    part_last = (last != first) & (hi % 4 != 0)
    whole = hi // 4 > (lo + 3) // 4
    byte = {(int(a), int(b), sh, (bool(f), bool(g), bool(w)))
            for a, b, f, g, w in distinct(lo % 4, hi % 4, part_first, part_last, whole)
            for sh in range(4)}
    covered = np.maximum(hi // 256 - (lo + 255) // 256, 0)
    cov = np.where(covered == 0, 0, np.where(covered == pb // 256, 2, 1))
    row = {(bool(a), bool(b), bool(c), ("none", "some", "all")[int(d)])
           for a, b, c, d in distinct(lo % 256 != 0, hi % 256 != 0, lo // 256 == (hi - 1) // 256, cov)}
    l63 = (part_first & (first % 64 == 63)) | (part_last & (last % 64 == 63))
    l0 = (part_first & (first % 64 == 0)) | (part_last & (last % 64 == 0))
    flags = {tuple(bool(x) for x in f) for f in distinct(lo == 0, hi == pb, l63, l0)}
    return byte, row, flags


@pytest.fixture(scope="module")
def reachable():
    return {pb: brute_force(pb) for pb in (256, 512, 1024)}


def test_class_counts(reachable):
    """136 byte classes at every page size; 4 / 8 / 10 row classes."""
    for pb, rows in ((256, 4), (512, 8), (1024, 10)):
        byte, row, _ = reachable[pb]
        assert len(byte) == 136 and len(row) == rows, (pb, len(byte), len(row))
    assert reachable[256][0] == reachable[512][0] == reachable[1024][0]


def test_classify_agrees_with_the_brute_force(reachable):
    """W.classify over every piece of a 256-byte page and every sh, and over
    20,000 random pieces of a 512 and a 1,024-byte page: the brute force's
    sets exactly at 256 B, nothing outside them at the other two."""
    got = W.class_sets(((lo, hi, sh) for lo in range(256) for hi in range(lo + 1, 257) for sh in range(4)), 256)
    assert got == reachable[256]
    rng = np.random.default_rng(1)
    for pb in (512, 1024):
        lo = rng.integers(0, pb, 20000)
        hi = rng.integers(lo + 1, pb + 1)
        byte, row, flags = W.class_sets(zip(lo.tolist(), hi.tolist(), rng.integers(0, 4, 20000).tolist()), pb)
        assert byte <= reachable[pb][0] and row <= reachable[pb][1] and flags <= reachable[pb][2]


def test_candidate_offsets():
    assert [len(W.candidate_offsets(pb)) for pb in W.PAGE_SIZES] == [23, 23, 45, 45, 45, 45]
    for pb in W.PAGE_SIZES:
        offs = W.candidate_offsets(pb)
        assert offs[0] == 0 and offs[-1] == pb and offs == sorted(set(offs))
        assert {256 - 5, 256 + 5 if pb > 256 else 256, pb // 2, pb - 256 + 5, pb - 5} <= set(offs)


@pytest.fixture(scope="module")
def matrices():
    return {pb: W.single_piece_matrix(pb, seed=3, spare=40) for pb in W.PAGE_SIZES}


@pytest.mark.parametrize("pb", W.PAGE_SIZES)
def test_matrix_reaches_every_class(reachable, matrices, pb):
    """Every reachable byte class, row class and flag tuple has a page in the
    matrix; from 2 KiB up the sets are those of 1 KiB pages."""
    m = matrices[pb]
    assert m.n == (1012 if pb <= 512 else 3960) and m.max_len == pb and m.slots == 2
    assert m.pool_bytes == (m.n + 40) * pb <= 32 << 20
    cls = m.info["classes"]
    got = ({c.byte for c in cls.values()}, {c.row for c in cls.values()}, {c.flags for c in cls.values()})
    assert got == reachable[min(pb, 1024)]
    # the classes are those of the writes as laid out, and each page has one piece
    pieces = W.pieces_by_page(pb, m.dst, m.src_off, m.lens)
    assert len(pieces) == m.n == len(cls)
    for page, pcs in pieces.items():
        assert len(pcs) == 1 and W.classify(*pcs[0][1:], pb) == cls[page]
    assert sorted(p[1:] for pcs in pieces.values() for p in pcs) == sorted(W.matrix_pieces(pb))


@pytest.mark.parametrize("pb", W.PAGE_SIZES)
def test_representatives(reachable, pb):
    reps = W.class_representatives(pb)
    assert len(reps) == 136 and {W.classify(*r, pb).byte for r in reps} == reachable[min(pb, 1024)][0]


def piece_classes(log):
    return {W.classify(*p[1:], log.pb).byte for pcs in W.pieces_by_page(log.pb, log.dst, log.src_off, log.lens).values()
            for p in pcs}


@pytest.mark.parametrize("pb", W.PAGE_SIZES)
def test_merge_by_class_builders(reachable, pb):
    """Path 1: three logs of <= 64 one-piece pages, 2 slots, together the 136
    classes.  Path 2: exactly two overlapping pieces a page, the representative
    later / earlier than its partner.  Path 3: exactly three."""
    all_classes = reachable[min(pb, 1024)][0]
    logs = W.small_path_logs(pb)
    assert len(logs) == 3 and all(1 <= g.n <= 64 and g.slots == 2 for g in logs) and sum(g.n for g in logs) == 136
    assert all(set(W.piece_counts(g).values()) == {1} for g in logs)
    assert set().union(*(piece_classes(g) for g in logs)) == all_classes
    assert len(set().union(*(set(W.piece_counts(g)) for g in logs))) == 136  # pages of their own
    reps = set(W.class_representatives(pb))
    for partner_first in (False, True):
        g = W.two_piece_log(pb, partner_first)
        assert g.n == 272 > 64 and g.slots == 2 and piece_classes(g) >= all_classes
        pieces = W.pieces_by_page(pb, g.dst, g.src_off, g.lens)
        assert len(pieces) == 136
        for pcs in pieces.values():
            assert len(pcs) == 2
            (_, alo, ahi, ash), (_, blo, bhi, bsh) = pcs  # in log order
            rep, other = ((blo, bhi, bsh), (alo, ahi)) if partner_first else ((alo, ahi, ash), (blo, bhi))
            assert rep in reps and max(rep[0], other[0]) < min(rep[1], other[1])  # they overlap
    g = W.three_piece_log(pb)
    assert g.n == 408 and g.slots == 2 and piece_classes(g) >= all_classes
    counts = W.piece_counts(g)
    assert len(counts) == 136 and set(counts.values()) == {3}
    orders = set()
    for pcs in W.pieces_by_page(pb, g.dst, g.src_off, g.lens).values():
        assert sum(p[1:] in reps for p in pcs) >= 1
        orders.add(tuple(p[1:] in reps for p in pcs))
    assert {(True, False, False), (False, True, False), (False, False, True)} <= orders  # first, middle and last


@pytest.mark.parametrize("pb", [2048, 4096])
def test_piece_count_builder(pb):
    g = W.piece_count_log(pb)
    counts = W.piece_counts(g)
    hot = g.info["hot"]
    assert sorted(hot.values()) == [1, 2, 3, 63, 64, 65, 66, 130] == sorted(W.HOT_COUNTS)
    assert all(counts[p] == c for p, c in hot.items())
    assert g.n == sum(W.HOT_COUNTS) + W.N_SCATTERED and g.slots == 2
    assert sorted(counts.values()).count(1) == W.N_SCATTERED + 1 and len(counts) == W.N_SCATTERED + 8
    pieces = W.pieces_by_page(pb, g.dst, g.src_off, g.lens)
    for p in hot:  # every piece of a hot page covers its middle byte; they lie all through the log
        assert all(lo <= pb // 2 < hi for _, lo, hi, _ in pieces[p])
    idx = [i for i, *_ in pieces[max(hot, key=hot.get)]]
    assert idx[0] < g.n // 8 and idx[-1] > g.n - g.n // 8
    assert sum(b.n for b in g.split(3)) == g.n and all(b.n > 64 for b in g.split(3))


@pytest.mark.parametrize("pb", [256, 2048, 4096])
def test_small_distinct_builder(pb):
    g = W.small_distinct_log(pb)
    counts = W.piece_counts(g)
    assert g.n == 64 and g.slots == 2 and len(counts) == 128 and set(counts.values()) == {1}
    assert (g.dst // pb + 1 == (g.dst + g.lens - 1) // pb).all()  # each straddles one border


@pytest.mark.parametrize("block,pb", sorted(W.ALIGNED_GEOMETRY))
def test_block_aligned_builder(block, pb):
    g = W.block_aligned_log(block, pb)
    max_len, slots = W.ALIGNED_GEOMETRY[block, pb]
    assert (g.max_len, g.slots) == (max_len, slots) and g.n == W.ALIGNED_N and g.n * g.slots <= 60000
    assert max_len == block * W.aligned_k_max(block, pb) and (max_len == 32 * block or g.n * W.log_slots(
        max_len + block, pb) > 60000)
    # zero unaligned writes: offset, length and source offset
    assert not (g.dst % block).any() and not (g.lens % block).any() and not (g.src_off % block).any()
    assert g.pool_bytes <= 64 << 20
    lens = g.lens.astype(np.int64)
    assert lens.max() == max_len and (lens == block).sum() >= 200 and (lens > block).sum() >= 100
    at = (g.dst // block).astype(np.int64)
    one = at[lens == block]
    assert (one == g.info["hot_block"]).sum() == W.ALIGNED_HOT
    assert all((one == b).sum() == 2 for b in g.info["twice"]) and len(g.info["twice"]) == 20
    if pb <= block:  # the hot block's pages: whole-page pieces, more than a page walks
        counts = W.piece_counts(g)
        p0 = g.info["hot_block"] * block // pb
        assert all(counts[p0 + j] >= W.ALIGNED_HOT > 64 for j in range(block // pb))
        pieces = W.pieces_by_page(pb, g.dst, g.src_off, g.lens)
        assert all((lo, hi, sh) == (0, pb, 0) for pcs in pieces.values() for _, lo, hi, sh in pcs)
    assert all(b.n > 64 for b in g.split(3))


@pytest.mark.parametrize("pb", [256, 4096])
def test_long_unaligned_builder(pb):
    g = W.long_unaligned_log(pb)
    assert g.n == 200 and g.max_len == 32 * pb + 1 and g.slots == 34 and g.n * g.slots <= 60000
    lens = g.lens.astype(np.int64)
    assert lens.min() >= 1 and lens.max() == g.max_len and (lens <= 2 * pb).sum() >= 50
    assert ((g.dst % 4 != 0) | (lens % 4 != 0)).sum() >= 150 and g.pool_bytes <= 64 << 20
    assert max(W.piece_counts(g).values()) >= 3


def test_explain_names_the_classes():
    g = W.two_piece_log(512, True)
    page = int(g.info["pages"][0])
    text = W.explain(512, page, g.dst, g.src_off, g.lens)
    pcs = W.pieces_by_page(512, g.dst, g.src_off, g.lens)[page]
    assert "page %d of 512 B: 2 piece(s), log indices %s" % (page, [p[0] for p in pcs]) in text
    for i, lo, hi, sh in pcs:
        byte = W.classify(lo, hi, sh, 512).byte
        assert "write %d: bytes [%d, %d) sh %d  byte class %s" % (i, lo, hi, sh, byte) in text
    assert "no write touches it" in W.explain(512, g.pool_bytes // 512 + 5, g.dst, g.src_off, g.lens)


def test_apply_in_order_later_write_wins():
    host = np.zeros(16, np.uint8)
    src = np.arange(1, 17, dtype=np.uint8)
    want = W.apply_in_order(host, np.array([2, 4], np.uint64), np.array([0, 8], np.uint64), np.array([4, 3], np.uint32),
                            src)
    assert want.tolist() == [0, 0, 1, 2, 9, 10, 11, 0, 0, 0, 0, 0, 0, 0, 0, 0] and not host.any()
