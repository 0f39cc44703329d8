"""The write log (cc_apply_log_dev, cc_apply_log_delta_dev, cc_apply_logs_dev)
on the shapes of tests/write_shapes.py: every class of piece on the one-piece,
two-piece, list and replay paths, at every page size (2 KiB, M = 8, included),
block-aligned writes as the reference admits them, long writes with many
slots, and the piece counts at which a page changes path.

Every case compares the pool bytes with in-order application and every page
CRC with the oracle's CRC of the final bytes, bit-exact.  Full mode starts
from a CRC table of sentinels (a touched page's CRC must be recomputed, an
untouched page's entry must survive); delta mode starts from the oracle's CRCs
on the touched pages, so it must end at the same table.  A failure names the
first wrong page and the class of every piece in it (write_shapes.explain);
tests/test_write_shapes.py pins on the CPU what each builder contains.
"""
import numpy as np
import pytest

import write_shapes as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def run(dev, oracle, logs, delta, queue=False, seed=0):
    """Apply `logs` (Log objects over one pool, in order; queue=True: as one
    cc_apply_logs_dev call) and check bytes, CRCs and the untouched pages."""
    from curve_amd import crc as C
    pb, pool_bytes, max_len = logs[0].pb, logs[0].pool_bytes, logs[0].max_len
    assert all((g.pb, g.pool_bytes, g.max_len) == (pb, pool_bytes, max_len) for g in logs)
    n_pages = pool_bytes // pb
    rng = np.random.default_rng([seed, pb, n_pages])
    host = rng.integers(0, 256, pool_bytes, dtype=np.uint8)
    dst = np.concatenate([g.dst for g in logs])
    lens = np.concatenate([g.lens for g in logs])
    # one source buffer for the explain() of a failure: batch b's offsets moved behind batch b-1's buffer
    src = np.concatenate([g.src for g in logs])
    bases = np.cumsum([0] + [g.src.size for g in logs[:-1]])
    src_off = np.concatenate([g.src_off + np.uint64(b) for g, b in zip(logs, bases)])
    want = W.apply_in_order(host, dst, src_off, lens, src)
    touched = np.zeros(n_pages, bool)
    touched[W.touched_pages(pb, dst, lens)] = True
    sentinel = (np.arange(n_pages, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0xDEADBEEF)
    want_crcs = np.where(touched, oracle.page_crcs(want, pb), sentinel)
    start = np.where(touched, oracle.page_crcs(host, pb), sentinel) if delta else sentinel
    d_pool, crcs = to_dev(host, dev), to_dev(start.view(np.int32), dev)
    batches = [(to_dev(g.src, dev), torch.from_numpy(C.log_records(g.dst, g.src_off, g.lens).view(np.uint8)).to(dev),
                g.n) for g in logs]
    if queue:
        C.apply_logs(d_pool, crcs, batches, max_len, pb, delta=delta)
    else:
        for d_src, d_log, n in batches:
            C.apply_log(d_pool, crcs, d_src, d_log, n, max_len, pb, delta=delta)
    torch.cuda.synchronize()
    got, got_crcs = d_pool.cpu().numpy(), u32(crcs)
    what = "pb %d, %s, %d write(s) in %d %s, max_len %d (%d slots)" % (
        pb, "delta" if delta else "full", dst.size, len(logs), "queued batch(es)" if queue else "call(s)", max_len,
        logs[0].slots)
    bad = np.flatnonzero((got != want).reshape(n_pages, pb).any(axis=1))
    if bad.size:
        p = int(bad[0])
        at = p * pb + int(np.flatnonzero(got[p * pb:(p + 1) * pb] != want[p * pb:(p + 1) * pb])[0])
        pytest.fail("%s: %d page(s) with wrong bytes, first at page byte %d (got %#04x, want %#04x)\n%s" % (
            what, bad.size, at - p * pb, got[at], want[at], W.explain(pb, p, dst, src_off, lens)), pytrace=False)
    bad = np.flatnonzero(got_crcs != want_crcs)
    if bad.size:
        p = int(bad[0])
        pytest.fail("%s: bytes right, %d page CRC(s) wrong, first got %#010x, want %#010x (%s)\n%s" % (
            what, bad.size, got_crcs[p], want_crcs[p], "touched" if touched[p] else "UNTOUCHED: the sentinel",
            W.explain(pb, p, dst, src_off, lens)), pytrace=False)
    assert (got[np.repeat(~touched, pb)] == host[np.repeat(~touched, pb)]).all()  # (implied by the above)
    return int(touched.sum())


@pytest.fixture(scope="module")
def matrices():
    return {}


@pytest.mark.parametrize("delta", [False, True], ids=["full", "delta"])
@pytest.mark.parametrize("pb", W.PAGE_SIZES)
def test_single_piece_matrix(dev, oracle, matrices, pb, delta):
    """(a) One page per (rlo, rhi, sh) of the matrix, all in one call on the
    table path (n = 1,012 / 3,960 > 64, max_len = pb, 2 slots): full mode takes
    load_rows_sel + fetch_edges + merge_edges, delta load_rows with the row
    mask + fetch_piece + merge_piece.  40 spare pages stay untouched, their CRC
    entries too."""
    m = matrices.get(pb) or matrices.setdefault(pb, W.single_piece_matrix(pb, seed=3, spare=40))
    assert m.n > 64 and m.max_len == pb and m.slots == 2
    assert run(dev, oracle, [m], delta) == m.n == m.pool_bytes // pb - 40


@pytest.mark.parametrize("path", ["small", "two_first", "two_last", "three"])
@pytest.mark.parametrize("delta", [False, True], ids=["full", "delta"])
@pytest.mark.parametrize("pb", W.PAGE_SIZES)
def test_generic_merge_by_class(dev, oracle, pb, delta, path):
    """(b) The 136 byte-class representatives through the one-launch path
    (three logs of <= 64 writes), as one of exactly two overlapping pieces a
    page (the partner earlier / later in the log: both ranks of cnt == 2), and
    as one of exactly three."""
    if path == "small":
        logs = W.small_path_logs(pb)
        assert all(g.n <= 64 and g.slots == 2 for g in logs)
    elif path == "three":
        logs = [W.three_piece_log(pb)]
    else:
        logs = [W.two_piece_log(pb, partner_first=path == "two_first")]
    assert run(dev, oracle, logs, delta) == 136


@pytest.mark.parametrize("queue", [False, True], ids=["one_call", "three_batches"])
@pytest.mark.parametrize("delta", [False, True], ids=["full", "delta"])
@pytest.mark.parametrize("pb", [4096, 2048])
def test_piece_count_boundaries(dev, oracle, pb, delta, queue):
    """(c) Pages with exactly 1, 2, 3, 63, 64 (the longest list a page walks),
    65, 66 and 130 (its wave replays the log) overlapping pieces among 2,000
    scattered one-piece pages, as one call and as a queue of three batches."""
    g = W.piece_count_log(pb)
    assert run(dev, oracle, g.split(3) if queue else [g], delta, queue=queue) == W.N_SCATTERED + 8


@pytest.mark.parametrize("delta", [False, True], ids=["full", "delta"])
@pytest.mark.parametrize("pb", [256, 2048, 4096])
def test_small_log_all_distinct_pages(dev, oracle, pb, delta):
    """(d) 64 writes straddling two pages of their own each: 128 distinct
    pages on the one-launch path."""
    g = W.small_distinct_log(pb)
    assert g.n == 64 and g.slots == 2
    assert run(dev, oracle, [g], delta) == 128


@pytest.mark.parametrize("delta", [False, True], ids=["full", "delta"])
@pytest.mark.parametrize("block,pb,queue", [(b, p, False) for b, p in sorted(W.ALIGNED_GEOMETRY)]
                         + [(4096, 4096, True), (512, 4096, True)])
def test_block_aligned_writes(dev, oracle, block, pb, queue, delta):
    """(e) 320 writes with offset, length and source offset multiples of the
    block size: no edge row, no partial dword, every row from the source.
    (block, pb) -> max_len, slots: (4096, 4096) 128 KiB, 33; (512, 4096) 16 KiB,
    5; (512, 512) 16 KiB, 33; (4096, 512) 92 KiB, 185; (4096, 2048) 128 KiB, 65;
    (4096, 256) 44 KiB, 177; (4096, 8192) 128 KiB, 17 -- at most 60,000 pieces.
    60 + 140 one-block writes leave most of their slots empty; 20 blocks are
    written twice and one 100 times (whole-page pieces through the replay)."""
    g = W.block_aligned_log(block, pb)
    assert (g.max_len, g.slots) == W.ALIGNED_GEOMETRY[block, pb] and g.n * g.slots <= 60000
    run(dev, oracle, g.split(3) if queue else [g], delta, queue=queue)


@pytest.mark.parametrize("delta", [False, True], ids=["full", "delta"])
@pytest.mark.parametrize("pb", [4096, 256])
def test_long_writes_unaligned(dev, oracle, pb, delta):
    """(f) 200 byte-unaligned writes of 1 B .. 32 pages + 1 (max_len = 32 pb +
    1: 34 slots a write, most of them empty for the short ones)."""
    g = W.long_unaligned_log(pb)
    assert g.max_len == 32 * pb + 1 and g.slots == 34
    run(dev, oracle, [g], delta)
