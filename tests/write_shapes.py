"""Write-log piece shapes: the classes a piece of a write can fall into inside
its page, and the builders of the logs tests/test_write_shapes_gpu.py applies.
No test lives here; tests/test_write_shapes.py pins, on the CPU, what every
builder contains, so a generator that drifts fails there instead of thinning
the GPU test.

A PIECE is the part of one write inside one page: page bytes [rlo, rhi) and
sh = (src - dst) & 3, the byte shift between the source and the page dwords
(what fetch_piece / fetch_edges of curve_amd/csrc/kernels.hip compute from
sp & 3: the source buffer is dword aligned and a page starts on a multiple of
256).  Lane l of the owning wave holds page dwords l + 64 j: row j is page
bytes [256 j, 256 j + 256), M = page_bytes / 256 rows a page.
"""
from collections import namedtuple

import numpy as np

PAGE_SIZES = (256, 512, 1024, 2048, 4096, 8192)

# byte  (rlo & 3, rhi & 3, sh, (partial first dword, partial last dword distinct from it, a wholly covered dword))
# row   (rlo & 255 != 0, rhi & 255 != 0, row0 == row1, rows covered whole: "none" / "some" / "all")
# flags (rlo == 0, rhi == pb, a partial dword in lane 63 of its row, a partial dword in lane 0)
PieceClass = namedtuple("PieceClass", "byte row flags")


def log_slots(max_len, pb):
    """Pieces the write log reserves per write (log_slots of engine.hip): a
    write of max_len bytes touches at most (max_len - 1) // pb + 2 pages."""
    return (max_len - 1) // pb + 2


def candidate_offsets(pb):
    """Offsets within 5 bytes of a page end, of byte 256 (a row end), of the
    page's middle and of 256 bytes before its end."""
    return sorted({c + d for c in (0, 256, pb // 2, pb - 256, pb) for d in range(-5, 6) if 0 <= c + d <= pb})


def classify(rlo, rhi, sh, pb):
    """The class of the piece [rlo, rhi) with source shift sh in a page of pb
    bytes, from the numbers alone (piece_edges, edge_rows and covered_rows of
    kernels.hip decide by the same quantities)."""
    assert 0 <= rlo < rhi <= pb and 0 <= sh < 4
    df, dl = rlo >> 2, (rhi - 1) >> 2
    first_whole = rlo & 3 == 0 and 4 * df + 4 <= rhi
    last_whole = rhi & 3 == 0 and 4 * dl >= rlo
    part_first = not first_whole
    part_last = dl != df and not last_whole
    whole = (rhi >> 2) > ((rlo + 3) >> 2)
    byte = (rlo & 3, rhi & 3, sh, (part_first, part_last, whole))
    row0, row1 = rlo >> 8, (rhi - 1) >> 8
    f0, f1 = (rlo + 255) >> 8, rhi >> 8
    cov = "none" if f1 <= f0 else ("all" if f1 - f0 == pb // 256 else "some")
    row = (rlo & 255 != 0, rhi & 255 != 0, row0 == row1, cov)
    edges = ([df] if part_first else []) + ([dl] if part_last else [])
    flags = (rlo == 0, rhi == pb, any(e & 63 == 63 for e in edges), any(e & 63 == 0 for e in edges))
    return PieceClass(byte, row, flags)


def class_sets(pieces, pb):
    """(byte classes, row classes, flag tuples) of an iterable of (rlo, rhi, sh)."""
    cls = [classify(rlo, rhi, sh, pb) for rlo, rhi, sh in pieces]
    return {c.byte for c in cls}, {c.row for c in cls}, {c.flags for c in cls}


class Log:
    """One write log over a pool of pool_bytes (a multiple of pb): the writes
    in log order, their source buffer and the max_len the call is given."""

    def __init__(self, pb, pool_bytes, max_len, dst, src_off, lens, src, **info):
        self.pb, self.pool_bytes, self.max_len = pb, pool_bytes, max_len
        self.dst = np.asarray(dst, np.uint64)
        self.src_off = np.asarray(src_off, np.uint64)
        self.lens = np.asarray(lens, np.uint32)
        self.src = src
        self.info = info
        self.check()

    n = property(lambda self: int(self.dst.size))
    slots = property(lambda self: log_slots(self.max_len, self.pb))

    def check(self):
        """No builder breaks the call contract: every write lies inside the
        pool, every source range inside src, 1 <= len <= max_len."""
        d, s, m = self.dst.astype(np.int64), self.src_off.astype(np.int64), self.lens.astype(np.int64)
        assert d.size == s.size == m.size and d.size >= 1
        assert self.pool_bytes % self.pb == 0 and self.src.dtype == np.uint8 and self.src.size % 4 == 0
        assert (m >= 1).all() and (m <= self.max_len).all()
        assert (d >= 0).all() and (d + m <= self.pool_bytes).all()
        assert (s >= 0).all() and (s + m <= self.src.size).all()

    def split(self, parts):
        """The log cut into `parts` consecutive batches (a queue for apply_logs)."""
        cuts = [self.n * k // parts for k in range(parts + 1)]
        return [Log(self.pb, self.pool_bytes, self.max_len, self.dst[a:b], self.src_off[a:b], self.lens[a:b],
                    self.src) for a, b in zip(cuts, cuts[1:])]


def apply_in_order(host, dst, src_off, lens, src):
    """The reference: the writes applied to a copy of `host` one after another."""
    want = host.copy()
    for d, s, m in zip(dst.tolist(), src_off.tolist(), lens.tolist()):
        want[d:d + m] = src[s:s + m]
    return want


def pieces_by_page(pb, dst, src_off, lens):
    """page -> [(log index, rlo, rhi, sh)] in log order."""
    out = {}
    for i, (d, s, m) in enumerate(zip(np.asarray(dst).tolist(), np.asarray(src_off).tolist(),
                                      np.asarray(lens).tolist())):
        for p in range(d // pb, (d + m - 1) // pb + 1):
            out.setdefault(p, []).append((i, max(d, p * pb) - p * pb, min(d + m, (p + 1) * pb) - p * pb, (s - d) & 3))
    return out


def touched_pages(pb, dst, lens):
    d, m = np.asarray(dst).astype(np.int64), np.asarray(lens).astype(np.int64)
    p0, cnt = d // pb, (d + m - 1) // pb - d // pb + 1
    start = np.repeat(p0 - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt)
    return np.unique(start + np.arange(int(cnt.sum()), dtype=np.int64))


def explain(pb, page, dst, src_off, lens):
    """For assertion messages: the pieces of `page`, each with its log index,
    byte range and class."""
    pcs = pieces_by_page(pb, dst, src_off, lens).get(int(page), [])
    if not pcs:
        return "page %d of %d B: no write touches it" % (page, pb)
    lines = ["page %d of %d B: %d piece(s), log indices %s" % (page, pb, len(pcs), [i for i, _, _, _ in pcs])]
    for i, rlo, rhi, sh in pcs:
        c = classify(rlo, rhi, sh, pb)
        lines.append("  write %d: bytes [%d, %d) sh %d  byte class %s  row class %s  flags %s"
                     % (i, rlo, rhi, sh, c.byte, c.row, c.flags))
    return "\n".join(lines)


def _src_offsets(rng, dst, sh, span):
    """Random source offsets below span + 4 with (src - dst) & 3 == sh."""
    base = rng.integers(0, span // 4, len(dst)).astype(np.int64) * 4
    return base + ((np.asarray(sh, np.int64) + np.asarray(dst, np.int64)) & 3)


def _src(rng, span, max_len):
    return rng.integers(0, 256, (span + max_len + 11) // 4 * 4, dtype=np.uint8)


SRC_SPAN = 1 << 16


def _page_log(pb, pages, pieces, rng, n_pages, **info):
    """Writes that each stay inside one page: piece k = (rlo, rhi, sh) on page pages[k]."""
    rlo = np.array([p[0] for p in pieces], np.int64)
    rhi = np.array([p[1] for p in pieces], np.int64)
    sh = np.array([p[2] for p in pieces], np.int64)
    dst = np.asarray(pages, np.int64) * pb + rlo
    return Log(pb, n_pages * pb, pb, dst, _src_offsets(rng, dst, sh, SRC_SPAN), rhi - rlo, _src(rng, SRC_SPAN, pb),
               pages=np.asarray(pages, np.int64), pieces=list(pieces), **info)


def matrix_pieces(pb):
    offs = candidate_offsets(pb)
    return [(lo, hi, sh) for a, lo in enumerate(offs) for hi in offs[a + 1:] for sh in range(4)]


def single_piece_matrix(pb, seed=0, spare=0):
    """One write per page, one page per (rlo < rhi from candidate_offsets(pb))
    x sh in 0..3, in shuffled page order: 1,012 writes at 256 and 512 B, 3,960
    from 1 KiB up, over a pool of writes + spare pages (the spare ones stay
    untouched).  info: pages, pieces (as written), classes {page: PieceClass}."""
    rng = np.random.default_rng([seed, pb, 1])
    pieces = matrix_pieces(pb)
    n_pages = len(pieces) + spare
    pages = rng.permutation(n_pages)[:len(pieces)]
    log = _page_log(pb, pages, pieces, rng, n_pages)
    log.info["classes"] = {int(p): classify(*pc, pb) for p, pc in zip(pages, pieces)}
    return log


def class_representatives(pb):
    """One (rlo, rhi, sh) per reachable byte class, 136 of them, taken from the
    matrix in a fixed shuffled order (so they spread over the row classes)."""
    pieces = matrix_pieces(pb)
    rng = np.random.default_rng([pb, 2])
    reps = {}
    for k in rng.permutation(len(pieces)):
        reps.setdefault(classify(*pieces[k], pb).byte, pieces[k])
    return [reps[c] for c in sorted(reps)]


def small_path_logs(pb, seed=0, spare=8):
    """The representatives as three logs of at most 64 single-page writes on
    pages of their own (max_len = pb, 2 slots: the one-launch path)."""
    rng = np.random.default_rng([seed, pb, 3])
    reps = class_representatives(pb)
    n_pages = len(reps) + spare
    pages = rng.permutation(n_pages)[:len(reps)]
    cuts = [len(reps) * k // 3 for k in range(4)]
    return [_page_log(pb, pages[a:b], reps[a:b], rng, n_pages) for a, b in zip(cuts, cuts[1:])]


def _partner(rng, rep, pb, half):
    """A write inside the page that overlaps the first (half 0) or the second
    (half 1) half of rep and runs a few bytes beyond it."""
    rlo, rhi, _ = rep
    mid = rlo + (rhi - rlo) // 2
    if half:
        lo, hi = mid, min(pb, rhi + int(rng.integers(0, 9)))
    else:
        lo, hi = max(0, rlo - int(rng.integers(0, 9))), mid + 1
    return (lo, hi, int(rng.integers(0, 4)))


def _shuffled_pages_log(pb, per_page, rng, spare, **info):
    """per_page[k]: the pieces of page k in the order they must have in the
    log; the writes of different pages are interleaved at random."""
    n_pages = len(per_page) + spare
    pages = rng.permutation(n_pages)[:len(per_page)]
    total = sum(len(p) for p in per_page)
    owner = rng.permutation(np.repeat(np.arange(len(per_page)), [len(p) for p in per_page]))
    taken = [0] * len(per_page)
    pieces, pg = [], []
    for k in owner.tolist():
        pieces.append(per_page[k][taken[k]])
        pg.append(pages[k])
        taken[k] += 1
    assert len(pieces) == total
    return _page_log(pb, pg, pieces, rng, n_pages, page_of=pages, **info)


def two_piece_log(pb, partner_first, seed=0, spare=8):
    """Every page gets its representative and a partner overlapping its second
    half, the partner earlier (partner_first) or later in the log: 272 writes,
    exactly two pieces a page, on the table path (max_len = pb, 2 slots)."""
    rng = np.random.default_rng([seed, pb, 4, int(partner_first)])
    per_page = []
    for rep in class_representatives(pb):
        other = _partner(rng, rep, pb, 1)
        per_page.append([other, rep] if partner_first else [rep, other])
    return _shuffled_pages_log(pb, per_page, rng, spare)


def three_piece_log(pb, seed=0, spare=8):
    """Every page gets its representative and two partners (one over each
    half), the three in a random log order: 408 writes, three pieces a page."""
    rng = np.random.default_rng([seed, pb, 5])
    per_page = []
    for rep in class_representatives(pb):
        three = [rep, _partner(rng, rep, pb, 0), _partner(rng, rep, pb, 1)]
        per_page.append([three[k] for k in rng.permutation(3)])
    return _shuffled_pages_log(pb, per_page, rng, spare)


HOT_COUNTS = (1, 2, 3, 63, 64, 65, 66, 130)  # 64: the longest list a page walks; 65: its wave replays the log
N_SCATTERED = 2000


def piece_count_log(pb, seed=0, spare=8):
    """Eight pages receive exactly HOT_COUNTS pieces, every one of them covering
    the page's middle byte (so they overlap and log order decides the bytes),
    interleaved with N_SCATTERED single-piece writes on pages of their own.
    info: hot {page: count}."""
    rng = np.random.default_rng([seed, pb, 6])
    per_page = []
    for c in HOT_COUNTS:
        lo = rng.integers(0, pb // 2 + 1, c)
        hi = rng.integers(pb // 2 + 1, pb + 1, c)
        per_page.append([(int(a), int(b), int(s)) for a, b, s in zip(lo, hi, rng.integers(0, 4, c))])
    for _ in range(N_SCATTERED):
        lo = int(rng.integers(0, pb))
        per_page.append([(lo, int(rng.integers(lo + 1, pb + 1)), int(rng.integers(0, 4)))])
    log = _shuffled_pages_log(pb, per_page, rng, spare)
    log.info["hot"] = {int(p): c for p, c in zip(log.info["page_of"], HOT_COUNTS)}
    return log


def small_distinct_log(pb, seed=0, spare=8):
    """64 writes of at most pb bytes, each straddling the border between two
    pages of its own: 128 distinct pages, the most the one-launch path sees."""
    rng = np.random.default_rng([seed, pb, 7])
    n_pages = 128 + spare
    pairs = rng.permutation(n_pages // 2)[:64]
    a = rng.integers(1, pb, 64)            # bytes in the first page
    b = rng.integers(1, pb - a + 1)        # bytes in the second: a + b <= pb
    dst = (2 * pairs + 1) * pb - a
    sh = rng.integers(0, 4, 64)
    return Log(pb, n_pages * pb, pb, dst, _src_offsets(rng, dst, sh, SRC_SPAN), a + b, _src(rng, SRC_SPAN, pb))


# (block, pb) -> (max_len, slots): max_len = block * k_max, k_max the largest
# k <= 32 with ALIGNED_N * log_slots(block * k, pb) <= 60,000 pieces
ALIGNED_N = 320  # 120 of 1..k_max blocks + 60 of one block + 20 blocks written twice + one block written 100 times
ALIGNED_GEOMETRY = {
    (4096, 4096): (131072, 33),
    (512, 4096): (16384, 5),
    (512, 512): (16384, 33),
    (4096, 512): (94208, 185),
    (4096, 2048): (131072, 65),
    (4096, 256): (45056, 177),
    (4096, 8192): (131072, 17),
}
ALIGNED_HOT = 100


def aligned_k_max(block, pb, n=ALIGNED_N, pieces=60000):
    return max(k for k in range(1, 33) if n * log_slots(block * k, pb) <= pieces)


def block_aligned_log(block, pb, seed=0):
    """ALIGNED_N writes whose offset, length and source offset are multiples of
    `block` (what the reference's CheckRequestOffsetAndLength admits), in
    random log order: 120 of 1..k_max blocks, 60 of one block (most of their
    slots empty beside the long ones), 20 blocks written twice and one block
    written ALIGNED_HOT times.  info: hot_block, twice (block indices)."""
    rng = np.random.default_rng([seed, block, pb, 8])
    k_max = aligned_k_max(block, pb)
    max_len = block * k_max
    n_blocks = 2048
    pool_bytes = n_blocks * block
    k = np.concatenate((rng.integers(1, k_max + 1, 120), np.ones(60 + 40 + ALIGNED_HOT, np.int64)))
    k[:2] = (k_max, 1)
    special = rng.permutation(n_blocks - k_max)[:21]
    at = rng.integers(0, n_blocks - k_max, k.size)
    for i in range(180):  # the other writes keep off the blocks written twice / ALIGNED_HOT times
        while ((special >= at[i]) & (special < at[i] + k[i])).any():
            at[i] = rng.integers(0, n_blocks - k_max)
    at[180:220] = np.repeat(special[:20], 2)
    at[220:] = special[20]
    src_blocks = SRC_SPAN // block + 1
    order = rng.permutation(k.size)
    k, at = k[order], at[order]
    src = rng.integers(0, 256, (src_blocks + k_max) * block, dtype=np.uint8)
    return Log(pb, pool_bytes, max_len, at * block, rng.integers(0, src_blocks, k.size) * block, k * block, src,
               block=block, hot_block=int(special[20]), twice=sorted(special[:20].tolist()))


def long_unaligned_log(pb, seed=0):
    """200 byte-unaligned writes of 1 B .. max_len = 32 pages + 1 (34 slots;
    every fourth at most two pages long) over 2,048 pages."""
    rng = np.random.default_rng([seed, pb, 9])
    n, max_len, pool_bytes = 200, 32 * pb + 1, 2048 * pb
    lens = rng.integers(1, max_len + 1, n)
    lens[::4] = rng.integers(1, 2 * pb + 1, lens[::4].size)
    lens[1] = max_len
    dst = rng.integers(0, pool_bytes - lens + 1)
    span = 1 << 18
    return Log(pb, pool_bytes, max_len, dst, _src_offsets(rng, dst, rng.integers(0, 4, n), span), lens,
               _src(rng, span, max_len))


def piece_counts(log):
    """{page: pieces} of a log."""
    return {p: len(v) for p, v in pieces_by_page(log.pb, log.dst, log.src_off, log.lens).items()}
