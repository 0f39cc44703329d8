"""Batch shapes for the gathered page kernels (cc_verify_reads_dev,
cc_read_snap_dev, cc_read_merge_dev, cc_paste_dev, cc_repair_dev): what the
slot schedule of kernels.hip (rv_begin, rv_next, rv_walk and the copies in
merge_read_kernel and repair_kernel) decides differently on.  No GPU here.

A shape is a list of entries (first_page, n_pages, kind) on a pool of
n_pages_pool pages, page-aligned throughout:
  VALID    n_pages >= 1 pages inside the pool: n_pages slots;
  EMPTY    length 0 (first_page inside the pool): no slot, counted as 0;
  INVALID  past the pool (it starts at its end, far past it, or runs over it):
           no slot, marked UINT32_MAX by every call.
Every shape has at least 65 entries (the tiled kernels; up to 64 entries go to
the one-launch kernels, which have tests of their own).  Every generator is
seeded: the same arguments give the same batch in every process.

The schedule's constants (kernels.hip): kRvMinSlots 8, kRvDynDiv 16,
kRvDynSlots 32, kReadTiles 512, kRvWaves 8; Wg = 8 x the grid.
"""
import os

import numpy as np

VALID, EMPTY, INVALID = "valid", "empty", "invalid"
MIN_ENTRIES = 65
WAVES = 8                  # kRvWaves
N_POOL = 320               # the suite's small rigs: 8 chunks of 40 pages
LONG_POOL = 3000           # `long`'s pool (8 chunks of 375 pages)


def grid():
    """Workgroups of every gathered launch: $CC_TEST_CUS when set (the engine
    reads it when the device context is made), else the device's CU count."""
    if os.environ.get("CC_TEST_CUS"):
        return int(os.environ["CC_TEST_CUS"])
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def waves():
    return WAVES * grid()


def EDGES(Wg):
    """The slot totals at which the schedule changes its mind.
    0: no slot at all.  8, 9: W = min(ceil(T / 8), Wg) goes 1 -> 2.  63, 64, 65:
    one group of 64, and the second workgroup's first wave.  511, 512, 528: the
    dynamic tail T / 16 is 31 slots (one short chunk), 32 (one exact chunk), 33
    (a full chunk and a chunk of one slot).  1023: what paste's and repair's own
    edge tests use.  8 Wg - 1, 8 Wg, 8 Wg + 1: W reaches the grid."""
    return sorted({0, 1, 8, 9, 63, 64, 65, 511, 512, 528, 1023, 8 * Wg - 1, 8 * Wg, 8 * Wg + 1})


# the same totals by name, so that a case keeps its id at every grid (at 8 waves 8 Wg is 64 again)
EDGE_NAMES = ["0", "1", "8", "9", "63", "64", "65", "511", "512", "528", "1023", "8Wg-1", "8Wg", "8Wg+1"]


def edge_total(name, Wg):
    at_grid = {"8Wg-1": 8 * Wg - 1, "8Wg": 8 * Wg, "8Wg+1": 8 * Wg + 1}
    return at_grid[name] if name in at_grid else int(name)


def _invalid(rng, n_pool, j):
    """An entry past the pool, one of three kinds in turn."""
    return [(n_pool, 1, INVALID), (n_pool + (1 << 28), int(rng.integers(1, 9)), INVALID),
            (n_pool - 1, 2, INVALID)][j % 3]


def _valid(rng, n_pool, k):
    return (int(rng.integers(0, n_pool - k + 1)), k, VALID)


def _empty(rng, n_pool):
    return (int(rng.integers(0, n_pool)), 0, EMPTY)


def exact(total, n_pool=N_POOL, seed=0):
    """Valid entries of 1-8 pages whose page counts sum to `total` exactly,
    padded with EMPTY entries at random positions up to 65 entries.  total == 0:
    65 entries, EMPTY at the even indices and INVALID at the odd ones."""
    rng = np.random.default_rng([seed, total, n_pool])
    if total == 0:
        return [_empty(rng, n_pool) if i % 2 == 0 else _invalid(rng, n_pool, i // 2) for i in range(MIN_ENTRIES)]
    out, left = [], total
    while left:
        k = min(int(rng.integers(1, 9)), left)
        out.append(_valid(rng, n_pool, k))
        left -= k
    while len(out) < MIN_ENTRIES:
        out.insert(int(rng.integers(0, len(out) + 1)), _empty(rng, n_pool))
    return out


SPARSE_N = 2000
SPARSE_AT = (0, 63, 64, 127, 128, 1000, 1935, 1999)
SPARSE_INVALID = range(200, 500)


def sparse(n_pool=N_POOL, seed=0):
    """2000 entries (31 groups of 64 and a short one of 16); VALID of 1-40 pages
    only at SPARSE_AT, INVALID at [200, 500), EMPTY everywhere else: groups and
    tiles without a slot before, between and after the populated entries."""
    rng = np.random.default_rng([seed, 1, n_pool])
    out = []
    for i in range(SPARSE_N):
        if i in SPARSE_AT:
            out.append(_valid(rng, n_pool, int(rng.integers(1, 41))))
        elif i in SPARSE_INVALID:
            out.append(_invalid(rng, n_pool, i))
        else:
            out.append(_empty(rng, n_pool))
    return out


FEW = (65, 100, 511)


def few(n, n_pool=N_POOL, seed=0):
    """n < 512 VALID entries of 1-3 pages: fewer entries than tiles, so the
    tiles' entry ranges [n t / 512, n (t + 1) / 512) are empty or single."""
    rng = np.random.default_rng([seed, 2, n, n_pool])
    return [_valid(rng, n_pool, int(rng.integers(1, 4))) for _ in range(n)]


GIANT_N = 300
GIANT_AT = (0, 150, 299)


def giant(at, n_pool=N_POOL, seed=0):
    """300 VALID one-page entries, entry `at` replaced by one over the whole
    pool: every wave cuts it, and what is counted on it is counted by atomics."""
    rng = np.random.default_rng([seed, 3, at, n_pool])
    out = [_valid(rng, n_pool, 1) for _ in range(GIANT_N)]
    out[at] = (0, n_pool, VALID)
    return out


LONG_N = 130


def long(n_pool=LONG_POOL, seed=0):
    """130 VALID entries of n_pool / 6 .. n_pool pages (500-3000 on the
    3000-page pool): whole shares lie inside one entry and seeks land
    mid-group.  Meant for the smallest page size: ~227,000 slots."""
    rng = np.random.default_rng([seed, 4, n_pool])
    return [_valid(rng, n_pool, int(rng.integers(n_pool // 6, n_pool + 1))) for _ in range(LONG_N)]


SHAPE_NAMES = (["exact-" + e for e in EDGE_NAMES] + ["sparse"] + ["few-%d" % n for n in FEW] +
               ["giant-%d" % at for at in GIANT_AT] + ["long"])


def pool_pages(name):
    return LONG_POOL if name == "long" else N_POOL


def make(name, Wg):
    """The shape of that name at Wg waves, on the pool of pool_pages(name) pages."""
    kind, _, arg = name.partition("-")
    if kind == "exact":
        return exact(edge_total(arg, Wg))
    if kind == "few":
        return few(int(arg))
    if kind == "giant":
        return giant(int(arg))
    return {"sparse": sparse, "long": long}[kind]()


def slots(shape):
    """Page slots per entry (0 for EMPTY and INVALID) as int64."""
    return np.array([k if kind == VALID else 0 for _, k, kind in shape], np.int64)


def expected(shape):
    """What a call that counts every slot of every entry reports per entry:
    its pages, 0 for EMPTY, UINT32_MAX for INVALID."""
    return np.array([0xFFFFFFFF if kind == INVALID else k for _, k, kind in shape], np.uint32)


def byte_ranges(shape, pb):
    """The shape as [(offset, length)] in bytes."""
    return [(p0 * pb, k * pb) for p0, k, _ in shape]
