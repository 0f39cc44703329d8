"""The slot schedule of the gathered page kernels (rv_begin, rv_next, rv_walk
in kernels.hip, and the copies in merge_read_kernel and repair_kernel) at the
batch shapes of gather_shapes.py and at grids other than the device's own.

Every decision of that schedule depends on Wg = 8 waves x the grid, which on an
MI355X is always 256 workgroups; $CC_TEST_CUS (read when the device context is
made) sizes every grid for another CU count.  test_case runs every shape
through the five calls that take entries, test_case_scrub runs cc_scrub_dev
over pools whose geometry plays the shapes' part, both at the grid the process
has; test_other_grid runs the 4 KiB cases again in a child process at 1, 3, 63
and 304 workgroups:
    1    8 waves, 64 tiles a wave, W reaches the grid at 64 slots;
    3    24 waves do not divide 512 tiles: uneven tile and share splits;
    63   504 waves: some count two tiles and some one;
    304  more workgroups than fit beside each other: the waits give up and
         claim tiles (implied by the grid, not asserted).

"Every slot handled exactly once" is checked on ALL ROTTEN tables (every CRC
word XOR 1): a call then reports every page of every entry, so a slot the
schedule skips or takes twice changes a count.  The expected values are the
numpy models' (test_gather_shapes.py checks those against the generators' own
page counts without a device) and the oracle's CRCs, never the library's.

Page sizes: 4096 and, per call, one more: 1024 for paste and repair (their own
edge tests name it), 256 for the others.  `long` runs at 256 bytes only, so
that its ~227,000 slots stay quick for the models; the children run it too.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import gather_shapes as G
from test_clone_gpu import N_SLOTS, Rig as CloneRig, classes, to_dev, u32
from test_gather_shapes import (SCRUB_GEOMETRIES, paste_entries, present, rot, rot_scrub, scrub_expectation,
                                scrub_kwargs, total_geometry, trim_to_total, unwritten_mask, verify_model,
                                written_per_entry)
from test_read_merge import NO_ORIGIN
from test_read_merge_gpu import merged, same as same_merged, unchanged
from test_repair_gpu import rig_for
from test_scrub_gpu import DevRig
from test_snap_read import U32_MAX
from test_snap_read_gpu import filled_rig, same as same_view, view

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_CHUNKS = 8
CALLS = ["verify", "snap", "merge", "paste", "repair"]
OTHER_PB = {"verify": 256, "snap": 256, "merge": 256, "paste": 1024, "repair": 1024, "scrub": 256}
OTHER_GRIDS = [1, 3, 63, 304]                                # 304 last: the one that leaves workgroups waiting
CASES = [(call, name, pb) for call in CALLS for name in G.SHAPE_NAMES
         for pb in ([256] if name == "long" else [4096, OTHER_PB[call]])]
SCRUB_CASES = [(what, pb) for what in ["%dx%d" % g for g in SCRUB_GEOMETRIES] + ["8Wg+1", "plain"]
               for pb in (4096, OTHER_PB["scrub"])]
CHILD_SELECT = "test_case and (pb4096 or long)"              # never the wrapper itself
N_CHILD = len([c for c in CASES if c[2] == 4096 or c[1] == "long"]) + len([c for c in SCRUB_CASES if c[1] == 4096])
# The child's selection measured in-process at the native grid: 5.0 s of tests,
# and the children took 5.4 to 8.2 s each, interpreter start included; the
# limit is fifteen to twenty times that.
CHILD_TIMEOUT = 120


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from curve_amd import crc as C
    C.engine_init()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def rigs():
    """The rigs of the calls that only read, built once per (call, page size, pool)."""
    return {}


def rotten(tensor, *host):
    """XOR 1 into every word of a device table and its host mirrors (its own inverse)."""
    tensor.bitwise_xor_(1)
    for h in host:
        rot(h)


def split(shape):
    want = G.expected(shape)
    return want, want != U32_MAX, int(G.slots(shape).sum())


# --------------------------------------------------------------------------- one adapter a call
def run_verify(dev, oracle, rigs, shape, n_pool, pb):
    """bad_per_read[i] == pages of entry i, UINT32_MAX for an invalid one, 0 for an empty one; bad_total == T."""
    from curve_amd import crc as C
    key = ("verify", pb, n_pool)
    if key not in rigs:
        host = np.random.default_rng(pb + n_pool).integers(0, 256, n_pool * pb, dtype=np.uint8)
        stored = np.asarray(oracle.page_crcs(host, pb), np.uint32).copy()
        rot(stored)
        rigs[key] = (host, stored, to_dev(host, dev), to_dev(stored.view(np.int32), dev))
    host, stored, d_pool, d_crcs = rigs[key]
    reads = G.byte_ranges(shape, pb)
    want, ok, T = split(shape)
    model = verify_model(host, stored, reads, pb, oracle.page_crcs)
    assert (model == want).all()
    bad, total = C.verify_reads(d_pool, d_crcs, [r[0] for r in reads], [r[1] for r in reads], pb)
    torch.cuda.synchronize()
    bad = u32(bad)
    assert (bad == model).all(), np.nonzero(bad != model)[0][:10]
    assert int(total.item()) == T


def run_snap(dev, oracle, rigs, shape, n_pool, pb):
    """With an output: every delivered byte and every sentinel byte around the
    outputs equal the model's, nothing counted.  Then both tables rotten,
    without an output: every page of every entry counted."""
    key = ("snap", pb, n_pool)
    if key not in rigs:
        rigs[key] = filled_rig(dev, oracle, pb, seed=7, batches=(60,), ppc=n_pool // N_CHUNKS)
    rig = rigs[key]
    reads = G.byte_ranges(shape, pb)
    want, ok, T = split(shape)
    got, model = view(rig, oracle, reads, copy=True)
    same_view(got, model)
    assert got[2] == 0 and not got[1][ok].any() and (got[1][~ok] == U32_MAX).all()
    rotten(rig.crcs, rig.stored)
    rotten(rig.cow.snap_crcs, rig.scrc)
    try:
        got, model = view(rig, oracle, reads, copy=False)
    finally:
        rotten(rig.crcs, rig.stored)
        rotten(rig.cow.snap_crcs, rig.scrc)
    same_view(got, model)
    assert (got[1] == want).all(), np.nonzero(got[1] != want)[0][:10]
    assert got[2] == T


def run_merge(dev, oracle, rigs, shape, n_pool, pb):
    """Half the clone bits set: the output, gaps and all, equals the model's;
    then with the pool's table rotten bad == the entry's written pages."""
    key = ("merge", pb, n_pool)
    if key not in rigs:
        rigs[key] = CloneRig(dev, oracle, pb, seed=9, density=0.5, ppc=n_pool // N_CHUNKS,
                             src_pages=max(512, n_pool + 8))
    rig = rigs[key]
    reads = G.byte_ranges(shape, pb)
    want, ok, T = split(shape)
    # every fourth read has no origin; the others' origin bytes start at one of eight places
    origin_off = np.array([NO_ORIGIN if i % 4 == 3 else (i % 8) * pb for i in range(len(reads))], np.uint64)
    got, model = merged(rig, reads, origin_off)
    same_merged(got, model)
    written = written_per_entry(shape, unwritten_mask(rig.slots, rig.bm, n_pool // N_CHUNKS))
    assert got[2] == 0 and got[4] == T - int(written.sum())
    rotten(rig.crcs, rig.stored)
    try:
        got, model = merged(rig, reads, origin_off)
    finally:
        rotten(rig.crcs, rig.stored)
    same_merged(got, model)
    out, bad, bt, unw, ut = got
    assert (bad[~ok] == U32_MAX).all() and (unw[~ok] == U32_MAX).all()
    assert (bad[ok] == written[ok]).all(), np.nonzero(bad[ok] != written[ok])[0][:10]
    assert (bad[ok].astype(np.int64) + unw[ok] == want[ok]).all() and bt + ut == T
    unchanged(rig)


def run_paste(dev, oracle, rigs, shape, n_pool, pb):
    """Every bit clear (as the call's own edge test): pasted + lost + plain == T, and the rig in full.
    A slot the schedule skipped shows here only where it would have won its page: on the 320-page pool
    the late slots of a large batch mostly lose theirs to earlier entries (giant-299 is the shape whose
    last slots win; a tail chunk cut short failed that case alone)."""
    ppc = n_pool // N_CHUNKS
    rig = CloneRig(dev, oracle, pb, seed=11, density=0.0, ppc=ppc, src_pages=max(512, n_pool))
    entries = paste_entries(shape, pb)
    want, ok, T = split(shape)
    pasted, held, lost, plain = classes(entries, rig.slots, rig.bm, pb, rig.host.size, rig.src.size, ppc=ppc)
    assert held == 0 and pasted + lost + plain == T
    got, model = rig.paste(entries)
    assert got.tolist() == model.tolist()
    assert (got[~ok] == U32_MAX).all() and int(got[ok].sum()) == pasted == rig.total
    rig.check()


def run_repair(dev, oracle, rigs, shape, n_pool, pb):
    """Every (entry, page) pair lands in exactly one class: per-entry sums == pages, the totals sum to T; the
    rig (pool, tables, claim words, guards) in full against the model inside rig.call."""
    rig, _ = rig_for(dev, oracle, pb, 13, n=0, invalid=0, n_pages=n_pool, src_pages=max(512, n_pool))
    entries = paste_entries(shape, pb)                       # source page p: the first copy for pool page p
    want, ok, T = split(shape)
    got, totals = rig.call(entries)
    assert (got[~ok] == U32_MAX).all()
    assert (got[ok].sum(axis=1) == want[ok]).all(), np.nonzero(got[ok].sum(axis=1) != want[ok])[0][:10]
    assert int(sum(int(t) for t in totals)) == T
    rig.check()


RUN = {"verify": run_verify, "snap": run_snap, "merge": run_merge, "paste": run_paste, "repair": run_repair}


@pytest.mark.parametrize("call,name,pb", CASES, ids=["%s-%s-pb%d" % c for c in CASES])
def test_case(dev, oracle, rigs, call, name, pb):
    shape = G.make(name, G.waves())
    RUN[call](dev, oracle, rigs, shape, G.pool_pages(name), pb)


# --------------------------------------------------------------------------- scrub: its domain is the pool
@pytest.mark.parametrize("what,pb", SCRUB_CASES, ids=["scrub-%s-pb%d" % c for c in SCRUB_CASES])
def test_case_scrub(dev, oracle, what, pb):
    """Both tables rotten: `listed` == the pages that exist (max_list above it),
    the listed set, the per-chunk words and the three owed counts equal the
    model's and the bitmaps' own count.  8Wg+1: a pool trimmed, by its bitmaps,
    to exactly 8 Wg + 1 existing pages.  plain: neither struct."""
    if what == "8Wg+1":
        total = 8 * G.waves() + 1
        n_chunks, ppc = total_geometry(total)
    elif what == "plain":
        n_chunks, ppc = 16, 256
    else:
        n_chunks, ppc = (int(v) for v in what.split("x"))
    rig = DevRig(dev, oracle, pb, 90, max_list=2 * n_chunks * ppc + 8, **scrub_kwargs(n_chunks, ppc))
    if what == "8Wg+1":
        trim_to_total(rig.h, total)
    rot_scrub(rig.h)
    rig.upload()
    if what == "plain":
        cnt, ent, per = rig.check(cow=False, clone=False)    # against the model, list and per-chunk words included
        n = rig.h.n_pages
        assert cnt == dict(live_checked=n, live_bad=n, snap_checked=0, snap_bad=0, unwritten=0, listed=n)
        assert sorted(ent) == list(range(n)) and (per[:, 0] == ppc).all() and not per[:, 1].any()
        return
    cnt, ent, per = rig.check()
    scrub_expectation(rig.h, cnt, ent, per)
    assert what != "8Wg+1" or cnt["listed"] == total


# --------------------------------------------------------------------------- the same at other grids
@pytest.mark.parametrize("cus", OTHER_GRIDS)
def test_other_grid(dev, cus):
    """The 4 KiB cases above (and `long`) in one child process whose engine
    sizes every grid for `cus` CUs.  The children run one after another; a
    child that fails, dies by a signal or passes its time limit fails this
    test with the end of its output, and nothing is tried again."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CC_TEST_CUS=str(cus))
    t0 = time.monotonic()
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                            os.path.join(root, "tests", "test_gather_grids_gpu.py"), "-k", CHILD_SELECT],
                           cwd=root, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("the child at %d CUs passed its %d s limit:\n%s" % (cus, CHILD_TIMEOUT, out[-3000:]))
    print("child at %d CUs: %.1f s" % (cus, time.monotonic() - t0))
    failed = [ln for ln in r.stdout.splitlines() if ln.startswith(("FAILED", "ERROR"))]
    tail = "\n".join(["exit %d" % r.returncode] + failed[:250] + [r.stdout[-3000:], r.stderr[-2000:]])
    assert r.returncode == 0, tail
    assert "%d passed" % N_CHILD in r.stdout, r.stdout[-2000:]
