#!/usr/bin/env python3
"""Interleaved in-process A/B of the write-log queue WITH paste batches in it
(cc_apply_ops_dev) against what a caller had to do before it: cut the queue at
every paste batch.  ONE loaded library, the bench's partial-write shape: 10
write batches of 65,536 random 512 B-4 KiB writes, 4 KiB pages, a 16 GiB pool
of 16 MiB chunks, every chunk a clone chunk, paste batches between the write
batches.  Variants, each event-timed on its own:
  P   the queue cut at every paste batch: cc_apply_logs_cow_dev(clone) for each
      run of write batches, cc_paste_dev for each paste batch
  Q   one cc_apply_ops_dev call (the C call on a prebuilt descriptor array, as a
      chunkserver would hold it; per-entry counts in preallocated words, as P's)
States, set before every call outside the timed span:
  i    9 paste batches of 64 entries of 4-128 KiB, one after each of the first nine
       write batches, every bit clear: the clone-read case
  ii   2 paste batches of 65,536 entries of 4-128 KiB (paste_ab.py's list), after
       write batches 3 and 6, every bit clear
  iii  i with every bit set: every paste loses
The writes have any alignment, so some (write, page) pairs are contested and
Q's bytes differ from P's there (the header says how); the work is the same,
and both variants must paste the same number of pages.  The run is cut into
rounds; per (state, variant) it prints the median ms a queue of every round and
overall, then per state Q against P and the range of P's round medians.  Under
rocprofv3 --kernel-trace --stats (a run of its own, --rounds 1 --reps 3) the
passes' own times are the rows of ops_bid_kernel, ops_resolve_kernel and
ops_paste_kernel.
usage: apply_ops_ab.py [--delta] [--rounds R] [--reps CALLS_PER_ROUND] [--only STATE] [--n WRITES] [--pool-gib G]"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curve_amd import _lib  # noqa: E402
from curve_amd import crc as C  # noqa: E402


def opt(name, default):
    if name in sys.argv:
        return type(default)(sys.argv[sys.argv.index(name) + 1])
    return default


delta = "--delta" in sys.argv
U, rounds, reps, only = opt("--n", 65536), opt("--rounds", 5), opt("--reps", 15), opt("--only", "")
B, SMALL, MPL = 10, 64, 128 << 10
dev = torch.device("cuda", 0)
pb, cb = 4096, 16 << 20
pool = torch.empty(opt("--pool-gib", 16) << 30, dtype=torch.uint8, device=dev).random_(0, 256)
crcs = C.page_crc(pool, pb)
n_pages = pool.numel() // pb
src = torch.empty(U * pb, dtype=torch.uint8, device=dev).random_(0, 256)
rng = np.random.default_rng(7)
logs = [torch.from_numpy(C.log_records(rng.integers(0, pool.numel() - pb, U), rng.integers(0, U * pb - pb, U),
                                       rng.integers(512, 4097, U)).view(np.uint8)).to(dev) for _ in range(B)]
n_chunks = pool.numel() // cb
clone = C.Clone(n_chunks, cb, pb, n_slots=n_chunks, device=dev)
clone.clone_slot.copy_(torch.arange(n_chunks, dtype=torch.int32, device=dev))
contested = torch.zeros(1, dtype=torch.int64, device=dev)


def paste_batch(n):
    """n page-aligned ranges of 4-128 KiB, their origin bytes back to back (paste_ab.py's list)."""
    npg = rng.integers(1, 33, n)
    first = rng.integers(0, n_pages - 32, n)
    off = (np.cumsum(npg) - npg) * pb
    rec = torch.from_numpy(C.log_records(first * pb, off, npg * pb).view(np.uint8)).to(dev)
    return rec, n, int(npg.sum()) * pb, torch.zeros(n, dtype=torch.int32, device=dev)


small = [paste_batch(SMALL) for _ in range(B - 1)]
large = [paste_batch(U) for _ in range(2)]
origin = torch.empty(max(p[2] for p in small + large), dtype=torch.uint8, device=dev).random_(0, 256)
# a queue: ("write", k) | ("paste", batch)
QUEUES = {"i": [], "ii": []}
for k in range(B):
    QUEUES["i"].append(("write", k))
    QUEUES["ii"].append(("write", k))
    if k < B - 1:
        QUEUES["i"].append(("paste", small[k]))
    if k in (2, 5):
        QUEUES["ii"].append(("paste", large[k // 3]))
QUEUES["iii"] = QUEUES["i"]
L = _lib.lib()
work = torch.empty(int(L.cc_apply_logs_work_bytes(U, pb, pb)), dtype=torch.uint8, device=dev)
cs = clone.struct()


def descriptors(queue):
    arr = (_lib.CcOpBatch * len(queue))()
    for i, (kind, x) in enumerate(queue):
        if kind == "write":
            arr[i].kind, arr[i].d_src, arr[i].d_recs, arr[i].n = _lib.CC_OP_WRITE, src.data_ptr(), logs[x].data_ptr(), U
        else:
            rec, n, nbytes, per = x
            arr[i].kind, arr[i].d_src, arr[i].src_bytes, arr[i].d_recs, arr[i].n = \
                _lib.CC_OP_PASTE, origin.data_ptr(), origin.numel(), rec.data_ptr(), n
            arr[i].d_pasted_per_entry = per.data_ptr()
    return arr


ARR = {st: descriptors(q) for st, q in QUEUES.items()}
s = torch.cuda.current_stream()


def call(state, variant):
    queue = QUEUES[state]
    if variant == "Q":
        rc = L.cc_apply_ops_dev(pool.data_ptr(), pool.numel(), pb, ctypes.cast(ARR[state], ctypes.c_void_p), len(queue), pb,
                                MPL, crcs.data_ptr(), 1 if delta else 0, work.data_ptr(), work.numel(), None, None,
                                ctypes.byref(cs), contested.data_ptr())
        assert rc == 0, rc
        return
    run = []
    for kind, x in queue + [("paste", None)]:
        if kind == "write":
            run.append((src, logs[x], U))
            continue
        if run:
            C.apply_logs(pool, crcs, run, pb, pb, delta=delta, clone=clone)
            run = []
        if x is not None:
            rec, n, nbytes, per = x
            C.paste_records(pool, crcs, origin, rec, n, clone, per, page_bytes=pb)


def timed(state, variant):
    clone.bitmap.fill_(-1 if state == "iii" else 0)
    before = int(clone.pasted.item())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    call(state, variant)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), int(clone.pasted.item()) - before


states = [only] if only else ["i", "ii", "iii"]
variants = ["P", "Q"]
for _ in range(6):  # warm-up: clocks, the stream's tables, the work buffers, every kernel once
    for st in states:
        for v in variants:
            timed(st, v)
ms = {(st, v): [[] for _ in range(rounds)] for st in states for v in variants}
pasted = {}
for r in range(rounds):
    for i in range(reps):
        for st in states:
            for v in (variants if (r + i) % 2 == 0 else variants[::-1]):
                t, n = timed(st, v)
                ms[(st, v)][r].append(t)
                assert pasted.setdefault(st, n) == n, (st, v, n)  # P and Q paste the same pages, every time
ok = bool(torch.equal(crcs, C.page_crc(pool, pb))) if not delta else None
mode = "delta" if delta else "full"


def med(v):
    return sorted(v)[len(v) // 2]


for st in states:
    row = {}
    for v in variants:
        per = [med(x) for x in ms[(st, v)]]
        row[v] = (med([t for x in ms[(st, v)] for t in x]), per)
        print(f"{mode} n={U} x{B} state {st} {v}: median {row[v][0]:.4f} ms a queue; rounds "
              + " ".join(f"{t:.4f}" for t in per), flush=True)
    p, q = row["P"], row["Q"]
    spread = max(p[1]) - min(p[1])
    print(f"{mode} state {st}: {pasted[st]} pages pasted a queue; Q - P = {q[0] - p[0]:+.4f} ms a queue "
          f"({100 * (q[0] - p[0]) / p[0]:+.2f} %), range of P's round medians {spread:.4f} ms: "
          f"{'within' if q[0] <= p[0] + spread else 'ABOVE'} the bar")
print(f"contested pairs counted by Q over the run: {int(contested.item())}")
if ok is not None:
    print(f"crcs_consistent {ok}")
    assert ok
