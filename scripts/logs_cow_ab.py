#!/usr/bin/env python3
"""Interleaved in-process A/B of the write-log QUEUE for a pool with open
snapshots (cc_apply_logs_cow_dev) against one cc_apply_log_cow_dev call per
batch, on ONE loaded library, in the bench's partial-write shape: a queue of 10
batches of 65,536 random 512 B-4 KiB writes, 4 KiB pages, a 16 GiB pool of
16 MiB chunks, every chunk slotted.  Variants, each event-timed on its own:
  P      ten cc_apply_log_cow_dev calls (with --clone: each followed by cc_clone_mark_dev)
  Q      one cc_apply_logs_cow_dev call
  plain  one cc_apply_logs_dev call: the rate of a pool with no snapshot (reference line)
States of the snapshot bitmaps, set before every call outside the timed span:
  set    all bits set: nothing is copied (what Q adds over `plain` is the pass alone)
  clear  all bits clear: every touched page is copied
  skew   all set but the pages of batch 0's first 4,096 entries: every copy falls
         to the first waves of the pass
--clone makes every chunk a clone chunk as well (not a state of the reference:
the cost of the marks alone).  The run is cut into rounds; per (state, variant)
it prints the median ms a batch of every round and overall, then per state Q
against P and the range of P's round medians.  Under rocprofv3 --kernel-trace
--stats (a run of its own, --rounds 1 --only set) the pass's own time is
logs_prepass_kernel's row.
usage: logs_cow_ab.py [--delta] [--verify] [--clone] [--rounds R] [--reps CALLS_PER_ROUND] [--only STATE] [--n WRITES]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curve_amd import crc as C  # noqa: E402


def opt(name, default):
    if name in sys.argv:
        return type(default)(sys.argv[sys.argv.index(name) + 1])
    return default


delta, verify, with_clone = "--delta" in sys.argv, "--verify" in sys.argv, "--clone" in sys.argv
U, rounds, reps, only = opt("--n", 65536), opt("--rounds", 5), opt("--reps", 7), opt("--only", "")
B, SKEW = 10, 4096
dev = torch.device("cuda", 0)
pb, cb = 4096, 16 << 20
pool = torch.empty(opt("--pool-gib", 16) << 30, dtype=torch.uint8, device=dev).random_(0, 256)
crcs = C.page_crc(pool, pb)
src = torch.empty(U * pb, dtype=torch.uint8, device=dev).random_(0, 256)
rng = np.random.default_rng(7)
recs = [C.log_records(rng.integers(0, pool.numel() - pb, U), rng.integers(0, U * pb - pb, U),
                      rng.integers(512, 4097, U)) for _ in range(B)]
logs = [torch.from_numpy(r.view(np.uint8)).to(dev) for r in recs]
queue = [(src, log, U) for log in logs]
n_chunks, ppc = pool.numel() // cb, cb // pb
cow = C.Cow(n_chunks, cb, pb, n_slots=n_chunks, device=dev, verify=verify)
cow.snap_slot.copy_(torch.arange(n_chunks, dtype=torch.int32, device=dev))
clone = None
if with_clone:
    clone = C.Clone(n_chunks, cb, pb, n_slots=n_chunks, device=dev)
    clone.clone_slot.copy_(torch.arange(n_chunks, dtype=torch.int32, device=dev))
# skew: every bit set but those of the pages the first SKEW entries of batch 0 touch
first = recs[0][:SKEW]
p0 = first["dst"] // pb
p1 = (first["dst"] + first["len"] - 1) // pb
pages = np.unique(np.concatenate([p0, p1])).astype(np.int64)
skew_bits = np.full(n_chunks * ((ppc + 31) // 32), 0xFFFFFFFF, np.uint32)
np.bitwise_and.at(skew_bits, (pages // ppc) * ((ppc + 31) // 32) + (pages % ppc) // 32,
                  ~(np.uint32(1) << (pages % ppc % 32).astype(np.uint32)))
skew_bits = torch.from_numpy(skew_bits.view(np.int32)).to(dev).view_as(cow.bitmap)
s = torch.cuda.current_stream()


def call(variant):
    if variant == "P":
        for _, log, n in queue:
            C.apply_log_cow(pool, crcs, src, log, n, pb, cow, pb, delta=delta)
            if clone is not None:
                C.clone_mark(pool, log, n, pb, clone, pb)
    elif variant == "Q":
        C.apply_logs(pool, crcs, queue, pb, pb, delta=delta, cow=cow, clone=clone)
    else:
        C.apply_logs(pool, crcs, queue, pb, pb, delta=delta)


def timed(state, variant):
    if state == "skew":
        cow.bitmap.copy_(skew_bits)
    else:
        cow.bitmap.fill_(0 if state == "clear" else -1)
    if clone is not None:
        clone.bitmap.fill_(0)
    before = int(cow.copied.item())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    call(variant)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / B, int(cow.copied.item()) - before


states = [only] if only else ["set", "clear", "skew"]
variants = ["P", "Q", "plain"]
for _ in range(6):  # warm-up: clocks, the stream's tables, the work buffers, every kernel once
    for st in states:
        for v in variants:
            timed(st, v)
ms = {(st, v): [[] for _ in range(rounds)] for st in states for v in variants}
copied = {}
for r in range(rounds):
    for i in range(reps):
        for st in states:
            for v in (variants if (r + i) % 2 == 0 else variants[::-1]):
                if v == "plain" and st != states[0]:
                    continue  # no bitmap is read: one state is enough
                t, n = timed(st, v)
                ms[(st, v)][r].append(t)
                if v != "plain":
                    assert copied.setdefault(st, n) == n, (st, v, n)  # P and Q copy the same pages, every time
ok = bool(torch.equal(crcs, C.page_crc(pool, pb))) if not delta else None
mode = ("delta" if delta else "full") + (" verify" if verify else "") + (" clone" if with_clone else "")


def med(v):
    return sorted(v)[len(v) // 2]


for st in states:
    row = {}
    for v in variants:
        per = [med(x) for x in ms[(st, v)] if x]
        if not per:
            continue
        row[v] = (med([t for x in ms[(st, v)] for t in x]), per)
        print(f"{mode} n={U} x{B} {st} {v}: median {row[v][0]:.4f} ms a batch; rounds "
              + " ".join(f"{t:.4f}" for t in per), flush=True)
    p, q = row["P"], row["Q"]
    spread = max(p[1]) - min(p[1])
    print(f"{mode} {st}: {copied[st]} pages copied a queue; Q - P = {q[0] - p[0]:+.4f} ms a batch "
          f"({100 * (q[0] - p[0]) / p[0]:+.2f} %), range of P's round medians {spread:.4f} ms: "
          f"{'within' if q[0] <= p[0] + spread else 'ABOVE'} the bar")
if ok is not None:
    print(f"crcs_consistent {ok}")
    assert ok
