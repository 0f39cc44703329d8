#!/usr/bin/env python3
"""Interleaved in-process A/B of the copy-on-write write log (cc_apply_log_cow_dev)
against the plain call on ONE loaded library, in the bench's partial-write
shape: 65,536 random 512 B-4 KiB writes over a 16 GiB pool of 16 MiB chunks.
Three calls alternate, each event-timed on its own:
  plain  cc_apply_log_dev (cc_apply_log_delta_dev with --delta)
  clear  the COW call, every chunk slotted, all bits clear: every touched page is copied
         (the bitmaps are zeroed before the call, outside the timed span)
  set    the COW call, every chunk slotted, all bits set: the scan of the heads only
--verify adds d_stale (the pass rehashes what it copies).  Printed per variant:
median / min ms; for `clear` the pages copied, the pass's bytes (pages x (2 x
page_bytes + 8) + 8 B a head record) and, from the time added over `plain`,
its share of 8 TB/s and of this run's read probe.  Under rocprofv3
--kernel-trace --stats (a run of its own, --reps 1) the kernel's own time is
log_cow_kernel's row.
usage: log_cow_ab.py [--delta] [--verify] [--reps SECONDS_WORTH] [--n WRITES]"""
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


delta, verify = "--delta" in sys.argv, "--verify" in sys.argv
U, budget_s = opt("--n", 65536), opt("--reps", 1.0)
dev = torch.device("cuda", 0)
pb, cb = 4096, 16 << 20
pool = torch.empty(16 << 30, dtype=torch.uint8, device=dev).random_(0, 256)
crcs = C.page_crc(pool, pb)
src = torch.empty(U * pb, dtype=torch.uint8, device=dev).random_(0, 256)
rng = np.random.default_rng(7)
logs = []
for _ in range(8):
    rec = C.log_records(rng.integers(0, pool.numel() - pb, U), rng.integers(0, U * pb - pb, U),
                        rng.integers(512, 4097, U))
    logs.append(torch.from_numpy(rec.view(np.uint8)).to(dev))
n_chunks = pool.numel() // cb
cow = C.Cow(n_chunks, cb, pb, n_slots=n_chunks, device=dev, verify=verify)
cow.snap_slot.copy_(torch.arange(n_chunks, dtype=torch.int32, device=dev))
s = torch.cuda.current_stream()


def call(kind, k):
    log = logs[k % len(logs)]
    if kind == "plain":
        C.apply_log(pool, crcs, src, log, U, pb, pb, delta=delta)
    else:
        C.apply_log_cow(pool, crcs, src, log, U, pb, cow, pb, delta=delta)


def timed(kind, k):
    if kind != "plain":
        cow.bitmap.fill_(0 if kind == "clear" else -1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    call(kind, k)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = ["plain", "clear", "set"]
k = 0
for _ in range(10):  # warm-up: the stream's table, the work buffer, every kernel once
    for kind in kinds:
        timed(kind, k)
        k += 1
# read probe of this run (the HBM read rate the pass's share is taken of)
sink = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
C.hbm_read_probe(pool, sink)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(s)
C.hbm_read_probe(pool, sink)
e1.record(s)
torch.cuda.synchronize()
probe_tbs = pool.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e12

ms = {kind: [] for kind in kinds}
copied = []
spent, r = 0.0, 0
while spent < budget_s * 1e3 or r < 3:
    for kind in (kinds if r % 2 == 0 else kinds[::-1]):
        before = int(cow.copied.item()) if kind == "clear" else 0
        t = timed(kind, k)
        k += 1
        ms[kind].append(t)
        spent += t
        if kind == "clear":
            copied.append(int(cow.copied.item()) - before)
    r += 1
ok = bool(torch.equal(crcs, C.page_crc(pool, pb))) if not delta else None
med = {kind: sorted(v)[len(v) // 2] for kind, v in ms.items()}
mode = ("delta" if delta else "full") + (" verify" if verify else "")
for kind in kinds:
    print(f"{mode} n={U} {kind}: median {med[kind]:.4f} ms min {min(ms[kind]):.4f} ms over {len(ms[kind])} calls",
          flush=True)
pages = sorted(copied)[len(copied) // 2]
nbytes = pages * (2 * pb + 8) + pages * 8
added = med["clear"] - med["plain"]
rate = nbytes / (added * 1e-3) / 1e12 if added > 0 else float("nan")
print(f"{mode} clear: {pages} pages copied a call, {nbytes / 1e6:.1f} MB by the pass, +{added:.4f} ms over plain "
      f"= {rate:.2f} TB/s = {100 * rate / 8:.1f} % of 8 TB/s, {100 * rate / probe_tbs:.1f} % of the read probe "
      f"({probe_tbs:.2f} TB/s)")
print(f"{mode} set: +{med['set'] - med['plain']:.4f} ms over plain (the scan of the heads)")
if ok is not None:
    print(f"crcs_consistent {ok}")
    assert ok
