#!/usr/bin/env python3
"""Interleaved in-process A/B of snapshot reads (cc_read_snap_dev) against
verify on read (cc_verify_reads_dev) on ONE loaded library, on the bench's
verify-on-read workload: 65,536 random reads of 4-128 KiB at page-aligned
offsets over a 1024 x 16 MiB pool of 4 KiB pages.  Five calls alternate, each
event-timed on its own, after a clock warm-up:
  verify   cc_verify_reads_dev (the yardstick)
  live     cc_read_snap_dev, cow = NULL, verify only
  snap     the same with every second chunk slotted, random bitmaps about half set
  copy     `snap` with the bytes delivered to an output buffer
  clear    (diagnostic) `snap`'s slots with every bitmap clear: the per-page resolution alone,
           on `live`'s access pattern
Printed (and written to --out): median / min ms of each, the ratio of its
median to `verify`'s, the pages a call touches and, for `copy`, its algorithmic
bytes (2 x 4096 + 4 a page) and their rate as a share of 8 TB/s.  The pool is
clean: every call must count 0 mismatches.
usage: snap_read_ab.py [--reads N] [--chunks N] [--reps SECONDS_WORTH] [--out FILE]"""
import copy
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curve_amd import crc as C  # noqa: E402


def opt(name, default):
    if name in sys.argv:
        return type(default)(sys.argv[sys.argv.index(name) + 1])
    return default


N, n_chunks, budget_s, out_path = opt("--reads", 65536), opt("--chunks", 1024), opt("--reps", 1.0), opt("--out", "")
dev = torch.device("cuda", 0)
pb, cb = 4096, 16 << 20
ppc = cb // pb
pool = torch.empty(n_chunks * cb, dtype=torch.uint8, device=dev).random_(0, 256)
crcs = C.page_crc(pool, pb)
n_pages = pool.numel() // pb
n_slots = n_chunks // 2
cow = C.Cow(n_chunks, cb, pb, n_slots=n_slots, device=dev)
slot = np.full(n_chunks, -1, np.int32)
slot[::2] = np.arange(n_slots, dtype=np.int32)[:slot[::2].size]
cow.snap_slot.copy_(torch.from_numpy(slot).to(dev))
cow.snap.random_(0, 256)
cow.snap_crcs.copy_(C.page_crc(cow.snap.view(-1), pb).view(n_slots, ppc))
cow_clear = copy.copy(cow)  # the same slots behind bitmaps that hold nothing
cow_clear.bitmap = torch.zeros_like(cow.bitmap)
rng = np.random.default_rng(0xEAD)
bits = rng.integers(0, 1 << 32, tuple(cow.bitmap.shape), dtype=np.uint64).astype(np.uint32)
cow.bitmap.copy_(torch.from_numpy(bits.view(np.int32)).to(dev))
batches = []
for _ in range(6):
    npg = rng.integers(1, 33, N)
    first = rng.integers(0, n_pages - 32, N)
    d_reads = torch.from_numpy(np.stack([first * pb, npg * pb], axis=1).reshape(-1).astype(np.int64)).to(dev)
    d_off = torch.from_numpy((np.cumsum(npg) - npg).astype(np.int64) * pb).to(dev)
    batches.append((d_reads, d_off, int(npg.sum())))
out = torch.empty(max(b[2] for b in batches) * pb, dtype=torch.uint8, device=dev)
bad = torch.zeros(N, dtype=torch.int32, device=dev)
total = torch.zeros(1, dtype=torch.int64, device=dev)
s = torch.cuda.current_stream()


def call(kind, k):
    d_reads, d_off, _ = batches[k % len(batches)]
    if kind == "verify":
        C.verify_read_records(pool, crcs, d_reads, N, bad, total, pb)
    elif kind == "live":
        C.read_snap_records(pool, crcs, d_reads, N, None, bad, total, page_bytes=pb)
    elif kind == "snap":
        C.read_snap_records(pool, crcs, d_reads, N, cow, bad, total, page_bytes=pb)
    elif kind == "clear":
        C.read_snap_records(pool, crcs, d_reads, N, cow_clear, bad, total, page_bytes=pb)
    else:
        C.read_snap_records(pool, crcs, d_reads, N, cow, bad, total, out=out, out_off=d_off, page_bytes=pb)


def timed(kind, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    call(kind, k)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = ["verify", "live", "snap", "copy", "clear"]
k = 0
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:  # clock warm-up: every kernel, about a second of load
    for kind in kinds:
        call(kind, k)
        k += 1
    torch.cuda.synchronize()
ms = {kind: [] for kind in kinds}
spent, r = 0.0, 0
while spent < budget_s * 1e3 or r < 5:
    for kind in (kinds if r % 2 == 0 else kinds[::-1]):
        t = timed(kind, k)
        k += 1
        ms[kind].append(t)
        spent += t
    r += 1
assert int(total.item()) == 0 and not bool(bad.any()), "clean pool flagged"
med = {kind: sorted(v)[len(v) // 2] for kind, v in ms.items()}
pages = sum(b[2] for b in batches) / len(batches)
lines = [f"snap_read_ab: {N} reads of 4-128 KiB, {n_chunks} x 16 MiB pool, 4 KiB pages, {pages:.0f} pages a call, "
         f"{len(ms['verify'])} interleaved calls each, {torch.cuda.get_device_name(dev)}"]
for kind in kinds:
    lines.append(f"{kind:7s} median {med[kind]:.4f} ms  min {min(ms[kind]):.4f} ms  x{med[kind] / med['verify']:.3f} "
                 f"of verify  {pages * (pb + 4) / (med[kind] * 1e-3) / 1e12:.2f} TB/s read")
nbytes = pages * (2 * pb + 4)
rate = nbytes / (med["copy"] * 1e-3) / 1e12
lines.append(f"copy: {nbytes / 1e9:.2f} GB algorithmic (2 x {pb} + 4 a page) = {rate:.2f} TB/s = "
             f"{100 * rate / 8:.1f} % of 8 TB/s")
print("\n".join(lines), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
