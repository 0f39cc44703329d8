#!/usr/bin/env python3
"""Interleaved in-process A/B of clone reads (cc_read_merge_dev) against
snapshot reads (cc_read_snap_dev) on ONE loaded library, on snap_read_ab.py's
pool and read list: 65,536 random reads of 4-128 KiB at page-aligned offsets
over a 1024 x 16 MiB pool of 4 KiB pages, every read delivered to an output
buffer.  Six calls alternate (five rows and a diagnostic), each event-timed on
its own, after a clock warm-up:
  snap    (a) cc_read_snap_dev, cow = NULL, copy-out (the yardstick)
  set     (b) cc_read_merge_dev, every chunk a clone, every bit set: (a)'s bytes and hashing plus the resolution
  origin  (c) every bit clear, every read with an origin: pure gather, nothing hashed
  half    (d) half the bits set at random, every read with an origin
  count   (e) (c)'s bitmaps with no origin: counting only, no page traffic
  apart   (diagnostic) (c) with read i's origin bytes where another read's output lies, not its own
Printed (and written to --out): median, p10 and p90 ms of each, the ratio of
its median to (a)'s, and the algorithmic bytes a page (read + write) as a rate.
The pool is clean: no call may count a mismatch, and the unwritten totals must
be the pages the bitmaps say.
usage: read_merge_ab.py [--reads N] [--chunks N] [--reps SECONDS_WORTH] [--out FILE]"""
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
clone_set = C.Clone(n_chunks, cb, pb, n_slots=n_chunks, device=dev)   # every chunk a clone
clone_set.clone_slot.copy_(torch.arange(n_chunks, dtype=torch.int32, device=dev))
clone_set.bitmap.fill_(-1)
clone_clear, clone_half = copy.copy(clone_set), copy.copy(clone_set)  # the same slots behind other bitmaps
clone_clear.bitmap = torch.zeros_like(clone_set.bitmap)
rng = np.random.default_rng(0xEAD)
bits = rng.integers(0, 1 << 32, tuple(clone_set.bitmap.shape), dtype=np.uint64).astype(np.uint32)
clone_half.bitmap = torch.from_numpy(bits.view(np.int32)).to(dev)
held = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(n_chunks, ppc).ravel()  # page -> its bit
csum = np.concatenate([[0], np.cumsum(held, dtype=np.int64)])
batches = []
for _ in range(6):
    npg = rng.integers(1, 33, N)
    first = rng.integers(0, n_pages - 32, N)
    d_reads = torch.from_numpy(np.stack([first * pb, npg * pb], axis=1).reshape(-1).astype(np.int64)).to(dev)
    d_off = torch.from_numpy((np.cumsum(npg) - npg).astype(np.int64) * pb).to(dev)
    batches.append((d_reads, d_off, int(npg.sum()), int((csum[first + npg] - csum[first]).sum()),
                    torch.roll(d_off, N // 2)))  # `apart`: read i's origin starts where read i + N / 2's output does
most = max(b[2] for b in batches) * pb
out = torch.empty(most, dtype=torch.uint8, device=dev)
# read i's origin bytes lie where its output does (32 pages of slack: `apart` pairs a long read with a short one's place)
origin = torch.empty(most + 32 * pb, dtype=torch.uint8, device=dev).random_(0, 256)
bad = torch.zeros(N, dtype=torch.int32, device=dev)
total = torch.zeros(1, dtype=torch.int64, device=dev)
unw = torch.zeros(N, dtype=torch.int32, device=dev)
unw_total = {kind: torch.zeros(1, dtype=torch.int64, device=dev) for kind in ("set", "origin", "half", "count", "apart")}
want = {kind: 0 for kind in unw_total}
s = torch.cuda.current_stream()


def call(kind, k):
    d_reads, d_off, pages, pages_held, d_apart = batches[k % len(batches)]
    if kind == "snap":
        C.read_snap_records(pool, crcs, d_reads, N, None, bad, total, out=out, out_off=d_off, page_bytes=pb)
        return
    clone = {"set": clone_set, "origin": clone_clear, "half": clone_half, "count": clone_clear,
             "apart": clone_clear}[kind]
    o_off = {"count": None, "apart": d_apart}.get(kind, d_off)
    C.read_merge_records(pool, crcs, d_reads, N, clone, out, d_off, bad, total, unw, unw_total[kind],
                         origin=origin if o_off is not None else None, origin_off=o_off, page_bytes=pb)
    want[kind] += {"set": 0, "half": pages - pages_held}.get(kind, pages)


def timed(kind, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    call(kind, k)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = ["snap", "set", "origin", "half", "count", "apart"]
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
for kind in unw_total:
    assert int(unw_total[kind].item()) == want[kind], (kind, int(unw_total[kind].item()), want[kind])


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


med = {kind: pct(v, 0.5) for kind, v in ms.items()}
pages = sum(b[2] for b in batches) / len(batches)
share = sum(b[3] for b in batches) / sum(b[2] for b in batches)
# algorithmic bytes a page: the page read and written (none for `count`), plus the stored CRC of a hashed page
per_page = {"snap": 2 * pb + 4, "set": 2 * pb + 4, "origin": 2 * pb, "half": 2 * pb + 4 * share, "count": 0,
            "apart": 2 * pb}
lines = [f"read_merge_ab: {N} reads of 4-128 KiB, {n_chunks} x 16 MiB pool, 4 KiB pages, {pages:.0f} pages a call, "
         f"{len(ms['snap'])} interleaved calls each, {torch.cuda.get_device_name(dev)}",
         f"half: {100 * share:.1f} % of the touched pages have their bit set"]
for kind in kinds:
    nbytes = pages * per_page[kind]
    lines.append(f"{kind:7s} median {med[kind]:.4f} ms  p10 {pct(ms[kind], 0.1):.4f}  p90 {pct(ms[kind], 0.9):.4f}  "
                 f"x{med[kind] / med['snap']:.3f} of snap  {nbytes / 1e9:.2f} GB = "
                 f"{nbytes / (med[kind] * 1e-3) / 1e12:.2f} TB/s")
print("\n".join(lines), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
