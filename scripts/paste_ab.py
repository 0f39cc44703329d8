#!/usr/bin/env python3
"""Interleaved in-process A/B of cc_paste_dev against its yardstick, the copying
cc_read_snap_dev over the same page list (one page read, hashed and stored per
slot: a pasted page's traffic), on ONE loaded library and snap_read_ab.py's
workload: 65,536 random page-aligned ranges of 4-128 KiB over a 1024 x 16 MiB
pool of 4 KiB pages, every chunk a clone chunk.  Three calls alternate, each
event-timed on its own, after a clock warm-up:
  read    cc_read_snap_dev, cow = NULL, the bytes delivered to an output buffer
  paste   cc_paste_dev with every bit clear: every distinct page of the list is pasted
          (the bitmaps are cleared before each call, outside the timed region)
  loser   cc_paste_dev with every bit set: the claim launch plus a paste launch of losers only
The ranges overlap, so `paste` writes fewer pages than `read` delivers (the
pages a later entry loses to an earlier one are not copied); both counts are
printed with the algorithmic bytes of each (read: 2 x 4096 + 4 a slot; paste:
2 x 4096 + 4 a pasted page + 12 a slot for the claim word, twice, and the chunk's
slot).  Printed (and written to --out): median, min, the 10th and 90th
percentile of each and the half-to-half drift of its median (the spread).
Under `rocprofv3 --kernel-trace --stats` (a run of its own, `--reps 0.05 --kinds read,paste`)
the rows of paste_claim_kernel and paste_kernel are the two launches' own times.
usage: paste_ab.py [--reads N] [--chunks N] [--reps SECONDS_WORTH] [--kinds read,paste,loser] [--out FILE]"""
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
clone = C.Clone(n_chunks, cb, pb, n_slots=n_chunks, device=dev)
clone.clone_slot.copy_(torch.arange(n_chunks, dtype=torch.int32, device=dev))
rng = np.random.default_rng(0xEAD)
batches = []
for _ in range(6):
    npg = rng.integers(1, 33, N)
    first = rng.integers(0, n_pages - 32, N)
    off = (np.cumsum(npg) - npg) * pb
    d_reads = torch.from_numpy(np.stack([first * pb, npg * pb], axis=1).reshape(-1).astype(np.int64)).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_pastes = torch.from_numpy(C.log_records(first * pb, off, npg * pb).view(np.uint8)).to(dev)
    covered = np.zeros(n_pages, bool)
    for k in range(1, 33):  # the distinct pages of the list: what a paste into clear bitmaps writes
        covered[first[npg >= k] + k - 1] = True
    batches.append((d_reads, d_off, d_pastes, int(npg.sum()), int(covered.sum())))
buf = torch.empty(max(b[3] for b in batches) * pb, dtype=torch.uint8, device=dev).random_(0, 256)  # read's out, paste's src
bad = torch.zeros(N, dtype=torch.int32, device=dev)
total = torch.zeros(1, dtype=torch.int64, device=dev)
per_entry = torch.zeros(N, dtype=torch.int32, device=dev)
s = torch.cuda.current_stream()
pasted_want = {"paste": 0, "loser": 0}


def prepare(kind):
    if kind == "paste":
        clone.bitmap.zero_()
    elif kind == "loser":
        clone.bitmap.fill_(-1)


def call(kind, k):
    d_reads, d_off, d_pastes, _, distinct = batches[k % len(batches)]
    if kind == "read":
        C.read_snap_records(pool, crcs, d_reads, N, None, bad, total, out=buf, out_off=d_off, page_bytes=pb)
    else:
        C.paste_records(pool, crcs, buf, d_pastes, N, clone, per_entry, page_bytes=pb)
        pasted_want[kind] += distinct if kind == "paste" else 0


def timed(kind, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prepare(kind)
    e0.record(s)
    call(kind, k)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = opt("--kinds", "read,paste,loser").split(",")
assert kinds[0] == "read" and set(kinds) <= {"read", "paste", "loser"}, kinds
k = 0
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:  # clock warm-up: every kernel, about a second of load
    for kind in kinds:
        prepare(kind)
        call(kind, k)
        k += 1
    torch.cuda.synchronize()
ms = {kind: [] for kind in kinds}
spent, r = 0.0, 0
while spent < budget_s * 1e3 or r < 6:
    for kind in (kinds if r % 2 == 0 else kinds[::-1]):
        t = timed(kind, k)
        k += 1
        ms[kind].append(t)
        spent += t
    r += 1
# the pool stays consistent with its CRC table whatever was pasted; the counts are the distinct pages'
assert int(total.item()) == 0 and not bool(bad.any()), "a pasted page does not match its CRC"
assert int(clone.pasted.item()) == pasted_want["paste"], (int(clone.pasted.item()), pasted_want["paste"])
assert bool((clone.claim == -1).all()), "claim table not restored"
crcs_now = C.page_crc(pool, pb)
assert bool((crcs_now == crcs).all()), "CRC table differs from the pool's"


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


med = {kind: pct(v, 0.5) for kind, v in ms.items()}
slots = sum(b[3] for b in batches) / len(batches)
distinct = sum(b[4] for b in batches) / len(batches)
lines = [f"paste_ab: {N} ranges of 4-128 KiB, {n_chunks} x 16 MiB pool (all clone chunks), 4 KiB pages, "
         f"{slots:.0f} page slots a call, {distinct:.0f} distinct pages, {len(ms['read'])} interleaved calls each, "
         f"{torch.cuda.get_device_name(dev)}"]
for kind in kinds:
    v = ms[kind]
    half = len(v) // 2
    drift = abs(pct(v[:half], 0.5) - pct(v[half:], 0.5)) / med[kind]
    lines.append(f"{kind:6s} median {med[kind]:.4f} ms  min {min(v):.4f}  p10 {pct(v, 0.1):.4f}  p90 {pct(v, 0.9):.4f}  "
                 f"half-to-half drift {100 * drift:.2f} %  x{med[kind] / med['read']:.3f} of read")
rd = slots * (2 * pb + 4)
ps = distinct * (2 * pb + 4) + slots * 12
lines.append(f"read : {rd / 1e9:.2f} GB algorithmic (2 x {pb} + 4 a slot) = {rd / (med['read'] * 1e-3) / 1e12:.2f} TB/s")
if "paste" in med:
    lines.append(f"paste: {ps / 1e9:.2f} GB algorithmic (2 x {pb} + 4 a pasted page, 12 a slot) = "
             f"{ps / (med['paste'] * 1e-3) / 1e12:.2f} TB/s; per pasted page {med['paste'] * 1e6 / distinct:.3f} ns "
             f"against read's {med['read'] * 1e6 / slots:.3f} ns per slot")
if "loser" in med:
    lines.append(f"loser: {med['loser'] * 1e6 / slots:.3f} ns per slot (claim launch + a paste launch that copies nothing)")
print("\n".join(lines), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
