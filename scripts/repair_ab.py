#!/usr/bin/env python3
"""Interleaved in-process A/B of cc_repair_dev against its yardstick, cc_paste_dev
into clear bitmaps (one page read and one written per distinct page), on ONE
loaded library and paste_ab.py's pool and entry list: 65,536 random page-aligned
ranges of 4-128 KiB over a 1024 x 16 MiB pool of 4 KiB pages, every chunk a clone
chunk.  Four calls alternate, each event-timed on its own, after a clock warm-up:
  paste   (a) cc_paste_dev with every bit clear: every distinct page of the list is pasted
  bad     (b) cc_repair_dev, every page bad and every candidate good: two pages read,
              two hashed and one written per distinct page
  clean   (c) cc_repair_dev, every page clean: one page read and hashed, none written
  shadow  (d) cc_repair_dev, every pair shadowed: the claim launch and the schedule alone
The state each call needs is made before it, outside the timed region: `bad`
follows an untimed paste of OTHER bytes over the same pages (so every live page
misses the record), `clean` an untimed paste of the candidates' own bytes;
`shadow` runs the list behind an empty entry 0 on a claim table pre-filled with
0, which no pair's index equals (a diagnostic: that table is not left at rest).
The record is d_expect: per batch, the CRC table a paste of the candidates
leaves (paste and repair give a page to the same lowest-indexed entry).
Printed (and written to --out): median, min, p10, p90 and half-to-half drift of
each, each call's algorithmic bytes and TB/s, and (b) against 1.5 x (a).
usage: repair_ab.py [--reads N] [--chunks N] [--reps SECONDS_WORTH] [--kinds paste,bad,clean,shadow] [--out FILE]"""
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
pool = torch.empty(n_chunks * cb, dtype=torch.uint8, device=dev).random_(0, 256)
crcs = C.page_crc(pool, pb)
n_pages = pool.numel() // pb
clone = C.Clone(n_chunks, cb, pb, n_slots=n_chunks, device=dev)
clone.clone_slot.copy_(torch.arange(n_chunks, dtype=torch.int32, device=dev))
claim = C.repair_claim(pool, pb)
claim_floor = torch.zeros(n_pages, dtype=torch.int32, device=dev)
rng = np.random.default_rng(0xEAD)
raw = []
for _ in range(6):
    npg = rng.integers(1, 33, N)
    first = rng.integers(0, n_pages - 32, N)
    off = (np.cumsum(npg) - npg) * pb
    covered = np.zeros(n_pages, bool)
    for k in range(1, 33):  # the distinct pages of the list: what a paste into clear bitmaps writes
        covered[first[npg >= k] + k - 1] = True
    raw.append((first, npg, off, int(npg.sum()), int(covered.sum())))
buf = torch.empty(max(b[3] for b in raw) * pb, dtype=torch.uint8, device=dev).random_(0, 256)  # the candidates
other = torch.empty_like(buf).random_(0, 256)                                                  # what a bad page holds
per_paste = torch.zeros(N, dtype=torch.int32, device=dev)
per_entry = torch.zeros((N + 1, 4), dtype=torch.int32, device=dev)
totals = {kind: torch.zeros(4, dtype=torch.int64, device=dev) for kind in ("bad", "clean", "shadow")}
want = {kind: np.zeros(4, np.int64) for kind in totals}
s = torch.cuda.current_stream()


def paste_from(src, d_reqs):
    clone.bitmap.zero_()
    C.paste_records(pool, crcs, src, d_reqs, N, clone, per_paste, page_bytes=pb)


batches = []
for first, npg, off, slots, distinct in raw:
    d_reqs = torch.from_numpy(C.log_records(first * pb, off, npg * pb).view(np.uint8)).to(dev)
    behind = C.log_records(np.concatenate([[0], first * pb]), np.concatenate([[0], off]), np.concatenate([[0], npg * pb]))
    d_behind = torch.from_numpy(behind.view(np.uint8)).to(dev)
    paste_from(buf, d_reqs)
    batches.append((d_reqs, d_behind, crcs.clone(), slots, distinct))


def prepare(kind, k):
    d_reqs = batches[k % len(batches)][0]
    if kind == "paste":
        clone.bitmap.zero_()
    elif kind == "bad":
        paste_from(other, d_reqs)
    elif kind == "clean":
        paste_from(buf, d_reqs)


def call(kind, k):
    d_reqs, d_behind, expect, slots, distinct = batches[k % len(batches)]
    if kind == "paste":
        C.paste_records(pool, crcs, buf, d_reqs, N, clone, per_paste, page_bytes=pb)
    elif kind == "shadow":
        C.repair_records(pool, crcs, buf, d_behind, N + 1, claim_floor, per_entry, expect=expect, totals=totals[kind],
                         page_bytes=pb)
        want[kind] += [0, 0, 0, slots]
    else:
        C.repair_records(pool, crcs, buf, d_reqs, N, claim, per_entry, expect=expect, totals=totals[kind],
                         page_bytes=pb)
        want[kind] += [distinct, 0, 0, slots - distinct] if kind == "clean" else [0, distinct, 0, slots - distinct]


def timed(kind, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prepare(kind, k)
    e0.record(s)
    call(kind, k)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


kinds = opt("--kinds", "paste,bad,clean,shadow").split(",")
assert kinds[0] == "paste" and set(kinds) <= {"paste", "bad", "clean", "shadow"}, kinds
k = 0
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:  # clock warm-up: every kernel, about a second of load
    for kind in kinds:
        prepare(kind, k)
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
# every call did what its row says, and the pool stays consistent with its CRC table
for kind in totals:
    assert totals[kind].cpu().numpy().tolist() == want[kind].tolist(), (kind, totals[kind], want[kind])
assert bool((claim == -1).all()), "claim table not restored"
assert bool((C.page_crc(pool, pb) == crcs).all()), "CRC table differs from the pool's"


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


med = {kind: pct(v, 0.5) for kind, v in ms.items()}
slots = sum(b[3] for b in batches) / len(batches)
distinct = sum(b[4] for b in batches) / len(batches)
moved = {"paste": distinct * (2 * pb + 4) + slots * 12,   # a page in, a page and its CRC out; claim word twice + slot word
         "bad": distinct * (3 * pb + 8) + slots * 4,      # two pages and the record in, a page and its CRC out; claim word
         "clean": distinct * (pb + 8) + slots * 4,        # the live page and the record in, the CRC word out
         "shadow": slots * 4}
what = {"paste": "(a) cc_paste_dev, every bit clear", "bad": "(b) cc_repair_dev, every page bad, every candidate good",
        "clean": "(c) cc_repair_dev, every page clean", "shadow": "(d) cc_repair_dev, every pair shadowed"}
lines = [f"repair_ab: {N} ranges of 4-128 KiB, {n_chunks} x 16 MiB pool, 4 KiB pages, {slots:.0f} page slots a call, "
         f"{distinct:.0f} distinct pages, {len(ms['paste'])} interleaved calls each, {torch.cuda.get_device_name(dev)}"]
for kind in kinds:
    v = ms[kind]
    half = len(v) // 2
    drift = abs(pct(v[:half], 0.5) - pct(v[half:], 0.5)) / med[kind]
    lines.append(f"{kind:6s} {what[kind]}: median {med[kind]:.4f} ms  min {min(v):.4f}  p10 {pct(v, 0.1):.4f}  "
                 f"p90 {pct(v, 0.9):.4f}  drift {100 * drift:.2f} %  x{med[kind] / med['paste']:.3f} of paste;  "
                 f"{moved[kind] / 1e9:.2f} GB = {moved[kind] / (med[kind] * 1e-3) / 1e12:.2f} TB/s, "
                 f"{med[kind] * 1e6 / slots:.3f} ns a slot")
if "bad" in med:
    lines.append(f"(b) moves {moved['bad'] / moved['paste']:.3f} x (a)'s bytes and takes {med['bad'] / med['paste']:.3f} x "
                 f"its time: {med['bad'] - 1.5 * med['paste']:+.4f} ms against 1.5 x (a)")
print("\n".join(lines), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
