#!/usr/bin/env python3
"""Interleaved in-process A/B of the scrub (cc_scrub_dev) against the calls it
is held to, on ONE loaded library and one pool of 1024 x 16 MiB chunks of
4 KiB pages (the headline configuration).  Each call is event-timed on its
own, after a clock warm-up, the kinds alternating:
  verify_list  cc_page_verify_list_dev over the pool (the page kernel)
  plain    (A) cc_scrub_dev with neither struct: by contract the same launch plus two one-thread kernels
  reads        cc_verify_reads_dev over one read a chunk covering the pool (the schedule family's yardstick)
  dense    (B) cc_scrub_dev with both structs, no chunk a clone, no slot mapped: the dense pool through scrub_kernel
  mix      (C) 1/8 of the chunks clones with 30 % of their bits set, 64 snapshot slots with 10 % of theirs
Printed (and written to --out): median, p10 and p90 ms of each, the bytes
hashed ((live_checked + snap_checked) x 4100) as a rate, and the ratios the
DESIGN quotes.  The pool is clean: no call may count a mismatch, and the counts
must be what the bitmaps say.
--profile: a few calls of verify_list, dense and mix only, untimed, for a
counter run (rocprofv3 --pmc FETCH_SIZE, collected on its own).
usage: scrub_ab.py [--chunks N] [--reps SECONDS_WORTH] [--out FILE] [--profile]"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curve_amd import crc as C  # noqa: E402
from curve_amd import _lib      # noqa: E402


def opt(name, default):
    if name in sys.argv:
        return type(default)(sys.argv[sys.argv.index(name) + 1])
    return default


n_chunks, budget_s, out_path = opt("--chunks", 1024), opt("--reps", 2.0), opt("--out", "")
profile = "--profile" in sys.argv
dev = torch.device("cuda", 0)
pb, cb = 4096, 16 << 20
ppc = cb // pb
wps = ppc // 32
pool = torch.empty(n_chunks * cb, dtype=torch.uint8, device=dev).random_(0, 256)
crcs = C.page_crc(pool, pb)
n_pages = pool.numel() // pb
rng = np.random.default_rng(0x5C2B)


def bits(n_slots, density):
    b = rng.random((n_slots, ppc)) < density
    return np.packbits(b, axis=1, bitorder="little").view(np.uint32).reshape(n_slots, wps), b


# (B) both structs, nothing behind them: every chunk ordinary, no snapshot open
cow_none = C.Cow(n_chunks, cb, pb, n_slots=1, device=dev)
clone_none = C.Clone(n_chunks, cb, pb, n_slots=1, device=dev)
# (C) every 8th chunk a clone with 30 % of its bits set; 64 snapshot slots on ordinary chunks with 10 % of theirs
n_clone, n_snap = n_chunks // 8, min(64, n_chunks // 2)
clone_mix = C.Clone(n_chunks, cb, pb, n_slots=n_clone, device=dev)
slot = np.full(n_chunks, 0xFFFFFFFF, np.uint32)
slot[::8] = np.arange(n_clone, dtype=np.uint32)
clone_mix.clone_slot.copy_(torch.from_numpy(slot.view(np.int32)).to(dev))
cbm, cset = bits(n_clone, 0.30)
clone_mix.bitmap.copy_(torch.from_numpy(cbm.view(np.int32)).to(dev))
cow_mix = C.Cow(n_chunks, cb, pb, n_slots=n_snap, device=dev)
sslot = np.full(n_chunks, 0xFFFFFFFF, np.uint32)
owners = (np.arange(n_snap) * (n_chunks // n_snap) + 3) % n_chunks       # chunks 3, 19, ...: never a clone chunk
sslot[owners] = np.arange(n_snap, dtype=np.uint32)
cow_mix.snap_slot.copy_(torch.from_numpy(sslot.view(np.int32)).to(dev))
sbm, sset = bits(n_snap, 0.10)
cow_mix.bitmap.copy_(torch.from_numpy(sbm.view(np.int32)).to(dev))
# a slot's page is its chunk's live page, so its CRC is the table's: the snapshot half is clean wherever a bit is set
cow_mix.snap.view(n_snap, cb).copy_(pool.view(n_chunks, cb)[torch.from_numpy(owners).to(dev)])
cow_mix.snap_crcs.copy_(crcs.view(n_chunks, ppc)[torch.from_numpy(owners).to(dev)])
want = {"plain": (n_pages, 0, 0), "dense": (n_pages, 0, 0),
        "mix": (n_pages - int((~cset).sum()), int(sset.sum()), int((~cset).sum()))}  # live_checked, snap_checked, unwritten

counts = {k: torch.zeros(6, dtype=torch.int64, device=dev) for k in want}
calls = {k: 0 for k in want}
lst = torch.zeros(4096, dtype=torch.int64, device=dev)
per = torch.zeros((n_chunks, 2), dtype=torch.int32, device=dev)
vl = torch.tensor([0, -1], dtype=torch.int64, device=dev)
d_reads = torch.from_numpy(np.stack([np.arange(n_chunks, dtype=np.int64) * cb, np.full(n_chunks, cb, np.int64)],
                                    axis=1).reshape(-1)).to(dev)
rbad = torch.zeros(n_chunks, dtype=torch.int32, device=dev)
rtotal = torch.zeros(1, dtype=torch.int64, device=dev)
s = torch.cuda.current_stream()
L = _lib.lib()
vp = ctypes.c_void_p


def call(kind):
    if kind == "verify_list":
        C.check(L.cc_page_verify_list_dev(vp(pool.data_ptr()), n_pages, pb, vp(crcs.data_ptr()), vp(vl.data_ptr()),
                                          vp(vl.data_ptr() + 8), vp(lst.data_ptr()), lst.numel(), vp(s.cuda_stream)),
                "cc_page_verify_list_dev")
    elif kind == "reads":
        C.verify_read_records(pool, crcs, d_reads, n_chunks, rbad, rtotal, page_bytes=pb)
    else:
        cow, clone = {"plain": (None, None), "dense": (cow_none, clone_none), "mix": (cow_mix, clone_mix)}[kind]
        C.scrub_records(pool, crcs, cb, counts[kind], lst, per, cow=cow, clone=clone, page_bytes=pb)
        calls[kind] += 1


def timed(kind):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    call(kind)
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def checked():
    assert int(vl[0].item()) == 0 and int(rtotal.item()) == 0 and not bool(per.any()), "clean pool flagged"
    for k, (live, snap, unw) in want.items():
        got = [int(v) for v in counts[k].cpu().tolist()]
        assert got == [calls[k] * live, 0, calls[k] * snap, 0, calls[k] * unw, 0], (k, got, calls[k], want[k])


if profile:
    for kind in ("verify_list", "dense", "mix", "verify_list", "dense", "mix"):
        call(kind)
        torch.cuda.synchronize()
    checked()
    print(f"scrub_ab --profile: 2 calls each of verify_list, dense, mix; mix hashes {(want['mix'][0] + want['mix'][1])} "
          f"pages of {n_pages} live + {n_pages} snapshot indices = {(want['mix'][0] + want['mix'][1]) * pb} page bytes; "
          f"the pool is {n_pages * pb} bytes", flush=True)
    del pool, crcs, cow_mix, clone_mix
    C.engine_fini()  # release the device contexts while the profiler is still up, not from a destructor at exit
    sys.exit(0)

kinds = ["verify_list", "plain", "reads", "dense", "mix"]
t0 = time.perf_counter()
while time.perf_counter() - t0 < 1.0:  # clock warm-up: every kernel, about a second of load
    for kind in kinds:
        call(kind)
    torch.cuda.synchronize()
ms = {kind: [] for kind in kinds}
spent, r = 0.0, 0
while spent < budget_s * 1e3 or r < 20:
    for kind in (kinds if r % 2 == 0 else kinds[::-1]):
        t = timed(kind)
        ms[kind].append(t)
        spent += t
    r += 1
checked()


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


med = {kind: pct(v, 0.5) for kind, v in ms.items()}
hashed = {"verify_list": n_pages, "plain": n_pages, "reads": n_pages, "dense": n_pages,
          "mix": want["mix"][0] + want["mix"][1]}
rate = {k: hashed[k] * (pb + 4) / (med[k] * 1e-3) for k in kinds}
lines = [f"scrub_ab: {n_chunks} x 16 MiB pool, 4 KiB pages ({n_pages} pages), {len(ms['mix'])} interleaved calls each, "
         f"{torch.cuda.get_device_name(dev)}",
         f"mix: {n_clone} clone chunks with {100 * cset.mean():.1f} % of their bits set, {n_snap} snapshot slots with "
         f"{100 * sset.mean():.1f} %: {want['mix'][0]} live + {want['mix'][1]} snapshot pages hashed, "
         f"{want['mix'][2]} never written"]
for kind in kinds:
    lines.append(f"{kind:11s} median {med[kind]:.4f} ms  p10 {pct(ms[kind], 0.1):.4f}  p90 {pct(ms[kind], 0.9):.4f}  "
                 f"{hashed[kind] * (pb + 4) / 1e9:.3f} GB hashed = {rate[kind] / 1e12:.3f} TB/s")
lines.append(f"(A) plain / verify_list = {med['plain'] / med['verify_list']:.4f}")
lines.append(f"(B) dense / reads = {med['dense'] / med['reads']:.4f}   dense / verify_list = "
             f"{med['dense'] / med['verify_list']:.4f}")
lines.append(f"(C) mix rate / dense rate = {rate['mix'] / rate['dense']:.4f}")
print("\n".join(lines), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
