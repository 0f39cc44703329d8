"""cc_read_merge_dev on the GPU: reads of a pool with clone chunks, the written
pages verified and gathered from the pool, the never-written ones gathered from
the reads' origin buffers -- checked bit for bit against the numpy model of
test_read_merge.py (itself checked against a request-by-request restatement of
CloneCore::ReadThenMerge), the oracle's CRCs and the existing device calls.

The rig is test_clone_gpu's: 8 chunks of 40 pages (two bitmap words a slot, the
second partial; 40 is no power of two), clone slots {0, none, 2, none, 1, out of
range, none, 3}, n_slots = 4, about 30 % of the bits set; its 512-page source
buffer is the origin.  Every output starts as OUT_SENT and is compared in full,
gaps included.
"""
import threading

import numpy as np
import pytest

from test_clone import NOT_CLONE, U32_MAX, bit, check_reads_model
from test_clone_gpu import N_PAGES, N_SLOTS, PPC, SRC_PAGES, Rig, i32, to_dev, u32
from test_read_merge import (GPU_SEEDS, NO_ORIGIN, OUT_SENT, gpu_batch, gpu_reads, page_classes, read_merge_model,
                             replay_handle_read_requests)
from test_snap_read import packed_offsets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAGE_SIZES = sorted(GPU_SEEDS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from curve_amd import crc as C
    C.engine_init()
    return torch.device("cuda", 0)


def merged(rig, reads, origin_off, origin=True, out_off=None, out_bytes=None, gap=64, src=None):
    """One cc_read_merge_dev call on the rig and the model's answer to it:
    ((out, bad, bad_total, unwritten, unwritten_total), the model's).  The
    output starts as OUT_SENT everywhere; out_off leaves `gap` bytes between the
    reads unless given.  origin=False: d_origin == NULL; src: an origin buffer
    other than the rig's."""
    C, dev, pb = rig.C, rig.dev, rig.pb
    src = rig.src if src is None else src
    n = len(reads)
    if out_off is None:
        out_off, out_bytes = packed_offsets([ln for _, ln in reads], gap=gap)
        out_bytes += gap
    with C._on_stream(rig.stream):
        d_reads = to_dev(np.array(reads, np.uint64).reshape(-1).view(np.int64), dev)
        bad = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        unw = torch.zeros(n, dtype=torch.int32, device=dev)
        unw_total = torch.zeros(1, dtype=torch.int64, device=dev)
        out = torch.full((out_bytes,), OUT_SENT, dtype=torch.uint8, device=dev)
        d_off = to_dev(np.asarray(out_off, np.uint64).view(np.int64), dev)
        d_ooff = to_dev(np.asarray(origin_off, np.uint64).view(np.int64), dev) if origin else None
        d_src = rig.d_src if src is rig.src else to_dev(src, dev)
    C.read_merge_records(rig.d_pool, rig.crcs, d_reads, n, rig.clone, out, d_off, bad, total, unw, unw_total,
                         origin=d_src if origin else None, origin_off=d_ooff, page_bytes=pb, stream=rig.stream)
    rig.sync()
    got = (out.cpu().numpy(), u32(bad), int(total.item()), u32(unw), int(unw_total.item()))
    m_out = np.full(out_bytes, OUT_SENT, np.uint8)
    m_bad, m_bt, m_unw, m_ut = read_merge_model(rig.host, rig.stored, rig.slots, N_SLOTS, rig.bm, reads,
                                                src if origin else None, origin_off, out_off, m_out, pb, rig.cb,
                                                crc_fn=rig.crc_fn)
    return got, (m_out, m_bad, m_bt, m_unw, m_ut)


def same(got, want):
    (out, bad, bt, unw, ut), (m_out, m_bad, m_bt, m_unw, m_ut) = got, want
    assert (bad == m_bad).all(), np.nonzero(bad != m_bad)[0][:10]
    assert (unw == m_unw).all(), np.nonzero(unw != m_unw)[0][:10]
    assert bt == m_bt and ut == m_ut
    assert (out == m_out).all(), np.nonzero(out != m_out)[0][:10]


def unchanged(rig):
    """The call writes nothing but its outputs: pool, CRC table, bitmaps, claim
    table and paste count are the mirror's (Rig.check less its oracle pass: some
    tests here corrupt pages and CRC words on purpose)."""
    rig.sync()
    assert (rig.d_pool.cpu().numpy() == rig.host).all()
    assert (u32(rig.crcs) == rig.stored).all()
    assert (u32(rig.clone.bitmap) == rig.bm).all()
    assert (u32(rig.clone.claim) == U32_MAX).all()
    assert int(rig.clone.pasted.item()) == rig.total


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n", [1, 64, 65, 3000])
@pytest.mark.parametrize("pb", PAGE_SIZES)
def test_every_page_size_and_both_paths(dev, oracle, pb, n):
    """M = 1 .. 32 x 1 / 64 (the one-launch path) / 65 / 3,000 reads of 1-8
    pages, about a quarter without an origin, the first four crossing chunks
    with different slots: outputs and all four counters equal the model's.  For
    n >= 65 every class of page slot (plain chunk, out-of-range slot, clone page
    with its bit set, unwritten with an origin, unwritten without) has at least
    10 members, asserted on the model's inputs before the device is asked."""
    rig = Rig(dev, oracle, pb, seed=GPU_SEEDS[pb])
    reads, origin_off = gpu_batch(GPU_SEEDS[pb], n, pb)
    counts = page_classes(reads, origin_off, rig.slots, N_SLOTS, rig.bm, pb)
    if n >= 65:
        assert min(counts) >= 10, counts
    got, want = merged(rig, reads, origin_off)
    same(got, want)
    out, bad, bt, unw, ut = got
    assert bt == 0 and not bad.any() and ut == counts[3] + counts[4]
    unchanged(rig)


# --------------------------------------------------------------------------- 2
def pick_pages(rig):
    """A written page of a clone chunk, a page of a plain chunk, two never-written pages."""
    held = [(c, q) for c, s in enumerate(rig.slots) if s < N_SLOTS for q in range(1, PPC - 1) if bit(rig.bm, s, q)]
    clear = [(c, q) for c, s in enumerate(rig.slots) if s < N_SLOTS for q in range(1, PPC - 1)
             if not bit(rig.bm, s, q)]
    assert held and len(clear) >= 2
    (ch, qh), (c1, q1), (c2, q2) = held[len(held) // 2], clear[len(clear) // 3], clear[2 * len(clear) // 3]
    return ch * PPC + qh, 1 * PPC + 5, c1 * PPC + q1, c2 * PPC + q2


@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("pb", [256, 4096])
def test_corruption_is_attributed_to_written_pages_only(dev, oracle, pb, n):
    """One flipped byte in (a) a written page of a clone chunk and (b) a page of
    a plain chunk: every read covering them counts exactly those pages and still
    delivers the bytes.  (c) a flipped byte in a pool page under a clear bit:
    nothing counted, the origin's bytes delivered.  (d) the flipped stored CRC of
    a never-written page: nothing counted."""
    rig = Rig(dev, oracle, pb, seed=21)
    pa, p_b, pc, pd = pick_pages(rig)
    with rig.C._on_stream(rig.stream):
        for p in (pa, p_b, pc):
            rig.d_pool[p * pb + 100] ^= 0x01
            rig.host[p * pb + 100] ^= 0x01
        rig.crcs[pd] ^= 0x10000
        rig.stored[pd] ^= np.uint32(0x10000)
    reads, origin_off = gpu_batch(pb + n, n, pb)
    marks = {"a": pa, "b": p_b, "c": pc, "d": pd}
    first = 8
    for j, (name, p) in enumerate(sorted(marks.items())):
        reads[first + 2 * j] = (p * pb, pb)                      # the page alone
        reads[first + 2 * j + 1] = ((p - 1) * pb, 3 * pb)        # and inside a 3-page read
        origin_off[first + 2 * j] = (7 + j) * pb                 # both with an origin
        origin_off[first + 2 * j + 1] = (20 + 3 * j) * pb
    got, want = merged(rig, reads, origin_off)
    same(got, want)
    out, bad, bt, unw, ut = got
    hits = np.zeros(n, np.uint32)                                # without the model: (a) and (b) only
    for i, (off, ln) in enumerate(reads):
        for name in "ab":
            hits[i] += off <= marks[name] * pb < off + ln
    assert (bad == hits).all() and bt == int(hits.sum()) and bt >= 4
    out_off, _ = packed_offsets([ln for _, ln in reads], gap=64)
    at = {name: int(out_off[first + 2 * j]) for j, name in enumerate(sorted(marks))}
    for name in "ab":                                            # the corrupt written pages, as they are
        p = marks[name]
        assert bad[first + 2 * "ab".index(name)] == 1
        assert (out[at[name]:at[name] + pb] == rig.host[p * pb:(p + 1) * pb]).all()
    for j, name in ((2, "c"), (3, "d")):                         # the origin's bytes, nothing counted
        assert bad[first + 2 * j] == 0 and unw[first + 2 * j] == 1
        assert (out[at[name]:at[name] + pb] == rig.src[(7 + j) * pb:(8 + j) * pb]).all()
    unchanged(rig)


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("n", [24, 200])
def test_invalid_reads_write_nothing(dev, oracle, n):
    """Misaligned off, misaligned len, past the pool, an unaligned or overrunning
    output offset, an unaligned or overrunning origin offset: both words
    UINT32_MAX, not a byte written, the neighbours served.  An origin overrun on
    a read with CC_NO_ORIGIN is no overrun: the origin is never looked at."""
    pb = 512
    rig = Rig(dev, oracle, pb, seed=33)
    reads, origin_off = gpu_batch(n, n, pb)
    pool_bytes, src_bytes = rig.host.size, rig.src.size
    reads[5] = (3 * pb + 256, pb)                   # misaligned off
    reads[6] = (7 * pb, pb + 4)                     # misaligned len
    reads[7] = (pool_bytes - pb, 2 * pb)            # runs past the pool
    reads[9] = (pool_bytes, pb)                     # starts at its end
    reads[10] = (1 << 40, pb)                       # far past it
    reads[11] = (2 * pb, 0)                         # empty
    reads[12] = ((1 << 64) - pb, 2 * pb)            # off + len wraps
    reads[20] = (2 * PPC * pb, PPC * pb)            # chunk 2 whole, no origin: valid whatever the origin's size
    origin_off[20] = NO_ORIGIN
    out_off, out_bytes = packed_offsets([ln for _, ln in reads], gap=64)
    out_bytes += 64
    out_off[13] += 2                                # unaligned output offset
    out_off[14] = out_bytes - reads[14][1] + 4      # 4 bytes over the end
    out_off[15] = 1 << 50                           # far outside
    out_off[n - 1] = out_bytes - reads[n - 1][1]    # ends exactly at the end: valid
    origin_off[16] = 2                              # unaligned origin offset
    origin_off[17] = src_bytes - reads[17][1] + 4   # 4 bytes over the origin's end
    origin_off[18] = 1 << 50                        # far outside
    origin_off[19] = src_bytes - reads[19][1]       # ends exactly at the origin's end: valid
    origin_off[4], origin_off[8], origin_off[n - 1] = 0, 4 * pb, 8 * pb   # neighbours with an origin: every byte arrives
    got, want = merged(rig, reads, origin_off, out_off=out_off, out_bytes=out_bytes)
    same(got, want)
    out, bad, bt, unw, ut = got
    invalid = [5, 6, 7, 9, 10, 12, 13, 14, 15, 16, 17, 18]
    assert (bad[invalid] == U32_MAX).all() and (unw[invalid] == U32_MAX).all()
    assert (np.delete(bad, invalid) == 0).all() and (np.delete(unw, invalid) != U32_MAX).all()
    assert bad[11] == 0 and unw[11] == 0 and unw[20] == sum(1 - bit(rig.bm, 2, q) for q in range(PPC)) > 0
    for i in invalid:  # where each would have landed had it been served (clipped to the buffer)
        if i != 14:    # (14's range is the buffer's end, where the last read rightly lands)
            o = min(int(out_off[i]), out_bytes)
            assert (out[o:min(o + reads[i][1], out_bytes)] == OUT_SENT).all(), i
    for i in (4, 8, 19, n - 1):                     # the neighbours are served
        o = int(out_off[i])
        assert (out[o:o + reads[i][1]] != OUT_SENT).any(), i
    o, ln = int(out_off[n - 1]), reads[n - 1][1]
    assert o + ln == out_bytes
    # every read with CC_NO_ORIGIN against a 4-byte origin buffer: each read is longer than origin_bytes, and none
    # is invalid for it -- the reads whose origin range was at fault above are served now
    none = np.full(n, NO_ORIGIN, np.uint64)
    got, want = merged(rig, reads, none, out_off=out_off, out_bytes=out_bytes, src=rig.src[:4].copy())
    same(got, want)
    out, bad, bt, unw, ut = got
    still = [5, 6, 7, 9, 10, 12, 13, 14, 15]
    assert (bad[still] == U32_MAX).all() and (np.delete(bad, still) == 0).all()
    assert (np.delete(unw, still) != U32_MAX).all() and unw[20] > 0 and ut == int(np.delete(unw, still).sum()) > 0
    assert min(reads[i][1] for i in (16, 17, 18, 20)) > 4
    unchanged(rig)


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n", [40, 500])
@pytest.mark.parametrize("pb", [256, 4096])
def test_agrees_with_the_existing_calls(dev, oracle, pb, n):
    """Every bit set, and every chunk CC_NOT_CLONE: output and bad counts of
    cc_read_snap_dev(cow = NULL) on the same reads, corrupt pages included.  On
    any bitmaps the unwritten counts are cc_clone_check_reads_dev's.  With
    d_origin == NULL the call runs: written pages arrive, the others stay at
    the sentinel."""
    rig = Rig(dev, oracle, pb, seed=44)
    C = rig.C
    for p in (0 * PPC + 3, 1 * PPC + 7, 6 * PPC + 39):
        rig.d_pool[p * pb + 5] ^= 0x80
        rig.host[p * pb + 5] ^= 0x80
    reads, origin_off = gpu_batch(pb + n, n, pb)
    reads[4] = (3 * pb, pb)
    offs, lens = [r[0] for r in reads], [r[1] for r in reads]
    # any bitmaps: the counts of the check call; no origin buffer at all
    got, want = merged(rig, reads, origin_off, origin=False)
    same(got, want)
    out, bad, bt, unw, ut = got
    c_unw, c_total = C.clone_check_reads(rig.d_pool, offs, lens, rig.clone, pb)
    torch.cuda.synchronize()
    assert (u32(c_unw) == unw).all() and int(c_total.item()) == ut and ut > 0
    out_off, _ = packed_offsets(lens, gap=64)
    for i, (off, ln) in enumerate(reads):
        for k in range(ln // pb):
            c, q = divmod(off // pb + k, PPC)
            s = int(rig.slots[c])
            seen = out[int(out_off[i]) + k * pb:int(out_off[i]) + (k + 1) * pb]
            if s < N_SLOTS and not bit(rig.bm, s, q):
                assert (seen == OUT_SENT).all(), (i, k)
            else:
                assert (seen == rig.host[off + k * pb:off + (k + 1) * pb]).all(), (i, k)
    # every bit set, then every chunk no clone: cc_read_snap_dev(cow = NULL)
    s_out, s_bad, s_total = C.read_snap(rig.d_pool, rig.crcs, offs, lens, None, pb)
    torch.cuda.synchronize()
    s_out, s_bad, s_total = s_out.cpu().numpy(), u32(s_bad), int(s_total.item())
    assert s_total >= 1
    bm_rig = rig.bm.copy()
    for case in ("all_set", "no_clone"):
        if case == "all_set":
            rig.bm[:] = 0
            for s in range(N_SLOTS):
                for q in range(PPC):
                    rig.bm[s, q // 32] |= np.uint32(1 << (q % 32))
            rig.clone.bitmap.copy_(to_dev(i32(rig.bm), dev))
        else:
            rig.bm[:] = bm_rig
            rig.clone.bitmap.copy_(to_dev(i32(rig.bm), dev))
            rig.slots[:] = NOT_CLONE
            rig.clone.clone_slot.fill_(-1)
        got, want = merged(rig, reads, origin_off, gap=0)
        same(got, want)
        out, bad, bt, unw, ut = got
        assert ut == 0 and not unw.any(), case
        assert (out == s_out).all() and (bad == s_bad).all() and bt == s_total, case


# --------------------------------------------------------------------------- 5
@pytest.mark.parametrize("pb", [512, 4096])
def test_read_paste_read(dev, oracle, pb):
    """read_merge with origins, paste of the same buffers, then read_merge of
    the same reads with no origin: byte-identical output, nothing unwritten,
    nothing bad."""
    rig = Rig(dev, oracle, pb, seed=5)
    C = rig.C
    rng = np.random.default_rng(pb)
    reads = gpu_reads(rng, 300, pb)
    offs, lens = [r[0] for r in reads], [r[1] for r in reads]
    assert SRC_PAGES >= N_PAGES
    origin_off = np.array(offs, np.uint64)                       # the origin is one image: the source's first N_PAGES
    out1, _, bad1, bt1, unw1, ut1 = C.read_merge(rig.d_pool, rig.crcs, offs, lens, rig.clone, origin=rig.d_src,
                                                 origin_off=origin_off, page_bytes=pb)
    torch.cuda.synchronize()
    assert int(ut1.item()) > 0 and int(bt1.item()) == 0
    entries = [(o, int(g), ln) for (o, ln), g in zip(reads, origin_off)]
    per, want = rig.paste(entries)
    assert per.tolist() == want.tolist()
    rig.check()
    out2, _, bad2, bt2, unw2, ut2 = C.read_merge(rig.d_pool, rig.crcs, offs, lens, rig.clone, page_bytes=pb)
    torch.cuda.synchronize()
    assert int(ut2.item()) == 0 and not u32(unw2).any() and int(bt2.item()) == 0 and not u32(bad2).any()
    out1, out2 = out1.cpu().numpy(), out2.cpu().numpy()
    assert (u32(unw1) > 0).sum() >= 100 and int(per.sum()) > 0
    assert (out1 == out2).all(), np.nonzero(out1 != out2)[0][:10]
    at = 0
    for i, ln in enumerate(lens):
        assert (out2[at:at + ln] == rig.host[offs[i]:offs[i] + ln]).all(), i
        at += ln


@pytest.mark.parametrize("side", [False, True])
@pytest.mark.parametrize("paste", [True, False])
def test_clone_read_end_to_end(dev, oracle, paste, side):
    """crc.clone_read (check -> fetch -> merge -> paste) on a fresh rig against
    the CPU replay of HandleReadRequest -> ReadThenMerge -> Paste, request by
    request; the origin is one image the size of the pool.  side: everything on
    a stream that is NOT the current one, with work queued on it ahead of the
    call, so the host's look at the check's counts has to wait for that stream."""
    pb = 1024
    s = torch.cuda.Stream(device=dev) if side else None
    rig = Rig(dev, oracle, pb, seed=77, stream=s)
    C = rig.C
    rng = np.random.default_rng(78)
    image = rng.integers(0, 256, rig.host.size, dtype=np.uint8)
    with C._on_stream(s):
        d_image = to_dev(image, dev)
        if side:
            # work queued ahead of the call, kept alive to its end
            busy = [torch.empty(1 << 28, dtype=torch.uint8, device=dev).random_(0, 256) for _ in range(4)]  # noqa: F841
    reads = gpu_reads(rng, 150, pb) + [(3 * pb, 6 * pb), (5 * pb, 6 * pb), (3 * pb, 6 * pb)]
    offs, lens = [r[0] for r in reads], [r[1] for r in reads]
    fetched = []

    def fetch(idx):
        fetched.append(np.asarray(idx).tolist())
        at, total = packed_offsets([lens[i] for i in idx])
        with C._on_stream(s):                                    # the download lands on the call's stream
            return torch.cat([d_image[offs[i]:offs[i] + lens[i]] for i in idx]), at

    counts, _ = check_reads_model(reads, rig.host.size, rig.slots, N_SLOTS, rig.bm, pb, rig.cb)
    bits_before = sum(bin(int(w)).count("1") for w in rig.bm.ravel())
    assert s is None or torch.cuda.current_stream(dev).cuda_stream != s.cuda_stream
    out, out_off, bad, bt, unw, ut = C.clone_read(rig.d_pool, rig.crcs, offs, lens, rig.clone, fetch, paste=paste,
                                                  page_bytes=pb, stream=s)
    torch.cuda.synchronize()
    assert fetched == [[i for i, k in enumerate(counts) if k > 0]] and 20 <= len(fetched[0]) < len(reads)
    assert (u32(unw) == counts).all() and int(ut.item()) == int(counts.sum())
    assert int(bt.item()) == 0 and not u32(bad).any()
    responses = replay_handle_read_requests(rig.host, rig.stored, image, rig.slots, N_SLOTS, rig.bm, reads, pb, rig.cb,
                                            rig.crc_fn, paste)
    rig.total += sum(bin(int(w)).count("1") for w in rig.bm.ravel()) - bits_before
    assert (rig.total > 0) == paste
    out, out_off = out.cpu().numpy(), out_off.cpu().numpy()
    at = {}
    for i, data in responses:
        o = int(out_off[i]) + at.get(i, 0)
        assert (out[o:o + data.size] == data).all(), i
        at[i] = at.get(i, 0) + data.size
    assert sum(at.values()) == out.size
    rig.check()
    # nothing left to fetch after the paste: fetch is not called again
    if paste:
        res = C.clone_read(rig.d_pool, rig.crcs, offs, lens, rig.clone, fetch, page_bytes=pb, stream=s)
        torch.cuda.synchronize()
        assert len(fetched) == 1 and (res[0].cpu().numpy() == out).all() and int(res[5].item()) == 0
        rig.check()


# --------------------------------------------------------------------------- 6
@pytest.mark.parametrize("density", [0.0, 0.5, 1.0])
def test_dynamic_tail_and_every_wave(dev, oracle, density):
    """3,000 reads of 5..8 pages on the 256-byte geometry: more page slots than
    8 waves x CUs x 8, so every wave of the grid has a share and the 1/16 tail
    is handed out dynamically; no bit set, half of them, all of them."""
    pb = 256
    rig = Rig(dev, oracle, pb, seed=55, density=density)
    reads, origin_off = gpu_batch(6, 3000, pb, lo=5, hi=8)
    slots = sum(ln // pb for _, ln in reads)
    assert slots > 8 * torch.cuda.get_device_properties(dev).multi_processor_count * 8
    got, want = merged(rig, reads, origin_off)
    same(got, want)
    assert got[2] == 0 and (got[4] == 0) == (density == 1.0)
    unchanged(rig)


# --------------------------------------------------------------------------- 7
def test_streams_and_threads(dev, oracle):
    """A non-default stream, then two threads with a stream, a pool and a Clone
    each: paste -> merged read -> check, three times over."""
    pb = 4096
    s0 = torch.cuda.Stream(device=dev)
    rig = Rig(dev, oracle, pb, seed=61, stream=s0)
    same(*merged(rig, *gpu_batch(61, 300, pb)))
    same(*merged(rig, *gpu_batch(62, 30, pb)))
    errs = []

    def work(i):
        try:
            s = torch.cuda.Stream(device=dev)
            r = Rig(dev, oracle, pb, seed=70 + i, density=0.1, stream=s)
            g = np.random.default_rng(600 + i)
            for n in (20, 65, 200):
                pastes = [(int(g.integers(0, N_PAGES - 4)), int(g.integers(0, SRC_PAGES - 4)), int(g.integers(1, 5)))
                          for _ in range(n)]
                per, want = r.paste(r.entries(pastes))
                assert per.tolist() == want.tolist()
                got, model = merged(r, *gpu_batch(700 + i + n, 40 + n, pb))
                same(got, model)
                assert got[2] == 0
                r.check()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append((i, e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
