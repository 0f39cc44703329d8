"""cc_read_snap_dev on the GPU: reads through the snapshot view, verified
against the CRC table each page came from and gathered into the caller's
buffer -- checked against the numpy model of test_snap_read.py (itself checked
against a per-request restatement of ReadSpecifiedChunk) and, independently of
it, against the bytes the chunks held before the first copy-on-write batch.

The pools are test_log_cow_gpu's Rig: 8 chunks of 40 pages (two bitmap words a
slot, the second partial; 40 is no power of two), slots {0, none, 2, none, 1,
out of range, none, 3}, four bits held before the first batch, and real
cc_apply_log_cow_dev batches fill the slots.
"""
import threading

import numpy as np
import pytest

from test_log_cow import NO_SNAPSHOT, SENT_BYTE
from test_log_cow_gpu import N_SLOTS, PPC, PRESET, SLOTS, Rig, i32, random_log, to_dev, u32
from test_snap_read import U32_MAX, packed_offsets, snap_read_model

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OUT_SENT = 0x3C   # what the output buffers hold before a call (the slots' sentinel is SENT_BYTE)
N_CHUNKS = len(SLOTS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from curve_amd import crc as C
    C.engine_init()
    return torch.device("cuda", 0)


def sync(rig):
    if rig.stream is not None:
        rig.stream.synchronize()
    else:
        torch.cuda.synchronize()


def filled_rig(dev, oracle, pb, seed, batches=(60,), stream=None, delta=False, ppc=PPC):
    """A Rig after real COW batches, checked, with the four preset slot pages
    (which hold the sentinel bytes) given the CRC of those bytes, on the device
    and in the model: a clean rig reads back with no mismatch anywhere."""
    rig = Rig(dev, oracle, pb, ppc=ppc, seed=seed, stream=stream)
    rng = np.random.default_rng(seed * 31 + pb)
    for n in batches:
        rig.batch(*random_log(rng, n, rig.orig.size, pb, pb), pb, delta)
        rig.check()
    sent_crc = oracle.crc32c(bytes([SENT_BYTE]) * pb)
    with rig.C._on_stream(stream):
        for s, q in PRESET:
            rig.scrc[s, q] = sent_crc
            rig.cow.snap_crcs[s, q] = int(np.uint32(sent_crc).view(np.int32))
    return rig


def view(rig, oracle, reads, copy=True, cow=True, out_off=None, out_bytes=None, gap=64):
    """One cc_read_snap_dev call on the rig and the model's answer to it:
    ((out, bad, total), (model out, model bad, model total)); out None with
    copy=False.  The output starts as OUT_SENT everywhere; out_off leaves `gap`
    bytes between the reads unless given."""
    C, dev, pb = rig.C, rig.dev, rig.pb
    n = len(reads)
    if copy and out_off is None:
        out_off, out_bytes = packed_offsets([ln for _, ln in reads], gap=gap)
        out_bytes += gap
    with C._on_stream(rig.stream):
        d_reads = to_dev(np.array(reads, np.uint64).reshape(-1).view(np.int64), dev)
        bad = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        out = torch.full((out_bytes,), OUT_SENT, dtype=torch.uint8, device=dev) if copy else None
        d_off = to_dev(np.asarray(out_off, np.uint64).view(np.int64), dev) if copy else None
    C.read_snap_records(rig.d_pool, rig.crcs, d_reads, n, rig.cow if cow else None, bad, total, out=out,
                        out_off=d_off, page_bytes=pb, stream=rig.stream)
    sync(rig)
    got = (out.cpu().numpy() if copy else None, u32(bad), int(total.item()))
    want = snap_read_model(rig.host, rig.stored, rig.snap, rig.scrc, rig.bm, rig.slots if cow else None, rig.n_slots,
                           reads, out_off if copy else None, out_bytes if copy else None, pb, rig.cb,
                           crc_fn=lambda b: oracle.crc32c(b.tobytes()),
                           out=np.full(out_bytes, OUT_SENT, np.uint8) if copy else None)
    return got, want


def same(got, want):
    (out, bad, total), (m_out, m_bad, m_total) = got, want
    assert (bad == m_bad).all(), np.nonzero(bad != m_bad)[0][:10]
    assert total == m_total
    assert (out is None) == (m_out is None)
    if out is not None:
        assert (out == m_out).all(), np.nonzero(out != m_out)[0][:10]


def random_reads(rng, n, pb, lo=1, hi=8):
    """n page-aligned reads of lo..hi pages anywhere in the pool; the first four
    cross chunk boundaries between chunks with different slots (slot 0 | none,
    none | slot 2, slot 1 | out of range) and end on the pool's last page."""
    n_pages = N_CHUNKS * PPC
    reads = []
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        reads.append((int(rng.integers(0, n_pages - k + 1)) * pb, k * pb))
    fixed = [(PPC - 2, 4), (2 * PPC - 3, 5), (5 * PPC - 1, 2), (n_pages - 3, 3)]
    for i, (p0, k) in enumerate(fixed[:n]):
        reads[i] = (p0 * pb, k * pb)
    return reads


def set_bits(rig):
    """(slot, page in chunk) of the bits the batches set (not the preset ones), and
    (chunk, page in chunk) of the clear bits of slotted chunks."""
    owner = {int(s): c for c, s in enumerate(rig.slots) if s < rig.n_slots}
    held, clear = [], []
    for s, c in sorted(owner.items()):
        for q in range(PPC):
            if (int(rig.bm[s, q // 32]) >> (q % 32)) & 1:
                if (s, q) not in rig.preset:
                    held.append((s, q))
            else:
                clear.append((c, q))
    return owner, held, clear


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("copy", [True, False])
@pytest.mark.parametrize("n", [1, 64, 65, 3000])
@pytest.mark.parametrize("pb", [256, 512, 2048, 4096, 8192])
def test_view_after_cow_batches(dev, oracle, pb, n, copy):
    """Every M family x 1 / 64 (the one-launch path) / 65 / 3,000 reads x copy
    and verify-only, after one to three real COW batches: outputs and counts
    (all 0) equal the model's, gaps and all; and, without the model, every
    slotted chunk read whole shows its bytes from before the first batch (the
    preset pages: the slot's sentinel bytes), every other chunk its live bytes."""
    batches = {1: (60,), 64: (60, 200), 65: (40, 100, 300), 3000: (60,)}[n]
    rig = filled_rig(dev, oracle, pb, seed=n + 3, batches=batches)
    rng = np.random.default_rng(pb * 13 + n)
    got, want = view(rig, oracle, random_reads(rng, n, pb), copy=copy)
    same(got, want)
    assert got[2] == 0 and not got[1].any()
    # independently of the model
    cb = rig.cb
    (out, bad, total), _ = view(rig, oracle, [(c * cb, cb) for c in range(N_CHUNKS)], copy=True, gap=0)
    assert total == 0 and not bad.any()
    live = rig.d_pool.cpu().numpy()
    assert (live != rig.orig).any()
    for c, s in enumerate(SLOTS):
        seen = out[c * cb:(c + 1) * cb].reshape(PPC, pb)
        exp = (rig.orig if s < N_SLOTS else live)[c * cb:(c + 1) * cb].reshape(PPC, pb).copy()
        for ps, q in PRESET:
            if ps == s:
                exp[q] = SENT_BYTE
        assert (seen == exp).all(), c


# --------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("pb", [256, 4096])
def test_corruption_is_attributed_to_the_right_table(dev, oracle, pb, n):
    """One flipped byte in (a) a slot page whose bit is set, (b) a live page
    whose bit is clear in a slotted chunk, (c) a live page of an unslotted chunk,
    (d) a live page under a set bit (shadowed), and (e) a flipped stored CRC in
    d_snap_crcs: (a), (b), (c), (e) are counted once on every read that touches
    them, (d) is not reported; the delivered bytes are the corrupt ones."""
    rig = filled_rig(dev, oracle, pb, seed=21, batches=(60,))
    owner, held, clear = set_bits(rig)
    assert len(held) >= 3 and clear
    (sa, qa), (sd, qd), (se, qe) = held[0], held[len(held) // 2], held[-1]
    cbk, qb = clear[len(clear) // 2]
    pa, pd, pe = owner[sa] * PPC + qa, owner[sd] * PPC + qd, owner[se] * PPC + qe
    p_b, p_c = cbk * PPC + qb, 1 * PPC + 5                       # chunk 1: no snapshot
    with rig.C._on_stream(rig.stream):
        rig.cow.snap[sa, qa * pb + 11] ^= 0x20                   # (a)
        rig.snap[sa, qa * pb + 11] ^= 0x20
        for p in (p_b, p_c, pd):                                 # (b) (c) (d)
            rig.d_pool[p * pb + 100] ^= 0x01
            rig.host[p * pb + 100] ^= 0x01
        rig.cow.snap_crcs[se, qe] ^= 0x10000                     # (e)
        rig.scrc[se, qe] ^= np.uint32(0x10000)
    rng = np.random.default_rng(pb + n)
    reads = random_reads(rng, n, pb)
    marks = {"a": pa, "b": p_b, "c": p_c, "d": pd, "e": pe}
    first = 8
    for j, (name, p) in enumerate(sorted(marks.items())):
        reads[first + 2 * j] = (p * pb, pb)                      # the page alone
        p0 = min(max(p - 1, 0), N_CHUNKS * PPC - 3)
        reads[first + 2 * j + 1] = (p0 * pb, 3 * pb)             # and inside a 3-page read
    got, want = view(rig, oracle, reads, copy=True)
    same(got, want)
    out, bad, total = got
    # without the model: how many of the four reported pages each read touches
    hits = np.zeros(n, np.uint32)
    for i, (off, ln) in enumerate(reads):
        for name in "abce":
            hits[i] += off <= marks[name] * pb < off + ln
    assert (bad == hits).all() and total == int(hits.sum())
    for j, name in enumerate(sorted(marks)):
        assert bad[first + 2 * j] == (0 if name == "d" else 1), name
    out_off, _ = packed_offsets([ln for _, ln in reads], gap=64)
    at = {name: int(out_off[first + 2 * j]) for j, name in enumerate(sorted(marks))}
    assert (out[at["a"]:at["a"] + pb] == rig.snap[sa, qa * pb:(qa + 1) * pb]).all()  # the corrupt slot page
    for name, p in (("b", p_b), ("c", p_c)):
        assert (out[at[name]:at[name] + pb] == rig.host[p * pb:(p + 1) * pb]).all()  # the corrupt live pages
    assert (out[at["d"]:at["d"] + pb] == rig.snap[sd, qd * pb:(qd + 1) * pb]).all()  # the slot page, not the live one
    assert (out[at["d"]:at["d"] + pb] != rig.host[pd * pb:(pd + 1) * pb]).any()


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("copy", [True, False])
@pytest.mark.parametrize("n", [24, 200])
def test_invalid_reads_write_nothing(dev, oracle, n, copy):
    """Misaligned off, misaligned len, past the pool, far past it, an unaligned
    out_off and an output range that leaves the buffer: UINT32_MAX each, not a
    byte written (the sentinel holds); len == 0 leaves its counter alone; the
    valid reads of the batch are served.  Verify-only has no output to break."""
    pb = 512
    rig = filled_rig(dev, oracle, pb, seed=33, batches=(60, 60))
    rng = np.random.default_rng(n)
    reads = random_reads(rng, n, pb)
    pool_bytes = rig.orig.size
    reads[5] = (3 * pb + 256, pb)                   # misaligned off
    reads[6] = (7 * pb, pb + 4)                     # misaligned len
    reads[7] = (pool_bytes - pb, 2 * pb)            # runs past the pool
    reads[9] = (pool_bytes, pb)                     # starts at its end
    reads[10] = (1 << 40, pb)                       # far past it
    reads[11] = (2 * pb, 0)                         # empty
    reads[12] = ((1 << 64) - pb, 2 * pb)            # off + len wraps
    out_off, out_bytes = packed_offsets([ln for _, ln in reads], gap=64)
    out_bytes += 64
    out_off[13] += 2                                # unaligned output offset
    out_off[14] = out_bytes - reads[14][1] + 4      # 4 bytes over the end
    out_off[15] = 1 << 50                           # far outside
    out_off[n - 1] = out_bytes - reads[n - 1][1]    # ends exactly at the end: valid
    got, want = view(rig, oracle, reads, copy=copy, out_off=out_off, out_bytes=out_bytes)
    same(got, want)
    out, bad, total = got
    assert total == 0
    invalid = [5, 6, 7, 9, 10, 12] + ([13, 14, 15] if copy else [])
    assert (bad[invalid] == U32_MAX).all()
    assert bad[11] == 0 and bad[n - 1] == 0
    assert (np.delete(bad, invalid) == 0).all()
    if copy:
        for i in invalid:  # where each would have landed had it been served (clipped to the buffer)
            if i != 14:    # (14's range is the buffer's end, where the last read rightly lands)
                o = min(int(out_off[i]), out_bytes)
                assert (out[o:min(o + reads[i][1], out_bytes)] == OUT_SENT).all(), i
        o, ln = int(out_off[n - 1]), reads[n - 1][1]
        assert o + ln == out_bytes and (out[o:] != OUT_SENT).any()


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n", [40, 500])
@pytest.mark.parametrize("pb", [256, 4096])
def test_cow_null_reads_the_live_pool(dev, oracle, pb, n):
    """cow == NULL: the live bytes whatever the slots hold, and the counts of
    cc_verify_reads_dev on the same reads, corrupt live pages included."""
    rig = filled_rig(dev, oracle, pb, seed=44, batches=(80,))
    owner, held, _ = set_bits(rig)
    s, q = held[0]
    for p in (owner[s] * PPC + q, 1 * PPC + 7, 6 * PPC + 39):  # a shadowed page and two plain ones
        rig.d_pool[p * pb + 5] ^= 0x80
        rig.host[p * pb + 5] ^= 0x80
    rng = np.random.default_rng(pb + n)
    reads = random_reads(rng, n, pb)
    reads[4] = ((owner[s] * PPC + q) * pb, pb)
    got, want = view(rig, oracle, reads, copy=True, cow=False)
    same(got, want)
    out, bad, total = got
    assert total >= 1 and bad[4] == 1
    out_off, _ = packed_offsets([ln for _, ln in reads], gap=64)
    for i, (off, ln) in enumerate(reads):
        o = int(out_off[i])
        assert (out[o:o + ln] == rig.host[off:off + ln]).all(), i
    v_bad, v_total = rig.C.verify_reads(rig.d_pool, rig.crcs, [r[0] for r in reads], [r[1] for r in reads], pb)
    torch.cuda.synchronize()
    assert (u32(v_bad) == bad).all() and int(v_total.item()) == total
    # verify only: the same counts
    (_, bad2, total2), _ = view(rig, oracle, reads, copy=False, cow=False)
    assert (bad2 == bad).all() and total2 == total


# --------------------------------------------------------------------------- 5
@pytest.mark.parametrize("copy", [True, False])
def test_dynamic_tail_and_every_wave(dev, oracle, copy):
    """3,000 reads of 5..8 pages on the 256-byte geometry: more page slots than
    8 waves x CUs x 8, so every wave of the grid has a share and the 1/16 tail
    is handed out dynamically; every read against the model."""
    pb = 256
    rig = filled_rig(dev, oracle, pb, seed=55, batches=(300,))
    rng = np.random.default_rng(5)
    reads = random_reads(rng, 3000, pb, lo=5, hi=8)
    slots = sum(ln // pb for _, ln in reads)
    assert slots > 8 * torch.cuda.get_device_properties(dev).multi_processor_count * 8
    got, want = view(rig, oracle, reads, copy=copy)
    same(got, want)
    assert got[2] == 0


# --------------------------------------------------------------------------- 6
def test_streams_and_threads(dev, oracle):
    """A non-default stream, then two threads with a stream, a pool and slots
    each: COW batch -> snapshot read -> check, three times over."""
    pb = 4096
    s0 = torch.cuda.Stream(device=dev)
    rig = filled_rig(dev, oracle, pb, seed=61, batches=(200,), stream=s0, delta=True)
    rng = np.random.default_rng(6)
    same(*view(rig, oracle, random_reads(rng, 300, pb)))
    same(*view(rig, oracle, random_reads(rng, 30, pb)))
    errs = []

    def work(i):
        try:
            s = torch.cuda.Stream(device=dev)
            r = Rig(dev, oracle, pb, seed=70 + i, stream=s, preset=[])
            g = np.random.default_rng(600 + i)
            for n in (300, 65, 900):
                r.batch(*random_log(g, n, r.orig.size, pb, pb), pb, bool(i))
                r.check()
                got, want = view(r, oracle, random_reads(g, 40 + n, pb), copy=bool((n + i) & 1))
                same(got, want)
                assert got[2] == 0
                cb = r.cb
                (out, bad, total), _ = view(r, oracle, [(c * cb, cb) for c in range(N_CHUNKS)], gap=0)
                assert total == 0
                for c, sl in enumerate(SLOTS):
                    exp = r.orig if sl < N_SLOTS else r.host
                    assert (out[c * cb:(c + 1) * cb] == exp[c * cb:(c + 1) * cb]).all(), (i, n, c)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
