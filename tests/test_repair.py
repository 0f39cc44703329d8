"""Page repair on the device (cc_repair_dev, crc.repair_pages,
DevicePool.repair_bad_pages): everything that needs no GPU.

repair_model is the numpy model of the call as it is built (the claim launch's
table, then every (entry, page) pair against it); replay_repair restates the
header comment of include/curve_crc.h page by page with no claim table at all.
The two must agree.  The GPU tests (test_repair_gpu.py) lean on the model, never
on the code under test.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

U32_MAX = 0xFFFFFFFF
CLEAN, REPAIRED, FAILED, SHADOWED = 0, 1, 2, 3


# --------------------------------------------------------------------------- model and replay
def repair_valid(dst, so, ln, pool_bytes, src_bytes, pb):
    """cc_repair_dev's contract per entry (include/curve_crc.h)."""
    if ln == 0:
        return True
    if dst % pb or ln % pb:
        return False
    if dst >= pool_bytes or ln > pool_bytes - dst:
        return False
    return not (so % 4 or so > src_bytes or ln > src_bytes - so)


def repair_model(pool, crcs, expect, src, entries, pb, crc_fn):
    """One cc_repair_dev call on host arrays, in place (pool uint8, crcs uint32;
    expect uint32 or None; entries = [(dst, src, len)]), the way the device
    does it: the claim table takes the lowest valid index per page, then every
    (entry, page) pair looks its page's word up; the holder judges the page by
    the pool BEFORE the call and resets the word.  Returns (per_entry uint32
    [n, 4], totals uint64 [4], claim uint32 [pool pages])."""
    n_pages = pool.size // pb
    claim = np.full(n_pages, U32_MAX, np.uint32)
    per = np.zeros((len(entries), 4), np.uint32)
    ok = [repair_valid(d, s, n, pool.size, src.size, pb) for d, s, n in entries]
    for i, (dst, so, ln) in enumerate(entries):
        if not ok[i]:
            per[i] = U32_MAX
            continue
        lo, hi = dst // pb, (dst + ln) // pb
        claim[lo:hi] = np.minimum(claim[lo:hi], np.uint32(i))
    before, rec = pool.copy(), (expect if expect is not None else crcs).copy()
    totals = np.zeros(4, np.uint64)
    for i, (dst, so, ln) in enumerate(entries):
        if not ok[i]:
            continue
        for p in range(dst // pb, (dst + ln) // pb):
            if claim[p] != i:
                k = SHADOWED
            else:
                e = int(rec[p])
                at = so + p * pb - dst
                if crc_fn(before[p * pb:(p + 1) * pb]) == e:
                    k = CLEAN
                    if expect is not None:
                        crcs[p] = e
                elif crc_fn(src[at:at + pb]) == e:
                    k = REPAIRED
                    pool[p * pb:(p + 1) * pb] = src[at:at + pb]
                    crcs[p] = e
                else:
                    k = FAILED
            per[i, k] += 1
            totals[k] += 1
    for i, (dst, so, ln) in enumerate(entries):  # the holders put all-ones back
        if ok[i]:
            sel = claim[dst // pb:(dst + ln) // pb]
            sel[sel == i] = U32_MAX
    return per, totals, claim


def replay_repair(pool, crcs, expect, src, entries, pb, crc_fn):
    """The header comment, page by page: the entries naming the page, the
    lowest-indexed valid one handles it, the others are shadowed."""
    per = np.zeros((len(entries), 4), np.uint32)
    for i, (dst, so, ln) in enumerate(entries):
        if not repair_valid(dst, so, ln, pool.size, src.size, pb):
            per[i] = U32_MAX
    for p in range(pool.size // pb):
        naming = [i for i, (dst, so, ln) in enumerate(entries) if per[i, 0] != U32_MAX and dst <= p * pb < dst + ln]
        if not naming:
            continue
        h = naming[0]
        for i in naming[1:]:
            per[i, SHADOWED] += 1
        dst, so, _ = entries[h]
        cand = src[so + p * pb - dst:so + (p + 1) * pb - dst].copy()
        page = pool[p * pb:(p + 1) * pb]
        e = int(expect[p]) if expect is not None else int(crcs[p])
        if crc_fn(page) == e:
            per[h, CLEAN] += 1
            if expect is not None:
                crcs[p] = e
        elif crc_fn(cand) == e:
            per[h, REPAIRED] += 1
            page[:] = cand
            crcs[p] = e
        else:
            per[h, FAILED] += 1
    return per


def flip(a, byte, bit=0):
    a[byte] ^= np.uint8(1 << bit)


def random_case(oracle, rng, pb, n_pages=48, src_pages=256, n=40, with_expect=False, invalid=True):
    """A pool with ~40 % of its pages corrupted (first dword, last dword or a
    random one), a source whose pages are good copies, copies one bit off, or
    copies of the bad live bytes, and n entries of 1-6 pages whose source pages
    line up with their pool pages' kinds.  Returns (pool, crcs, expect, src, entries)."""
    good = rng.integers(0, 256, n_pages * pb, dtype=np.uint8)
    crcs = oracle.page_crcs(good, pb)
    pool = good.copy()
    for p in np.nonzero(rng.random(n_pages) < 0.4)[0]:
        at = [0, pb - 4, 4 * int(rng.integers(0, pb // 4))][int(rng.integers(0, 3))]
        flip(pool, p * pb + at + int(rng.integers(0, 4)), int(rng.integers(0, 8)))
    expect = None
    if with_expect:
        # the authority's table: a third of the pages differ from the local table -- some because the
        # authority holds other bytes (the local page is then bad against it), some because only the
        # local WORD is stale (the live bytes already match the authority)
        expect = crcs.copy()
        for p in np.nonzero(rng.random(n_pages) < 0.33)[0]:
            if rng.random() < 0.5:
                crcs[p] ^= np.uint32(1 << int(rng.integers(0, 32)))            # stale word, bytes as expected
            else:
                good[p * pb:(p + 1) * pb] = rng.integers(0, 256, pb, dtype=np.uint8)  # the authority's bytes differ
                expect[p] = oracle.crc32c(good[p * pb:(p + 1) * pb].tobytes())
    src = rng.integers(0, 256, src_pages * pb, dtype=np.uint8)
    entries, used = [], 0
    for _ in range(n):
        k = int(rng.integers(1, 7))
        p0 = int(rng.integers(0, n_pages - k + 1))
        if used + k > src_pages:
            used = 0
        for j in range(k):
            kind = rng.random()
            s = src[(used + j) * pb:(used + j + 1) * pb]
            if kind < 0.6:
                s[:] = good[(p0 + j) * pb:(p0 + j + 1) * pb]
            elif kind < 0.8:
                s[:] = good[(p0 + j) * pb:(p0 + j + 1) * pb]
                flip(s, int(rng.integers(0, pb)), int(rng.integers(0, 8)))
            else:
                s[:] = pool[(p0 + j) * pb:(p0 + j + 1) * pb]
        entries.append((p0 * pb, used * pb, k * pb))
        used += k
    if invalid:
        bad = [(pb // 2, 0, pb), (0, 0, pb + 4), ((n_pages - 1) * pb, 0, 2 * pb), (n_pages * pb, 0, pb),
               (1 << 40, 0, pb), (0, 6, pb), (0, (src_pages - 1) * pb, 2 * pb), (0, 1 << 40, pb), (3 * pb, 0, 0)]
        for e in bad:
            entries.insert(int(rng.integers(0, len(entries) + 1)), e)
    return pool, crcs, expect, src, entries


@pytest.mark.parametrize("with_expect", [False, True])
@pytest.mark.parametrize("pb", [256, 1024])
def test_model_equals_the_page_by_page_replay(oracle, pb, with_expect):
    crc_fn = lambda b: oracle.crc32c(b.tobytes())
    seen = np.zeros(4, np.uint64)
    for seed in range(6):
        rng = np.random.default_rng(1000 * pb + seed)
        pool, crcs, expect, src, entries = random_case(oracle, rng, pb, with_expect=with_expect)
        pool0, crcs0 = pool.copy(), crcs.copy()
        r_pool, r_crcs = pool.copy(), crcs.copy()
        per, totals, claim = repair_model(pool, crcs, expect, src, entries, pb, crc_fn)
        r_per = replay_repair(r_pool, r_crcs, expect, src, entries, pb, crc_fn)
        assert (per == r_per).all() and (pool == r_pool).all() and (crcs == r_crcs).all()
        assert (claim == U32_MAX).all()
        ok = per[:, 0] != U32_MAX
        assert (totals == per[ok].sum(axis=0)).all()
        for i, (dst, so, ln) in enumerate(entries):
            valid = repair_valid(dst, so, ln, pool.size, src.size, pb)
            assert valid == bool(ok[i])
            if valid:
                assert int(per[i].sum()) == ln // pb                         # the four counts sum to the page count
            else:
                assert (per[i] == U32_MAX).all()
        assert (~ok).sum() == 8
        # the postcondition, page by page
        rec = expect if expect is not None else crcs0
        now = oracle.page_crcs(pool, pb)
        handled = np.zeros(pool.size // pb, bool)
        for i, (dst, so, ln) in enumerate(entries):
            if ok[i]:
                handled[dst // pb:(dst + ln) // pb] = True
        fine = handled & (now == rec)                                        # clean or repaired
        assert (crcs[fine] == rec[fine]).all()
        rest = ~fine                                                         # failed, or named by no valid entry
        assert (pool.reshape(-1, pb)[rest] == pool0.reshape(-1, pb)[rest]).all() and (crcs[rest] == crcs0[rest]).all()
        assert fine.sum() == int(totals[CLEAN] + totals[REPAIRED]) and (handled & rest).sum() == int(totals[FAILED])
        seen += totals
    assert (seen >= 20).all(), seen


# --------------------------------------------------------------------------- cases by hand
PB = 256


def hand(oracle, n_pages=8, src_pages=8, seed=3):
    rng = np.random.default_rng(seed)
    good = rng.integers(0, 256, n_pages * PB, dtype=np.uint8)
    return good, oracle.page_crcs(good, PB), rng.integers(0, 256, src_pages * PB, dtype=np.uint8)


def run(oracle, pool, crcs, expect, src, entries):
    return repair_model(pool, crcs, expect, src, entries, PB, lambda b: oracle.crc32c(b.tobytes()))


def page(a, p):
    return a[p * PB:(p + 1) * PB]


def test_a_good_candidate_repairs_and_a_bad_one_does_not(oracle):
    good, crcs, src = hand(oracle)
    pool = good.copy()
    flip(pool, 2 * PB + 7, 3)
    flip(pool, 5 * PB + PB - 1, 7)
    page(src, 0)[:] = page(good, 2)                        # a good copy
    page(src, 1)[:] = page(good, 5)
    flip(src, 1 * PB + 100, 0)                             # one bit off
    before = pool.copy()
    per, totals, _ = run(oracle, pool, crcs, None, src, [(2 * PB, 0, PB), (5 * PB, PB, PB)])
    assert per.tolist() == [[0, 1, 0, 0], [0, 0, 1, 0]] and totals.tolist() == [0, 1, 1, 0]
    assert (page(pool, 2) == page(good, 2)).all()
    assert (page(pool, 5) == page(before, 5)).all()        # untouched
    assert (crcs == oracle.page_crcs(good, PB)).all()


def test_a_good_live_page_is_clean_and_nothing_is_written(oracle):
    good, crcs, src = hand(oracle)
    pool = good.copy()
    page(src, 0)[:] = 0xAB                                 # whatever the candidate holds
    per, totals, _ = run(oracle, pool, crcs, None, src, [(3 * PB, 0, PB)])
    assert per.tolist() == [[1, 0, 0, 0]] and (pool == good).all() and (crcs == oracle.page_crcs(good, PB)).all()


def test_a_candidate_equal_to_the_bad_live_bytes_fails(oracle):
    good, crcs, src = hand(oracle)
    pool = good.copy()
    flip(pool, 4 * PB, 0)
    page(src, 3)[:] = page(pool, 4)
    before = pool.copy()
    per, _, _ = run(oracle, pool, crcs, None, src, [(4 * PB, 3 * PB, PB)])
    assert per.tolist() == [[0, 0, 1, 0]] and (pool == before).all()


def test_expect_mends_a_stale_word_and_leaves_a_failed_page_alone(oracle):
    good, crcs, src = hand(oracle)
    expect = crcs.copy()
    pool = good.copy()
    crcs[1] ^= 0x10                                        # page 1: only the local word is stale
    other = np.arange(PB, dtype=np.uint8)                  # page 6: the authority holds other bytes ...
    expect[6] = oracle.crc32c(other.tobytes())
    page(src, 0)[:] = 0                                    # ... and this peer's copy is not them
    page(src, 1)[:] = 0
    page(src, 2)[:] = other                                # page 7 likewise, with a true copy on offer
    expect[7] = expect[6]
    crcs0 = crcs.copy()
    per, totals, _ = run(oracle, pool, crcs, expect, src, [(1 * PB, 0, PB), (6 * PB, PB, PB), (7 * PB, 2 * PB, PB)])
    assert per.tolist() == [[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0]]
    assert crcs[1] == expect[1] != crcs0[1] and (page(pool, 1) == page(good, 1)).all()
    assert crcs[6] == crcs0[6] != expect[6] and (page(pool, 6) == page(good, 6)).all()   # page and word kept
    assert crcs[7] == expect[7] and (page(pool, 7) == other).all()


def test_the_lowest_index_handles_the_page_even_with_a_bad_candidate(oracle):
    good, crcs, src = hand(oracle)
    pool = good.copy()
    flip(pool, 2 * PB + 9, 1)
    page(src, 0)[:] = 0x11                                 # entry 0: a bad candidate
    page(src, 1)[:] = page(good, 2)                        # entry 1: a good one, never looked at
    before = pool.copy()
    per, totals, claim = run(oracle, pool, crcs, None, src, [(2 * PB, 0, PB), (2 * PB, PB, PB)])
    assert per.tolist() == [[0, 0, 1, 0], [0, 0, 0, 1]] and totals.tolist() == [0, 0, 1, 1]
    assert (pool == before).all() and (claim == U32_MAX).all()
    # sent again in a later call, the second peer's copy mends it
    per, _, _ = run(oracle, pool, crcs, None, src, [(2 * PB, PB, PB)])
    assert per.tolist() == [[0, 1, 0, 0]] and (pool == good).all()


def test_each_invalidity_rule_and_the_empty_entry(oracle):
    good, crcs, src = hand(oracle)
    pool = good.copy()
    pool_bytes, src_bytes = pool.size, src.size
    cases = {
        "dst misaligned": (PB // 2, 0, PB),
        "len misaligned": (0, 0, PB + 4),
        "past the pool": (pool_bytes - PB, 0, 2 * PB),
        "at the pool's end": (pool_bytes, 0, PB),
        "src unaligned": (0, 2, PB),
        "src past its buffer": (0, src_bytes - PB, 2 * PB),
    }
    for name, e in cases.items():
        assert not repair_valid(*e, pool_bytes, src_bytes, PB), name
        per, totals, claim = run(oracle, pool, crcs, None, src, [e])
        assert (per == U32_MAX).all() and not totals.any() and (claim == U32_MAX).all(), name
    assert (pool == good).all()
    assert repair_valid(pool_bytes - PB, src_bytes - PB, PB, pool_bytes, src_bytes, PB)     # both ends exactly
    per, totals, _ = run(oracle, pool, crcs, None, src, [(3 * PB, 0, 0), (1 << 40, 1, 0)])
    assert not per.any() and not totals.any()              # len == 0: valid, its words left alone


# --------------------------------------------------------------------------- the drivers over the model
class Host:
    """A host array where crc.repair_pages expects a device tensor it reads back (.cpu().numpy())."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def as_np(x, dtype=None):
    a = x.numpy() if hasattr(x, "numpy") else x
    a = a.reshape(-1)
    return a.view(dtype) if dtype is not None else a


def model_repair(monkeypatch, oracle, calls):
    """crc.repair replaced by repair_model on the host arrays (or CPU tensors) it is handed."""
    from curve_amd import crc as C

    def fake_repair(pool, crcs, src, dst, so, lens, claim, expect=None, page_bytes=PB, stream=None):
        entries = [(int(d), int(s), int(n)) for d, s, n in zip(dst, so, lens)]
        calls.append(entries)
        per, totals, _ = repair_model(as_np(pool, np.uint8), as_np(crcs, np.uint32),
                                      as_np(expect, np.uint32) if expect is not None else None,
                                      as_np(src, np.uint8), entries, page_bytes, lambda b: oracle.crc32c(b.tobytes()))
        return Host(per.view(np.int32)), totals

    monkeypatch.setattr(C, "repair", fake_repair)
    return C


def peers(good, pool, pages_bad_at_first):
    """Two peers holding the pool's good pages; the first one's copy of some pages is itself corrupt.
    Each fetcher packs the pages it is asked for back to back."""
    first = good.copy()
    for p in pages_bad_at_first:
        flip(first, p * PB + 17, 2)
    asked = []

    def fetcher(image, who):
        def fetch(pages):
            asked.append((who, [int(p) for p in pages]))
            return np.concatenate([page(image, int(p)) for p in pages]), np.arange(len(pages)) * PB
        return fetch

    return fetcher(first, 0), fetcher(good, 1), asked


def test_repair_pages_goes_to_the_second_peer_for_what_the_first_could_not_mend(oracle, monkeypatch):
    calls = []
    C = model_repair(monkeypatch, oracle, calls)
    good, crcs, _ = hand(oracle, n_pages=16)
    pool = good.copy()
    for p in (1, 4, 9, 12):
        flip(pool, p * PB + p, 5)
    f0, f1, asked = peers(good, pool, [4, 12])
    pages, cls, by = C.repair_pages(pool, crcs, [12, 4, 7, 9, 4, 1, 12], [f0, f1], None, page_bytes=PB)   # 7 is fine
    assert pages.tolist() == [1, 4, 7, 9, 12]                                # unique, ascending
    assert cls.tolist() == [REPAIRED, REPAIRED, CLEAN, REPAIRED, REPAIRED] and by.tolist() == [0, 1, -1, 0, 1]
    assert asked == [(0, [1, 4, 7, 9, 12]), (1, [4, 12])]
    assert [[e[0] // PB for e in c] for c in calls] == [[1, 4, 7, 9, 12], [4, 12]]
    assert all(e[2] == PB for c in calls for e in c)                         # one one-page entry per page
    assert (pool == good).all()
    # a page no peer can mend stays failed, and a fetcher after the last failure is not asked
    flip(pool, 3 * PB, 0)
    bad_peer = lambda pages: (np.zeros(len(pages) * PB, np.uint8), np.arange(len(pages)) * PB)
    pages, cls, by = C.repair_pages(pool, crcs, [3], [bad_peer, bad_peer], None, page_bytes=PB)
    assert cls.tolist() == [FAILED] and by.tolist() == [-1]
    del asked[:]
    pages, cls, by = C.repair_pages(pool, crcs, [3, 5], [f1, f0], None, page_bytes=PB)
    assert cls.tolist() == [REPAIRED, CLEAN] and by.tolist() == [0, -1] and asked == [(1, [3, 5])]
    pages, cls, by = C.repair_pages(pool, crcs, [], [f1], None, page_bytes=PB)
    assert pages.size == 0 and cls.size == 0 and by.size == 0


def test_repair_pages_refuses_a_fetcher_with_the_wrong_number_of_offsets(oracle, monkeypatch):
    from curve_amd._lib import CC_EINVAL, CurveCrcError
    C = model_repair(monkeypatch, oracle, [])
    good, crcs, src = hand(oracle)
    with pytest.raises(CurveCrcError) as e:
        C.repair_pages(good.copy(), crcs, [1, 2, 3], [lambda pages: (src, [0, PB])], None, page_bytes=PB)
    assert e.value.code == CC_EINVAL
    with pytest.raises(CurveCrcError) as e:                                  # a page beyond the pool
        C.repair_pages(good.copy(), crcs, [1, 99], [lambda pages: (src, [0, PB])], None, page_bytes=PB)
    assert e.value.code == CC_EINVAL


def test_repair_bad_pages_chains_detect_repair_verify(oracle, monkeypatch):
    torch = pytest.importorskip("torch")
    from curve_amd import scan as S
    calls = []
    C = model_repair(monkeypatch, oracle, calls)
    n_chunks, ppc = 3, 8
    good, expect, _ = hand(oracle, n_pages=n_chunks * ppc)
    pool = good.copy()
    bad = [2, 9, 15, 20]
    for p in bad:
        flip(pool, p * PB + 3, 4)
    verifies = []

    def mismatches(pages, expected):
        now = oracle.page_crcs(as_np(pages, np.uint8), PB)
        return np.nonzero(now != as_np(expected, np.uint32))[0]

    def fake_list(pages, expected, page_bytes=PB, max_bad=4096, stream=None):
        m = mismatches(pages, expected)[::-1]                                # unordered, as the device's list
        lst = torch.full((max(1, max_bad),), -1, dtype=torch.int64)
        lst[:min(m.size, max_bad)] = torch.from_numpy(m[:max_bad].copy())
        return torch.tensor([m.size, int(m.min()) if m.size else -1]), lst

    def fake_verify(pages, expected, page_bytes=PB, stream=None, counters=None):
        m = mismatches(pages, expected)
        verifies.append(m.tolist())
        return torch.tensor([m.size, int(m.min()) if m.size else -1])

    monkeypatch.setattr(C, "page_verify_list", fake_list)
    monkeypatch.setattr(C, "page_verify", fake_verify)
    data = torch.from_numpy(pool).reshape(n_chunks, ppc * PB)
    meta = torch.zeros((n_chunks, PB), dtype=torch.uint8)
    dp = S.ChunkPool(data, meta, [7, 8, 9], page_bytes=PB, scan_size=ppc * PB)
    assert S.ChunkPool is S.DevicePool
    dp.page_crcs.zero_()                                                     # a local table that is all stale
    d_expect = torch.from_numpy(expect.view(np.int32).copy())
    f0, f1, asked = peers(good, pool, [9, 20])
    bad_peer = lambda pages: (np.zeros(len(pages) * PB, np.uint8), np.arange(len(pages)) * PB)
    repaired, still = dp.repair_bad_pages(d_expect, [f0, f1])
    assert repaired == [(0, 2, 0), (1, 1, 1), (1, 7, 0), (2, 4, 1)] and still == []
    assert asked == [(0, bad), (1, [9, 20])] and verifies == [[]]
    assert (pool == good).all()                                              # the tensor's memory: mended in place
    assert (as_np(dp.page_crcs, np.uint32)[bad] == expect[bad]).all()
    # nothing bad: no fetch, no second verify
    del asked[:], verifies[:]
    assert dp.repair_bad_pages(d_expect, [f0, f1]) == ([], []) and asked == [] and verifies == []
    # a page no peer holds stays bad and is reported
    flip(pool, 11 * PB, 0)
    flip(pool, 12 * PB, 0)
    repaired, still = dp.repair_bad_pages(d_expect, [bad_peer, lambda pages: f1(pages) if 11 not in pages else
                                                     bad_peer(pages)])
    assert repaired == [] and still == [(1, 3), (1, 4)] and verifies == [[11, 12]]
    repaired, still = dp.repair_bad_pages(d_expect, [f1])
    assert repaired == [(1, 3, 0), (1, 4, 0)] and still == []
    with pytest.raises(C.CurveCrcError):
        flip(pool, 0, 0)
        dp.repair_bad_pages(d_expect, [f1], max_bad=0)


# --------------------------------------------------------------------------- ABI
FAKE = 1 << 20  # a fake device pointer: never dereferenced (the checks come first, and no device is present)


def _repair(L, pool=FAKE, pool_bytes=1 << 20, page_bytes=4096, src=FAKE, src_bytes=1 << 20, reqs=FAKE, n=3, crcs=FAKE,
            expect=None, claim=FAKE, per_entry=FAKE, totals=None):
    vp = ctypes.c_void_p
    return L.cc_repair_dev(vp(pool), pool_bytes, page_bytes, vp(src), src_bytes, vp(reqs), n, vp(crcs), vp(expect),
                           vp(claim), vp(per_entry), vp(totals), None)


def test_header_declares_and_library_exports_the_symbol():
    from curve_amd import _lib
    from curve_amd import crc as C
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    assert re.search(r"^int cc_repair_dev\(", hdr, re.M)
    assert hasattr(_lib.lib(), "cc_repair_dev") and len(_lib.SIGNATURES["cc_repair_dev"][1]) == 13
    decl = hdr[hdr.index("int cc_repair_dev("):]
    decl = decl[:decl.index(";")]
    assert len(decl.split(",")) == 13
    for name in ("repair_records", "repair", "repair_claim", "repair_pages"):
        assert callable(getattr(C, name)), name
    from curve_amd.scan import DevicePool
    assert callable(DevicePool.repair_bad_pages)


def test_cc_repair_counts_has_the_headers_layout():
    from curve_amd import _lib
    from curve_amd import crc as C
    hdr = open(os.path.join(ROOT, "include", "curve_crc.h")).read()
    body = hdr[hdr.index("typedef struct cc_repair_counts {"):hdr.index("} cc_repair_counts;")]
    names = re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["clean", "repaired", "failed", "shadowed"] == list(C.REPAIR_CLASSES)
    assert [f[0] for f in _lib.CcRepairCounts._fields_] == names
    assert ctypes.sizeof(_lib.CcRepairCounts) == 16
    assert [getattr(_lib.CcRepairCounts, n).offset for n in names] == [0, 4, 8, 12]
    assert (C.REPAIR_CLEAN, C.REPAIR_REPAIRED, C.REPAIR_FAILED, C.REPAIR_SHADOWED) == (0, 1, 2, 3)


def test_argument_checks_need_no_gpu():
    from curve_amd import _lib
    L = _lib.lib()
    E = _lib.CC_EINVAL
    for pb in (0, 100, 128, 1000, 3 * 256, 16384):                           # not 256 * 2^k, k = 0..5
        assert _repair(L, page_bytes=pb) == E, pb
    assert _repair(L, pool_bytes=(1 << 20) + 256) == E                       # not whole 4 KiB pages
    assert _repair(L, n=1 << 31) == E
    assert _repair(L, pool=FAKE + 2) == E and _repair(L, src=FAKE + 1) == E  # misaligned pool / source
    for name in ("pool", "src", "reqs", "crcs", "claim", "per_entry"):
        assert _repair(L, **{name: None}) == E, name
    assert _repair(L, n=0) == _lib.CC_OK                                     # an empty batch is a no-op
    assert _repair(L, n=0, expect=FAKE, totals=FAKE) == _lib.CC_OK


def test_the_built_library_holds_the_repair_kernels_for_gfx950_without_scratch(tmp_path):
    """The code object inside libcurvecrc.so, as the build left it: the claim
    kernel and the six repair_kernel<M> are there for gfx950, none with a
    private segment (scratch) or a spilled VGPR, each within the 256 VGPRs of two
    waves a SIMD (the 160 KiB LDS image allows no more)."""
    import shutil
    import subprocess
    from curve_amd import _lib
    llvm = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin")
    so = shutil.copy(_lib.LIB_PATH, str(tmp_path / "libcurvecrc.so"))
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], check=True, capture_output=True)
    kernels = {}
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        assert f.endswith("gfx950"), f
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", str(tmp_path / f)], check=True,
                               capture_output=True, text=True).stdout
        for entry in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            kernels[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|"
                                                              r"vgpr_spill_count|sgpr_spill_count):\s+(\d+)", entry)}
    assert any("paste_kernel" in k for k in kernels)              # the parse sees the kernels that were there before
    new = {k: v for k, v in kernels.items() if "repair_claim_kernel" in k or "repair_kernelILi" in k}
    assert sorted(re.search(r"repair_kernelILi(\d+)E", k).group(1) for k in new if "ILi" in k) == \
        sorted(["1", "2", "4", "8", "16", "32"]) and len(new) == 7, sorted(new)
    for k, v in new.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 256, (k, v)


def test_a_well_formed_call_needs_a_device():
    from curve_amd import _lib
    L = _lib.lib()
    if L.cc_device_count() > 0:
        pytest.skip("a GPU is visible")
    N = _lib.CC_ENODEV
    assert _repair(L) == N and _repair(L, expect=FAKE, totals=FAKE) == N     # both optional pointers, either way
    assert _repair(L, n=(1 << 31) - 1) == N
    for pb in (256, 512, 1024, 2048, 4096, 8192):
        assert _repair(L, page_bytes=pb) == N, pb
    assert _repair(L, src_bytes=0) == N                                      # every entry invalid: still a device call
