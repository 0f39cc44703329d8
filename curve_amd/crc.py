"""Host-side mirror of the reference's CRC32C surface.

`CRC32` mirrors curve::common::CRC32 (src/common/crc32.h:40-55): the two
overloads become one function with an optional leading `crc`.  Device batch
operations work on torch CUDA tensors (device memory + the current stream are
plumbing; the compute is libcurvecrc's HIP kernels) and raise `CurveCrcError`
on any failure -- there is no CPU fallback for them.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Union

from . import _lib
from ._lib import CurveCrcError, check, lib

PAGE_SIZE = 4096                # conf/chunkserver.conf:22 (blocksize / page)
CHUNK_SIZE = 16 * 1024 * 1024   # conf/chunkserver.conf:13
META_PAGE_SIZE = 4096           # conf/chunkserver.conf:16
SCAN_SIZE = 4 * 1024 * 1024     # conf/chunkserver.conf:114


def _host_buf(data):
    if isinstance(data, (bytes, bytearray)):
        b = bytes(data)
        return ctypes.c_char_p(b), len(b), b
    if isinstance(data, memoryview):
        b = data.tobytes()
        return ctypes.c_char_p(b), len(b), b
    try:  # numpy array
        import numpy as np
        if isinstance(data, np.ndarray):
            a = np.ascontiguousarray(data)
            return ctypes.c_void_p(a.ctypes.data), a.nbytes, a
    except ImportError:  # pragma: no cover
        pass
    if isinstance(data, str):
        b = data.encode()
        return ctypes.c_char_p(b), len(b), b
    raise TypeError(f"unsupported buffer type {type(data)!r}")


def CRC32(*args) -> int:
    """CRC32(data) == curve::common::CRC32(pData, iLen)           (crc32.h:40-42)
       CRC32(crc, data) == curve::common::CRC32(crc, pData, iLen)  (crc32.h:53-55)
    CPU primitive for small buffers (metapage headers, conf-epoch, ...)."""
    if len(args) == 1:
        crc, data = 0, args[0]
    elif len(args) == 2:
        crc, data = args
    else:
        raise TypeError("CRC32(data) or CRC32(crc, data)")
    p, n, _keep = _host_buf(data)
    return int(lib().crc32c_extend(int(crc) & 0xFFFFFFFF, p, n))


def CRC32_iov(fragments, crc: int = 0) -> int:
    """crc32c_extend_iov: one CRC over a scattered buffer, as braft::crc32(const
    butil::IOBuf&) extends it across the IOBuf's blocks (raftlog/curve_segment.cpp:405)."""
    keep = [_host_buf(f) for f in fragments]
    iov = (_lib.IoVec * max(1, len(keep)))()
    for i, (p, n, _k) in enumerate(keep):
        iov[i].iov_base = ctypes.cast(p, ctypes.c_void_p).value if n else None
        iov[i].iov_len = n
    return int(lib().crc32c_extend_iov(int(crc) & 0xFFFFFFFF, iov, len(keep)))


def slice_fold(page_crcs, pages_per_slice: int, page_bytes: int = PAGE_SIZE):
    """cc_slice_fold: page CRCs -> one CRC per slice of pages_per_slice pages (host)."""
    import numpy as np
    a = np.ascontiguousarray(page_crcs, dtype=np.uint32)
    if pages_per_slice <= 0 or a.size % pages_per_slice:
        raise CurveCrcError(_lib.CC_EINVAL, "page count is not a multiple of pages_per_slice")
    out = np.empty(a.size // pages_per_slice, dtype=np.uint32)
    check(lib().cc_slice_fold(ctypes.c_void_p(a.ctypes.data), a.size, pages_per_slice, page_bytes,
                              ctypes.c_void_p(out.ctypes.data)), "cc_slice_fold")
    return out


def crc_bufs_host(bufs):
    """cc_crc_bufs_host: CRC32 of every host buffer in one blocking device call."""
    import numpy as np
    keep = [_host_buf(b) for b in bufs]
    n = len(keep)
    ptrs = (ctypes.c_void_p * max(1, n))(*[ctypes.cast(p, ctypes.c_void_p).value for p, _, _ in keep])
    lens = np.array([k[1] for k in keep], dtype=np.uint64)
    out = np.empty(n, dtype=np.uint32)
    check(lib().cc_crc_bufs_host(ptrs, ctypes.c_void_p(lens.ctypes.data), n, ctypes.c_void_p(out.ctypes.data)),
          "cc_crc_bufs_host")
    return out


def combine(crc_a: int, crc_b: int, len_b: int) -> int:
    return int(lib().crc32c_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, int(len_b)))


def shift(crc: int, nbytes: int) -> int:
    return int(lib().crc32c_shift(crc & 0xFFFFFFFF, int(nbytes)))


def zeros(nbytes: int) -> int:
    return int(lib().crc32c_zeros(int(nbytes)))


def fold_host(page_crcs, page_bytes: int) -> int:
    import numpy as np
    a = np.ascontiguousarray(page_crcs, dtype=np.uint32)
    return int(lib().cc_fold_host(ctypes.c_void_p(a.ctypes.data), a.size, int(page_bytes)))


def device_count() -> int:
    return int(lib().cc_device_count())


def engine_init(page_bytes: int = 0, slice_bytes: int = 0, staging_bytes: int = 0) -> None:
    o = _lib.CcOpts(page_bytes, slice_bytes, staging_bytes)
    check(lib().cc_engine_init(ctypes.byref(o)), "cc_engine_init")


def engine_fini() -> None:
    check(lib().cc_engine_fini(), "cc_engine_fini")


# ---------------------------------------------------------------------------
# device batch operations (torch tensors as device-memory handles)
# ---------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _stream_handle(stream) -> Optional[int]:
    torch = _torch()
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _on_stream(stream):
    """Context in which tensors are created on `stream` (the stream the native
    call enqueues on), so an output's initialisation (torch.full / zeros) is
    ordered before the kernel that writes it."""
    import contextlib
    torch = _torch()
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _stream_key(device, stream):
    """Cache key of per-stream scratch: (device, HIP stream handle)."""
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return (device, s.cuda_stream)


def _dev_ptr(t, what: str):
    if not t.is_cuda:
        raise CurveCrcError(_lib.CC_EINVAL, f"{what} must be a device tensor")
    if not t.is_contiguous():
        raise CurveCrcError(_lib.CC_EINVAL, f"{what} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def page_crc(pages, page_bytes: int = PAGE_SIZE, out=None, stream=None):
    """CRC32C of every `page_bytes` page of the device tensor `pages` (any dtype,
    contiguous, size a multiple of page_bytes) -> int32 tensor of CRC bits
    (uint32 values viewed as int32; `.view(torch.uint32)` / `& 0xFFFFFFFF` to read)."""
    torch = _torch()
    nb = _nbytes(pages)
    if nb % page_bytes:
        raise CurveCrcError(_lib.CC_EINVAL, "pages size is not a multiple of page_bytes")
    n = nb // page_bytes
    if out is None:
        with _on_stream(stream):  # created on the stream the kernel writes it on
            out = torch.empty(n, dtype=torch.int32, device=pages.device)
    elif out.numel() < n or out.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "out too small or not 32-bit")
    with torch.cuda.device(pages.device):
        check(lib().cc_page_crc_dev(_dev_ptr(pages, "pages"), n, page_bytes, _dev_ptr(out, "out"),
                                    _stream_handle(stream)), "cc_page_crc_dev")
    return out


def page_verify(pages, expected, page_bytes: int = PAGE_SIZE, stream=None, counters=None):
    """Recompute and compare.  Returns a 2-element int64 device tensor
    [bad_count, first_bad] (first_bad = 2^64-1 -> -1 when clean); no host sync."""
    torch = _torch()
    nb = _nbytes(pages)
    if nb % page_bytes:
        raise CurveCrcError(_lib.CC_EINVAL, "pages size is not a multiple of page_bytes")
    n = nb // page_bytes
    if expected.numel() < n or expected.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "expected must hold one 32-bit CRC per page")
    if counters is None:
        with _on_stream(stream):
            counters = torch.tensor([0, -1], dtype=torch.int64, device=pages.device)
    base = counters.data_ptr()
    with torch.cuda.device(pages.device):
        check(lib().cc_page_verify_dev(_dev_ptr(pages, "pages"), n, page_bytes, _dev_ptr(expected, "expected"),
                                       ctypes.c_void_p(base), ctypes.c_void_p(base + 8),
                                       _stream_handle(stream)), "cc_page_verify_dev")
    return counters


def hbm_read_probe(buf, sink, stream=None):
    """cc_hbm_read_probe_dev (diagnostic): pure nt read of `buf`; sink must hold
    2*CUs*16 int32."""
    check(lib().cc_hbm_read_probe_dev(_dev_ptr(buf, "buf"), _nbytes(buf), _dev_ptr(sink, "sink"),
                                      _stream_handle(stream)), "cc_hbm_read_probe_dev")


def page_load_probe(pages, out, stream=None):
    """cc_page_load_probe_dev (diagnostic): the page kernel's schedule and
    traffic over the 4 KiB pages of `pages` without the CRC arithmetic; `out`
    (one int32 per page) receives meaningless words."""
    n = _nbytes(pages) // PAGE_SIZE
    if out.numel() < n or out.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "out too small or not 32-bit")
    check(lib().cc_page_load_probe_dev(_dev_ptr(pages, "pages"), n, _dev_ptr(out, "out"), _stream_handle(stream)),
          "cc_page_load_probe_dev")


def page_verify_list(pages, expected, page_bytes: int = PAGE_SIZE, max_bad: int = 4096, stream=None):
    """cc_page_verify_list_dev: -> (counters [bad_count, first_bad] int64 device
    tensor, bad page indices int64 device tensor of max_bad slots; the first
    min(bad_count, max_bad) are valid, unordered).  No host sync."""
    torch = _torch()
    nb = _nbytes(pages)
    if nb % page_bytes:
        raise CurveCrcError(_lib.CC_EINVAL, "pages size is not a multiple of page_bytes")
    n = nb // page_bytes
    if expected.numel() < n or expected.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "expected must hold one 32-bit CRC per page")
    with _on_stream(stream):
        counters = torch.tensor([0, -1], dtype=torch.int64, device=pages.device)
        bad = torch.full((max(1, max_bad),), -1, dtype=torch.int64, device=pages.device)
    base = counters.data_ptr()
    with torch.cuda.device(pages.device):
        check(lib().cc_page_verify_list_dev(_dev_ptr(pages, "pages"), n, page_bytes, _dev_ptr(expected, "expected"),
                                            ctypes.c_void_p(base), ctypes.c_void_p(base + 8),
                                            ctypes.c_void_p(bad.data_ptr()), max_bad,
                                            _stream_handle(stream)), "cc_page_verify_list_dev")
    return counters, bad


def fold(crcs, per_group: int, unit_bytes: int, out=None, stream=None):
    """Group fold on device: out[g] = CRC of the concatenation of `per_group`
    consecutive units (each `unit_bytes`) given their CRCs."""
    torch = _torch()
    n = crcs.numel()
    if per_group <= 0 or n % per_group:
        raise CurveCrcError(_lib.CC_EINVAL, "crcs count is not a multiple of per_group")
    g = n // per_group
    if out is None:
        with _on_stream(stream):  # created on the stream the kernel writes it on
            out = torch.empty(g, dtype=torch.int32, device=crcs.device)
    with torch.cuda.device(crcs.device):
        check(lib().cc_fold_dev(_dev_ptr(crcs, "crcs"), g, per_group, int(unit_bytes), _dev_ptr(out, "out"),
                                _stream_handle(stream)), "cc_fold_dev")
    return out


def shift_dev(crcs, shift_bytes, out=None, stream=None):
    """out[i] = shift(crcs[i], shift_bytes[i]) on device (int64 shift counts)."""
    torch = _torch()
    n = crcs.numel()
    if shift_bytes.numel() != n or shift_bytes.element_size() != 8:
        raise CurveCrcError(_lib.CC_EINVAL, "shift_bytes must be int64, one per crc")
    if out is None:
        with _on_stream(stream):  # created on the stream the kernel writes it on
            out = torch.empty(n, dtype=torch.int32, device=crcs.device)
    with torch.cuda.device(crcs.device):
        check(lib().cc_shift_dev(_dev_ptr(crcs, "crcs"), _dev_ptr(shift_bytes, "shift_bytes"), n,
                                 _dev_ptr(out, "out"), _stream_handle(stream)), "cc_shift_dev")
    return out


def crc_ranges(buf, offsets, lengths, out=None, stream=None):
    """CRC32C (Value) of arbitrary byte ranges of the device tensor `buf`
    (cc_crc_ranges_dev) -> int32 device tensor."""
    import numpy as np
    torch = _torch()
    offs = np.asarray(offsets, dtype=np.uint64)
    lens = np.asarray(lengths, dtype=np.uint64)
    if offs.size != lens.size:
        raise CurveCrcError(_lib.CC_EINVAL, "offsets / lengths mismatch")
    if (offs + lens > _nbytes(buf)).any():
        raise CurveCrcError(_lib.CC_EINVAL, "range beyond the buffer")
    rec = np.empty((offs.size, 2), dtype=np.uint64)
    rec[:, 0], rec[:, 1] = offs, lens
    with _on_stream(stream):
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(buf.device)
        if out is None:
            out = torch.empty(offs.size, dtype=torch.int32, device=buf.device)
    with torch.cuda.device(buf.device):
        check(lib().cc_crc_ranges_dev(_dev_ptr(buf, "buf"), _dev_ptr(d_rec, "ranges"), offs.size,
                                      _dev_ptr(out, "out"), _stream_handle(stream)), "cc_crc_ranges_dev")
    if stream is not None:
        d_rec.record_stream(stream)
    return out


def xpow8(nbytes, out=None, stream=None):
    """x^(8*n) mod P per element (cc_xpow8_dev): the shift multipliers of a static layout."""
    torch = _torch()
    if out is None:
        with _on_stream(stream):  # created on the stream the kernel writes it on
            out = torch.empty(nbytes.numel(), dtype=torch.int32, device=nbytes.device)
    with torch.cuda.device(nbytes.device):
        check(lib().cc_xpow8_dev(_dev_ptr(nbytes, "nbytes"), nbytes.numel(), _dev_ptr(out, "out"),
                                 _stream_handle(stream)), "cc_xpow8_dev")
    return out


def scan_epilogue(page_crcs, meta_crcs, n_chunks: int, pages_per_chunk: int, page_bytes: int,
                  pages_per_slice: int, slice_out, file_out=None, after_mult=None, group=None, digest=None,
                  stream=None):
    """Fused epilogue (cc_scan_epilogue_dev): slices, file CRCs, digest partials in
    one launch.  after_mult = xpow8(after_bytes) (int32 view of the multipliers)."""
    torch = _torch()
    opt = lambda t, w: _dev_ptr(t, w) if t is not None else None  # noqa: E731
    with torch.cuda.device(page_crcs.device):
        check(lib().cc_scan_epilogue_dev(_dev_ptr(page_crcs, "page_crcs"), _dev_ptr(meta_crcs, "meta_crcs"),
                                         n_chunks, pages_per_chunk, page_bytes, pages_per_slice,
                                         _dev_ptr(slice_out, "slice_out"), opt(file_out, "file_out"),
                                         opt(after_mult, "after_mult"), opt(group, "group"), opt(digest, "digest"),
                                         _stream_handle(stream)), "cc_scan_epilogue_dev")
    return slice_out


def combine_dev(a, b, len_b: int, out=None, stream=None):
    """out[i] = combine(a[i], b[i], len_b) on device."""
    torch = _torch()
    n = a.numel()
    if b.numel() != n:
        raise CurveCrcError(_lib.CC_EINVAL, "a / b length mismatch")
    if out is None:
        with _on_stream(stream):  # created on the stream the kernel writes it on
            out = torch.empty(n, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().cc_combine_dev(_dev_ptr(a, "a"), _dev_ptr(b, "b"), int(len_b), n, _dev_ptr(out, "out"),
                                   _stream_handle(stream)), "cc_combine_dev")
    return out


def digest_fold_dev(gathered, nranks: int, out=None, stream=None):
    """cc_digest_fold_dev: gathered [nranks * n] int32 device partials -> XOR over ranks [n]."""
    torch = _torch()
    if nranks <= 0 or gathered.numel() % nranks:
        raise CurveCrcError(_lib.CC_EINVAL, "gathered size is not a multiple of nranks")
    n = gathered.numel() // nranks
    if out is None:
        with _on_stream(stream):  # created on the stream the kernel writes it on
            out = torch.empty(n, dtype=torch.int32, device=gathered.device)
    with torch.cuda.device(gathered.device):
        check(lib().cc_digest_fold_dev(_dev_ptr(gathered, "gathered"), nranks, n, _dev_ptr(out, "out"),
                                       _stream_handle(stream)), "cc_digest_fold_dev")
    return out


def digest_dev(file_crcs, after_bytes, group, n_groups: int, out=None, stream=None):
    """Per-copyset digest partials: out[group[i]] ^= shift(file_crcs[i], after_bytes[i])."""
    torch = _torch()
    n = file_crcs.numel()
    if after_bytes.numel() != n or group.numel() != n:
        raise CurveCrcError(_lib.CC_EINVAL, "file_crcs / after_bytes / group length mismatch")
    if out is None:
        with _on_stream(stream):  # created on the stream the kernel writes it on
            out = torch.zeros(n_groups, dtype=torch.int32, device=file_crcs.device)
    with torch.cuda.device(file_crcs.device):
        check(lib().cc_digest_dev(_dev_ptr(file_crcs, "file_crcs"), _dev_ptr(after_bytes, "after_bytes"),
                                  _dev_ptr(group, "group"), n, _dev_ptr(out, "out"), _stream_handle(stream)),
              "cc_digest_dev")
    return out


def page_crc_host(data, page_bytes: int = PAGE_SIZE):
    """Host in / host out (blocking): numpy uint8 buffer -> numpy uint32 CRCs."""
    import numpy as np
    a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    if a.nbytes % page_bytes:
        raise CurveCrcError(_lib.CC_EINVAL, "size is not a multiple of page_bytes")
    n = a.nbytes // page_bytes
    out = np.empty(n, dtype=np.uint32)
    check(lib().cc_page_crc_host(ctypes.c_void_p(a.ctypes.data), n, page_bytes,
                                 ctypes.c_void_p(out.ctypes.data)), "cc_page_crc_host")
    return out


def scan_host(chunks, chunk_bytes: int = CHUNK_SIZE, meta_bytes: int = META_PAGE_SIZE,
              page_bytes: int = PAGE_SIZE, slice_bytes: int = SCAN_SIZE, after_bytes=None, group=None,
              n_groups: int = 0):
    """Streaming scan of host-resident chunk files (cc_scan_host / cc_scan_host_digest).
    `chunks`: sequence of (meta, data) numpy uint8 arrays (pinned or pageable, mixed).
    Returns (meta_crcs[n], slice_crcs[n, chunk/slice], file_crcs[n]) as uint32 numpy;
    with after_bytes / group / n_groups also the per-copyset digests [n_groups]
    computed on the device (4th element)."""
    import numpy as np
    n = len(chunks)
    arr = (_lib.CcChunkSrc * max(n, 1))()
    keep = []
    for i, (m, d) in enumerate(chunks):
        m = np.ascontiguousarray(m)
        d = np.ascontiguousarray(d)
        if m.nbytes != meta_bytes or d.nbytes != chunk_bytes:
            raise CurveCrcError(_lib.CC_EINVAL, f"chunk {i}: wrong metapage/data size")
        keep += [m, d]
        arr[i].meta = m.ctypes.data
        arr[i].data = d.ctypes.data
    S = chunk_bytes // slice_bytes
    mc = np.empty(n, dtype=np.uint32)
    sc = np.empty((n, S), dtype=np.uint32)
    fc = np.empty(n, dtype=np.uint32)
    if after_bytes is None:
        check(lib().cc_scan_host(arr, n, chunk_bytes, meta_bytes, page_bytes, slice_bytes,
                                 ctypes.c_void_p(mc.ctypes.data), ctypes.c_void_p(sc.ctypes.data),
                                 ctypes.c_void_p(fc.ctypes.data)), "cc_scan_host")
        return mc, sc, fc
    ab = np.ascontiguousarray(after_bytes, dtype=np.uint64)
    gr = np.ascontiguousarray(group, dtype=np.uint32)
    if ab.size != n or gr.size != n:
        raise CurveCrcError(_lib.CC_EINVAL, "after_bytes / group must hold one entry per chunk")
    dig = np.empty(max(1, n_groups), dtype=np.uint32)
    d = _lib.CcScanDigest(ab.ctypes.data, gr.ctypes.data, n_groups, dig.ctypes.data)
    check(lib().cc_scan_host_digest(arr, n, chunk_bytes, meta_bytes, page_bytes, slice_bytes,
                                    ctypes.c_void_p(mc.ctypes.data), ctypes.c_void_p(sc.ctypes.data),
                                    ctypes.c_void_p(fc.ctypes.data), ctypes.byref(d)), "cc_scan_host_digest")
    return mc, sc, fc, dig[:n_groups]


UPDATE_DTYPE = None


def _update_dtype():
    global UPDATE_DTYPE
    if UPDATE_DTYPE is None:
        import numpy as np
        UPDATE_DTYPE = np.dtype([("dst", "<u8"), ("src", "<u8"), ("len", "<u4"), ("reserved", "<u4")])
    return UPDATE_DTYPE


def log_records(dst_off, src_off, lens):
    """Write log (in write order) as cc_update records (numpy structured array)."""
    import numpy as np
    dst_off = np.asarray(dst_off, dtype=np.uint64)
    rec = np.zeros(dst_off.size, dtype=_update_dtype())
    rec["dst"], rec["src"], rec["len"] = dst_off, np.asarray(src_off, dtype=np.uint64), np.asarray(lens, np.uint32)
    return rec


_log_work = {}


def apply_log(pool, page_crcs, src, d_log, n_updates: int, max_len: int, page_bytes: int = PAGE_SIZE, stream=None,
              delta: bool = False):
    """cc_apply_log_dev: the write log `d_log` (device tensor of n_updates
    cc_update records, WRITE order, overlaps allowed) applied to `pool` with
    later writes winning, and the CRC of every touched page recomputed in
    `page_crcs` -- ordering, apply and rehash all on the device.
    delta=True -> cc_apply_log_delta_dev: `page_crcs` must hold the CRCs of the
    pages before the batch; they are updated by linearity from the touched rows
    only (a stale CRC stays stale instead of being refreshed)."""
    torch = _torch()
    need = int(lib().cc_apply_log_work_bytes(n_updates, max_len, page_bytes))
    if need == 0:
        raise CurveCrcError(_lib.CC_EINVAL, "unsupported log geometry")
    # scratch per (device, stream): calls on different streams may run at the
    # same time (the apply-thread model) and must not share keys / heads
    key = _stream_key(pool.device, stream)
    work = _log_work.get(key)
    if work is None or work.numel() < need:
        with _on_stream(stream):
            work = torch.empty(need, dtype=torch.uint8, device=pool.device)
        _log_work[key] = work
    with torch.cuda.device(pool.device):
        fn = "cc_apply_log_delta_dev" if delta else "cc_apply_log_dev"
        check(getattr(lib(), fn)(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(src, "src"),
                                 _dev_ptr(d_log, "log"), n_updates, max_len, _dev_ptr(page_crcs, "page_crcs"),
                                 _dev_ptr(work, "work"), work.numel(), _stream_handle(stream)), fn)
    if stream is not None:
        work.record_stream(stream)
    return 1


class Cow:
    """The snapshot slots of apply_log_cow (cc_cow, include/curve_crc.h), as
    device tensors for a pool of `n_chunks` chunks of `chunk_bytes`:
      snap_slot int32 [n_chunks]   chunk c's slot, or -1 (CC_NO_SNAPSHOT; the default)
      snap      uint8 [n_slots, chunk_bytes]
      snap_crcs int32 [n_slots, pages_per_chunk]
      bitmap    int32 [n_slots, ceil(pages_per_chunk / 32)]  (a row's bytes are SnapshotMetaPage's bitmap)
      copied, stale int64 [1]      running counts (stale only with verify=True:
                                   the pass then rehashes what it copies)
    `fill` / `crc_fill` initialise snap and snap_crcs (tests use sentinels)."""

    def __init__(self, n_chunks: int, chunk_bytes: int, page_bytes: int = PAGE_SIZE, n_slots: int = 1, device=None,
                 verify: bool = False, fill: int = 0, crc_fill: int = 0):
        torch = _torch()
        if chunk_bytes <= 0 or chunk_bytes % page_bytes:
            raise CurveCrcError(_lib.CC_EINVAL, "chunk_bytes must be a multiple of page_bytes")
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_chunks, self.chunk_bytes, self.page_bytes, self.n_slots = n_chunks, chunk_bytes, page_bytes, n_slots
        self.pages_per_chunk = chunk_bytes // page_bytes
        self.words_per_slot = (self.pages_per_chunk + 31) // 32
        self.snap_slot = torch.full((n_chunks,), -1, dtype=torch.int32, device=dev)
        self.snap = torch.full((n_slots, chunk_bytes), fill, dtype=torch.uint8, device=dev)
        self.snap_crcs = torch.full((n_slots, self.pages_per_chunk), crc_fill, dtype=torch.int32, device=dev)
        self.bitmap = torch.zeros((n_slots, self.words_per_slot), dtype=torch.int32, device=dev)
        self.copied = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stale = torch.zeros(1, dtype=torch.int64, device=dev) if verify else None

    def struct(self) -> "_lib.CcCow":
        c = _lib.CcCow()
        c.chunk_bytes, c.n_slots = self.chunk_bytes, self.n_slots
        c.d_snap_slot = _dev_ptr(self.snap_slot, "snap_slot")
        c.d_snap = _dev_ptr(self.snap, "snap")
        c.d_snap_crcs = _dev_ptr(self.snap_crcs, "snap_crcs")
        c.d_snap_bitmap = _dev_ptr(self.bitmap, "bitmap")
        c.d_copied = _dev_ptr(self.copied, "copied")
        c.d_stale = _dev_ptr(self.stale, "stale") if self.stale is not None else None
        return c

    def slot_bitmap_bytes(self, slot: int) -> bytes:
        """Slot `slot`'s bitmap as SnapshotMetaPage holds it (snap_meta_encode's `bitmap`)."""
        return self.bitmap[slot].cpu().numpy().tobytes()[:(self.pages_per_chunk + 7) // 8]


def apply_log_cow(pool, page_crcs, src, d_log, n_updates: int, max_len: int, cow: Optional[Cow],
                  page_bytes: int = PAGE_SIZE, stream=None, delta: bool = False):
    """cc_apply_log_cow_dev: apply_log (delta or not) for chunks with an open
    snapshot -- before the writes land, every touched page whose chunk has a
    slot in `cow` and whose bit in the slot's bitmap is clear is copied into the
    slot with its stored CRC (page_crcs must hold the CRCs before the batch) and
    its bit set.  cow=None is apply_log."""
    torch = _torch()
    need = int(lib().cc_apply_log_work_bytes(n_updates, max_len, page_bytes))
    if need == 0:
        raise CurveCrcError(_lib.CC_EINVAL, "unsupported log geometry")
    key = _stream_key(pool.device, stream)
    work = _log_work.get(key)
    if work is None or work.numel() < need:
        with _on_stream(stream):
            work = torch.empty(need, dtype=torch.uint8, device=pool.device)
        _log_work[key] = work
    cs = cow.struct() if cow is not None else None
    with torch.cuda.device(pool.device):
        check(lib().cc_apply_log_cow_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(src, "src"),
                                         _dev_ptr(d_log, "log"), n_updates, max_len,
                                         _dev_ptr(page_crcs, "page_crcs"), _dev_ptr(work, "work"), work.numel(),
                                         _stream_handle(stream), 1 if delta else 0,
                                         ctypes.byref(cs) if cs is not None else None), "cc_apply_log_cow_dev")
    if stream is not None:
        work.record_stream(stream)
        if cow is not None:
            for t in (cow.snap_slot, cow.snap, cow.snap_crcs, cow.bitmap, cow.copied, cow.stale):
                if t is not None:
                    t.record_stream(stream)
    return 1


def snap_meta_encode(sn: int, bitmap: bytes, bits: int, page_bytes: int = META_PAGE_SIZE,
                     damaged: bool = False) -> bytes:
    """cc_snap_meta_encode: the snapshot file's metapage (SnapshotMetaPage::encode)
    for `bits` blocks whose bitmap bytes are `bitmap` (Cow.slot_bitmap_bytes)."""
    bitmap = bytes(bitmap)
    if len(bitmap) < (bits + 7) // 8:
        raise CurveCrcError(_lib.CC_EINVAL, "bitmap shorter than bits")
    out = ctypes.create_string_buffer(page_bytes)
    check(lib().cc_snap_meta_encode(sn, 1 if damaged else 0, bits, bitmap, out, page_bytes), "cc_snap_meta_encode")
    return out.raw


def snap_meta_decode(buf: bytes):
    """cc_snap_meta_decode -> (sn, damaged, bits, bitmap bytes); CurveCrcError
    (CC_ECORRUPT) for a bad CRC, version or length."""
    buf = bytes(buf)
    sn, damaged, bits = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_uint32()
    bm = ctypes.create_string_buffer(max(len(buf), 1))
    check(lib().cc_snap_meta_decode(buf, len(buf), ctypes.byref(sn), ctypes.byref(damaged), ctypes.byref(bits), bm,
                                    len(buf)), "cc_snap_meta_decode")
    return int(sn.value), bool(damaged.value), int(bits.value), bm.raw[:(bits.value + 7) // 8]


def read_pages_list(offs, lens, page_bytes: int = PAGE_SIZE):
    """Diagnostic helper (host): the pages a batch of reads touches, read after
    read -- the list cc_page_list_probe_dev walks (int64 page indices; an empty
    read adds none)."""
    import numpy as np
    offs = np.asarray(offs, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    keep = lens > 0
    p0 = offs[keep] // page_bytes
    cnt = (offs[keep] + lens[keep] - 1) // page_bytes - p0 + 1
    start = np.repeat(p0 - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt)
    return start + np.arange(int(cnt.sum()), dtype=np.int64)


def page_list_probe(pool, d_pages, n: int, out, stream=None):
    """cc_page_list_probe_dev (diagnostic): the read traffic of a page list alone
    -- the ceiling of verify-on-read's access pattern.  `out` gets a word per page."""
    torch = _torch()
    with torch.cuda.device(pool.device):
        check(lib().cc_page_list_probe_dev(_dev_ptr(pool, "pool"), _nbytes(pool), _dev_ptr(d_pages, "pages"), n,
                                           _dev_ptr(out, "out"), _stream_handle(stream)), "cc_page_list_probe_dev")


def apply_logs(pool, page_crcs, batches, max_len: int, page_bytes: int = PAGE_SIZE, stream=None,
               delta: bool = False, cow: Optional["Cow"] = None, clone: Optional["Clone"] = None):
    """cc_apply_logs_dev: a QUEUE of write logs applied in order -- the same
    pool bytes and page CRCs as one apply_log call per batch, pipelined (each
    batch's page kernel also groups the next batch's pieces).  `batches`: a
    list of (src, d_log, n_updates) -- device tensors as for apply_log.
    With `cow` and/or `clone` it is cc_apply_logs_cow_dev: one pass before the
    queue leaves the snapshot slots and the clone bitmaps as apply_log_cow +
    clone_mark per batch would (page_crcs must hold the CRCs before the queue)."""
    import ctypes
    torch = _torch()
    if not batches:
        return 0
    n_max = max(int(n) for _, _, n in batches)
    need = int(lib().cc_apply_logs_work_bytes(max(n_max, 1), max_len, page_bytes))
    if need == 0:
        raise CurveCrcError(_lib.CC_EINVAL, "unsupported log geometry")
    key = ("logs",) + tuple(_stream_key(pool.device, stream))
    work = _log_work.get(key)
    if work is None or work.numel() < need:
        with _on_stream(stream):
            work = torch.empty(need, dtype=torch.uint8, device=pool.device)
        _log_work[key] = work
    arr = (_lib.CcLogBatch * len(batches))()
    for i, (src, d_log, n) in enumerate(batches):
        arr[i].d_src = _dev_ptr(src, "src").value if int(n) else None
        arr[i].d_log = _dev_ptr(d_log, "log").value if int(n) else None
        arr[i].n_updates = int(n)
    with torch.cuda.device(pool.device):
        if cow is None and clone is None:
            check(lib().cc_apply_logs_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes,
                                          ctypes.cast(arr, ctypes.c_void_p), len(batches), max_len,
                                          _dev_ptr(page_crcs, "page_crcs"), 1 if delta else 0, _dev_ptr(work, "work"),
                                          work.numel(), _stream_handle(stream)), "cc_apply_logs_dev")
        else:
            ws = cow.struct() if cow is not None else None
            ls = clone.struct() if clone is not None else None
            check(lib().cc_apply_logs_cow_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes,
                                              ctypes.cast(arr, ctypes.c_void_p), len(batches), max_len,
                                              _dev_ptr(page_crcs, "page_crcs"), 1 if delta else 0,
                                              _dev_ptr(work, "work"), work.numel(), _stream_handle(stream),
                                              ctypes.byref(ws) if ws is not None else None,
                                              ctypes.byref(ls) if ls is not None else None), "cc_apply_logs_cow_dev")
    if stream is not None:
        work.record_stream(stream)
        if cow is not None:
            _record_cow(cow, stream)
            for t in (cow.copied, cow.stale):
                if t is not None:
                    t.record_stream(stream)
        if clone is not None:
            _record_clone(clone, stream)
    return 1


def apply_updates(pool, page_crcs, src, dst_off, src_off, lens, page_bytes: int = PAGE_SIZE, stream=None,
                  delta: bool = False):
    """Client partial-write path: host-side write log -> device (one copy of the
    records) -> cc_apply_log_dev (cc_apply_log_delta_dev with delta=True).
    Returns the number of device calls (1)."""
    import numpy as np
    torch = _torch()
    lens = np.asarray(lens, dtype=np.uint32)
    dst_off = np.asarray(dst_off, dtype=np.uint64)
    src_off = np.asarray(src_off, dtype=np.uint64)
    if not (dst_off.size == src_off.size == lens.size):
        raise CurveCrcError(_lib.CC_EINVAL, "dst/src/len size mismatch")
    if lens.size == 0:
        return 0
    if (lens == 0).any() or (dst_off + lens > _nbytes(pool)).any() or (src_off + lens > _nbytes(src)).any():
        raise CurveCrcError(_lib.CC_EINVAL, "update out of range or empty")
    rec = log_records(dst_off, src_off, lens)
    with _on_stream(stream):
        d_log = torch.from_numpy(rec.view(np.uint8)).to(pool.device)
    n = apply_log(pool, page_crcs, src, d_log, rec.size, int(lens.max()), page_bytes, stream, delta)
    if stream is not None:
        d_log.record_stream(stream)
    return n


def log_probe_descs(dst_off, src_off, lens, page_bytes: int = PAGE_SIZE):
    """Descriptors of cc_apply_log_probe_dev (the write log's page traffic
    alone) for one write log, built on the host: one per touched page, in the
    order of the first write touching it (the page pass's head order).  A page
    with ONE piece reads the rows that piece covers whole from the source (as
    cc_apply_log_dev does) and the rest from the page; every page stores back
    the rows its pieces touch.  Diagnostic: not part of the write path."""
    import numpy as np
    if page_bytes != 4096:
        raise CurveCrcError(_lib.CC_EINVAL, "the probe is built for 4 KiB pages")
    dst = np.asarray(dst_off, dtype=np.uint64)
    src = np.asarray(src_off, dtype=np.uint64)
    ln = np.asarray(lens, dtype=np.uint64)
    pb = np.uint64(page_bytes)
    p0, p1 = dst // pb, (dst + ln - np.uint64(1)) // pb
    span = int((p1 - p0).max()) + 1 if dst.size else 0
    pg, upd = [], []
    for k in range(span):  # piece k of every write that reaches its k-th page
        m = p0 + np.uint64(k) <= p1
        pg.append(p0[m] + np.uint64(k))
        upd.append(np.nonzero(m)[0])
    pg, upd = np.concatenate(pg), np.concatenate(upd)
    pbase = pg * pb
    rlo = (np.maximum(dst[upd], pbase) - pbase).astype(np.int64)
    rhi = (np.minimum(dst[upd] + ln[upd], pbase + pb) - pbase).astype(np.int64)
    r0, r1 = rlo >> 8, (rhi - 1) >> 8
    dirty = ((np.int64(2) << r1) - 1) & ~((np.int64(1) << r0) - 1)
    f0, f1 = (rlo + 255) >> 8, rhi >> 8
    cov = np.where(f1 > f0, ((np.int64(1) << f1) - 1) & ~((np.int64(1) << f0) - 1), 0)
    soff = src[upd] - dst[upd] + pbase  # modular, as cc_apply_log_dev's per-piece source pointer
    order = np.lexsort((upd, pg))  # pieces grouped by page, log order inside
    pg, upd, dirty, cov, soff = pg[order], upd[order], dirty[order], cov[order], soff[order]
    starts = np.flatnonzero(np.r_[True, pg[1:] != pg[:-1]])
    counts = np.diff(np.r_[starts, pg.size])
    out = np.zeros(starts.size, dtype=[("page", "<u8"), ("src_off", "<u8"), ("covered", "<u4"), ("dirty", "<u4")])
    out["page"] = pg[starts]
    out["dirty"] = np.bitwise_or.reduceat(dirty, starts).astype(np.uint32)
    single = counts == 1
    out["covered"] = np.where(single, cov[starts], 0).astype(np.uint32)
    out["src_off"] = np.where(single, soff[starts], 0)
    return out[np.argsort(upd[starts], kind="stable")]  # head order: by the first write touching the page


def log_probe(pool, src, d_desc, n: int, out, stream=None):
    """cc_apply_log_probe_dev over `n` descriptors resident on the device."""
    with _torch().cuda.device(pool.device):
        check(lib().cc_apply_log_probe_dev(_dev_ptr(pool, "pool"), _nbytes(pool), _dev_ptr(src, "src"),
                                           _dev_ptr(d_desc, "desc"), n, _dev_ptr(out, "out"),
                                           _stream_handle(stream)), "cc_apply_log_probe_dev")


_reads_work = {}


def verify_read_records(pool, page_crcs, d_reads, n_reads: int, bad, total, page_bytes: int = PAGE_SIZE,
                        stream=None):
    """cc_verify_reads_dev on a batch already resident on the device: `d_reads`
    = int64 device tensor of n_reads (offset, length) pairs; mismatches are
    ADDED to `bad` (int32 [n_reads], -1 marks a read past the pool) and
    `total` (int64 [1]).  Work buffer cached per (device, stream).  No host sync."""
    torch = _torch()
    need = int(lib().cc_verify_reads_work_bytes(n_reads))
    if need == 0:
        raise CurveCrcError(_lib.CC_EINVAL, "unsupported read batch")
    key = _stream_key(pool.device, stream)
    work = _reads_work.get(key)
    if work is None or work.numel() < need:
        with _on_stream(stream):
            work = torch.empty(need, dtype=torch.uint8, device=pool.device)
        _reads_work[key] = work
    with torch.cuda.device(pool.device):
        check(lib().cc_verify_reads_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(d_reads, "reads"),
                                        n_reads, _dev_ptr(page_crcs, "page_crcs"), _dev_ptr(bad, "bad"),
                                        _dev_ptr(total, "total"), _dev_ptr(work, "work"), work.numel(),
                                        _stream_handle(stream)), "cc_verify_reads_dev")
    if stream is not None:
        work.record_stream(stream)


def verify_reads(pool, page_crcs, offsets, lengths, page_bytes: int = PAGE_SIZE, stream=None):
    """cc_verify_reads_dev: verify-on-read for a batch of reads of the pool.
    Returns (bad pages per read: int32 device tensor, -1 = read past the pool;
    total bad pages: int64 device tensor [1]).  No host sync."""
    import numpy as np
    torch = _torch()
    off = np.asarray(offsets, dtype=np.uint64)
    ln = np.asarray(lengths, dtype=np.uint64)
    if off.size != ln.size:
        raise CurveCrcError(_lib.CC_EINVAL, "offsets/lengths size mismatch")
    n = off.size
    with _on_stream(stream):
        bad = torch.zeros(max(n, 1), dtype=torch.int32, device=pool.device)
        total = torch.zeros(1, dtype=torch.int64, device=pool.device)
        if n == 0:
            return bad[:0], total
        rng = torch.from_numpy(np.stack([off, ln], axis=1).reshape(-1).view(np.int64)).to(pool.device)
        need = int(lib().cc_verify_reads_work_bytes(n))
        work = torch.empty(need, dtype=torch.uint8, device=pool.device)
    with torch.cuda.device(pool.device):
        check(lib().cc_verify_reads_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(rng, "reads"), n,
                                        _dev_ptr(page_crcs, "page_crcs"), _dev_ptr(bad, "bad"),
                                        _dev_ptr(total, "total"), _dev_ptr(work, "work"), need,
                                        _stream_handle(stream)), "cc_verify_reads_dev")
    if stream is not None:
        for t in (rng, work):
            t.record_stream(stream)
    return bad, total


def _record_cow(cow, stream):
    for t in (cow.snap_slot, cow.snap, cow.snap_crcs, cow.bitmap):
        t.record_stream(stream)


def read_snap_records(pool, page_crcs, d_reads, n_reads: int, cow: Optional[Cow], bad, total, out=None, out_off=None,
                      page_bytes: int = PAGE_SIZE, stream=None):
    """cc_read_snap_dev on a batch already resident on the device: `d_reads` =
    int64 device tensor of n_reads page-aligned (offset, length) pairs, read
    through the snapshot view of `cow` (None: the live pool).  Every page is
    rehashed against the CRC of its source; mismatches are ADDED to `bad`
    (int32 [n_reads], -1 marks an invalid read) and `total` (int64 [1]).  With
    `out` (uint8 device tensor) and `out_off` (int64 [n_reads]) read i's bytes
    land at out[out_off[i]:]; out=None verifies only.  No host sync."""
    torch = _torch()
    cs = cow.struct() if cow is not None else None
    with torch.cuda.device(pool.device):
        check(lib().cc_read_snap_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(d_reads, "reads"),
                                     n_reads, _dev_ptr(page_crcs, "page_crcs"),
                                     ctypes.byref(cs) if cs is not None else None,
                                     _dev_ptr(out, "out") if out is not None else None,
                                     _dev_ptr(out_off, "out_off") if out_off is not None else None,
                                     _nbytes(out) if out is not None else 0, _dev_ptr(bad, "bad"),
                                     _dev_ptr(total, "total"), _stream_handle(stream)), "cc_read_snap_dev")
    if stream is not None and cow is not None:
        _record_cow(cow, stream)


def read_snap(pool, page_crcs, offsets, lengths, cow: Optional[Cow], page_bytes: int = PAGE_SIZE, stream=None,
              copy: bool = True):
    """cc_read_snap_dev: the page-aligned reads (offsets, lengths) of the pool
    as its chunks were when their snapshots in `cow` were taken (cow=None: as
    they are), every page verified against the CRC of the table it came from.
    Returns (out, bad_per_read, bad_total): `out` holds the reads' bytes back to
    back in read order (uint8 device tensor; None with copy=False), the counts
    are as verify_reads returns them (-1 = invalid read).  No host sync."""
    import numpy as np
    torch = _torch()
    off = np.asarray(offsets, dtype=np.uint64)
    ln = np.asarray(lengths, dtype=np.uint64)
    if off.size != ln.size:
        raise CurveCrcError(_lib.CC_EINVAL, "offsets/lengths size mismatch")
    n = off.size
    with _on_stream(stream):
        bad = torch.zeros(max(n, 1), dtype=torch.int32, device=pool.device)
        total = torch.zeros(1, dtype=torch.int64, device=pool.device)
        out = out_off = None
        if copy:
            ends = np.cumsum(ln, dtype=np.uint64)
            out = torch.empty(int(ends[-1]) if n else 0, dtype=torch.uint8, device=pool.device)
            out_off = torch.from_numpy((ends - ln).view(np.int64)).to(pool.device)
        if n == 0:
            return out, bad[:0], total
        rng = torch.from_numpy(np.stack([off, ln], axis=1).reshape(-1).view(np.int64)).to(pool.device)
    buf = out
    if copy and out.numel() == 0:  # nothing but empty reads: a buffer nobody writes keeps the pointer non-NULL
        with _on_stream(stream):
            buf = torch.empty(4, dtype=torch.uint8, device=pool.device)
    read_snap_records(pool, page_crcs, rng, n, cow, bad, total, out=buf, out_off=out_off, page_bytes=page_bytes,
                      stream=stream)
    if stream is not None:
        for t in (rng, buf, out_off):
            if t is not None:
                t.record_stream(stream)
    return out, bad[:n], total


class Clone:
    """The written-page bitmaps of a pool's clone chunks (cc_clone,
    include/curve_crc.h), as device tensors for a pool of `n_chunks` chunks of
    `chunk_bytes`:
      clone_slot int32 [n_chunks]   chunk c's bitmap slot, or -1 (CC_NOT_CLONE; the default)
      bitmap     int32 [n_slots, ceil(pages_per_chunk / 32)]  (a row's bytes are ChunkFileMetaPage's bitmap)
      claim      int32 [n_slots, pages_per_chunk]  paste's scratch: -1 everywhere between calls
      pasted     int64 [1]          running count of pasted pages"""

    def __init__(self, n_chunks: int, chunk_bytes: int, page_bytes: int = PAGE_SIZE, n_slots: int = 1, device=None):
        torch = _torch()
        if chunk_bytes <= 0 or chunk_bytes % page_bytes:
            raise CurveCrcError(_lib.CC_EINVAL, "chunk_bytes must be a multiple of page_bytes")
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_chunks, self.chunk_bytes, self.page_bytes, self.n_slots = n_chunks, chunk_bytes, page_bytes, n_slots
        self.pages_per_chunk = chunk_bytes // page_bytes
        self.words_per_slot = (self.pages_per_chunk + 31) // 32
        self.clone_slot = torch.full((n_chunks,), -1, dtype=torch.int32, device=dev)
        self.bitmap = torch.zeros((n_slots, self.words_per_slot), dtype=torch.int32, device=dev)
        self.claim = torch.full((n_slots, self.pages_per_chunk), -1, dtype=torch.int32, device=dev)
        self.pasted = torch.zeros(1, dtype=torch.int64, device=dev)

    def struct(self) -> "_lib.CcClone":
        c = _lib.CcClone()
        c.chunk_bytes, c.n_slots = self.chunk_bytes, self.n_slots
        c.d_clone_slot = _dev_ptr(self.clone_slot, "clone_slot")
        c.d_bitmap = _dev_ptr(self.bitmap, "bitmap")
        c.d_claim = _dev_ptr(self.claim, "claim")
        c.d_pasted = _dev_ptr(self.pasted, "pasted")
        return c

    def slot_bitmap_bytes(self, slot: int) -> bytes:
        """Slot `slot`'s bitmap as ChunkFileMetaPage holds it (chunkfile.clone_metapage_after's `bitmap`)."""
        return self.bitmap[slot].cpu().numpy().tobytes()[:(self.pages_per_chunk + 7) // 8]


def _record_clone(clone, stream):
    for t in (clone.clone_slot, clone.bitmap, clone.claim, clone.pasted):
        t.record_stream(stream)


def paste_records(pool, page_crcs, src, d_pastes, n: int, clone: Clone, pasted_per_entry, page_bytes: int = PAGE_SIZE,
                  stream=None):
    """cc_paste_dev on a batch already resident on the device: `d_pastes` =
    device tensor of n cc_update records (log_records), an ORDERED batch of
    Paste requests.  A page of a clone chunk whose bit in `clone` is clear is
    written once, from the lowest-indexed valid entry covering it, its bit set
    and its CRC recomputed in `page_crcs`; every other page keeps bytes and CRC.
    The pages entry i pasted are ADDED to pasted_per_entry[i] (int32 [n], -1
    marks an invalid entry), all of them to clone.pasted.  No host sync."""
    torch = _torch()
    cs = clone.struct()
    with torch.cuda.device(pool.device):
        check(lib().cc_paste_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(src, "src"),
                                 _nbytes(src), _dev_ptr(d_pastes, "pastes"), n, _dev_ptr(page_crcs, "page_crcs"),
                                 ctypes.byref(cs), _dev_ptr(pasted_per_entry, "pasted_per_entry"),
                                 _stream_handle(stream)), "cc_paste_dev")
    if stream is not None:
        _record_clone(clone, stream)


def paste(pool, page_crcs, src, dst_off, src_off, lens, clone: Clone, page_bytes: int = PAGE_SIZE, stream=None):
    """cc_paste_dev: the Paste requests (dst_off, src_off, lens), in order, from
    the device tensor `src` into `pool`.  Returns the pages each entry pasted
    (int32 device tensor, -1 = invalid entry); clone.pasted keeps the running
    total.  No host sync."""
    import numpy as np
    torch = _torch()
    rec = log_records(dst_off, src_off, lens)
    n = rec.size
    with _on_stream(stream):
        per_entry = torch.zeros(max(n, 1), dtype=torch.int32, device=pool.device)
        if n == 0:
            return per_entry[:0]
        d_pastes = torch.from_numpy(rec.view(np.uint8)).to(pool.device)
    paste_records(pool, page_crcs, src, d_pastes, n, clone, per_entry, page_bytes=page_bytes, stream=stream)
    if stream is not None:
        for t in (d_pastes, per_entry):
            t.record_stream(stream)
    return per_entry[:n]


def clone_mark(pool, d_log, n_updates: int, max_len: int, clone: Clone, page_bytes: int = PAGE_SIZE, stream=None):
    """cc_clone_mark_dev: after apply_log* of the same log on the same stream,
    set the bit of every page of a clone chunk that a valid entry covered whole
    (flush() after Write).  A partly covered page keeps its bit."""
    torch = _torch()
    cs = clone.struct()
    with torch.cuda.device(pool.device):
        check(lib().cc_clone_mark_dev(_nbytes(pool), page_bytes, _dev_ptr(d_log, "log"), n_updates, max_len,
                                      ctypes.byref(cs), _stream_handle(stream)), "cc_clone_mark_dev")
    if stream is not None:
        _record_clone(clone, stream)


def apply_ops(pool, page_crcs, ops, max_len: int, max_paste_len: int, page_bytes: int = PAGE_SIZE, stream=None,
              delta: bool = False, cow: Optional["Cow"] = None, clone: Optional[Clone] = None, contested=None):
    """cc_apply_ops_dev: a queue of write logs AND paste batches, in log order,
    as one call -- a chunkserver's apply loop.  `ops`: a list of
    ("write", src, d_log, n) and ("paste", origin, d_pastes, n) items (device
    tensors; d_log / d_pastes hold cc_update records, log_records).  Every page
    whose first setter in the queue is a paste entry is pasted before the
    queue's first write; then the write batches run as apply_logs(cow=, clone=)
    runs them.  The result equals apply_log_cow + clone_mark / paste per batch
    bit for bit unless an unaligned write precedes a paste of the same page;
    such pairs are ADDED to `contested` (int64 [1] device tensor, optional).
    Returns the per-paste-batch count tensors (int32 [n], -1 = invalid entry),
    in queue order.  Without a paste item this is apply_logs.  No host sync."""
    import ctypes
    torch = _torch()
    kinds = {"write": _lib.CC_OP_WRITE, "paste": _lib.CC_OP_PASTE}
    for item in ops:
        if item[0] not in kinds:
            raise CurveCrcError(_lib.CC_EINVAL, f"unknown op kind {item[0]!r}")
    if not any(kind == "paste" for kind, _, _, _ in ops):
        apply_logs(pool, page_crcs, [(src, d_log, n) for _, src, d_log, n in ops], max_len, page_bytes, stream=stream,
                   delta=delta, cow=cow, clone=clone)
        return []
    n_max = max([int(n) for kind, _, _, n in ops if kind == "write"] + [1])
    need = int(lib().cc_apply_logs_work_bytes(n_max, max(max_len, 1), page_bytes))
    if need == 0:
        raise CurveCrcError(_lib.CC_EINVAL, "unsupported log geometry")
    key = ("logs",) + tuple(_stream_key(pool.device, stream))
    work = _log_work.get(key)
    if work is None or work.numel() < need:
        with _on_stream(stream):
            work = torch.empty(need, dtype=torch.uint8, device=pool.device)
        _log_work[key] = work
    arr = (_lib.CcOpBatch * len(ops))()
    counts = []
    for i, (kind, src, d_recs, n) in enumerate(ops):
        arr[i].kind = kinds[kind]
        arr[i].n = int(n)
        if not int(n) and kind == "write":
            continue
        if int(n):
            arr[i].d_src = _dev_ptr(src, "src").value
            arr[i].d_recs = _dev_ptr(d_recs, "records").value
        if kind == "paste":
            with _on_stream(stream):
                per = torch.zeros(max(int(n), 1), dtype=torch.int32, device=pool.device)
            counts.append(per[:int(n)])
            if int(n):
                arr[i].src_bytes = _nbytes(src)
                arr[i].d_pasted_per_entry = _dev_ptr(per, "pasted_per_entry").value
    ws = cow.struct() if cow is not None else None
    ls = clone.struct() if clone is not None else None
    with torch.cuda.device(pool.device):
        check(lib().cc_apply_ops_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, ctypes.cast(arr, ctypes.c_void_p),
                                     len(ops), max_len, max_paste_len, _dev_ptr(page_crcs, "page_crcs"),
                                     1 if delta else 0, _dev_ptr(work, "work"), work.numel(), _stream_handle(stream),
                                     ctypes.byref(ws) if ws is not None else None,
                                     ctypes.byref(ls) if ls is not None else None,
                                     _dev_ptr(contested, "contested") if contested is not None else None),
              "cc_apply_ops_dev")
    if stream is not None:
        work.record_stream(stream)
        for t in counts:
            t.record_stream(stream)
        if contested is not None:
            contested.record_stream(stream)
        if cow is not None:
            _record_cow(cow, stream)
            for t in (cow.copied, cow.stale):
                if t is not None:
                    t.record_stream(stream)
        if clone is not None:
            _record_clone(clone, stream)
    return counts


def clone_check_reads(pool, offsets, lengths, clone: Clone, page_bytes: int = PAGE_SIZE, stream=None):
    """cc_clone_check_reads_dev: for the reads (offsets, lengths; any
    alignment) of the pool, how many of the pages each touches lie in a clone
    chunk and were never written.  Returns (unwritten_per_read int32 device
    tensor, -1 = read past the pool; unwritten_total int64 [1]).  A read with
    count 0 may be served (verify_reads / read_snap); any other needs its
    origin fetched and pasted first.  No host sync."""
    import numpy as np
    torch = _torch()
    off = np.asarray(offsets, dtype=np.uint64)
    ln = np.asarray(lengths, dtype=np.uint64)
    if off.size != ln.size:
        raise CurveCrcError(_lib.CC_EINVAL, "offsets/lengths size mismatch")
    n = off.size
    with _on_stream(stream):
        unwritten = torch.zeros(max(n, 1), dtype=torch.int32, device=pool.device)
        total = torch.zeros(1, dtype=torch.int64, device=pool.device)
        if n == 0:
            return unwritten[:0], total
        rng = torch.from_numpy(np.stack([off, ln], axis=1).reshape(-1).view(np.int64)).to(pool.device)
    cs = clone.struct()
    with torch.cuda.device(pool.device):
        check(lib().cc_clone_check_reads_dev(_nbytes(pool), page_bytes, _dev_ptr(rng, "reads"), n, ctypes.byref(cs),
                                             _dev_ptr(unwritten, "unwritten"), _dev_ptr(total, "total"),
                                             _stream_handle(stream)), "cc_clone_check_reads_dev")
    if stream is not None:
        _record_clone(clone, stream)
        for t in (rng, unwritten, total):
            t.record_stream(stream)
    return unwritten[:n], total


NO_ORIGIN = _lib.CC_NO_ORIGIN  # origin_off of a read that has no origin buffer


def read_merge_records(pool, page_crcs, d_reads, n_reads: int, clone: Clone, out, out_off, bad, total, unwritten,
                       unwritten_total, origin=None, origin_off=None, page_bytes: int = PAGE_SIZE, stream=None):
    """cc_read_merge_dev on a batch already resident on the device: `d_reads` =
    int64 device tensor of n_reads page-aligned (offset, length) pairs.  A
    written page (no clone chunk, or its bit in `clone` set) is rehashed against
    `page_crcs` and stored at out[out_off[i] + its position in read i]; a
    never-written page comes from origin[origin_off[i] + the same position],
    unhashed, or -- with origin=None or origin_off[i] = NO_ORIGIN -- leaves its
    output bytes alone.  Mismatches are ADDED to `bad` / `total`, never-written
    pages to `unwritten` / `unwritten_total` (int32 [n_reads] and int64 [1]
    each; -1 in both per-read words marks an invalid read).  `out` uint8,
    `out_off` / `origin_off` int64 [n_reads] device tensors.  Reads the bitmaps
    only.  No host sync."""
    torch = _torch()
    if origin is not None and origin_off is None:
        raise CurveCrcError(_lib.CC_EINVAL, "origin needs origin_off")
    cs = clone.struct()
    with torch.cuda.device(pool.device):
        check(lib().cc_read_merge_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(d_reads, "reads"),
                                      n_reads, _dev_ptr(page_crcs, "page_crcs"), ctypes.byref(cs),
                                      _dev_ptr(origin, "origin") if origin is not None else None,
                                      _dev_ptr(origin_off, "origin_off") if origin is not None else None,
                                      _nbytes(origin) if origin is not None else 0, _dev_ptr(out, "out"),
                                      _dev_ptr(out_off, "out_off"), _nbytes(out), _dev_ptr(bad, "bad"),
                                      _dev_ptr(total, "total"), _dev_ptr(unwritten, "unwritten"),
                                      _dev_ptr(unwritten_total, "unwritten_total"), _stream_handle(stream)),
              "cc_read_merge_dev")
    if stream is not None:
        _record_clone(clone, stream)


def read_merge(pool, page_crcs, offsets, lengths, clone: Clone, origin=None, origin_off=None,
               page_bytes: int = PAGE_SIZE, stream=None):
    """cc_read_merge_dev: the page-aligned reads (offsets, lengths) of a pool
    with clone chunks, each answered from the written pages of the pool
    (verified) and the never-written pages of its origin buffer: read i's
    origin bytes start at origin[origin_off[i]] (`origin` a uint8 device
    tensor, `origin_off` host integers, NO_ORIGIN = none).  Returns (out,
    out_off, bad_per_read, bad_total, unwritten_per_read, unwritten_total):
    `out` holds the reads' bytes back to back at `out_off` (int64 device
    tensor); a never-written page with no origin leaves zeros there and shows
    in the unwritten counts (PageNerverWrittenError).  Counts as read_snap's,
    -1 in both = invalid read.  No host sync."""
    import numpy as np
    torch = _torch()
    off = np.asarray(offsets, dtype=np.uint64)
    ln = np.asarray(lengths, dtype=np.uint64)
    if off.size != ln.size:
        raise CurveCrcError(_lib.CC_EINVAL, "offsets/lengths size mismatch")
    n = off.size
    d_ooff = None
    if origin is not None:
        if origin_off is None:
            raise CurveCrcError(_lib.CC_EINVAL, "origin needs origin_off")
        o_off = np.asarray(origin_off, dtype=np.uint64)
        if o_off.size != n:
            raise CurveCrcError(_lib.CC_EINVAL, "origin_off size mismatch")
    with _on_stream(stream):
        bad = torch.zeros(max(n, 1), dtype=torch.int32, device=pool.device)
        total = torch.zeros(1, dtype=torch.int64, device=pool.device)
        unwritten = torch.zeros(max(n, 1), dtype=torch.int32, device=pool.device)
        unwritten_total = torch.zeros(1, dtype=torch.int64, device=pool.device)
        ends = np.cumsum(ln, dtype=np.uint64)
        out = torch.zeros(int(ends[-1]) if n else 0, dtype=torch.uint8, device=pool.device)
        out_off = torch.from_numpy((ends - ln).view(np.int64)).to(pool.device)
        if n == 0:
            return out, out_off, bad[:0], total, unwritten[:0], unwritten_total
        rng = torch.from_numpy(np.stack([off, ln], axis=1).reshape(-1).view(np.int64)).to(pool.device)
        if origin is not None:
            d_ooff = torch.from_numpy(o_off.view(np.int64)).to(pool.device)
        buf = out if out.numel() else torch.empty(4, dtype=torch.uint8, device=pool.device)  # never a NULL output
    read_merge_records(pool, page_crcs, rng, n, clone, buf, out_off, bad, total, unwritten, unwritten_total,
                       origin=origin, origin_off=d_ooff, page_bytes=page_bytes, stream=stream)
    if stream is not None:
        for t in (rng, buf, out_off, d_ooff, origin, bad, total, unwritten, unwritten_total):
            if t is not None:
                t.record_stream(stream)
    return out, out_off, bad[:n], total, unwritten[:n], unwritten_total


def _paste_fetched(pool, page_crcs, origin, dst_off, src_off, lens, clone, page_bytes, stream):
    """clone_read's PasteCloneData step (inside clone_read the name `paste` is its enablePaste_ argument)."""
    return paste(pool, page_crcs, origin, dst_off, src_off, lens, clone, page_bytes=page_bytes, stream=stream)


def clone_read(pool, page_crcs, offsets, lengths, clone: Clone, fetch, paste: bool = True,
               page_bytes: int = PAGE_SIZE, stream=None):
    """CloneCore::HandleReadRequest for a batch (clone_core.cpp:165-194):
    clone_check_reads; `fetch(indices)` ONCE for the reads that touch a
    never-written page (numpy indices into the batch, ascending) -- the control
    plane's download: it returns (origin uint8 device tensor, origin_off: one
    byte offset per index); read_merge for all reads; and with paste=True
    (enablePaste_) the fetched buffers are pasted over the same ranges
    (PasteCloneData).  When no read needs its origin, fetch is not called and
    nothing is pasted.  A read whose offset or length is no multiple of
    page_bytes is never fetched or pasted (CloneReadByLocalInfo refuses it
    before any download): read_merge marks it invalid.  Returns read_merge's
    tuple.  One host sync, on `stream`: the check's counts choose what to
    fetch."""
    import numpy as np
    off = np.asarray(offsets, dtype=np.uint64)
    ln = np.asarray(lengths, dtype=np.uint64)
    if off.size != ln.size:
        raise CurveCrcError(_lib.CC_EINVAL, "offsets/lengths size mismatch")
    counts, _ = clone_check_reads(pool, off, ln, clone, page_bytes=page_bytes, stream=stream)
    if stream is not None:
        stream.synchronize()  # the counts were made on `stream`; the copy below runs on the current one
    counts = counts.cpu().numpy()
    aligned = ((off | ln) & np.uint64(page_bytes - 1)) == 0
    need = np.nonzero((counts > 0) & aligned)[0]  # -1 (past the pool): nothing to fetch, read_merge marks it
    origin = o_off = None
    if need.size:
        origin, got = fetch(need)
        got = np.asarray(got, dtype=np.uint64)
        if got.size != need.size:
            raise CurveCrcError(_lib.CC_EINVAL, "fetch must return one origin offset per index")
        o_off = np.full(off.size, NO_ORIGIN, dtype=np.uint64)
        o_off[need] = got
    res = read_merge(pool, page_crcs, off, ln, clone, origin=origin, origin_off=o_off, page_bytes=page_bytes,
                     stream=stream)
    if paste and need.size:
        if (ln[need] >> np.uint64(32)).any():
            raise CurveCrcError(_lib.CC_EINVAL, "a paste entry holds at most 2^32 - 1 bytes")
        _paste_fetched(pool, page_crcs, origin, off[need], o_off[need], ln[need], clone, page_bytes, stream)
    return res


REPAIR_CLEAN, REPAIR_REPAIRED, REPAIR_FAILED, REPAIR_SHADOWED = 0, 1, 2, 3  # the words of cc_repair_counts, in order
REPAIR_CLASSES = ("clean", "repaired", "failed", "shadowed")


def repair_claim(pool, page_bytes: int = PAGE_SIZE):
    """cc_repair_dev's claim table for `pool`: one int32 per pool page, -1
    (all-ones) everywhere, which is how every completed call leaves it.  Keep it
    beside the pool and hand it to every repair call on it."""
    torch = _torch()
    nb = _nbytes(pool)
    if nb % page_bytes:
        raise CurveCrcError(_lib.CC_EINVAL, "pool size is not a multiple of page_bytes")
    return torch.full((nb // page_bytes,), -1, dtype=torch.int32, device=pool.device)


def repair_records(pool, page_crcs, src, d_reqs, n: int, claim, per_entry, expect=None, totals=None,
                   page_bytes: int = PAGE_SIZE, stream=None):
    """cc_repair_dev on a batch already resident on the device: `d_reqs` =
    device tensor of n cc_update records (log_records), an ORDERED batch: entry
    i offers src[src_i + ...] as the candidate for the pool pages of [dst_i,
    dst_i + len_i).  The lowest-indexed valid entry naming a page handles it:
    with e = expect[p] (or page_crcs[p] when expect is None) the page is clean
    (the live bytes hash to e), repaired (the candidate does: it is stored, and
    page_crcs[p] = e) or failed (neither: nothing written); every other pair is
    shadowed.  `per_entry` int32 [n, 4] gets += by class (clean, repaired,
    failed, shadowed; -1 in all four marks an invalid entry), `totals` int64
    [4] (optional) the sums; `claim` = repair_claim(pool).  No host sync."""
    torch = _torch()
    if claim.numel() * page_bytes < _nbytes(pool) or claim.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "claim must hold one 32-bit word per pool page")
    if page_crcs.numel() * page_bytes < _nbytes(pool) or page_crcs.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "page_crcs must hold one 32-bit CRC per pool page")
    if expect is not None and (expect.numel() * page_bytes < _nbytes(pool) or expect.element_size() != 4):
        raise CurveCrcError(_lib.CC_EINVAL, "expect must hold one 32-bit CRC per pool page")
    if per_entry.numel() < 4 * n or per_entry.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "per_entry must hold four 32-bit words per entry")
    if totals is not None and (totals.numel() < 4 or totals.element_size() != 8):
        raise CurveCrcError(_lib.CC_EINVAL, "totals must hold four 64-bit words")
    with torch.cuda.device(pool.device):
        check(lib().cc_repair_dev(_dev_ptr(pool, "pool"), _nbytes(pool), page_bytes, _dev_ptr(src, "src"),
                                  _nbytes(src), _dev_ptr(d_reqs, "reqs"), n, _dev_ptr(page_crcs, "page_crcs"),
                                  _dev_ptr(expect, "expect") if expect is not None else None,
                                  _dev_ptr(claim, "claim"), _dev_ptr(per_entry, "per_entry"),
                                  _dev_ptr(totals, "totals") if totals is not None else None,
                                  _stream_handle(stream)), "cc_repair_dev")
    if stream is not None:
        for t in (claim, expect, totals):
            if t is not None:
                t.record_stream(stream)


def repair(pool, page_crcs, src, dst_off, src_off, lens, claim, expect=None, page_bytes: int = PAGE_SIZE,
           stream=None):
    """cc_repair_dev: the candidate ranges (dst_off, src_off, lens), in order,
    from the device tensor `src` (a peer's copies) for `pool`.  Returns
    (per_entry int32 [n, 4] device tensor: each entry's pages as clean,
    repaired, failed, shadowed, -1 in all four = invalid entry; totals int64
    [4]).  No host sync."""
    import numpy as np
    torch = _torch()
    rec = log_records(dst_off, src_off, lens)
    n = rec.size
    with _on_stream(stream):
        per_entry = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=pool.device)
        totals = torch.zeros(4, dtype=torch.int64, device=pool.device)
        if n == 0:
            return per_entry[:0], totals
        d_reqs = torch.from_numpy(rec.view(np.uint8)).to(pool.device)
    repair_records(pool, page_crcs, src, d_reqs, n, claim, per_entry, expect=expect, totals=totals,
                   page_bytes=page_bytes, stream=stream)
    if stream is not None:
        for t in (d_reqs, per_entry, totals, src):
            t.record_stream(stream)
    return per_entry[:n], totals


def repair_pages(pool, page_crcs, pages, fetchers, claim, expect=None, page_bytes: int = PAGE_SIZE, stream=None):
    """Repair the pool pages `pages` (page indices, any order, duplicates
    allowed) from a list of peers, in the spirit of clone_read.  The pages are
    made unique and ascending; then for each fetcher in order
    `fetch(remaining_pages)` -- the control plane's ReadChunk from that peer --
    returns (src uint8 device tensor, src_off: one byte offset per page), and
    ONE repair call sends one one-page entry per remaining page, so every
    entry's counts are a status.  Pages still failed go to the next fetcher; the
    rounds stop when none is left.  Returns (pages, cls, by): the unique
    ascending pages (numpy int64), each page's final class (numpy int8:
    REPAIR_CLEAN, REPAIR_REPAIRED or REPAIR_FAILED) and the index of the fetcher
    whose copy repaired it (numpy int64, -1 unless repaired).  With no fetcher
    nothing is judged and every page stays REPAIR_FAILED.  A page beyond the
    pool or a fetched range outside its buffer raises CC_EINVAL (the earlier
    rounds' repairs stand).  One host sync a round, on `stream`: the statuses
    choose what the next peer is asked for."""
    import numpy as np
    pg = np.unique(np.asarray(pages, dtype=np.int64))
    cls = np.full(pg.size, REPAIR_FAILED, dtype=np.int8)
    by = np.full(pg.size, -1, dtype=np.int64)
    left = np.arange(pg.size)
    for f, fetch in enumerate(fetchers):
        if not left.size:
            break
        src, got = fetch(pg[left])
        got = np.asarray(got, dtype=np.uint64)
        if got.size != left.size:
            raise CurveCrcError(_lib.CC_EINVAL, "fetch must return one source offset per page")
        dst = pg[left].astype(np.uint64) * np.uint64(page_bytes)
        per, _ = repair(pool, page_crcs, src, dst, got, np.full(left.size, page_bytes, np.uint32), claim,
                        expect=expect, page_bytes=page_bytes, stream=stream)
        if stream is not None:
            stream.synchronize()  # the statuses were made on `stream`; the copy below runs on the current one
        st = per.cpu().numpy().reshape(-1, 4)
        if (st < 0).any():
            raise CurveCrcError(_lib.CC_EINVAL, "a page lies beyond the pool or its fetched range outside the buffer")
        now = st[:, :3].argmax(axis=1).astype(np.int8)  # unique pages: nothing is shadowed, one word is 1
        cls[left] = now
        by[left[now == REPAIR_REPAIRED]] = f
        left = left[now == REPAIR_FAILED]
    return pg, cls, by


SCRUB_SNAP = _lib.CC_SCRUB_SNAP  # scrub list entry: the snapshot copy of pool page (entry & ~SCRUB_SNAP)
SCRUB_COUNTS = ("live_checked", "live_bad", "snap_checked", "snap_bad", "unwritten", "listed")


def scrub_records(pool, page_crcs, chunk_bytes: int, counts, bad_list, bad_per_chunk=None, cow: Optional[Cow] = None,
                  clone: Optional[Clone] = None, page_bytes: int = PAGE_SIZE, stream=None):
    """cc_scrub_dev on buffers already resident on the device: the integrity
    pass over `pool` as the datastore sees it.  Every live page that exists (not
    a never-written page of a clone chunk of `clone`) is hashed against
    `page_crcs`, every snapshot page that exists (its bit set in a slot of `cow`
    that a chunk names) against cow.snap_crcs; never-written pages are counted
    and not read.  `counts` int64 [6] gets += (SCRUB_COUNTS: live_checked,
    live_bad, snap_checked, snap_bad, unwritten, listed); every mismatch takes
    the next list position from `listed` and, while it is below
    bad_list.numel(), stores its entry there (`bad_list` int64, or None for no
    list: the pool page, | SCRUB_SNAP -- the sign bit -- for a snapshot copy);
    `bad_per_chunk` int32 [chunks, 2] (optional) gets += (live_bad, snap_bad).
    Reads the pool, the tables and the bitmaps only.  No host sync."""
    torch = _torch()
    nb = _nbytes(pool)
    if page_bytes <= 0 or nb % page_bytes:
        raise CurveCrcError(_lib.CC_EINVAL, "pool size is not a multiple of page_bytes")
    if page_crcs.numel() * page_bytes < nb or page_crcs.element_size() != 4:
        raise CurveCrcError(_lib.CC_EINVAL, "page_crcs must hold one 32-bit CRC per pool page")
    if counts.numel() < 6 or counts.element_size() != 8:
        raise CurveCrcError(_lib.CC_EINVAL, "counts must hold six 64-bit words")
    if bad_list is not None and bad_list.element_size() != 8:
        raise CurveCrcError(_lib.CC_EINVAL, "bad_list must hold 64-bit words")
    if bad_per_chunk is not None and (chunk_bytes <= 0 or bad_per_chunk.element_size() != 4 or
                                      bad_per_chunk.numel() * chunk_bytes < 2 * nb):
        raise CurveCrcError(_lib.CC_EINVAL, "bad_per_chunk must hold two 32-bit words per chunk")
    ws = cow.struct() if cow is not None else None
    cs = clone.struct() if clone is not None else None
    max_list = bad_list.numel() if bad_list is not None else 0
    with torch.cuda.device(pool.device):
        check(lib().cc_scrub_dev(_dev_ptr(pool, "pool"), nb, page_bytes, chunk_bytes, _dev_ptr(page_crcs, "page_crcs"),
                                 ctypes.byref(ws) if ws is not None else None,
                                 ctypes.byref(cs) if cs is not None else None, _dev_ptr(counts, "counts"),
                                 _dev_ptr(bad_list, "bad_list") if max_list else None, max_list,
                                 _dev_ptr(bad_per_chunk, "bad_per_chunk") if bad_per_chunk is not None else None,
                                 _stream_handle(stream)), "cc_scrub_dev")
    if stream is not None:
        if cow is not None:
            _record_cow(cow, stream)
        if clone is not None:
            _record_clone(clone, stream)


class ScrubResult:
    """What scrub() found: the six counts as attributes (SCRUB_COUNTS),
    `live_bad_pages` / `snap_bad_pages` = sorted (chunk index, page in chunk)
    pairs, and `per_chunk` = numpy int32 [chunks, 2] of (live_bad, snap_bad)."""

    def __init__(self, counts, live_bad_pages, snap_bad_pages, per_chunk):
        for name, v in zip(SCRUB_COUNTS, counts):
            setattr(self, name, int(v))
        self.live_bad_pages, self.snap_bad_pages, self.per_chunk = live_bad_pages, snap_bad_pages, per_chunk

    @property
    def clean(self) -> bool:
        return self.live_bad == 0 and self.snap_bad == 0

    def __repr__(self):
        return "ScrubResult(" + ", ".join(f"{n}={getattr(self, n)}" for n in SCRUB_COUNTS) + ")"


def scrub(pool, page_crcs, chunk_bytes: int, cow: Optional[Cow] = None, clone: Optional[Clone] = None,
          max_bad: int = 4096, page_bytes: int = PAGE_SIZE, stream=None) -> ScrubResult:
    """cc_scrub_dev: scrub `pool` (chunks of `chunk_bytes`) with its snapshot
    slots `cow` and clone bitmaps `clone` (either may be None) and read the
    result back.  Returns a ScrubResult.  Raises CC_ECORRUPT when more than
    max_bad pages mismatch (the list cannot name them all), as
    DevicePool.bad_pages does.  One host sync, on `stream`."""
    import numpy as np
    torch = _torch()
    nb = _nbytes(pool)
    if chunk_bytes <= 0 or nb % chunk_bytes:
        raise CurveCrcError(_lib.CC_EINVAL, "pool size is not a multiple of chunk_bytes")
    with _on_stream(stream):
        counts = torch.zeros(6, dtype=torch.int64, device=pool.device)
        lst = torch.full((max(1, max_bad),), -1, dtype=torch.int64, device=pool.device)
        per = torch.zeros((max(1, nb // chunk_bytes), 2), dtype=torch.int32, device=pool.device)
        scrub_records(pool, page_crcs, chunk_bytes, counts, lst[:max_bad] if max_bad else None, per, cow=cow,
                      clone=clone, page_bytes=page_bytes, stream=stream)
        if stream is not None:
            for t in (counts, lst, per):
                t.record_stream(stream)
            stream.synchronize()  # the results were made on `stream`; the copies below run on the current one
        cnt = counts.cpu().numpy()
        listed = int(cnt[5])
        if listed > max_bad:
            raise CurveCrcError(_lib.CC_ECORRUPT, f"{listed} bad pages > max_bad={max_bad}")
        ent = lst[:listed].cpu().numpy().view(np.uint64)
        per_chunk = per[:nb // chunk_bytes].cpu().numpy()
    ppc = chunk_bytes // page_bytes
    snap = (ent >> np.uint64(63)).astype(bool)
    pg = ent & np.uint64(SCRUB_SNAP - 1)
    live_pages = sorted((int(p) // ppc, int(p) % ppc) for p in pg[~snap])
    snap_pages = sorted((int(p) // ppc, int(p) % ppc) for p in pg[snap])
    return ScrubResult(cnt, live_pages, snap_pages, per_chunk)


def scan_files(paths, chunk_bytes: int = CHUNK_SIZE, meta_bytes: int = META_PAGE_SIZE,
               page_bytes: int = PAGE_SIZE, slice_bytes: int = SCAN_SIZE, io_threads: int = 0):
    """cc_scan_files: native pread + scan of chunk files.
    Returns (status[n] int32, meta_crcs[n], slice_crcs[n, S], file_crcs[n]) numpy."""
    import numpy as np
    n = len(paths)
    arr = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
    res = (_lib.CcFileResult * max(n, 1))()
    S = chunk_bytes // slice_bytes
    sc = np.zeros((n, S), dtype=np.uint32)
    check(lib().cc_scan_files(arr, n, chunk_bytes, meta_bytes, page_bytes, slice_bytes, io_threads,
                              ctypes.c_void_p(sc.ctypes.data), res), "cc_scan_files")
    st = np.array([res[i].status for i in range(n)], dtype=np.int32)
    mc = np.array([res[i].meta_crc for i in range(n)], dtype=np.uint32)
    fc = np.array([res[i].file_crc for i in range(n)], dtype=np.uint32)
    return st, mc, sc, fc


def default_io_threads() -> int:
    """cc_default_io_threads: the reader count scan_files(io_threads=0) uses."""
    return int(lib().cc_default_io_threads())


def as_u32(t) -> "list[int]":
    """Device/host int32 CRC tensor -> python ints in [0, 2^32)."""
    return [int(x) & 0xFFFFFFFF for x in t.detach().cpu().tolist()]
