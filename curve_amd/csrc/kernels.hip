// curve_amd/csrc/kernels.hip -- hand-written gfx950 (CDNA4) kernels for the
// per-page CRC32C hot path.  Bandwidth-bound integer GF(2) work: no MFMA.
//
// Page kernel (one wavefront per page, grid-stride over pages)
// ------------------------------------------------------------
// A page of P = 256*M bytes is M steps of one coalesced 256-byte wave load:
// lane l holds dwords w[l + 64 j], j = 0..M-1.  In the raw (zero-init) CRC
// domain the page register is XOR_i F^(n-i)(w_i), F = "multiply by x^32 mod P"
// (feeding one dword).  Lane l runs a Horner chain with the 256-byte jump
// G = F^64:   s = w[l]; s = G(s) ^ w[l + 64 j]   (j = 1..M-1)
// which leaves s = XOR_j F^(64(M-1-j)) w_j, so lane l's share of the page
// register is F^(64-l)(s) -- independent of M.  The wave XOR-reduces the 64
// shares and adds the length constant K(P) = ~shift(~0, P) to get V(page).
//
// G is applied with 4 byte lookups per dword from LDS tables replicated 32x
// so that lane l always reads bank (l mod 32): every ds_read_b32 is
// conflict-free (2 LDS cycles per wave instruction).  The address of a lookup
// is ONE v_perm_b32 that splices {lane slot, state byte k, region} into a
// dword; the lookups are XORed with v_bitop3_b32.  F^(64-l) is lane-specific: 8 nibble lookups into per-lane tables
// (bank = lane mod 32 again).  Layout: DESIGN.md "LDS image".
//
// Reference being replaced: the CRC32(buf, size) loop of the scan hasher
// (src/chunkserver/op_request.cpp:794, :847) and of the chunk/copyset hashers
// (src/chunkserver/datastore/chunkserver_chunkfile.cpp:805,
// src/chunkserver/copyset_node.cpp:964), all of which call
// curve::common::CRC32 (src/common/crc32.h:40-55).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <type_traits>
#include <stdint.h>

#include "kernels.h"

namespace cc {
namespace {

constexpr uint32_t kPolyDev = 0x82F63B78u;

__device__ __forceinline__ uint32_t lds_u32(const uint32_t* tab, uint32_t byte_addr) {
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(tab) + byte_addr);
}

// One step of a lane's Horner chain: G(s) ^ w, G = x^(32*64) mod P.
// c0 = lane slot (region 0), c1 = lane slot | region 1 (bit 16).  v_perm_b32
// selector bytes: [0] = c.byte0 (lane*4), [1] = s.byte_k, [2] = c.byte2
// (region), [3] = 0x00.  The 4 lookups and w are XORed by two v_bitop3_b32
// (truth table 0x96 = 3-input XOR; gfx950 has no v_xor3): 6 VALU per step
// instead of 8 measured +3 % on the page kernel.
__device__ __forceinline__ uint32_t apply_g_xor(const uint32_t* tab, uint32_t s, uint32_t w, uint32_t c0,
                                                uint32_t c1) {
    const uint32_t a0 = __builtin_amdgcn_perm(c0, s, 0x0C060004u);
    const uint32_t a1 = __builtin_amdgcn_perm(c0, s, 0x0C060104u);
    const uint32_t a2 = __builtin_amdgcn_perm(c1, s, 0x0C060204u);
    const uint32_t a3 = __builtin_amdgcn_perm(c1, s, 0x0C060304u);
    const uint32_t t0 = lds_u32(tab, a0);
    const uint32_t t1 = lds_u32(tab, a1 + 128u);
    const uint32_t t2 = lds_u32(tab, a2);
    const uint32_t t3 = lds_u32(tab, a3 + 128u);
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(t0, t1, t2, 0x96), t3, w, 0x96);
}

// Lane-specific final shift F^(64-l) via 8 nibble lookups.  cf = kFinBase + 4*lane.
__device__ __forceinline__ uint32_t apply_fin(const uint32_t* tab, uint32_t s, uint32_t cf) {
    uint32_t r = 0;
#pragma unroll
    for (int n = 0; n < 8; n++) {
        const uint32_t v = (s >> (4 * n)) & 15u;
        r ^= lds_u32(tab, ((v << 8) | cf) + 4096u * n);
    }
    return r;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t l) {
    // readlane returns int: go through uint32_t so the low half is not sign-extended
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)v, l);
}

// XOR over the 64 lanes, result wave-uniform (SGPR).
__device__ __forceinline__ uint32_t wave_xor(uint32_t r) {
    r ^= __builtin_amdgcn_mov_dpp(r, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    r ^= __builtin_amdgcn_mov_dpp(r, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    r ^= __builtin_amdgcn_mov_dpp(r, 0x124, 0xF, 0xF, false);  // row_ror:4
    r ^= __builtin_amdgcn_mov_dpp(r, 0x128, 0xF, 0xF, false);  // row_ror:8
    return __builtin_amdgcn_readlane(r, 0) ^ __builtin_amdgcn_readlane(r, 16) ^
           __builtin_amdgcn_readlane(r, 32) ^ __builtin_amdgcn_readlane(r, 48);
}

template <int THREADS = kBlockThreads>
__device__ __forceinline__ void fill_lds(uint32_t* tab, const uint4* __restrict__ image) {
    uint4* t4 = reinterpret_cast<uint4*>(tab);
#pragma unroll 2
    for (uint32_t i = threadIdx.x; i < kLdsBytes / 16; i += THREADS) t4[i] = image[i];
    __syncthreads();
}

template <int M>
__device__ __forceinline__ void load_page(uint32_t (&w)[M], const uint32_t* __restrict__ p) {
#pragma unroll
    for (int j = 0; j < M; j++)
        w[j] = __builtin_nontemporal_load(p + 64 * j);  // read-once stream: nt (probe: +12 % read BW)
    // keep the whole page's loads ahead of the chain that follows (the
    // machine scheduler otherwise sinks them into it, shrinking the prefetch)
    __builtin_amdgcn_sched_barrier(0);
}

template <int M>
__device__ __forceinline__ uint32_t chain(const uint32_t* tab, const uint32_t (&w)[M], uint32_t c0, uint32_t c1) {
    uint32_t s = w[0];
#pragma unroll
    for (int j = 1; j < M; j++) s = apply_g_xor(tab, s, w[j], c0, c1);
    return s;
}

template <int MODE>
__device__ __forceinline__ void emit(uint32_t crc, uint64_t page, uint32_t lane, uint32_t* __restrict__ out,
                                     const uint32_t* __restrict__ expected, const VerifySink& vs) {
    if (MODE == 0) {
        if (lane == 0) out[page] = crc;
    } else {
        const uint32_t want = expected[page];
        if (crc != want && lane == 0) {
            const unsigned long long at = atomicAdd(vs.bad_count, 1ull);
            atomicMin(vs.first_bad, (unsigned long long)page);
            if (vs.list && at < vs.max_list) vs.list[at] = page;
            if (vs.per_chunk) atomicAdd(vs.per_chunk + 2 * (page / vs.pages_per_chunk), 1u);
        }
    }
}

// Tile of 64 consecutive pages per wave: the page CRCs are gathered into one
// register (lane k <- page k of the tile) and leave as ONE coalesced 256-byte
// store (compute) or are compared against ONE 256-byte load of expected CRCs
// with a ballot (verify).  Sparse 4-byte single-lane stores cost ~10 % of HBM
// efficiency in the first version.
template <int MODE>
__device__ __forceinline__ void flush_tile(uint32_t acc, uint64_t tile_first, uint32_t cnt, uint32_t lane,
                                           uint32_t* __restrict__ out, const uint32_t* __restrict__ expected,
                                           const VerifySink& vs) {
    if (MODE != 1) {  // compute (0; 3 = the metapage pass) and the load-only probe (2) store the tile
        // nt: the CRC stream must not interleave cached partial-line writes with
        // the 16 GiB nt read stream (plain stores cost 3 % of HBM throughput)
        if (lane < cnt) __builtin_nontemporal_store(acc, out + tile_first + lane);
    } else {
        const uint32_t want = lane < cnt ? __builtin_nontemporal_load(expected + tile_first + lane) : acc;
        const uint64_t bad = __ballot(want != acc);
        if (bad) {  // rare: wave-uniform branch
            unsigned long long at = 0;
            if (lane == 0) {
                at = atomicAdd(vs.bad_count, (unsigned long long)__popcll(bad));
                atomicMin(vs.first_bad, (unsigned long long)(tile_first + __ffsll((long long)bad) - 1));
            }
            if (vs.list) {  // every bad page of the tile gets a slot after `at`
                at = (unsigned long long)__shfl((long long)at, 0);
                const unsigned long long idx = at + (unsigned long long)__popcll(bad & ((1ull << lane) - 1ull));
                if (((bad >> lane) & 1ull) && idx < vs.max_list) vs.list[idx] = tile_first + lane;
            }
            if (vs.per_chunk && ((bad >> lane) & 1ull))  // cc_scrub_dev's per-chunk words
                atomicAdd(vs.per_chunk + 2 * ((tile_first + lane) / vs.pages_per_chunk), 1u);
        }
    }
}

constexpr int kPrefetch = 2;  // wave steps in flight ahead of the one being hashed (2..4 measured equal)

// Page sequence of one wave: its k-th page is wfirst + (k >> ts) * wstride + (k & tmask),
// strictly increasing in k.
struct Walk {
    uint64_t wfirst, wstride;
    uint32_t tshift, tmask;
    __device__ __forceinline__ uint64_t page(uint64_t k) const {
        return wfirst + (k >> tshift) * wstride + (k & tmask);
    }
};

constexpr int kPair = 1;  // pages hashed together per wave step (2 measured equal)

template <int M, int P>
__device__ __forceinline__ void load_pages(uint32_t (&w)[P][M], const uint32_t* __restrict__ base, const Walk& W,
                                           uint64_t k, uint64_t last) {
#pragma unroll
    for (int q = 0; q < P; q++) {
        const uint64_t pg = W.page(k + q);
        load_page<M>(w[q], base + (pg < last ? pg : last) * (64u * M));
    }
}

// P independent Horner chains, interleaved step by step so each wave keeps
// 4*P LDS lookups in flight instead of 4.
// LOADS_ONLY: the chain replaced by a rotate-XOR that keeps every loaded word
// live (the load-only probe, MODE 2: the kernel's own schedule and traffic
// without the CRC arithmetic)
template <int M, int P, bool LOADS_ONLY = false>
__device__ __forceinline__ void chains(const uint32_t* tab, const uint32_t (&w)[P][M], uint32_t c0, uint32_t c1,
                                       uint32_t (&s)[P]) {
#pragma unroll
    for (int q = 0; q < P; q++) s[q] = w[q][0];
#pragma unroll
    for (int j = 1; j < M; j++) {
#pragma unroll
        for (int q = 0; q < P; q++) {
            if (LOADS_ONLY)
                s[q] = ((s[q] << 1) | (s[q] >> 31)) ^ w[q][j];
            else
                s[q] = apply_g_xor(tab, s[q], w[q][j], c0, c1);
        }
    }
}

// MODE 0: compute CRCs into out[]; MODE 1: verify against expected[].
// Wave w walks tiles w, w+W, w+2W, ... (W = waves in the grid) of 2^ts pages,
// P pages per step.  kPrefetch+1 register buffers rotate so kPrefetch
// steps' loads are in flight while the current step is hashed.  Loads are
// unconditional (index clamped to the item's last page) so hipcc counts vmcnt
// exactly.
// Dynamic tail (dyn_ctr != null): the strided walk covers tiles [0, static_tiles)
// only; the remaining tiles are handed out kPageDynPages pages at a time through
// the atomic counter *dyn_ctr (zeroed by the caller) to whichever waves finish
// first.  Per-wave rates differ by XCD (a kernel trace shows odd XCDs ~10 %
// slower on the same work), so a purely static split waits for the slowest.
constexpr uint64_t kPageDynPages = 64;  // pages per dynamic chunk (A/B: 64 beats 128)
// Dynamic-tail heads (kernels.h kDynHeads): 1 = one counter for the whole grid;
// 8 = one per XCD (MI355X_MICROARCH.md "dequeue": one word saturates at ~88
// dequeues/us, shard above 64 pullers).  With 8 heads the tail's chunks are cut
// into 8 contiguous regions; a wave pulls from its own XCD's region
// (blockIdx.x % 8: workgroups go round-robin over the XCDs -- placement is
// speed only, never correctness) and, once that is drained, steals from the
// next regions in turn.
// Next chunk of a dynamic tail of n_chunks chunks, from kDynHeads counters
// kDynHeadStride words apart (zeroed before the launch).  With one head: a
// plain dequeue.  With 8: the chunks are cut into 8 contiguous regions, a wave
// pulls from its own XCD's region first (blockIdx.x % 8 -- workgroups go
// round-robin over the XCDs; placement is speed only, never correctness) and
// steals from the next regions once that is drained.  `head` / `tried` are the
// wave's (uniform) cursor, initialised by tail_cursor().  Returns n_chunks when
// every region is drained.  Lane 0 does the atomics.
template <uint32_t H = kDynHeads>
__device__ __forceinline__ void tail_cursor(uint32_t& head, uint32_t& tried) {
    head = blockIdx.x % H;
    tried = 0;
}
template <uint32_t H = kDynHeads>
__device__ __forceinline__ uint64_t tail_pull(unsigned long long* __restrict__ ctr, uint64_t n_chunks, uint32_t& head,
                                              uint32_t& tried, uint32_t lane) {
    static_assert(H >= 1 && H <= kDynHeads, "heads beyond the zeroed counters");
    if constexpr (H == 1) {
        unsigned long long c = 0;
        if (lane == 0) c = atomicAdd(ctr, 1ull);
        c = readlane64(c, 0);
        return c < n_chunks ? c : n_chunks;
    } else {
        const uint64_t per = (n_chunks + H - 1) / H;
        for (; tried < H; tried++, head = (head + 1) % H) {
            unsigned long long c = 0;
            if (lane == 0) c = atomicAdd(ctr + head * kDynHeadStride, 1ull);
            c = readlane64(c, 0);
            const uint64_t chunk = head * per + c;
            if (c < per && chunk < n_chunks) return chunk;
        }
        return n_chunks;
    }
}

struct ZeroRanges {
    uint32_t* p[2];
    uint64_t n[2];
    __device__ __forceinline__ void clear() const {
#pragma unroll
        for (int k = 0; k < 2; k++)
            for (uint64_t i = threadIdx.x; i < n[k]; i += blockDim.x) p[k][i] = 0u;
    }
};
// The dynamic tail's extras (PageLaunch::meta_pages / dyn_next): a second page
// array appended to the tail as chunks of its own, and the other slot set of
// the stream's tail block, which this launch zeroes for the stream's next one.
// (Round 3 reset the counters at the END: every wave added to an arrival word
// and the last one zeroed the heads -- 2,048 returning atomics on one word in
// the kernel's last microseconds, ~12 ns each when they queue.)
struct TailExtra {
    const uint32_t* pages;
    uint64_t n;
    uint32_t* out;
    unsigned long long* next;
};
__device__ __forceinline__ void tail_clear_next(const TailExtra& ex) {
    if (ex.next && blockIdx.x == 0 && threadIdx.x < kDynHeads) atomicExch(ex.next + threadIdx.x * kDynHeadStride, 0ull);
}

template <int M, int MODE>
__global__ __launch_bounds__(kBlockThreads) void page_crc_kernel(
    const uint32_t* __restrict__ pages, uint64_t n_pages, const uint4* __restrict__ image,
    uint32_t kconst, uint32_t* __restrict__ out, const uint32_t* __restrict__ expected, VerifySink vs,
    uint32_t tshift, unsigned long long* __restrict__ dyn_ctr, uint64_t static_tiles, ZeroRanges zr, TailExtra ex) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    if (blockIdx.x == 0) zr.clear();
    tail_clear_next(ex);
    fill_lds(tab, image);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    const uint32_t* base = pages + lane;
    uint32_t* dst = out;
    constexpr int D = kPrefetch;
    constexpr int P = (M <= 16) ? kPair : 1;  // register budget: P*(D+1)*M data VGPRs
    // item 0: the strided static walk over tiles [0, static_tiles); then dynamic chunks
    Walk W;
    W.tshift = tshift;
    W.tmask = (1u << tshift) - 1u;
    W.wstride = ((uint64_t)gridDim.x * kWavesPerBlock) << tshift;
    W.wfirst = ((uint64_t)blockIdx.x * kWavesPerBlock + wave) << tshift;
    uint64_t lim = dyn_ctr ? (static_tiles << tshift < n_pages ? static_tiles << tshift : n_pages) : n_pages;
    uint32_t dyn_head, dyn_tried;  // this XCD's tail region first
    tail_cursor(dyn_head, dyn_tried);
#pragma unroll 1
    for (;;) {
        if (W.wfirst < lim) {
            const uint64_t last = lim - 1;
            uint32_t acc = 0;
            // ring of D+1 register buffers; after full unrolling every index is a
            // compile-time constant, so the ring lives in VGPRs (no scratch)
            uint32_t ring[D + 1][P][M];
#pragma unroll
            for (int st = 0; st < D; st++) load_pages<M, P>(ring[st], base, W, (uint64_t)st * P, last);
            // Every step's loads are unconditional (clamped) and termination is tested
            // once per ring revolution: path-insensitive waitcnt dataflow then sees the
            // same D stages outstanding on every edge into a step and keeps each wait
            // at its exact count (a per-step early exit made hipcc over-wait a stage).
            for (uint64_t k = 0;; k += (uint64_t)(D + 1) * P) {
#pragma unroll
                for (int st = 0; st <= D; st++) {
                    const uint64_t kk = k + (uint64_t)st * P;
                    load_pages<M, P>(ring[(st + D) % (D + 1)], base, W, kk + (uint64_t)D * P, last);
                    uint32_t s[P];
                    chains<M, P, MODE == 2>(tab, ring[st], c0, c1, s);
#pragma unroll
                    for (int q = 0; q < P; q++) {
                        const uint64_t kq = kk + q;
                        const uint64_t pc = W.page(kq);
                        if (pc < lim) {
                            const uint64_t pn = W.page(kq + 1);
                            const uint32_t crc = MODE == 2 ? wave_xor(s[q]) : wave_xor(apply_fin(tab, s[q], cf)) ^ kconst;
                            const uint32_t slot = (uint32_t)(kq & W.tmask);
                            acc = lane == slot ? crc : acc;
                            if (slot == W.tmask || pn >= lim)
                                flush_tile<MODE>(acc, pc - slot, slot + 1u, lane, dst, expected, vs);
                        }
                    }
                }
                if (W.page(k + (uint64_t)(D + 1) * P) >= lim) break;
            }
        }
        if (!dyn_ctr) break;
        // next dynamic chunk: kPageDynPages consecutive pages of the fused
        // metapages (the first chunk indices: pulled early, so the tail's last
        // chunks stay data chunks that even out as before), then of the data
        const uint64_t tail0 = static_tiles << tshift;
        const uint64_t mchunks = (ex.n + kPageDynPages - 1) / kPageDynPages;
        const uint64_t chunks = mchunks + (n_pages - tail0 + kPageDynPages - 1) / kPageDynPages;
        const uint64_t chunk = tail_pull(dyn_ctr, chunks, dyn_head, dyn_tried, lane);
        if (chunk >= chunks) break;
        uint64_t p0, end;
        if (chunk >= mchunks) {
            base = pages + lane;
            dst = out;
            p0 = tail0 + (chunk - mchunks) * kPageDynPages;
            end = n_pages;
        } else {
            base = ex.pages + lane;
            dst = ex.out;
            p0 = chunk * kPageDynPages;
            end = ex.n;
        }
        W.wfirst = p0;
        W.wstride = 1ull << tshift;  // consecutive tiles: page(k) = p0 + k
        lim = p0 + kPageDynPages < end ? p0 + kPageDynPages : end;
    }
}

// Any M (page_bytes = 256*M): no register prefetch, dynamic chain length.
template <int MODE>
__global__ __launch_bounds__(kBlockThreads) void page_crc_kernel_dyn(
    const uint32_t* __restrict__ pages, uint64_t n_pages, uint32_t M, const uint4* __restrict__ image,
    uint32_t kconst, uint32_t* __restrict__ out, const uint32_t* __restrict__ expected, VerifySink vs,
    ZeroRanges zr) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    if (blockIdx.x == 0) zr.clear();
    fill_lds(tab, image);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t stride = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    for (uint64_t page = (uint64_t)blockIdx.x * kWavesPerBlock + wave; page < n_pages; page += stride) {
        const uint32_t* p = pages + page * (64ull * M) + lane;
        uint32_t s = p[0];
        for (uint32_t j = 1; j < M; j++) s = apply_g_xor(tab, s, p[64ull * j], c0, c1);
        emit<MODE>(wave_xor(apply_fin(tab, s, cf)) ^ kconst, page, lane, out, expected, vs);
    }
}

// cache policy bits (aux) of the write log's buffer instructions: 2 = nontemporal.
// Row loads nt (A/B of 0-3 within 1 %); row stores nt (-20 us a batch); source
// loads default (nt measured 6 % slower).
constexpr int kLogRowAux = 2;
constexpr int kLogStoreAux = 2;
constexpr uint32_t kBufOOB = 0x80000000u;   // offset past num_records: load 0 / store dropped
constexpr uint32_t kBufFlags = 0x00020000u;  // buffer resource dword 3 for gfx9-family (CDNA)
// A per-row buffer offset is `sel + 256 j` with sel = (lane's dword wanted ?
// its offset : kBufOOB).  Left alone, the compiler folds the add into both arms
// of the select and keeps 2 x M loop-invariant row constants in VGPRs (32 at
// 4 KiB pages); with sel opaque the 256 j goes into the instruction's 12-bit
// offset field (kBufOOB + 256 j is still past num_records).
__device__ __forceinline__ uint32_t row_sel(uint32_t v) {
    asm("" : "+v"(v));
    return v;
}


// ---------------------------------------------------------------------------
// GF(2) helpers for the fold / shift kernels (tiny volume: 4 B per page).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mulmod_dev(uint32_t a, uint32_t b) {
    uint32_t prod = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        prod ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (kPolyDev & (0u - (b & 1u)));
    }
    return prod;
}

struct X2k {
    uint32_t t[64];
};
__constant__ X2k c_x2k;  // x^(2^k) mod P, uploaded once per device by engine.hip

__device__ __forceinline__ uint32_t xpow_dev(uint64_t n) {
    uint32_t r = 0x80000000u;
    for (int k = 0; n; k++, n >>= 1)
        if (n & 1u) r = mulmod_dev(r, c_x2k.t[k]);
    return r;
}

// Compact forms for once-per-range code inside unrolled block loops (keeps
// the kernel's instruction footprint small; the unrolled ones are 6x larger).
__device__ __forceinline__ uint32_t mulmod_small(uint32_t a, uint32_t b) {
    uint32_t prod = 0;
#pragma unroll 4
    for (int i = 0; i < 32; i++) {
        prod ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (kPolyDev & (0u - (b & 1u)));
    }
    return prod;
}
__device__ __forceinline__ uint32_t xpow_wave_small(uint64_t n, uint32_t lane) {
    uint32_t f = ((n >> lane) & 1u) ? c_x2k.t[lane] : 0x80000000u;
#pragma unroll 1
    for (int t = 1; t < 64; t <<= 1) f = mulmod_small(f, __shfl_xor(f, t, 64));
    return f;
}

// Product over the wave of per-lane GF(2)[x]/P factors (lane k: x^(2^k) if bit k
// of n is set, else 1) = x^n mod P; result in every lane.
__device__ __forceinline__ uint32_t xpow_wave(uint64_t n, uint32_t lane) {
    uint32_t f = (lane < 64 && ((n >> lane) & 1u)) ? c_x2k.t[lane] : 0x80000000u;
#pragma unroll
    for (int t = 1; t < 64; t <<= 1) f = mulmod_dev(f, __shfl_xor(f, t, 64));
    return f;
}

// ---------------------------------------------------------------------------
// CRC32C of arbitrary byte ranges (WAL entries on replay, raw-file hashes).
// The range [off, off+len) is viewed as whole 256-byte rows starting at the
// row-aligned address a = off & ~255, bytes before off and at/after off+len
// masked to zero.  Leading zeros do not change a zero-init (raw) CRC, so the
// page-kernel chain yields raw(data' || 0^t) = x^(8t) raw(data'), t = pad after
// the range in its last 4 KiB block; multiplying by x^(-8t) removes the pad.  butil's
// init is folded into the data (len >= 4): for a reflected CRC, Value(M) =
// raw(M ^ (~0 || 0...)) ^ ~0, so the first four bytes of the range are XORed
// with 0xFF as they are loaded.  (len < 4: K(len) = ~shift(~0, len) instead.)
//
// Blocks are loaded as buffer loads with an out-of-range offset for rows past
// the range (no branches around them: exact vmcnt waits); the schedule is the
// flat block stream below (range_flat_kernel).
// ---------------------------------------------------------------------------
struct RangeGeo {
    uint64_t a;      // 256-byte-aligned start
    uint64_t lim;    // bytes from a to the range's end
    uint64_t len;
    uint32_t head;   // off - a
    uint32_t rows;   // 256-byte rows from a
    uint32_t nb;     // 4 KiB blocks from a
};
__device__ __forceinline__ RangeGeo range_geo(uint64_t off, uint64_t len) {
    RangeGeo g;
    g.a = off & ~255ull;  // row-aligned: a 256-byte row load touches 2 cache lines, not 3
    g.head = (uint32_t)(off - g.a);
    g.len = len;
    g.lim = len + g.head;
    g.rows = (uint32_t)((g.lim + 255) >> 8);
    g.nb = (g.rows + 15) >> 4;
    return g;
}

// Block k of range g (16 rows, lane l holds dwords l + 64j of the block) into
// w[0..15]; when k is the range's last block, w[16] of lane i < 32 =
// x^(-8t) * x^i, t = the zero pad after the range (the table behind the LDS
// image; one 128-byte load in flight with the block), so the pad is removed by
// a lane-parallel multiply (mul_xinv) instead of a 32-step serial one.
__device__ __forceinline__ void load_range_block(uint32_t (&w)[17], const unsigned char* buf, const RangeGeo& g,
                                                 uint32_t k, uint32_t lane, __amdgpu_buffer_rsrc_t xr,
                                                 bool live = true) {
    // the descriptor's record count ends the block at the range's last dword
    // (rounded up to 4 bytes: a dword that starts inside the range is in
    // bounds, the next one is not, whether the unit tests the dword's start or
    // its end), so rows past the range read 0 with no per-row select
    // (a stream position past the wave's last block -- `live` false -- loads nothing)
    const uint64_t rem = g.lim - ((uint64_t)k << 12);  // > 0 for every block of the range
    const uint32_t nr = !live ? 0u : rem >= 4096u ? 4096u : (((uint32_t)rem + 3u) & ~3u);
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(buf + g.a + ((uint64_t)k << 12)), 0, nr, kBufFlags);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = __builtin_amdgcn_raw_buffer_load_b32(r, 4u * lane + 256u * j, 0, 2);
    const uint32_t xo = (live && k + 1 == g.nb) ? 128u * (uint32_t)(((uint64_t)g.nb << 12) - g.lim) + 4u * (lane & 31u)
                                                : kBufOOB;
    w[16] = __builtin_amdgcn_raw_buffer_load_b32(xr, xo, 0, 0);
}

// Zero the bytes outside the range (first / last dword) and fold butil's init
// into the first four bytes.  Block k; the row/lane tests are per-lane compares.
__device__ __forceinline__ void mask_range_block(uint32_t (&w)[17], const RangeGeo& g, uint32_t k, uint32_t lane) {
    const uint64_t last = g.lim - 1;  // byte offset (from a) of the range's last byte
    const uint32_t tail = (uint32_t)(g.lim & 3u);
    if (tail && k + 1 == g.nb) {  // uniform: only a range's last block has bytes after its end
        const uint32_t mhi = 0xFFFFFFFFu >> (8u * (4u - tail));
        const uint64_t lrow = last >> 8;
        uint32_t rl = lane == (uint32_t)((last >> 2) & 63u) ? (uint32_t)(lrow & 15u) : 0xFFFFu;
        asm volatile("" : "+v"(rl));
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = rl == (uint32_t)j ? w[j] & mhi : w[j];
    }
    if (k == 0) {  // uniform: row 0 holds the bytes before the range (head < 256) and its first 4
        const uint32_t hl = g.head >> 2, hb = g.head & 3u;
        const uint32_t lo = lane < hl ? 0u : (lane == hl ? 0xFFFFFFFFu << (8u * hb) : 0xFFFFFFFFu);
        uint32_t init = 0u, spill = 0u;  // butil's ~0 init over the range's first 4 bytes
        if (g.len >= 4) {
            const uint32_t rest = hb ? 0xFFFFFFFFu >> (8u * (4u - hb)) : 0u;  // bytes of it in the next dword
            init = lane == hl ? 0xFFFFFFFFu << (8u * hb) : (lane == hl + 1 ? rest : 0u);
            spill = (hl == 63u && lane == 0) ? rest : 0u;  // next dword is row 1, lane 0
        }
        w[0] = (w[0] & lo) ^ init;
        w[1] ^= spill;
    }
}

// ---------------------------------------------------------------------------
// Flat block schedule of a range batch (WAL replay, raw-file hashes), ONE
// launch.  The batch is one stream of 4 KiB blocks (range 0's blocks, then
// range 1's, ...), B blocks in all.  The first Bs = B - B/kDynDiv are dealt
// out statically: rounds * W equal pieces, wave w taking pieces w, w + W, ...
// whatever the range sizes.  The last B/kDynDiv blocks are kDynBlocks-block
// chunks handed out through an atomic counter to whichever waves finish first
// (per-wave rates differ by ~7 % -- some XCDs run slower -- so a purely static
// split waits for the slowest wave).
// Where a piece starts comes from kRangeTiles per-tile block counts, held in
// registers by every wave.  The launch computes them itself: wave g counts
// tiles g, g + W, ... and publishes each as one epoch-tagged word (a plain
// device-coherent store: the word carries its own data, so no fence); every
// wave then polls the words of the call's epoch while its workgroup's LDS
// fills.  No wave ever waits on another without a bound: a tile word still
// missing after kTileWaitTicks (a workgroup not resident -- CUs taken by other
// work) is counted by the waiting wave itself from the descriptors.
// A range cut by a piece or chunk boundary is hashed in segments: segment
// [kb, ke) of the range contributes raw(segment || 0-pad) * x^(8 * (lim -
// 4096*ke)) (x^(-8t) for the one that ends the range).  Segments meet in the
// range's accumulator pair acc[2r] (XOR of the contributions) / acc[2r+1]
// (blocks arrived): a segment XORs in, then adds its block count; the one
// whose count completes the range takes the XOR, stores out[r] and leaves the
// pair zero for the next call.  The tail's chunk counter alternates between
// two slots by epoch, each call zeroing the one the next call uses.  A range hashed whole by one wave is stored
// directly; an empty range (V = 0) by the wave that counts its tile.
// ---------------------------------------------------------------------------
constexpr uint64_t kTileWaitTicks = 10000;  // 100 us of s_memrealtime (100 MHz) before a wave counts a tile itself
constexpr uint32_t kEpochShift = 40;        // tile word: epoch << 40 | blocks

// Blocks of tile t (ranges [n t / T, n (t+1) / T)), uniform; zero_empty: store
// V = 0 for the tile's empty ranges.
__device__ __forceinline__ uint64_t range_tile_count(const RangeLaunch& a, uint32_t t, uint32_t lane, bool zero_empty) {
    const uint64_t lo = a.n * t / kRangeTiles, hi = a.n * (t + 1) / kRangeTiles;
    uint64_t sum = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) {
        const RangeDesc d = a.ranges[i];
        sum += d.len ? range_geo(d.off, d.len).nb : 0u;
        if (zero_empty && !d.len) a.out[i] = 0u;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return sum;
}

__device__ __forceinline__ uint64_t wave_scan_incl(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}

// Every tile count of this call into tb (lane l: tiles kTpl*l .. kTpl*l + kTpl-1):
// poll the epoch-tagged words (sc1 loads: a data-tagged granule needs no
// fence).  A tile whose word is still missing after kTileWaitTicks belongs to
// a workgroup that is not running (a kernel on another stream holds the CUs,
// or a CU mask): the waiting wave CLAIMS it -- one CAS of the word to this
// call's tag with kTileClaim set -- counts it with count(t) and publishes the
// count, so each missing tile is counted once, by the first wave to claim it,
// while the others keep polling (round 4 had every waiting wave count every
// missing tile itself: unbounded in practice when many workgroups wait).  The
// owner's own later store writes the same count.  No wave waits on another
// without a bound: every claimed tile is counted by a running wave.
constexpr uint64_t kTileClaim = 1ull << (kEpochShift - 1);  // tile word: claimed, count pending
template <int kTpl, typename Count>
__device__ __forceinline__ void wait_tiles(uint64_t (&tb)[kTpl], uint64_t* tiles, uint64_t tag, uint32_t lane,
                                           Count count) {
    constexpr uint64_t kCountMask = (1ull << kEpochShift) - 1;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint32_t have = 0;  // bit j: tb[j] holds this call's count
    for (;;) {
#pragma unroll
        for (int j = 0; j < kTpl; j++) {
            const uint64_t v = __hip_atomic_load(tiles + kTpl * lane + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool ok = (v & ~kCountMask) == tag && !(v & kTileClaim);
            tb[j] = ok ? v & kCountMask : tb[j];
            have |= ok ? 1u << j : 0u;
        }
        if (!__ballot(have != (1u << kTpl) - 1u)) return;
        if (__builtin_amdgcn_s_memrealtime() - t0 > kTileWaitTicks) {
#pragma unroll
            for (int j = 0; j < kTpl; j++) {
                for (uint64_t m = __ballot(!((have >> j) & 1u)); m; m &= m - 1) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(m);
                    const uint32_t t = kTpl * l + j;
                    uint32_t mine = 0;
                    if (lane == 0) {  // neither published nor claimed this call: claim it
                        const uint64_t cur = __hip_atomic_load(tiles + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        uint64_t exp = cur;
                        mine = (cur & ~kCountMask) != tag &&
                               __hip_atomic_compare_exchange_strong(tiles + t, &exp, tag | kTileClaim,
                                                                    __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (__builtin_amdgcn_readlane(mine, 0)) {
                        const uint64_t cnt = count(t);
                        if (lane == 0) __hip_atomic_store(tiles + t, tag | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        tb[j] = lane == l ? cnt : tb[j];
                        have |= lane == l ? 1u << j : 0u;
                    }
                }
            }
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// The tile holding unit u of the stream, and the units before it: lane tl's
// tiles (cum = inclusive prefix of the lanes' sums), then the first of them
// whose running count passes u.
struct TileHit {
    uint32_t tile;
    uint64_t before;
};
template <int kTpl>
__device__ __forceinline__ TileHit tile_of(uint64_t cum, const uint64_t (&tb)[kTpl], uint64_t u, uint32_t lane) {
    const uint32_t tl = (uint32_t)__builtin_ctzll(__ballot(cum > u));
    TileHit h;
    h.before = tl ? readlane64(cum, tl - 1) : 0;
    h.tile = kTpl * tl;
    bool found = false;
#pragma unroll
    for (int j = 0; j < kTpl; j++) {
        const uint64_t v = readlane64(tb[j], tl);
        if (!found) {
            if (h.before + v > u) {
                found = true;
                h.tile = kTpl * tl + j;
            } else {
                h.before += v;
            }
        }
    }
    return h;
}

constexpr int kFlatWaves = 8;  // waves per CU of the flat range kernel (A/B on WAL sizes: 8 beats 12 by ~4 %, 16 by ~10 %)
constexpr uint32_t kRangeRounds = 1;  // static pieces per wave (round 4, one launch: 1 beats 2 by 0.7 % on random and on equal sizes; 4 +4.7 %, 8 +10.6 %)
constexpr uint64_t kRangeDynDiv = 32;  // 1/32 of the blocks go to the dynamic tail (A/B: 1/8 and 1/16 lose to
                                       // the one counter's atomics, 1/64 leaves tail)
constexpr uint32_t kRangeHeads = 1;    // tail heads (A/B round 3: 8 per-XCD heads = one counter at 1/32)
constexpr uint64_t kRangeDynBlocks = 16;  // blocks per dynamic chunk (A/B: 8 slower, 16 = 32)
__global__ __launch_bounds__(64 * kFlatWaves) void range_flat_kernel(RangeLaunch a) {
    constexpr uint32_t rounds = kRangeRounds;
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t W = (uint64_t)gridDim.x * kFlatWaves;
    const uint64_t w = (uint64_t)blockIdx.x * kFlatWaves + wave;
    const uint64_t tag = (uint64_t)a.epoch << kEpochShift;
    // this wave's tile counts, published before the LDS fill (which hides the
    // stores' and the other workgroups' latency)
    for (uint64_t t = w; t < kRangeTiles; t += W) {
        const uint64_t cnt = range_tile_count(a, (uint32_t)t, lane, true);
        if (lane == 0) __hip_atomic_store(a.tiles + t, tag | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    fill_lds<64 * kFlatWaves>(tab, static_cast<const uint4*>(a.image));
    const unsigned char* __restrict__ buf = a.buf;
    const RangeDesc* __restrict__ ranges = a.ranges;
    const uint64_t n = a.n;
    uint32_t* __restrict__ out = a.out;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4*>(static_cast<const uint4*>(a.image)) + kLdsBytes / 16, 0, kXinvEntries * 128u, kBufFlags);

    // every tile count of this call: lane l holds tiles kTpl*l .. kTpl*l + kTpl-1,
    // cum = inclusive prefix of the lane sums
    constexpr int kTpl = kRangeTiles / 64;
    uint64_t tb[kTpl];
    wait_tiles<kTpl>(tb, a.tiles, tag, lane, [&](uint32_t t) { return range_tile_count(a, t, lane, false); });
    uint64_t lsum = 0;
#pragma unroll
    for (int j = 0; j < kTpl; j++) lsum += tb[j];
    const uint64_t cum = wave_scan_incl(lsum, lane);
    const uint64_t B = readlane64(cum, 63);
    const uint64_t Bs = kRangeDynDiv ? B - B / kRangeDynDiv : B;  // statically dealt blocks
    const uint64_t n_dyn = (B - Bs + kRangeDynBlocks - 1) / kRangeDynBlocks;
    // the tail's counter: slot epoch % 2 of the block; this call zeroes the
    // other slot for the stream's next call (nobody here touches it), so no
    // wave has to count arrivals at the end to reset it
    unsigned long long* dyn_ctr = a.tail + (a.epoch & 1u) * kDynCtrWords64;
    if (blockIdx.x == 0 && threadIdx.x < kRangeHeads)
        atomicExch(a.tail + ((a.epoch + 1u) & 1u) * kDynCtrWords64 + threadIdx.x * kDynHeadStride, 0ull);
    uint32_t dyn_head, dyn_tried;
    tail_cursor<kRangeHeads>(dyn_head, dyn_tried);

    // work items: static pieces item < rounds, then dynamic chunks until the counter runs out
#pragma unroll 1
    for (uint32_t item = 0;; item++) {
        uint64_t b0, b1;
        if (item < rounds) {
            const uint64_t RW = (uint64_t)rounds * W, c = (uint64_t)item * W + w;
            b0 = Bs * c / RW;
            b1 = Bs * (c + 1) / RW;
            if (b0 >= b1) continue;
        } else {
            const uint64_t c = tail_pull<kRangeHeads>(dyn_ctr, n_dyn, dyn_head, dyn_tried, lane);
            if (c >= n_dyn) break;
            b0 = Bs + c * kRangeDynBlocks;
            b1 = b0 + kRangeDynBlocks < B ? b0 + kRangeDynBlocks : B;
        }
        const TileHit th = tile_of(cum, tb, b0, lane);
        const uint32_t tile = th.tile;
        const uint64_t before = th.before;
        // range holding block b0: the tile's ranges 64 at a time
        uint64_t r = n * tile / kRangeTiles;
        uint64_t rel = b0 - before;
        uint32_t k0 = 0;
        // window of 64 descriptors (ranges wb + lane), refilled when passed; the
        // search's last 64 descriptors are the first window (no second load)
        uint64_t wb;
        RangeDesc wd;
        uint64_t wbits;  // lanes of the window holding a range with blocks
        for (;;) {
            const uint64_t ri = r + lane;
            wd = ranges[ri < n ? ri : n - 1];
            const uint64_t nbl = (ri < n && wd.len) ? range_geo(wd.off, wd.len).nb : 0u;
            const uint64_t c = wave_scan_incl(nbl, lane);
            const uint64_t tot = readlane64(c, 63);
            if (rel < tot) {
                const uint32_t h = (uint32_t)__builtin_ctzll(__ballot(c > rel));
                k0 = (uint32_t)(rel - (h ? readlane64(c, h - 1) : 0));
                wb = r;
                wbits = __ballot(ri < n && wd.len != 0);
                r += h;
                break;
            }
            rel -= tot;
            r += 64;
        }
        auto load_window = [&]() {
            const uint64_t ri = wb + lane;
            wd = ranges[ri < n ? ri : n - 1];
            wbits = __ballot(ri < n && wd.len != 0);
        };
        uint64_t left = b1 - b0;  // blocks not yet issued
        struct Pos {
            RangeGeo g;
            uint64_t r;              // range index
            uint32_t k;              // block of the range
            bool real, first, last;  // issued block / first and last block of the item
        };
        auto at = [&](uint64_t ri, uint32_t k) -> Pos {
            Pos p;
            const uint32_t h = (uint32_t)(ri - wb);
            p.g = range_geo(readlane64(wd.off, h), readlane64(wd.len, h));
            p.r = ri;
            p.k = k;
            p.real = true;
            p.first = false;
            p.last = --left == 0;
            return p;
        };
        auto adv = [&](const Pos& p) -> Pos {
            if (!p.real || p.last) {
                Pos q = p;
                q.real = false;
                q.first = q.last = false;
                return q;
            }
            if (p.k + 1 < p.g.nb) {
                Pos q = p;
                q.k = p.k + 1;
                q.first = false;
                q.last = --left == 0;
                return q;
            }
            uint32_t h = (uint32_t)(p.r - wb);
            uint64_t nx = h < 63 ? (wbits & (~0ull << (h + 1))) : 0ull;
            while (!nx) {  // window passed (rare): the next 64 descriptors
                wb += 64;
                load_window();
                nx = wbits;
            }
            return at(wb + (uint64_t)__builtin_ctzll(nx), 0);
        };
        // ring of 4 blocks: three blocks of loads in flight behind the one being folded
        uint32_t A[17], B4[17], Cq[17], Dq[17];
        Pos pA = at(r, k0);
        pA.first = true;
        load_range_block(A, buf, pA.g, pA.k, lane, xr);
        Pos pB = adv(pA);
        load_range_block(B4, buf, pB.g, pB.k, lane, xr, pB.real);
        Pos pC = adv(pB);
        load_range_block(Cq, buf, pC.g, pC.k, lane, xr, pC.real);
        Pos pD = pC;
        uint32_t s = 0;
        uint32_t segk = 0;  // block of the range the current segment began at
        // split-range segments of this item (at most its first and its last):
        // their accumulator atomics return values, and waiting on a returning
        // atomic waits for every load issued before it -- so they run after
        // the ring, when nothing is in flight (inside it: +1.8 % a batch)
        uint64_t seg_r0 = 0, seg_r1 = 0;
        uint32_t seg_v0 = 0, seg_v1 = 0, seg_n0 = 0, seg_n1 = 0, seg_nb0 = 0, seg_nb1 = 0, nseg = 0;
        auto step = [&](uint32_t (&X)[17], const Pos& px, uint32_t (&Y)[17], const Pos& py) {
            load_range_block(Y, buf, py.g, py.k, lane, xr, py.real);
            const RangeGeo& gx = px.g;
            const uint32_t kx = px.k;
            mask_range_block(X, gx, kx, lane);
            const bool start = kx == 0 || px.first;
            if (start) segk = kx;
            s = start ? X[0] : apply_g_xor(tab, s, X[0], c0, c1);
#pragma unroll
            for (int j = 1; j < 16; j++) s = apply_g_xor(tab, s, X[j], c0, c1);
            const bool end = kx + 1 == gx.nb;
            if (end || px.last) {
                const uint32_t raw_pad = wave_xor(apply_fin(tab, s, cf));
                // the item ends inside the range: shift over the range's bytes
                // after this block; a range of < 4 bytes: its K(len) (no folded init)
                const bool pw_needed = !end || gx.len < 4;
                const uint32_t pw =
                    pw_needed ? xpow_wave_small(end ? gx.len << 3 : (gx.lim - ((uint64_t)(kx + 1) << 12)) << 3, lane)
                              : 0u;
                // x^(-8t) * raw_pad = XOR over i of bit (31 - i) of raw_pad ? x^(-8t) x^i : 0
                const uint32_t bit = lane < 32u ? (raw_pad >> (31u - lane)) & 1u : 0u;
                uint32_t v = end ? wave_xor(bit ? X[16] : 0u) : mulmod_small(pw, raw_pad);
                if (end) v ^= gx.len >= 4 ? 0xFFFFFFFFu : ~mulmod_small(pw, 0xFFFFFFFFu);
                if (end && segk == 0) {
                    if (lane == 0) out[px.r] = v;
                } else {  // a segment of a split range: the item's first and/or last, met after the ring
                    // (selects, not an index: a dynamically indexed array lives in scratch)
                    const bool second = nseg != 0;
                    seg_r1 = second ? px.r : seg_r1;
                    seg_v1 = second ? v : seg_v1;
                    seg_n1 = second ? kx + 1 - segk : seg_n1;
                    seg_nb1 = second ? gx.nb : seg_nb1;
                    seg_r0 = second ? seg_r0 : px.r;
                    seg_v0 = second ? seg_v0 : v;
                    seg_n0 = second ? seg_n0 : kx + 1 - segk;
                    seg_nb0 = second ? seg_nb0 : gx.nb;
                    nseg++;
                }
            }
        };
        for (;;) {
            if (!pA.real) break;
            pD = adv(pC);
            step(A, pA, Dq, pD);
            if (!pB.real) break;
            pA = adv(pD);
            step(B4, pB, A, pA);
            if (!pC.real) break;
            pB = adv(pA);
            step(Cq, pC, B4, pB);
            if (!pD.real) break;
            pC = adv(pB);
            step(Dq, pD, Cq, pC);
        }
        // the item's split segments meet in their ranges' accumulator pairs:
        // XOR in, then add the blocks; the add that completes the range takes
        // the XOR, stores it and leaves the pair zero
        auto meet = [&](uint64_t r, uint32_t v, uint32_t nblk, uint32_t nb) {
            uint32_t* acc = a.acc + 2 * r;
            const uint32_t x = atomicXor(acc, v);
            asm volatile("" ::"v"(x) : "memory");  // the XOR is performed before the count says so
            if (atomicAdd(acc + 1, nblk) + nblk == nb) {
                out[r] = atomicExch(acc, 0u);
                atomicExch(acc + 1, 0u);
            }
        };
        if (lane == 0 && nseg > 0) meet(seg_r0, seg_v0, seg_n0, seg_nb0);
        if (lane == 0 && nseg > 1) meet(seg_r1, seg_v1, seg_n1, seg_nb1);
    }
}

// Fast path: per_group = 64*q.  One wave per group, grid-stride over groups;
// lane l folds units [l*q, (l+1)*q) by Horner with the constant multiplier
// m_unit applied through a 4 x 256-entry product table in LDS (4 lookups +
// 2 v_bitop3 instead of a 32-step multiply), then a 6-level shuffle tree merges
// lanes (one multiply per level).
__global__ __launch_bounds__(256) void fold_kernel_wave(const uint32_t* __restrict__ crcs, uint64_t n_groups,
                                                        uint32_t per_group, FoldLaunch a,
                                                        uint32_t* __restrict__ out) {
    __shared__ uint32_t mt[4][256];
    for (uint32_t i = threadIdx.x; i < 1024; i += 256) mt[i >> 8][i & 255] = mulmod_dev(a.m_unit, (i & 255u) << (8 * (i >> 8)));
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = per_group >> 6;
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += (uint64_t)gridDim.x * 4) {
        const uint32_t* p = crcs + g * per_group + (uint64_t)lane * q;
        uint32_t s = p[0];
        for (uint32_t i = 1; i < q; i++) {
            const uint32_t t = __builtin_amdgcn_bitop3_b32(mt[0][s & 255u], mt[1][(s >> 8) & 255u],
                                                           mt[2][(s >> 16) & 255u], 0x96);
            s = __builtin_amdgcn_bitop3_b32(t, mt[3][s >> 24], p[i], 0x96);
        }
#pragma unroll
        for (int t = 0; t < 6; t++) {
            const uint32_t other = __shfl_down(s, 1u << t, 64);
            if ((lane & ((2u << t) - 1u)) == 0) s = mulmod_dev(a.m_tree[t], s) ^ other;
        }
        if (lane == 0) out[g] = s;
    }
}

// ---------------------------------------------------------------------------
// Fused scan epilogue (one launch per batch instead of fold + fold + combine +
// digest): block b = chunk b, 256 threads.  Thread t loads its q page CRCs
// (coalesced), folds them by Horner through an LDS product table of
// x^(8*page_bytes), then a combine tree over threads (shuffles inside a wave,
// LDS across the 4 waves): after slice_shift levels thread (k << slice_shift)
// holds slice k's CRC (ScanMap.crc), after 8 levels thread 0 holds the chunk
// data CRC -> file CRC = combine(metapage CRC, data CRC, chunk_bytes) -> digest
// contribution atomicXor'ed into its copyset.
// ---------------------------------------------------------------------------
// multiply by a constant through its 4 x 256 product table (global, L1-resident)
__device__ __forceinline__ uint32_t mul_tab(const uint32_t* __restrict__ t, uint32_t s) {
    return __builtin_amdgcn_bitop3_b32(
        __builtin_amdgcn_bitop3_b32(t[s & 255u], t[256 + ((s >> 8) & 255u)], t[512 + ((s >> 16) & 255u)], 0x96),
        t[768 + (s >> 24)], 0u, 0x96);
}

__global__ __launch_bounds__(256) void epilogue_kernel(EpilogueLaunch a) {
    __shared__ uint32_t mt[1024];  // x^(8 page_bytes) product table (Horner), copied once per block
    __shared__ uint32_t part[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    for (uint32_t i = t; i < 1024; i += 256) mt[i] = a.mtab[i];
    __syncthreads();
    const uint32_t slices = 256u >> a.slice_shift;
    const uint32_t* lvl = a.mtab + 1024;           // level k table at lvl + 1024 k
    const uint32_t* chk = a.mtab + 9 * 1024;
    for (uint64_t c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
        const uint32_t* p = a.page_crcs + c * a.pages_per_chunk + (uint64_t)t * a.q;
        auto horner = [&](uint32_t s, uint32_t w) {
            const uint32_t u = __builtin_amdgcn_bitop3_b32(mt[s & 255u], mt[256 + ((s >> 8) & 255u)],
                                                           mt[512 + ((s >> 16) & 255u)], 0x96);
            return __builtin_amdgcn_bitop3_b32(u, mt[768 + (s >> 24)], w, 0x96);
        };
        uint32_t s;
        if (a.q == 16 && ((uintptr_t)a.page_crcs & 15u) == 0) {
            // 16 MiB chunks of 4 KiB pages: the thread's 64 B in four 16-byte loads, all in flight
            uint4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = reinterpret_cast<const uint4*>(p)[k];
            s = v[0].x;
            s = horner(s, v[0].y);
            s = horner(s, v[0].z);
            s = horner(s, v[0].w);
#pragma unroll
            for (int k = 1; k < 4; k++) {
                s = horner(s, v[k].x);
                s = horner(s, v[k].y);
                s = horner(s, v[k].z);
                s = horner(s, v[k].w);
            }
        } else {
            s = p[0];
            for (uint32_t i = 1; i < a.q; i++) s = horner(s, p[i]);
        }
        if (a.slice_shift == 0) a.slice_crcs[c * 256 + t] = s;  // one thread per slice
        // levels 0..5 inside the wave
#pragma unroll
        for (uint32_t k = 0; k < 6; k++) {
            const uint32_t other = __shfl_down(s, 1u << k, 64);
            if ((lane & ((2u << k) - 1u)) == 0) s = mul_tab(lvl + 1024 * k, s) ^ other;
            if (k + 1 == a.slice_shift && (t & ((2u << k) - 1u)) == 0) a.slice_crcs[c * slices + (t >> a.slice_shift)] = s;
        }
        // levels 6..7 across the 4 waves
        if (lane == 0) part[wv] = s;
        __syncthreads();
        if (t == 0) {
            const uint32_t w0 = mul_tab(lvl + 6 * 1024, part[0]) ^ part[1];
            const uint32_t w1 = mul_tab(lvl + 6 * 1024, part[2]) ^ part[3];
            if (a.slice_shift == 7) {
                a.slice_crcs[c * 2] = w0;
                a.slice_crcs[c * 2 + 1] = w1;
            }
            const uint32_t data = mul_tab(lvl + 7 * 1024, w0) ^ w1;
            if (a.slice_shift == 8) a.slice_crcs[c] = data;
            const uint32_t file = mul_tab(chk, a.meta_crcs[c]) ^ data;
            if (a.file_crcs) a.file_crcs[c] = file;
            if (a.digest) atomicXor(a.digest + a.group[c], mulmod_dev(a.after_mult[c], file));
        }
        __syncthreads();
    }
}

__global__ void xpow8_kernel(const uint64_t* __restrict__ nbytes, uint64_t n, uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * 4) {
        const uint32_t m = xpow_wave(nbytes[i] << 3, lane);
        if (lane == 0) out[i] = m;
    }
}

// Generic path: one thread per group, serial combine.
__global__ void fold_kernel_serial(const uint32_t* __restrict__ crcs, uint64_t n_groups, uint32_t per_group,
                                   uint32_t m_unit, uint32_t* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t* p = crcs + g * per_group;
    uint32_t s = per_group ? p[0] : 0u;
    for (uint32_t i = 1; i < per_group; i++) s = mulmod_dev(m_unit, s) ^ p[i];
    out[g] = s;
}

__global__ void shift_kernel(const uint32_t* __restrict__ crcs, const uint64_t* __restrict__ nbytes, uint64_t n,
                             uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = crcs[i];
    const uint64_t nb = nbytes[i];
    out[i] = (c == 0u || nb == 0u) ? c : mulmod_dev(xpow_dev(nb << 3), c);
}

// ---------------------------------------------------------------------------
// Write-log path (cc_apply_log_dev): ordering on the device, no host planning.
// ---------------------------------------------------------------------------
// Grouping by page without a sort.  Piece t = (update t / slots, its k-th page,
// k = t % slots).  Every piece inserts its page into an open-addressing table
// (linear probing, <= 12.5 % load: >= 8 x pieces, engine.hip) whose 64-bit entry holds {page + 1, piece + 1}
// of the page's most recently inserted piece: one CAS both claims the page and
// pushes the piece onto the page's list (next[piece] = the previous head).
// The piece that claims an empty entry appends the entry's slot to the head
// list (one atomic per wave).  The list order is arbitrary; the page kernel
// restores log order from the update indices.  An update that breaks the
// contract (len 0, len > max_len, beyond the pool) produces no pieces and is
// not applied at all (never half-applied).  The table and the counters were
// zeroed earlier on the stream.
__device__ __forceinline__ uint32_t page_hash(uint32_t page, uint32_t mask) {
    return (page * 2654435761u) & mask;  // Fibonacci hashing; sequential pages spread
}

// Piece t of the log (t >= n_pieces: none) into the table; its head record,
// if it claims a page, goes to the block's own segment (no global counter: a
// per-wave atomic on one counter serialised 2,048 waves, 26 of the kernel's 31
// us, and even one per block was a returning atomic on the critical path).
// Every thread of the block calls it; `wcount` = LDS scratch of blockDim/64 + 1
// words; `used` = the segment's records so far (uniform), advanced here.
// (A = LogLaunch for log_insert_kernel, LogInsert for the next batch's grouping
// inside log_pages_kernel: the same field names.)
template <class A>
__device__ __forceinline__ void insert_piece(const A& a, uint64_t t, uint32_t* wcount, uint32_t& used) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    bool fresh = false;
    uint32_t slot = 0;
    if (t < a.n_pieces) {
        const uint64_t i = t / a.slots;
        const uint32_t k = (uint32_t)(t - i * a.slots);
        const UpdateDesc d = a.upd[i];
        const bool ok = d.len >= 1 && d.len <= a.max_len && d.dst < a.pool_bytes && d.len <= a.pool_bytes - d.dst;
        const uint64_t p0 = ok ? d.dst / a.page_bytes : 0;
        const uint64_t p1 = ok ? (d.dst + d.len - 1) / a.page_bytes : 0;
        if (ok && p0 + k <= p1) {
            const uint32_t page = (uint32_t)(p0 + k);
            const unsigned long long tag = (unsigned long long)(page + 1u) << 32;
            unsigned long long* tab = reinterpret_cast<unsigned long long*>(a.table);
            slot = page_hash(page, a.table_mask);
            // CAS first (one atomic for a page seen first, the common case);
            // next[] is only read by later kernels, so it can follow the CAS
            unsigned long long cur = 0ull;
            for (;;) {
                const unsigned long long old = atomicCAS(tab + slot, cur, tag | (unsigned long long)(t + 1));
                if (old == cur) {  // claimed (cur == 0) or pushed onto the page's list
                    a.next[t] = cur ? (uint32_t)cur - 1u : kNoPiece;
                    fresh = cur == 0ull;
                    break;
                }
                if (old == 0ull || (old & 0xFFFFFFFF00000000ull) == tag) {
                    cur = old;  // the page's entry (or an empty one): retry against it
                    continue;
                }
                slot = (slot + 1u) & a.table_mask;  // another page: probe on, expecting empty
                cur = 0ull;
            }
        }
    }
    const uint64_t m = __ballot(fresh);
    if (lane == 0) wcount[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = used, tot = 0;
    for (uint32_t w = 0; w < nw; w++) {
        base += w < wv ? wcount[w] : 0u;
        tot += wcount[w];
    }
    used += tot;
    // the head record: the page's table slot and the claiming piece (the list's
    // tail: a page whose entry still names it has no other piece)
    if (fresh)
        reinterpret_cast<uint2*>(a.heads)[(uint64_t)blockIdx.x * a.seg_cap + base +
                                          (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = make_uint2(slot, (uint32_t)t);
    __syncthreads();  // wcount reused by the next chunk
}

// Block b inserts chunks b, b + grid, ... of kInsertThreads pieces into its
// head segment and leaves its record count in seg_count[b].
__global__ __launch_bounds__(kInsertThreads) void log_insert_kernel(LogLaunch a) {
    __shared__ uint32_t wcount[kInsertThreads / 64 + 1];
    if (a.zero_ctrs && blockIdx.x == 0 && threadIdx.x < 3) a.zero_ctrs[threadIdx.x] = 0ull;  // the queue's counters
    uint32_t used = 0;
    const uint64_t chunks = (a.n_pieces + kInsertThreads - 1) / kInsertThreads;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x)
        insert_piece(a, c * kInsertThreads + threadIdx.x, wcount, used);
    if (threadIdx.x == 0) a.seg_count[blockIdx.x] = used;
}

// The bytes of one update that fall inside one page, page-relative: page bytes
// [rlo, rhi); the source byte of page byte r is sp[r] (sp is uniform, so every
// load below is an SGPR base + the lane's 32-bit offset + an immediate).
struct Piece {
    uint32_t rlo, rhi;
    const unsigned char* sp;
};
__device__ __forceinline__ Piece piece_in_page(uint64_t pbase, uint32_t page_bytes, uint64_t dst, uint64_t src,
                                               uint32_t len, const unsigned char* __restrict__ srcbuf) {
    Piece p;
    const uint64_t end = dst + len, pend = pbase + page_bytes;
    p.rlo = (uint32_t)((dst > pbase ? dst : pbase) - pbase);
    p.rhi = (uint32_t)((end < pend ? end : pend) - pbase);
    p.sp = srcbuf + (src - dst) + pbase;  // modular: only sp[r], r in [rlo, rhi), is ever dereferenced
    return p;
}

// Source bytes of one piece in the layout of the page registers (lane l holds
// page dwords l + 64j, i.e. page byte r = 4l + 256j), fetched with buffer
// loads: a lane that needs nothing passes an out-of-range offset, which the
// buffer unit answers with 0 without touching memory.  So every load is issued
// unconditionally (no branches around loads: hipcc's vmcnt counts stay exact
// and the next page's fetch really overlaps this page's merge + hash) and no
// byte outside the update's source range is ever read.  A dword the piece
// covers WHOLLY is one unaligned buffer_load_dword (gfx950 serves unaligned
// dword loads).  The at most two partially covered dwords (the piece's first
// and last) are spliced from the aligned source dwords holding their needed
// bytes, kept in 4 edge registers instead of a second [M] array.

template <int M>
struct PieceSrc {
    uint32_t S[M];
    uint32_t ea[2], eb[2];  // aligned source dwords holding edge dword k's bytes
};

// page dword index of the partially covered first / last dword (none = 0xffffffff)
__device__ __forceinline__ void piece_edges(const Piece& p, uint32_t (&e)[2]) {
    const uint32_t df = p.rlo >> 2, dl = (p.rhi - 1) >> 2;
    const bool ff = (p.rlo & 3u) == 0 && 4 * df + 4 <= p.rhi;
    const bool fl = (p.rhi & 3u) == 0 && 4 * dl >= p.rlo;
    e[0] = ff ? 0xffffffffu : df;
    e[1] = (dl != df && !fl) ? dl : 0xffffffffu;
}

// Row structure of a piece (wave-uniform).  Row j = page bytes [256j, 256j+256)
// = dword l + 64j of every lane.  A piece is one contiguous byte range, so it
// touches rows [row0, row1] (the rows it dirties; in delta mode the rows read).
struct PieceRows {
    uint32_t row0, row1;
};
__device__ __forceinline__ PieceRows piece_rows(const Piece& p) {
    return {p.rlo >> 8, (p.rhi - 1) >> 8};
}

// Per-lane position of a piece: x_j = (page byte of the lane's row-j dword) -
// rlo, in wrapping 32-bit arithmetic, so "dword wholly inside the piece" is ONE
// unsigned compare per row, x_j < len - 3 (a dword below rlo wraps to >= 2^31),
// on the vector unit: no per-row scalar masks or uniform row selects.
struct PieceLane {
    uint32_t o;   // 4 * lane - rlo (wrapping)
    uint32_t l3;  // len - 3 if len >= 4, else 0 (no whole dword)
};
__device__ __forceinline__ PieceLane piece_lane(const Piece& p, uint32_t lane) {
    const uint32_t len = p.rhi - p.rlo;
    return {lane * 4u - p.rlo, len >= 4u ? len - 3u : 0u};
}

template <int M>
__device__ __forceinline__ void fetch_piece(PieceSrc<M>& r, const Piece& p, uint32_t lane) {
    const uint32_t sh = (uint32_t)(uintptr_t)p.sp & 3u;  // the same for every dword of the piece
    // whole dwords: base sp, offset = page byte; edges: aligned base sp - sh
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.sp), 0, 64u * 4u * M + 8u, kBufFlags);
    const __amdgpu_buffer_rsrc_t re =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.sp - sh), 0, 64u * 4u * M + 8u, kBufFlags);
    const uint32_t l4 = lane * 4u;
    const PieceLane pl = piece_lane(p, lane);
#pragma unroll
    for (int j = 0; j < M; j++) {
        const bool full = pl.o + 256u * j < pl.l3;
        r.S[j] = __builtin_amdgcn_raw_buffer_load_b32(
            rw, row_sel(full ? l4 : kBufOOB) + 256u * j, 0, 0);
    }
    uint32_t e[2];
    piece_edges(p, e);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t b = 4 * (e[k] & 0x3fffffffu);
        const bool mine = e[k] != 0xffffffffu && lane == (e[k] & 63u);
        const uint32_t k0 = p.rlo > b ? p.rlo - b : 0u;
        const uint32_t k1 = p.rhi < b + 4 ? p.rhi - b : 4u;
        r.ea[k] = __builtin_amdgcn_raw_buffer_load_b32(re, (mine && k0 < 4u - sh) ? b : kBufOOB, 0, 0);
        r.eb[k] = __builtin_amdgcn_raw_buffer_load_b32(re, (mine && sh && k1 > 4u - sh) ? b + 4 : kBufOOB, 0, 0);
    }
}

// Whole dwords: one compare + select per row, on the vector unit.  The <= 2
// partially covered dwords (the piece's first and last: each is one lane in
// one row) are spliced under their byte mask; the owning lane carries the row
// index, so each row costs a compare + select and there are no lane or row
// branches.  `dirty` (rows written) is uniform.
template <int M>
__device__ __forceinline__ void merge_piece(uint32_t (&w)[M], uint32_t& dirty, const PieceSrc<M>& r, const Piece& p,
                                            uint32_t lane) {
    const PieceLane pl = piece_lane(p, lane);
#pragma unroll
    for (int j = 0; j < M; j++) w[j] = pl.o + 256u * j < pl.l3 ? r.S[j] : w[j];
    uint32_t e[2];
    piece_edges(p, e);
    const uint32_t sh = (uint32_t)(uintptr_t)p.sp & 3u;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t v = sh ? __builtin_amdgcn_alignbyte(r.eb[k], r.ea[k], sh) : r.ea[k];
        const uint32_t b = 4 * (e[k] & 0x3fffffffu);
        const uint32_t k0 = p.rlo > b ? p.rlo - b : 0u;
        const uint32_t k1 = p.rhi < b + 4 ? p.rhi - b : 4u;
        const uint32_t mhi = k1 >= 4u ? 0xFFFFFFFFu : (1u << (8u * k1)) - 1u;
        const uint32_t mask = mhi & ~((1u << (8u * (k0 & 3u))) - 1u);  // uniform
        // row of edge k on its lane; no row elsewhere (or when there is no edge k)
        uint32_t row = (e[k] != 0xffffffffu && lane == (e[k] & 63u)) ? e[k] >> 6 : 0xFFFFu;
        asm volatile("" : "+v"(row));  // keep the per-row test one vector compare (not a scalar compare + mask)
#pragma unroll
        for (int j = 0; j < M; j++) w[j] = row == (uint32_t)j ? (v & mask) | (w[j] & ~mask) : w[j];
    }
    const PieceRows pr = piece_rows(p);
    const uint32_t top = pr.row1 >= 31 ? 0xFFFFFFFFu : (2u << pr.row1) - 1u;
    dirty |= top & ~((1u << pr.row0) - 1u);
}


// Full-mode fast path for a page with ONE piece (the common case).  Every row
// is, uniformly, untouched (read from the page), covered whole by the piece
// (read from the source: that row's buffer descriptor is the source's, chosen
// by a scalar select, with the same vector offset), or an edge row -- the
// first / last touched row when the piece starts / ends inside it (read from
// the page; its source dwords are fetched on their own and merged).  So no row
// but the <= 2 edge rows costs a vector compare or select (the generic path
// spends ~12 VALU a row on them: 411 VALU a page, the kernel's issue bound).
struct PieceEdges {
    uint32_t r[2];          // edge rows (uniform; kNoRow = none)
    uint32_t s[2];          // the lane's source dword in edge row q, if wholly inside the piece
    uint32_t ea[2], eb[2];  // the partially covered dwords' aligned source dwords (as PieceSrc)
};
constexpr uint32_t kNoRow = 0xFFFFu;

__device__ __forceinline__ void edge_rows(const Piece& p, uint32_t (&r)[2]) {
    const uint32_t row0 = p.rlo >> 8, row1 = (p.rhi - 1) >> 8;
    r[0] = (p.rlo & 255u) ? row0 : kNoRow;
    r[1] = ((p.rhi & 255u) && row1 != r[0]) ? row1 : kNoRow;
}

__device__ __forceinline__ uint32_t covered_rows(const Piece& p) {  // rows [f0, f1) the piece covers whole
    const uint32_t f0 = (p.rlo + 255u) >> 8, f1 = p.rhi >> 8;
    return f1 > f0 ? ((f1 >= 32u ? 0xFFFFFFFFu : (1u << f1) - 1u) & ~((1u << f0) - 1u)) : 0u;
}

template <int M>
__device__ __forceinline__ void load_rows_sel(uint32_t (&w)[M], const unsigned char* page, const unsigned char* sp,
                                              uint32_t cov, uint32_t lane) {
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(page), 0, 256u * M,
                                                                         kBufFlags);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(sp), 0, 256u * M,
                                                                         kBufFlags);
#pragma unroll
    for (int j = 0; j < M; j++)
        w[j] = __builtin_amdgcn_raw_buffer_load_b32(((cov >> j) & 1u) ? rs : rp, row_sel(4u * lane) + 256u * j, 0,
                                                    kLogRowAux);
}

template <int M>
__device__ __forceinline__ void fetch_edges(PieceEdges& r, const Piece& p, uint32_t lane) {
    const uint32_t sh = (uint32_t)(uintptr_t)p.sp & 3u;
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.sp), 0, 64u * 4u * M + 8u, kBufFlags);
    const __amdgpu_buffer_rsrc_t re =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.sp - sh), 0, 64u * 4u * M + 8u, kBufFlags);
    edge_rows(p, r.r);
    const PieceLane pl = piece_lane(p, lane);
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const bool in = r.r[q] != kNoRow && pl.o + 256u * r.r[q] < pl.l3;
        r.s[q] = __builtin_amdgcn_raw_buffer_load_b32(rw, in ? 4u * lane + 256u * r.r[q] : kBufOOB, 0, 0);
    }
    uint32_t e[2];
    piece_edges(p, e);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t b = 4 * (e[k] & 0x3fffffffu);
        const bool mine = e[k] != 0xffffffffu && lane == (e[k] & 63u);
        const uint32_t k0 = p.rlo > b ? p.rlo - b : 0u;
        const uint32_t k1 = p.rhi < b + 4 ? p.rhi - b : 4u;
        r.ea[k] = __builtin_amdgcn_raw_buffer_load_b32(re, (mine && k0 < 4u - sh) ? b : kBufOOB, 0, 0);
        r.eb[k] = __builtin_amdgcn_raw_buffer_load_b32(re, (mine && sh && k1 > 4u - sh) ? b + 4 : kBufOOB, 0, 0);
    }
}

// w: rows loaded by load_rows_sel (covered rows already hold the new bytes)
template <int M>
__device__ __forceinline__ void merge_edges(uint32_t (&w)[M], uint32_t& dirty, const PieceEdges& r, const Piece& p,
                                            uint32_t lane) {
    const PieceLane pl = piece_lane(p, lane);
    uint32_t e[2];
    piece_edges(p, e);
    const uint32_t sh = (uint32_t)(uintptr_t)p.sp & 3u;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const uint32_t rq = r.r[q];
        if (rq == kNoRow) continue;  // uniform
        uint32_t v = w[rq];          // uniform dynamic row index
        v = pl.o + 256u * rq < pl.l3 ? r.s[q] : v;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (e[k] == 0xffffffffu || (e[k] >> 6) != rq) continue;  // uniform
            const uint32_t spl = sh ? __builtin_amdgcn_alignbyte(r.eb[k], r.ea[k], sh) : r.ea[k];
            const uint32_t b = 4 * e[k];
            const uint32_t k0 = p.rlo > b ? p.rlo - b : 0u;
            const uint32_t k1 = p.rhi < b + 4 ? p.rhi - b : 4u;
            const uint32_t mhi = k1 >= 4u ? 0xFFFFFFFFu : (1u << (8u * k1)) - 1u;
            const uint32_t mask = mhi & ~((1u << (8u * (k0 & 3u))) - 1u);
            v = lane == (e[k] & 63u) ? (spl & mask) | (v & ~mask) : v;
        }
        w[rq] = v;
    }
    const PieceRows pr = piece_rows(p);
    const uint32_t top = pr.row1 >= 31 ? 0xFFFFFFFFu : (2u << pr.row1) - 1u;
    dirty |= top & ~((1u << pr.row0) - 1u);
}

// One wave per touched page, balanced: wave w owns heads w, w + W, w + 2W, ...
// (W = waves in the grid), ~pages/W each.  Its lanes load the metadata of up to
// 64 of its heads at once (table entry: page + one piece, that piece's list
// link and update descriptor: a few round trips per 64 pages), then the wave
// software-pipelines them: while page k's pieces are merged, stored and
// hashed, page k+1's data AND the source bytes of its piece are in flight.  A
// page with several pieces (overlapping / neighbouring writes: rare) walks its
// list, ranks the pieces by update index and applies them in log order; for
// a page with more than 64 (a log hammering it) the wave replays the whole log
// in place.  Every page is owned by exactly one wave: no write races, no
// flags, no atomics on the data.
// Delta mode (cc_apply_log_delta_dev): the stored CRC of each touched page is
// taken as the CRC of its bytes before the batch and updated through
// linearity, V(new) = V(old) ^ raw0(old ^ new) (equal lengths: the init and
// xorout terms cancel), so only the rows the page's pieces touch are read --
// untouched rows get an out-of-range buffer offset (0, no memory traffic) and
// contribute 0 to old ^ new.  A page with several pieces reads all rows.
// Bit-identical to the full rehash whenever the stored CRC matched the page;
// if it did not (latent corruption), the mismatch survives the write instead
// of being laundered into a fresh CRC.
template <int M>
__device__ __forceinline__ void load_rows(uint32_t (&w)[M], const unsigned char* page, uint32_t rows, uint32_t lane) {
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(page), 0, 256u * M,
                                                                         kBufFlags);
#pragma unroll
    for (int j = 0; j < M; j++)
        w[j] = __builtin_amdgcn_raw_buffer_load_b32(rp, row_sel(((rows >> j) & 1u) ? 4u * lane : kBufOOB) + 256u * j, 0, 2);
}

// cc_apply_logs_dev: the next batch's grouping in this page kernel's tail.  A
// workgroup whose waves are all done with their pages (its LDS image no longer
// read: the insert's scratch) takes kGroupTake chunks of 64*WV pieces at a time
// from one counter until none is left or it holds `rounds` of them (its head
// segment's bound);
// the workgroups that finish first take them while the slow ones finish, so
// the grouping costs no kernel time and no launch.  Every workgroup stores its
// segment's count.  Block 0 zeroes the counter the grouping after next uses
// (the one before this used it; it has completed).
template <int WV>
__device__ __forceinline__ void group_next(const LogInsert& nx, uint32_t* tab) {
    if (!nx.n_pieces) return;  // uniform
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(nx.zero, 0ull);
    __syncthreads();  // every wave of the workgroup is past its pages
    constexpr uint32_t T = 64u * WV;
    const uint64_t chunks = (nx.n_pieces + T - 1) / T;
    uint32_t used = 0;
    for (uint32_t r = 0; r + kGroupTake <= nx.rounds; r += kGroupTake) {
        if (threadIdx.x == 0) tab[T] = (uint32_t)atomicAdd(nx.take, 1ull);  // (< 2^32 takes: n_pieces < 2^31)
        __syncthreads();
        const uint64_t c = (uint64_t)kGroupTake * tab[T];
        if (c >= chunks) break;  // uniform
        for (uint32_t i = 0; i < kGroupTake && c + i < chunks; i++)
            insert_piece(nx, (c + i) * T + threadIdx.x, tab, used);  // ends with a barrier: tab[T] free again
    }
    if (threadIdx.x == 0) nx.seg_count[blockIdx.x] = used;
}

template <int M, bool Delta>
__device__ __forceinline__ void log_pages_body(const LogLaunch& a, uint32_t* tab) {
    constexpr int WV = log_waves(M, Delta);
    // the insert blocks' segment counts: lane l holds segments 4l .. 4l+3,
    // scum = inclusive prefix of the lanes' sums; head h (in segment order) is
    // record h - (heads before its segment) of its segment
    constexpr int kSpl = kInsertBlocks / 64;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t sc[kSpl];  // (32-bit: these stay live over the page loop)
#pragma unroll
    for (int j = 0; j < kSpl; j++) {
        const uint32_t sg = kSpl * lane + j;
        sc[j] = sg < a.n_segs ? a.seg_count[sg] : 0u;
    }
    uint32_t ssum = 0;
#pragma unroll
    for (int j = 0; j < kSpl; j++) ssum += sc[j];
    uint32_t scum = ssum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(scum, d, 64);
        if (lane >= (uint32_t)d) scum += o;
    }
    // an equal share of the heads per workgroup: [hb0, hb1); a workgroup without
    // one (a small log) leaves before filling its 160 KiB of LDS
    const uint32_t Hall = __builtin_amdgcn_readlane(scum, 63);
    const uint32_t hb0 = (uint32_t)((uint64_t)Hall * blockIdx.x / gridDim.x);
    const uint32_t hb1 = (uint32_t)((uint64_t)Hall * (blockIdx.x + 1) / gridDim.x);
    if (hb0 >= hb1) {
        group_next<WV>(a.nx, tab);
        return;
    }
    fill_lds<64 * WV>(tab, static_cast<const uint4*>(a.image));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    constexpr uint32_t pb = 256u * M;  // = a.page_bytes (launch_log_pages picks M = page_bytes / 256): shifts, not 64-bit multiplies
    // The workgroup's heads are cut among its waves by age.  Its waves sit 4 to a
    // SIMD (wave t on SIMD t % 4, the (t / 4)-th oldest there) and the SIMD
    // issues oldest-first: with equal shares the four age groups ended at 80, 92,
    // 103 and 113 us (per-wave clocks, scripts/trace_log.py) and the workgroup
    // ran its last ~30 us with fewer waves than pages in flight.  Shares
    // weighted by age group (kSkew[t / 4]) end them within ~10 us of each other:
    // -3 % a batch (a priority that rotates every step instead: -1.5 %).  A/B
    // (profiles/write_log_skew_ab_r03.txt): 33/27/22/18 = 32/28/22/18 =
    // 34/26/22/18 < 30/26/23/21 < 28/26/24/22 < 36/28/21/15 < equal.
    constexpr uint32_t kSkew[4] = {33, 27, 22, 18};
    auto wprefix = [&](uint32_t t) {  // sum of the weights of waves 0 .. t-1
        uint32_t p = 0;
        for (uint32_t u = 0; u < t; u++) p += kSkew[(u / 4) & 3];
        return p;
    };
    const uint32_t Hb = hb1 - hb0, wsum = wprefix(WV);
    const uint32_t H = hb0 + (uint32_t)((uint64_t)Hb * wprefix(wave + 1) / wsum);  // this wave: [first, H)
    const uint32_t first = hb0 + (uint32_t)((uint64_t)Hb * wprefix(wave) / wsum);
    constexpr uint32_t W = 1;  // lane k <- head base + k
    // static shares only: a dynamic tail (the last 1/8 or 1/16 of the heads in
    // chunks of 4-16 through one atomic counter, as the page kernel does) measured
    // 7-19 % slower here (0.177-0.197 vs 0.165 ms a batch)
    for (uint32_t base = first; base < H; base += 64u * W) {
        // lane k <- head base + k*W (clamped loads: no branches around them)
        const uint64_t ih = (uint64_t)base + (uint64_t)lane * W;
        const bool hv = ih < H;
        // the lane's head in its segment: the segment holding head `base` (lane
        // tl's segments, then the first of them past it), then a walk over the
        // (few) segments the batch spans
        const uint32_t hi = hv ? (uint32_t)ih : base;
        uint32_t seg, sbefore;
        {
            const uint32_t tl = (uint32_t)__builtin_ctzll(__ballot(scum > base));
            uint32_t st = tl ? __builtin_amdgcn_readlane(scum, tl - 1) : 0u, s = kSpl * tl;
            bool found = false;
#pragma unroll
            for (int j = 0; j < kSpl; j++) {
                const uint32_t v = __builtin_amdgcn_readlane(sc[j], tl);
                if (!found) {
                    if (st + v > base) {
                        found = true;
                        s = kSpl * tl + j;
                    } else {
                        st += v;
                    }
                }
            }
            seg = s;
            sbefore = st;
            const uint32_t last = base + 63u < H - 1u ? base + 63u : H - 1u;
            for (;;) {
                uint32_t v = sc[0];
#pragma unroll
                for (int j = 1; j < kSpl; j++) v = (s % kSpl) == (uint32_t)j ? sc[j] : v;
                const uint32_t cnt = __builtin_amdgcn_readlane(v, s / kSpl);
                if (st + cnt > last || s + 1 >= a.n_segs) break;
                st += cnt;
                s++;
                seg = hi >= st ? s : seg;
                sbefore = hi >= st ? st : sbefore;
            }
        }
        // the head record gives the table slot AND the claiming piece, so the
        // claimer's descriptor loads beside the table entry: two dependent
        // round trips to a page's geometry instead of three (the list link is
        // needed by pages with several pieces only, far behind)
        const uint2 hrec = reinterpret_cast<const uint2*>(a.heads)[(uint64_t)seg * a.seg_cap + (hi - sbefore)];
        const uint32_t hslot = hrec.x, claimer = hrec.y;
        const unsigned long long ent = reinterpret_cast<const unsigned long long*>(a.table)[hslot];
        const UpdateDesc d = a.upd[claimer / a.slots];
        if (a.clear_table && hv) a.table[hslot] = 0ull;  // the slot is this lane's alone (one head per page)
        const uint32_t key = (uint32_t)(ent >> 32) - 1u;  // the page
        const uint32_t pfirst = (uint32_t)ent - 1u;       // the list head (the latest piece)
        const uint32_t nxt = a.next[pfirst];              // consumed by the several-piece path only
        const uint32_t u0 = pfirst / a.slots;  // the head piece's update
        // the claimer's geometry in its page (the only piece when single), packed:
        // rlo | rhi << 16 and the source pointer (3 VGPRs instead of the 5 of its descriptor)
        const Piece hp0 = piece_in_page((uint64_t)key * pb, pb, d.dst, d.src, d.len, a.src);
        const uint32_t hrr = hp0.rlo | hp0.rhi << 16;
        const uint64_t hsp = (uint64_t)(uintptr_t)hp0.sp;
        const bool single = pfirst == claimer;  // nobody pushed onto the claimer: the page's only piece
        const uint64_t singles = __ballot(single);
        const uint32_t cnt = (uint32_t)__popcll(__ballot(hv));  // valid lanes are 0 .. cnt-1
        // two pages in flight: k (being merged + hashed) and k+1.  (A third
        // bought nothing, round 3: 0.1488 vs 0.1454 ms in a timing ablation.  A
        // page iteration issues ~39 VMEM instructions in full mode -- 16 row
        // loads, 6 edge loads, 16 row stores, the CRC -- and ~53 on the generic
        // path; gfx950's 6-bit vmcnt counts at most 63 outstanding.)
        uint32_t A[M], B[M];
        constexpr bool kRowSel = !Delta;  // full mode: one-piece pages through the per-row source/page select
        using Src = typename std::conditional<kRowSel, PieceEdges, PieceSrc<M>>::type;
        Src S0, S1;
        auto fetch = [&](Src& r, const Piece& p) {
            if constexpr (kRowSel) {
                fetch_edges<M>(r, p, lane);
            } else {
                fetch_piece<M>(r, p, lane);
            }
        };
        auto head_piece = [&](uint32_t k) {
            const uint32_t rr = __builtin_amdgcn_readlane(hrr, k);
            return Piece{rr & 0xFFFFu, rr >> 16, reinterpret_cast<const unsigned char*>(readlane64(hsp, k))};
        };
        // one page step: merge + store + rehash page `pg` from (X, SX, px) while
        // the loads of the next page go into (Y, SY); false after the last page
        // delta mode: rows of page h to read (the head piece's if it is the
        // page's only piece) and the page's stored CRC (a vector load: a scalar
        // one would share lgkmcnt with the chain's LDS lookups)
        auto load_next = [&](uint32_t (&Y)[M], const Piece& py, uint32_t pgy, uint32_t h, uint32_t& ocy) {
            if constexpr (Delta) {
                const PieceRows r = piece_rows(py);
                const uint32_t top = r.row1 >= 31 ? 0xFFFFFFFFu : (2u << r.row1) - 1u;
                const uint32_t rows = ((singles >> h) & 1ull) ? top & ~((1u << r.row0) - 1u) : 0xFFFFFFFFu;
                load_rows<M>(Y, a.pool + (uint64_t)pgy * pb, rows, lane);
                uint32_t vz = 0;
                asm volatile("" : "+v"(vz));
                ocy = a.page_crcs[pgy + vz];
            } else {
                // rows the page's only piece covers whole come straight from the source
                load_rows_sel<M>(Y, a.pool + (uint64_t)pgy * pb, py.sp, ((singles >> h) & 1ull) ? covered_rows(py) : 0u,
                                 lane);
            }
        };
        auto step = [&](uint32_t (&X)[M], Src& SX, const Piece& px, uint32_t pg, uint32_t hh, uint32_t ocx,
                        uint32_t (&Y)[M], Src& SY, Piece& py, uint32_t& pgy, uint32_t& ocy) {
            const bool more = hh + 1 < cnt;
            // next page + its first piece's source bytes in flight (clamped to the
            // last page: a harmless re-read, so every step issues the same loads
            // and the vmcnt waits stay exact)
            const uint32_t h1 = more ? hh + 1 : hh;
            pgy = __builtin_amdgcn_readlane(key, h1);
            py = head_piece(h1);
            load_next(Y, py, pgy, h1, ocy);
            fetch(SY, py);
            const uint64_t pbase = (uint64_t)pg * pb;
            uint32_t dirty = 0;
            uint32_t O[Delta ? M : 1];
            if constexpr (Delta) {
#pragma unroll
                for (int j = 0; j < M; j++) O[j] = X[j];
            }
            if ((singles >> hh) & 1ull) {
                if constexpr (kRowSel) {
                    merge_edges<M>(X, dirty, SX, px, lane);
                } else {
                    merge_piece<M>(X, dirty, SX, px, lane);
                }
            } else {  // several pieces: collect the list, apply in log (update index) order
                // the list's first two pieces came with the metadata; their
                // descriptors (lanes 0, 1) and the link after the second load
                // together, so a two-piece page (nearly every page with several)
                // pays one round trip for its list instead of four.  (Loading these
                // with the previous step's edge loads instead measured equal.)
                const uint32_t u0h = __builtin_amdgcn_readlane(u0, hh);
                const uint32_t u1h = (uint32_t)__builtin_amdgcn_readlane(nxt, hh) / a.slots;  // the second piece's update
                uint32_t cnt = 2, mu = lane == 0 ? u0h : (lane == 1 ? u1h : 0xFFFFFFFFu);  // update of lane's piece
                const UpdateDesc dq = a.upd[lane < 2 ? mu : u0h];
                uint32_t q = a.next[__builtin_amdgcn_readlane(nxt, hh)];
                uint64_t dd = dq.dst, ds = dq.src;
                uint32_t dn = dq.len;
                while (q != kNoPiece && cnt < 64u) {
                    mu = lane == cnt ? q / a.slots : mu;
                    cnt++;
                    q = a.next[q];
                }
                if (cnt > 2 && q == kNoPiece) {  // rare: the other descriptors
                    const UpdateDesc dq = a.upd[lane < cnt ? mu : u0h];
                    dd = dq.dst, ds = dq.src, dn = dq.len;
                }
                if (q != kNoPiece) {  // > 64 pieces (a log hammering this page: rare)
                    // its own wave replays the whole log for this page, 64 records per round
                    // (a ballot of the records touching it), in log order
                    for (uint64_t b = 0; b < a.n_updates; b += 64) {
                        const uint64_t i = b + lane;
                        const UpdateDesc dr = a.upd[i < a.n_updates ? i : b];
                        const bool ok = i < a.n_updates && dr.len >= 1 && dr.len <= a.max_len &&
                                        dr.dst < a.pool_bytes && dr.len <= a.pool_bytes - dr.dst &&
                                        dr.dst < pbase + pb && dr.dst + dr.len > pbase;
                        for (uint64_t m = __ballot(ok); m; m &= m - 1) {
                            const uint32_t l = (uint32_t)__builtin_ctzll(m);
                            const Piece pq = piece_in_page(pbase, pb, readlane64(dr.dst, l), readlane64(dr.src, l),
                                                           __builtin_amdgcn_readlane(dr.len, l), a.src);
                            PieceSrc<M> T;
                            fetch_piece<M>(T, pq, lane);
                            merge_piece<M>(X, dirty, T, pq, lane);
                        }
                    }
                } else {
                    uint32_t rank = lane < cnt ? 0u : 0xFFFFu;  // lanes < cnt: distinct updates
                    for (uint32_t j = 0; j < cnt; j++) rank += (uint32_t)__builtin_amdgcn_readlane(mu, j) < mu;
                    auto lane_piece = [&](uint32_t l) {
                        return piece_in_page(pbase, pb, readlane64(dd, l), readlane64(ds, l),
                                             __builtin_amdgcn_readlane(dn, l), a.src);
                    };
                    if (kRowSel && cnt == 2) {  // both pieces' source bytes in flight together
                        const uint32_t l0 = (uint32_t)__builtin_ctzll(__ballot(rank == 0)), l1 = l0 ^ 1u;
                        const Piece q0 = lane_piece(l0), q1 = lane_piece(l1);
                        PieceSrc<M> T0, T1;
                        fetch_piece<M>(T0, q0, lane);
                        fetch_piece<M>(T1, q1, lane);
                        merge_piece<M>(X, dirty, T0, q0, lane);
                        merge_piece<M>(X, dirty, T1, q1, lane);
                    } else
                    for (uint32_t r = 0; r < cnt; r++) {
                        const Piece pq = lane_piece((uint32_t)__builtin_ctzll(__ballot(rank == r)));
                        if constexpr (kRowSel) {
                            PieceSrc<M> T;
                            fetch_piece<M>(T, pq, lane);
                            merge_piece<M>(X, dirty, T, pq, lane);
                        } else {
                            fetch_piece<M>(SX, pq, lane);  // SX (the prefetched head piece) is not used: reuse it
                            merge_piece<M>(X, dirty, SX, pq, lane);
                        }
                    }
                }
            }
            {  // changed rows only; the others get an out-of-range offset and are dropped
                const __amdgpu_buffer_rsrc_t rp =
                    __builtin_amdgcn_make_buffer_rsrc(a.pool + pbase, 0, 256u * M, kBufFlags);
#pragma unroll
                for (int j = 0; j < M; j++)
                    __builtin_amdgcn_raw_buffer_store_b32(
                        X[j], rp,
                        row_sel(((dirty >> j) & 1u) ? 4u * lane : kBufOOB) + 256u * j, 0, kLogStoreAux);
            }
            uint32_t crc;
            if constexpr (Delta) {
#pragma unroll
                for (int j = 0; j < M; j++) O[j] ^= X[j];  // old ^ new: 0 outside the changed bytes
                crc = wave_xor(apply_fin(tab, chain<M>(tab, O, c0, c1), cf)) ^ ocx;
            } else {
                crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
            }
            if (lane == 0) a.page_crcs[pg] = crc;
            return more;
        };
        // the two register sets alternate (no copies): page k in one while page
        // k+1's loads land in the other
        uint32_t pgA = __builtin_amdgcn_readlane(key, 0), pgB = pgA;
        uint32_t ocA = 0, ocB = 0;
        Piece pA = head_piece(0), pB = pA;
        load_next(A, pA, pgA, 0, ocA);
        fetch(S0, pA);
        for (uint32_t h = 0;; h += 2) {
            if (!step(A, S0, pA, pgA, h, ocA, B, S1, pB, pgB, ocB)) break;
            if (!step(B, S1, pB, pgB, h + 1, ocB, A, S0, pA, pgA, ocA)) break;
        }
    }
    group_next<WV>(a.nx, tab);
}

template <int M, bool Delta>
__global__ __launch_bounds__(64 * log_waves(M, Delta)) void log_pages_kernel(LogLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    log_pages_body<M, Delta>(a, tab);
}

// Copy on write (cc_apply_log_cow_dev), between the insert and the page kernel:
// CSChunkFile::Write's copy2Snapshot for a whole batch.  The heads are cut into
// equal shares per workgroup and per wave, as in log_pages_body; lane k of a
// wave step takes head base + k: its page (table[slot] >> 32), the page's chunk,
// the chunk's snapshot slot and its bit in the slot's bitmap.  A page with a
// slot below n_slots and a clear bit is copied: the lane sets the bit (one
// atomicOr: 32 pages share a word and sit in other lanes and waves) and moves
// the page's stored CRC; the wave then copies the marked pages two at a time,
// lane l holding dwords l + 64 j of each (whole 256-byte rows, load_page's
// layout).  Verify also rehashes every copied page and counts those whose
// bytes do not match the stored CRC (still copied with it); without it the
// kernel takes no LDS and does no CRC arithmetic.  No spin waits, nothing
// shared between workgroups but the bitmap words and the two counters (one
// atomicAdd a wave each).
template <int M, bool Verify>
__global__ __launch_bounds__(64 * kCowWaves) void log_cow_kernel(LogCowLaunch a) {
    __shared__ uint32_t tab[Verify ? kLdsBytes / 4 : 1];
    constexpr int kSpl = kInsertBlocks / 64;
    constexpr uint32_t pb = 256u * M;  // = a.page_bytes (launch_log_cow picks M)
    const uint32_t lane = threadIdx.x & 63u;
    // the insert blocks' segment counts, as in log_pages_body: lane l holds
    // segments kSpl * l .. kSpl * l + kSpl - 1, scum = inclusive prefix of the lanes' sums
    uint32_t sc[kSpl];
    uint32_t ssum = 0;
#pragma unroll
    for (int j = 0; j < kSpl; j++) {
        const uint32_t sg = kSpl * lane + j;
        sc[j] = sg < a.n_segs ? a.seg_count[sg] : 0u;
        ssum += sc[j];
    }
    uint32_t scum = ssum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(scum, d, 64);
        if (lane >= (uint32_t)d) scum += o;
    }
    const uint32_t sexcl = scum - ssum;
    const uint32_t Hall = __builtin_amdgcn_readlane(scum, 63);
    const uint32_t hb0 = (uint32_t)((uint64_t)Hall * blockIdx.x / gridDim.x);
    const uint32_t hb1 = (uint32_t)((uint64_t)Hall * (blockIdx.x + 1) / gridDim.x);
    if (hb0 >= hb1) return;  // (uniform over the workgroup)
    if constexpr (Verify) fill_lds<64 * kCowWaves>(tab, static_cast<const uint4*>(a.image));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    const uint32_t Hb = hb1 - hb0;
    const uint32_t first = hb0 + (uint32_t)((uint64_t)Hb * wave / kCowWaves);
    const uint32_t H = hb0 + (uint32_t)((uint64_t)Hb * (wave + 1) / kCowWaves);  // this wave: [first, H)
    uint32_t ncopied = 0, nstale = 0;
    for (uint32_t base = first; base < H; base += 64u) {
        const uint64_t ih = (uint64_t)base + lane;
        const bool hv = ih < H;
        const uint32_t hi = hv ? (uint32_t)ih : base;  // (clamped: the loads below need no branch)
        // the lane's head in its segment: the first lane tl with scum > hi holds
        // the segment (a binary search over the lanes), then its kSpl counts
        uint32_t lo = 0, up = 63;
#pragma unroll
        for (int st = 0; st < 6; st++) {
            const uint32_t mid = (lo + up) >> 1;
            const bool le = __shfl(scum, (int)mid, 64) > hi;
            up = le ? mid : up;
            lo = le ? lo : (mid + 1u > 63u ? 63u : mid + 1u);
        }
        uint32_t sbefore = __shfl(sexcl, (int)lo, 64), seg = kSpl * lo;
        bool found = false;
#pragma unroll
        for (int j = 0; j < kSpl; j++) {
            const uint32_t v = __shfl(sc[j], (int)lo, 64);
            if (!found) {
                if (sbefore + v > hi) {
                    found = true;
                    seg = kSpl * lo + j;
                } else {
                    sbefore += v;
                }
            }
        }
        const bool hok = hv && found && seg < a.n_segs && hi - sbefore < a.seg_cap;
        const uint2 hrec =
            hok ? reinterpret_cast<const uint2*>(a.heads)[(uint64_t)seg * a.seg_cap + (hi - sbefore)] : make_uint2(0u, 0u);
        const uint64_t ent = hok ? a.table[hrec.x] : 0ull;
        const uint32_t key = (uint32_t)(ent >> 32) - 1u;  // the page
        const bool pok = hok && ent != 0ull && key < a.n_pages;
        const uint32_t chunk = pok ? key / a.pages_per_chunk : 0u;
        const uint32_t q = pok ? key - chunk * a.pages_per_chunk : 0u;  // the page within its chunk
        const uint32_t slot = pok ? a.snap_slot[chunk] : 0xFFFFFFFFu;
        const bool has = pok && slot < a.n_slots;  // CC_NO_SNAPSHOT and any slot out of range: written in place
        uint32_t* word = a.snap_bitmap + ((uint64_t)(has ? slot : 0u) * a.words_per_slot + (q >> 5));
        const uint32_t bit = 1u << (q & 31u);
        bool need = false;
        if (has) need = !(*word & bit);  // a set bit: the snapshot keeps its first version
        const uint64_t sidx = need ? (uint64_t)slot * a.pages_per_chunk + q : 0ull;  // page of d_snap / entry of d_snap_crcs
        uint32_t oc = 0;
        if (need) {
            oc = a.page_crcs[key];
            a.snap_crcs[sidx] = oc;  // moved, not recomputed
            atomicOr(word, bit);
        }
        uint64_t todo = __ballot(need);
        ncopied += (uint32_t)__popcll(todo);
        while (todo) {
            // two pages in flight: both loads, then both stores
            const uint32_t b0 = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const bool two = todo != 0ull;
            const uint32_t b1 = two ? (uint32_t)__builtin_ctzll(todo) : b0;
            todo &= todo - 1ull;  // (0 stays 0)
            const uint32_t p0 = __builtin_amdgcn_readlane(key, b0), p1 = __builtin_amdgcn_readlane(key, b1);
            const uint64_t d0 = readlane64(sidx, b0), d1 = readlane64(sidx, b1);
            uint32_t w0[M], w1[M];
            load_page<M>(w0, reinterpret_cast<const uint32_t*>(a.pool + (uint64_t)p0 * pb) + lane);
            load_page<M>(w1, reinterpret_cast<const uint32_t*>(a.pool + (uint64_t)p1 * pb) + lane);
            uint32_t* o0 = reinterpret_cast<uint32_t*>(a.snap + d0 * pb) + lane;
            uint32_t* o1 = reinterpret_cast<uint32_t*>(a.snap + d1 * pb) + lane;
#pragma unroll
            for (int j = 0; j < M; j++) __builtin_nontemporal_store(w0[j], o0 + 64 * j);
            if (two) {
#pragma unroll
                for (int j = 0; j < M; j++) __builtin_nontemporal_store(w1[j], o1 + 64 * j);
            }
            if constexpr (Verify) {
                const uint32_t e0 = __builtin_amdgcn_readlane(oc, b0), e1 = __builtin_amdgcn_readlane(oc, b1);
                const uint32_t r0 = wave_xor(apply_fin(tab, chain<M>(tab, w0, c0, c1), cf)) ^ a.kconst;
                nstale += r0 != e0 ? 1u : 0u;
                if (two) {
                    const uint32_t r1 = wave_xor(apply_fin(tab, chain<M>(tab, w1, c0, c1), cf)) ^ a.kconst;
                    nstale += r1 != e1 ? 1u : 0u;
                }
            }
        }
    }
    if (lane == 0) {
        if (a.copied && ncopied) atomicAdd(a.copied, (unsigned long long)ncopied);
        if (Verify && nstale) atomicAdd(a.stale, (unsigned long long)nstale);
    }
}

// A small log (<= 64 writes of <= one page each: at most 2 pieces a write) in
// ONE launch, for the per-request latency of the write path: no table memset,
// no insert.  Every wave loads the log into its lanes and finds the distinct
// touched pages itself (a page belongs to the first write touching it: a
// 64-step scan over the earlier lanes); page u goes to wave u, which applies
// every write touching it in log order (a ballot over the lanes, set bits in
// lane order) through the generic piece merge, stores the changed rows and
// rehashes the page.  Blocks without a page exit before filling LDS.
template <int M, bool Delta>
__global__ __launch_bounds__(64 * log_small_waves(M, Delta)) void log_small_kernel(LogLaunch a) {
    constexpr int WV = log_small_waves(M, Delta);
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t pb = a.page_bytes;
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));
    const bool valid = lane < a.n_updates;
    const UpdateDesc d = a.upd[(valid ? lane : 0u) + vz];
    const bool ok = valid && d.len >= 1 && d.len <= a.max_len && d.dst < a.pool_bytes && d.len <= a.pool_bytes - d.dst;
    const uint64_t q0 = ok ? d.dst / pb : 0, q1 = ok ? (d.dst + d.len - 1) / pb : 0;
    // write `lane` owns its page q0 (q1) unless an earlier write touches it
    bool own0 = ok, own1 = ok && q1 != q0;
    for (uint32_t j = 0; j < 63u && j + 1 < a.n_updates; j++) {
        const bool okj = __builtin_amdgcn_readlane((uint32_t)ok, j) != 0u;
        const uint64_t j0 = readlane64(q0, j), j1 = readlane64(q1, j);
        if (okj && lane > j) {
            own0 = own0 && !(j0 <= q0 && q0 <= j1);
            own1 = own1 && !(j0 <= q1 && q1 <= j1);
        }
    }
    const uint64_t m0 = __ballot(own0), m1 = __ballot(own1);
    const uint32_t D = (uint32_t)__popcll(m0) + (uint32_t)__popcll(m1);  // distinct touched pages
    const uint32_t Wg = gridDim.x * WV, W = D < Wg ? D : Wg;
    if (blockIdx.x * (uint32_t)WV >= W) return;  // uniform per block (an empty log: every block)
    fill_lds<64 * WV>(tab, static_cast<const uint4*>(a.image));
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    const uint32_t* pages = reinterpret_cast<const uint32_t*>(a.pool) + lane;
    const uint32_t n0 = (uint32_t)__popcll(m0);
    for (uint32_t u = blockIdx.x * WV + wave; u < D; u += W) {
        // page u: the u-th owned q0 (lane order), then the owned q1s
        uint64_t mm = u < n0 ? m0 : m1;
        for (uint32_t r = u < n0 ? u : u - n0; r; r--) mm &= mm - 1;  // drop the lowest r set bits
        const uint32_t l = (uint32_t)__builtin_ctzll(mm);
        const uint64_t pg = u < n0 ? readlane64(q0, l) : readlane64(q1, l);
        const uint64_t pbase = pg * pb;
        uint32_t X[M], O[Delta ? M : 1];
        load_page<M>(X, pages + pg * (64u * M));
        if constexpr (Delta) {
#pragma unroll
            for (int j = 0; j < M; j++) O[j] = X[j];
        }
        uint32_t dirty = 0;
        const bool hit = ok && d.dst < pbase + pb && d.dst + d.len > pbase;
        for (uint64_t m = __ballot(hit); m; m &= m - 1) {  // the writes touching the page, in log order
            const uint32_t wl = (uint32_t)__builtin_ctzll(m);
            const Piece pq = piece_in_page(pbase, pb, readlane64(d.dst, wl), readlane64(d.src, wl),
                                           __builtin_amdgcn_readlane(d.len, wl), a.src);
            PieceSrc<M> T;
            fetch_piece<M>(T, pq, lane);
            merge_piece<M>(X, dirty, T, pq, lane);
        }
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(a.pool + pbase, 0, 256u * M, kBufFlags);
#pragma unroll
        for (int j = 0; j < M; j++)
            __builtin_amdgcn_raw_buffer_store_b32(X[j], rp, row_sel(((dirty >> j) & 1u) ? 4u * lane : kBufOOB) + 256u * j, 0, 0);
        uint32_t crc;
        if constexpr (Delta) {
#pragma unroll
            for (int j = 0; j < M; j++) O[j] ^= X[j];
            crc = wave_xor(apply_fin(tab, chain<M>(tab, O, c0, c1), cf)) ^ a.page_crcs[pg + vz];
        } else {
            crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
        }
        if (lane == 0) a.page_crcs[pg] = crc;
    }
}

// ---------------------------------------------------------------------------
// Write-log traffic probe (diagnostic, cc_apply_log_probe_dev): the memory
// traffic of the write log's page pass with everything else removed -- no
// hash table, no head segments, no list walk, no CRC.  The touched pages come
// as a host-built list (one descriptor a page: rows the page's only piece
// covers whole, read from the source as the real kernel reads them; rows the
// page's pieces dirty, stored back nt).  Same grid and occupancy as
// log_pages_kernel<16, false> (one workgroup of kLogWavesFull waves per CU),
// each wave an equal contiguous share of the pages, kProbeDepth pages in
// flight (the next pages' rows load while page k's dirty rows are stored; 2,
// as the page pass holds).  The stores write back
// what was loaded, so run right after the log it describes was applied, the
// probe changes no byte; `out` gets an XOR of each page's words (keeps every
// load live).  Its time is the ceiling of the write log's access pattern.
// ---------------------------------------------------------------------------
constexpr int kProbeDepth = 2;
template <int M>
__global__ __launch_bounds__(64 * kLogWavesFull) void log_probe_kernel(LogProbeLaunch a) {
    constexpr int D = kProbeDepth;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t W = (uint64_t)gridDim.x * kLogWavesFull, gw = (uint64_t)blockIdx.x * kLogWavesFull + wave;
    const uint64_t first = a.n * gw / W, last = a.n * (gw + 1) / W;
    for (uint64_t base = first; base < last; base += 64) {
        const uint64_t ih = base + lane;
        LogProbeDesc d = a.desc[ih < last ? ih : base];
        if (d.page >= a.pool_pages) d = LogProbeDesc{0, 0, 0u, 0u};  // past the pool: read page 0, store nothing
        const uint32_t cnt = (uint32_t)(last - base < 64 ? last - base : 64);
        uint32_t ring[D][M];
        auto load = [&](uint32_t (&Y)[M], uint32_t k) {
            const uint64_t pg = readlane64(d.page, k);
            const uint64_t so = readlane64(d.src_off, k);
            load_rows_sel<M>(Y, a.pool + pg * (256u * M), a.src + so, __builtin_amdgcn_readlane(d.covered, k), lane);
        };
        auto finish = [&](uint32_t (&X)[M], uint32_t k) {
            const uint64_t pg = readlane64(d.page, k);
            const uint32_t dirty = __builtin_amdgcn_readlane(d.dirty, k);
            const __amdgpu_buffer_rsrc_t rp =
                __builtin_amdgcn_make_buffer_rsrc(a.pool + pg * (256u * M), 0, 256u * M, kBufFlags);
            uint32_t x = 0;
#pragma unroll
            for (int j = 0; j < M; j++) {
                __builtin_amdgcn_raw_buffer_store_b32(X[j], rp, row_sel(((dirty >> j) & 1u) ? 4u * lane : kBufOOB) + 256u * j,
                                                      0, kLogStoreAux);
                x ^= X[j];
            }
            x = wave_xor(x);
            if (lane == 0) a.out[base + k] = x;
        };
#pragma unroll
        for (int st = 0; st < D - 1; st++) load(ring[st], (uint32_t)st < cnt ? st : cnt - 1);
        for (uint32_t k = 0;; k += D) {
            bool done = false;
#pragma unroll
            for (int st = 0; st < D; st++) {
                if (!done) {  // uniform
                    const uint32_t kn = k + st + D - 1;
                    load(ring[(st + D - 1) % D], kn < cnt ? kn : cnt - 1);  // clamped: every step issues the same loads
                    finish(ring[st], k + st);
                    done = k + st + 1 >= cnt;
                }
            }
            if (done) break;
        }
    }
}

// ---------------------------------------------------------------------------
// Diagnostic: the read traffic of a page list (cc_page_list_probe_dev) -- the
// access pattern of a batch of datastore reads with everything else removed:
// verify-on-read's grid and occupancy (kRvWaves waves a CU, LDS unused), each
// wave an equal contiguous share of the list (64 indices a lane-load), two
// pages in flight behind the one being reduced, a rotate-XOR instead of the
// CRC, one word a page out.
// ---------------------------------------------------------------------------
constexpr int kListProbeWaves = 8;  // = kRvWaves (verify-on-read's occupancy)
constexpr uint64_t kRvDynDivList = 16;   // = kRvDynDiv: the last 1/16 of the list is the dynamic tail
constexpr uint64_t kRvDynSlotsList = 32;  // = kRvDynSlots: pages per tail chunk
template <int M>
__global__ __launch_bounds__(64 * kListProbeWaves) void page_list_probe_kernel(PageListProbeLaunch a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t W = (uint64_t)gridDim.x * kListProbeWaves, gw = (uint64_t)blockIdx.x * kListProbeWaves + wave;
    // the stream's other slot set, every head of it (the page kernel's next launch may pull from all)
    if (a.dyn_next && blockIdx.x == 0 && threadIdx.x < kDynHeads) atomicExch(a.dyn_next + threadIdx.x * kDynHeadStride, 0ull);
    // static shares of the first Ts entries, then 32-entry chunks of the rest from
    // one counter (verify-on-read's tail: kRvDynDiv, kRvDynSlots)
    const uint64_t Ts = a.dyn_ctr ? a.n - a.n / kRvDynDivList : a.n;
    const uint64_t n_dyn = (a.n - Ts + kRvDynSlotsList - 1) / kRvDynSlotsList;
    uint64_t first = Ts * gw / W, last = Ts * (gw + 1) / W;
    const uint32_t* pages = a.pool + lane;
    for (;;) {
    for (uint64_t base = first; base < last; base += 64) {
        const uint64_t ih = base + lane;
        const uint64_t pg0 = a.pages[ih < last ? ih : base];
        const uint64_t pg = pg0 < a.pool_pages ? pg0 : 0;  // a bad index reads page 0, never past the pool
        const uint32_t cnt = (uint32_t)(last - base < 64 ? last - base : 64);
        auto at = [&](uint32_t k) { return readlane64(pg, k < cnt ? k : cnt - 1); };  // clamped: same loads every step
        uint32_t A[M], B[M], Cq[M];
        load_page<M>(A, pages + at(0) * (64u * M));
        load_page<M>(B, pages + at(1) * (64u * M));
        auto step = [&](uint32_t (&X)[M], uint32_t k, uint32_t (&Y)[M]) {
            load_page<M>(Y, pages + at(k + 2) * (64u * M));
            uint32_t x = X[0];
#pragma unroll
            for (int j = 1; j < M; j++) x = ((x << 1) | (x >> 31)) ^ X[j];
            x = wave_xor(x);
            if (lane == 0) a.out[base + k] = x;
            return k + 1 < cnt;
        };
        for (uint32_t k = 0;; k += 3) {
            if (!step(A, k, Cq)) break;
            if (!step(B, k + 1, A)) break;
            if (!step(Cq, k + 2, B)) break;
        }
    }
    if (!a.dyn_ctr) break;
    unsigned long long c = 0;
    if (lane == 0) c = atomicAdd(a.dyn_ctr, 1ull);
    c = readlane64(c, 0);
    if (c >= n_dyn) break;
    first = Ts + c * kRvDynSlotsList;
    last = first + kRvDynSlotsList < a.n ? first + kRvDynSlotsList : a.n;
    }
}

// ---------------------------------------------------------------------------
// Verify-on-read for a batch of datastore reads (cc_verify_reads_dev)
// ---------------------------------------------------------------------------
// Pages a read touches (0 for an empty read and for one past the pool).
__device__ __forceinline__ uint64_t read_pages(const ReadVerifyLaunch& a, const RangeDesc& r) {
    if (!r.len || r.off >= a.pool_bytes || r.len > a.pool_bytes - r.off) return 0;
    return ((r.off + r.len - 1) >> a.page_shift) - (r.off >> a.page_shift) + 1;
}

// Pages of tile t (reads [n t / T, n (t+1) / T)), uniform; mark: reads past the
// pool get bad_per_read = UINT32_MAX (the tile's counting wave marks them).
__device__ __forceinline__ uint64_t read_tile_count(const ReadVerifyLaunch& a, uint32_t t, uint32_t lane, bool mark) {
    const uint64_t lo = a.n_reads * t / kReadTiles, hi = a.n_reads * (t + 1) / kReadTiles;
    uint64_t sum = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) {
        const RangeDesc r = a.reads[i];
        sum += read_pages(a, r);
        if (mark && r.len && (r.off >= a.pool_bytes || r.len > a.pool_bytes - r.off)) a.bad_per_read[i] = 0xFFFFFFFFu;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return sum;
}

// ---------------------------------------------------------------------------
// The slot schedule and the group walk of the gathered page kernels.
// rv_begin / rv_next: read_verify, snap_read, paste, scrub.  rv_walk: the first
// three (scrub walks groups of pool pages with a cursor of its own).
// merge_read_kernel and repair_kernel follow the same schedule and walk from
// copies of their own (their comments say why): a change here is made there too.
// ---------------------------------------------------------------------------
// Every page an entry (a read, a paste, a repair request) touches is one slot;
// the batch's slots are entry 0's pages, then entry 1's, ...  ONE launch,
// scheduled as the range kernel is (§7): the waves count kReadTiles tiles of
// entries themselves (epoch-tagged words, a bounded wait) and hold the counts
// in registers; wave w owns the slots [Ts w / W, Ts (w+1) / W) at PAGE
// granularity (an entry may be split over waves; what is counted on it is
// counted by atomics), the last T / kRvDynDiv slots are dynamic chunks (the
// page kernel's tail: the XCDs run at different rates).  The tail's counter is
// slot epoch % 2 of the block; each call zeroes the other slot for the next.
// A share starts at the entry holding its first slot (tile search in
// registers, then the tile's entries 64 at a time); the wave takes its entries
// 64 at a time (lane j <- one entry: first page, page count) and lays their
// pages out as one stream with a wave prefix sum: page k of the stream belongs
// to the first lane whose running count exceeds k (a ballot), so the stream is
// walked with uniform scalar math only -- no loads in the per-page path --
// and handled with the next two pages' loads in flight (three register sets
// rotating, in each kernel's own body).  Table words and stored CRCs come in
// with VECTOR loads (an opaque zero in the address) so they never share
// lgkmcnt with the chain's LDS lookups.
// (Rounds 2-3: a count kernel and rocPRIM's two-launch exclusive scan ran
// first, 16-24 us of a 0.67 ms call.)
constexpr int kRvWaves = 8;  // waves per CU of the verify-on-read kernel
constexpr uint64_t kRvDynDiv = 16;  // 1/16 of the slots form the dynamic tail (A/B: 2-3 % over none; 1/8, 1/32 less)
constexpr uint32_t kRvHeads = 1;  // tail heads (A/B round 3: 8 per-XCD heads = one counter at 1/16)
constexpr uint64_t kRvDynSlots = 32;  // slots (pages) per dynamic chunk (64: -1 %, 128: -5 %, 256: -18 % -- too coarse)
constexpr uint64_t kRvMinSlots = 8;  // a small batch goes to the fewest waves that give each >= 8 page slots
constexpr uint32_t kRvSmallMinSlots = 2;  // the one-launch path (<= 64 reads): >= 2 pages per wave

// A wave's view of the schedule: every tile count of the call (lane l holds
// tiles kTpl*l .. kTpl*l + kTpl-1, cum = inclusive prefix of the lane sums),
// the totals, the tail's cursor and the share it is working on.
struct RvShares {
    uint64_t tb[kReadTiles / 64];
    uint64_t cum;
    uint64_t T, Ts, W;         // slots, statically dealt slots, waves sharing them
    unsigned long long* ctr;   // the tail's counter
    uint32_t head, tried;      // the tail's cursor (tail_cursor)
    uint64_t lo_slot, hi_slot; // the current share
};

// From the tile-count publication to the wave's static share.  count(t, mark)
// is the kernel's own tile count (mark: the counting pass of the tile's own
// wave, which marks invalid entries; without it, a wave counting a missing
// tile).  Fills the workgroup's LDS on the way (which hides the stores' and
// the other workgroups' latency).  False for a workgroup with no share.
template <typename Count>
__device__ __forceinline__ bool rv_begin(RvShares& sh, uint32_t* tab, uint64_t* tiles, unsigned long long* tail,
                                         uint32_t epoch, const void* image, uint32_t lane, Count count) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t Wg = (uint64_t)gridDim.x * kRvWaves;
    const uint64_t w = (uint64_t)blockIdx.x * kRvWaves + wave;
    const uint64_t tag = (uint64_t)epoch << kEpochShift;
    for (uint64_t t = w; t < kReadTiles; t += Wg) {
        const uint64_t cnt = count((uint32_t)t, true);
        if (lane == 0) __hip_atomic_store(tiles + t, tag | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    sh.ctr = tail + (epoch & 1u) * kDynCtrWords64;
    if (blockIdx.x == 0 && threadIdx.x < kRvHeads)
        atomicExch(tail + ((epoch + 1u) & 1u) * kDynCtrWords64 + threadIdx.x * kDynHeadStride, 0ull);
    fill_lds<64 * kRvWaves>(tab, static_cast<const uint4*>(image));
    constexpr int kTpl = kReadTiles / 64;
    wait_tiles<kTpl>(sh.tb, tiles, tag, lane, [&](uint32_t t) { return count(t, false); });
    uint64_t lsum = 0;
#pragma unroll
    for (int j = 0; j < kTpl; j++) lsum += sh.tb[j];
    sh.cum = wave_scan_incl(lsum, lane);
    sh.T = readlane64(sh.cum, 63);
    // W waves share the slots: all of the grid for a large batch, fewer for a small one
    const uint64_t Wt = (sh.T + kRvMinSlots - 1) / kRvMinSlots;
    sh.W = Wt < Wg ? (Wt ? Wt : 1) : Wg;
    if ((uint64_t)blockIdx.x * kRvWaves >= sh.W) return false;  // uniform per block: no share, no tail
    sh.Ts = sh.T - sh.T / kRvDynDiv;
    tail_cursor<kRvHeads>(sh.head, sh.tried);
    sh.lo_slot = w < sh.W ? sh.Ts * w / sh.W : sh.Ts;  // waves past W: tail only
    sh.hi_slot = w < sh.W ? sh.Ts * (w + 1) / sh.W : sh.Ts;
    return true;
}

// The next dynamic chunk of kRvDynSlots slots; false when the tail is drained.
__device__ __forceinline__ bool rv_next(RvShares& sh, uint32_t lane) {
    const uint64_t n_dyn = (sh.T - sh.Ts + kRvDynSlots - 1) / kRvDynSlots;
    const uint64_t c = tail_pull<kRvHeads>(sh.ctr, n_dyn, sh.head, sh.tried, lane);
    if (c >= n_dyn) return false;
    sh.lo_slot = sh.Ts + c * kRvDynSlots;
    sh.hi_slot = sh.lo_slot + kRvDynSlots < sh.T ? sh.lo_slot + kRvDynSlots : sh.T;
    return true;
}

// What lane j holds of its entry in a group of 64, and slot k of the group's
// page stream: the lane of its entry, its position in the entry, its pool page.
struct RvEntry {
    uint64_t pages;  // 0 for an entry that takes no slot (empty or invalid)
    uint64_t p0;     // its first pool page
};
struct RvSlot {
    uint32_t owner, rel;
    uint64_t g;
};
__device__ __forceinline__ RvSlot slot_at(uint32_t cum32, uint64_t p0, uint32_t k) {
    RvSlot s;
    s.owner = (uint32_t)__builtin_ctzll(__ballot(cum32 > k));
    s.rel = k - (s.owner ? (uint32_t)__builtin_amdgcn_readlane(cum32, s.owner - 1) : 0u);
    s.g = readlane64(p0, s.owner) + s.rel;
    return s;
}

// The share [lo_slot, hi_slot) at PAGE granularity: from the entry holding
// slot lo_slot through the entries starting before hi_slot, cut at both ends.
// entry(i) loads entry i for this lane (whatever else the kernel keeps of it,
// such as an output offset, stays in the lambda's captures); body(base, cum32,
// p0, ks, ke) handles slots [ks, ke) of the group of entries base .. base + 63,
// cum32 their inclusive page counts.  The seek's last 64 descriptors are the
// first group's: they are not loaded a second time.
template <typename Entry, typename Body>
__device__ __forceinline__ void rv_walk(const RvShares& sh, uint64_t n, uint32_t lane, Entry entry, Body body) {
    if (sh.lo_slot >= sh.hi_slot) return;
    auto load = [&](uint64_t base) {
        const uint64_t i = base + lane;
        RvEntry e = entry(i < n ? i : base);
        if (i >= n) e.pages = 0;
        return e;
    };
    const TileHit th = tile_of(sh.cum, sh.tb, sh.lo_slot, lane);
    uint64_t base = n * th.tile / kReadTiles;  // the group's first entry
    uint64_t S = th.before;                    // the slot of its page 0
    RvEntry e;
    // the tile's entries 64 at a time, to the group whose pages pass lo_slot
    for (;;) {
        e = load(base);
        const uint64_t tot = readlane64(wave_scan_incl(e.pages, lane), 63);
        if (S + tot > sh.lo_slot || base + 64 >= n) break;
        S += tot;
        base += 64;
    }
    for (bool first = true; base < n && S < sh.hi_slot; base += 64, first = false) {
        if (!first) e = load(base);
        const uint32_t cum32 = wave_scan_incl((uint32_t)e.pages, lane);
        const uint32_t P = __builtin_amdgcn_readlane(cum32, 63);
        const uint32_t ks = sh.lo_slot > S ? (uint32_t)(sh.lo_slot - S) : 0u;
        const uint32_t ke = sh.hi_slot - S < (uint64_t)P ? (uint32_t)(sh.hi_slot - S) : P;
        S += P;
        if (ks < ke) body(base, cum32, e.p0, ks, ke);
    }
}

// The one-launch path of the three read calls (<= 64 reads, one per lane): no
// tiles and no scratch.  Every wave works out the batch's pages per read and
// their wave prefix sum; entry(i, mark) loads read i as rv_walk's does (mark:
// wave 0 of block 0, which marks the invalid ones).  The P pages are split
// evenly over the fewest waves that give each >= kRvSmallMinSlots, at PAGE
// granularity; the blocks left without pages exit before filling LDS.  False
// for a wave without pages; otherwise it owns slots [k0, k1) of the stream.
struct RvSmallShare {
    uint32_t cum;  // inclusive page counts of the lanes' reads
    uint64_t p0;   // the lane's read's first pool page
    uint32_t k0, k1;
};
template <typename Entry>
__device__ __forceinline__ bool rv_small_begin(RvSmallShare& sm, uint32_t* tab, const ReadVerifyLaunch& rv,
                                               uint32_t lane, Entry entry) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool valid = lane < rv.n_reads;
    const RvEntry e = entry(valid ? lane : 0u, valid && blockIdx.x == 0 && wave == 0);
    sm.p0 = e.p0;
    sm.cum = wave_scan_incl(valid ? (uint32_t)e.pages : 0u, lane);
    const uint32_t P = __builtin_amdgcn_readlane(sm.cum, 63);
    const uint32_t Wg = gridDim.x * kRvWaves, Wt = (P + kRvSmallMinSlots - 1) / kRvSmallMinSlots;
    const uint32_t W = Wt < Wg ? Wt : Wg;
    if (blockIdx.x * (uint32_t)kRvWaves >= W) return false;  // uniform per block (P == 0: every block)
    fill_lds<64 * kRvWaves>(tab, static_cast<const uint4*>(rv.image));
    const uint32_t w = blockIdx.x * kRvWaves + wave;
    if (w >= W) return false;
    sm.k0 = (uint32_t)((uint64_t)P * w / W);
    sm.k1 = (uint32_t)((uint64_t)P * (w + 1) / W);
    return sm.k0 < sm.k1;
}

// ---------------------------------------------------------------------------
// cc_verify_reads_dev's kernels
// ---------------------------------------------------------------------------
// Per page: the stored CRC and the page are loaded two steps ahead, the page
// is hashed and a mismatch is counted on its read (rare: atomics).
template <int M>
__global__ __launch_bounds__(64 * kRvWaves) void read_verify_kernel(ReadVerifyLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint64_t n = a.n_reads;
    const uint32_t lane = threadIdx.x & 63u;
    RvShares sh;
    if (!rv_begin(sh, tab, a.tiles, a.tail, a.epoch, a.image, lane,
                  [&](uint32_t t, bool mark) { return read_tile_count(a, t, lane, mark); }))
        return;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    const uint32_t* pages = a.pool + lane;
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));  // opaque zero: keeps uniform-address loads on the vector path
    auto stored_crc = [&](uint64_t g) { return a.page_crcs[g + vz]; };
    auto entry = [&](uint64_t i) -> RvEntry {
        const RangeDesc r = a.reads[i + vz];
        return {read_pages(a, r), r.off >> a.page_shift};  // 0 pages also for reads past the pool
    };
#pragma unroll 1
    do {
        rv_walk(sh, n, lane, entry, [&](uint64_t base, uint32_t cum32, uint64_t p0, uint32_t ks, uint32_t ke) {
            auto page_at = [&](uint32_t k, uint32_t& owner) -> uint64_t {
                const RvSlot s = slot_at(cum32, p0, k);
                owner = s.owner;
                return s.g;
            };
            uint32_t A[M], B[M], Cq[M];
            uint32_t oA, oB, oC;
            uint64_t gA = page_at(ks, oA), gB = page_at(ks + 1 < ke ? ks + 1 : ks, oB), gC = gB;
            oC = oB;
            uint32_t sA = stored_crc(gA), sB = stored_crc(gB), sC = sB;
            load_page<M>(A, pages + gA * (64u * M));
            load_page<M>(B, pages + gB * (64u * M));
            // hash X (page k: stored CRC sx, owner lane ox); page k+2's loads go into Y
            auto step = [&](uint32_t (&X)[M], uint32_t sx, uint32_t ox, uint32_t k, uint32_t (&Y)[M], uint64_t& gy,
                            uint32_t& sy, uint32_t& oy) {
                const bool more = k + 1 < ke;
                gy = page_at(k + 2 < ke ? k + 2 : ke - 1, oy);  // clamped: same loads every step
                sy = stored_crc(gy);
                load_page<M>(Y, pages + gy * (64u * M));
                const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
                if (crc != sx && lane == 0) {
                    atomicAdd(a.bad_per_read + base + ox, 1u);
                    atomicAdd(a.bad_total, 1ull);
                }
                return more;
            };
            for (uint32_t k = ks;; k += 3) {
                if (!step(A, sA, oA, k, Cq, gC, sC, oC)) break;
                if (!step(B, sB, oB, k + 1, A, gA, sA, oA)) break;
                if (!step(Cq, sC, oC, k + 2, B, gB, sB, oB)) break;
            }
        });
    } while (rv_next(sh, lane));
}


// A small batch (<= 64 reads: one per lane) in ONE launch, for the per-request
// latency of the read path: no count kernel and no scan (rv_small_begin; a
// 32-page read is verified by 4 waves).  A wave hashes one page with the next
// page's loads in flight.
template <int M>
__global__ __launch_bounds__(64 * kRvWaves) void read_verify_small_kernel(ReadVerifyLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));
    RvSmallShare sm;
    if (!rv_small_begin(sm, tab, a, lane, [&](uint32_t i, bool mark) -> RvEntry {
            const RangeDesc r = a.reads[i + vz];
            if (mark && r.len && (r.off >= a.pool_bytes || r.len > a.pool_bytes - r.off)) a.bad_per_read[i] = 0xFFFFFFFFu;
            return {read_pages(a, r), r.off >> a.page_shift};
        }))
        return;
    const uint32_t k0 = sm.k0, k1 = sm.k1;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    const uint32_t* pages = a.pool + lane;
    auto page_at = [&](uint32_t k, uint32_t& owner) -> uint64_t {
        const RvSlot s = slot_at(sm.cum, sm.p0, k);
        owner = s.owner;
        return s.g;
    };
    // pages k0 .. k1-1, the next page's loads in flight while one is hashed
    uint32_t X[M], Y[M];
    uint32_t ox, oy;
    uint64_t gx = page_at(k0, ox);
    uint32_t sx = a.page_crcs[gx + vz];
    load_page<M>(X, pages + gx * (64u * M));
    for (uint32_t k = k0; k < k1; k++) {
        const uint64_t gy = page_at(k + 1 < k1 ? k + 1 : k, oy);  // clamped: same loads every step
        const uint32_t sy = a.page_crcs[gy + vz];
        load_page<M>(Y, pages + gy * (64u * M));
        const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
        if (crc != sx && lane == 0) {
            atomicAdd(a.bad_per_read + ox, 1u);
            atomicAdd(a.bad_total, 1ull);
        }
#pragma unroll
        for (int j = 0; j < M; j++) X[j] = Y[j];
        sx = sy;
        ox = oy;
    }
}

// ---------------------------------------------------------------------------
// Snapshot reads (cc_read_snap_dev): verify-on-read's schedule, every page
// slot resolved to its snapshot-view source, rehashed against that source's
// CRC and (Copy) delivered.  Replaces the host loop of
// CSChunkFile::ReadSpecifiedChunk (chunkserver_chunkfile.cpp:550-636:
// Divide() into copied and uncopied ranges, readData for one set,
// snapshot_->Read for the other); with no slots, CSChunkFile::Read (:497-536).
// ---------------------------------------------------------------------------
// Pages of a read that is served: 0 for an empty read and for an invalid one
// (misaligned, past the pool, or -- with an output -- an output range that is
// unaligned or leaves the buffer), so an invalid read takes no slot.
template <bool Copy>
__device__ __forceinline__ bool snap_read_bad(const SnapReadLaunch& a, const RangeDesc& r, uint64_t oo) {
    if (!r.len) return false;
    if ((r.off | r.len) & (uint64_t)(a.rv.page_bytes - 1u)) return true;
    if (r.off >= a.rv.pool_bytes || r.len > a.rv.pool_bytes - r.off) return true;
    return Copy && ((oo & 3u) || oo > a.out_bytes || r.len > a.out_bytes - oo);
}
template <bool Copy>
__device__ __forceinline__ uint64_t snap_pages(const SnapReadLaunch& a, const RangeDesc& r, uint64_t oo) {
    return snap_read_bad<Copy>(a, r, oo) ? 0u : read_pages(a.rv, r);
}

// Pages of tile t, uniform; mark: invalid reads get bad_per_read = UINT32_MAX
// (the tile's counting wave marks them, as read_tile_count does).
template <bool Copy>
__device__ __forceinline__ uint64_t snap_tile_count(const SnapReadLaunch& a, uint32_t t, uint32_t lane, bool mark) {
    const uint64_t lo = a.rv.n_reads * t / kReadTiles, hi = a.rv.n_reads * (t + 1) / kReadTiles;
    uint64_t sum = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) {
        const RangeDesc r = a.rv.reads[i];
        const uint64_t oo = Copy ? a.out_off[i] : 0u;
        const bool bad = snap_read_bad<Copy>(a, r, oo);
        sum += bad ? 0u : read_pages(a.rv, r);
        if (mark && bad) a.rv.bad_per_read[i] = 0xFFFFFFFFu;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return sum;
}

// One page slot on its way to its loads.  Its position is uniform (SGPRs);
// the source is resolved in three stages a step apart: snap_slot_of (chunk,
// page in chunk, the chunk's slot), snap_word_of (the slot's bitmap word),
// snap_source (data and CRC address).  The two table words come in with VECTOR
// loads (the opaque zero: a scalar load would share lgkmcnt with the chain's
// LDS lookups) and stay in a VGPR, the same value in every lane, until the
// next stage takes them with a readfirstlane a step later -- the wait sits
// there, a whole page's hash after the load, not at the load.
struct SnapPg : RvSlot {  // owner: lane holding the page's read; rel: the page's position in it; g: pool page
    uint32_t q;      // page in chunk
    uint32_t s;      // the chunk's slot (>= n_slots: none), once snap_word_of has taken it
    uint32_t sv;     // VGPR: the slot as loaded
    uint32_t wv;     // VGPR: the slot's bitmap word holding bit q, as loaded
};
__device__ __forceinline__ void snap_slot_of(const SnapReadLaunch& a, SnapPg& p, uint32_t vz) {
    p.q = 0;
    p.s = 0xFFFFFFFFu;
    p.sv = 0xFFFFFFFFu;
    p.wv = 0;
    if (!a.n_slots) return;  // uniform: no snapshot, nothing to resolve
    uint64_t c;
    if ((p.g >> 32) || a.pages_per_chunk == 1) {  // beyond the reciprocal's range (uniform, rare)
        c = p.g / a.pages_per_chunk;
    } else {
        const uint32_t g32 = (uint32_t)p.g;
        c = ((uint64_t)g32 * a.ppc_mhi + ((uint64_t)g32 * a.ppc_mlo >> 32)) >> 32;
    }
    p.q = (uint32_t)(p.g - c * a.pages_per_chunk);
    p.sv = a.snap_slot[c + vz];
}
__device__ __forceinline__ void snap_word_of(const SnapReadLaunch& a, SnapPg& p, uint32_t vz) {
    if (!a.n_slots) return;
    p.s = __builtin_amdgcn_readfirstlane(p.sv);
    const uint32_t sc = p.s < a.n_slots ? p.s : 0u;  // clamped: the same load every page
    p.wv = a.snap_bitmap[(uint64_t)sc * a.words_per_slot + (p.q >> 5) + vz];
}
struct SnapSrc {
    const uint32_t* data;
    const uint32_t* crc;
};
__device__ __forceinline__ SnapSrc snap_source(const SnapReadLaunch& a, const SnapPg& p) {
    SnapSrc r;
    r.data = reinterpret_cast<const uint32_t*>(reinterpret_cast<const unsigned char*>(a.rv.pool) +
                                               (p.g << a.rv.page_shift));
    r.crc = a.rv.page_crcs + p.g;
    if (!a.n_slots) return r;
    const uint32_t word = __builtin_amdgcn_readfirstlane(p.wv);
    if (p.s < a.n_slots && ((word >> (p.q & 31u)) & 1u)) {
        const uint64_t sp = (uint64_t)p.s * a.pages_per_chunk + p.q;
        r.data = reinterpret_cast<const uint32_t*>(a.snap + (sp << a.rv.page_shift));
        r.crc = a.snap_crcs + sp;
    }
    return r;
}

// load_page's layout back out: M coalesced 256-byte rows (nt: written once, read by the caller later)
template <int M>
__device__ __forceinline__ void store_page(const uint32_t (&w)[M], uint32_t* p) {
#pragma unroll
    for (int j = 0; j < M; j++) __builtin_nontemporal_store(w[j], p + 64 * j);
}

// Three register sets rotating, with the per-page source resolution: the step
// that hashes page k first takes the table words loaded a step earlier, issues
// page k+3's bitmap-word load and page k+4's slot load, and then page k+2's
// loads from the source just resolved.  The table loads go BEFORE the page's:
// vmcnt retires in order, so a table word issued after a page's loads would
// hold the step that needs it until that page had landed, a page early.  Lane
// j of a group of 64 reads also holds its read's output offset; a page's
// output address is the owner lane's offset (readlane) plus its position in
// the read.
template <int M, bool Copy>
__global__ __launch_bounds__(64 * kRvWaves) void snap_read_kernel(SnapReadLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint64_t n = a.rv.n_reads;
    const uint32_t lane = threadIdx.x & 63u;
    RvShares sh;
    if (!rv_begin(sh, tab, a.rv.tiles, a.rv.tail, a.rv.epoch, a.rv.image, lane,
                  [&](uint32_t t, bool mark) { return snap_tile_count<Copy>(a, t, lane, mark); }))
        return;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));  // opaque zero: keeps uniform-address loads on the vector path
    uint64_t oo = 0;  // the lane's read's output offset
    auto entry = [&](uint64_t i) -> RvEntry {
        const RangeDesc r = a.rv.reads[i + vz];
        oo = Copy ? a.out_off[i + vz] : 0u;
        return {snap_pages<Copy>(a, r, oo), r.off >> a.rv.page_shift};  // 0 pages also for invalid reads
    };
#pragma unroll 1
    do {
        rv_walk(sh, n, lane, entry, [&](uint64_t base, uint32_t cum32, uint64_t p0, uint32_t ks, uint32_t ke) {
            // slot k (clamped to the share's last): its read's lane, its page, its source's chunk slot
            auto locate = [&](uint32_t k) {
                SnapPg p = {slot_at(cum32, p0, k < ke ? k : ke - 1)};
                snap_slot_of(a, p, vz);
                return p;
            };
            // the resolved page's stored CRC, output offset and loads; then the
            // page behind it moves up: its bitmap word, and the slot of the one after
            SnapPg p3, p4;
            auto issue = [&](uint32_t kn, uint32_t (&Y)[M], uint32_t& sy, uint32_t& oy, uint64_t& dy) {
                const SnapSrc src = snap_source(a, p3);
                oy = p3.owner;
                dy = Copy ? readlane64(oo, p3.owner) + ((uint64_t)p3.rel << a.rv.page_shift) : 0u;
                p3 = p4;
                snap_word_of(a, p3, vz);
                p4 = locate(kn);
                __builtin_amdgcn_sched_barrier(0);  // the table loads stay ahead of the page's
                sy = src.crc[vz];
                load_page<M>(Y, src.data + lane);
            };
            uint32_t A[M], B[M], Cq[M];
            uint32_t sA, sB, sC, oA, oB, oC;
            uint64_t dA, dB, dC;
            p3 = locate(ks);
            snap_word_of(a, p3, vz);
            p4 = locate(ks + 1);
            issue(ks + 2, A, sA, oA, dA);
            issue(ks + 3, B, sB, oB, dB);
            sC = sB, oC = oB, dC = dB;
            // hash X (page k: stored CRC sx, owner lane ox, output offset dx); page k+2's loads go into Y
            auto step = [&](uint32_t (&X)[M], uint32_t sx, uint32_t ox, uint64_t dx, uint32_t k, uint32_t (&Y)[M],
                            uint32_t& sy, uint32_t& oy, uint64_t& dy) {
                const bool more = k + 1 < ke;
                issue(k + 4, Y, sy, oy, dy);
                const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.rv.kconst;
                if (Copy) store_page<M>(X, reinterpret_cast<uint32_t*>(a.out + dx) + lane);
                if (crc != sx && lane == 0) {
                    atomicAdd(a.rv.bad_per_read + base + ox, 1u);
                    atomicAdd(a.rv.bad_total, 1ull);
                }
                return more;
            };
            for (uint32_t k = ks;; k += 3) {
                if (!step(A, sA, oA, dA, k, Cq, sC, oC, dC)) break;
                if (!step(B, sB, oB, dB, k + 1, A, sA, oA, dA)) break;
                if (!step(Cq, sC, oC, dC, k + 2, B, sB, oB, dB)) break;
            }
        });
    } while (rv_next(sh, lane));
}

// <= 64 reads (one per lane) in ONE launch (rv_small_begin): a wave resolves
// the next page's source while it hashes one.
template <int M, bool Copy>
__global__ __launch_bounds__(64 * kRvWaves) void snap_read_small_kernel(SnapReadLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));
    uint64_t oo = 0;  // the lane's read's output offset
    RvSmallShare sm;
    if (!rv_small_begin(sm, tab, a.rv, lane, [&](uint32_t i, bool mark) -> RvEntry {
            const RangeDesc r = a.rv.reads[i + vz];
            oo = Copy ? a.out_off[i + vz] : 0u;
            const bool bad = snap_read_bad<Copy>(a, r, oo);
            if (mark && bad) a.rv.bad_per_read[i] = 0xFFFFFFFFu;
            return {bad ? 0u : read_pages(a.rv, r), r.off >> a.rv.page_shift};
        }))
        return;
    const uint32_t k0 = sm.k0, k1 = sm.k1;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    auto locate = [&](uint32_t k) {
        SnapPg p = {slot_at(sm.cum, sm.p0, k < k1 ? k : k1 - 1)};
        snap_slot_of(a, p, vz);
        snap_word_of(a, p, vz);
        return p;
    };
    auto issue = [&](const SnapPg& p, uint32_t (&Y)[M], uint32_t& sy, uint32_t& oy, uint64_t& dy) {
        const SnapSrc src = snap_source(a, p);
        sy = src.crc[vz];
        oy = p.owner;
        dy = Copy ? readlane64(oo, p.owner) + ((uint64_t)p.rel << a.rv.page_shift) : 0u;
        load_page<M>(Y, src.data + lane);
    };
    // pages k0 .. k1-1, the next page's loads in flight while one is hashed
    uint32_t X[M], Y[M];
    uint32_t sx, sy, ox, oy;
    uint64_t dx, dy;
    issue(locate(k0), X, sx, ox, dx);
    SnapPg pn = locate(k0 + 1);
    for (uint32_t k = k0; k < k1; k++) {
        issue(pn, Y, sy, oy, dy);  // clamped: same loads every step
        pn = locate(k + 2);
        const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.rv.kconst;
        if (Copy) store_page<M>(X, reinterpret_cast<uint32_t*>(a.out + dx) + lane);
        if (crc != sx && lane == 0) {
            atomicAdd(a.rv.bad_per_read + ox, 1u);
            atomicAdd(a.rv.bad_total, 1ull);
        }
#pragma unroll
        for (int j = 0; j < M; j++) X[j] = Y[j];
        sx = sy;
        ox = oy;
        dx = dy;
    }
}

// ---------------------------------------------------------------------------
// Clone chunks (cc_paste_dev, cc_clone_mark_dev, cc_clone_check_reads_dev):
// the written-page bitmap of a lazily allocated chunk on the device.  Replaces
// the host loops of CSChunkFile::Paste (chunkserver_chunkfile.cpp:440-495:
// Divide(begin, end, &uncopied, nullptr), writeData per uncopied range, then
// flush() sets the bits), of flush() after a Write (:405-406, :965-1000) and of
// Read's NextClearBit test (:510-526).
// ---------------------------------------------------------------------------
// page / pages_per_chunk: the host-made reciprocal below 2^32 pages (snap_recip), a division beyond
__device__ __forceinline__ uint64_t clone_chunk_of(const CloneGeo& g, uint64_t page) {
    if ((page >> 32) || g.pages_per_chunk == 1) return page / g.pages_per_chunk;
    const uint32_t p32 = (uint32_t)page;
    return ((uint64_t)p32 * g.ppc_mhi + ((uint64_t)p32 * g.ppc_mlo >> 32)) >> 32;
}

// The three one-launch passes walk (entry, page) pairs with one LANE per pair
// and no page traffic: a wave takes 64 entries at a time (lane j <- entry
// base + j: load(i, first page, pages); 0 pages for an entry that takes no
// part), lays their pages out as one stream with a wave prefix sum and walks
// the stream 64 pairs a step; a lane finds its pair's entry with a binary
// search over the prefix sums (six shuffles) and calls fn(entry, pool page).
constexpr int kCloneWaves = 4;  // waves per workgroup of the claim, mark and check kernels
template <typename Load, typename Fn>
__device__ __forceinline__ void clone_entry_pages(uint64_t n, uint32_t lane, Load load, Fn fn) {
    const uint64_t Wg = (uint64_t)gridDim.x * kCloneWaves;
    const uint64_t w = (uint64_t)blockIdx.x * kCloneWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t base = w * 64; base < n; base += Wg * 64) {
        uint64_t p0 = 0, cnt = 0;
        if (base + lane < n) load(base + lane, p0, cnt);
        const uint64_t cum = wave_scan_incl(cnt, lane);
        const uint64_t P = readlane64(cum, 63);
        for (uint64_t k0 = 0; k0 < P; k0 += 64) {
            const bool on = k0 + lane < P;
            const uint64_t k = on ? k0 + lane : P - 1;
            uint32_t o = 0;  // entries of the group whose pages end at or before pair k: the pair's entry
#pragma unroll
            for (int d = 32; d; d >>= 1)
                if (__shfl(cum, (int)(o + d - 1), 64) <= k) o += d;
            const uint64_t upto = __shfl(cum, (int)(o ? o - 1 : 0), 64);
            const uint64_t first = __shfl(p0, (int)o, 64);
            if (on) fn(base + o, first + (k - (o ? upto : 0)));
        }
    }
}

// An entry that cc_paste_dev skips whole: misaligned dst or len, past the
// pool, a source range that is unaligned or leaves the buffer (len == 0 is
// valid and covers nothing).
__device__ __forceinline__ bool paste_bad(const PasteLaunch& a, const UpdateDesc& u) {
    if (!u.len) return false;
    if ((u.dst | u.len) & (uint64_t)(a.page_bytes - 1u)) return true;
    if (u.dst >= a.pool_bytes || u.len > a.pool_bytes - u.dst) return true;
    return (u.src & 3u) || u.src > a.src_bytes || u.len > a.src_bytes - u.src;
}
__device__ __forceinline__ uint32_t paste_pages(const PasteLaunch& a, const UpdateDesc& u) {
    return paste_bad(a, u) ? 0u : u.len >> a.page_shift;
}

// Launch 1 of cc_paste_dev: every (valid entry, page) pair whose chunk is a
// clone and whose bit is clear bids for the page with its entry index; the
// lowest index holds the claim word when the launch ends.  The lane that loads
// an invalid entry marks it.  Reads the bitmap; the paste launch sets bits only
// after this one has finished.
__global__ __launch_bounds__(64 * kCloneWaves) void paste_claim_kernel(PasteLaunch a) {
    const uint32_t lane = threadIdx.x & 63u;
    clone_entry_pages(
        a.n, lane,
        [&](uint64_t i, uint64_t& p0, uint64_t& cnt) {
            const UpdateDesc u = a.pastes[i];
            if (paste_bad(a, u)) {
                a.pasted_per_entry[i] = 0xFFFFFFFFu;
                return;
            }
            p0 = u.dst >> a.page_shift;
            cnt = u.len >> a.page_shift;
        },
        [&](uint64_t e, uint64_t page) {
            const uint64_t c = clone_chunk_of(a.geo, page);
            const uint32_t q = (uint32_t)(page - c * a.geo.pages_per_chunk);
            const uint32_t s = a.geo.clone_slot[c];
            if (s >= a.geo.n_slots) return;  // not a clone chunk
            const uint32_t word = a.geo.bitmap[(uint64_t)s * a.geo.words_per_slot + (q >> 5)];
            if ((word >> (q & 31u)) & 1u) return;  // written already: the page keeps its bytes
            atomicMin(a.geo.claim + (uint64_t)s * a.geo.pages_per_chunk + q, (uint32_t)e);
        });
}

// Pages of tile t of the paste batch, uniform (snap_tile_count without the marks: the claim launch made them).
__device__ __forceinline__ uint64_t paste_tile_count(const PasteLaunch& a, uint32_t t, uint32_t lane) {
    const uint64_t lo = a.n * t / kReadTiles, hi = a.n * (t + 1) / kReadTiles;
    uint64_t sum = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) sum += paste_pages(a, a.pastes[i]);
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return sum;
}

// One (entry, page) slot of the paste launch on its way to its loads, resolved
// in stages a step apart as snap_read_kernel resolves its pages: paste_slot_of
// (chunk, page in chunk, the chunk's bitmap slot), paste_claim_of (the page's
// claim word), and the comparison with the slot's own entry index.  Both table
// words come in with vector loads of a uniform address and stay in a VGPR until
// the next stage takes them a step later.
struct PastePg : RvSlot {  // owner: lane holding the page's entry; rel: the page's position in it; g: pool page
    uint32_t q;      // page in chunk
    uint32_t s;      // the chunk's bitmap slot (>= n_slots: not a clone), once paste_claim_of has taken it
    uint32_t sv;     // VGPR: the slot as loaded
    uint32_t cv;     // VGPR: the page's claim word as loaded
};
__device__ __forceinline__ void paste_slot_of(const PasteLaunch& a, PastePg& p, uint32_t vz) {
    const uint64_t c = clone_chunk_of(a.geo, p.g);
    p.q = (uint32_t)(p.g - c * a.geo.pages_per_chunk);
    p.s = 0xFFFFFFFFu;
    p.cv = 0xFFFFFFFFu;
    p.sv = a.geo.clone_slot[c + vz];
}
__device__ __forceinline__ void paste_claim_of(const PasteLaunch& a, PastePg& p, uint32_t vz) {
    p.s = __builtin_amdgcn_readfirstlane(p.sv);
    const uint32_t sc = p.s < a.geo.n_slots ? p.s : 0u;  // clamped: the same load every slot (n_slots >= 1 here)
    p.cv = a.geo.claim[(uint64_t)sc * a.geo.pages_per_chunk + p.q + vz];
}
// A slot whose loads are out: where its page goes when it holds the claim.
struct PasteDst {
    uint64_t g;
    uint32_t owner, s, q;
    bool win;
};

// Launch 2 of cc_paste_dev, over the batch's (entry, page) slots, three
// register sets rotating.  The slot whose
// claim word equals its own entry index is the page's winner: its source page is
// loaded two steps ahead, hashed as it passes through the registers, stored to
// the pool, and the lane-0 epilogue writes the CRC, ORs the bit, counts and puts
// 0xFFFFFFFF back into the claim word.  Every other slot issues no page load
// and hashes nothing.  A loser may read the claim word before or after the
// winner's reset: neither value is its own index (only entry i ever writes i,
// and only the slot that found i there resets it), so no third launch is needed.
template <int M>
__global__ __launch_bounds__(64 * kRvWaves) void paste_kernel(PasteLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint64_t n = a.n;
    const uint32_t lane = threadIdx.x & 63u;
    RvShares sh;
    if (!rv_begin(sh, tab, a.tiles, a.tail, a.epoch, a.image, lane,
                  [&](uint32_t t, bool) { return paste_tile_count(a, t, lane); }))
        return;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));  // opaque zero: keeps uniform-address loads on the vector path
    uint32_t npasted = 0;  // uniform: this wave's pasted pages, added to the total once
    uint64_t so = 0;       // the lane's entry's source offset
    auto entry = [&](uint64_t i) -> RvEntry {
        const UpdateDesc u = a.pastes[i + vz];
        so = u.src;
        return {paste_pages(a, u), u.dst >> a.page_shift};  // 0 pages also for invalid entries
    };
#pragma unroll 1
    do {
        rv_walk(sh, n, lane, entry, [&](uint64_t base, uint32_t cum32, uint64_t p0, uint32_t ks, uint32_t ke) {
            // slot k (clamped to the share's last): its entry's lane, its page, its chunk's bitmap slot
            auto locate = [&](uint32_t k) {
                PastePg p = {slot_at(cum32, p0, k < ke ? k : ke - 1)};
                paste_slot_of(a, p, vz);
                return p;
            };
            // the resolved slot: does it hold its page's claim?  Then the slot
            // behind it moves up (its claim word, and the bitmap slot of the one
            // after), and the winner's source page is loaded
            PastePg p3, p4;
            auto issue = [&](uint32_t kn, uint32_t (&Y)[M], PasteDst& dy) {
                const uint32_t holder = __builtin_amdgcn_readfirstlane(p3.cv);
                dy.g = p3.g;
                dy.owner = p3.owner;
                dy.s = p3.s;
                dy.q = p3.q;
                dy.win = p3.s < a.geo.n_slots && holder == (uint32_t)base + p3.owner;
                const uint64_t from = readlane64(so, p3.owner) + ((uint64_t)p3.rel << a.page_shift);
                p3 = p4;
                paste_claim_of(a, p3, vz);
                p4 = locate(kn);
                __builtin_amdgcn_sched_barrier(0);  // the table loads stay ahead of the page's
                if (dy.win) load_page<M>(Y, reinterpret_cast<const uint32_t*>(a.src + from) + lane);
            };
            uint32_t A[M], B[M], Cq[M];
            PasteDst dA, dB, dC;
            p3 = locate(ks);
            paste_claim_of(a, p3, vz);
            p4 = locate(ks + 1);
            issue(ks + 2, A, dA);
            issue(ks + 3, B, dB);
            dC = dB;
            // slot k (registers X when it won); slot k+2's loads go into Y
            auto step = [&](uint32_t (&X)[M], const PasteDst dx, uint32_t k, uint32_t (&Y)[M], PasteDst& dy) {
                const bool more = k + 1 < ke;
                issue(k + 4, Y, dy);
                if (dx.win) {
                    const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
                    store_page<M>(X, a.pool + (dx.g << (a.page_shift - 2u)) + lane);
                    if (lane == 0) {
                        a.page_crcs[dx.g] = crc;
                        atomicOr(a.geo.bitmap + (uint64_t)dx.s * a.geo.words_per_slot + (dx.q >> 5), 1u << (dx.q & 31u));
                        atomicAdd(a.pasted_per_entry + base + dx.owner, 1u);
                        __hip_atomic_store(a.geo.claim + (uint64_t)dx.s * a.geo.pages_per_chunk + dx.q, 0xFFFFFFFFu,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    npasted++;
                }
                return more;
            };
            for (uint32_t k = ks;; k += 3) {
                if (!step(A, dA, k, Cq, dC)) break;
                if (!step(B, dB, k + 1, A, dA)) break;
                if (!step(Cq, dC, k + 2, B, dB)) break;
            }
        });
    } while (rv_next(sh, lane));
    if (npasted && lane == 0 && a.pasted) atomicAdd(a.pasted, (unsigned long long)npasted);
}

// cc_clone_mark_dev: flush()'s bitmap step after a write log.  Every page that
// a valid entry (the write log's contract) covers WHOLE and whose chunk is a
// clone gets its bit set; a partly covered page keeps its bit.
__global__ __launch_bounds__(64 * kCloneWaves) void clone_mark_kernel(CloneMarkLaunch a) {
    const uint32_t lane = threadIdx.x & 63u;
    clone_entry_pages(
        a.n, lane,
        [&](uint64_t i, uint64_t& p0, uint64_t& cnt) {
            const UpdateDesc u = a.log[i];
            if (!u.len || u.len > a.max_len || u.dst >= a.pool_bytes || u.len > a.pool_bytes - u.dst) return;
            const uint64_t first = (u.dst >> a.page_shift) + ((u.dst & (uint64_t)(a.page_bytes - 1u)) ? 1u : 0u);
            const uint64_t end = (u.dst + u.len) >> a.page_shift;
            p0 = first;
            cnt = end > first ? end - first : 0u;
        },
        [&](uint64_t, uint64_t page) {
            const uint64_t c = clone_chunk_of(a.geo, page);
            const uint32_t q = (uint32_t)(page - c * a.geo.pages_per_chunk);
            const uint32_t s = a.geo.clone_slot[c];
            if (s >= a.geo.n_slots) return;
            atomicOr(a.geo.bitmap + (uint64_t)s * a.geo.words_per_slot + (q >> 5), 1u << (q & 31u));
        });
}

// cc_apply_logs_cow_dev's pass before the queue: copy2Snapshot and flush()'s
// bitmap step for EVERY batch of a queue at once.  The pairs (entry, page slot)
// of the launch's batches form one index space, split evenly and STATICALLY:
// the space is cut into granules of 16 pairs, a wave step takes four granules a
// quarter of the space apart (lane l: granule s + S (l / 16), pair l % 16 of
// it), and the steps go round the workgroups and then round their waves.  So
// the copies of a skewed queue (all in one batch's first entries) spread over
// as many waves as there are granules in that stretch, not over the few waves a
// contiguous share would give them (measured: DESIGN 6a), with no counter and
// no atomic.  A lane finds its pair's batch with a loop over the descriptors
// (kernel arguments, read with a wave-uniform index), then its entry and the
// entry's k-th page.
//   Snapshot side: a page whose chunk has a slot below n_slots and whose bit
// is not seen set (a plain read may skip a set bit: bits only rise during the
// pass) bids with one atomicOr; the lane that gets the word back with the bit
// clear is the page's only winner among the duplicates (the same page within a
// batch, across batches, or twice in this step).  It moves the page's stored
// CRC; the wave then copies the winners' pages as log_cow_kernel does (two in
// flight, load_page's layout, whole rows, nontemporal stores).  Nothing has
// written the pool yet, so every copy is the page as it stood before the queue.
//   Clone side: where the entry covers the page whole and the chunk's clone
// slot is below n_slots, one atomicOr of its bit unless it is seen set.
//   Verify rehashes every copied page and counts mismatches (still copied with
// the stored CRC); without it no LDS image and no CRC arithmetic.  No spin
// waits; workgroups share the bitmap words and the two counters (one atomicAdd
// a wave each) and nothing else.
template <int M, bool Verify>
__global__ __launch_bounds__(64 * kPrepassWaves) void logs_prepass_kernel(LogsPrepassLaunch a) {
    __shared__ uint32_t tab[Verify ? kLdsBytes / 4 : 1];
    constexpr uint32_t pb = 256u * M;  // = a.page_bytes (launch_logs_prepass picks M)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t S = (((a.n_pairs + 15u) >> 4) + 3u) >> 2;  // wave steps of four granules
    if (blockIdx.x >= S) return;  // (uniform over the workgroup)
    if constexpr (Verify) fill_lds<64 * kPrepassWaves>(tab, static_cast<const uint4*>(a.image));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    const bool cow = a.snap_slot != nullptr, clone = a.clone.clone_slot != nullptr;
    uint32_t ncopied = 0, nstale = 0;
    // consecutive steps go to different workgroups, then to the next wave of each
    for (uint64_t s = (uint64_t)wave * gridDim.x + blockIdx.x; s < S; s += (uint64_t)gridDim.x * kPrepassWaves) {
        const uint64_t pair = ((s + S * (lane >> 4)) << 4) + (lane & 15u);
        const bool on = pair < a.n_pairs;
        const uint64_t idx = on ? pair : 0ull;  // (clamped: the loads below need no branch)
        const UpdateDesc* upd = a.b[0].upd;
        uint64_t pair0 = 0;
        for (uint32_t h = 1; h < a.n_batches; h++) {  // the pair's batch: the last one that starts at or before it
            const uint64_t q0 = a.b[h].pair0;
            if (idx >= q0) {
                upd = a.b[h].upd;
                pair0 = q0;
            }
        }
        const uint32_t t = (uint32_t)(idx - pair0);  // < the batch's n_pairs < 2^31
        const uint32_t i = t / a.slots, k = t - i * a.slots;
        const UpdateDesc d = upd[i];
        // the write log's rule, as insert_piece applies it: an entry that breaks it has no pair
        const bool ok = on && d.len >= 1 && d.len <= a.max_len && d.dst < a.pool_bytes && d.len <= a.pool_bytes - d.dst;
        const uint64_t pg0 = ok ? d.dst >> a.page_shift : 0;
        const uint64_t pg1 = ok ? (d.dst + d.len - 1) >> a.page_shift : 0;
        const bool pok = ok && pg0 + k <= pg1;
        const uint32_t key = pok ? (uint32_t)(pg0 + k) : 0u;  // the page (< 2^32 - 1 pool pages)
        bool win = false;
        uint64_t sidx = 0;  // page of d_snap / entry of d_snap_crcs
        uint32_t oc = 0;
        if (cow) {
            const uint32_t chunk = key / a.pages_per_chunk;
            const uint32_t q = key - chunk * a.pages_per_chunk;  // the page within its chunk
            const uint32_t slot = pok ? a.snap_slot[chunk] : 0xFFFFFFFFu;
            const bool has = pok && slot < a.n_slots;  // CC_NO_SNAPSHOT and any slot out of range: written in place
            uint32_t* word = a.snap_bitmap + ((uint64_t)(has ? slot : 0u) * a.words_per_slot + (q >> 5));
            const uint32_t bit = 1u << (q & 31u);
            if (has && !(*word & bit)) win = !(atomicOr(word, bit) & bit);  // a set bit: the snapshot keeps its first version
            if (win) {
                sidx = (uint64_t)slot * a.pages_per_chunk + q;
                oc = a.page_crcs[key];
                a.snap_crcs[sidx] = oc;  // moved, not recomputed
            }
        }
        if (clone && pok && ((uint64_t)key << a.page_shift) >= d.dst &&
            ((uint64_t)key + 1u) << a.page_shift <= d.dst + d.len) {  // covered whole (cc_clone_mark_dev's rule)
            const uint64_t c = clone_chunk_of(a.clone, key);
            const uint32_t q = (uint32_t)(key - c * a.clone.pages_per_chunk);
            const uint32_t s = a.clone.clone_slot[c];
            if (s < a.clone.n_slots) {
                uint32_t* word = a.clone.bitmap + (uint64_t)s * a.clone.words_per_slot + (q >> 5);
                const uint32_t bit = 1u << (q & 31u);
                if (!(*word & bit)) atomicOr(word, bit);
            }
        }
        uint64_t todo = __ballot(win);
        ncopied += (uint32_t)__popcll(todo);
        while (todo) {
            // two pages in flight: both loads, then both stores
            const uint32_t b0 = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const bool two = todo != 0ull;
            const uint32_t b1 = two ? (uint32_t)__builtin_ctzll(todo) : b0;
            todo &= todo - 1ull;  // (0 stays 0)
            const uint32_t p0 = __builtin_amdgcn_readlane(key, b0), p1 = __builtin_amdgcn_readlane(key, b1);
            const uint64_t d0 = readlane64(sidx, b0), d1 = readlane64(sidx, b1);
            uint32_t w0[M], w1[M];
            load_page<M>(w0, reinterpret_cast<const uint32_t*>(a.pool + (uint64_t)p0 * pb) + lane);
            load_page<M>(w1, reinterpret_cast<const uint32_t*>(a.pool + (uint64_t)p1 * pb) + lane);
            uint32_t* o0 = reinterpret_cast<uint32_t*>(a.snap + d0 * pb) + lane;
            uint32_t* o1 = reinterpret_cast<uint32_t*>(a.snap + d1 * pb) + lane;
#pragma unroll
            for (int j = 0; j < M; j++) __builtin_nontemporal_store(w0[j], o0 + 64 * j);
            if (two) {
#pragma unroll
                for (int j = 0; j < M; j++) __builtin_nontemporal_store(w1[j], o1 + 64 * j);
            }
            if constexpr (Verify) {
                const uint32_t e0 = __builtin_amdgcn_readlane(oc, b0), e1 = __builtin_amdgcn_readlane(oc, b1);
                const uint32_t r0 = wave_xor(apply_fin(tab, chain<M>(tab, w0, c0, c1), cf)) ^ a.kconst;
                nstale += r0 != e0 ? 1u : 0u;
                if (two) {
                    const uint32_t r1 = wave_xor(apply_fin(tab, chain<M>(tab, w1, c0, c1), cf)) ^ a.kconst;
                    nstale += r1 != e1 ? 1u : 0u;
                }
            }
        }
    }
    if (lane == 0) {
        if (a.copied && ncopied) atomicAdd(a.copied, (unsigned long long)ncopied);
        if (Verify && nstale) atomicAdd(a.stale, (unsigned long long)nstale);
    }
}

// ---------------------------------------------------------------------------
// cc_apply_ops_dev: paste batches inside the write-log queue.  Three pass kinds
// before the queue's own launches (BID, RESOLVE, PASTE: kernels.h), each a lane
// per (entry, page slot) pair on logs_prepass_kernel's static split: granules
// of 16 pairs, four a wave step a quarter of the space apart, steps round the
// workgroups and then round their waves.  A page's FIRST SETTER -- the entry of
// the lowest ordinal that is a valid paste covering it or a valid write covering
// it whole -- is found with atomicMin on the page's claim word; the key
// 2 x ordinal + kind orders by ordinal and tells a paste (odd) from a write
// (even).  All-ones (odd, but no key: ordinals stay below 2^31 - 1) is "no bid".
// ---------------------------------------------------------------------------
// The pair a lane holds in wave step s of S: its batch's descriptor (found with
// a loop over the kernel argument, wave-uniform index), its entry's record and
// ordinal, and the page slot k within the entry.
struct OpsPair {
    bool on;             // a pair of the launch (the rest is pair 0's when not)
    UpdateDesc d;
    uint32_t h;          // descriptor index
    uint32_t i, k;       // entry of the batch, page slot of the entry
    uint32_t ord, kind;  // the entry's ordinal; the batch's kind
    uint64_t src_bytes;  // the batch's (paste)
};
__device__ __forceinline__ OpsPair ops_pair_of(const OpsLaunch& a, uint64_t s, uint64_t S, uint32_t lane) {
    OpsPair p;
    const uint64_t pair = ((s + S * (lane >> 4)) << 4) + (lane & 15u);
    p.on = pair < a.n_pairs;
    const uint64_t idx = p.on ? pair : 0ull;  // (clamped: the loads below need no branch)
    const UpdateDesc* recs = a.b[0].recs;
    uint64_t pair0 = 0;
    p.h = 0;
    p.ord = a.b[0].ord0;
    p.kind = a.b[0].kind;
    p.src_bytes = a.b[0].src_bytes;
    for (uint32_t h = 1; h < a.n_batches; h++) {  // the pair's batch: the last one that starts at or before it
        const uint64_t q0 = a.b[h].pair0;
        if (idx >= q0) {
            recs = a.b[h].recs;
            pair0 = q0;
            p.h = h;
            p.ord = a.b[h].ord0;
            p.kind = a.b[h].kind;
            p.src_bytes = a.b[h].src_bytes;
        }
    }
    const uint32_t t = (uint32_t)(idx - pair0);  // < the batch's pairs < 2^32 (checked by the host)
    const uint32_t per = p.kind == kOpPaste ? a.paste_slots : a.slots;
    p.i = t / per;
    p.k = t - p.i * per;
    p.ord += p.i;
    p.d = recs[p.i];
    return p;
}
// the write log's rule, as insert_piece applies it
__device__ __forceinline__ bool ops_write_ok(const OpsLaunch& a, const UpdateDesc& d) {
    return d.len >= 1 && d.len <= a.max_len && d.dst < a.pool_bytes && d.len <= a.pool_bytes - d.dst;
}
// cc_paste_dev's rule (paste_bad) and len <= max_paste_len, which bounds an entry's pairs (len == 0 is valid)
__device__ __forceinline__ bool ops_paste_bad(const OpsLaunch& a, const UpdateDesc& u, uint64_t src_bytes) {
    if (!u.len) return false;
    if ((u.dst | u.len) & (uint64_t)(a.page_bytes - 1u)) return true;
    if (u.len > a.max_paste_len) return true;
    if (u.dst >= a.pool_bytes || u.len > a.pool_bytes - u.dst) return true;
    return (u.src & 3u) || u.src > src_bytes || u.len > src_bytes - u.src;
}
// A page of the pool behind the clone tables: its claim word's index, or false
// for a page of a chunk that is no clone.  `page` lies inside the pool.
__device__ __forceinline__ bool ops_claim_of(const CloneGeo& g, uint64_t page, uint32_t& s, uint32_t& q, uint64_t& cidx) {
    const uint64_t c = clone_chunk_of(g, page);
    q = (uint32_t)(page - c * g.pages_per_chunk);
    s = g.clone_slot[c];
    if (s >= g.n_slots) return false;
    cidx = (uint64_t)s * g.pages_per_chunk + q;
    return true;
}

// BID: no page traffic.  A valid paste pair, and a valid write pair that covers
// its page whole, bids with its key where the page's chunk is a clone and its
// bit is clear; the lowest key holds the claim word when every BID launch of
// the call has ended.  The lane with page slot 0 of an invalid paste entry
// marks it.  Reads the bitmap and writes none (the bits rise in PASTE and in the
// queue's own pass, both later on the stream).
__global__ __launch_bounds__(64 * kOpsWaves) void ops_bid_kernel(OpsLaunch a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t S = (((a.n_pairs + 15u) >> 4) + 3u) >> 2;  // wave steps of four granules
    if (blockIdx.x >= S) return;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t s = (uint64_t)wave * gridDim.x + blockIdx.x; s < S; s += (uint64_t)gridDim.x * kOpsWaves) {
        const OpsPair p = ops_pair_of(a, s, S, lane);
        const bool paste = p.kind == kOpPaste;
        const bool bad = p.on && paste && ops_paste_bad(a, p.d, p.src_bytes);
        uint64_t mark = __ballot(bad && p.k == 0);
        while (mark) {  // (rare) the entry's word lies behind its batch's pointer: a uniform descriptor index
            const uint32_t b = (uint32_t)__builtin_ctzll(mark);
            mark &= mark - 1ull;
            uint32_t* per = a.b[__builtin_amdgcn_readlane(p.h, b)].pasted_per_entry;
            if (lane == b) per[p.i] = 0xFFFFFFFFu;
        }
        const uint64_t page = (p.d.dst >> a.page_shift) + p.k;
        bool bid;
        if (paste)
            bid = p.on && !bad && p.k < (p.d.len >> a.page_shift);
        else  // covered whole (cc_clone_mark_dev's rule); dst + len <= pool_bytes: no overflow
            bid = p.on && ops_write_ok(a, p.d) && (page << a.page_shift) >= p.d.dst &&
                  ((page + 1u) << a.page_shift) <= p.d.dst + p.d.len;
        if (!bid) continue;
        uint32_t sl, q;
        uint64_t cidx;
        if (!ops_claim_of(a.geo, page, sl, q, cidx)) continue;
        const uint32_t word = a.geo.bitmap[(uint64_t)sl * a.geo.words_per_slot + (q >> 5)];
        if ((word >> (q & 31u)) & 1u) continue;  // written before the queue: nobody sets it again
        atomicMin(a.geo.claim + cidx, 2u * p.ord + p.kind);
    }
}

// RESOLVE: the write pairs of the batches that bid, after every BID launch.  A
// whole cover that finds its own key is the page's first setter: no paste lands
// there, and the pair puts all-ones back.  A partial cover that finds the key of
// a paste of a HIGHER ordinal is contested: in the per-batch sequence that paste
// would bury the write, here the write lands on the pasted bytes.  The resets
// run beside these reads, and harmlessly: a word being reset holds a write key
// (even) or all-ones, and neither counts.  One LDS add a wave and one global
// add a workgroup: the kernel is so short that every wave's add to the one
// counter arrived at once, and 8,192 of them in a row took most of its time
// (measured: DESIGN 6a, "Pastes inside the queue").
__global__ __launch_bounds__(64 * kOpsWaves) void ops_resolve_kernel(OpsLaunch a) {
    __shared__ uint32_t block_contested;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t S = (((a.n_pairs + 15u) >> 4) + 3u) >> 2;
    if (blockIdx.x >= S) return;  // (uniform over the workgroup)
    if (threadIdx.x == 0) block_contested = 0;
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t ncontested = 0;  // uniform
    for (uint64_t s = (uint64_t)wave * gridDim.x + blockIdx.x; s < S; s += (uint64_t)gridDim.x * kOpsWaves) {
        const OpsPair p = ops_pair_of(a, s, S, lane);
        const bool ok = p.on && p.kind == kOpWrite && ops_write_ok(a, p.d);
        const uint64_t page = (p.d.dst >> a.page_shift) + p.k;
        const bool touched = ok && page <= (p.d.dst + p.d.len - 1u) >> a.page_shift;
        const bool whole = touched && (page << a.page_shift) >= p.d.dst && ((page + 1u) << a.page_shift) <= p.d.dst + p.d.len;
        bool hit = false;
        uint32_t sl, q;
        uint64_t cidx;
        if (touched && ops_claim_of(a.geo, page, sl, q, cidx)) {
            const uint32_t v = __hip_atomic_load(a.geo.claim + cidx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (whole) {
                if (v == 2u * p.ord)
                    __hip_atomic_store(a.geo.claim + cidx, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                hit = v != 0xFFFFFFFFu && (v & 1u) && (v >> 1) > p.ord;
            }
        }
        ncontested += (uint32_t)__popcll(__ballot(hit));
    }
    if (lane == 0 && ncontested) atomicAdd(&block_contested, ncontested);
    __syncthreads();
    if (threadIdx.x == 0 && block_contested && a.contested) atomicAdd(a.contested, (unsigned long long)block_contested);
}

// PASTE: the pairs of the paste batches, after every RESOLVE launch.  The pair
// that finds its own key in the claim word is the page's winner; the wave walks
// its winners by ballot, one page ahead of the hash: the source page is loaded from the
// winner's batch's buffer (the descriptor read with a uniform index), hashed as
// it passes through the registers and stored; the winner's own lane then writes
// the CRC, ORs the bit, counts the page on its entry and puts all-ones back.
// Every other pair moves no page.  paste_kernel's argument holds: a loser reads
// the winner's key or all-ones, never its own (only the pairs of entry e ever
// write e's key, one page each, and only the pair that found it resets it).
template <int M>
__global__ __launch_bounds__(64 * kOpsWaves) void ops_paste_kernel(OpsLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t S = (((a.n_pairs + 15u) >> 4) + 3u) >> 2;
    if (blockIdx.x >= S) return;  // (uniform over the workgroup)
    fill_lds<64 * kOpsWaves>(tab, static_cast<const uint4*>(a.image));
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    uint32_t npasted = 0;  // uniform
    for (uint64_t s = (uint64_t)wave * gridDim.x + blockIdx.x; s < S; s += (uint64_t)gridDim.x * kOpsWaves) {
        const OpsPair p = ops_pair_of(a, s, S, lane);
        const bool ok = p.on && p.kind == kOpPaste && !ops_paste_bad(a, p.d, p.src_bytes) &&
                        p.k < (p.d.len >> a.page_shift);
        const uint64_t page = (p.d.dst >> a.page_shift) + p.k;
        const uint64_t from = p.d.src + ((uint64_t)p.k << a.page_shift);  // < src_bytes for a valid pair
        bool win = false;
        uint32_t sl = 0, q = 0;
        uint64_t cidx = 0;
        if (ok && ops_claim_of(a.geo, page, sl, q, cidx)) win = a.geo.claim[cidx] == 2u * p.ord + kOpPaste;
        uint64_t todo = __ballot(win);
        npasted += (uint32_t)__popcll(todo);
        if (!todo) continue;
        // the winners in lane order, one page ahead: the next winner's page is on its way
        // while this one is hashed and stored
        auto src_of = [&](uint32_t b) {
            const uint32_t h = __builtin_amdgcn_readlane(p.h, b);
            return reinterpret_cast<const uint32_t*>(a.b[h].src + readlane64(from, b)) + lane;
        };
        uint32_t b = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        uint32_t cur[M], nxt[M];
        load_page<M>(cur, src_of(b));
        for (;;) {
            const bool more = todo != 0ull;
            const uint32_t bn = more ? (uint32_t)__builtin_ctzll(todo) : b;
            todo &= todo - 1ull;  // (0 stays 0)
            if (more) load_page<M>(nxt, src_of(bn));
            const uint32_t r = wave_xor(apply_fin(tab, chain<M>(tab, cur, c0, c1), cf)) ^ a.kconst;
            store_page<M>(cur, a.pool + (readlane64(page, b) << (a.page_shift - 2u)) + lane);
            uint32_t* per = a.b[__builtin_amdgcn_readlane(p.h, b)].pasted_per_entry;
            if (lane == b) {  // the winner's own lane: its page, slot, entry
                a.page_crcs[page] = r;
                atomicOr(a.geo.bitmap + (uint64_t)sl * a.geo.words_per_slot + (q >> 5), 1u << (q & 31u));
                atomicAdd(per + p.i, 1u);
                __hip_atomic_store(a.geo.claim + cidx, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (!more) break;
#pragma unroll
            for (int j = 0; j < M; j++) cur[j] = nxt[j];
            b = bn;
        }
    }
    if (npasted && lane == 0 && a.pasted) atomicAdd(a.pasted, (unsigned long long)npasted);
}

// cc_clone_check_reads_dev: Read's NextClearBit test for a batch.  Every page a
// read touches that lies in a clone chunk with a clear bit counts on its read;
// a read past the pool is marked by the lane that loads it.
__global__ __launch_bounds__(64 * kCloneWaves) void clone_check_kernel(CloneCheckLaunch a) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t mine = 0;  // this lane's hits, summed over the wave for the total
    clone_entry_pages(
        a.n, lane,
        [&](uint64_t i, uint64_t& p0, uint64_t& cnt) {
            const RangeDesc r = a.reads[i];
            if (!r.len) return;
            if (r.off >= a.pool_bytes || r.len > a.pool_bytes - r.off) {
                a.unwritten_per_read[i] = 0xFFFFFFFFu;
                return;
            }
            p0 = r.off >> a.page_shift;
            cnt = ((r.off + r.len - 1) >> a.page_shift) - p0 + 1;
        },
        [&](uint64_t e, uint64_t page) {
            const uint64_t c = clone_chunk_of(a.geo, page);
            const uint32_t q = (uint32_t)(page - c * a.geo.pages_per_chunk);
            const uint32_t s = a.geo.clone_slot[c];
            if (s >= a.geo.n_slots) return;
            const uint32_t word = a.geo.bitmap[(uint64_t)s * a.geo.words_per_slot + (q >> 5)];
            if ((word >> (q & 31u)) & 1u) return;
            atomicAdd(a.unwritten_per_read + e, 1u);
            mine++;
        });
#pragma unroll
    for (int d = 32; d; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (mine && lane == 0) atomicAdd(a.unwritten_total, (unsigned long long)mine);
}

// ---------------------------------------------------------------------------
// Clone reads (cc_read_merge_dev): snap_read_kernel's schedule, every page
// slot resolved against its chunk's written-page bitmap, the written pages
// rehashed and delivered from the pool, the never-written ones delivered from
// the read's fetched origin buffer.  Replaces the host loops of
// CloneCore::ReadThenMerge (clone_core.cpp:352-416: Divide() into copied and
// uncopied ranges, ReadChunk per copied range, cloneData->copy_to per uncopied
// one).
// ---------------------------------------------------------------------------
// A read that is not served: misaligned, past the pool, an output range that
// is unaligned or leaves the buffer, or -- with an origin (go != kNoOrigin) --
// an origin range that is unaligned or leaves its buffer (len == 0 is valid).
__device__ __forceinline__ bool merge_read_bad(const MergeReadLaunch& a, const RangeDesc& r, uint64_t oo, uint64_t go) {
    if (!r.len) return false;
    if ((r.off | r.len) & (uint64_t)(a.rv.page_bytes - 1u)) return true;
    if (r.off >= a.rv.pool_bytes || r.len > a.rv.pool_bytes - r.off) return true;
    if ((oo & 3u) || oo > a.out_bytes || r.len > a.out_bytes - oo) return true;
    return go != kNoOrigin && ((go & 3u) || go > a.origin_bytes || r.len > a.origin_bytes - go);
}
__device__ __forceinline__ uint64_t merge_pages(const MergeReadLaunch& a, const RangeDesc& r, uint64_t oo, uint64_t go) {
    return merge_read_bad(a, r, oo, go) ? 0u : read_pages(a.rv, r);
}

// Pages of tile t, uniform; mark: invalid reads get both of their words = UINT32_MAX
// (the tile's counting wave marks them, as snap_tile_count does).
__device__ __forceinline__ uint64_t merge_tile_count(const MergeReadLaunch& a, uint32_t t, uint32_t lane, bool mark) {
    const uint64_t lo = a.rv.n_reads * t / kReadTiles, hi = a.rv.n_reads * (t + 1) / kReadTiles;
    uint64_t sum = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) {
        const RangeDesc r = a.rv.reads[i];
        const bool bad = merge_read_bad(a, r, a.out_off[i], a.origin ? a.origin_off[i] : kNoOrigin);
        sum += bad ? 0u : read_pages(a.rv, r);
        if (mark && bad) {
            a.rv.bad_per_read[i] = 0xFFFFFFFFu;
            a.unwritten_per_read[i] = 0xFFFFFFFFu;
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return sum;
}

// One page slot on its way to its loads, resolved in the stages SnapPg goes
// through: merge_slot_of (chunk, page in chunk, the chunk's bitmap slot),
// merge_word_of (the slot's bitmap word), merge_unwritten (the bit, inverted:
// a CLEAR bit of a clone chunk sends the page away from the pool).  Both table
// words come in with vector loads of a uniform address and stay in a VGPR until
// the next stage takes them a step later.
struct MergePg : RvSlot {  // owner: lane holding the page's read; rel: the page's position in it; g: pool page
    uint32_t q;      // page in chunk
    uint32_t s;      // the chunk's bitmap slot (>= n_slots: not a clone), once merge_word_of has taken it
    uint32_t sv;     // VGPR: the slot as loaded
    uint32_t wv;     // VGPR: the slot's bitmap word holding bit q, as loaded
};
__device__ __forceinline__ void merge_slot_of(const MergeReadLaunch& a, MergePg& p, uint32_t vz) {
    p.q = 0;
    p.s = 0xFFFFFFFFu;
    p.sv = 0xFFFFFFFFu;
    p.wv = 0xFFFFFFFFu;
    if (!a.geo.n_slots) return;  // uniform: no clone chunk, nothing to resolve
    const uint64_t c = clone_chunk_of(a.geo, p.g);
    p.q = (uint32_t)(p.g - c * a.geo.pages_per_chunk);
    p.sv = a.geo.clone_slot[c + vz];
}
__device__ __forceinline__ void merge_word_of(const MergeReadLaunch& a, MergePg& p, uint32_t vz) {
    if (!a.geo.n_slots) return;
    p.s = __builtin_amdgcn_readfirstlane(p.sv);
    const uint32_t sc = p.s < a.geo.n_slots ? p.s : 0u;  // clamped: the same load every page
    p.wv = a.geo.bitmap[(uint64_t)sc * a.geo.words_per_slot + (p.q >> 5) + vz];
}
__device__ __forceinline__ bool merge_unwritten(const MergeReadLaunch& a, const MergePg& p) {
    if (!a.geo.n_slots) return false;
    const uint32_t word = __builtin_amdgcn_readfirstlane(p.wv);
    return p.s < a.geo.n_slots && !((word >> (p.q & 31u)) & 1u);
}
// A slot whose loads are out.  Its three outcomes, uniform: the live page
// (stored CRC and page loaded: hash, compare, store), the origin's page (page
// loaded: store), nothing (counted only).
constexpr uint32_t kMergeLive = 0, kMergeOrigin = 1, kMergeNone = 2;
struct MergeDst {
    uint64_t out;    // the page's byte offset in the output
    uint32_t owner;
    uint32_t kind;
    uint32_t crc;    // VGPR: the live page's stored CRC
};
__device__ __forceinline__ const uint32_t* merge_live_page(const MergeReadLaunch& a, uint64_t g) {
    return a.rv.pool + (g << (a.rv.page_shift - 2u));
}

// The never-written pages of a wave's share come in runs of one read: a run is
// held in two SGPRs and lands on its read with ONE lane-0 atomic when the next
// read's first unwritten page arrives or the group of reads ends; the total
// goes out once a wave.
struct MergeRun {
    uint32_t owner, count;  // uniform: the pending run's read (lane of the group) and its pages
    uint64_t total;         // uniform: this wave's unwritten pages
};
__device__ __forceinline__ void merge_run_flush(const MergeReadLaunch& a, MergeRun& u, uint64_t base, uint32_t lane) {
    if (!u.count) return;
    if (lane == 0) atomicAdd(a.unwritten_per_read + base + u.owner, u.count);
    u.total += u.count;
    u.count = 0;
}
__device__ __forceinline__ void merge_run_add(const MergeReadLaunch& a, MergeRun& u, uint64_t base, uint32_t owner,
                                              uint32_t lane) {
    if (u.owner != owner) merge_run_flush(a, u, base, lane);
    u.owner = owner;
    u.count++;
}

// snap_read_kernel<M, true> with the clone resolution: the same tile counts,
// shares, dynamic tail and three rotating register sets; the step that handles
// page k first takes the table words loaded a step earlier, issues page k+3's
// bitmap-word load and page k+4's slot load, and then page k+2's loads -- the
// stored CRC and the pool page, the origin page, or none.  Lane j of a group
// of 64 reads holds its read's output offset and its origin offset.
// This kernel keeps its own copy of the slot schedule and the group walk
// (rv_begin, rv_next and rv_walk above, written out): on the shared functions
// its count-only path (every page never written, no origin: no page traffic
// to hide the scalar work behind) measured 5.5 % slower, 0.290 ms against the
// parent's 0.2743-0.2749 ms over three runs (profiles/gather_refactor_ab.txt).  A change to the schedule is made here too.
template <int M>
__global__ __launch_bounds__(64 * kRvWaves) void merge_read_kernel(MergeReadLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint64_t n = a.rv.n_reads;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t Wg = (uint64_t)gridDim.x * kRvWaves;
    const uint64_t w = (uint64_t)blockIdx.x * kRvWaves + wave;
    const uint64_t tag = (uint64_t)a.rv.epoch << kEpochShift;
    for (uint64_t t = w; t < kReadTiles; t += Wg) {
        const uint64_t cnt = merge_tile_count(a, (uint32_t)t, lane, true);
        if (lane == 0) __hip_atomic_store(a.rv.tiles + t, tag | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned long long* dyn_ctr = a.rv.tail + (a.rv.epoch & 1u) * kDynCtrWords64;
    if (blockIdx.x == 0 && threadIdx.x < kRvHeads)
        atomicExch(a.rv.tail + ((a.rv.epoch + 1u) & 1u) * kDynCtrWords64 + threadIdx.x * kDynHeadStride, 0ull);
    fill_lds<64 * kRvWaves>(tab, static_cast<const uint4*>(a.rv.image));
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));  // opaque zero: keeps uniform-address loads on the vector path

    constexpr int kTpl = kReadTiles / 64;
    uint64_t tb[kTpl];
    wait_tiles<kTpl>(tb, a.rv.tiles, tag, lane, [&](uint32_t t) { return merge_tile_count(a, t, lane, false); });
    uint64_t lsum = 0;
#pragma unroll
    for (int j = 0; j < kTpl; j++) lsum += tb[j];
    const uint64_t cum = wave_scan_incl(lsum, lane);
    const uint64_t T = readlane64(cum, 63);
    const uint64_t Wt = (T + kRvMinSlots - 1) / kRvMinSlots;
    const uint64_t W = Wt < Wg ? (Wt ? Wt : 1) : Wg;
    if ((uint64_t)blockIdx.x * kRvWaves >= W) return;  // uniform per block: no share, no tail
    const uint64_t Ts = T - T / kRvDynDiv;
    uint32_t dyn_head, dyn_tried;
    tail_cursor<kRvHeads>(dyn_head, dyn_tried);
    uint64_t lo_slot = w < W ? Ts * w / W : Ts, hi_slot = w < W ? Ts * (w + 1) / W : Ts;  // waves past W: tail only
    MergeRun run = {0u, 0u, 0ull};
#pragma unroll 1
    for (;;) {
        uint64_t base = n, S = 0;
        RangeDesc rs;
        uint64_t os = 0, gs = kNoOrigin;
        bool have_rs = false;
        if (lo_slot < hi_slot) {
            const TileHit th = tile_of(cum, tb, lo_slot, lane);
            base = n * th.tile / kReadTiles;
            S = th.before;
            for (;;) {
                const uint64_t ri = base + lane;
                const uint64_t at = (ri < n ? ri : base) + vz;
                rs = a.rv.reads[at];
                os = a.out_off[at];
                gs = a.origin ? a.origin_off[at] : kNoOrigin;
                const uint64_t c = wave_scan_incl(ri < n ? merge_pages(a, rs, os, gs) : 0u, lane);
                const uint64_t tot = readlane64(c, 63);
                if (S + tot > lo_slot || base + 64 >= n) break;
                S += tot;
                base += 64;
            }
            have_rs = true;
        }
        for (; base < n && S < hi_slot; base += 64) {
            const uint64_t ri = base + lane;
            const bool valid = ri < n;
            const uint64_t at = (valid ? ri : base) + vz;
            const RangeDesc r = have_rs ? rs : a.rv.reads[at];
            const uint64_t oo = have_rs ? os : a.out_off[at];
            const uint64_t go = have_rs ? gs : a.origin ? a.origin_off[at] : kNoOrigin;
            have_rs = false;
            const uint32_t cnt = valid ? (uint32_t)merge_pages(a, r, oo, go) : 0u;  // 0 also for invalid reads
            const uint64_t p0 = r.off >> a.rv.page_shift;
            uint32_t cum32 = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(cum32, d, 64);
                if (lane >= (uint32_t)d) cum32 += o;
            }
            const uint32_t P = __builtin_amdgcn_readlane(cum32, 63);
            const uint32_t ks = lo_slot > S ? (uint32_t)(lo_slot - S) : 0u;
            const uint32_t ke = hi_slot - S < (uint64_t)P ? (uint32_t)(hi_slot - S) : P;
            S += P;
            if (ks >= ke) continue;
            // slot k (clamped to the share's last): its read's lane, its page, its chunk's bitmap slot
            auto locate = [&](uint32_t k) {
                k = k < ke ? k : ke - 1;
                MergePg p;
                p.owner = (uint32_t)__builtin_ctzll(__ballot(cum32 > k));
                const uint32_t before = p.owner ? (uint32_t)__builtin_amdgcn_readlane(cum32, p.owner - 1) : 0u;
                p.rel = k - before;
                p.g = readlane64(p0, p.owner) + p.rel;
                merge_slot_of(a, p, vz);
                return p;
            };
            // the resolved page's outcome, output offset and loads; then the page
            // behind it moves up: its bitmap word, and the slot of the one after
            MergePg p3, p4;
            auto issue = [&](uint32_t kn, uint32_t (&Y)[M], MergeDst& dy) {
                const bool unwritten = merge_unwritten(a, p3);
                const uint64_t from = readlane64(go, p3.owner);
                const uint64_t in_read = (uint64_t)p3.rel << a.rv.page_shift;
                const uint64_t g = p3.g;
                dy.owner = p3.owner;
                dy.kind = !unwritten ? kMergeLive : from != kNoOrigin ? kMergeOrigin : kMergeNone;
                dy.out = readlane64(oo, p3.owner) + in_read;
                dy.crc = 0;
                p3 = p4;
                merge_word_of(a, p3, vz);
                p4 = locate(kn);
                __builtin_amdgcn_sched_barrier(0);  // the table loads stay ahead of the page's
                if (dy.kind == kMergeLive) {
                    dy.crc = a.rv.page_crcs[g + vz];
                    load_page<M>(Y, merge_live_page(a, g) + lane);
                } else if (dy.kind == kMergeOrigin) {
                    load_page<M>(Y, reinterpret_cast<const uint32_t*>(a.origin + from + in_read) + lane);
                }
            };
            uint32_t A[M], B[M], Cq[M];
            MergeDst dA, dB, dC;
            p3 = locate(ks);
            merge_word_of(a, p3, vz);
            p4 = locate(ks + 1);
            issue(ks + 2, A, dA);
            issue(ks + 3, B, dB);
            dC = dB;
            // page k (registers X unless its outcome is none); page k+2's loads go into Y
            auto step = [&](uint32_t (&X)[M], const MergeDst dx, uint32_t k, uint32_t (&Y)[M], MergeDst& dy) {
                const bool more = k + 1 < ke;
                issue(k + 4, Y, dy);
                uint32_t* to = reinterpret_cast<uint32_t*>(a.out + dx.out) + lane;
                if (dx.kind == kMergeLive) {
                    const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.rv.kconst;
                    store_page<M>(X, to);
                    if (crc != dx.crc && lane == 0) {
                        atomicAdd(a.rv.bad_per_read + base + dx.owner, 1u);
                        atomicAdd(a.rv.bad_total, 1ull);
                    }
                } else {
                    if (dx.kind == kMergeOrigin) store_page<M>(X, to);
                    merge_run_add(a, run, base, dx.owner, lane);
                }
                return more;
            };
            for (uint32_t k = ks;; k += 3) {
                if (!step(A, dA, k, Cq, dC)) break;
                if (!step(B, dB, k + 1, A, dA)) break;
                if (!step(Cq, dC, k + 2, B, dB)) break;
            }
            merge_run_flush(a, run, base, lane);  // a run never outlives its group of reads
        }
        const uint64_t n_dyn = (T - Ts + kRvDynSlots - 1) / kRvDynSlots;
        const uint64_t c = tail_pull<kRvHeads>(dyn_ctr, n_dyn, dyn_head, dyn_tried, lane);
        if (c >= n_dyn) break;
        lo_slot = Ts + c * kRvDynSlots;
        hi_slot = lo_slot + kRvDynSlots < T ? lo_slot + kRvDynSlots : T;
    }
    if (run.total && lane == 0) atomicAdd(a.unwritten_total, (unsigned long long)run.total);
}

// <= 64 reads (one per lane) in ONE launch (rv_small_begin): a wave resolves
// the next page while it handles one.
template <int M>
__global__ __launch_bounds__(64 * kRvWaves) void merge_read_small_kernel(MergeReadLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));
    uint64_t oo = 0, go = kNoOrigin;  // the lane's read's output and origin offsets
    RvSmallShare sm;
    if (!rv_small_begin(sm, tab, a.rv, lane, [&](uint32_t i, bool mark) -> RvEntry {
            const uint32_t at = i + vz;
            const RangeDesc r = a.rv.reads[at];
            oo = a.out_off[at];
            go = a.origin ? a.origin_off[at] : kNoOrigin;
            const bool bad = merge_read_bad(a, r, oo, go);
            if (mark && bad) {
                a.rv.bad_per_read[i] = 0xFFFFFFFFu;
                a.unwritten_per_read[i] = 0xFFFFFFFFu;
            }
            return {bad ? 0u : read_pages(a.rv, r), r.off >> a.rv.page_shift};
        }))
        return;
    const uint32_t k0 = sm.k0, k1 = sm.k1;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    auto locate = [&](uint32_t k) {
        MergePg p = {slot_at(sm.cum, sm.p0, k < k1 ? k : k1 - 1)};
        merge_slot_of(a, p, vz);
        merge_word_of(a, p, vz);
        return p;
    };
    auto issue = [&](const MergePg& p, uint32_t (&Y)[M], MergeDst& dy) {
        const bool unwritten = merge_unwritten(a, p);
        const uint64_t from = readlane64(go, p.owner);
        const uint64_t in_read = (uint64_t)p.rel << a.rv.page_shift;
        dy.owner = p.owner;
        dy.kind = !unwritten ? kMergeLive : from != kNoOrigin ? kMergeOrigin : kMergeNone;
        dy.out = readlane64(oo, p.owner) + in_read;
        dy.crc = 0;
        if (dy.kind == kMergeLive) {
            dy.crc = a.rv.page_crcs[p.g + vz];
            load_page<M>(Y, merge_live_page(a, p.g) + lane);
        } else if (dy.kind == kMergeOrigin) {
            load_page<M>(Y, reinterpret_cast<const uint32_t*>(a.origin + from + in_read) + lane);
        }
    };
    // pages k0 .. k1-1, the next page's loads in flight while one is handled
    uint32_t X[M], Y[M];
    MergeDst dx, dy;
    MergeRun run = {0u, 0u, 0ull};
    issue(locate(k0), X, dx);
    MergePg pn = locate(k0 + 1);
    for (uint32_t k = k0; k < k1; k++) {
        issue(pn, Y, dy);  // clamped: same loads every step
        pn = locate(k + 2);
        uint32_t* to = reinterpret_cast<uint32_t*>(a.out + dx.out) + lane;
        if (dx.kind == kMergeLive) {
            const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.rv.kconst;
            store_page<M>(X, to);
            if (crc != dx.crc && lane == 0) {
                atomicAdd(a.rv.bad_per_read + dx.owner, 1u);
                atomicAdd(a.rv.bad_total, 1ull);
            }
        } else {
            if (dx.kind == kMergeOrigin) store_page<M>(X, to);
            merge_run_add(a, run, 0, dx.owner, lane);
        }
#pragma unroll
        for (int j = 0; j < M; j++) X[j] = Y[j];
        dx = dy;
    }
    merge_run_flush(a, run, 0, lane);
    if (run.total && lane == 0) atomicAdd(a.unwritten_total, (unsigned long long)run.total);
}

// ---------------------------------------------------------------------------
// Page repair (cc_repair_dev): a peer's copy of a page enters the pool only
// when it hashes to the CRC on record.  A sibling of the paste pair above: the
// same ordered batch of UpdateDesc entries, the same claim launch, the same
// (entry, page) slots on verify-on-read's schedule; the gate is a hash
// comparison where paste's is a bitmap bit, and the claim table is indexed by
// pool page (there are no chunks here).
// ---------------------------------------------------------------------------
// An entry that cc_repair_dev skips whole: cc_paste_dev's rule (paste_bad).
__device__ __forceinline__ bool repair_bad(const RepairLaunch& a, const UpdateDesc& u) {
    if (!u.len) return false;
    if ((u.dst | u.len) & (uint64_t)(a.page_bytes - 1u)) return true;
    if (u.dst >= a.pool_bytes || u.len > a.pool_bytes - u.dst) return true;
    return (u.src & 3u) || u.src > a.src_bytes || u.len > a.src_bytes - u.src;
}
__device__ __forceinline__ uint32_t repair_pages(const RepairLaunch& a, const UpdateDesc& u) {
    return repair_bad(a, u) ? 0u : u.len >> a.page_shift;
}

// Launch 1 of cc_repair_dev: every (valid entry, page) pair bids for its page
// with its entry index; the lowest index holds the claim word when the launch
// ends.  The lane that loads an invalid entry marks its four count words.
// Moves no page and reads no table.
__global__ __launch_bounds__(64 * kCloneWaves) void repair_claim_kernel(RepairLaunch a) {
    const uint32_t lane = threadIdx.x & 63u;
    clone_entry_pages(
        a.n, lane,
        [&](uint64_t i, uint64_t& p0, uint64_t& cnt) {
            const UpdateDesc u = a.reqs[i];
            if (repair_bad(a, u)) {
                for (int j = 0; j < 4; j++) a.per_entry[4 * i + j] = 0xFFFFFFFFu;
                return;
            }
            p0 = u.dst >> a.page_shift;
            cnt = u.len >> a.page_shift;
        },
        [&](uint64_t e, uint64_t page) { atomicMin(a.claim + page, (uint32_t)e); });
}

// Pages of tile t of the repair batch, uniform (paste_tile_count's twin).
__device__ __forceinline__ uint64_t repair_tile_count(const RepairLaunch& a, uint32_t t, uint32_t lane) {
    const uint64_t lo = a.n * t / kReadTiles, hi = a.n * (t + 1) / kReadTiles;
    uint64_t sum = 0;
    for (uint64_t i = lo + lane; i < hi; i += 64) sum += repair_pages(a, a.reqs[i]);
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return sum;
}

// One (entry, page) slot of the repair launch on its way to its loads: located
// (its entry's lane, its pool page) with the page's claim word loaded at once,
// by a vector load of a uniform address that stays in a VGPR until the slot's
// loads are issued two steps later.
struct RepairPg {
    uint64_t g;      // pool page
    uint32_t owner;  // lane holding the page's entry
    uint32_t rel;    // the page's position in its entry
    uint32_t cv;     // VGPR: the page's claim word as loaded
};
// A slot whose loads are out: the page it handles when it holds the claim.
struct RepairDst {
    uint64_t g;
    uint64_t from;   // the candidate page's byte offset in the source
    uint32_t owner;
    uint32_t ev;     // VGPR: the CRC on record for the page (expect[g], or page_crcs[g])
    bool win;
};

// The shadowed slots of a wave's share come in runs of one entry (an entry
// whose pages all belong to lower-indexed ones): MergeRun's scheme, the run in
// two SGPRs and ONE lane-0 atomic on the entry's fourth word when the next
// entry's first shadowed slot arrives or the group of entries ends.
struct RepairRun {
    uint32_t owner, count;  // uniform: the pending run's entry (lane of the group) and its slots
    uint64_t total;         // uniform: this wave's shadowed slots
};
__device__ __forceinline__ void repair_run_flush(const RepairLaunch& a, RepairRun& u, uint64_t base, uint32_t lane) {
    if (!u.count) return;
    if (lane == 0) atomicAdd(a.per_entry + 4 * (base + u.owner) + kRepairShadowed, u.count);
    u.total += u.count;
    u.count = 0;
}
__device__ __forceinline__ void repair_run_add(const RepairLaunch& a, RepairRun& u, uint64_t base, uint32_t owner,
                                               uint32_t lane) {
    if (u.owner != owner) repair_run_flush(a, u, base, lane);
    u.owner = owner;
    u.count++;
}

// Launch 2 of cc_repair_dev, on paste_kernel's schedule (tile counts published
// by the waves, shares at slot granularity, 1/16 dynamic tail) over the batch's
// (entry, page) slots.  The slot whose claim word equals its own entry index
// handles the page: the CRC on record and the live page are loaded two steps
// ahead (the table word before the page) and the page is hashed as it passes
// through the registers.  Only when it misses the record is the candidate page
// loaded, there and then, and hashed, and stored when it hits (measured: the
// other waves of the CU hide that wait, and a clean page costs one page read
// instead of two; DESIGN 6b "Page repair").  The lane-0 epilogue mends the
// CRC word, counts the page on its entry by class and puts 0xFFFFFFFF back
// into the claim word.  Every other
// slot is shadowed: no page load, no hash, counted a run at a time.  A loser
// may read the claim word before or after the winner's reset: neither value is
// its own index (paste_kernel's comment), so no third launch is needed.  Only
// the page's handler reads or writes the page and its CRC word, so every page
// is judged by the pool as it stood before the call.
// Like merge_read_kernel this kernel keeps its own copy of the slot schedule
// and the group walk: on the shared functions its two rows without page
// traffic to hide scalar work behind measured slower, every page clean 0.47 %
// and every pair shadowed 0.62 % above the parent's range of five runs
// (profiles/gather_refactor_ab.txt).  A change to the schedule is made here too.
template <int M>
__global__ __launch_bounds__(64 * kRvWaves) void repair_kernel(RepairLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint64_t n = a.n;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t Wg = (uint64_t)gridDim.x * kRvWaves;
    const uint64_t w = (uint64_t)blockIdx.x * kRvWaves + wave;
    const uint64_t tag = (uint64_t)a.epoch << kEpochShift;
    for (uint64_t t = w; t < kReadTiles; t += Wg) {
        const uint64_t cnt = repair_tile_count(a, (uint32_t)t, lane);
        if (lane == 0) __hip_atomic_store(a.tiles + t, tag | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned long long* dyn_ctr = a.tail + (a.epoch & 1u) * kDynCtrWords64;
    if (blockIdx.x == 0 && threadIdx.x < kRvHeads)
        atomicExch(a.tail + ((a.epoch + 1u) & 1u) * kDynCtrWords64 + threadIdx.x * kDynHeadStride, 0ull);
    fill_lds<64 * kRvWaves>(tab, static_cast<const uint4*>(a.image));
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    uint32_t vz = 0;
    asm volatile("" : "+v"(vz));  // opaque zero: keeps uniform-address loads on the vector path
    const uint32_t* record = a.expect ? a.expect : a.page_crcs;

    constexpr int kTpl = kReadTiles / 64;
    uint64_t tb[kTpl];
    wait_tiles<kTpl>(tb, a.tiles, tag, lane, [&](uint32_t t) { return repair_tile_count(a, t, lane); });
    uint64_t lsum = 0;
#pragma unroll
    for (int j = 0; j < kTpl; j++) lsum += tb[j];
    const uint64_t cum = wave_scan_incl(lsum, lane);
    const uint64_t T = readlane64(cum, 63);
    const uint64_t Wt = (T + kRvMinSlots - 1) / kRvMinSlots;
    const uint64_t W = Wt < Wg ? (Wt ? Wt : 1) : Wg;
    if ((uint64_t)blockIdx.x * kRvWaves >= W) return;  // uniform per block: no share, no tail
    const uint64_t Ts = T - T / kRvDynDiv;
    uint32_t dyn_head, dyn_tried;
    tail_cursor<kRvHeads>(dyn_head, dyn_tried);
    uint64_t lo_slot = w < W ? Ts * w / W : Ts, hi_slot = w < W ? Ts * (w + 1) / W : Ts;  // waves past W: tail only
    uint32_t nclean = 0, nrepaired = 0, nfailed = 0;  // uniform: this wave's handled pages, added to the totals once
    RepairRun run = {0u, 0u, 0ull};
#pragma unroll 1
    for (;;) {
        uint64_t base = n, S = 0;
        UpdateDesc us;
        bool have_us = false;
        if (lo_slot < hi_slot) {
            const TileHit th = tile_of(cum, tb, lo_slot, lane);
            base = n * th.tile / kReadTiles;
            S = th.before;
            for (;;) {
                const uint64_t ei = base + lane;
                us = a.reqs[(ei < n ? ei : base) + vz];
                const uint64_t c = wave_scan_incl(ei < n ? repair_pages(a, us) : 0u, lane);
                const uint64_t tot = readlane64(c, 63);
                if (S + tot > lo_slot || base + 64 >= n) break;
                S += tot;
                base += 64;
            }
            have_us = true;
        }
        for (; base < n && S < hi_slot; base += 64) {
            const uint64_t ei = base + lane;
            const bool valid = ei < n;
            const UpdateDesc u = have_us ? us : a.reqs[(valid ? ei : base) + vz];
            have_us = false;
            const uint32_t cnt = valid ? repair_pages(a, u) : 0u;  // 0 also for invalid entries
            const uint64_t p0 = u.dst >> a.page_shift;
            const uint64_t so = u.src;
            uint32_t cum32 = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(cum32, d, 64);
                if (lane >= (uint32_t)d) cum32 += o;
            }
            const uint32_t P = __builtin_amdgcn_readlane(cum32, 63);
            const uint32_t ks = lo_slot > S ? (uint32_t)(lo_slot - S) : 0u;
            const uint32_t ke = hi_slot - S < (uint64_t)P ? (uint32_t)(hi_slot - S) : P;
            S += P;
            if (ks >= ke) continue;
            // slot k (clamped to the share's last): its entry's lane, its page, and the page's claim word on its way
            auto locate = [&](uint32_t k) {
                k = k < ke ? k : ke - 1;
                RepairPg p;
                p.owner = (uint32_t)__builtin_ctzll(__ballot(cum32 > k));
                const uint32_t before = p.owner ? (uint32_t)__builtin_amdgcn_readlane(cum32, p.owner - 1) : 0u;
                p.rel = k - before;
                p.g = readlane64(p0, p.owner) + p.rel;
                p.cv = a.claim[p.g + vz];
                return p;
            };
            // the located slot: does it hold its page's claim?  Then the slot
            // behind it moves up, and the winner's record word and live page are loaded
            RepairPg p3, p4;
            auto issue = [&](uint32_t kn, uint32_t (&Y)[M], RepairDst& dy) {
                const uint32_t holder = __builtin_amdgcn_readfirstlane(p3.cv);
                dy.g = p3.g;
                dy.owner = p3.owner;
                dy.win = holder == (uint32_t)base + p3.owner;
                dy.ev = 0;
                dy.from = readlane64(so, p3.owner) + ((uint64_t)p3.rel << a.page_shift);
                p3 = p4;
                p4 = locate(kn);
                if (dy.win) dy.ev = record[dy.g + vz];
                __builtin_amdgcn_sched_barrier(0);  // the table loads stay ahead of the page's
                if (dy.win) load_page<M>(Y, a.pool + (dy.g << (a.page_shift - 2u)) + lane);
            };
            // slot k (registers X when it won); the loads of slot k + 2 go into Y
            auto step = [&](uint32_t (&X)[M], const RepairDst dx, uint32_t k, uint32_t (&Y)[M], RepairDst& dy) {
                const bool more = k + 1 < ke;
                issue(k + 4, Y, dy);
                if (dx.win) {
                    const uint32_t live = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
                    const uint32_t e = __builtin_amdgcn_readfirstlane(dx.ev);
                    uint32_t cls = kRepairClean;
                    if (live == e) {
                        nclean++;
                    } else {  // the candidate, now: X is free to take it
                        load_page<M>(X, reinterpret_cast<const uint32_t*>(a.src + dx.from) + lane);
                        const uint32_t cand = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
                        if (cand == e) {
                            cls = kRepairRepaired;
                            nrepaired++;
                            store_page<M>(X, a.pool + (dx.g << (a.page_shift - 2u)) + lane);
                        } else {
                            cls = kRepairFailed;
                            nfailed++;
                        }
                    }
                    if (lane == 0) {
                        if (cls == kRepairRepaired || (cls == kRepairClean && a.expect)) a.page_crcs[dx.g] = e;
                        atomicAdd(a.per_entry + 4 * (base + dx.owner) + cls, 1u);
                        __hip_atomic_store(a.claim + dx.g, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else {
                    repair_run_add(a, run, base, dx.owner, lane);
                }
                return more;
            };
            uint32_t A[M], B[M], Cq[M];
            RepairDst dA, dB, dC;
            p3 = locate(ks);
            p4 = locate(ks + 1);
            issue(ks + 2, A, dA);
            issue(ks + 3, B, dB);
            dC = dB;
            for (uint32_t k = ks;; k += 3) {
                if (!step(A, dA, k, Cq, dC)) break;
                if (!step(B, dB, k + 1, A, dA)) break;
                if (!step(Cq, dC, k + 2, B, dB)) break;
            }
            repair_run_flush(a, run, base, lane);  // a run never outlives its group of entries
        }
        const uint64_t n_dyn = (T - Ts + kRvDynSlots - 1) / kRvDynSlots;
        const uint64_t c = tail_pull<kRvHeads>(dyn_ctr, n_dyn, dyn_head, dyn_tried, lane);
        if (c >= n_dyn) break;
        lo_slot = Ts + c * kRvDynSlots;
        hi_slot = lo_slot + kRvDynSlots < T ? lo_slot + kRvDynSlots : T;
    }
    if (lane == 0 && a.totals) {
        if (nclean) atomicAdd(a.totals + kRepairClean, (unsigned long long)nclean);
        if (nrepaired) atomicAdd(a.totals + kRepairRepaired, (unsigned long long)nrepaired);
        if (nfailed) atomicAdd(a.totals + kRepairFailed, (unsigned long long)nfailed);
        if (run.total) atomicAdd(a.totals + kRepairShadowed, (unsigned long long)run.total);
    }
}

__global__ void combine_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t m,
                               uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = mulmod_dev(m, a[i]) ^ b[i];
}

// One wave per file: x^(8*after) as a wave-parallel product of x^(2^k)
// factors (6 shuffle-multiply levels instead of ~40 serial multiplies).
__global__ __launch_bounds__(256) void digest_kernel(const uint32_t* __restrict__ crcs,
                                                     const uint64_t* __restrict__ after,
                                                     const uint32_t* __restrict__ group, uint64_t n,
                                                     uint32_t* __restrict__ digest) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * 4) {
        const uint32_t c = crcs[i];
        const uint64_t nb = after[i];
        const uint32_t m = xpow_wave(nb << 3, lane);
        if (lane == 0) atomicXor(digest + group[i], mulmod_dev(m, c));
    }
}

// out[i] = XOR over r of gathered[r*n + i]: the local fold after the RCCL
// all-gather of per-copyset digest partials (XOR is not an RCCL op).
__global__ void xor_fold_kernel(const uint32_t* __restrict__ gathered, uint32_t nranks, uint64_t n,
                                uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t v = 0;
    for (uint32_t r = 0; r < nranks; r++) v ^= gathered[(uint64_t)r * n + i];
    out[i] = v;
}

// ---------------------------------------------------------------------------
// Scrub (cc_scrub_dev): the bulk integrity pass over a pool as the datastore
// sees it.  The domain is [0, n_pages) -- the live pages -- and, with a cc_cow,
// [n_pages, 2 n_pages) -- the snapshot copies of the same pool pages -- cut
// into groups of 64 consecutive indices.  An index is PRESENT when its page
// exists: a live page unless its chunk is a clone chunk whose bit is clear, a
// snapshot page when its chunk names a slot whose bit is set.  Only present
// pages move bytes; the groups sit on verify-on-read's schedule in the place
// of reads (tile counts published by the waves, equal shares of present pages,
// the last 1/16 dynamic).
// ---------------------------------------------------------------------------
// Set bits of a slot's bitmap in [q0, q1), q1 <= pages_per_chunk (so the unused
// bits of the last word are never looked at).
__device__ __forceinline__ uint32_t scrub_bits(const uint32_t* bm, uint32_t q0, uint32_t q1) {
    uint32_t n = 0;
    for (uint32_t wi = q0 >> 5; wi <= (q1 - 1u) >> 5; wi++) {
        const uint32_t lo = q0 > wi * 32u ? q0 - wi * 32u : 0u;
        const uint32_t hi = q1 < wi * 32u + 32u ? q1 - wi * 32u : 32u;
        const uint32_t m = (hi == 32u ? 0xFFFFFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
        n += (uint32_t)__popc(bm[wi] & m);
    }
    return n;
}
struct ScrubCount {
    uint64_t live, snap, unwritten;  // present live pages, present snapshot pages, never-written pages
};
// The counts of the pool pages [p0, p1) of one half (per lane; chunk by chunk, a bitmap word at a time)
__device__ __forceinline__ void scrub_count_half(const ScrubLaunch& a, bool snap, uint32_t p0, uint64_t p1, ScrubCount& r) {
    uint64_t p = p0;
    while (p < p1) {
        const uint32_t c = (uint32_t)p / a.pages_per_chunk;
        const uint32_t q0 = (uint32_t)p - c * a.pages_per_chunk;
        const uint64_t left = p1 - p;
        const uint32_t q1 = left < a.pages_per_chunk - q0 ? q0 + (uint32_t)left : a.pages_per_chunk;
        const uint32_t seg = q1 - q0;
        if (snap) {
            const uint32_t s = a.snap_slot[c];
            if (s < a.snap_n_slots) r.snap += scrub_bits(a.snap_bitmap + (uint64_t)s * a.words_per_slot, q0, q1);
        } else {
            const uint32_t cs = a.clone_slot ? a.clone_slot[c] : 0xFFFFFFFFu;
            if (cs < a.clone_n_slots) {
                const uint32_t w = scrub_bits(a.clone_bitmap + (uint64_t)cs * a.words_per_slot, q0, q1);
                r.live += w;
                r.unwritten += seg - w;
            } else {
                r.live += seg;
            }
        }
        p += seg;
    }
}
// The counts of group g (indices [64 g, 64 g + 64) of the domain), per lane
__device__ __forceinline__ ScrubCount scrub_group_count(const ScrubLaunch& a, uint64_t g) {
    ScrubCount r = {0, 0, 0};
    const uint64_t lo = g * 64, hi = lo + 64 < a.n_index ? lo + 64 : a.n_index;
    if (lo < a.n_pages) scrub_count_half(a, false, (uint32_t)lo, hi < a.n_pages ? hi : a.n_pages, r);
    if (hi > a.n_pages) scrub_count_half(a, true, (uint32_t)(lo > a.n_pages ? lo - a.n_pages : 0u), hi - a.n_pages, r);
    return r;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// Tile t is the groups [G t / T, G (t+1) / T); its present pages, uniform.  `all`
// also gets the tile's three counts (the counting pass of the tile's own wave).
__device__ __forceinline__ uint64_t scrub_tile_count(const ScrubLaunch& a, uint32_t t, uint32_t lane, ScrubCount* all) {
    const uint64_t lo = a.n_groups * t / kReadTiles, hi = a.n_groups * (t + 1) / kReadTiles;
    ScrubCount s = {0, 0, 0};
    for (uint64_t g = lo + lane; g < hi; g += 64) {
        const ScrubCount r = scrub_group_count(a, g);
        s.live += r.live;
        s.snap += r.snap;
        s.unwritten += r.unwritten;
    }
    const uint64_t present = wave_sum64(s.live + s.snap);
    if (all) {
        all->live += wave_sum64(s.live);
        all->snap += wave_sum64(s.snap);
        all->unwritten += wave_sum64(s.unwritten);
    }
    return present;
}

// One present page on its way through the hash: everything uniform.
struct ScrubPg {
    uint64_t src;   // its bytes
    uint64_t idx;   // its index in the domain
    uint32_t want;  // the stored CRC
};

// The slot schedule with groups in the place of entries.  A wave's
// share is [lo, hi) of the present pages in domain order: the tile search in
// registers, then the tile's groups 64 at a time (a lane counts one group from
// the bitmap words) to the group holding page lo.  From there one lane
// resolves one index -- slot word, bitmap word, source address -- and loads
// its stored CRC (present lanes only: nothing of an absent page is read); the
// ballot of the present lanes is the group's page list, walked with scalar
// math across group boundaries so three register sets keep rotating for the
// whole share.  The three counts a scrub owes for pages it never hashes leave
// with the tile counts: each tile's own wave counts it once and adds the
// tile's counts with one atomic each.  With gridDim.x * kRvWaves >= kReadTiles
// (one workgroup a CU on 64 CUs or more: the MI355X has 256) a wave counts at
// most one tile, so that is one atomic a count a wave; a smaller grid pays up
// to three atomics for every further tile of a wave, with the same sums.  A
// mismatch costs its atomics on the spot.
template <int M>
__global__ __launch_bounds__(64 * kRvWaves) void scrub_kernel(ScrubLaunch a) {
    __shared__ uint32_t tab[kLdsBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t G = a.n_groups;
    RvShares sh;
    if (!rv_begin(sh, tab, a.tiles, a.tail, a.epoch, a.image, lane, [&](uint32_t t, bool mark) {
            ScrubCount mine = {0, 0, 0};  // the tile's three counts, owed by the tile's own wave alone
            const uint64_t present = scrub_tile_count(a, t, lane, mark ? &mine : nullptr);
            if (mark && lane == 0) {
                if (mine.live) atomicAdd(a.counts + 0, (unsigned long long)mine.live);
                if (mine.snap) atomicAdd(a.counts + 2, (unsigned long long)mine.snap);
                if (mine.unwritten) atomicAdd(a.counts + 4, (unsigned long long)mine.unwritten);
            }
            return present;
        }))
        return;
    const uint32_t c0 = lane << 2 & 0x7Cu;
    const uint32_t c1 = c0 | 0x10000u;
    const uint32_t cf = kFinBase + (lane << 2);
    uint32_t live_bad = 0, snap_bad = 0;
    // a mismatch (rare; lane 0): the list cursor, the chunk's word
    auto report = [&](const ScrubPg& p) {
        const bool snap = p.idx >= a.n_pages;
        const uint64_t pg = snap ? p.idx - a.n_pages : p.idx;
        if (lane == 0) {
            const unsigned long long at = atomicAdd(a.counts + 5, 1ull);
            if (at < a.max_list) a.list[at] = snap ? (pg | (1ull << 63)) : pg;
            if (a.per_chunk) atomicAdd(a.per_chunk + 2 * (pg / a.pages_per_chunk) + (snap ? 1u : 0u), 1u);
        }
        if (snap)
            snap_bad++;
        else
            live_bad++;
    };
#pragma unroll 1
    do {
        const uint64_t lo_slot = sh.lo_slot, hi_slot = sh.hi_slot;
        if (lo_slot < hi_slot) {
            // the group holding present page lo_slot, and the present pages before it
            const TileHit th = tile_of(sh.cum, sh.tb, lo_slot, lane);
            uint64_t g = G * th.tile / kReadTiles, S = th.before;
            for (;;) {
                const uint64_t gi = g + lane;
                uint64_t cnt = 0;
                if (gi < G) {
                    const ScrubCount r = scrub_group_count(a, gi);
                    cnt = r.live + r.snap;
                }
                const uint64_t c = wave_scan_incl(cnt, lane);
                const uint64_t hit = __ballot(S + c > lo_slot);
                if (hit) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(hit);
                    S += l ? readlane64(c, l - 1) : 0;
                    g += l;
                    break;
                }
                S += readlane64(c, 63);
                g += 64;
                if (g >= G) break;  // the counts moved under the call (a caller error): nothing to walk
            }
            uint32_t skip = (uint32_t)(lo_slot - S);  // present pages of group g before the share (< 64)
            uint64_t ke = hi_slot - lo_slot;          // pages to hash
            // the page cursor: group gcur resolved a lane an index, `mask` its present lanes not yet taken
            uint64_t gcur = g - 1, mask = 0;
            uint64_t vsrc = 0;
            uint32_t vwant = 0;
            uint64_t fetched = 0;
            ScrubPg last = {0, 0, 0};
            // the next present page into p; none left: p = the last one (the same loads every step)
            auto fetch = [&](ScrubPg& p) {
                if (fetched < ke) {
                    while (!mask) {
                        if (++gcur >= G) break;
                        const uint64_t idx = gcur * 64 + lane;
                        bool present = false;
                        if (idx < a.n_index) {
                            const bool snap = idx >= a.n_pages;
                            const uint32_t pg = (uint32_t)(snap ? idx - a.n_pages : idx);
                            const uint32_t c = a.pages_per_chunk == 1
                                                   ? pg
                                                   : (uint32_t)(((uint64_t)pg * a.ppc_mhi + ((uint64_t)pg * a.ppc_mlo >> 32)) >> 32);
                            const uint32_t q = pg - c * a.pages_per_chunk;
                            if (snap) {
                                const uint32_t s = a.snap_slot[c];
                                if (s < a.snap_n_slots &&
                                    ((a.snap_bitmap[(uint64_t)s * a.words_per_slot + (q >> 5)] >> (q & 31u)) & 1u)) {
                                    const uint64_t sp = (uint64_t)s * a.pages_per_chunk + q;
                                    present = true;
                                    vsrc = (uint64_t)(uintptr_t)a.snap + (sp << a.page_shift);
                                    vwant = a.snap_crcs[sp];
                                }
                            } else {
                                const uint32_t cs = a.clone_slot ? a.clone_slot[c] : 0xFFFFFFFFu;
                                if (cs >= a.clone_n_slots ||
                                    ((a.clone_bitmap[(uint64_t)cs * a.words_per_slot + (q >> 5)] >> (q & 31u)) & 1u)) {
                                    present = true;
                                    vsrc = (uint64_t)(uintptr_t)a.pool + ((uint64_t)pg << a.page_shift);
                                    vwant = a.page_crcs[pg];
                                }
                            }
                        }
                        mask = __ballot(present);
                        for (; skip && mask; skip--) mask &= mask - 1;
                    }
                    if (mask) {
                        const uint32_t j = (uint32_t)__builtin_ctzll(mask);
                        mask &= mask - 1;
                        last.src = readlane64(vsrc, j);
                        last.want = (uint32_t)__builtin_amdgcn_readlane(vwant, j);
                        last.idx = gcur * 64 + j;
                        fetched++;
                    } else {
                        ke = fetched;  // ran off the domain (see above)
                    }
                }
                p = last;
            };
            ScrubPg pA, pB, pC;
            fetch(pA);
            if (ke) {
                fetch(pB);
                pC = pB;
                uint32_t A[M], B[M], Cq[M];
                load_page<M>(A, reinterpret_cast<const uint32_t*>(pA.src) + lane);
                load_page<M>(B, reinterpret_cast<const uint32_t*>(pB.src) + lane);
                // hash X (page k of the share); page k+2's loads go into Y
                auto step = [&](uint32_t (&X)[M], const ScrubPg& px, uint64_t k, uint32_t (&Y)[M], ScrubPg& py) {
                    fetch(py);
                    load_page<M>(Y, reinterpret_cast<const uint32_t*>(py.src) + lane);
                    const uint32_t crc = wave_xor(apply_fin(tab, chain<M>(tab, X, c0, c1), cf)) ^ a.kconst;
                    if (crc != px.want) report(px);
                    return k + 1 < ke;
                };
                for (uint64_t k = 0;; k += 3) {
                    if (!step(A, pA, k, Cq, pC)) break;
                    if (!step(B, pB, k + 1, A, pA)) break;
                    if (!step(Cq, pC, k + 2, B, pB)) break;
                }
            }
        }
    } while (rv_next(sh, lane));
    if (lane == 0) {
        if (live_bad) atomicAdd(a.counts + 1, (unsigned long long)live_bad);
        if (snap_bad) atomicAdd(a.counts + 3, (unsigned long long)snap_bad);
    }
}

// cc_scrub_dev with neither struct is the page kernel in verify mode, its
// cursor the scrub's `listed`; these two one-thread kernels around it turn the
// cursor's advance into live_bad (pre: live_bad -= listed, post: += listed,
// mod 2^64) and count the pages, all of them checked.
__global__ void scrub_plain_kernel(unsigned long long* counts, unsigned long long n_pages, int post) {
    if (post) {
        counts[1] += counts[5];
        counts[0] += n_pages;
    } else {
        counts[1] -= counts[5];
    }
}

// Fused metapages only ride a dynamic tail (the static walk knows one array).
TailExtra tail_extra(const PageLaunch& a) {
    const bool meta = a.dyn_ctr && a.meta_pages && a.n_meta;
    return {meta ? a.meta_pages : nullptr, meta ? a.n_meta : 0, meta ? a.meta_out : nullptr,
            a.dyn_ctr ? a.dyn_next : nullptr};
}

// The kernels are instantiated for M = page_bytes / 256 in 1, 2, 4, ..., 32:
// launch(std::integral_constant<int, M>) for the one that matches, and the
// launch's error; hipErrorInvalidValue for any other page size.
template <typename Launch>
hipError_t for_page_words(uint32_t m, Launch launch) {
    switch (m) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        case 8: launch(std::integral_constant<int, 8>()); break;
        case 16: launch(std::integral_constant<int, 16>()); break;
        case 32: launch(std::integral_constant<int, 32>()); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_page(const PageLaunch& a, hipStream_t s) {
    const dim3 grid(a.blocks), block(kBlockThreads);
    const uint4* img = static_cast<const uint4*>(a.image);
    const ZeroRanges zr = {{a.zero[0], a.zero[1]}, {a.zero[0] ? a.zero_words[0] : 0, a.zero[1] ? a.zero_words[1] : 0}};
    const TailExtra ex = tail_extra(a);
    const uint32_t m = a.words_per_lane;
    if (m == 0 || m > 32 || (m & (m - 1))) {  // no instantiation for this page size: the any-size kernel
        hipExtLaunchKernelGGL((page_crc_kernel_dyn<MODE>), grid, block, 0, s, a.ev_begin, a.ev_end, 0u, a.pages,
                              a.n_pages, m, img, a.kconst, a.out, a.expected, a.sink, zr);
        return hipGetLastError();
    }
    return for_page_words(m, [&](auto mm) {
        hipExtLaunchKernelGGL((page_crc_kernel<decltype(mm)::value, MODE>), grid, block, 0, s, a.ev_begin, a.ev_end, 0u,
                              a.pages, a.n_pages, img, a.kconst, a.out, a.expected, a.sink, a.tile_shift, a.dyn_ctr,
                              a.static_tiles, zr, ex);
    });
}

}  // namespace

hipError_t launch_page_crc(const PageLaunch& a, hipStream_t s) { return launch_page<0>(a, s); }

// The scan step's metapage pass: the compute kernel as its own instantiation
// (MODE 3 = MODE 0), so a kernel trace reports the 1,024-page metapage launches
// apart from the 16 GiB data launches instead of averaging the two.
hipError_t launch_page_meta(const PageLaunch& a, hipStream_t s) {
    if (a.words_per_lane != 16) return launch_page<0>(a, s);
    const ZeroRanges zr = {{a.zero[0], a.zero[1]}, {a.zero[0] ? a.zero_words[0] : 0, a.zero[1] ? a.zero_words[1] : 0}};
    hipLaunchKernelGGL((page_crc_kernel<16, 3>), dim3(a.blocks), dim3(kBlockThreads), 0, s, a.pages, a.n_pages,
                       static_cast<const uint4*>(a.image), a.kconst, a.out, a.expected, a.sink, a.tile_shift,
                       a.dyn_ctr, a.static_tiles, zr, tail_extra(a));
    return hipGetLastError();
}

hipError_t launch_page_load_probe(const PageLaunch& a, hipStream_t s) {
    if (a.words_per_lane != 16) return hipErrorInvalidValue;  // 4 KiB pages only
    const ZeroRanges zr = {{nullptr, nullptr}, {0, 0}};
    hipLaunchKernelGGL((page_crc_kernel<16, 2>), dim3(a.blocks), dim3(kBlockThreads), 0, s, a.pages, a.n_pages,
                       static_cast<const uint4*>(a.image), a.kconst, a.out, a.expected, a.sink, a.tile_shift,
                       a.dyn_ctr, a.static_tiles, zr, tail_extra(a));
    return hipGetLastError();
}

// Read-only probe (diagnostic): dwordx4 nt loads, 4 in flight per lane, the
// fastest pure-read shape found by scripts/hbm_probe.hip.  Static strided
// schedule: it waits for the slowest XCD as the page kernel did before its
// dynamic tail (a dynamic-tail version of this probe measured slower, 6.7 TB/s).
__global__ __launch_bounds__(1024) void read_probe_kernel(const uint4* __restrict__ p, uint64_t n16,
                                                          uint32_t* __restrict__ sink) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint64_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 6);
    const uint64_t waves = (uint64_t)gridDim.x * 16;
    constexpr uint64_t kStep = 64 * 4;  // 16-byte elements per wave per step
    uint32_t acc = 0;
    const u32x4* q = reinterpret_cast<const u32x4*>(p);
    for (uint64_t b = wave * kStep; b + kStep <= n16; b += waves * kStep) {
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = __builtin_nontemporal_load(q + b + u * 64 + lane);
#pragma unroll
        for (int u = 0; u < 4; u++) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    acc ^= __shfl_xor(acc, 32);
    if (lane == 0) sink[wave] = acc;
}

hipError_t launch_read_probe(const void* buf, uint64_t bytes, uint32_t* sink, int blocks, hipStream_t s) {
    hipLaunchKernelGGL(read_probe_kernel, dim3(blocks), dim3(1024), 0, s, static_cast<const uint4*>(buf), bytes / 16,
                       sink);
    return hipGetLastError();
}
hipError_t launch_page_verify(const PageLaunch& a, hipStream_t s) { return launch_page<1>(a, s); }

hipError_t launch_fold(const FoldLaunch& a, hipStream_t s) {
    if (a.n_groups == 0) return hipSuccess;
    if (a.per_group >= 64 && a.per_group % 64 == 0) {
        uint64_t blocks = (a.n_groups + 3) / 4;
        if (blocks > 2048) blocks = 2048;  // grid-stride: the LDS product table is built once per block
        hipLaunchKernelGGL(fold_kernel_wave, dim3((uint32_t)blocks), dim3(256), 0, s, a.crcs, a.n_groups,
                           a.per_group, a, a.out);
    } else {
        const uint64_t blocks = (a.n_groups + 255) / 256;
        hipLaunchKernelGGL(fold_kernel_serial, dim3((uint32_t)blocks), dim3(256), 0, s, a.crcs, a.n_groups,
                           a.per_group, a.m_unit, a.out);
    }
    return hipGetLastError();
}



hipError_t launch_range_flat(const RangeLaunch& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(range_flat_kernel, dim3(a.blocks), dim3(64 * kFlatWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t upload_x2k(const uint32_t* t64) { return hipMemcpyToSymbol(HIP_SYMBOL(c_x2k), t64, sizeof(X2k)); }

hipError_t launch_shift(const uint32_t* crcs, const uint64_t* shift_bytes, uint64_t n, uint32_t* out,
                        hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(shift_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, crcs, shift_bytes, n, out);
    return hipGetLastError();
}

hipError_t launch_log_insert(const LogLaunch& a, hipStream_t s) {
    if (a.n_pieces == 0) return hipSuccess;
    if (a.n_segs == 0 || a.n_segs > kInsertBlocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(log_insert_kernel, dim3(a.n_segs), dim3(kInsertThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_log_pages(const LogLaunch& a, hipStream_t s) {
    if (a.n_pieces == 0) return hipSuccess;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        constexpr int MM = decltype(m)::value;
        if (a.delta)
            hipLaunchKernelGGL((log_pages_kernel<MM, true>), dim3(a.blocks), dim3(64 * log_waves(MM, true)), 0, s, a);
        else
            hipLaunchKernelGGL((log_pages_kernel<MM, false>), dim3(a.blocks), dim3(64 * log_waves(MM, false)), 0, s, a);
    });
}

hipError_t launch_log_cow(const LogCowLaunch& a, hipStream_t s) {
    if (a.n_segs == 0 || a.n_segs > kInsertBlocks || a.blocks <= 0) return hipErrorInvalidValue;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        constexpr int MM = decltype(m)::value;
        if (a.stale)
            hipLaunchKernelGGL((log_cow_kernel<MM, true>), dim3(a.blocks), dim3(64 * kCowWaves), 0, s, a);
        else
            hipLaunchKernelGGL((log_cow_kernel<MM, false>), dim3(a.blocks), dim3(64 * kCowWaves), 0, s, a);
    });
}

hipError_t launch_log_small(const LogLaunch& a, hipStream_t s) {
    if (a.n_updates == 0 || a.n_updates > 64 || a.slots > 2) return hipErrorInvalidValue;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        constexpr int MM = decltype(m)::value;
        if (a.delta)
            hipLaunchKernelGGL((log_small_kernel<MM, true>), dim3(a.blocks), dim3(64 * log_small_waves(MM, true)), 0, s,
                               a);
        else
            hipLaunchKernelGGL((log_small_kernel<MM, false>), dim3(a.blocks), dim3(64 * log_small_waves(MM, false)), 0,
                               s, a);
    });
}


hipError_t launch_page_list_probe(const PageListProbeLaunch& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(page_list_probe_kernel<16>, dim3(a.blocks), dim3(64 * kListProbeWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_log_probe(const LogProbeLaunch& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(log_probe_kernel<16>, dim3(a.blocks), dim3(64 * kLogWavesFull), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_read_verify_small(const ReadVerifyLaunch& a, hipStream_t s) {
    if (a.n_reads == 0 || a.n_reads > 64) return hipErrorInvalidValue;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        hipLaunchKernelGGL((read_verify_small_kernel<decltype(m)::value>), dim3(a.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_read_verify(const ReadVerifyLaunch& a, hipStream_t s) {
    if (a.n_reads == 0) return hipSuccess;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        hipLaunchKernelGGL((read_verify_kernel<decltype(m)::value>), dim3(a.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_snap_read_small(const SnapReadLaunch& a, hipStream_t s) {
    if (a.rv.n_reads == 0 || a.rv.n_reads > 64) return hipErrorInvalidValue;
    return for_page_words(a.rv.page_bytes / kWaveBytes, [&](auto m) {
        constexpr int MM = decltype(m)::value;
        if (a.out)
            hipLaunchKernelGGL((snap_read_small_kernel<MM, true>), dim3(a.rv.blocks), dim3(64 * kRvWaves), 0, s, a);
        else
            hipLaunchKernelGGL((snap_read_small_kernel<MM, false>), dim3(a.rv.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_snap_read(const SnapReadLaunch& a, hipStream_t s) {
    if (a.rv.n_reads == 0) return hipSuccess;
    return for_page_words(a.rv.page_bytes / kWaveBytes, [&](auto m) {
        constexpr int MM = decltype(m)::value;
        if (a.out)
            hipLaunchKernelGGL((snap_read_kernel<MM, true>), dim3(a.rv.blocks), dim3(64 * kRvWaves), 0, s, a);
        else
            hipLaunchKernelGGL((snap_read_kernel<MM, false>), dim3(a.rv.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

// a wave per 64 entries, up to 8 workgroups a CU
static dim3 clone_grid(uint64_t n, int cus) {
    const uint64_t want = (n + 64ull * kCloneWaves - 1) / (64ull * kCloneWaves), cap = 8ull * (uint64_t)(cus > 0 ? cus : 1);
    return dim3((unsigned)(want < cap ? (want ? want : 1) : cap));
}

hipError_t launch_paste_claim(const PasteLaunch& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(paste_claim_kernel, clone_grid(a.n, a.blocks), dim3(64 * kCloneWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_paste(const PasteLaunch& a, hipStream_t s) {
    if (a.n == 0 || a.geo.n_slots == 0) return hipSuccess;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        hipLaunchKernelGGL((paste_kernel<decltype(m)::value>), dim3(a.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_clone_mark(const CloneMarkLaunch& a, hipStream_t s) {
    if (a.n == 0 || a.geo.n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(clone_mark_kernel, clone_grid(a.n, a.blocks), dim3(64 * kCloneWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_logs_prepass(const LogsPrepassLaunch& a, hipStream_t s) {
    if (a.n_batches == 0 || a.n_batches > (uint32_t)kPrepassBatches || a.n_pairs == 0 || a.slots == 0 || a.blocks <= 0)
        return hipErrorInvalidValue;
    if (a.page_bytes != 1u << a.page_shift || (a.snap_slot && a.pages_per_chunk == 0) ||
        (a.clone.clone_slot && a.clone.pages_per_chunk == 0))
        return hipErrorInvalidValue;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        constexpr int MM = decltype(m)::value;
        if (a.stale)
            hipLaunchKernelGGL((logs_prepass_kernel<MM, true>), dim3(a.blocks), dim3(64 * kPrepassWaves), 0, s, a);
        else
            hipLaunchKernelGGL((logs_prepass_kernel<MM, false>), dim3(a.blocks), dim3(64 * kPrepassWaves), 0, s, a);
    });
}

static bool ops_launch_ok(const OpsLaunch& a) {
    if (a.n_batches == 0 || a.n_batches > (uint32_t)kOpsBatches || a.n_pairs == 0 || a.blocks <= 0) return false;
    if (a.page_bytes != 1u << a.page_shift || a.page_shift < 8 || a.geo.pages_per_chunk == 0 || !a.geo.clone_slot) return false;
    for (uint32_t h = 0; h < a.n_batches; h++)
        if ((a.b[h].kind == kOpPaste ? a.paste_slots : a.slots) == 0) return false;
    return true;
}

hipError_t launch_ops_bid(const OpsLaunch& a, hipStream_t s) {
    if (!ops_launch_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ops_bid_kernel, dim3(a.blocks), dim3(64 * kOpsWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ops_resolve(const OpsLaunch& a, hipStream_t s) {
    if (!ops_launch_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ops_resolve_kernel, dim3(a.blocks), dim3(64 * kOpsWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ops_paste(const OpsLaunch& a, hipStream_t s) {
    if (!ops_launch_ok(a)) return hipErrorInvalidValue;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        hipLaunchKernelGGL((ops_paste_kernel<decltype(m)::value>), dim3(a.blocks), dim3(64 * kOpsWaves), 0, s, a);
    });
}

hipError_t launch_clone_check(const CloneCheckLaunch& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(clone_check_kernel, clone_grid(a.n, a.blocks), dim3(64 * kCloneWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_merge_read_small(const MergeReadLaunch& a, hipStream_t s) {
    if (a.rv.n_reads == 0 || a.rv.n_reads > 64) return hipErrorInvalidValue;
    return for_page_words(a.rv.page_bytes / kWaveBytes, [&](auto m) {
        hipLaunchKernelGGL((merge_read_small_kernel<decltype(m)::value>), dim3(a.rv.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_merge_read(const MergeReadLaunch& a, hipStream_t s) {
    if (a.rv.n_reads == 0) return hipSuccess;
    return for_page_words(a.rv.page_bytes / kWaveBytes, [&](auto m) {
        hipLaunchKernelGGL((merge_read_kernel<decltype(m)::value>), dim3(a.rv.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_repair_claim(const RepairLaunch& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(repair_claim_kernel, clone_grid(a.n, a.blocks), dim3(64 * kCloneWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_repair(const RepairLaunch& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    return for_page_words(a.page_bytes / kWaveBytes, [&](auto m) {
        hipLaunchKernelGGL((repair_kernel<decltype(m)::value>), dim3(a.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_scrub(const ScrubLaunch& a, hipStream_t s) {
    if (a.n_index == 0) return hipSuccess;
    return for_page_words(a.words_per_lane, [&](auto m) {
        hipLaunchKernelGGL((scrub_kernel<decltype(m)::value>), dim3(a.blocks), dim3(64 * kRvWaves), 0, s, a);
    });
}

hipError_t launch_scrub_plain(unsigned long long* counts, uint64_t n_pages, int post, hipStream_t s) {
    hipLaunchKernelGGL(scrub_plain_kernel, dim3(1), dim3(1), 0, s, counts, (unsigned long long)n_pages, post);
    return hipGetLastError();
}

hipError_t launch_epilogue(const EpilogueLaunch& a, hipStream_t s) {
    if (a.n_chunks == 0) return hipSuccess;
    const uint64_t blocks = a.n_chunks < 8192 ? a.n_chunks : 8192;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_xpow8(const uint64_t* nbytes, uint64_t n, uint32_t* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(xpow8_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, nbytes, n, out);
    return hipGetLastError();
}

hipError_t launch_combine(const uint32_t* a, const uint32_t* b, uint32_t m_len_b, uint64_t n, uint32_t* out,
                          hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(combine_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a, b, m_len_b, n, out);
    return hipGetLastError();
}

hipError_t launch_xor_fold(const uint32_t* gathered, uint32_t nranks, uint64_t n, uint32_t* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(xor_fold_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, gathered, nranks, n, out);
    return hipGetLastError();
}

hipError_t launch_digest(const uint32_t* crcs, const uint64_t* after_bytes, const uint32_t* group, uint64_t n,
                         uint32_t* digest, hipStream_t s) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(digest_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, crcs, after_bytes, group, n, digest);
    return hipGetLastError();
}

}  // namespace cc
