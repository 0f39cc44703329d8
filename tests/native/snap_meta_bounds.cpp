// Host only, built with ASan/UBSan by tests/test_log_cow.py: cc_snap_meta_encode /
// cc_snap_meta_decode on heap buffers of their exact size -- a page that the
// bitmap fills to its last byte, every truncation of a valid page, and `bits`
// fields that claim more bitmap than the buffer holds.  Any read or write past
// a buffer is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "curve_crc.h"

#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            return 1;                                              \
        }                                                          \
    } while (0)

// integrity.cpp's check job calls the engine's file scan (engine.hip, device code: not linked here)
extern "C" int cc_scan_files(const char* const*, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*,
                             cc_file_result*) {
    return CC_ENODEV;
}

namespace {
struct Heap {  // exactly n bytes, so one byte past it is poisoned
    unsigned char* p;
    size_t n;
    explicit Heap(size_t n_) : p(static_cast<unsigned char*>(malloc(n_ ? n_ : 1))), n(n_) {}
    ~Heap() { free(p); }
};
}  // namespace

int main() {
    const uint32_t pages[] = {19, 64, 512, 4096, 8192};
    for (uint32_t page : pages) {
        const uint32_t max_bits = (page - 18) * 8;
        const uint32_t bit_cases[] = {1, 7, 8, 9, max_bits - 7, max_bits};
        for (uint32_t bits : bit_cases) {
            if (bits == 0 || bits > max_bits) continue;
            const uint32_t nb = (bits + 7) / 8;
            Heap bm(nb), out(page), back(nb);
            for (uint32_t i = 0; i < nb; i++) bm.p[i] = (unsigned char)(i * 37 + bits);
            EXPECT(cc_snap_meta_encode(0xA1B2C3D4E5F60718ull, 1, bits, bm.p, out.p, page) == CC_OK);
            uint64_t sn = 0;
            int damaged = 0;
            uint32_t got = 0;
            EXPECT(cc_snap_meta_decode(out.p, page, &sn, &damaged, &got, back.p, nb) == CC_OK);
            EXPECT(sn == 0xA1B2C3D4E5F60718ull && damaged == 1 && got == bits && memcmp(bm.p, back.p, nb) == 0);
            if (nb > 1) EXPECT(cc_snap_meta_decode(out.p, page, nullptr, nullptr, nullptr, back.p, nb - 1) == CC_EINVAL);
            // one bit more than fits
            if (bits == max_bits) {
                Heap big(nb + 1);
                memset(big.p, 0xFF, nb + 1);
                EXPECT(cc_snap_meta_encode(1, 0, max_bits + 1, big.p, out.p, page) == CC_EINVAL);
            }
            // every truncation: a copy of exactly `cut` bytes
            const uint32_t need = 14 + nb + 4;
            for (uint32_t cut = 0; cut <= page; cut = (cut >= 40 && cut + 140 < need) ? cut + 97 : cut + 1) {
                Heap t(cut);
                memcpy(t.p, out.p, cut);
                const int rc = cc_snap_meta_decode(t.p, cut, &sn, &damaged, &got, back.p, nb);
                EXPECT(rc == (cut >= need ? CC_OK : CC_ECORRUPT));
                if (cut > need + 40) break;
            }
            // hostile bits fields over a full-size page
            const uint32_t hostile[] = {max_bits + 1, max_bits + 8, 0x7FFFFFFFu, 0xFFFFFFF8u, 0xFFFFFFFFu};
            for (uint32_t h : hostile) {
                Heap t(page);
                memcpy(t.p, out.p, page);
                memcpy(t.p + 10, &h, 4);
                EXPECT(cc_snap_meta_decode(t.p, page, &sn, &damaged, &got, nullptr, 0) == CC_ECORRUPT);
            }
        }
        Heap tiny(page);
        EXPECT(cc_snap_meta_encode(1, 0, 8, tiny.p, tiny.p, 18) == CC_EINVAL);  // 14 + 1 + 4 > 18
    }
    printf("snap_meta_bounds: ok\n");
    return 0;
}
