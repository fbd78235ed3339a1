// The grouping of evk_denoise_group ("all events of one pixel -- and polarity class --, in stream order"): its limits, the layout
// of its scratch, the opening check of every entry point on it (dn_open) and the decode of a key (dn_pixel).  Shared by the passes
// that read order[] and the run table start[]: evk_denoise.hip (which builds it), evk_tsurf.hip, evk_corner.hip,
// evk_planeflow.hip (the last three through evk_pred.h as well) and evk_reconstruct.hip.
#pragma once
#include "evk_common.h"

namespace evk {

constexpr int64_t DN_MAX_N = 0x7FFFFFFF;              // hipcub's item count is an int; indices and positions are uint32
constexpr int64_t DN_MAX_KEYS = 0x7FFFFFFE;           // K + 1 run-table entries, 32-bit keys

static inline int64_t dn_al(int64_t b) { return (b + 255) & ~(int64_t)255; }

// the keys are sorted from bit 0 over at least 8 bits (evk_augment.hip: hipcub's onesweep path and narrow bit ranges)
static inline int dn_key_bits(int64_t nkeys) {
    int bits = 8;
    while (bits < 32 && ((int64_t)1 << bits) < nkeys) ++bits;
    return bits;
}

// hipcub's storage for the sort of n (key, index) pairs over `bits` key bits (evk_denoise.hip, the one file that includes hipcub)
size_t dn_sort_temp_bytes(int64_t n, int bits);

// scratch: [256 header][keys n][order n][start K+1] -- what the support and refractory passes read -- then the sort's other
// halves [sorted keys n][iota n] and hipcub's own storage
struct DnScratch {
    uint32_t *keys, *order, *start, *sorted, *iota;
    void *temp;
    int64_t temp_bytes, total;
};

static DnScratch dn_layout(void *scratch, int64_t n, int64_t nkeys) {
    char *sb = static_cast<char *>(scratch);
    DnScratch L;
    int64_t off = 256;
    L.keys = reinterpret_cast<uint32_t *>(sb + off), off += dn_al(4 * n);
    L.order = reinterpret_cast<uint32_t *>(sb + off), off += dn_al(4 * n);
    L.start = reinterpret_cast<uint32_t *>(sb + off), off += dn_al(4 * (nkeys + 1));
    L.sorted = reinterpret_cast<uint32_t *>(sb + off), off += dn_al(4 * n);
    L.iota = reinterpret_cast<uint32_t *>(sb + off), off += dn_al(4 * n);
    L.temp = sb + off;
    L.temp_bytes = n > 0 ? (int64_t)dn_sort_temp_bytes(n, dn_key_bits(nkeys)) : 0;
    L.total = off + dn_al(L.temp_bytes);
    return L;
}

static bool dn_shape_ok(int64_t n, int h, int w, int classes) {
    return n >= 0 && n <= DN_MAX_N && h > 0 && w > 0 && (classes == 1 || classes == 2) &&
           (int64_t)classes * h * w <= DN_MAX_KEYS;
}

// How every entry point on a grouping opens: the shape and the scratch pointer (EVK_EINVAL), its alignment (EVK_EALIGN), then
// the layout.  An entry point states its own EINVAL checks BEFORE the call, so that they win over EALIGN as they always have.
static int dn_open(const void *scratch, int64_t n, int h, int w, int classes, DnScratch *L) {
    if (!dn_shape_ok(n, h, w, classes) || !scratch) return EVK_EINVAL;
    if ((uintptr_t)scratch & 255u) return EVK_EALIGN;
    *L = dn_layout(const_cast<void *>(scratch), n, (int64_t)classes * h * w);
    return EVK_OK;
}

// a key of the grouping -> the base of its class (0 or hw) and its pixel
struct DnPixel {
    uint32_t cbase;
    int x, y;
};
__device__ __forceinline__ DnPixel dn_pixel(uint32_t key, uint32_t hw, uint32_t w) {
    DnPixel p;
    p.cbase = key >= hw ? hw : 0u;
    const uint32_t pix = key - p.cbase;
    p.y = (int)(pix / w), p.x = (int)(pix - (uint32_t)p.y * w);
    return p;
}

}  // namespace evk
