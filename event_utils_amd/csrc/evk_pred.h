// "The last event before event i at pixel q" on the grouping of evk_group.h: the exact conversion of a time column to double and
// the predecessor search in a run of order[].  Shared by evk_tsurf.hip and evk_corner.hip.
#pragma once
#include "evk_common.h"

namespace evk {

__device__ __forceinline__ double ts_time(const void *t, int kind, uint32_t i) {
    switch (kind) {
        case EVK_SELECT_I16: return (double)static_cast<const int16_t *>(t)[i];
        case EVK_SELECT_I32: return (double)static_cast<const int32_t *>(t)[i];
        case EVK_SELECT_I64: return (double)static_cast<const int64_t *>(t)[i];
        case EVK_SELECT_F32: return (double)static_cast<const float *>(t)[i];
        default: return static_cast<const double *>(t)[i];
    }
}

// the lower bound of `i` in the run [s, e) of order[] (ascending indices): the predecessor of i is order[result - 1], and there
// is none when the result is s
__device__ __forceinline__ uint32_t ts_pred(const uint32_t *__restrict__ order, uint32_t s, uint32_t e, uint32_t i) {
    uint32_t lo = s, hi = e;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;           // (n < 2^31: no wrap)
        if (order[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

static bool ts_kind_ok(int t_kind) { return t_kind >= EVK_SELECT_I16 && t_kind <= EVK_SELECT_F64; }

}  // namespace evk
