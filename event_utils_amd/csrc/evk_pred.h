// "The last event before event i at pixel q" on the grouping of evk_group.h: the predecessor search in a run of order[] (one at
// a time, or several side by side in one lane) and the argument check of the per-event passes that take a selection.  Shared by
// evk_tsurf.hip, evk_corner.hip and evk_planeflow.hip; evk_reconstruct.hip takes ts_pred and ts_kind_ok.  (The conversion of a
// time column to double, ts_time, is in evk_common.h.)
#pragma once
#include "evk_common.h"
#include "evk_group.h"

namespace evk {

constexpr uint32_t TS_NONE = 0xFFFFFFFFu;             // no key / no predecessor (keys stay below 2^31 - 1)

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

// WAYS predecessor searches of one lane, run side by side.  In pixel order a pass is bound by the latency of the dependent
// probes of a binary search, and a lane that keeps the probes of several runs in flight hides most of it.  With a selection
// the lanes of a wave search unrelated runs, the pass is bound by the cache lines it moves and more probes in flight
// measured no faster (profiles/corner_time.txt).
// q[u]: the key to search, TS_NONE for no search.  -> pos[u]: the position of the predecessor of i in order[], TS_NONE when
// there is none.  A finished or switched-off search probes order[0] (n >= 1) and ignores it, so the loads need no branch.
template <int WAYS>
__device__ __forceinline__ void ts_search(const uint32_t *__restrict__ order, const uint32_t *__restrict__ start,
                                          const uint32_t (&q)[WAYS], uint32_t i, uint32_t (&pos)[WAYS]) {
    uint32_t s[WAYS], lo[WAYS], hi[WAYS];
#pragma unroll
    for (int u = 0; u < WAYS; ++u) {
        const uint32_t k = q[u] != TS_NONE ? q[u] : 0u;
        s[u] = start[k];
        hi[u] = start[k + 1];
    }
#pragma unroll
    for (int u = 0; u < WAYS; ++u) {
        if (q[u] == TS_NONE) hi[u] = s[u];
        lo[u] = s[u];
    }
    for (;;) {
        bool more = false;
#pragma unroll
        for (int u = 0; u < WAYS; ++u) more |= lo[u] < hi[u];
        if (!more) break;
        uint32_t mid[WAYS], val[WAYS];
#pragma unroll
        for (int u = 0; u < WAYS; ++u) {
            mid[u] = (lo[u] + hi[u]) >> 1;             // (n < 2^31: no wrap)
            val[u] = order[lo[u] < hi[u] ? mid[u] : 0u];
        }
#pragma unroll
        for (int u = 0; u < WAYS; ++u) {
            if (lo[u] < hi[u]) {
                if (val[u] < i) lo[u] = mid[u] + 1;
                else hi[u] = mid[u];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < WAYS; ++u) pos[u] = lo[u] > s[u] ? lo[u] - 1 : TS_NONE;
}

static bool ts_kind_ok(int t_kind) { return t_kind >= EVK_SELECT_I16 && t_kind <= EVK_SELECT_F64; }

// what the per-event passes with a selection refuse; *items: the events the call takes (0: nothing to do).  out: the (first)
// required output, NULL when one of them is missing.  *L: the grouping in `scratch`
static int ts_rows_check(int t_kind, const void *t, int64_t n, int h, int w, int classes, const int64_t *select, int64_t rows,
                         const void *scratch, const void *out, int64_t *items, DnScratch *L) {
    if (!ts_kind_ok(t_kind) || rows < 0 || (n > 0 && !t)) return EVK_EINVAL;
    if (const int rc = dn_open(scratch, n, h, w, classes, L)) return rc;
    *items = select ? rows : n;
    if (*items > 0 && (!out || n == 0)) return EVK_EINVAL;      // (a selection from no events)
    return EVK_OK;
}

}  // namespace evk
