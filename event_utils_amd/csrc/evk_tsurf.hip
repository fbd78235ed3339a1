// Time surfaces (include/evk.h, "Time surfaces"): the surface of active events at a query, the per-event local time surface
// of HOTS and the cell-averaged histograms of HATS.  All three ask what the support pass of evk_denoise.hip asks -- "the last
// event before event i at pixel q" -- and keep the age instead of comparing it with dt, so they run on the same grouping
// (evk_group.h: order[], the indices grouped by key = class * H*W + pixel and ascending inside a key, and the run table start[]).
//
//   k_ts_global   one thread per output element (query, class, pixel): lower bound of the query's cut in the pixel's run, one
//                 gathered time; neighbouring lanes store neighbouring pixels
//   k_ts_local    one lane per output element (event, channel, window pixel), the events taken in pixel order so that the lanes
//                 of a wave search the runs of the same few pixels; the (2R+1)^2 * C values of an event are contiguous, so a wave
//                 stores whole patches.  With `select` the selected events are taken in the order given
//   k_ts_gather   t_run[pos] = (double)t[order[pos]]: the times in run order, so that a walk along a run is a sequential load
//   k_ts_hats     one wave per (cell, class), lane = window element: the wave goes through the cell's pixels in row-major order
//                 and each pixel's run in ascending order; per neighbour run a lane keeps two positions that only move forward
//                 (the predecessor of the event and the first time within dt) and sums the window in double into a register.
//                 No atomics: the order of every sum is fixed by the grouping
//   k_ts_sorted   counts the places where a time column steps back
//
// The time column is read through ts_time (evk_pred.h: a switch on the wave-uniform column kind) rather than through a template parameter:
// the kernels are bound by their searches, gathers and stores, and the local kernel is already instantiated per radius and
// channel count.  Every index comes from a key below K, a position below n or a checked selection: nothing leaves its array
// whatever the columns hold.
#include "evk_common.h"
#include "evk_group.h"
#include "evk_pred.h"

namespace evk {

// the value of an age under `decay`, stored as element e of `out` (float64 ages, float32 otherwise)
__device__ __forceinline__ void ts_store(void *out, int64_t e, double age, int decay, double tau) {
    if (decay == EVK_TSURF_AGE) {
        static_cast<double *>(out)[e] = age;
    } else if (decay == EVK_TSURF_EXP) {
        static_cast<float *>(out)[e] = (float)exp(-age / tau);
    } else {
        const double v = 1.0 - age / tau;
        static_cast<float *>(out)[e] = (float)(v > 0.0 ? v : 0.0);
    }
}

// the age, at time ti, of the last event with an index below `i` in the run [s, e) of order[]; +inf when there is none
__device__ __forceinline__ double ts_age(const void *t, int kind, const uint32_t *__restrict__ order, uint32_t s, uint32_t e,
                                         uint32_t i, double ti) {
    const uint32_t lo = ts_pred(order, s, e, i);
    return lo > s ? ti - ts_time(t, kind, order[lo - 1]) : (double)__builtin_inff();
}

__global__ void __launch_bounds__(EVK_BLOCK) k_ts_global(const void *__restrict__ t, int kind, const uint32_t *__restrict__ order,
                                                       const uint32_t *__restrict__ start, int64_t n, int64_t nkeys, int64_t nq,
                                                       const int64_t *__restrict__ cuts, const double *__restrict__ t_refs,
                                                       int decay, double tau, void *__restrict__ out) {
    const int64_t total = nq * nkeys;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / nkeys, key = e - k * nkeys;
        int64_t m = cuts[k];
        m = m < 0 ? 0 : (m > n ? n : m);
        double age = (double)__builtin_inff();
        if (m > 0) {
            const double tk = t_refs ? t_refs[k] : ts_time(t, kind, (uint32_t)(m - 1));
            age = ts_age(t, kind, order, start[key], start[key + 1], (uint32_t)m, tk);
        }
        ts_store(out, e, age, decay, tau);
    }
}

// C: the channels of the output.  C == 1: the run of the event's own key (every event of the pixel when the grouping has one
// class, the event's own class when it has two); C == 2 (a grouping with two classes): channel c is class c.
template <int R, int C>
__global__ void __launch_bounds__(EVK_BLOCK) k_ts_local(const void *__restrict__ t, int kind, const uint32_t *__restrict__ keys,
                                                      const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ order,
                                                      const uint32_t *__restrict__ start, int64_t n, int h, int w,
                                                      const int64_t *__restrict__ select, int64_t items, int include_self,
                                                      int decay, double tau, void *__restrict__ out) {
    constexpr int P = 2 * R + 1, PP = P * P, E = C * PP;
    const uint32_t hw = (uint32_t)h * (uint32_t)w;
    const int64_t total = items * E;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t item = e / E;
        const int el = (int)(e - item * E);
        const int c = el / PP, z = el - c * PP;
        const int dy = z / P - R, dx = z - (z / P) * P - R;
        uint32_t i, key;
        int64_t dst = item;
        bool ok = true;
        if (select) {
            const int64_t sel = select[item];
            ok = sel >= 0 && sel < n;
            i = ok ? (uint32_t)sel : 0u;
            key = ok ? keys[i] : 0u;
        } else {
            i = order[item];
            key = sorted[item];
            dst = (int64_t)i;
        }
        const DnPixel px = dn_pixel(key, hw, (uint32_t)w);
        const uint32_t own = px.cbase, cbase = C == 2 ? (uint32_t)c * hw : own;
        const int y = px.y, x = px.x;
        const int yy = y + dy, xx = x + dx;
        double age = (double)__builtin_inff();
        if (ok && yy >= 0 && yy < h && xx >= 0 && xx < w) {
            if (include_self && dx == 0 && dy == 0 && cbase == own) {
                age = 0.0;
            } else {
                const uint32_t q = cbase + (uint32_t)yy * (uint32_t)w + (uint32_t)xx;
                age = ts_age(t, kind, order, start[q], start[q + 1], i, ts_time(t, kind, i));
            }
        }
        ts_store(out, dst * E + el, age, decay, tau);
    }
}

__global__ void __launch_bounds__(EVK_BLOCK) k_ts_gather(const void *__restrict__ t, int kind, const uint32_t *__restrict__ order,
                                                       int64_t n, double *__restrict__ t_run) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x)
        t_run[p] = ts_time(t, kind, order[p]);
}

__global__ void __launch_bounds__(EVK_BLOCK) k_ts_sorted(const void *__restrict__ t, int kind, int64_t n,
                                                       uint32_t *__restrict__ unsorted) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += (int64_t)gridDim.x * blockDim.x)
        if (ts_time(t, kind, (uint32_t)(i + 1)) < ts_time(t, kind, (uint32_t)i)) count_oob(unsorted);
}

// One wave per (cell, class).  Lane l holds window elements l, l + 64, ... (SLOTS of them: two at R = 4).  For the pixel u of the
// cell and the lane's neighbour v = u + z inside the cell: the events of u in ascending order (non-decreasing times), pv = the
// events of v with a smaller index, wv = the first of them within dt; both only move forward.  Events of v with the same time
// but a larger index stay behind pv; the window test is the definition's own t_i - t_j <= dt in double.
template <int R>
__global__ void __launch_bounds__(EVK_BLOCK) k_ts_hats(const uint32_t *__restrict__ order, const uint32_t *__restrict__ start,
                                                     const double *__restrict__ t_run, int h, int w, int cell, int cells_x,
                                                     int64_t npairs, double tau, double dt, int normalise,
                                                     float *__restrict__ out, int32_t *__restrict__ counts) {
    constexpr int P = 2 * R + 1, PP = P * P, SLOTS = (PP + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int64_t pair = ((int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x) >> 6;
    if (pair >= npairs) return;                        // (the whole wave)
    const int64_t g = pair >> 1;
    const uint32_t cbase = (pair & 1) ? (uint32_t)h * (uint32_t)w : 0u;
    const int gy = (int)(g / cells_x), gx = (int)(g - (int64_t)gy * cells_x);
    const int y0 = gy * cell, x0 = gx * cell;
    const int y1 = h - y0 < cell ? h : y0 + cell, x1 = w - x0 < cell ? w : x0 + cell;
    double acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) acc[s] = 0.0;
    uint32_t cnt = 0;
    for (int y = y0; y < y1; ++y) {
        for (int x = x0; x < x1; ++x) {
            const uint32_t ku = cbase + (uint32_t)y * (uint32_t)w + (uint32_t)x;
            const uint32_t su = start[ku], eu = start[ku + 1];
            cnt += eu - su;
            if (su == eu) continue;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const int z = lane + 64 * s;
                const int yy = y + z / P - R, xx = x + (z - (z / P) * P) - R;
                if (z >= PP || yy < y0 || yy >= y1 || xx < x0 || xx >= x1) continue;
                const uint32_t kv = cbase + (uint32_t)yy * (uint32_t)w + (uint32_t)xx;
                const uint32_t ev = start[kv + 1];
                uint32_t pv = start[kv], wv = pv;
                if (pv == ev) continue;
                double sum = acc[s];
                for (uint32_t a = su; a < eu; ++a) {
                    const uint32_t i = order[a];
                    const double ti = t_run[a];
                    while (pv < ev && order[pv] < i) ++pv;
                    while (wv < pv && ti - t_run[wv] > dt) ++wv;
                    for (uint32_t b = wv; b < pv; ++b) sum += exp(-(ti - t_run[b]) / tau);
                }
                acc[s] = sum;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int z = lane + 64 * s;
        if (z < PP) out[pair * PP + z] = (float)(normalise && cnt ? acc[s] / (double)cnt : acc[s]);
    }
    if (counts && lane == 0) counts[pair] = (int32_t)cnt;
}

template <int R>
static void ts_local_launch(const void *t, int kind, const DnScratch &L, int64_t n, int h, int w, int channels,
                            const int64_t *select, int64_t items, int include_self, int decay, double tau, void *out,
                            hipStream_t s) {
    constexpr int PP = (2 * R + 1) * (2 * R + 1);
    const int g = stream_grid(items * PP * channels);
    if (channels == 2)
        k_ts_local<R, 2><<<g, EVK_BLOCK, 0, s>>>(t, kind, L.keys, L.sorted, L.order, L.start, n, h, w, select, items, include_self, decay, tau, out);
    else
        k_ts_local<R, 1><<<g, EVK_BLOCK, 0, s>>>(t, kind, L.keys, L.sorted, L.order, L.start, n, h, w, select, items, include_self, decay, tau, out);
}

static bool ts_decay_ok(int decay, double tau) { return decay >= EVK_TSURF_EXP && decay <= EVK_TSURF_AGE && tau > 0.0; }

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_tsurf_scratch_bytes(int64_t n) {
    if (n < 0 || n > DN_MAX_N) return EVK_EINVAL;
    return dn_al(8 * n);
}

extern "C" int evk_tsurf_check_sorted(int t_kind, const void *t, int64_t n, uint32_t *unsorted, void *stream) {
    if (n < 0 || n > DN_MAX_N || !ts_kind_ok(t_kind) || !unsorted || (n > 0 && !t)) return EVK_EINVAL;
    if (n < 2) return EVK_OK;
    k_ts_sorted<<<stream_grid(n - 1), EVK_BLOCK, 0, (hipStream_t)stream>>>(t, t_kind, n, unsorted);
    return launch_status();
}

extern "C" int evk_tsurf_global(int t_kind, const void *t, int64_t n, int h, int w, int classes, int64_t nq, const int64_t *cuts,
                                const double *t_refs, int decay, double tau, void *scratch, void *out, void *stream) {
    if (!ts_kind_ok(t_kind) || !ts_decay_ok(decay, tau) || nq < 0 || (n > 0 && !t) || (nq > 0 && (!cuts || !out))) return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, n, h, w, classes, &L)) return rc;
    if (nq == 0) return EVK_OK;
    const int64_t nkeys = (int64_t)classes * h * w;
    k_ts_global<<<stream_grid(nq * nkeys), EVK_BLOCK, 0, (hipStream_t)stream>>>(t, t_kind, L.order, L.start, n, nkeys, nq, cuts, t_refs,
                                                                              decay, tau, out);
    return launch_status();
}

extern "C" int evk_tsurf_local(int t_kind, const void *t, int64_t n, int h, int w, int classes, int radius, int decay, double tau,
                               int split, int include_self, const int64_t *select, int64_t m, void *scratch, void *out,
                               void *stream) {
    if (!ts_kind_ok(t_kind) || !ts_decay_ok(decay, tau) || radius < 1 || radius > EVK_TSURF_MAX_RADIUS || (split && classes != 2) ||
        m < 0 || (n > 0 && !t))
        return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, n, h, w, classes, &L)) return rc;
    const int64_t items = select ? m : n;
    if (items == 0) return EVK_OK;
    if (!out || n == 0) return EVK_EINVAL;             // (a selection from no events)
    const int channels = split ? 2 : 1;
    include_self = include_self ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    switch (radius) {
        case 1: ts_local_launch<1>(t, t_kind, L, n, h, w, channels, select, items, include_self, decay, tau, out, s); break;
        case 2: ts_local_launch<2>(t, t_kind, L, n, h, w, channels, select, items, include_self, decay, tau, out, s); break;
        case 3: ts_local_launch<3>(t, t_kind, L, n, h, w, channels, select, items, include_self, decay, tau, out, s); break;
        default: ts_local_launch<4>(t, t_kind, L, n, h, w, channels, select, items, include_self, decay, tau, out, s); break;
    }
    return launch_status();
}

extern "C" int evk_tsurf_hats(int t_kind, const void *t, int64_t n, int h, int w, int cell, int radius, double tau, double dt,
                              int normalise, void *scratch, void *t_scratch, int64_t t_scratch_bytes, float *out, int32_t *counts,
                              void *stream) {
    if (!ts_kind_ok(t_kind) || !(tau > 0.0) || !(dt >= 0.0) || cell < 1 || radius < 1 || radius > EVK_TSURF_MAX_RADIUS ||
        !t_scratch || !out || (n > 0 && !t))
        return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, n, h, w, 2, &L)) return rc;
    if ((uintptr_t)t_scratch & 255u) return EVK_EALIGN;
    if (t_scratch_bytes < dn_al(8 * n)) return EVK_ESCRATCH;
    if (cell > (h > w ? h : w)) cell = h > w ? h : w;
    const int cells_x = (w + cell - 1) / cell, cells_y = (h + cell - 1) / cell;
    const int64_t npairs = 2 * (int64_t)cells_x * cells_y;
    const int64_t blocks = (npairs + EVK_BLOCK / EVK_WAVE - 1) / (EVK_BLOCK / EVK_WAVE);
    if (blocks > 0x7FFFFFFF) return EVK_EINVAL;
    double *t_run = static_cast<double *>(t_scratch);
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) k_ts_gather<<<stream_grid(n), EVK_BLOCK, 0, s>>>(t, t_kind, L.order, n, t_run);
    const int g = (int)blocks;
    switch (radius) {
        case 1: k_ts_hats<1><<<g, EVK_BLOCK, 0, s>>>(L.order, L.start, t_run, h, w, cell, cells_x, npairs, tau, dt, normalise, out, counts); break;
        case 2: k_ts_hats<2><<<g, EVK_BLOCK, 0, s>>>(L.order, L.start, t_run, h, w, cell, cells_x, npairs, tau, dt, normalise, out, counts); break;
        case 3: k_ts_hats<3><<<g, EVK_BLOCK, 0, s>>>(L.order, L.start, t_run, h, w, cell, cells_x, npairs, tau, dt, normalise, out, counts); break;
        default: k_ts_hats<4><<<g, EVK_BLOCK, 0, s>>>(L.order, L.start, t_run, h, w, cell, cells_x, npairs, tau, dt, normalise, out, counts); break;
    }
    return launch_status();
}
