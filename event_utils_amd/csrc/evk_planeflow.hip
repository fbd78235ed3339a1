// Plane-fit flow (include/evk.h, "Plane-fit flow"): the local plane fit of Benosman et al. (TNNLS 2014; "LocalPlanes" in Rueckauer
// & Delbruck 2016) with the event lifetime of Mueggler et al. (ICRA 2015), event by event, and the per-pixel average of the
// per-event flow.  The fit asks what the corner passes ask -- "the last event before event i at pixel q" (evk_pred.h) -- at the
// (2r + 1)^2 - 1 pixels of a window, so it runs on the grouping of evk_group.h (order[], start[]) with the lane grouping of
// evk_corner.hip:
//   decode    thread e < 64 decodes event e once (index, key, column, row, t_i); the key of an event past the end or outside
//             a checked selection is TS_NONE, nothing is looked up for it and its row is invalid
//   look-ups  lane = event, the window element z (row-major, dy outer) wave-uniform: wave v takes z = v, v + 4, ...; a lane runs
//             WAYS searches side by side (ts_search).  tau = t_j - t_i goes to LDS as doubles, [z][event], the in-use flags
//             as bytes beside it; the window is clipped to the sensor per lane
//   sums      the definition fixes the order of the three double sums (row-major from 0.0), so they cannot be split over
//             lanes; they are split over waves instead: wave 0 forms st, wave 1 sxt, wave 2 syt, wave 3 the six integer sums,
//             each over all elements in row-major order with lane = event
//   solve     every wave that needs the plane solves the 3 x 3 system from the sums in LDS (the same arithmetic in each: no
//             barrier to hand (a, b, c) round)
//   reject    the residual test is spread like the look-ups; a dropped sample clears its flag; the workgroup goes round again
//             (sums, solve) while any of its 64 events dropped a sample.  An event that dropped nothing, or whose fit failed,
//             keeps its flags, so the refit gives it the same result: no per-event "done" state
// The LDS is 10 / 19 / 32 / 50 KB for r = 1 .. 4: at r = 4 three workgroups (twelve waves) share a CU, so a lane keeps seven
// searches in flight where the corner kernels keep three (PfShape::WAYS).  The sums and the residual test load a row / a group
// from LDS before they use it, without a branch: with a load, a wait and a branch per element the pass took 7.3 ms instead of
// 6.6 ms at r = 4 (profiles/plane_flow_time.txt).  No atomics; every index comes from a key below K, a position below
// n or a checked selection, and every look-up of a lane is a pixel of the sensor.
#include "evk_common.h"
#include "evk_group.h"
#include "evk_pred.h"

namespace evk {

constexpr int PF_EVENTS = 64;                         // events per workgroup and step: one per lane
constexpr int PF_WAVES = EVK_BLOCK / EVK_WAVE;
static_assert(PF_WAVES == 4, "one wave per double sum and one for the integer sums");

template <int R>
struct PfShape {
    static constexpr int P = 2 * R + 1, PP = P * P, CENTRE = PP / 2;
    static constexpr int PER_WAVE = (PP + PF_WAVES - 1) / PF_WAVES;      // 3, 7, 13, 21 window elements
    static constexpr int WAYS = R == 1 ? 3 : 7;       // searches a lane runs side by side
    static constexpr int GROUPS = (PER_WAVE + WAYS - 1) / WAYS;          // 1, 1, 2, 3
};

struct PfParams {
    double dt, threshold, max_speed2;                 // max_speed2 = max_speed * max_speed, formed in double on the host
    int min_samples, iterations;                      // iterations: 0 without a threshold
    bool use_max_speed;
};

struct PfPlane {
    double a, b, c;
    bool ok;
};

// the plane of the sums of event `lane`: cofactors and determinant as exact integers, then the three quotients
__device__ __forceinline__ PfPlane pf_solve(const int32_t (&si)[6][PF_EVENTS], const double (&sd)[3][PF_EVENTS], int lane,
                                            int min_samples) {
    // (32 bits hold them: n <= 81, |sx|, |sy| <= 180, sxx, syy, |sxy| <= 540 at r = 4, so |cofactor| < 2^19 and |det| < 2^28)
    const int32_t n = si[0][lane], sx = si[1][lane], sy = si[2][lane], sxx = si[3][lane], sxy = si[4][lane], syy = si[5][lane];
    const int32_t c11 = syy * n - sy * sy, c12 = sx * sy - sxy * n, c13 = sxy * sy - syy * sx;
    const int32_t c22 = sxx * n - sx * sx, c23 = sxy * sx - sxx * sy, c33 = sxx * syy - sxy * sxy;
    const int32_t det = sxx * c11 + sxy * c12 + sx * c13;
    PfPlane f = {0.0, 0.0, 0.0, n >= min_samples && det != 0};
    if (f.ok) {
        const double st = sd[0][lane], sxt = sd[1][lane], syt = sd[2][lane], d = (double)det;
        f.a = (((double)c11 * sxt + (double)c12 * syt) + (double)c13 * st) / d;
        f.b = (((double)c12 * sxt + (double)c22 * syt) + (double)c23 * st) / d;
        f.c = (((double)c13 * sxt + (double)c23 * syt) + (double)c33 * st) / d;
    }
    return f;
}

template <int R>
__global__ void __launch_bounds__(EVK_BLOCK) k_planeflow_fit(const void *__restrict__ t, int kind, const uint32_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ start, int64_t n, int h, int w, PfParams prm,
                                                           const int64_t *__restrict__ select, int64_t items,
                                                           float *__restrict__ flow, float *__restrict__ lifetime,
                                                           uint8_t *__restrict__ valid) {
    using S = PfShape<R>;
    constexpr int P = S::P, PP = S::PP, WAYS = S::WAYS;
    __shared__ double tau[PP][PF_EVENTS];             // t_j - t_i of the window elements
    __shared__ uint8_t use[PP][PF_EVENTS];            // 1: the sample is in use
    __shared__ double ev_t[PF_EVENTS], sd[3][PF_EVENTS];      // st, sxt, syt
    __shared__ int32_t si[6][PF_EVENTS];              // n, sx, sy, sxx, sxy, syy
    __shared__ uint32_t ev_i[PF_EVENTS], ev_q[PF_EVENTS];
    __shared__ int32_t ev_x[PF_EVENTS], ev_y[PF_EVENTS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t steps = (items + PF_EVENTS - 1) / PF_EVENTS;
    for (int64_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const int64_t item = step * PF_EVENTS + lane;
        if (wave == 0) {
            uint32_t i = 0u, centre = TS_NONE;
            int32_t x = 0, y = 0;
            if (item < items) {
                const int64_t sel = select ? select[item] : 0;
                if (!select) i = order[item], centre = sorted[item];
                else if (sel >= 0 && sel < n) i = (uint32_t)sel, centre = keys[i];
            }
            if (centre != TS_NONE) {
                const DnPixel px = dn_pixel(centre, (uint32_t)h * (uint32_t)w, (uint32_t)w);
                y = px.y, x = px.x;
            }
            ev_i[lane] = i, ev_q[lane] = centre, ev_x[lane] = x, ev_y[lane] = y;
            ev_t[lane] = centre != TS_NONE ? ts_time(t, kind, i) : 0.0;
        }
        __syncthreads();
        const uint32_t i = ev_i[lane], centre = ev_q[lane];
        const int x = ev_x[lane], y = ev_y[lane];
        const double ti = ev_t[lane];
#pragma unroll 1
        for (int g = 0; g < S::GROUPS; ++g) {
            uint32_t q[WAYS], pos[WAYS], jn[WAYS];
#pragma unroll
            for (int u = 0; u < WAYS; ++u) {
                const int z = wave + PF_WAVES * (g * WAYS + u);
                const int dy = z / P - R, dx = z - (z / P) * P - R;
                const bool on = x + dx >= 0 && x + dx < w && y + dy >= 0 && y + dy < h;
                q[u] = centre != TS_NONE && z < PP && z != S::CENTRE && on ? (uint32_t)((int)centre + dy * w + dx) : TS_NONE;
            }
            ts_search(order, start, q, i, pos);
#pragma unroll
            for (int u = 0; u < WAYS; ++u) jn[u] = order[pos[u] != TS_NONE ? pos[u] : 0u];
#pragma unroll
            for (int u = 0; u < WAYS; ++u) {
                const int z = wave + PF_WAVES * (g * WAYS + u);
                const double tj = ts_time(t, kind, jn[u]);
                const bool in_use = z == S::CENTRE ? centre != TS_NONE : (pos[u] != TS_NONE && ti - tj <= prm.dt);
                if (z < PP) {
                    tau[z][lane] = z == S::CENTRE ? 0.0 : tj - ti;
                    use[z][lane] = in_use ? 1 : 0;
                }
            }
        }
        PfPlane fit = {0.0, 0.0, 0.0, false};
        for (int round = 0;; ++round) {
            __syncthreads();                           // the samples (of the look-ups, or less those the last round dropped)
            if (wave < 3) {
                double s = 0.0;
#pragma unroll 1
                for (int dy = -R; dy <= R; ++dy) {
                    double tv[P];                      // the row's loads first, then the chain of additions: no branch
                    uint8_t uv[P];
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) tv[dx + R] = tau[(dy + R) * P + dx + R][lane], uv[dx + R] = use[(dy + R) * P + dx + R][lane];
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        const double f = wave == 0 ? 1.0 : (double)(wave == 1 ? dx : dy);
                        const double next = s + f * tv[dx + R];
                        s = uv[dx + R] ? next : s;
                    }
                }
                sd[wave][lane] = s;
            } else {
                int cnt = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
#pragma unroll 1
                for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        const int b = use[(dy + R) * P + dx + R][lane];
                        cnt += b, sx += dx * b, sy += dy * b, sxx += dx * dx * b, sxy += dx * dy * b, syy += dy * dy * b;
                    }
                }
                si[0][lane] = cnt, si[1][lane] = sx, si[2][lane] = sy, si[3][lane] = sxx, si[4][lane] = sxy, si[5][lane] = syy;
            }
            __syncthreads();
            if (wave == 0 || prm.iterations > 0) fit = pf_solve(si, sd, lane, prm.min_samples);
            if (round >= prm.iterations) break;
            bool dropped = false;
#pragma unroll 1
            for (int g = 0; g < S::GROUPS; ++g) {      // (the elements of the look-ups; a group's loads first, no branch)
                double tv[WAYS];
                uint8_t uv[WAYS];
#pragma unroll
                for (int u = 0; u < WAYS; ++u) {
                    const int z = wave + PF_WAVES * (g * WAYS + u), zc = z < PP ? z : PP - 1;
                    tv[u] = tau[zc][lane], uv[u] = use[zc][lane];
                }
#pragma unroll
                for (int u = 0; u < WAYS; ++u) {
                    const int z = wave + PF_WAVES * (g * WAYS + u), zc = z < PP ? z : PP - 1;
                    const int dy = zc / P - R, dx = zc - (zc / P) * P - R;
                    const double e = fabs(((fit.a * (double)dx + fit.b * (double)dy) + fit.c) - tv[u]);
                    if (fit.ok && z < PP && z != S::CENTRE && uv[u] && e > prm.threshold) use[zc][lane] = 0, dropped = true;
                }
            }
            if (!__syncthreads_or(dropped ? 1 : 0)) break;      // nothing dropped in the workgroup: every fit stands
        }
        if (wave == 0 && item < items) {
            const double g = fit.a * fit.a + fit.b * fit.b;
            const bool v = fit.ok && g > 0.0 && (!prm.use_max_speed || 1.0 / g <= prm.max_speed2);
            const float nan = __builtin_nanf("");
            const int64_t row = select ? item : (int64_t)i;
            flow[2 * row] = v ? (float)(fit.a / g) : nan;
            flow[2 * row + 1] = v ? (float)(fit.b / g) : nan;
            if (lifetime) lifetime[row] = v ? (float)sqrt(g) : nan;
            valid[row] = v ? 1 : 0;
        }
    }
}

// lane = pixel: the valid flows of the pixel's run(s), class p <= 0 before class p > 0 and each in stream order, widened to
// double and summed in that order.  A hot pixel makes one lane slow; the pixels are not balanced.
__global__ void __launch_bounds__(EVK_BLOCK) k_planeflow_field(const uint32_t *__restrict__ order, const uint32_t *__restrict__ start,
                                                             int64_t n, int64_t hw, int classes, const float *__restrict__ flow,
                                                             const uint8_t *__restrict__ valid, float *__restrict__ field,
                                                             int32_t *__restrict__ count) {
    for (int64_t pix = (int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x; pix < hw; pix += (int64_t)gridDim.x * EVK_BLOCK) {
        double sx = 0.0, sy = 0.0;
        int32_t c = 0;
        for (int cls = 0; cls < classes && n > 0; ++cls) {
            const uint32_t e = start[cls * hw + pix + 1];
            for (uint32_t p = start[cls * hw + pix]; p < e; ++p) {
                const uint32_t i = order[p];
                if (!valid[i]) continue;
                sx += (double)flow[2 * (int64_t)i];
                sy += (double)flow[2 * (int64_t)i + 1];
                ++c;
            }
        }
        field[pix] = c ? (float)(sx / (double)c) : 0.0f;
        field[hw + pix] = c ? (float)(sy / (double)c) : 0.0f;
        count[pix] = c;
    }
}

template <int R>
static void pf_launch(int grid, hipStream_t s, const void *t, int kind, const DnScratch &L, int64_t n, int h, int w, const PfParams &prm,
                      const int64_t *select, int64_t items, float *flow, float *lifetime, uint8_t *valid) {
    k_planeflow_fit<R><<<grid, EVK_BLOCK, 0, s>>>(t, kind, L.keys, L.sorted, L.order, L.start, n, h, w, prm, select, items, flow, lifetime,
                                                 valid);
}

}  // namespace evk

using namespace evk;

extern "C" int evk_planeflow_fit(int t_kind, const void *t, int64_t n, int h, int w, int classes, int radius, double dt, int min_samples,
                                 int use_threshold, double threshold, int iterations, int use_max_speed, double max_speed,
                                 const int64_t *select, int64_t rows, const void *scratch, float *flow, float *lifetime,
                                 uint8_t *valid, void *stream) {
    if (radius < 1 || radius > EVK_PLANEFLOW_MAX_RADIUS || !(dt >= 0.0) || min_samples < 3 ||
        min_samples > (2 * radius + 1) * (2 * radius + 1) || (use_threshold != 0 && use_threshold != 1) || threshold != threshold ||
        (use_threshold && !(threshold > 0.0)) || iterations < 0 || iterations > EVK_PLANEFLOW_MAX_ITERATIONS ||
        (use_max_speed != 0 && use_max_speed != 1) || max_speed != max_speed || (use_max_speed && !(max_speed > 0.0)))
        return EVK_EINVAL;
    int64_t items = 0;
    DnScratch L;
    const int rc = ts_rows_check(t_kind, t, n, h, w, classes, select, rows, scratch, flow && valid ? flow : nullptr, &items, &L);
    if (rc != EVK_OK || items == 0) return rc;
    const PfParams prm = {dt, threshold, max_speed * max_speed, min_samples, use_threshold ? iterations : 0, use_max_speed != 0};
    const int64_t steps = (items + PF_EVENTS - 1) / PF_EVENTS, cap = (int64_t)EVK_NUM_CU * 8;
    const int g = (int)(steps < cap ? steps : cap);
    hipStream_t s = (hipStream_t)stream;
    switch (radius) {
        case 1: pf_launch<1>(g, s, t, t_kind, L, n, h, w, prm, select, items, flow, lifetime, valid); break;
        case 2: pf_launch<2>(g, s, t, t_kind, L, n, h, w, prm, select, items, flow, lifetime, valid); break;
        case 3: pf_launch<3>(g, s, t, t_kind, L, n, h, w, prm, select, items, flow, lifetime, valid); break;
        default: pf_launch<4>(g, s, t, t_kind, L, n, h, w, prm, select, items, flow, lifetime, valid); break;
    }
    return launch_status();
}

extern "C" int evk_planeflow_field(int64_t n, int h, int w, int classes, const void *scratch, const float *flow, const uint8_t *valid,
                                   float *field, int32_t *count, void *stream) {
    if (!field || !count || (n > 0 && (!flow || !valid))) return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, n, h, w, classes, &L)) return rc;
    const int64_t hw = (int64_t)h * w;
    k_planeflow_field<<<stream_grid(hw), EVK_BLOCK, 0, (hipStream_t)stream>>>(L.order, L.start, n, hw, classes, flow, valid, field, count);
    return launch_status();
}
