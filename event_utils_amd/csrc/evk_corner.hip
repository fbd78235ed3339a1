// Event corner detection (include/evk.h, "Corner detection"): the eFAST arc test (Mueggler, Bartolozzi, Scaramuzza, BMVC 2017)
// and the Harris score of a binary patch (Vasco, Glover, Bartolozzi, IROS 2016).  Both ask, for one event, what the time
// surfaces ask -- "the last event before event i at pixel q" (evk_pred.h) -- at many pixels (36 and 80), reduce the answers
// on chip and store one byte or one float, so they run on the grouping of evk_group.h (order[], start[]).
//
// Lane grouping (both kernels): a workgroup of four waves takes 64 events per step, in pixel order (order[p] with its sorted
// key) or in the order of `select`.
//   decode    thread e < 64 decodes event e once -- index, key, row, column, the border rule (and t_i for the time window) -- and
//             leaves the index and the key of the centre pixel in LDS; the key of an ineligible event is CN_NONE, and nothing is
//             looked up for it
//   look-ups  lane = event, and the look-up number (circle element, patch pixel) is wave-uniform: wave v takes the look-ups
//             v, v + 4, ...  So the 64 lanes of a load search the run at ONE offset from 64 events that are neighbours in pixel
//             order -- a few runs, as in the pixel-order walk of evk_denoise_support -- instead of 36 runs of one event, and
//             the offset is scalar.  A lane runs three searches side by side (ts_search; one at a time with `select`).  The
//             answers (float64 times, or patch bits as bytes) go to LDS, [look-up][event]: consecutive lanes write consecutive
//             words
//   reduce    eFAST: lane = event, wave v takes the circle elements j = v, v + 4, ...: the lane forms m_j = {k : v_k >= v_j}
//             from the circle's times in LDS; the circle has a valid arc iff some m_j has its popcount in range and is
//             cyclically contiguous (m ^ rot1(m) has two bits set): any valid arc equals m_j of its oldest element.  No loop
//             over starts and lengths.
//             Harris: lane = event, the gradient cell (a, c) wave-uniform: (Ix, Iy) as integers from the 25 patch bytes; then
//             thread e sums the 25 weighted products in float64 in the fixed order of the cells and stores the score
// The three phases are separated by workgroup barriers; at 18 KB (eFAST) and 13 KB (Harris) of LDS eight workgroups share a CU,
// so the searches of one hide the barrier of another.  No atomics; the flags of the arc test are bytes that every finder sets
// to the same 1.  Every index comes from a key below K, a position below n or a checked selection; the border rule
// (EVK_CORNER_BORDER = the largest offset) keeps every look-up of an eligible event on the sensor.
#include "evk_common.h"
#include "evk_group.h"
#include "evk_pred.h"

namespace evk {

constexpr int CN_EVENTS = 64;                         // events per workgroup and step: one per lane
constexpr int CN_WAVES = EVK_BLOCK / EVK_WAVE;
constexpr uint32_t CN_NONE = TS_NONE;
constexpr int CN_C3 = 16, CN_C4 = 20, CN_CIRCLE = CN_C3 + CN_C4;
constexpr int CN_P = 2 * EVK_CORNER_BORDER + 1, CN_PP = CN_P * CN_P;      // the 9 x 9 patch
constexpr int CN_G = 5, CN_GG = CN_G * CN_G;          // the 5 x 5 gradients
constexpr int CN_WAYS = 3;                            // searches a lane runs side by side (pixel order)
static_assert(CN_CIRCLE % (CN_WAVES * CN_WAYS) == 0, "the circle look-ups are dealt out in whole groups");

// the two circles, C3 then C4, in the cyclic order of the definition
__constant__ int8_t CN_DX[CN_CIRCLE] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1,
                                        0, 1, 2, 3, 4, 4, 4, 3, 2, 1, 0, -1, -2, -3, -4, -4, -4, -3, -2, -1};
__constant__ int8_t CN_DY[CN_CIRCLE] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3,
                                        4, 4, 3, 2, 1, 0, -1, -2, -3, -4, -4, -4, -3, -2, -1, 0, 1, 2, 3, 4};

struct CnWindow {
    double g[CN_GG];                                  // exp(-((a - 2)^2 + (c - 2)^2) / 2), normalised to sum 1
};

// Event `item` of the call: its index and the key of its pixel (CN_NONE when the event is past the end, outside a checked
// selection or on the border).  Its result goes to out[item] with `select`, to out[i] without.
__device__ __forceinline__ void cn_decode(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ sorted,
                                          const uint32_t *__restrict__ order, int64_t n, int h, int w,
                                          const int64_t *__restrict__ select, int64_t item, int64_t items, uint32_t &i,
                                          uint32_t &centre) {
    i = 0u, centre = CN_NONE;
    if (item >= items) return;
    uint32_t key;
    if (select) {
        const int64_t sel = select[item];
        if (sel < 0 || sel >= n) return;
        i = (uint32_t)sel;
        key = keys[i];
    } else {
        i = order[item];
        key = sorted[item];
    }
    const DnPixel px = dn_pixel(key, (uint32_t)h * (uint32_t)w, (uint32_t)w);
    const int y = px.y, x = px.x;
    if (x >= EVK_CORNER_BORDER && x < w - EVK_CORNER_BORDER && y >= EVK_CORNER_BORDER && y < h - EVK_CORNER_BORDER) centre = key;
}

// m: the elements of a circle of `bits` values that are not older than one of them.  A valid arc: lmin .. lmax elements, contiguous
// on the circle.
__device__ __forceinline__ bool cn_arc(uint32_t m, int bits, int lmin, int lmax) {
    const int pc = __popc(m);
    const uint32_t rot = ((m << 1) | (m >> (bits - 1))) & ((1u << bits) - 1u);
    return pc >= lmin && pc <= lmax && __popc(m ^ rot) == 2;
}

// Event `lane`, the circle of M values from row BASE of vt: has one of the elements wave, wave + 4, ... a valid arc as its
// oldest?  Every value of the circle is read once and compared with the lane's M / 4 elements.
template <int M, int BASE>
__device__ __forceinline__ bool cn_circle(const double (&vt)[CN_CIRCLE][CN_EVENTS], int lane, int wave, int lmin, int lmax) {
    constexpr int R = M / CN_WAVES;
    static_assert(M % CN_WAVES == 0, "every wave takes the same number of elements");
    double vj[R];
    uint32_t m[R];
#pragma unroll
    for (int r = 0; r < R; ++r) vj[r] = vt[BASE + wave + CN_WAVES * r][lane], m[r] = 0u;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const double vk = vt[BASE + k][lane];
#pragma unroll
        for (int r = 0; r < R; ++r) m[r] |= (vk >= vj[r] ? 1u : 0u) << k;
    }
    bool any = false;
#pragma unroll
    for (int r = 0; r < R; ++r) any |= cn_arc(m[r], M, lmin, lmax);
    return any;
}

template <int WAYS>
__global__ void __launch_bounds__(EVK_BLOCK, 8) k_corner_fast(const void *__restrict__ t, int kind, const uint32_t *__restrict__ keys,
                                                         const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ start, int64_t n, int h, int w,
                                                         const int64_t *__restrict__ select, int64_t items,
                                                         uint8_t *__restrict__ out) {
    __shared__ double vt[CN_CIRCLE][CN_EVENTS];       // the time of last(q, i), -inf when there is none
    __shared__ uint32_t ev_i[CN_EVENTS], ev_q[CN_EVENTS];
    __shared__ uint8_t ok3[CN_EVENTS], ok4[CN_EVENTS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t steps = (items + CN_EVENTS - 1) / CN_EVENTS;
    for (int64_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const int64_t item = step * CN_EVENTS + lane;
        if (wave == 0) {
            uint32_t i, centre;
            cn_decode(keys, sorted, order, n, h, w, select, item, items, i, centre);
            ev_i[lane] = i, ev_q[lane] = centre;
            ok3[lane] = 0, ok4[lane] = 0;
        }
        __syncthreads();
        const uint32_t i = ev_i[lane], centre = ev_q[lane];
        for (int g = 0; g < CN_CIRCLE / (CN_WAVES * WAYS); ++g) {
            uint32_t q[WAYS], pos[WAYS], jn[WAYS];
#pragma unroll
            for (int u = 0; u < WAYS; ++u) {
                const int j = wave + CN_WAVES * (g * WAYS + u);
                q[u] = centre != CN_NONE ? (uint32_t)((int)centre + (int)CN_DY[j] * w + (int)CN_DX[j]) : CN_NONE;
            }
            ts_search(order, start, q, i, pos);
#pragma unroll
            for (int u = 0; u < WAYS; ++u) jn[u] = order[pos[u] != CN_NONE ? pos[u] : 0u];
#pragma unroll
            for (int u = 0; u < WAYS; ++u) {
                const double tj = ts_time(t, kind, jn[u]);
                vt[wave + CN_WAVES * (g * WAYS + u)][lane] = pos[u] != CN_NONE ? tj : -(double)__builtin_inff();
            }
        }
        __syncthreads();
        if (centre != CN_NONE) {
            const bool any3 = cn_circle<CN_C3, 0>(vt, lane, wave, 3, 6), any4 = cn_circle<CN_C4, CN_C3>(vt, lane, wave, 4, 8);
            if (any3) ok3[lane] = 1;
            if (any4) ok4[lane] = 1;
        }
        __syncthreads();
        if (wave == 0 && item < items) out[select ? item : (int64_t)i] = (uint8_t)(ok3[lane] & ok4[lane]);
    }
}

// WINDOW: EVK_CORNER_WINDOW_COUNT (recent iff j >= i - n_last) or EVK_CORNER_WINDOW_TIME (recent iff t_i - t_j <= dt in double)
template <int WINDOW, int WAYS>
__global__ void __launch_bounds__(EVK_BLOCK) k_corner_harris(const void *__restrict__ t, int kind, const uint32_t *__restrict__ keys,
                                                           const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ start, int64_t n, int h, int w,
                                                           int64_t n_last, double dt, double k, CnWindow win,
                                                           const int64_t *__restrict__ select, int64_t items,
                                                           float *__restrict__ out) {
    __shared__ double ev_t[CN_EVENTS];
    __shared__ uint32_t ev_i[CN_EVENTS], ev_q[CN_EVENTS];
    __shared__ uint8_t pb[CN_PP][CN_EVENTS];          // the binary patch, row-major (dy + 4, dx + 4)
    __shared__ int32_t gr[CN_GG][CN_EVENTS];          // Ix in the low half, Iy in the high half
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int S[CN_G] = {1, 4, 6, 4, 1}, D[CN_G] = {-1, -2, 0, 2, 1};
    const int64_t steps = (items + CN_EVENTS - 1) / CN_EVENTS;
    for (int64_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const int64_t item = step * CN_EVENTS + lane;
        if (wave == 0) {
            uint32_t i, centre;
            cn_decode(keys, sorted, order, n, h, w, select, item, items, i, centre);
            ev_i[lane] = i, ev_q[lane] = centre;
            if (WINDOW == EVK_CORNER_WINDOW_TIME) ev_t[lane] = centre != CN_NONE ? ts_time(t, kind, i) : 0.0;
        }
        __syncthreads();
        const uint32_t i = ev_i[lane], centre = ev_q[lane];
        const double ti = WINDOW == EVK_CORNER_WINDOW_TIME ? ev_t[lane] : 0.0;
        for (int g = 0; g < (CN_PP + CN_WAVES * WAYS - 1) / (CN_WAVES * WAYS); ++g) {
            uint32_t q[WAYS], pos[WAYS], jn[WAYS];
#pragma unroll
            for (int u = 0; u < WAYS; ++u) {
                const int z = wave + CN_WAVES * (g * WAYS + u);
                const int dy = z / CN_P - EVK_CORNER_BORDER, dx = z - (z / CN_P) * CN_P - EVK_CORNER_BORDER;
                q[u] = centre != CN_NONE && z < CN_PP && z != CN_PP / 2 ? (uint32_t)((int)centre + dy * w + dx) : CN_NONE;
            }
            ts_search(order, start, q, i, pos);
#pragma unroll
            for (int u = 0; u < WAYS; ++u) jn[u] = order[pos[u] != CN_NONE ? pos[u] : 0u];
#pragma unroll
            for (int u = 0; u < WAYS; ++u) {
                const int z = wave + CN_WAVES * (g * WAYS + u);
                bool recent;
                if (WINDOW == EVK_CORNER_WINDOW_COUNT) recent = (int64_t)jn[u] >= (int64_t)i - n_last;
                else recent = ti - ts_time(t, kind, jn[u]) <= dt;
                const bool b = centre != CN_NONE && (z == CN_PP / 2 || (pos[u] != CN_NONE && recent));
                if (z < CN_PP) pb[z][lane] = b ? 1 : 0;
            }
        }
        __syncthreads();
        if (centre != CN_NONE) {
            for (int cell = wave; cell < CN_GG; cell += CN_WAVES) {
                const int a = cell / CN_G, c = cell - a * CN_G;
                int ix = 0, iy = 0;
#pragma unroll
                for (int u = 0; u < CN_G; ++u) {
#pragma unroll
                    for (int v = 0; v < CN_G; ++v) {
                        const int b = pb[(a + u) * CN_P + c + v][lane];
                        ix += S[u] * D[v] * b;
                        iy += D[u] * S[v] * b;
                    }
                }
                gr[cell][lane] = (ix & 0xFFFF) | (int32_t)((uint32_t)iy << 16);
            }
        }
        __syncthreads();
        if (wave == 0 && item < items) {
            float score = __builtin_nanf("");
            if (centre != CN_NONE) {
                double A = 0.0, B = 0.0, C = 0.0;
                for (int cell = 0; cell < CN_GG; ++cell) {
                    const int32_t pk = gr[cell][lane];
                    const int ix = (int)(int16_t)(pk & 0xFFFF), iy = pk >> 16;
                    const double g = win.g[cell];
                    A += g * (double)(ix * ix);
                    B += g * (double)(iy * iy);
                    C += g * (double)(ix * iy);
                }
                A /= 144.0, B /= 144.0, C /= 144.0;
                score = (float)((A * B - C * C) - k * ((A + B) * (A + B)));
            }
            out[select ? item : (int64_t)i] = score;
        }
    }
}

static int cn_grid(int64_t items) {
    const int64_t steps = (items + CN_EVENTS - 1) / CN_EVENTS, cap = (int64_t)EVK_NUM_CU * 8;
    return (int)(steps < cap ? steps : cap);
}

}  // namespace evk

using namespace evk;

extern "C" int evk_corner_fast(int t_kind, const void *t, int64_t n, int h, int w, int classes, const int64_t *select, int64_t rows,
                               const void *scratch, uint8_t *out, void *stream) {
    int64_t items = 0;
    DnScratch L;
    const int rc = ts_rows_check(t_kind, t, n, h, w, classes, select, rows, scratch, out, &items, &L);
    if (rc != EVK_OK || items == 0) return rc;
    const int g = cn_grid(items);
    hipStream_t s = (hipStream_t)stream;
    if (select) k_corner_fast<1><<<g, EVK_BLOCK, 0, s>>>(t, t_kind, L.keys, L.sorted, L.order, L.start, n, h, w, select, items, out);
    else k_corner_fast<CN_WAYS><<<g, EVK_BLOCK, 0, s>>>(t, t_kind, L.keys, L.sorted, L.order, L.start, n, h, w, select, items, out);
    return launch_status();
}

extern "C" int evk_corner_harris(int t_kind, const void *t, int64_t n, int h, int w, int classes, int window, int64_t n_last,
                                 double dt, double k, const int64_t *select, int64_t rows, const void *scratch, float *out,
                                 void *stream) {
    if ((window != EVK_CORNER_WINDOW_COUNT && window != EVK_CORNER_WINDOW_TIME) || n_last < 1 || !(dt >= 0.0) || k != k)
        return EVK_EINVAL;                             // (both window parameters are checked whichever is used)
    int64_t items = 0;
    DnScratch L;
    const int rc = ts_rows_check(t_kind, t, n, h, w, classes, select, rows, scratch, out, &items, &L);
    if (rc != EVK_OK || items == 0) return rc;
    CnWindow win;
    double sum = 0.0;
    for (int a = 0; a < CN_G; ++a)
        for (int c = 0; c < CN_G; ++c) sum += win.g[a * CN_G + c] = exp(-(double)((a - 2) * (a - 2) + (c - 2) * (c - 2)) / 2.0);
    for (int e = 0; e < CN_GG; ++e) win.g[e] /= sum;
    const int g = cn_grid(items);
    hipStream_t s = (hipStream_t)stream;
    if (window == EVK_CORNER_WINDOW_COUNT && select)
        k_corner_harris<EVK_CORNER_WINDOW_COUNT, 1><<<g, EVK_BLOCK, 0, s>>>(t, t_kind, L.keys, L.sorted, L.order, L.start, n, h, w, n_last, dt, k, win, select, items, out);
    else if (window == EVK_CORNER_WINDOW_COUNT)
        k_corner_harris<EVK_CORNER_WINDOW_COUNT, CN_WAYS><<<g, EVK_BLOCK, 0, s>>>(t, t_kind, L.keys, L.sorted, L.order, L.start, n, h, w, n_last, dt, k, win, select, items, out);
    else if (select)
        k_corner_harris<EVK_CORNER_WINDOW_TIME, 1><<<g, EVK_BLOCK, 0, s>>>(t, t_kind, L.keys, L.sorted, L.order, L.start, n, h, w, n_last, dt, k, win, select, items, out);
    else
        k_corner_harris<EVK_CORNER_WINDOW_TIME, CN_WAYS><<<g, EVK_BLOCK, 0, s>>>(t, t_kind, L.keys, L.sorted, L.order, L.start, n, h, w, n_last, dt, k, win, select, items, out);
    return launch_status();
}
