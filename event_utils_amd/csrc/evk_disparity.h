// The disparity winner and its tests (include/evk.h, "Event stereo"), stated once for block matching (evk_stereo.hip, the costs of
// a pixel come out of the cost loop) and for a cost volume in memory (evk_sgm.hip):
//
//   DisparityWinner    the accumulator a pixel's costs go through in increasing step i
//   disparity_decide   the winner d*, c1, c2, the uniqueness test, the cost limit and the parabola
//   disparity_write / disparity_write_none   the four outputs of a candidate and of a pixel that is none, and the mark in scratch
//   k_disparity_lr     the left-right test, one lane per pixel
//   disparity_match    the host side of an entry point: the switches, the scratch and the order of the passes
//
// Every value is an integer but the parabola, which is one float64 formula: a result is the same bits from either caller.
#pragma once
#include <type_traits>

#include "evk_common.h"

namespace evk {

constexpr int kWanted = -2;                             // a scratch cell whose right pixel's winner is wanted (-1: it is not)

struct DisparityTests {
    int min_activity, uniqueness, lr, subpixel;         // lr: the tolerance of the left-right test, -1 without one
    int64_t max_cost;                                   // -1: no limit
};

struct DisparityOut {
    int32_t *scratch, *index, *cost;
    float *disparity;
    uint8_t *mask;
};

// The four smallest keys (cost << 8 | i: least cost first, the smaller step on ties) and the neighbours of the running winner.
// Key: uint32_t where a cost is below 2^24 (block matching: below 2^17), uint64_t for any present int32.  HOLES: a cell may be
// absent (cost < 0); it is nobody's neighbour.  A present cost is below 2^31, so the first one beats `best`.
template <class Key, bool HOLES>
struct DisparityWinner {
    using Wide = std::conditional_t<sizeof(Key) == 8, int64_t, int>;      // the width of the arithmetic on the costs
    static constexpr Key kNone = ~(Key)0;
    Key m0 = kNone, m1 = kNone, m2 = kNone, m3 = kNone;
    uint32_t best = 0xFFFFFFFFu;
    int at = -2, prev = -1, cm = -1, cp = -1;
    __device__ __forceinline__ void operator()(int i, int32_t cost) {
        if (HOLES && cost < 0) {
            prev = -1;
            return;
        }
        if (i == at + 1) cp = cost;
        if ((uint32_t)cost < best) best = cost, at = i, cm = prev, cp = -1;
        prev = cost;
        Key k = ((Key)(uint32_t)cost << 8) | (Key)i, t;
        t = min(m0, k), k = max(m0, k), m0 = t;
        t = min(m1, k), k = max(m1, k), m1 = t;
        t = min(m2, k), k = max(m2, k), m2 = t;
        m3 = min(m3, k);
    }
    __device__ __forceinline__ bool empty() const { return at < 0; }     // no present cell: the pixel is no candidate
};

template <class Wide>
struct DisparityPick {
    int d;
    Wide c1;
    bool valid;
    float disparity;
};

// the decision on a winner that is not empty
template <class Key, bool HOLES>
__device__ __forceinline__ auto disparity_decide(const DisparityWinner<Key, HOLES> &win, int d_min, const DisparityTests &t) {
    using Wide = typename DisparityWinner<Key, HOLES>::Wide;
    const int at = (int)(win.m0 & 255u);
    const Wide c1 = (Wide)(win.m0 >> 8);
    Wide c2 = -1;                                                       // the least cost more than one step from the winner
    const Key rest[3] = {win.m3, win.m2, win.m1};
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (rest[j] != win.kNone && abs((int)(rest[j] & 255u) - at) > 1) c2 = (Wide)(rest[j] >> 8);
    bool valid = c2 < 0 || (int64_t)c2 * (100 - t.uniqueness) >= (int64_t)100 * c1;
    valid = valid && (t.max_cost < 0 || (int64_t)c1 <= t.max_cost);
    const int d = d_min + at;
    float disp = (float)d;
    if (t.subpixel && win.cm >= 0 && win.cp >= 0) {
        const Wide cm = win.cm, cp = win.cp, den = cm - 2 * c1 + cp;
        if (den > 0) disp = (float)((double)d + (double)(cm - cp) / (double)(2 * den));
    }
    return DisparityPick<Wide>{d, c1, valid, disp};
}

// pixel q (k, y, x in row-major order) is a candidate; its right pixel q - d is in the same row (x - d >= 0: d is admissible).
// (pick by value: by reference k_sgm_winner takes 36 VGPRs for 34)
template <class Wide>
__device__ __forceinline__ void disparity_write(const DisparityOut &o, int64_t q, DisparityPick<Wide> pick, int lr) {
    o.cost[q] = (int32_t)pick.c1;
    o.index[q] = pick.valid ? pick.d : -1;
    o.mask[q] = pick.valid ? 1 : 0;
    o.disparity[q] = pick.valid ? pick.disparity : __builtin_nanf("");
    if (pick.valid && lr >= 0) o.scratch[q - pick.d] = kWanted;
}

__device__ __forceinline__ void disparity_write_none(const DisparityOut &o, int64_t q) {
    o.cost[q] = -1, o.index[q] = -1, o.mask[q] = 0;
    o.disparity[q] = __builtin_nanf("");
}

// the left-right test of the pixels that passed the others: scratch holds the right image's own winner where one was wanted
static __global__ void __launch_bounds__(EVK_BLOCK) k_disparity_lr(const int32_t *__restrict__ scratch, int64_t total, int tolerance,
                                                                   int32_t *__restrict__ index, float *__restrict__ disparity,
                                                                   uint8_t *__restrict__ mask) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int d = index[q];
        if (d < 0) continue;
        if (abs(scratch[q - d] - d) > tolerance) {                      // (the same row: x - d >= 0)
            index[q] = -1, mask[q] = 0;
            disparity[q] = __builtin_nanf("");
        }
    }
}

// What evk_stereo_match and evk_sgm_match_volume share behind their own size checks: the switches and the outputs as the kernels
// take them, every scratch cell -1 (not wanted), and the passes in order.  pass(tests, out, right) launches the caller's winner
// pass (right false: it writes the outputs and the marks) or its right pass (true: scratch[q] = the right pixel's own winner where
// q is marked) and returns the launch's status.  total: the K H W pixels.
template <class Pass>
static int disparity_match(int min_activity, int uniqueness, int64_t max_cost, int lr_tolerance, int subpixel, void *scratch,
                           float *disparity, void *index, void *cost, void *mask, int64_t total, hipStream_t s, Pass &&pass) {
    if (!disparity || !index || !cost || !mask || min_activity < 1 || min_activity > 255 || uniqueness < 0 || uniqueness > 99 ||
        (subpixel != 0 && subpixel != 1) || (lr_tolerance >= 0 && !scratch))
        return EVK_EINVAL;
    const DisparityTests t = {min_activity, uniqueness, lr_tolerance < 0 ? -1 : lr_tolerance, subpixel, max_cost < 0 ? -1 : max_cost};
    const DisparityOut o = {static_cast<int32_t *>(scratch), static_cast<int32_t *>(index), static_cast<int32_t *>(cost), disparity,
                            static_cast<uint8_t *>(mask)};
    if (t.lr >= 0) {
        hipError_t e = hipMemsetAsync(scratch, 0xFF, (size_t)total * sizeof(int32_t), s);
        if (e != hipSuccess) return (int)e;
    }
    if (int rc = pass(t, o, false)) return rc;
    if (t.lr < 0) return EVK_OK;
    if (int rc = pass(t, o, true)) return rc;
    k_disparity_lr<<<stream_grid(total), EVK_BLOCK, 0, s>>>(o.scratch, total, t.lr, o.index, o.disparity, o.mask);
    return launch_status();
}

}  // namespace evk
