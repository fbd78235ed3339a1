// Semi-global matching (include/evk.h, "Semi-global matching"): path aggregation of a stereo cost volume after Hirschmueller
// (PAMI 2008), and the winner of any cost volume under the tests of "Event stereo".
//
//   k_sgm_transpose<IN>   the volume is d-major, (K, D, H W): one pixel's disparities lie 4 H W bytes apart.  The paths run on a
//                         d-contiguous copy (K, H W, D): a tile of 64 disparities x 64 pixels goes through LDS (pitch 65 dwords: no
//                         bank is hit twice either way), read and written in runs of 256 bytes.  IN clamps the costs on the way;
//                         the other direction carries the sums back.
//   k_sgm_path<G, R>      every chosen direction in one launch, blockIdx.y the direction.  A path is sequential along its line,
//                         so the lanes lie across d: a line owns G lanes (G = 64 / lines per wave, the power of two >= D) with R
//                         disparities each (R > 1 only past 64), d = 64 r + lane.  A step loads the pixel's D costs as one run,
//                         takes min_j L(q, j) by DPP (quad_perm, row_half_mirror, row_mirror, row_bcast: no LDS instruction),
//                         reads L(q, i -+ 1) from the neighbour lanes by DPP wave rotates, and adds L into the sum.  The loads do
//                         not depend on the walk, so those of the next kSgmAhead steps are issued before the current ones are
//                         worked: the chain of a line is the arithmetic alone.
//   k_sgm_winner / k_sgm_right / k_disparity_lr   the winner: one lane per pixel walks the D cells of its pixel, a row of lanes
//                         reading a row of the volume (coalesced); the marks, the right pixels' own winners and the comparison
//                         are the three passes of evk_stereo.hip on a volume in memory.  The winner and its tests are those of
//                         evk_disparity.h, the accumulator on 64-bit keys (a value may be 2^31 - 1) and with absent cells.
//
// A line is a chain of dependent steps, and one direction alone leaves most of the SIMDs without a wave, so the directions run side
// by side and each adds its L into the sums with an integer atomic that returns nothing: integer adds commute, the sums are the
// same bits in any order.  The transpose on the way in sets the sums to 0 (-1 where the cell is absent, which no direction touches).
#include "evk_disparity.h"

namespace evk {

constexpr int kSgmInf = 0x3FFFFFFF;                     // an absent cell of q: more than any L + P2, and twice it fits an int
constexpr int kSgmTile = 64;                            // the transpose tile: 64 disparities x 64 pixels
constexpr int kSgmPitch = kSgmTile + 1;
constexpr int kSgmThreads = 256;
constexpr int kSgmAhead = 4;                            // steps of a path whose loads are in flight

// v of the lane that `ctrl` names (all 64 lanes active); a lane without a source, or in a row left out, keeps its own
#define EVK_SGM_DPP(v, ctrl, rows) __builtin_amdgcn_update_dpp((v), (v), (ctrl), (rows), 0xf, false)

struct SgmPathArgs {
    const int32_t *c;
    int32_t *s;
    int nd, h, w, nk, p1, p2;
    uint32_t directions;                                    // four bits a chosen direction, dx + 1 | (dy + 1) << 2: blockIdx.y names one
};

struct SgmMatchArgs {
    const int32_t *volume;
    const uint8_t *activity;
    int nc, h, w, d_min, nd;
    DisparityTests tests;
    int64_t total;
    DisparityOut out;
};

// ---- the two layouts -------------------------------------------------------------------------------------------------------------

// IN: src (K, D, npix) -> dst (K, npix, D), a present cost clamped to EVK_SGM_MAX_COST and an absent one -1, and `sums` in the
// layout of dst 0 and -1 alike; else the way back
template <bool IN>
__global__ void __launch_bounds__(kSgmThreads) k_sgm_transpose(const int32_t *__restrict__ src, int32_t *__restrict__ dst,
                                                               int32_t *__restrict__ sums, int nd, int npix, int tiles_p, int tiles_d) {
    __shared__ int32_t tile[kSgmTile * kSgmPitch];
    const int per = tiles_p * tiles_d;
    const int k = blockIdx.x / per, rest = blockIdx.x - k * per;
    const int td = rest / tiles_p, tp = rest - td * tiles_p;
    const int p0 = tp * kSgmTile, d0 = td * kSgmTile;
    const int np = min(kSgmTile, npix - p0), nt = min(kSgmTile, nd - d0);
    const int32_t *dmajor_in = src + ((int64_t)k * nd + d0) * npix + p0;
    const int32_t *pmajor_in = src + ((int64_t)k * npix + p0) * nd + d0;
    int32_t *dmajor_out = dst + ((int64_t)k * nd + d0) * npix + p0;
    int32_t *pmajor_out = dst + ((int64_t)k * npix + p0) * nd + d0;
    if constexpr (IN) {
        for (int idx = threadIdx.x; idx < kSgmTile * kSgmTile; idx += kSgmThreads) {
            const int d = idx >> 6, p = idx & 63;
            if (d < nt && p < np) {
                const int32_t v = dmajor_in[(int64_t)d * npix + p];
                tile[d * kSgmPitch + p] = v < 0 ? -1 : min(v, (int32_t)EVK_SGM_MAX_COST);
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < np * nt; idx += kSgmThreads) {
            const int p = idx / nt, d = idx - p * nt;
            const int32_t v = tile[d * kSgmPitch + p];
            pmajor_out[(int64_t)p * nd + d] = v;
            sums[((int64_t)k * npix + p0 + p) * nd + d0 + d] = v < 0 ? -1 : 0;      // the sums start here: no direction touches an absent cell
        }
    } else {
        for (int idx = threadIdx.x; idx < np * nt; idx += kSgmThreads) {
            const int p = idx / nt, d = idx - p * nt;
            tile[d * kSgmPitch + p] = pmajor_in[(int64_t)p * nd + d];
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < kSgmTile * kSgmTile; idx += kSgmThreads) {
            const int d = idx >> 6, p = idx & 63;
            if (d < nt && p < np) dmajor_out[(int64_t)d * npix + p] = tile[d * kSgmPitch + p];
        }
    }
}

// ---- a direction -----------------------------------------------------------------------------------------------------------------

__host__ __device__ inline int sgm_lines(int h, int w, int dx, int dy) { return dy == 0 ? h : dx == 0 ? w : h + w - 1; }

// line l of direction (dx, dy): its first pixel (the one whose predecessor is off the sensor) and its length
__device__ __forceinline__ void sgm_line(int l, int h, int w, int dx, int dy, int &x0, int &y0, int &n) {
    const int xe = dx > 0 ? 0 : w - 1, ye = dy > 0 ? 0 : h - 1;
    if (dy == 0) {
        x0 = xe, y0 = l, n = w;
    } else if (dx == 0) {
        x0 = l, y0 = ye, n = h;
    } else {
        if (l < h) {
            x0 = xe, y0 = l;
        } else {
            const int j = l - h + 1;                                    // 1 .. w - 1: the corner belongs to the edge column
            x0 = dx > 0 ? j : w - 1 - j, y0 = ye;
        }
        n = min(dx > 0 ? w - x0 : x0 + 1, dy > 0 ? h - y0 : y0 + 1);
    }
}

// the least of the G lanes of a line's group, in every lane of the group.  All 64 lanes active.
template <int G>
__device__ __forceinline__ int sgm_group_min(int v) {
    if constexpr (G >= 2) v = min(v, EVK_SGM_DPP(v, 0xB1, 0xf));        // quad_perm:[1,0,3,2]
    if constexpr (G >= 4) v = min(v, EVK_SGM_DPP(v, 0x4E, 0xf));        // quad_perm:[2,3,0,1]
    if constexpr (G >= 8) v = min(v, EVK_SGM_DPP(v, 0x141, 0xf));       // row_half_mirror
    if constexpr (G >= 16) v = min(v, EVK_SGM_DPP(v, 0x140, 0xf));      // row_mirror: every row of 16 holds its least
    if constexpr (G == 32) v = min(v, __shfl_xor(v, 16));
    if constexpr (G == 64) {
        v = min(v, EVK_SGM_DPP(v, 0x142, 0xa));                         // row_bcast:15 into rows 1 and 3
        v = min(v, EVK_SGM_DPP(v, 0x143, 0xc));                         // row_bcast:31 into rows 2 and 3: lane 63 holds the least
        v = __builtin_amdgcn_readlane(v, 63);
    }
    return v;
}

template <int G, int R>
__global__ void __launch_bounds__(kSgmThreads) k_sgm_path(SgmPathArgs a) {
    static_assert(R == 1 || G == 64, "several disparities per lane only on a whole wave");
    constexpr int LPW = 64 / G;                                         // lines per wave
    const int lane = threadIdx.x & 63, sub = lane / G, dl = lane & (G - 1);
    const int64_t wave = (int64_t)blockIdx.x * (kSgmThreads / 64) + (threadIdx.x >> 6);
    const int64_t line = wave * LPW + sub;
    const int npix = a.h * a.w, nd = a.nd;
    const int code = (int)(a.directions >> (4 * blockIdx.y)) & 15;
    const int dx = (code & 3) - 1, dy = (code >> 2) - 1, nlines = sgm_lines(a.h, a.w, dx, dy);
    int x0 = 0, y0 = 0, n = 0;
    int64_t k = 0;
    if (line < (int64_t)a.nk * nlines) {
        k = line / nlines;
        sgm_line((int)(line - k * nlines), a.h, a.w, dx, dy, x0, y0, n);
    }
    int nmax = n;                                                       // the longest line of the wave: the loop is wave-uniform
#pragma unroll
    for (int off = 32; off >= G && off >= 1; off >>= 1) nmax = max(nmax, __shfl_xor(nmax, off));
    nmax = __builtin_amdgcn_readfirstlane(nmax);
    if (nmax == 0) return;

    const int64_t base = (k * npix + (int64_t)y0 * a.w + x0) * nd + dl;
    const int64_t stride = ((int64_t)dy * a.w + dx) * nd;
    const int p1 = a.p1, p2 = a.p2;
    bool dok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) dok[r] = 64 * r + dl < nd;

    int32_t cc[kSgmAhead][R], nc[kSgmAhead][R];
    const auto load = [&](int t0, int32_t (&c)[kSgmAhead][R]) {
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool ok = t0 + u < n && dok[r];
                const int64_t at = base + (int64_t)(t0 + u) * stride + 64 * r;
                c[u][r] = ok ? a.c[at] : -1;
            }
    };
    load(0, cc);
    int32_t prev[R];                                                    // L(q, .), kSgmInf where the cell is absent or q is off the line
#pragma unroll
    for (int r = 0; r < R; ++r) prev[r] = kSgmInf;

#pragma unroll 1
    for (int t0 = 0; t0 < nmax; t0 += kSgmAhead) {
        if (t0 + kSgmAhead < nmax) load(t0 + kSgmAhead, nc);
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u) {
            int least = prev[0];
#pragma unroll
            for (int r = 1; r < R; ++r) least = min(least, prev[r]);
            const int m = sgm_group_min<G>(least);                      // kSgmInf: q has no present cell, the path starts again
            int32_t lo[R], hi[R];                                       // L(q, i - 1) and L(q, i + 1)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int below = EVK_SGM_DPP(prev[r], 0x13C, 0xf);     // wave_ror:1: lane i reads lane i - 1, lane 0 lane 63
                const int above = EVK_SGM_DPP(prev[r], 0x134, 0xf);     // wave_rol:1: lane i reads lane i + 1, lane 63 lane 0
                const int carry_lo = r > 0 ? EVK_SGM_DPP(prev[r > 0 ? r - 1 : 0], 0x13C, 0xf) : kSgmInf;
                const int carry_hi = r < R - 1 ? EVK_SGM_DPP(prev[r < R - 1 ? r + 1 : 0], 0x134, 0xf) : kSgmInf;
                lo[r] = dl == 0 ? carry_lo : below;
                hi[r] = dl == G - 1 ? carry_hi : above;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int32_t c = cc[u][r];
                const int best = min(min(prev[r], m + p2), min(lo[r], hi[r]) + p1);
                const int32_t l = m < kSgmInf ? c + best - m : c;
                const int64_t at = base + (int64_t)(t0 + u) * stride + 64 * r;
                if (c >= 0) atomic_add(a.s + at, l);
                prev[r] = c >= 0 ? l : kSgmInf;
            }
        }
#pragma unroll
        for (int u = 0; u < kSgmAhead; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) cc[u][r] = nc[u][r];
    }
}

// ---- the winner of a volume ------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(EVK_BLOCK) k_sgm_winner(SgmMatchArgs p) {
    const int64_t npix = (int64_t)p.h * p.w;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < p.total; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = q / npix, pix = q - k * npix;
        const int x = (int)(pix % p.w);
        int act = 0;
        for (int c = 0; c < p.nc; ++c) act = max(act, (int)p.activity[(k * p.nc + c) * npix + pix]);
        const int lim = min(max(x - p.d_min + 1, 0), p.nd);             // the steps with a right pixel: x - d >= 0
        DisparityWinner<uint64_t, true> win;
        if (act >= p.tests.min_activity) {
            const int32_t *v = p.volume + k * p.nd * npix + pix;
            for (int i = 0; i < lim; ++i) win(i, v[(int64_t)i * npix]);
        }
        if (win.empty()) disparity_write_none(p.out, q);
        else disparity_write(p.out, q, disparity_decide(win, p.d_min, p.tests), p.tests.lr);
    }
}

// the right image's own winner where one is wanted: the d with x' + d <= w - 1 of least volume[k, d - d_min, y, x' + d]
__global__ void __launch_bounds__(EVK_BLOCK) k_sgm_right(SgmMatchArgs p) {
    const int64_t npix = (int64_t)p.h * p.w;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < p.total; q += (int64_t)gridDim.x * blockDim.x) {
        if (p.out.scratch[q] != kWanted) continue;
        const int64_t k = q / npix, pix = q - k * npix;
        const int room = p.w - 1 - (int)(pix % p.w);                    // d <= room
        const int lim = room < p.d_min ? 0 : min(room - p.d_min + 1, p.nd);
        const int32_t *v = p.volume + k * p.nd * npix + pix + p.d_min;
        int best = -1, at = 0;
        for (int i = 0; i < lim; ++i) {
            const int32_t c = v[(int64_t)i * npix + i];
            if (c >= 0 && (best < 0 || c < best)) best = c, at = i;
        }
        p.out.scratch[q] = p.d_min + at;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------

static inline bool sgm_sizes_ok(int nk, int nd, int h, int w) {
    if (nk < 1 || h < 1 || w < 1 || (int64_t)h * w > 0x7FFFFFFFll || nd < 1 || nd > EVK_STEREO_MAX_DISPARITIES) return false;
    if ((int64_t)nk * nd * h * w > ((int64_t)1 << 40)) return false;
    const int64_t tiles = (int64_t)nk * (((int64_t)h * w + kSgmTile - 1) / kSgmTile) * ((nd + kSgmTile - 1) / kSgmTile);
    return tiles <= 0x7FFFFFFFll && (int64_t)nk * ((int64_t)h + w) <= 0x7FFFFFFFll;       // the grids of the transposes and the paths
}

// every chosen direction in one launch: blockIdx.y is the direction, and a block past its direction's lines leaves at once
template <int G, int R>
static void sgm_path_launch(const SgmPathArgs &a, int directions, hipStream_t s) {
    int most = 0;                                                                                    // the lines of the longest chosen direction
    for (int j = 0; j < directions; ++j) {
        const int code = (int)(a.directions >> (4 * j)) & 15;
        most = max(most, sgm_lines(a.h, a.w, (code & 3) - 1, (code >> 2) - 1));
    }
    const int64_t lines = (int64_t)a.nk * most;
    const int64_t waves = (lines + 64 / G - 1) / (64 / G);
    const dim3 grid((unsigned)((waves + kSgmThreads / 64 - 1) / (kSgmThreads / 64)), (unsigned)directions);
    k_sgm_path<G, R><<<grid, kSgmThreads, 0, s>>>(a);
}

static void sgm_path(const SgmPathArgs &a, int n, hipStream_t s) {
    const int nd = a.nd;
    if (nd > 192) sgm_path_launch<64, 4>(a, n, s);
    else if (nd > 128) sgm_path_launch<64, 3>(a, n, s);
    else if (nd > 64) sgm_path_launch<64, 2>(a, n, s);
    else if (nd > 32) sgm_path_launch<64, 1>(a, n, s);
    else if (nd > 16) sgm_path_launch<32, 1>(a, n, s);
    else if (nd > 8) sgm_path_launch<16, 1>(a, n, s);
    else if (nd > 4) sgm_path_launch<8, 1>(a, n, s);
    else if (nd > 2) sgm_path_launch<4, 1>(a, n, s);
    else if (nd > 1) sgm_path_launch<2, 1>(a, n, s);
    else sgm_path_launch<1, 1>(a, n, s);
}

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_sgm_scratch_bytes(int call, int nk, int nd, int h, int w) {
    if ((call != EVK_SGM_AGGREGATE && call != EVK_SGM_MATCH) || !sgm_sizes_ok(nk, nd, h, w)) return EVK_EINVAL;
    const int64_t cells = (int64_t)nk * h * w;
    return call == EVK_SGM_AGGREGATE ? 2 * cells * nd * (int64_t)sizeof(int32_t) : cells * (int64_t)sizeof(int32_t);
}

extern "C" int evk_sgm_aggregate(const void *volume, int nk, int nd, int h, int w, int p1, int p2, int directions, void *scratch,
                                 void *out, void *stream) {
    if (!volume || !scratch || !out || !sgm_sizes_ok(nk, nd, h, w) || p1 < 0 || p1 > p2 || p2 > EVK_SGM_MAX_PENALTY || directions < 1 ||
        directions > 255)
        return EVK_EINVAL;
    static const int kDx[8] = {1, -1, 0, 0, 1, -1, 1, -1}, kDy[8] = {0, 0, 1, -1, 1, -1, -1, 1};
    hipStream_t s = (hipStream_t)stream;
    const int npix = h * w;
    const int tiles_p = (npix + kSgmTile - 1) / kSgmTile, tiles_d = (nd + kSgmTile - 1) / kSgmTile;
    const unsigned grid = (unsigned)((int64_t)nk * tiles_p * tiles_d);
    int32_t *ct = static_cast<int32_t *>(scratch), *st = ct + (int64_t)nk * nd * npix;
    k_sgm_transpose<true><<<grid, kSgmThreads, 0, s>>>(static_cast<const int32_t *>(volume), ct, st, nd, npix, tiles_p, tiles_d);
    if (int rc = launch_status()) return rc;
    SgmPathArgs a = {};
    a.c = ct, a.s = st, a.nd = nd, a.h = h, a.w = w, a.nk = nk, a.p1 = p1, a.p2 = p2;
    int n = 0;
    for (int j = 0; j < 8; ++j)
        if (directions >> j & 1) a.directions |= (uint32_t)((kDx[j] + 1) | (kDy[j] + 1) << 2) << (4 * n++);
    sgm_path(a, n, s);
    if (int rc = launch_status()) return rc;
    k_sgm_transpose<false><<<grid, kSgmThreads, 0, s>>>(st, static_cast<int32_t *>(out), nullptr, nd, npix, tiles_p, tiles_d);
    return launch_status();
}

extern "C" int evk_sgm_match_volume(const void *volume, const void *activity, int nk, int nc, int nd, int h, int w, int d_min,
                                    int min_activity, int uniqueness, int64_t max_cost, int lr_tolerance, int subpixel, void *scratch,
                                    float *disparity, void *index, void *cost, void *mask, void *stream) {
    if (!volume || !activity || !sgm_sizes_ok(nk, nd, h, w) || nc < 1 || nc > 2 || d_min < 0 || d_min > (1 << 30)) return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    SgmMatchArgs p = {};
    p.volume = static_cast<const int32_t *>(volume), p.activity = static_cast<const uint8_t *>(activity);
    p.nc = nc, p.h = h, p.w = w, p.d_min = d_min, p.nd = nd, p.total = (int64_t)nk * h * w;
    return disparity_match(min_activity, uniqueness, max_cost, lr_tolerance, subpixel, scratch, disparity, index, cost, mask, p.total, s,
                           [&](const DisparityTests &t, const DisparityOut &o, bool right) {
                               p.tests = t, p.out = o;
                               if (right) k_sgm_right<<<stream_grid(p.total), EVK_BLOCK, 0, s>>>(p);
                               else k_sgm_winner<<<stream_grid(p.total), EVK_BLOCK, 0, s>>>(p);
                               return launch_status();
                           });
}
