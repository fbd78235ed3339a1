// Event stereo (include/evk.h, "Event stereo"): disparity by block matching on time surfaces quantised to 8 bits, the mapping step of
// ESVO (Zhou et al., T-RO 2021) on two rectified, time-synchronised event cameras.
//
//   k_stereo_quantise   ages to bytes, one lane per element
//   k_stereo_scan<NW, MODE>   the cost loop.  A workgroup owns a tile of 64 x 8 pixels of one query; the left rows of the tile
//                       (2 r wider and taller) and the right rows (nd - 1 wider still) are bytes in LDS, zero off the sensor.  The
//                       pixels of the tile that have work are listed in row-major order (ballot and rank, no atomics), a lane takes
//                       a listed pixel and walks the disparities eight at a time: per window row it reads the row's dwords, shifts
//                       them to its own byte with v_alignbyte_b32, and forms every |a - b| row sum with v_sad_u8, four pixels an
//                       instruction; the bytes past the window in the last dword are masked.
//                       MODE 0 writes the cost volume; MODE 1 keeps the winner of a candidate pixel and applies the integer
//                       tests (evk_disparity.h: the accumulator on 32-bit keys, the decision, the outputs); MODE 2 is the same
//                       loop on the mirrored pair (right image as the reference) and keeps only the winner, at the right pixels
//                       that a surviving candidate of MODE 1 pointed at.
//   k_disparity_lr      the left-right test (evk_disparity.h): one lane per pixel
//
// Every cost is an integer, so the sums are exact whatever their order: the direct sum over the window is the definition itself.
// No atomics anywhere; the only cross-lane traffic is the tile in LDS.
#include "evk_disparity.h"

namespace evk {

constexpr int kStereoTW = 64;                           // tile width: one wave per tile row
constexpr int kStereoTH = 8;                            // tile height: 256 threads, two rows each
constexpr int kStereoThreads = 256;
constexpr int kStereoChunk = 8;                         // disparities per trip of the cost loop
constexpr uint32_t kStereoNone = 0xFFFFFFFFu;           // no cost yet: a cost is below 2^17

enum { kStereoVolume = 0, kStereoMatch = 1, kStereoRight = 2 };

struct StereoArgs {
    const uint8_t *ql, *qr;
    int nc, h, w, d_min, nd, radius;
    int tiles_x, tiles_y;
    DisparityTests tests;
    int32_t *volume;
    DisparityOut out;
};

__host__ __device__ constexpr int stereo_words(int radius) { return (2 * radius + 1 + 3) / 4; }      // dwords of a window row
__host__ __device__ inline int stereo_padded(int nd) { return (nd + kStereoChunk - 1) / kStereoChunk * kStereoChunk; }
__host__ __device__ inline int stereo_left_words(int nw) { return kStereoTW / 4 + nw; }              // dwords of a left tile row
__host__ __device__ inline int stereo_right_words(int nw, int dp) { return ((kStereoTW - kStereoChunk - 1 + dp) >> 2) + nw + 3; }

__global__ void __launch_bounds__(EVK_BLOCK) k_stereo_quantise(const double *__restrict__ ages, int64_t n, double tau,
                                                               uint8_t *__restrict__ q) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = 1.0 - ages[i] / tau;
        uint8_t out = 0;
        if (v > 0.0) {                                                  // (a NaN fails)
            const double f = floor(256.0 * v);
            out = f >= 255.0 ? (uint8_t)255 : (uint8_t)(int)f;
        }
        q[i] = out;
    }
}

// rows x words dwords per channel of `img` (nc x h x w bytes) from (gy0, gx0) on, zero off the sensor; `flip` reads column w - 1 - gx
__device__ __forceinline__ void stereo_fill(uint32_t *tile, const uint8_t *__restrict__ img, int nc, int h, int w, int rows, int words,
                                            int gy0, int gx0, bool flip) {
    const int total = nc * rows * words;
    for (int idx = threadIdx.x; idx < total; idx += kStereoThreads) {
        const int line = idx / words, cw = idx - line * words;
        const int c = line / rows, gy = gy0 + (line - c * rows);
        uint32_t v = 0u;
        if (gy >= 0 && gy < h) {
            const uint8_t *p = img + ((int64_t)c * h + gy) * w;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int gx = gx0 + 4 * cw + b;
                if (gx >= 0 && gx < w) v |= (uint32_t)p[flip ? w - 1 - gx : gx] << (8 * b);
            }
        }
        tile[idx] = v;
    }
}

// The costs of disparity steps 0 .. lim - 1 of the pixel at (lx, ly) of the tile, f(i, cost) in increasing i.  lt: left tile, row
// (c, ly + dy + r) holds columns x0 - r .. ; rt: right tile, column lx + dp - 1 - i + (dx + r) of a row holds the right pixel
// x + dx - (d_min + i).  tail: the mask of the window's bytes in its last dword.
template <int NW, class F>
__device__ __forceinline__ void stereo_scan(const uint32_t *lt, const uint32_t *rt, int nc, int trows, int win, int lx, int ly, int lim,
                                            int dp, uint32_t tail, F &&f) {
    const int lw = stereo_left_words(NW), rw = stereo_right_words(NW, dp);
    const int lq = lx >> 2, ls = lx & 3;
    for (int i0 = 0; i0 < lim; i0 += kStereoChunk) {
        uint32_t acc[kStereoChunk];
#pragma unroll
        for (int e = 0; e < kStereoChunk; ++e) acc[e] = 0u;
        const int b = lx + dp - kStereoChunk - i0;                      // the column of step i0 + 7, the leftmost of this trip
        const int bq = b >> 2, bs = b & 3;
        for (int c = 0; c < nc; ++c)
            for (int rr = 0; rr < win; ++rr) {
                const uint32_t *lrow = lt + (c * trows + ly + rr) * lw + lq;
                const uint32_t *rrow = rt + (c * trows + ly + rr) * rw + bq;
                uint32_t lraw[NW + 1], l[NW], rraw[NW + 3], a[NW + 2];
#pragma unroll
                for (int j = 0; j <= NW; ++j) lraw[j] = lrow[j];
#pragma unroll
                for (int j = 0; j < NW + 3; ++j) rraw[j] = rrow[j];
#pragma unroll
                for (int j = 0; j < NW; ++j) l[j] = __builtin_amdgcn_alignbyte(lraw[j + 1], lraw[j], ls);
                l[NW - 1] &= tail;
#pragma unroll
                for (int j = 0; j < NW + 2; ++j) a[j] = __builtin_amdgcn_alignbyte(rraw[j + 1], rraw[j], bs);
#pragma unroll
                for (int e = 0; e < kStereoChunk; ++e) {                // e bytes right of the base: step i0 + 7 - e
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        const int q = (e >> 2) + j;
                        uint32_t v = (e & 3) ? __builtin_amdgcn_alignbyte(a[q + 1], a[q], e & 3) : a[q];
                        if (j == NW - 1) v &= tail;
                        acc[kStereoChunk - 1 - e] = __builtin_amdgcn_sad_u8(l[j], v, acc[kStereoChunk - 1 - e]);
                    }
                }
            }
#pragma unroll
        for (int e = 0; e < kStereoChunk; ++e)
            if (i0 + e < lim) f(i0 + e, acc[e]);
    }
}

template <int NW, int MODE>
__global__ void __launch_bounds__(kStereoThreads) k_stereo_scan(StereoArgs p) {
    extern __shared__ uint32_t lds[];
    const int tiles = p.tiles_x * p.tiles_y;
    const int k = blockIdx.x / tiles, tile = blockIdx.x - k * tiles;
    const int tyi = tile / p.tiles_x, txi = tile - tyi * p.tiles_x;
    const int x0 = txi * kStereoTW, y0 = tyi * kStereoTH;
    const int h = p.h, w = p.w, r = p.radius, nd = p.nd, d_min = p.d_min;
    const int64_t npix = (int64_t)h * w;
    const uint8_t *ql = p.ql + (int64_t)k * p.nc * npix, *qr = p.qr + (int64_t)k * p.nc * npix;
    // MODE 2 walks the mirrored pair: column x of the tile is the right pixel w - 1 - x
    const auto column = [&](int x) { return MODE == kStereoRight ? w - 1 - x : x; };
    const auto steps = [&](int x) { return min(max(x - d_min + 1, 0), nd); };      // the admissible steps are 0 .. steps - 1 (x - d >= 0)

    // ---- the pixels of the tile that have work, in row-major order: wave j lists rows j and j + 4 by ballot and rank
    __shared__ uint16_t list[kStereoTW * kStereoTH];
    __shared__ int rows_n[kStereoTH];
    const int lane = threadIdx.x & (kStereoTW - 1), wave = threadIdx.x >> 6;
    int rank[2];
    bool active[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int x = x0 + lane, y = y0 + wave + 4 * s;
        const bool in = x < w && y < h;
        const int64_t q = (int64_t)k * npix + (int64_t)y * w + column(x);
        if constexpr (MODE == kStereoVolume) {
            active[s] = in;
        } else if constexpr (MODE == kStereoMatch) {
            int act = 0;
            if (in)
                for (int c = 0; c < p.nc; ++c) act = max(act, (int)ql[(int64_t)c * npix + (int64_t)y * w + x]);
            active[s] = in && steps(x) > 0 && act >= p.tests.min_activity;
            if (in && !active[s]) disparity_write_none(p.out, q);
        } else {
            active[s] = in && p.out.scratch[q] == kWanted;
        }
        const uint64_t votes = __ballot(active[s]);
        rank[s] = __popcll(votes & (((uint64_t)1 << lane) - 1));
        if (lane == 0) rows_n[wave + 4 * s] = __popcll(votes);
    }
    __syncthreads();
    int before[2] = {0, 0}, total = 0;
#pragma unroll
    for (int j = 0; j < kStereoTH; ++j) {
        if (j < wave) before[0] += rows_n[j];
        if (j < wave + 4) before[1] += rows_n[j];
        total += rows_n[j];
    }
    if (total == 0) return;                                             // (the same for every thread)
#pragma unroll
    for (int s = 0; s < 2; ++s)
        if (active[s]) list[before[s] + rank[s]] = (uint16_t)(((wave + 4 * s) << 6) | lane);

    const int dp = stereo_padded(nd), trows = kStereoTH + 2 * r, win = 2 * r + 1;
    const int lw = stereo_left_words(NW), rw = stereo_right_words(NW, dp);
    uint32_t *lt = lds, *rt = lds + p.nc * trows * lw;
    if constexpr (MODE == kStereoRight) {                              // the mirrored pair: the right image is the reference
        stereo_fill(lt, qr, p.nc, h, w, trows, lw, y0 - r, x0 - r, true);
        stereo_fill(rt, ql, p.nc, h, w, trows, rw, y0 - r, x0 - r - d_min - dp + 1, true);
    } else {
        stereo_fill(lt, ql, p.nc, h, w, trows, lw, y0 - r, x0 - r, false);
        stereo_fill(rt, qr, p.nc, h, w, trows, rw, y0 - r, x0 - r - d_min - dp + 1, false);
    }
    __syncthreads();
    const int nb = win - 4 * (NW - 1);                                  // 1 .. 4 bytes of the window in its last dword
    const uint32_t tail = nb == 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1u;

    // ---- a lane per listed pixel: idle pixels cost nothing, and a wave's lanes are still neighbours along a row
#pragma unroll 1
    for (int e = threadIdx.x; e < total; e += kStereoThreads) {
        const int lx = list[e] & (kStereoTW - 1), ly = list[e] >> 6;
        const int x = x0 + lx, y = y0 + ly, lim = steps(x);
        const int64_t q = (int64_t)k * npix + (int64_t)y * w + column(x);
        if constexpr (MODE == kStereoVolume) {
            int32_t *vol = p.volume + ((int64_t)k * nd) * npix + (int64_t)y * w + x;
            stereo_scan<NW>(lt, rt, p.nc, trows, win, lx, ly, lim, dp, tail,
                            [&](int i, uint32_t cost) { vol[(int64_t)i * npix] = (int32_t)cost; });
            for (int i = lim; i < nd; ++i) vol[(int64_t)i * npix] = -1;
        } else if constexpr (MODE == kStereoRight) {
            uint32_t best = kStereoNone;
            int at = 0;
            stereo_scan<NW>(lt, rt, p.nc, trows, win, lx, ly, lim, dp, tail, [&](int i, uint32_t cost) {
                if (cost < best) best = cost, at = i;
            });
            p.out.scratch[q] = d_min + at;
        } else {
            DisparityWinner<uint32_t, false> win4;                      // (a key is below 2^25; an inadmissible step is never walked)
            stereo_scan<NW>(lt, rt, p.nc, trows, win, lx, ly, lim, dp, tail, win4);
            disparity_write(p.out, q, disparity_decide(win4, d_min, p.tests), p.tests.lr);
        }
    }
}

static inline bool stereo_sizes_ok(int nk, int nc, int h, int w, int d_min, int nd, int radius) {
    if (nk < 1 || nc < 1 || nc > 2 || h < 1 || w < 1 || (int64_t)h * w > 0x7FFFFFFFll) return false;
    if (nd < 1 || nd > EVK_STEREO_MAX_DISPARITIES || d_min < 0 || d_min > (1 << 30) || radius < 1 || radius > EVK_STEREO_MAX_RADIUS)
        return false;
    if ((int64_t)nk * nd * h * w > ((int64_t)1 << 40)) return false;
    const int64_t groups = (int64_t)nk * ((w + kStereoTW - 1) / kStereoTW) * ((h + kStereoTH - 1) / kStereoTH);
    return groups <= 0x7FFFFFFFll;
}

template <int MODE>
static int stereo_launch(StereoArgs p, int nk, hipStream_t s) {
    p.tiles_x = (p.w + kStereoTW - 1) / kStereoTW, p.tiles_y = (p.h + kStereoTH - 1) / kStereoTH;
    const int nw = stereo_words(p.radius), dp = stereo_padded(p.nd);
    const size_t lds = (size_t)p.nc * (kStereoTH + 2 * p.radius) * (stereo_left_words(nw) + stereo_right_words(nw, dp)) * sizeof(uint32_t);
    const unsigned grid = (unsigned)((int64_t)nk * p.tiles_x * p.tiles_y);
    switch (nw) {                                                       // (at most 18 304 bytes of LDS: nc 2, radius 7, nd 256)
        case 1: k_stereo_scan<1, MODE><<<grid, kStereoThreads, lds, s>>>(p); break;
        case 2: k_stereo_scan<2, MODE><<<grid, kStereoThreads, lds, s>>>(p); break;
        case 3: k_stereo_scan<3, MODE><<<grid, kStereoThreads, lds, s>>>(p); break;
        default: k_stereo_scan<4, MODE><<<grid, kStereoThreads, lds, s>>>(p); break;
    }
    return launch_status();
}

}  // namespace evk

using namespace evk;

extern "C" int evk_stereo_quantise(const double *ages, int64_t n, double tau, void *q, void *stream) {
    if (n < 0 || !(tau > 0.0) || !(tau - tau == 0.0) || (n > 0 && (!ages || !q))) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    k_stereo_quantise<<<stream_grid(n), EVK_BLOCK, 0, (hipStream_t)stream>>>(ages, n, tau, static_cast<uint8_t *>(q));
    return launch_status();
}

extern "C" int evk_stereo_cost_volume(const void *ql, const void *qr, int nk, int nc, int h, int w, int d_min, int nd, int radius,
                                      void *volume, void *stream) {
    if (!ql || !qr || !volume || !stereo_sizes_ok(nk, nc, h, w, d_min, nd, radius)) return EVK_EINVAL;
    StereoArgs p = {};
    p.ql = static_cast<const uint8_t *>(ql), p.qr = static_cast<const uint8_t *>(qr);
    p.nc = nc, p.h = h, p.w = w, p.d_min = d_min, p.nd = nd, p.radius = radius;
    p.volume = static_cast<int32_t *>(volume);
    return stereo_launch<kStereoVolume>(p, nk, (hipStream_t)stream);
}

extern "C" int64_t evk_stereo_scratch_bytes(int nk, int h, int w, int lr_tolerance) {
    if (nk < 1 || h < 1 || w < 1 || (int64_t)h * w > 0x7FFFFFFFll || (int64_t)nk * h * w > ((int64_t)1 << 40)) return EVK_EINVAL;
    return lr_tolerance < 0 ? 0 : (int64_t)nk * h * w * (int64_t)sizeof(int32_t);
}

extern "C" int evk_stereo_match(const void *ql, const void *qr, int nk, int nc, int h, int w, int d_min, int nd, int radius,
                                int min_activity, int uniqueness, int64_t max_cost, int lr_tolerance, int subpixel, void *scratch,
                                float *disparity, void *index, void *cost, void *mask, void *stream) {
    if (!ql || !qr || !stereo_sizes_ok(nk, nc, h, w, d_min, nd, radius)) return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    StereoArgs p = {};
    p.ql = static_cast<const uint8_t *>(ql), p.qr = static_cast<const uint8_t *>(qr);
    p.nc = nc, p.h = h, p.w = w, p.d_min = d_min, p.nd = nd, p.radius = radius;
    return disparity_match(min_activity, uniqueness, max_cost, lr_tolerance, subpixel, scratch, disparity, index, cost, mask,
                           (int64_t)nk * h * w, s, [&](const DisparityTests &t, const DisparityOut &o, bool right) {
                               p.tests = t, p.out = o;
                               return right ? stereo_launch<kStereoRight>(p, nk, s) : stereo_launch<kStereoMatch>(p, nk, s);
                           });
}
