// Event-based multi-view stereo (include/evk.h, "Event-based multi-view stereo"; EMVS, Rebecq et al., IJCV 2018): every event is
// back-projected as a ray through a disparity space image (DSI), a (D, H, W) volume of depth planes in front of a reference
// view, the rays through each cell are counted, and depth is read off the maxima of the volume.
//
//   k_emvs_packet_times  the time of packet j: ts of its middle event (n / packet_size doubles, read back by the caller, who
//                        turns them into the packet table on the host)
//   k_emvs_rays          once per event: d = M (x, y, 1) with the packet's M, (a, b) = (d0 / d2, d1 / d2), NaN unless d2 > 0
//   k_emvs_votes         grid = (planes x tiles, event chunks): a workgroup owns one plane, one tile of it -- a band of rows, cut
//                        in columns only when one row is wider than the LDS -- and one chunk of the events; the tile is uint32
//                        cells in LDS, every vote one LDS integer add, and the non-zero cells are flushed with global integer adds
//   k_emvs_peak / _mask / _median   the depth map: one lane per pixel, loads coalesced along x, integer arithmetic only
//
// Cells are integers: adds commute, so a DSI is the same bits whatever order the votes land in and however the events are cut
// into chunks and the planes into tiles.  Every float64 operation is one IEEE rounding (-ffp-contract=off, no fast-math), in the
// order of the definition.  A NaN or an infinity fails every range test below and votes nowhere; an index is formed only from a
// double that passed its range test.
#include "evk_common.h"

namespace evk {

constexpr int kEmvsThreads = 1024;
constexpr int kEmvsUnroll = 4;                          // events per lane and trip of the vote loop
constexpr int kEmvsCells = 40000;                       // uint32 cells of a tile: 160 000 of the CU's 163 840 LDS bytes
constexpr int kEmvsMaxRadius = 16;
constexpr int64_t kEmvsMaxEvents = (int64_t)1 << 31;    // a nearest cell holds every event
constexpr int64_t kEmvsMaxEventsBilinear = EVK_EMVS_BILINEAR_MAX_EVENTS;      // 256 units each
constexpr int64_t kEmvsMinChunk = 16384;                // events: below that the tile's flush, not the events, is the work
constexpr int64_t kEmvsTargetGroups = 4 * EVK_NUM_CU;   // workgroups per launch the chunk count aims at

// i / d for 0 <= i < 2^31 and 1 <= d <= 2^31 as one 64-bit multiply and a shift: with l = ceil(log2 d) and m = ceil(2^(31 + l) / d)
// (m < 2^32), e = m d - 2^(31 + l) < d <= 2^l, so i e < 2^(31 + l) and floor(i m / 2^(31 + l)) = floor(i / d).
struct PacketDiv {
    uint32_t m;
    int shift;
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (uint32_t)(((uint64_t)i * m) >> shift); }
};
static inline PacketDiv packet_div(int64_t d) {
    const int l = d <= 1 ? 0 : 64 - __builtin_clzll((unsigned long long)(d - 1));
    const uint64_t p = (uint64_t)1 << (31 + l);
    return {(uint32_t)((p + (uint64_t)d - 1) / (uint64_t)d), 31 + l};
}

// The tiles of a plane: bands of `rows` rows; `cols` < w only when one row has more cells than the LDS.  Bands and columns are
// evened out, so that the last tile is not a sliver.
struct EmvsTiles {
    int rows, cols, row_bands, col_tiles;
};
static inline EmvsTiles emvs_tiles(int h, int w) {
    EmvsTiles g;
    g.col_tiles = (w + kEmvsCells - 1) / kEmvsCells;
    g.cols = (w + g.col_tiles - 1) / g.col_tiles;
    const int most = kEmvsCells / g.cols;
    g.row_bands = (h + most - 1) / most;
    g.rows = (h + g.row_bands - 1) / g.row_bands;
    g.row_bands = (h + g.rows - 1) / g.rows;
    return g;
}

template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_emvs_packet_times(const T *__restrict__ ts, int64_t n, int64_t packet_size,
                                                                 int64_t n_packets, double *__restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_packets; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t start = j * packet_size, cnt = min(packet_size, n - start);
        out[j] = (double)ts[start + cnt / 2];
    }
}

template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_emvs_rays(const T *__restrict__ xs, const T *__restrict__ ys, int64_t n, PacketDiv pd,
                                                         const double *__restrict__ packets, double2 *__restrict__ rays) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = (double)xs[i], y = (double)ys[i];
        const double *M = packets + 12 * (int64_t)pd((uint32_t)i);
        const double d0 = (M[0] * x + M[1] * y) + M[2];
        const double d1 = (M[3] * x + M[4] * y) + M[5];
        const double d2 = (M[6] * x + M[7] * y) + M[8];
        const double nan = __builtin_nan("");
        rays[i] = d2 > 0.0 ? make_double2(d0 / d2, d1 / d2) : make_double2(nan, nan);      // (a NaN ray votes nowhere)
    }
}

__device__ __forceinline__ void lds_vote(uint32_t *cell, uint32_t q) {
    __hip_atomic_fetch_add(cell, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One tile of one plane: its place in the plane and in LDS.
struct EmvsTile {
    int x0, y0, tw, th;
    double xlo, xhi, ylo, yhi;
};

// The vote of one ray (a, b) with the packet's camera centre C into the tile (the definition of include/evk.h from "plane" on).
template <bool BILINEAR>
__device__ __forceinline__ void emvs_vote(uint32_t *cells, const EmvsTile &t, double a, double b, double C0, double C1, double C2,
                                          double Z, double rZ, double fx, double fy, double cx, double cy) {
    const double s = Z - C2;
    if (!(s > 0.0)) return;                                             // the plane lies behind this packet's camera centre
    const double v = (fy * (C1 + s * b)) * rZ + cy;
    const double u = (fx * (C0 + s * a)) * rZ + cx;
    if constexpr (!BILINEAR) {
        const double rv = floor(v + 0.5), ru = floor(u + 0.5);
        if (!(rv >= t.ylo && rv < t.yhi && ru >= t.xlo && ru < t.xhi)) return;
        lds_vote(&cells[((int)rv - t.y0) * t.tw + ((int)ru - t.x0)], 1u);
    } else {
        const double fv0 = floor(v), fu0 = floor(u);
        if (!(fv0 >= t.ylo - 1.0 && fv0 < t.yhi && fu0 >= t.xlo - 1.0 && fu0 < t.xhi)) return;      // no corner in this tile
        const double fu = u - fu0, fv = v - fv0;
        const double gu = 1.0 - fu, gv = 1.0 - fv;
        const int ix = (int)fu0 - t.x0, iy = (int)fv0 - t.y0;           // -1 .. : the corner's place in the tile
        const bool l = ix >= 0, r = ix + 1 < t.tw, top = iy >= 0, bot = iy + 1 < t.th;
        const uint32_t q00 = (uint32_t)rint((gu * gv) * 256.0), q10 = (uint32_t)rint((fu * gv) * 256.0);
        const uint32_t q01 = (uint32_t)rint((gu * fv) * 256.0), q11 = (uint32_t)rint((fu * fv) * 256.0);
        const int o = iy * t.tw + ix;                                   // (used only for a corner inside the tile)
        if (l && top && q00) lds_vote(&cells[o], q00);
        if (r && top && q10) lds_vote(&cells[o + 1], q10);
        if (l && bot && q01) lds_vote(&cells[o + t.tw], q01);
        if (r && bot && q11) lds_vote(&cells[o + t.tw + 1], q11);
    }
}

template <bool BILINEAR>
__global__ void __launch_bounds__(kEmvsThreads) k_emvs_votes(const double2 *__restrict__ rays, int64_t n, int64_t chunk, PacketDiv pd,
                                                             const double *__restrict__ packets, const double *__restrict__ depths,
                                                             const double *__restrict__ inv_depths, double fx, double fy, double cx,
                                                             double cy, int h, int w, EmvsTiles g, uint32_t *__restrict__ raw) {
    extern __shared__ uint32_t cells[];
    const int tiles = g.row_bands * g.col_tiles;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int tr = tile / g.col_tiles, tc = tile - tr * g.col_tiles;
    const int y0 = tr * g.rows, y1 = min(y0 + g.rows, h), x0 = tc * g.cols, x1 = min(x0 + g.cols, w);
    const int tw = x1 - x0, ncell = (y1 - y0) * tw;                     // <= rows * cols <= kEmvsCells
    const EmvsTile t = {x0, y0, tw, y1 - y0, (double)x0, (double)x1, (double)y0, (double)y1};
    for (int i = threadIdx.x; i < ncell; i += blockDim.x) cells[i] = 0u;
    __syncthreads();
    const double Z = depths[plane], rZ = inv_depths[plane];
    const int64_t c0 = (int64_t)blockIdx.y * chunk, c1 = min(c0 + chunk, n);
    // kEmvsUnroll events per lane and trip, every load of the trip issued before the first vote: the loads are what a trip waits for
    for (int64_t base = c0 + threadIdx.x; base < c1; base += (int64_t)kEmvsUnroll * kEmvsThreads) {
        double2 ab[kEmvsUnroll];
        double C[kEmvsUnroll][3];
#pragma unroll
        for (int k = 0; k < kEmvsUnroll; ++k) {
            const int64_t i = min(base + (int64_t)k * kEmvsThreads, c1 - 1);       // (past the end: the last event again, not voted)
            ab[k] = rays[i];
            const double *Cj = packets + 12 * (int64_t)pd((uint32_t)i) + 9;
            C[k][0] = Cj[0], C[k][1] = Cj[1], C[k][2] = Cj[2];
        }
#pragma unroll
        for (int k = 0; k < kEmvsUnroll; ++k)
            if (base + (int64_t)k * kEmvsThreads < c1)
                emvs_vote<BILINEAR>(cells, t, ab[k].x, ab[k].y, C[k][0], C[k][1], C[k][2], Z, rZ, fx, fy, cx, cy);
    }
    __syncthreads();
    uint32_t *dst = raw + (int64_t)plane * h * w + (int64_t)y0 * w + x0;
    for (int i = threadIdx.x; i < ncell; i += blockDim.x) {
        const uint32_t q = cells[i];
        if (!q) continue;
        const int row = i / tw;
        __hip_atomic_fetch_add(dst + (int64_t)row * w + (i - row * tw), q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// conf = max_i raw[i], index = the smallest i that attains it, -1 where conf == 0
__global__ void __launch_bounds__(EVK_BLOCK) k_emvs_peak(const uint32_t *__restrict__ raw, int nd, int64_t npix,
                                                         uint32_t *__restrict__ conf, int32_t *__restrict__ peak) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
        uint32_t best = 0u;
        int32_t at = -1;
        for (int i = 0; i < nd; ++i) {
            const uint32_t v = raw[(int64_t)i * npix + q];
            if (v > best) best = v, at = i;
        }
        conf[q] = best;
        peak[q] = at;
    }
}

// mask = conf area - S > threshold area, S the sum of conf over the (2 r + 1)^2 window (zero outside), area = (2 r + 1)^2 always
__global__ void __launch_bounds__(EVK_BLOCK) k_emvs_mask(const uint32_t *__restrict__ conf, int h, int w, int radius, int64_t threshold,
                                                         uint8_t *__restrict__ mask) {
    const int64_t npix = (int64_t)h * w, area = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(q / w), x = (int)(q - (int64_t)y * w);
        int64_t S = 0;
        for (int yy = max(y - radius, 0); yy <= min(y + radius, h - 1); ++yy)
            for (int xx = max(x - radius, 0); xx <= min(x + radius, w - 1); ++xx) S += (int64_t)conf[(int64_t)yy * w + xx];
        mask[q] = (int64_t)conf[q] * area - S > threshold * area;
    }
}

// K = 0: the peak as it is.  K = 3, 5: the lower median (element (k - 1) / 2 of the k sorted values) of the peaks of the masked
// pixels of the K x K window, found by rank: the value with at most (k - 1) / 2 values below it and more than that at or below it.
template <int K>
__global__ void __launch_bounds__(EVK_BLOCK) k_emvs_median(const int32_t *__restrict__ peak, const uint8_t *__restrict__ mask, int h, int w,
                                                           const double *__restrict__ depths, int32_t *__restrict__ index,
                                                           double *__restrict__ depth) {
    const int64_t npix = (int64_t)h * w;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (int64_t)gridDim.x * blockDim.x) {
        int32_t out = -1;
        if (mask[q]) {
            out = peak[q];
            if constexpr (K > 0) {
                constexpr int R = K / 2;
                const int y = (int)(q / w), x = (int)(q - (int64_t)y * w);
                int32_t vals[K * K];                                   // -1: not in the window or not masked (a peak is >= 0 here)
                int k = 0;
#pragma unroll
                for (int dy = -R; dy <= R; ++dy)
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w && mask[(int64_t)yy * w + xx];
                        vals[(dy + R) * K + dx + R] = in ? peak[(int64_t)yy * w + xx] : -1;
                        k += in;
                    }
                const int m = (k - 1) / 2;
#pragma unroll
                for (int a = 0; a < K * K; ++a) {
                    int below = 0, upto = 0;
#pragma unroll
                    for (int b = 0; b < K * K; ++b) {
                        below += vals[b] >= 0 && vals[b] < vals[a];
                        upto += vals[b] >= 0 && vals[b] <= vals[a];
                    }
                    if (vals[a] >= 0 && below <= m && m < upto) out = vals[a];
                }
            }
        }
        index[q] = out;
        depth[q] = out >= 0 ? depths[out] : __builtin_nan("");
    }
}

static inline bool emvs_finite(double v) { return v - v == 0.0; }

static inline bool emvs_volume_ok(int nd, int h, int w) {
    return nd >= 1 && h >= 1 && w >= 1 && (int64_t)h * w <= 0x7FFFFFFFll && (int64_t)h * w * nd <= ((int64_t)1 << 40);
}

// the packets of n events: packet_size is clamped to max(n, 1), so that a packet_size beyond the stream is one packet
static inline int64_t emvs_packet(int64_t n, int64_t packet_size) { return packet_size < n ? packet_size : (n > 1 ? n : 1); }

}  // namespace evk

using namespace evk;

extern "C" int evk_emvs_packet_times(int t_kind, const void *ts, int64_t n, int64_t packet_size, double *packet_ts, void *stream) {
    if ((t_kind != EVK_T_F32 && t_kind != EVK_T_F64) || n < 0 || n >= kEmvsMaxEvents || packet_size < 1 || (n > 0 && (!ts || !packet_ts)))
        return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    const int64_t ps = emvs_packet(n, packet_size), np = (n + ps - 1) / ps;
    hipStream_t s = (hipStream_t)stream;
    if (t_kind == EVK_T_F32)
        k_emvs_packet_times<float><<<stream_grid(np), EVK_BLOCK, 0, s>>>((const float *)ts, n, ps, np, packet_ts);
    else
        k_emvs_packet_times<double><<<stream_grid(np), EVK_BLOCK, 0, s>>>((const double *)ts, n, ps, np, packet_ts);
    return launch_status();
}

extern "C" int evk_emvs_band_rows(int h, int w) {
    if (h < 1 || w < 1 || (int64_t)h * w > 0x7FFFFFFFll) return EVK_EINVAL;
    return emvs_tiles(h, w).rows;
}

extern "C" int evk_emvs_band_cols(int h, int w) {
    if (h < 1 || w < 1 || (int64_t)h * w > 0x7FFFFFFFll) return EVK_EINVAL;
    return emvs_tiles(h, w).cols;
}

extern "C" int evk_emvs_chunks(int64_t n, int nd, int h, int w) {
    if (n < 0 || n >= kEmvsMaxEvents || !emvs_volume_ok(nd, h, w)) return EVK_EINVAL;
    const EmvsTiles g = emvs_tiles(h, w);
    const int64_t groups = (int64_t)nd * g.row_bands * g.col_tiles;
    int64_t chunks = (kEmvsTargetGroups + groups - 1) / groups;
    const int64_t most = (n + kEmvsMinChunk - 1) / kEmvsMinChunk;
    if (chunks > most) chunks = most;
    return (int)(chunks < 1 ? 1 : chunks);
}

extern "C" int evk_emvs_votes(int xy_kind, const void *xs, const void *ys, int64_t n, int64_t packet_size, const double *packets,
                              int64_t n_packets, const double *depths, const double *inv_depths, int nd, double fx, double fy,
                              double cx, double cy, int h, int w, int mode, int chunks, double *rays, void *raw, void *stream) {
    if ((xy_kind != EVK_T_F32 && xy_kind != EVK_T_F64) || (mode != EVK_EMVS_NEAREST && mode != EVK_EMVS_BILINEAR) || n < 0 ||
        n >= kEmvsMaxEvents || (mode == EVK_EMVS_BILINEAR && n >= kEmvsMaxEventsBilinear) || packet_size < 1 ||
        !emvs_volume_ok(nd, h, w) || !depths || !inv_depths || !raw || !(fx > 0.0) || !(fy > 0.0) || !emvs_finite(fx) ||
        !emvs_finite(fy) || !emvs_finite(cx) || !emvs_finite(cy) || chunks < 0 || chunks > 65535)
        return EVK_EINVAL;
    const int64_t ps = emvs_packet(n, packet_size);
    if (n > 0 && (!xs || !ys || !packets || !rays || n_packets != (n + ps - 1) / ps)) return EVK_EINVAL;
    const EmvsTiles g = emvs_tiles(h, w);
    const int64_t groups = (int64_t)nd * g.row_bands * g.col_tiles;
    if (groups > 0x7FFFFFFFll) return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(raw, 0, (size_t)nd * h * w * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return EVK_OK;
    const PacketDiv pd = packet_div(ps);
    double2 *ab = reinterpret_cast<double2 *>(rays);
    if (xy_kind == EVK_T_F32)
        k_emvs_rays<float><<<stream_grid(n), EVK_BLOCK, 0, s>>>((const float *)xs, (const float *)ys, n, pd, packets, ab);
    else
        k_emvs_rays<double><<<stream_grid(n), EVK_BLOCK, 0, s>>>((const double *)xs, (const double *)ys, n, pd, packets, ab);
    if (int rc = launch_status()) return rc;
    int64_t nchunks = chunks ? chunks : evk_emvs_chunks(n, nd, h, w);
    if (nchunks > n) nchunks = n;
    const int64_t chunk = (n + nchunks - 1) / nchunks;
    nchunks = (n + chunk - 1) / chunk;
    const size_t lds = (size_t)g.rows * g.cols * sizeof(uint32_t);
    const dim3 grid((unsigned)groups, (unsigned)nchunks);
    uint32_t *out = static_cast<uint32_t *>(raw);
    if (mode == EVK_EMVS_BILINEAR) {
        (void)hipFuncSetAttribute((const void *)k_emvs_votes<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kEmvsCells * sizeof(uint32_t)));
        k_emvs_votes<true><<<grid, kEmvsThreads, lds, s>>>(ab, n, chunk, pd, packets, depths, inv_depths, fx, fy, cx, cy, h, w, g, out);
    } else {
        (void)hipFuncSetAttribute((const void *)k_emvs_votes<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kEmvsCells * sizeof(uint32_t)));
        k_emvs_votes<false><<<grid, kEmvsThreads, lds, s>>>(ab, n, chunk, pd, packets, depths, inv_depths, fx, fy, cx, cy, h, w, g, out);
    }
    return launch_status();
}

extern "C" int evk_emvs_depth_map(const void *raw, const double *depths, int nd, int h, int w, int radius, int64_t threshold,
                                  int median_size, void *confidence, void *peak, void *mask, void *index, double *depth, void *stream) {
    if (!raw || !depths || !emvs_volume_ok(nd, h, w) || radius < 0 || radius > kEmvsMaxRadius || threshold < 0 ||
        threshold > ((int64_t)1 << 45) || (median_size != 0 && median_size != 3 && median_size != 5) || !confidence || !peak || !mask ||
        !index || !depth)
        return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t npix = (int64_t)h * w;
    const int grid = stream_grid(npix);
    uint32_t *conf = static_cast<uint32_t *>(confidence);
    int32_t *pk = static_cast<int32_t *>(peak), *idx = static_cast<int32_t *>(index);
    uint8_t *mk = static_cast<uint8_t *>(mask);
    k_emvs_peak<<<grid, EVK_BLOCK, 0, s>>>(static_cast<const uint32_t *>(raw), nd, npix, conf, pk);
    k_emvs_mask<<<grid, EVK_BLOCK, 0, s>>>(conf, h, w, radius, threshold, mk);
    if (median_size == 3)
        k_emvs_median<3><<<grid, EVK_BLOCK, 0, s>>>(pk, mk, h, w, depths, idx, depth);
    else if (median_size == 5)
        k_emvs_median<5><<<grid, EVK_BLOCK, 0, s>>>(pk, mk, h, w, depths, idx, depth);
    else
        k_emvs_median<0><<<grid, EVK_BLOCK, 0, s>>>(pk, mk, h, w, depths, idx, depth);
    return launch_status();
}
