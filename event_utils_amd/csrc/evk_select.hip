// Event filters of lib/util/event_util.py on the device: an ORDER-PRESERVING stream compaction of the event columns under a
// per-event predicate (clip_events_to_bounds :61-94, get_events_from_mask :96-109, the removal step of remove_hot_pixels
// :166-187), and the hot-pixel selection of remove_hot_pixels as a radix select on the event image.
//
// Compaction = reduce, scan, write (three launches, no inter-workgroup hand-over: the result is independent of dispatch order
// and placement).  A chunk is 4096 events = 16 rounds of 256 consecutive events; k_sel_count counts each chunk's kept events,
// k_sel_scan turns the counts into output offsets, k_sel_write re-evaluates the predicate, ranks each kept event inside its
// chunk by wave ballots (round-major, wave-minor: stream order) and copies the payload columns.  Loads are per element, so a
// column that starts anywhere (a slice of a resident stream) is read in place.
#include <type_traits>

#include "evk_common.h"
#include "evk_philox.h"

namespace evk {

constexpr int SEL_ITEMS = 16;                         // rounds of EVK_BLOCK consecutive events per chunk
constexpr int64_t SEL_CHUNK = (int64_t)EVK_BLOCK * SEL_ITEMS;
constexpr int SEL_WAVES = EVK_BLOCK / EVK_WAVE;       // 4: SEL_ITEMS * SEL_WAVES = 64 = one wave scans the chunk's tallies
static_assert(SEL_ITEMS * SEL_WAVES == EVK_WAVE, "one wave scans the (round, wave) tallies of a chunk");
constexpr int SEL_MAX_COLS = 4;

typedef unsigned __int128 u128;

struct SelPred {
    double minx, maxx, miny, maxy;   // EVK_SELECT_BOX
    double thr;                      // EVK_SELECT_MASK
    const void *image;               // EVK_SELECT_NOT_HOT: uint8 (h, w) hot map; EVK_SELECT_MASK: float64 (h, w) mask;
                                     // EVK_SELECT_RANDOM: the HotState of evk_random_subset; EVK_SELECT_FLAGS: uint8 (n) flags
    int h, w;
    u128 key_thr;                    // EVK_SELECT_RANDOM (read from `image` by the kernel): keep subset_key >= key_thr
    uint64_t seed;
    uint32_t purpose, active;
    int64_t cap;                     // EVK_SELECT_RANDOM: k, the subset's size; no output position >= k is ever written
};

struct SelCols {
    const void *src[SEL_MAX_COLS];
    void *dst[SEL_MAX_COLS];
    int eb[SEL_MAX_COLS];
    int ncols, t_col;
    int64_t *index;                  // kept event indices (may be NULL)
    int64_t *result;                 // [count, raw first, raw last] of column t_col
};

// x.astype(int) truncates toward zero.  Every mask is narrower than 2^31 pixels, so an index outside int32 is out of range after
// its one wrap as well: NaN, +-inf and |x| >= 2^31 fail here (32-bit conversions instead of the slower 64-bit ones)
template <typename T>
__device__ __forceinline__ bool trunc_index(T v, int &out) {
    if constexpr (std::is_integral<T>::value) {
        if ((int64_t)v < INT32_MIN || (int64_t)v > INT32_MAX) return false;
    } else {
        if (!(v > (T)-2147483648.0 && v < (T)2147483648.0)) return false;
    }
    out = (int)v;
    return true;
}

// key of candidate i of a uniform subset (evk_random_subset): 64 Philox bits, then the 32-bit index, complemented, so that the k
// LARGEST of these keys (the hot-pixel select's order) are the k smallest of (bits, index): a uniform k-subset, all keys distinct
__device__ __forceinline__ u128 subset_key(uint64_t seed, uint32_t purpose, uint32_t i) {
    const Philox4 r = philox_at(seed, purpose, i);
    return ((u128)~words64(r.v[0], r.v[1]) << 32) | (u128)(uint32_t)~i;
}

template <typename T, int KIND, bool COUNT_OOB>
__device__ __forceinline__ bool sel_keep_xy(const SelPred &p, T x, T y, uint32_t *oob) {
    if constexpr (KIND == EVK_SELECT_BOX) {
        const double xd = (double)x, yd = (double)y;
        return p.minx <= xd && xd < p.maxx && p.miny <= yd && yd < p.maxy;
    } else if constexpr (KIND == EVK_SELECT_NOT_HOT) {
        const double xd = (double)x, yd = (double)y;
        if (!(xd >= 0.0 && xd < (double)p.w && yd >= 0.0 && yd < (double)p.h)) return true;   // x == W / y == H: never hot
        const int xi = (int)xd, yi = (int)yd;
        if ((double)xi != xd || (double)yi != yd) return true;                                 // not on a pixel
        return static_cast<const uint8_t *>(p.image)[(int64_t)yi * p.w + xi] == 0;
    } else {
        int xi, yi;
        bool ok = trunc_index(x, xi) && trunc_index(y, yi);
        if (ok) {                                     // numpy indexing: one wrap of a negative index, then a range check
            if (xi < 0) xi += p.w;
            if (yi < 0) yi += p.h;
            ok = xi >= 0 && xi < p.w && yi >= 0 && yi < p.h;
        }
        if (!ok) {
            if (COUNT_OOB) count_oob(oob);
            return false;
        }
        return static_cast<const double *>(p.image)[(int64_t)yi * p.w + xi] >= p.thr;
    }
}

template <typename T, int KIND, bool COUNT_OOB>
__device__ __forceinline__ bool sel_keep(const SelPred &p, const T *__restrict__ xs, const T *__restrict__ ys, int64_t j,
                                         uint32_t *oob) {
    if constexpr (KIND == EVK_SELECT_RANDOM) {
        return p.active && subset_key(p.seed, p.purpose, (uint32_t)j) >= p.key_thr;
    } else if constexpr (KIND == EVK_SELECT_FLAGS) {
        return static_cast<const uint8_t *>(p.image)[j] != 0;
    } else {
        return sel_keep_xy<T, KIND, COUNT_OOB>(p, xs[j], ys[j], oob);
    }
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

template <typename T, int KIND>
__device__ __forceinline__ void sel_count(const T *__restrict__ x, const T *__restrict__ y, int64_t n, const SelPred &p,
                                          uint32_t *__restrict__ counts, uint32_t *__restrict__ oob) {
    __shared__ uint32_t s_w[SEL_WAVES];
    const int64_t base = (int64_t)blockIdx.x * SEL_CHUNK + threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (int it = 0; it < SEL_ITEMS; ++it) {
        const int64_t j = base + (int64_t)it * EVK_BLOCK;
        if (j < n) c += sel_keep<T, KIND, true>(p, x, y, j, oob) ? 1u : 0u;
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) t += s_w[w];
        counts[blockIdx.x] = t;
    }
}

template <typename T, int KIND>
__global__ void __launch_bounds__(EVK_BLOCK) k_sel_count(const T *__restrict__ x, const T *__restrict__ y, int64_t n, SelPred p,
                                                       uint32_t *__restrict__ counts, uint32_t *__restrict__ oob) {
    sel_count<T, KIND>(x, y, n, p, counts, oob);
}

// one workgroup: offsets[c] = kept events of the chunks before c, offsets[nchunks] = result[0] = all kept events
constexpr int SCAN_THREADS = 1024;
__global__ void __launch_bounds__(SCAN_THREADS) k_sel_scan(const uint32_t *__restrict__ counts, int64_t nchunks,
                                                          int64_t *__restrict__ offsets, int64_t *__restrict__ result) {
    __shared__ int64_t s_w[SCAN_THREADS / EVK_WAVE];
    const int64_t per = (nchunks + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < nchunks ? lo + per : nchunks;
    int64_t s = 0;
    for (int64_t c = lo; c < hi; ++c) s += counts[c];
    const int64_t incl = wave_inclusive_scan(s);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    int64_t before = 0, total = 0;
    for (int w = 0; w < SCAN_THREADS / EVK_WAVE; ++w) {
        before += w < wave ? s_w[w] : 0;
        total += s_w[w];
    }
    int64_t run = before + incl - s;
    for (int64_t c = lo; c < hi; ++c) {
        offsets[c] = run;
        run += counts[c];
    }
    if (threadIdx.x == 0) {
        offsets[nchunks] = total;
        result[0] = total;
    }
}

// one payload column of the chunk: the kept elements of all rounds are loaded first, then stored (16 loads in flight per lane)
template <typename U>
__device__ __forceinline__ void copy_column(const U *__restrict__ src, U *__restrict__ dst, const uint64_t *ball,
                                            const int64_t *pos, int64_t base) {
    const int lane = threadIdx.x & 63;
    U v[SEL_ITEMS];
#pragma unroll
    for (int it = 0; it < SEL_ITEMS; ++it)
        if ((ball[it] >> lane) & 1ull) v[it] = src[base + (int64_t)it * EVK_BLOCK];
#pragma unroll
    for (int it = 0; it < SEL_ITEMS; ++it)
        if ((ball[it] >> lane) & 1ull) dst[pos[it]] = v[it];
}

__device__ __forceinline__ int64_t raw_elem(const void *src, int eb, int64_t j) {
    switch (eb) {
        case 1: return static_cast<const uint8_t *>(src)[j];
        case 2: return static_cast<const uint16_t *>(src)[j];
        case 4: return static_cast<const uint32_t *>(src)[j];
        default: return (int64_t) static_cast<const uint64_t *>(src)[j];
    }
}

template <typename T, int KIND>
__device__ __forceinline__ void sel_write(const T *__restrict__ x, const T *__restrict__ y, int64_t n, const SelPred &p,
                                          const int64_t *__restrict__ offsets, const SelCols &c) {
    __shared__ uint32_t s_off[SEL_ITEMS * SEL_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SEL_CHUNK + threadIdx.x;
    uint64_t ball[SEL_ITEMS];
#pragma unroll
    for (int it = 0; it < SEL_ITEMS; ++it) {
        const int64_t j = base + (int64_t)it * EVK_BLOCK;
        const bool k = j < n && sel_keep<T, KIND, false>(p, x, y, j, nullptr);
        ball[it] = __ballot(k);
        if (lane == 0) s_off[it * SEL_WAVES + wave] = (uint32_t)__popcll(ball[it]);
    }
    __syncthreads();
    if (wave == 0) {                                  // (round, wave) tallies in stream order -> exclusive offsets
        const uint32_t v = s_off[lane];
        s_off[lane] = wave_inclusive_scan(v) - v;
    }
    __syncthreads();
    const int64_t out0 = offsets[blockIdx.x], total = offsets[gridDim.x];
    const uint64_t below = (1ull << lane) - 1ull;
    int64_t pos[SEL_ITEMS];
#pragma unroll
    for (int it = 0; it < SEL_ITEMS; ++it) pos[it] = out0 + s_off[it * SEL_WAVES + wave] + __popcll(ball[it] & below);
    if constexpr (KIND == EVK_SELECT_RANDOM) {        // the outputs hold k elements: a position past them is dropped
#pragma unroll
        for (int it = 0; it < SEL_ITEMS; ++it) ball[it] = __ballot(((ball[it] >> lane) & 1ull) && pos[it] < p.cap);
    }
    for (int k = 0; k < c.ncols; ++k) {
        switch (c.eb[k]) {
            case 1: copy_column(static_cast<const uint8_t *>(c.src[k]), static_cast<uint8_t *>(c.dst[k]), ball, pos, base); break;
            case 2: copy_column(static_cast<const uint16_t *>(c.src[k]), static_cast<uint16_t *>(c.dst[k]), ball, pos, base); break;
            case 4: copy_column(static_cast<const uint32_t *>(c.src[k]), static_cast<uint32_t *>(c.dst[k]), ball, pos, base); break;
            default: copy_column(static_cast<const uint64_t *>(c.src[k]), static_cast<uint64_t *>(c.dst[k]), ball, pos, base); break;
        }
    }
#pragma unroll
    for (int it = 0; it < SEL_ITEMS; ++it) {
        if (!((ball[it] >> lane) & 1ull)) continue;
        const int64_t j = base + (int64_t)it * EVK_BLOCK;
        if (c.index) c.index[pos[it]] = j;
        if (c.t_col >= 0) {
            if (pos[it] == 0) c.result[1] = raw_elem(c.src[c.t_col], c.eb[c.t_col], j);
            if (pos[it] == total - 1) c.result[2] = raw_elem(c.src[c.t_col], c.eb[c.t_col], j);
        }
    }
}

template <typename T, int KIND>
__global__ void __launch_bounds__(EVK_BLOCK) k_sel_write(const T *__restrict__ x, const T *__restrict__ y, int64_t n, SelPred p,
                                                       const int64_t *__restrict__ offsets, SelCols c) {
    sel_write<T, KIND>(x, y, n, p, offsets, c);
}

// ---- hot pixels: the pixels the reference's "argmax, set to 0" loop picks in num_hot rounds ------------------------------
// Key of a pixel: 96 bits, order-mapped value (NaN above +inf, -0 as +0) then the complement of its flat index, so that the
// reference's order (value descending, ties to the lower index) is the keys' descending order and every key is distinct.  Eight
// passes of 12-bit digits (k_hot_hist, k_hot_find) find the k-th largest key T; hot = key >= T, plus at most one extra pixel.
// The same select takes its keys from any source (ImageKeys, SubsetKeys): evk_random_subset finds the threshold of a uniform
// k-subset with it.  Once the bucket of T holds a single key, T is that key's prefix with zero digits below it (the same key
// set >= T) and the remaining passes return at once (`done`).
constexpr int HOT_BITS = 12, HOT_BINS = 1 << HOT_BITS, HOT_PASSES = 8;   // 8 x 12 = 96 key bits
constexpr uint32_t HOT_NONE = 0xFFFFFFFFu;

struct HotState {
    u128 prefix;                // the digits found so far
    uint32_t P;                 // pixels > 0 or NaN
    uint32_t min_nonneg;        // lowest flat index of a pixel that is not < 0
    uint32_t remaining;         // rank of T among the keys that share the prefix
    uint32_t active;            // k > 0
    uint32_t extra;             // the one extra pixel, HOT_NONE if there is none
    uint32_t done;              // the bucket of T holds one key: T is final
    uint64_t seed;              // SubsetKeys: the Philox key and purpose of the subset keys
    uint32_t purpose;
    int64_t k;                  // the number of keys selected
};
constexpr int64_t HOT_HIST_OFFSET = 256;
constexpr int64_t HOT_SCRATCH = HOT_HIST_OFFSET + (int64_t)HOT_PASSES * HOT_BINS * 4;

// EVK_SELECT_RANDOM: the same count and write, the subset's seed and threshold read from the select's state in device memory
__device__ __forceinline__ SelPred subset_pred(const SelPred &p) {
    const HotState *st = static_cast<const HotState *>(p.image);
    SelPred q = p;
    q.key_thr = st->prefix;
    q.seed = st->seed;
    q.purpose = st->purpose;
    q.active = st->active;
    q.cap = st->k;
    return q;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_subset_count(int64_t n, SelPred p, uint32_t *__restrict__ counts) {
    const SelPred q = subset_pred(p);
    sel_count<int64_t, EVK_SELECT_RANDOM>(nullptr, nullptr, n, q, counts, nullptr);
}

__global__ void __launch_bounds__(EVK_BLOCK) k_subset_write(int64_t n, SelPred p, const int64_t *__restrict__ offsets, SelCols c) {
    const SelPred q = subset_pred(p);
    sel_write<int64_t, EVK_SELECT_RANDOM>(nullptr, nullptr, n, q, offsets, c);
}

// coordinates -> int32 pixel columns for the event image: *bad |= 1 for a value that is not an integer (NaN included); an
// integer outside int32 becomes -1, which the image kernels reject as off the canvas (the reference's ValueError)
template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_sel_to_i32(const T *__restrict__ in, int64_t n, int32_t *__restrict__ out,
                                                        uint32_t *__restrict__ bad) {
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T v = in[i];
        int32_t o = -1;
        if constexpr (std::is_integral<T>::value) {
            if ((int64_t)v >= INT32_MIN && (int64_t)v <= INT32_MAX) o = (int32_t)v;
        } else {
            const double d = (double)v;
            if (!(d == trunc(d))) b = true;
            else if (d >= -2147483648.0 && d < 2147483648.0) o = (int32_t)d;
        }
        out[i] = o;
    }
    if (bad && __any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

template <typename V>
__device__ __forceinline__ u128 hot_key(V v, uint32_t idx) {
    double d = (double)v;
    uint64_t hi;
    if (d != d) {
        hi = ~0ull;
    } else {
        if (d == 0.0) d = 0.0;
        const uint64_t b = (uint64_t)__double_as_longlong(d);
        hi = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
    return ((u128)hi << 32) | (u128)(uint32_t)~idx;
}

// key sources of the select: the pixels of an event image (with the pass-0 statistics of the hot-pixel rule), the candidates of
// a uniform subset
template <typename V>
struct ImageKeys {
    static constexpr bool STATS = true;
    const V *img;
    int h, w, pitch;
    __device__ __forceinline__ uint32_t count() const { return (uint32_t)h * (uint32_t)w; }
    __device__ __forceinline__ V value(uint32_t i) const {
        const uint32_t r = i / (uint32_t)w, col = i - r * (uint32_t)w;
        return img[(int64_t)r * pitch + col];
    }
};

struct SubsetKeys {
    static constexpr bool STATS = false;
    uint64_t seed;
    uint32_t purpose, n;
    __device__ __forceinline__ uint32_t count() const { return n; }
    __device__ __forceinline__ u128 key(uint32_t i) const { return subset_key(seed, purpose, i); }
};

__global__ void __launch_bounds__(EVK_BLOCK) k_hot_init(HotState *st, uint32_t *hist, uint64_t seed, uint32_t purpose) {
    for (int i = threadIdx.x; i < HOT_PASSES * HOT_BINS; i += EVK_BLOCK) hist[i] = 0;
    if (threadIdx.x == 0) {
        st->prefix = 0;
        st->P = 0;
        st->min_nonneg = HOT_NONE;
        st->remaining = 0;
        st->active = 0;
        st->extra = HOT_NONE;
        st->done = 0;
        st->seed = seed;
        st->purpose = purpose;
        st->k = 0;
    }
}

template <typename Src>
__global__ void __launch_bounds__(EVK_BLOCK) k_hot_hist(Src src, int pass, HotState *__restrict__ st, uint32_t *__restrict__ hist) {
    __shared__ uint32_t lh[HOT_BINS];
    if (pass > 0 && (!st->active || st->done)) return;   // (uniform: every workgroup reads the same words)
    for (int b = threadIdx.x; b < HOT_BINS; b += EVK_BLOCK) lh[b] = 0;
    __syncthreads();
    const int shift = (HOT_PASSES - 1 - pass) * HOT_BITS;
    const u128 pre = pass > 0 ? (st->prefix >> (shift + HOT_BITS)) : (u128)0;
    const uint32_t npix = src.count();
    uint32_t P = 0, mn = HOT_NONE;
    // (a 64-bit walk: with up to 2^32 - 1 keys a 32-bit index would wrap past 2^32 on its last stride and never end)
    for (int64_t i64 = (int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x; i64 < (int64_t)npix; i64 += (int64_t)gridDim.x * EVK_BLOCK) {
        const uint32_t i = (uint32_t)i64;
        u128 key;
        if constexpr (Src::STATS) {
            const auto v = src.value(i);
            if (pass == 0) {
                P += (v > 0 || v != v) ? 1u : 0u;
                if (!(v < 0) && i < mn) mn = i;
            }
            key = hot_key(v, i);
        } else {
            key = src.key(i);
        }
        if ((key >> (shift + HOT_BITS)) == pre) atomicAdd(&lh[(uint32_t)(key >> shift) & (HOT_BINS - 1)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < HOT_BINS; b += EVK_BLOCK)
        if (lh[b]) atomicAdd(&hist[pass * HOT_BINS + b], lh[b]);
    if (Src::STATS && pass == 0) {
        P = wave_sum(P);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t o = __shfl_xor(mn, off, 64);
            mn = o < mn ? o : mn;
        }
        if ((threadIdx.x & 63) == 0) {
            if (P) atomicAdd(&st->P, P);
            if (mn != HOT_NONE) atomicMin(&st->min_nonneg, mn);
        }
    }
}

// one workgroup: (pass 0) k and the extra pixel from P, the lowest non-negative pixel and num_hot -- or k = num_hot itself when
// `direct` (a subset); then the digit of T
__global__ void __launch_bounds__(EVK_BLOCK) k_hot_find(int pass, int64_t num_hot, int direct, HotState *__restrict__ st,
                                                      const uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_rem, s_active;
    __shared__ uint32_t s_w[SEL_WAVES];
    if (threadIdx.x == 0) {
        if (pass == 0) {
            const int64_t P = st->P;
            const uint32_t mn = st->min_nonneg;
            int64_t k = 0;
            uint32_t extra = HOT_NONE;
            if (num_hot <= 0) {
            } else if (direct) {
                k = num_hot;
            } else if (num_hot <= P) {
                k = num_hot;
            } else if (P > 0) {
                k = P;
                extra = mn;              // every pick so far is 0 now: argmax is the lowest pixel that is 0
            } else if (mn != HOT_NONE) {
                extra = mn;              // nothing positive: the first zero pixel, over and over
            } else {
                k = 1;                   // all negative: the argmax of the image, then it is 0 and stays the maximum
            }
            st->remaining = (uint32_t)k;
            st->k = k;
            st->active = k > 0;
            st->extra = extra;
        }
        s_rem = st->remaining;
        s_active = st->active && !st->done;
    }
    __syncthreads();
    if (!s_active) return;
    const uint32_t rem = s_rem;
    // thread t owns bins [top - 16 t - 15, top - 16 t]: the digits in descending order
    constexpr int PER = HOT_BINS / EVK_BLOCK;
    uint32_t b[PER], s = 0;
    const uint32_t *hp = hist + pass * HOT_BINS + (HOT_BINS - PER * (threadIdx.x + 1));
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        b[q] = hp[PER - 1 - q];
        s += b[q];
    }
    const uint32_t incl = wave_inclusive_scan(s);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int q = 0; q < wave; ++q) before += s_w[q];
    uint32_t cum = before + incl - s;
    if (cum < rem && rem <= cum + s) {                // exactly one thread holds the digit of the rem-th largest key
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (rem <= cum + b[q]) {
                const uint32_t digit = HOT_BINS - 1 - (PER * threadIdx.x + q);
                const int shift = (HOT_PASSES - 1 - pass) * HOT_BITS;
                st->prefix |= (u128)digit << shift;
                st->remaining = rem - cum;
                if (b[q] == 1) st->done = 1;
                break;
            }
            cum += b[q];
        }
    }
}

template <typename V>
__global__ void __launch_bounds__(EVK_BLOCK) k_hot_mark(const V *__restrict__ img, int h, int w, int pitch,
                                                      const HotState *__restrict__ st, uint8_t *__restrict__ hot) {
    const bool active = st->active;
    const u128 T = st->prefix;   // (zero below the found digits when `done`: the same pixels >= T)
    const uint32_t extra = st->extra;
    const uint32_t npix = (uint32_t)h * (uint32_t)w;
    for (int64_t i64 = (int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x; i64 < (int64_t)npix; i64 += (int64_t)gridDim.x * EVK_BLOCK) {
        const uint32_t i = (uint32_t)i64;
        const uint32_t r = i / (uint32_t)w, col = i - r * (uint32_t)w;
        hot[i] = ((active && hot_key(img[(int64_t)r * pitch + col], i) >= T) || i == extra) ? 1 : 0;
    }
}

// the radix select of the k-th largest key of `src` (over n keys) into the HotState at the head of `scratch`
template <typename Src>
static void select_kth(const Src &src, int64_t n, int64_t num_hot, int direct, uint64_t seed, uint32_t purpose, void *scratch,
                       hipStream_t s) {
    HotState *st = static_cast<HotState *>(scratch);
    uint32_t *hist = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + HOT_HIST_OFFSET);
    const int grid = stream_grid(n, 4);
    k_hot_init<<<1, EVK_BLOCK, 0, s>>>(st, hist, seed, purpose);
    for (int pass = 0; pass < HOT_PASSES; ++pass) {
        k_hot_hist<Src><<<grid, EVK_BLOCK, 0, s>>>(src, pass, st, hist);
        k_hot_find<<<1, EVK_BLOCK, 0, s>>>(pass, num_hot, direct, st, hist);
    }
}

template <typename V>
static int hot_pixels(const V *img, int h, int w, int pitch, int64_t num_hot, uint8_t *hot, void *scratch, hipStream_t s) {
    const HotState *st = static_cast<const HotState *>(scratch);
    select_kth(ImageKeys<V>{img, h, w, pitch}, (int64_t)h * w, num_hot, 0, 0, 0, scratch, s);
    k_hot_mark<V><<<stream_grid((int64_t)h * w, 4), EVK_BLOCK, 0, s>>>(img, h, w, pitch, st, hot);
    return launch_status();
}

template <typename T, int KIND>
static void compact(const T *x, const T *y, int64_t n, const SelPred &p, const SelCols &c, uint32_t *counts, int64_t *offsets,
                    uint32_t *oob, hipStream_t s) {
    const int64_t nchunks = (n + SEL_CHUNK - 1) / SEL_CHUNK;
    if (nchunks) k_sel_count<T, KIND><<<(unsigned)nchunks, EVK_BLOCK, 0, s>>>(x, y, n, p, counts, oob);
    k_sel_scan<<<1, SCAN_THREADS, 0, s>>>(counts, nchunks, offsets, c.result);
    if (nchunks) k_sel_write<T, KIND><<<(unsigned)nchunks, EVK_BLOCK, 0, s>>>(x, y, n, p, offsets, c);
}

template <typename T>
static void compact_kind(int pred, const T *xt, const void *y, int64_t n, const SelPred &p, const SelCols &c, uint32_t *counts,
                         int64_t *offsets, uint32_t *oob, hipStream_t s) {
    const T *yt = static_cast<const T *>(y);
    if (pred == EVK_SELECT_BOX) compact<T, EVK_SELECT_BOX>(xt, yt, n, p, c, counts, offsets, oob, s);
    else if (pred == EVK_SELECT_NOT_HOT) compact<T, EVK_SELECT_NOT_HOT>(xt, yt, n, p, c, counts, offsets, oob, s);
    else compact<T, EVK_SELECT_MASK>(xt, yt, n, p, c, counts, offsets, oob, s);
}

static void compact_subset(int64_t n, const SelPred &p, const SelCols &c, uint32_t *counts, int64_t *offsets, hipStream_t s) {
    const int64_t nchunks = (n + SEL_CHUNK - 1) / SEL_CHUNK;
    if (nchunks) k_subset_count<<<(unsigned)nchunks, EVK_BLOCK, 0, s>>>(n, p, counts);
    k_sel_scan<<<1, SCAN_THREADS, 0, s>>>(counts, nchunks, offsets, c.result);
    if (nchunks) k_subset_write<<<(unsigned)nchunks, EVK_BLOCK, 0, s>>>(n, p, offsets, c);
}

// EVK_SELECT_FLAGS: the predicate is a byte per event, the coordinate columns are not read
__global__ void __launch_bounds__(EVK_BLOCK) k_flags_count(int64_t n, SelPred p, uint32_t *__restrict__ counts) {
    sel_count<int64_t, EVK_SELECT_FLAGS>(nullptr, nullptr, n, p, counts, nullptr);
}

__global__ void __launch_bounds__(EVK_BLOCK) k_flags_write(int64_t n, SelPred p, const int64_t *__restrict__ offsets, SelCols c) {
    sel_write<int64_t, EVK_SELECT_FLAGS>(nullptr, nullptr, n, p, offsets, c);
}

static void compact_flags(int64_t n, const SelPred &p, const SelCols &c, uint32_t *counts, int64_t *offsets, hipStream_t s) {
    const int64_t nchunks = (n + SEL_CHUNK - 1) / SEL_CHUNK;
    if (nchunks) k_flags_count<<<(unsigned)nchunks, EVK_BLOCK, 0, s>>>(n, p, counts);
    k_sel_scan<<<1, SCAN_THREADS, 0, s>>>(counts, nchunks, offsets, c.result);
    if (nchunks) k_flags_write<<<(unsigned)nchunks, EVK_BLOCK, 0, s>>>(n, p, offsets, c);
}

static int64_t select_chunks(int64_t n) { return (n + SEL_CHUNK - 1) / SEL_CHUNK; }

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_select_scratch_bytes(int64_t n) {
    if (n < 0) return EVK_EINVAL;
    const int64_t nc = select_chunks(n);
    return 256 + ((4 * nc + 255) / 256) * 256 + 8 * (nc + 1);
}

extern "C" int evk_select_compact(int pred, int coord_kind, const void *x, const void *y, int64_t n, const double *host_params,
                                  const void *image, int h, int w, int ncols, const void *const *host_src, void *const *host_dst,
                                  const int *host_elem_bytes, int t_col, int64_t *index_out, int64_t *result, void *scratch,
                                  int64_t scratch_bytes, uint32_t *oob, void *stream) {
    if (n < 0 || !result || !scratch || coord_kind < EVK_SELECT_I16 || coord_kind > EVK_SELECT_F64 || ncols < 0 ||
        ncols > SEL_MAX_COLS || (ncols > 0 && (!host_src || !host_dst || !host_elem_bytes)) || t_col >= ncols ||
        (ncols == 0 && !index_out) || (pred != EVK_SELECT_RANDOM && pred != EVK_SELECT_FLAGS && n > 0 && (!x || !y)) || (n >> 31) >= SEL_CHUNK)
        return EVK_EINVAL;
    SelPred p = {};
    if (pred == EVK_SELECT_RANDOM) {
        if (!image || n > (int64_t)HOT_NONE) return EVK_EINVAL;
        p.image = image;
    } else if (pred == EVK_SELECT_FLAGS) {
        if (n > 0 && !image) return EVK_EINVAL;
        p.image = image;
    } else if (pred == EVK_SELECT_BOX) {
        if (!host_params) return EVK_EINVAL;
        p.minx = host_params[0], p.maxx = host_params[1], p.miny = host_params[2], p.maxy = host_params[3];
    } else if (pred == EVK_SELECT_NOT_HOT || pred == EVK_SELECT_MASK) {
        if (!image || h <= 0 || w <= 0 || (pred == EVK_SELECT_MASK && !host_params)) return EVK_EINVAL;
        p.thr = pred == EVK_SELECT_MASK ? host_params[0] : 0.0;
        p.image = image, p.h = h, p.w = w;
    } else {
        return EVK_EINVAL;
    }
    SelCols c = {};
    c.ncols = ncols, c.t_col = t_col, c.index = index_out, c.result = result;
    for (int k = 0; k < ncols; ++k) {
        const int eb = host_elem_bytes[k];
        if ((eb != 1 && eb != 2 && eb != 4 && eb != 8) || (n > 0 && (!host_src[k] || !host_dst[k]))) return EVK_EINVAL;
        c.src[k] = host_src[k], c.dst[k] = host_dst[k], c.eb[k] = eb;
    }
    if (scratch_bytes < evk_select_scratch_bytes(n)) return EVK_ESCRATCH;
    const int64_t nc = select_chunks(n);
    uint32_t *counts = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + 256);
    int64_t *offsets = reinterpret_cast<int64_t *>(static_cast<char *>(scratch) + 256 + ((4 * nc + 255) / 256) * 256);
    hipStream_t s = (hipStream_t)stream;
    if (pred == EVK_SELECT_RANDOM) {
        compact_subset(n, p, c, counts, offsets, s);
        return launch_status();
    }
    if (pred == EVK_SELECT_FLAGS) {
        compact_flags(n, p, c, counts, offsets, s);
        return launch_status();
    }
    with_time_kind(coord_kind, x, [&](auto *xt) { compact_kind(pred, xt, y, n, p, c, counts, offsets, oob, s); });
    return launch_status();
}

extern "C" int evk_select_to_i32(int coord_kind, const void *in, int64_t n, int32_t *out, uint32_t *bad, void *stream) {
    if (n < 0 || (n > 0 && (!in || !out)) || coord_kind < EVK_SELECT_I16 || coord_kind > EVK_SELECT_F64) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int g = stream_grid(n);
    with_time_kind(coord_kind, in, [&](auto *col) { k_sel_to_i32<<<g, EVK_BLOCK, 0, s>>>(col, n, out, bad); });
    return launch_status();
}

extern "C" int64_t evk_hot_pixels_scratch_bytes(void) { return HOT_SCRATCH; }

extern "C" int evk_hot_pixels(const void *image, int image_kind, int h, int w, int pitch, int64_t num_hot, uint8_t *hot,
                              void *scratch, int64_t scratch_bytes, void *stream) {
    if (!image || !hot || !scratch || h <= 0 || w <= 0 || pitch < w || (int64_t)h * w >= (int64_t)HOT_NONE ||
        (image_kind != EVK_SELECT_I32 && image_kind != EVK_SELECT_F64))
        return EVK_EINVAL;
    if (scratch_bytes < HOT_SCRATCH) return EVK_ESCRATCH;
    if (image_kind == EVK_SELECT_I32)
        return hot_pixels(static_cast<const int32_t *>(image), h, w, pitch, num_hot, hot, scratch, (hipStream_t)stream);
    return hot_pixels(static_cast<const double *>(image), h, w, pitch, num_hot, hot, scratch, (hipStream_t)stream);
}

extern "C" int evk_random_subset(uint64_t seed, uint32_t purpose, int64_t n, int64_t k, void *state, int64_t state_bytes,
                                 void *stream) {
    if (!state || n < 0 || n > (int64_t)HOT_NONE || k < 0 || k > n) return EVK_EINVAL;
    if (state_bytes < HOT_SCRATCH) return EVK_ESCRATCH;
    SubsetKeys src = {seed, purpose, (uint32_t)n};
    select_kth(src, n, k, 1, seed, purpose, state, (hipStream_t)stream);
    return launch_status();
}

// clip_events_to_bounds(set_zero=True) (event_util.py:80-84): out[i] = (double)in[i] * mask[i], as numpy's xs * mask; a
// non-zero offset is added first (time stamps stored relative to it)
template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_mask_multiply(const T *__restrict__ in, int64_t n, double offset,
                                                           const double *__restrict__ mask, double *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (offset != 0.0 ? (double)in[i] + offset : (double)in[i]) * mask[i];
}

extern "C" int evk_mask_multiply_f64(int kind, const void *in, int64_t n, double offset, const double *mask, double *out,
                                     void *stream) {
    if (n < 0 || (n > 0 && (!in || !mask || !out)) || kind < EVK_SELECT_I16 || kind > EVK_SELECT_F64) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int g = stream_grid(n);
    with_time_kind(kind, in, [&](auto *col) { k_mask_multiply<<<g, EVK_BLOCK, 0, s>>>(col, n, offset, mask, out); });
    return launch_status();
}
