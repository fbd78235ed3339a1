// Event simulation (include/evk.h, "Event simulation"): events from log-intensity frames by the threshold-crossing model (ESIM,
// Rebecq et al. 2018; the noise-free core of v2e), the forward model of which the leaky integrator with alpha = 0 is the inverse.
// The log intensity of a pixel is linear between two frames; the pixel fires whenever it has moved one contrast away from its
// reference level R, and R follows by that contrast.
//
//   k_sim_count   one lane per pixel (neighbouring lanes read neighbouring pixels of every frame): walks the nf - 1 intervals and
//                 stores the pixel's event count; overflowed pixel-intervals and refused map contrasts go to two device counters
//   (host)        an exclusive scan of the counts over the pixel index; the total and the counters come back in one read
//   k_sim_emit    the identical walk (sim_walk is the one statement of it): the events of pixel q go to offset[q] .. in emission
//                 order, as (sort key, pixel * 2 + polarity); the state R, tl of the pixel is stored
//   sort          a stable hipcub radix sort of the pairs over the key bits in which the times can differ; the pixel-major
//                 emission order makes stability the tie rule (equal t by pixel index, then by emission order)
//   k_sim_gather  one streaming pass: the time back from the key, x, y, p from the value
//
// The sort key of a time is its order-preserving 64-bit image minus that of frame_ts[0] (every t >= frame_ts[0]): the host knows
// the bit range from the frame times alone, and the gather gets t back from the key exactly.  Every operation of the walk is one
// IEEE rounding (-ffp-contract=off, no fast-math): the two walks, and a host restatement, take the same crossings at the same
// times bit for bit.  No atomics on the output path.  The step limit EVK_SIMULATE_MAX_STEPS bounds every lane's loop whatever the
// frames hold; a store of the emit pass is bounded by `total` whatever the offsets hold.
#include <hipcub/hipcub.hpp>

#include "evk_common.h"

namespace evk {

constexpr uint64_t SIM_SIGN = 0x8000000000000000ull;
constexpr double SIM_DBL_MAX = 1.79769313486231570815e308;
constexpr int64_t SIM_SORT_MAX = 0x7FFFFFFF;          // hipcub's item count is an int

// the order-preserving image of a double (unsigned order = numeric order; -0.0 below +0.0: the frame times hold no -0.0, so no t is)
__host__ __device__ __forceinline__ uint64_t sim_image(double t) {
    const uint64_t u = (uint64_t)__builtin_bit_cast(int64_t, t);
    return (u & SIM_SIGN) ? ~u : (u | SIM_SIGN);
}
__device__ __forceinline__ double sim_unimage(uint64_t k) {
    return __builtin_bit_cast(double, (int64_t)((k & SIM_SIGN) ? (k ^ SIM_SIGN) : ~k));
}

struct SimArgs {
    const double *frames, *frame_ts, *c_on_map, *c_off_map, *reference, *last_ts;
    int nf;
    int64_t nkeys;
    double c_on, c_off, refractory;
};

struct SimPixel {
    double R, tl;
    uint32_t count, overflows;
    bool bad;                                         // a map contrast that is not positive and finite: the pixel is not walked
};

__host__ __device__ __forceinline__ bool sim_contrast_ok(double c) { return c > 0.0 && c <= SIM_DBL_MAX; }

// The walk of pixel q (the definition of include/evk.h, one rounding per operation).  emit(k, t, up) is called for the k-th emitted
// event of the pixel.
template <typename Emit>
__device__ __forceinline__ SimPixel sim_walk(const SimArgs &a, int64_t q, Emit emit) {
    SimPixel s;
    s.R = a.reference ? a.reference[q] : a.frames[q];
    s.tl = a.last_ts ? a.last_ts[q] : -__builtin_inf();
    s.count = s.overflows = 0;
    const double c_on = a.c_on_map ? a.c_on_map[q] : a.c_on, c_off = a.c_off_map ? a.c_off_map[q] : a.c_off;
    s.bad = !sim_contrast_ok(c_on) || !sim_contrast_ok(c_off);
    if (s.bad) return s;
    double R = s.R, tl = s.tl;
    double L0 = a.frames[q], T0 = a.frame_ts[0];
    double L1 = a.frames[a.nkeys + q];                 // (nf >= 2) one frame loaded ahead of the interval that needs it
    for (int f = 0; f + 1 < a.nf; ++f) {
        const double L2 = f + 2 < a.nf ? a.frames[(int64_t)(f + 2) * a.nkeys + q] : 0.0;
        const double T1 = a.frame_ts[f + 1];
        const double d = L1 - L0, dT = T1 - T0;
        if (d != 0.0 && fabs(d) <= SIM_DBL_MAX) {      // (a NaN d fails both)
            const bool up = d > 0.0;
            const double c = up ? c_on : -c_off;       // R - c_off == R + (-c_off) in IEEE arithmetic
            uint32_t steps = 0;
            for (;;) {
                const double Rn = R + c;
                if (!(up ? Rn <= L1 : Rn >= L1)) break;
                if (steps == (uint32_t)EVK_SIMULATE_MAX_STEPS) {
                    ++s.overflows;
                    break;
                }
                ++steps;
                R = Rn;
                double frac = (R - L0) / d;
                frac = frac < 0.0 ? 0.0 : (frac > 1.0 ? 1.0 : frac);
                const double t = T0 + frac * dT;
                if (t - tl >= a.refractory) {
                    emit(s.count, t, up);
                    s.count += s.count != 0xFFFFFFFFu;   // (saturates: such a total is refused by the host)
                }
                tl = t;
            }
        }
        L0 = L1, L1 = L2, T0 = T1;
    }
    s.R = R, s.tl = tl;
    return s;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_sim_count(const SimArgs a, uint32_t *__restrict__ counts,
                                                         unsigned long long *__restrict__ report) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.nkeys; q += (int64_t)gridDim.x * blockDim.x) {
        const SimPixel s = sim_walk(a, q, [](uint32_t, double, bool) {});
        counts[q] = s.count;
        if (s.overflows) atomicAdd(&report[0], (unsigned long long)s.overflows);
        if (s.bad) atomicAdd(&report[1], 1ull);
    }
}

template <typename V>
__global__ void __launch_bounds__(EVK_BLOCK) k_sim_emit(const SimArgs a, const int64_t *__restrict__ offsets, int64_t total,
                                                        uint64_t base, uint64_t *__restrict__ keys, V *__restrict__ vals,
                                                        double *__restrict__ ref_out, double *__restrict__ tl_out) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < a.nkeys; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t off = offsets[q];
        const SimPixel s = sim_walk(a, q, [&](uint32_t k, double t, bool up) {
            const int64_t pos = off + k;
            if (pos >= 0 && pos < total) {
                keys[pos] = sim_image(t) - base;
                vals[pos] = (V)(((uint64_t)q << 1) | (up ? 1u : 0u));
            }
        });
        ref_out[q] = s.R;
        tl_out[q] = s.tl;
    }
}

template <typename V>
__global__ void __launch_bounds__(EVK_BLOCK) k_sim_gather(const uint64_t *__restrict__ keys, const V *__restrict__ vals, int64_t total,
                                                          uint64_t base, int64_t w, int64_t *__restrict__ xs, int64_t *__restrict__ ys,
                                                          double *__restrict__ ts, int64_t *__restrict__ ps) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t v = (uint64_t)vals[i];
        const int64_t q = (int64_t)(v >> 1);
        const int64_t y = q / w;
        xs[i] = q - y * w;
        ys[i] = y;
        ts[i] = sim_unimage(keys[i] + base);
        ps[i] = (v & 1u) ? 1 : -1;
    }
}

static inline int64_t sim_al(int64_t b) { return (b + 255) & ~(int64_t)255; }

// the pairs carry pixel * 2 + polarity: 32 bits hold it up to 2^31 pixels
static inline bool sim_wide(int64_t nkeys, int wide) { return wide != 0 || nkeys > ((int64_t)1 << 31); }

// the key bits in which two times of [t_first, t_max] can differ, at least 8 (evk_augment.hip on hipcub's narrow bit ranges)
static inline int sim_key_bits(double t_first, double t_max) {
    const uint64_t span = sim_image(t_max) - sim_image(t_first);
    const int bits = span ? 64 - __builtin_clzll(span) : 0;
    return bits < 8 ? 8 : bits;
}

template <typename V>
static size_t sim_temp_bytes(int64_t total, int bits) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const V *)nullptr, (V *)nullptr,
                                             (int)total, 0, bits);
    return b;
}

template <typename V>
static int sim_sort(const uint64_t *keys, const void *vals, int64_t total, int w, int bits, uint64_t base, char *sb, int64_t scratch_bytes,
                    int64_t *xs, int64_t *ys, double *ts, int64_t *ps, hipStream_t s) {
    uint64_t *keys_out = reinterpret_cast<uint64_t *>(sb);
    V *vals_out = reinterpret_cast<V *>(sb + sim_al(8 * total));
    const int64_t used = sim_al(8 * total) + sim_al((int64_t)sizeof(V) * total);
    size_t tb = sim_temp_bytes<V>(total, bits);
    if ((int64_t)tb > scratch_bytes - used) return EVK_ESCRATCH;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(sb + used, tb, keys, keys_out, static_cast<const V *>(vals), vals_out, (int)total,
                                                      0, bits, s);
    if (e != hipSuccess) return (int)e;
    k_sim_gather<V><<<stream_grid(total), EVK_BLOCK, 0, s>>>(keys_out, vals_out, total, base, (int64_t)w, xs, ys, ts, ps);
    return launch_status();
}

static bool sim_args(SimArgs &a, const double *frames, const double *frame_ts, int nf, int h, int w, double c_on, double c_off,
                     const double *c_on_map, const double *c_off_map, double refractory, const double *reference,
                     const double *last_event_ts) {
    if (!frames || !frame_ts || nf < 2 || h <= 0 || w <= 0 || (int64_t)h * w > 0xFFFFFFFFll || (!c_on_map && !sim_contrast_ok(c_on)) ||
        (!c_off_map && !sim_contrast_ok(c_off)) || !(refractory >= 0.0))
        return false;
    a.frames = frames, a.frame_ts = frame_ts, a.c_on_map = c_on_map, a.c_off_map = c_off_map, a.reference = reference;
    a.last_ts = last_event_ts;
    a.nf = nf, a.nkeys = (int64_t)h * w;
    a.c_on = c_on, a.c_off = c_off, a.refractory = refractory;
    return true;
}

}  // namespace evk

using namespace evk;

extern "C" int evk_simulate_count(const double *frames, const double *frame_ts, int nf, int h, int w, double c_on, double c_off,
                                  const double *c_on_map, const double *c_off_map, double refractory, const double *reference,
                                  const double *last_event_ts, uint32_t *counts, uint64_t *report, void *stream) {
    SimArgs a;
    if (!sim_args(a, frames, frame_ts, nf, h, w, c_on, c_off, c_on_map, c_off_map, refractory, reference, last_event_ts) || !counts ||
        !report)
        return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(report, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return (int)e;
    k_sim_count<<<stream_grid(a.nkeys), EVK_BLOCK, 0, s>>>(a, counts, reinterpret_cast<unsigned long long *>(report));
    return launch_status();
}

extern "C" int evk_simulate_emit(const double *frames, const double *frame_ts, int nf, int h, int w, double c_on, double c_off,
                                 const double *c_on_map, const double *c_off_map, double refractory, const double *reference,
                                 const double *last_event_ts, const int64_t *offsets, int64_t total, double t_first, int wide,
                                 uint64_t *keys, void *vals, double *reference_out, double *last_event_ts_out, void *stream) {
    SimArgs a;
    if (!sim_args(a, frames, frame_ts, nf, h, w, c_on, c_off, c_on_map, c_off_map, refractory, reference, last_event_ts) || !offsets ||
        total < 0 || total > SIM_SORT_MAX || (total > 0 && (!keys || !vals)) || !reference_out || !last_event_ts_out ||
        !(t_first == t_first))
        return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t base = sim_image(t_first);
    const int g = stream_grid(a.nkeys);
    if (sim_wide(a.nkeys, wide))
        k_sim_emit<uint64_t><<<g, EVK_BLOCK, 0, s>>>(a, offsets, total, base, keys, (uint64_t *)vals, reference_out, last_event_ts_out);
    else
        k_sim_emit<uint32_t><<<g, EVK_BLOCK, 0, s>>>(a, offsets, total, base, keys, (uint32_t *)vals, reference_out, last_event_ts_out);
    return launch_status();
}

extern "C" int64_t evk_simulate_sort_scratch_bytes(int64_t total, int h, int w, int wide, double t_first, double t_max) {
    if (total < 0 || total > SIM_SORT_MAX || h <= 0 || w <= 0 || (int64_t)h * w > 0xFFFFFFFFll || !(t_max >= t_first)) return EVK_EINVAL;
    const int bits = sim_key_bits(t_first, t_max);
    const bool wd = sim_wide((int64_t)h * w, wide);
    return sim_al(8 * total) + sim_al((wd ? 8 : 4) * total) +
           sim_al((int64_t)(wd ? sim_temp_bytes<uint64_t>(total, bits) : sim_temp_bytes<uint32_t>(total, bits)));
}

extern "C" int evk_simulate_sort(const uint64_t *keys, const void *vals, int64_t total, int h, int w, int wide, double t_first,
                                 double t_max, void *scratch, int64_t scratch_bytes, int64_t *xs, int64_t *ys, double *ts, int64_t *ps,
                                 void *stream) {
    if (total < 0 || total > SIM_SORT_MAX || h <= 0 || w <= 0 || (int64_t)h * w > 0xFFFFFFFFll || !(t_max >= t_first) ||
        (total > 0 && (!keys || !vals || !scratch || !xs || !ys || !ts || !ps)) || ((uintptr_t)scratch & 255u))
        return EVK_EINVAL;
    if (total == 0) return EVK_OK;
    if (scratch_bytes < evk_simulate_sort_scratch_bytes(total, h, w, wide, t_first, t_max)) return EVK_ESCRATCH;
    hipStream_t s = (hipStream_t)stream;
    const int bits = sim_key_bits(t_first, t_max);
    const uint64_t base = sim_image(t_first);
    char *sb = static_cast<char *>(scratch);
    if (sim_wide((int64_t)h * w, wide)) return sim_sort<uint64_t>(keys, vals, total, w, bits, base, sb, scratch_bytes, xs, ys, ts, ps, s);
    return sim_sort<uint32_t>(keys, vals, total, w, bits, base, sb, scratch_bytes, xs, ys, ts, ps, s);
}
