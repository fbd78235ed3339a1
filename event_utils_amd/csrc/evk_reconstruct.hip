// Intensity reconstruction (include/evk.h, "Intensity reconstruction"): the leaky event integrator (high-pass filter) and the
// complementary filter of Scheerlinck, Barnes & Mahony (ACCV 2018).  Per pixel the state follows dL/dt = -alpha (L - F(t))
// between events and steps by +c_on / -c_off at an event.  The system is linear, so L(T) = P(T) + E(T):
//
//   P(T)  the event-free solution from L(t_start) = initial under the frame target F(t): one exp per frame interval and query,
//         formed inline by the lane that owns the pixel
//   E(T)  the event term sum_j c_j exp(-alpha (T - t_j)) over the counted events before the query's cut.  Every term is
//         independent of the others, so a run is an order-fixed sum, and from one query to the next the sum chains as
//         E_k = exp(-alpha (T_k - T_{k-1})) E_{k-1} + (the terms of the new events): one exp per event whatever K is
//
// k_reconstruct runs on the one-class grouping of evk_group.h (order[], start[]) the way k_dn_refractory does: a wave takes 64
// consecutive keys; lane l walks the run of its key by itself when that run is shorter than wave_run (four events loaded ahead
// of their exps), and the longer runs are then taken by the whole wave, one after the other, 64 * RC_WAVE_ITEMS consecutive
// events per step.  On the wave path lane l sums the events at positions l, l + 64, ... of the query's part of the run, and a
// wave reduction in a fixed order (DPP row scans, as wave_incl_scan_u32) joins the 64 sums once per query.  A query's cut inside
// a run is where the ascending stream indices of the run reach m_k: the lane path finds it as it walks, the wave path by a lower
// bound.  No atomics: results repeat bit for bit.  Every index comes from a key below H*W, a position below n or a frame below
// nf: nothing leaves its array whatever the columns hold.
#include "evk_common.h"
#include "evk_group.h"
#include "evk_pred.h"

namespace evk {

constexpr int RC_WAVE_ITEMS = 4;                      // chunks of 64 events per step of a wave on a long run

struct RcArgs {
    const uint8_t *pos;                               // n "positive" flags, stream order
    const uint32_t *order, *start;
    int64_t n, nkeys, nq, start_cut;
    const int64_t *cuts;
    const double *t_refs, *initial, *frames, *frame_ts;
    int nf;
    double alpha, c_on, c_off, t_start;
    uint32_t wave_run;
    float *out;
};

// the event-free part P of one pixel: its value, the time it stands at and the frame that holds there
struct RcPixel {
    double p, cur;
    int f;
};

__device__ __forceinline__ RcPixel rc_begin(const RcArgs &a, int64_t key) {
    RcPixel s;
    s.p = a.initial ? a.initial[key] : 0.0;
    s.cur = a.t_start;
    s.f = 0;
    return s;
}

// P from s.cur to tk >= s.cur, split at every frame time inside (s.cur, tk); alpha == 0 leaves P as it is
__device__ __forceinline__ double rc_advance(const RcArgs &a, int64_t key, RcPixel &s, double tk) {
    if (a.alpha == 0.0) return s.p;
    while (s.f + 1 < a.nf && a.frame_ts[s.f + 1] <= s.cur) ++s.f;
    for (;;) {
        const double target = a.nf ? a.frames[(int64_t)s.f * a.nkeys + key] : 0.0;
        const bool split = s.f + 1 < a.nf && a.frame_ts[s.f + 1] < tk;
        const double b = split ? a.frame_ts[s.f + 1] : tk;
        s.p = target + (s.p - target) * exp(-a.alpha * (b - s.cur));
        s.cur = b;
        if (!split) break;
        ++s.f;
    }
    return s.p;
}

// one lane's value through the DPP path, as two 32-bit halves (old = 0, bound_ctrl = false: a lane without a source gets +0.0)
template <int CTRL, int ROWS>
__device__ __forceinline__ double rc_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, false);
    return __hiloint2double(hi, lo);
}

// the sum of the 64 lanes' values in the fixed order of wave_incl_scan_u32 (lane 63's inclusive scan), to every lane.  ALL 64
// LANES MUST BE ACTIVE at the call.
__device__ __forceinline__ double rc_wave_sum(double v) {
    v += rc_dpp<0x111, 0xf>(v);                       // row_shr:1
    v += rc_dpp<0x112, 0xf>(v);                       // row_shr:2
    v += rc_dpp<0x114, 0xf>(v);                       // row_shr:4
    v += rc_dpp<0x118, 0xf>(v);                       // row_shr:8
    v += rc_dpp<0x142, 0xa>(v);                       // row_bcast:15 into rows 1 and 3
    v += rc_dpp<0x143, 0xc>(v);                       // row_bcast:31 into rows 2 and 3
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63), hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int64_t rc_cut(const RcArgs &a, int64_t k) {
    const int64_t m = a.cuts[k];
    return m < 0 ? 0 : (m > a.n ? a.n : m);
}

template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_reconstruct(const T *__restrict__ t, const RcArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (EVK_BLOCK / EVK_WAVE);
    const uint32_t sc = (uint32_t)a.start_cut;
    for (int64_t kb = (((int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x) >> 6) * 64; kb < a.nkeys; kb += nwaves * 64) {
        const int64_t key = kb + lane;
        uint32_t s = 0, e = 0;
        if (key < a.nkeys && a.n > 0) s = a.start[key], e = a.start[key + 1];
        const uint32_t len = e - s;
        const bool is_long = len >= a.wave_run && len > 0;
        if (key < a.nkeys && !is_long) {
            RcPixel px = rc_begin(a, key);
            double sum = 0.0, tprev = 0.0;
            uint32_t pos = s;
            for (int64_t k = 0; k < a.nq; ++k) {
                const double tk = a.t_refs[k];
                const uint32_t mk = (uint32_t)rc_cut(a, k);
                if (k > 0) sum = sum * exp(-a.alpha * (tk - tprev));
                tprev = tk;
                bool more = true;
                while (pos < e && more) {
                    const uint32_t m = e - pos;
                    uint32_t j[4];
                    double tv[4], term[4];
                    uint8_t pf[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) j[u] = (uint32_t)u < m ? a.order[pos + u] : 0xFFFFFFFFu;
                    // (the run's indices ascend, so the events before the cut are a prefix of the four)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool in = j[u] < mk;     // (mk <= n: also false past the run's end)
                        tv[u] = in ? (double)t[j[u]] : tk;
                        pf[u] = in ? a.pos[j[u]] : (uint8_t)0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) term[u] = (pf[u] ? a.c_on : -a.c_off) * exp(-a.alpha * (tk - tv[u]));
                    uint32_t taken = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (j[u] < mk) {
                            ++taken;
                            if (j[u] >= sc) sum += term[u];
                        }
                    }
                    pos += taken;
                    more = taken == 4;
                }
                a.out[k * a.nkeys + key] = (float)(rc_advance(a, key, px, tk) + sum);
            }
        }
        uint64_t longs = __ballot(is_long);
        while (longs) {                                // wave-uniform from here on
            const int l = __builtin_ctzll(longs);
            longs &= longs - 1;
            const uint32_t ws = __shfl(s, l, 64), we = __shfl(e, l, 64);
            const int64_t wkey = kb + l;
            constexpr uint32_t STEP = 64 * RC_WAVE_ITEMS;
            RcPixel px = rc_begin(a, wkey);            // (used by lane 0)
            double acc = 0.0, tprev = 0.0;             // lane l: the events at positions l, l + 64, ... of the run
            uint32_t from = ws;
            for (int64_t k = 0; k < a.nq; ++k) {
                const double tk = a.t_refs[k];
                const uint32_t mk = (uint32_t)rc_cut(a, k);
                uint32_t to = ts_pred(a.order, ws, we, mk);
                if (to < from) to = from;
                if (k > 0) acc = acc * exp(-a.alpha * (tk - tprev));
                tprev = tk;
                // (to <= we < 2^31: positions past the part's end do not wrap)
                // the indices two steps and the times and flags one step ahead of their exps
                uint32_t j0[RC_WAVE_ITEMS], j1[RC_WAVE_ITEMS], j2[RC_WAVE_ITEMS];
                double tv0[RC_WAVE_ITEMS], tv1[RC_WAVE_ITEMS];
                uint8_t pf0[RC_WAVE_ITEMS], pf1[RC_WAVE_ITEMS];
#pragma unroll
                for (int u = 0; u < RC_WAVE_ITEMS; ++u) {
                    const uint32_t p0 = from + 64u * u + lane, p1 = p0 + STEP;
                    j0[u] = p0 < to ? a.order[p0] : 0u;
                    j1[u] = p1 < to ? a.order[p1] : 0u;
                }
#pragma unroll
                for (int u = 0; u < RC_WAVE_ITEMS; ++u) {
                    const bool in = from + 64u * u + lane < to;
                    tv0[u] = in ? (double)t[j0[u]] : tk;
                    pf0[u] = in ? a.pos[j0[u]] : (uint8_t)0;
                }
                for (uint32_t base = from; base < to; base += STEP) {
#pragma unroll
                    for (int u = 0; u < RC_WAVE_ITEMS; ++u) {
                        const uint32_t p1 = base + STEP + 64u * u + lane, p2 = p1 + STEP;
                        j2[u] = p2 < to ? a.order[p2] : 0u;
                        tv1[u] = p1 < to ? (double)t[j1[u]] : tk;
                        pf1[u] = p1 < to ? a.pos[j1[u]] : (uint8_t)0;
                    }
#pragma unroll
                    for (int u = 0; u < RC_WAVE_ITEMS; ++u) {
                        const double term = (pf0[u] ? a.c_on : -a.c_off) * exp(-a.alpha * (tk - tv0[u]));
                        if (base + 64u * u + lane < to && j0[u] >= sc) acc += term;
                    }
#pragma unroll
                    for (int u = 0; u < RC_WAVE_ITEMS; ++u) j0[u] = j1[u], j1[u] = j2[u], tv0[u] = tv1[u], pf0[u] = pf1[u];
                }
                from = to;
                const double sum = rc_wave_sum(acc);
                if (lane == 0) a.out[k * a.nkeys + wkey] = (float)(rc_advance(a, wkey, px, tk) + sum);
            }
        }
    }
}

template <typename T>
static void rc_launch(const T *t, const RcArgs &a, hipStream_t s) {
    k_reconstruct<T><<<stream_grid(a.nkeys), EVK_BLOCK, 0, s>>>(t, a);
}

}  // namespace evk

using namespace evk;

extern "C" int evk_reconstruct(int t_kind, const void *t, const uint8_t *pos_flags, int64_t n, int h, int w, double alpha,
                               double c_on, double c_off, double t_start, const double *initial, int nf, const double *frames,
                               const double *frame_ts, int64_t nq, const int64_t *cuts, const double *t_refs, int64_t start_cut,
                               int wave_run, const void *scratch, float *out, void *stream) {
    if (!ts_kind_ok(t_kind) || (n > 0 && (!t || !pos_flags)) || nq < 1 || !cuts || !t_refs || !out || !(alpha >= 0.0) ||
        !(alpha <= 1.79769313486231570815e308) || !(c_on > 0.0) || !(c_off > 0.0) || !(c_on <= 1.79769313486231570815e308) ||
        !(c_off <= 1.79769313486231570815e308) || !(t_start == t_start) || nf < 0 || (nf > 0 && (!frames || !frame_ts)) ||
        start_cut < 0 || start_cut > n)
        return EVK_EINVAL;
    DnScratch L;
    if (dn_open(scratch, n, h, w, 1, &L)) return EVK_EINVAL;      // (a misaligned scratch too: this entry point has no EALIGN)
    const int64_t nkeys = (int64_t)h * w;
    RcArgs a;
    a.pos = pos_flags;
    a.order = n > 0 ? L.order : nullptr;               // (no events: every run is empty and the grouping is not read)
    a.start = n > 0 ? L.start : nullptr;
    a.n = n, a.nkeys = nkeys, a.nq = nq, a.start_cut = start_cut;
    a.cuts = cuts;
    a.t_refs = t_refs, a.initial = initial, a.frames = nf ? frames : nullptr, a.frame_ts = nf ? frame_ts : nullptr;
    a.nf = nf;
    a.alpha = alpha, a.c_on = c_on, a.c_off = c_off, a.t_start = t_start;
    a.wave_run = wave_run > 0 ? (uint32_t)wave_run : (uint32_t)EVK_RECONSTRUCT_WAVE_RUN;
    a.out = out;
    hipStream_t s = (hipStream_t)stream;
    with_time_kind(t_kind, t, [&](auto *tt) { rc_launch(tt, a, s); });
    return launch_status();
}
