// Prophesee EVT3 (16-bit words) and EVT2 (32-bit words) raw event streams -> xs, ys, ts, ps columns (evk.h).
//
// The decoder is a state machine only on the surface: every piece of its state is a last-write-wins value (y, polarity, t_low,
// t_high), a segmented sum (base_x: the increments behind the last VECT_BASE_X) or a count, so a run of words reduces to an
// ASSOCIATIVE summary (Sum, combine) and decoding is scan + order-preserving expansion -- the structure of the compaction of
// evk_select.hip: three launches, no hand-over, ticket or wait between workgroups, a result independent of dispatch order.
//   k_raw_sum    one workgroup per chunk of RAW_CHUNK words: the chunk's summary
//   k_raw_scan   one workgroup: the summaries combined in order behind the caller's state (each lane a run of consecutive chunks,
//                the lanes' runs by a wave scan) -> per chunk the state it starts from and its output offset (one wide
//                summary), the total, the final state, the counters
//   k_raw_write  one workgroup per chunk: the lanes' summaries scanned behind the chunk's start, each lane then walks its
//                words from its own start state and writes its events at offset + rank
// A lane owns RAW_ITEMS consecutive words (16-byte loads at dword alignment, evk_part.h's load_col16; an EVT3 column that starts
// on an odd half word is read from the dword below it and shifted).  Every index that reaches memory comes from ranks and
// offsets, never from a word's payload, and every store is guarded by the total the scan found: any byte stream decodes to
// something defined.
#include "evk_common.h"

namespace evk {

constexpr int RAW_ITEMS = 16;                                  // consecutive words per lane
constexpr int64_t RAW_CHUNK = (int64_t)EVK_BLOCK * RAW_ITEMS;
static_assert(RAW_CHUNK == EVK_RAW_CHUNK, "evk.h states the chunk");
static_assert(EVK_BLOCK == EVK_RAW_SCAN_WIDTH, "evk.h states the lanes of the scan");
constexpr int RAW_WAVES = EVK_BLOCK / EVK_WAVE;
constexpr int RAW_STAGE = 4096;                                // events per round of the LDS staging (13 bytes each)
constexpr uint32_t RAW_LOOP_STEP = 4085;                       // a TIME_HIGH this far below the last one is a wrap

// Summary of a run of words.  lww: bit 0 / 1 / 2 / 3 = the run sets y / base_x and polarity / t_low / t_high; y in bits 4-14,
// the vector polarity in bit 15, t_low in bits 16-27.  base: the last base_x plus the increments behind it, or the increments of
// the whole run when it sets none (mod 2^16).  first_h, last_h: the run's first and last TIME_HIGH.  loops, back: wraps and
// small backward steps between TIME_HIGH words INSIDE the run.  pre, post: events of the words before / from the run's first
// TIME_HIGH (whether `pre` is emitted depends on have_time at the run's start).  C: uint32 inside a chunk, int64 across chunks.
constexpr uint32_t HAS_Y = 1, HAS_BASE = 2, HAS_TLOW = 4, HAS_TH = 8;
constexpr uint32_t M_Y = 0x7FF0u | HAS_Y, M_BASE = 0x8000u | HAS_BASE, M_TLOW = 0x0FFF0000u | HAS_TLOW;
template <typename C>
struct Sum {
    uint32_t lww, base, first_h, last_h;
    C loops, back, pre, post, trig, other;
};
typedef Sum<uint32_t> Sum32;
typedef Sum<int64_t> Sum64;

// a then b.  Associative: lww fields and t_high are "the last writer's", base is a sum restarted at the last writer, the
// counters add, and the two terms that look at both sides -- the wrap between a's last and b's first TIME_HIGH, the side of a's
// first TIME_HIGH on which b's early events fall -- depend on a and b only through fields the combination carries on.
template <int FMT, typename C, typename D>
__device__ __forceinline__ Sum<C> combine(const Sum<C> &a, const Sum<D> &b) {
    Sum<C> c;
    const uint32_t m = ((b.lww & HAS_Y) ? M_Y : 0u) | ((b.lww & HAS_BASE) ? M_BASE : 0u) | ((b.lww & HAS_TLOW) ? M_TLOW : 0u);
    c.lww = (b.lww & m) | (a.lww & ~m) | (b.lww & HAS_TH);
    c.base = (b.lww & HAS_BASE) ? b.base : ((a.base + b.base) & 0xFFFFu);
    const bool ah = a.lww & HAS_TH, bh = b.lww & HAS_TH;
    c.first_h = ah ? a.first_h : b.first_h;
    c.last_h = bh ? b.last_h : a.last_h;
    c.loops = a.loops + (C)b.loops;
    c.back = a.back + (C)b.back;
    if (FMT == EVK_RAW_EVT3 && ah && bh) {
        if (a.last_h >= b.first_h + RAW_LOOP_STEP) c.loops += 1;
        else if (a.last_h > b.first_h) c.back += 1;
    }
    c.pre = a.pre + (ah ? (C)0 : (C)b.pre);
    c.post = a.post + (C)b.post + (ah ? (C)b.pre : (C)0);
    c.trig = a.trig + (C)b.trig;
    c.other = a.other + (C)b.other;
    return c;
}

template <typename S>
__device__ __forceinline__ S shfl_up_sum(const S &v, int off) {
    constexpr int N = sizeof(S) / 4;
    uint32_t a[N];
    __builtin_memcpy(a, &v, sizeof(S));
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = __shfl_up(a[k], off, 64);
    S r;
    __builtin_memcpy(&r, a, sizeof(S));
    return r;
}

// inclusive scan of the wave's summaries in lane order (all 64 lanes active)
template <int FMT, typename S>
__device__ __forceinline__ S wave_scan_sum(S v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const S o = shfl_up_sum(v, off);
        if (lane >= off) v = combine<FMT>(o, v);
    }
    return v;
}

// ---- the two formats: one word into a summary, one word through a lane's running state --------------------------------------
template <typename P>
struct Lane {                        // a lane's decoder state while it walks its words; pos: where its next event goes (P: a
    uint32_t y, base, pol, tlow, th; // position in the output, or an int relative to the staged round)
    bool have;
    int64_t loops;
    P pos;
};

template <typename P, typename C>
__device__ __forceinline__ Lane<P> lane_start(const Sum<C> &s, P pos) {
    Lane<P> l;
    l.y = (s.lww >> 4) & 0x7FFu, l.pol = (s.lww >> 15) & 1u, l.tlow = (s.lww >> 16) & 0xFFFu;
    l.base = s.base, l.th = s.last_h, l.have = s.lww & HAS_TH, l.loops = (int64_t)s.loops, l.pos = pos;
    return l;
}

template <int FMT>
struct Format;

// EVT3 without a branch per word type: neighbouring lanes hold words of different types, so a wave would execute every branch.
// Every field is updated by a select on the type; the events of a word are the set bits of `emask` (an ADDR_X is a one-bit
// vector at its own x), and the only loop is over those bits.
constexpr uint32_t EVT3_KNOWN = (1u << 0x0) | (1u << 0x2) | (1u << 0x3) | (1u << 0x4) | (1u << 0x5) | (1u << 0x6) | (1u << 0x8) | (1u << 0xA);
__device__ __forceinline__ uint32_t evt3_emask(uint32_t type, uint32_t v) {
    return type == 0x2 ? 1u : type == 0x4 ? v : type == 0x5 ? (v & 0xFFu) : 0u;
}
__device__ __forceinline__ uint32_t evt3_next_base(uint32_t base, uint32_t type, uint32_t v) {
    return type == 0x3 ? (v & 0x7FFu) : ((base + (type == 0x4 ? 12u : type == 0x5 ? 8u : 0u)) & 0xFFFFu);
}

template <>
struct Format<EVK_RAW_EVT3> {
    template <typename C>
    static __device__ __forceinline__ void sum_word(Sum<C> &s, uint32_t w) {
        const uint32_t v = w & 0xFFFu, type = w >> 12;
        const bool has = s.lww & HAS_TH, is_th = type == 0x8;
        const C ev = (C)__popc(evt3_emask(type, v));
        s.post += has ? ev : (C)0;
        s.pre += has ? (C)0 : ev;
        uint32_t lww = s.lww;
        lww = type == 0x0 ? ((lww & ~M_Y) | HAS_Y | ((v & 0x7FFu) << 4)) : lww;
        lww = type == 0x3 ? ((lww & ~M_BASE) | HAS_BASE | ((v >> 11) << 15)) : lww;
        lww = type == 0x6 ? ((lww & ~M_TLOW) | HAS_TLOW | (v << 16)) : lww;
        s.lww = is_th ? (lww | HAS_TH) : lww;
        s.base = evt3_next_base(s.base, type, v);
        const bool wrap = is_th && has && s.last_h >= v + RAW_LOOP_STEP;
        s.loops += wrap ? (C)1 : (C)0;
        s.back += (is_th && has && !wrap && s.last_h > v) ? (C)1 : (C)0;
        s.first_h = (is_th && !has) ? v : s.first_h;
        s.last_h = is_th ? v : s.last_h;
        s.trig += type == 0xA ? (C)1 : (C)0;
        s.other += ((EVT3_KNOWN >> type) & 1u) ? (C)0 : (C)1;
    }
    template <class L, class Sink>
    static __device__ __forceinline__ void walk_word(L &l, uint32_t w, Sink &sink) {
        const uint32_t v = w & 0xFFFu, type = w >> 12;
        uint32_t bits = l.have ? evt3_emask(type, v) : 0u;
        if (bits) {
            const uint32_t x0 = type == 0x2 ? (v & 0x7FFu) : l.base, p = type == 0x2 ? (v >> 11) : l.pol;
            const int64_t t = (l.loops << 24) + (int64_t)((l.th << 12) + l.tlow);
            do {                                                 // set bits in ascending order
                const uint32_t i = (uint32_t)__ffs((int)bits) - 1u;
                bits &= bits - 1u;
                sink.put(l.pos++, (x0 + i) & 0xFFFFu, l.y, t, p);
            } while (bits);
        }
        const bool is_th = type == 0x8;
        l.y = type == 0x0 ? (v & 0x7FFu) : l.y;
        l.base = evt3_next_base(l.base, type, v);
        l.pol = type == 0x3 ? (v >> 11) : l.pol;
        l.tlow = type == 0x6 ? v : l.tlow;
        l.loops += (is_th && l.have && l.th >= v + RAW_LOOP_STEP) ? 1 : 0;
        l.th = is_th ? v : l.th;
        l.have = l.have || is_th;
    }
};

template <>
struct Format<EVK_RAW_EVT2> {
    template <typename C>
    static __device__ __forceinline__ void sum_word(Sum<C> &s, uint32_t w) {
        switch (w >> 28) {
            case 0x0:
            case 0x1: ((s.lww & HAS_TH) ? s.post : s.pre) += 1; break;
            case 0x8:
                if (!(s.lww & HAS_TH)) s.lww |= HAS_TH, s.first_h = w & 0x0FFFFFFFu;
                s.last_h = w & 0x0FFFFFFFu;
                break;
            case 0xA: s.trig += 1; break;
            default: s.other += 1; break;
        }
    }
    template <class L, class Sink>
    static __device__ __forceinline__ void walk_word(L &l, uint32_t w, Sink &sink) {
        const uint32_t type = w >> 28;
        if (type <= 0x1) {
            if (l.have) sink.put(l.pos++, (w >> 11) & 0x7FFu, w & 0x7FFu, ((int64_t)l.th << 6) | (int64_t)((w >> 22) & 0x3Fu), type);
        } else if (type == 0x8) {
            l.th = w & 0x0FFFFFFFu, l.have = true;
        }
    }
};

// ---- a lane's words ---------------------------------------------------------------------------------------------------------
typedef uint32_t raw_u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) raw_quad4 {
    raw_u32x4 v;
};
__device__ __forceinline__ void load_quad(const uint32_t *p, uint32_t *d) {    // 16 bytes at any dword boundary
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Waddress-of-packed-member"
    const raw_u32x4 v = reinterpret_cast<const raw_quad4 *>(p)->v;
#pragma clang diagnostic pop
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
}

// words [first, first + RAW_ITEMS) of the stream into w[], those at or behind n left out -> the number loaded.  base32: the
// column's start rounded DOWN to a dword, half: 1 when an EVT3 column starts on that dword's upper half (the lower half then
// belongs to the same allocation: a tensor's storage starts on a dword).  A lane that is wholly inside the stream takes 16-byte
// loads; the dword that holds its last word is read whole, which stays inside the dword-rounded storage.
template <int FMT>
__device__ __forceinline__ int load_words(const uint32_t *base32, int half, int64_t first, int64_t n, uint32_t *w) {
    const int64_t left = n - first;
    const int nv = left >= RAW_ITEMS ? RAW_ITEMS : (left > 0 ? (int)left : 0);
    if constexpr (FMT == EVK_RAW_EVT2) {
        if (nv == RAW_ITEMS) {
#pragma unroll
            for (int q = 0; q < RAW_ITEMS / 4; ++q) load_quad(base32 + first + 4 * q, w + 4 * q);
        } else {
#pragma unroll
            for (int k = 0; k < RAW_ITEMS; ++k) w[k] = k < nv ? base32[first + k] : 0u;
        }
    } else {
        if (nv == RAW_ITEMS) {
            uint32_t d[RAW_ITEMS / 2 + 1];
            const uint32_t *p = base32 + first / 2;                 // (first is a multiple of RAW_ITEMS)
            load_quad(p, d);
            load_quad(p + 4, d + 4);
            d[8] = half ? p[8] : 0u;
#pragma unroll
            for (int k = 0; k < RAW_ITEMS / 2; ++k) {
                const uint32_t pair = half ? ((d[k] >> 16) | (d[k + 1] << 16)) : d[k];
                w[2 * k] = pair & 0xFFFFu, w[2 * k + 1] = pair >> 16;
            }
        } else {
            const uint16_t *p = reinterpret_cast<const uint16_t *>(base32) + half + first;
#pragma unroll
            for (int k = 0; k < RAW_ITEMS; ++k) w[k] = k < nv ? (uint32_t)p[k] : 0u;
        }
    }
    return nv;
}

template <int FMT>
__device__ __forceinline__ Sum32 lane_summary(const uint32_t *w, int nv) {
    Sum32 s = {};
#pragma unroll
    for (int k = 0; k < RAW_ITEMS; ++k)
        if (k < nv) Format<FMT>::sum_word(s, w[k]);
    return s;
}

// ---- launch 1: the chunk's summary ------------------------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(EVK_BLOCK) k_raw_sum(const uint32_t *__restrict__ base32, int half, int64_t n,
                                                     Sum32 *__restrict__ sums) {
    __shared__ Sum32 s_w[RAW_WAVES];
    uint32_t w[RAW_ITEMS];
    const int64_t first = (int64_t)blockIdx.x * RAW_CHUNK + (int64_t)threadIdx.x * RAW_ITEMS;
    const int nv = load_words<FMT>(base32, half, first, n, w);
    const Sum32 incl = wave_scan_sum<FMT>(lane_summary<FMT>(w, nv));
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        Sum32 t = s_w[0];
#pragma unroll
        for (int k = 1; k < RAW_WAVES; ++k) t = combine<FMT>(t, s_w[k]);
        sums[blockIdx.x] = t;
    }
}

// ---- launch 2: one workgroup of EVK_RAW_SCAN_WIDTH lanes; with more chunks than lanes a lane combines several ----------------
// state: y, base_x, vect_pol, t_low, t_high, loops, have_time, 0.  result: events, triggers, other, before_time, time_went_back,
// out_of_range (zeroed here, summed by the write), loops counted, 0.
template <int FMT>
__global__ void __launch_bounds__(EVK_BLOCK) k_raw_scan(const Sum32 *__restrict__ sums, int64_t nchunks,
                                                      const int64_t *__restrict__ state_in, Sum64 *__restrict__ starts,
                                                      int64_t *__restrict__ result, int64_t *__restrict__ state_out) {
    __shared__ Sum64 s_w[RAW_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Sum64 carry = {};                                   // the caller's state as the summary of everything before the stream
    carry.lww = HAS_Y | HAS_BASE | HAS_TLOW;
    int64_t loops_in = 0;
    if (state_in) {
        const uint32_t hmask = FMT == EVK_RAW_EVT3 ? 0xFFFu : 0x0FFFFFFFu;
        carry.lww |= (((uint32_t)state_in[0] & 0x7FFu) << 4) | (((uint32_t)state_in[2] & 1u) << 15) |
                     (((uint32_t)state_in[3] & 0xFFFu) << 16) | (state_in[6] ? HAS_TH : 0u);
        carry.base = (uint32_t)state_in[1] & 0xFFFFu;
        carry.first_h = carry.last_h = (uint32_t)state_in[4] & hmask;
        carry.loops = loops_in = state_in[5];
    }
    // lane t owns the run of `per` consecutive chunks [lo, hi): its loads do not depend on one another
    const int64_t per = (nchunks + EVK_BLOCK - 1) / EVK_BLOCK;
    const int64_t lo = (int64_t)threadIdx.x * per < nchunks ? (int64_t)threadIdx.x * per : nchunks;
    const int64_t hi = lo + per < nchunks ? lo + per : nchunks;
    Sum64 v = {};
#pragma unroll 4
    for (int64_t c = lo; c < hi; ++c) v = combine<FMT>(v, sums[c]);
    const Sum64 incl = wave_scan_sum<FMT>(v);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    Sum64 before = {}, total = {};
#pragma unroll
    for (int k = 0; k < RAW_WAVES; ++k) {
        if (k < wave) before = combine<FMT>(before, s_w[k]);
        total = combine<FMT>(total, s_w[k]);
    }
    Sum64 excl = shfl_up_sum(incl, 1);
    if (lane == 0) excl = Sum64{};
    Sum64 run = combine<FMT>(carry, combine<FMT>(before, excl));
#pragma unroll 4
    for (int64_t c = lo; c < hi; ++c) {
        starts[c] = run;
        run = combine<FMT>(run, sums[c]);
    }
    carry = combine<FMT>(carry, total);
    if (threadIdx.x == 0) {
        result[0] = carry.post, result[1] = carry.trig, result[2] = carry.other, result[3] = carry.pre, result[4] = carry.back;
        result[5] = 0, result[6] = carry.loops - loops_in, result[7] = 0;
        state_out[0] = (carry.lww >> 4) & 0x7FFu, state_out[1] = carry.base, state_out[2] = (carry.lww >> 15) & 1u;
        state_out[3] = (carry.lww >> 16) & 0xFFFu, state_out[4] = carry.last_h, state_out[5] = carry.loops;
        state_out[6] = (carry.lww & HAS_TH) ? 1 : 0, state_out[7] = 0;
    }
}

// ---- launch 3: the events ---------------------------------------------------------------------------------------------------
struct RawOut {
    int16_t *xs, *ys;
    void *ts;
    uint8_t *ps;
    int64_t total;                   // no position at or behind it is written
    uint32_t w, h;                   // the sensor, 0 x 0: none given
};

template <bool SECONDS>
__device__ __forceinline__ uint32_t store_event(const RawOut &o, int64_t pos, uint32_t x, uint32_t y, int64_t t, uint32_t p) {
    o.xs[pos] = (int16_t)x, o.ys[pos] = (int16_t)y, o.ps[pos] = (uint8_t)p;
    if constexpr (SECONDS) static_cast<double *>(o.ts)[pos] = (double)t / 1e6;
    else static_cast<int64_t *>(o.ts)[pos] = t;
    return (o.w && (x >= o.w || y >= o.h)) ? 1u : 0u;
}

template <bool SECONDS>
struct DirectSink {
    const RawOut &o;
    uint32_t bad;
    __device__ __forceinline__ void put(int64_t pos, uint32_t x, uint32_t y, int64_t t, uint32_t p) {
        if (pos < o.total) bad += store_event<SECONDS>(o, pos, x, y, t, p);
    }
};

struct Stage {
    int64_t t[RAW_STAGE];
    int16_t x[RAW_STAGE], y[RAW_STAGE];
    uint8_t p[RAW_STAGE];
};
struct StageSink {                   // k: the event's position relative to the round's first
    Stage &s;
    __device__ __forceinline__ void put(int k, uint32_t x, uint32_t y, int64_t t, uint32_t p) {
        if ((uint32_t)k < (uint32_t)RAW_STAGE) s.x[k] = (int16_t)x, s.y[k] = (int16_t)y, s.t[k] = t, s.p[k] = (uint8_t)p;
    }
};

template <int FMT, bool SECONDS, bool STAGED>
__global__ void __launch_bounds__(EVK_BLOCK) k_raw_write(const uint32_t *__restrict__ base32, int half, int64_t n,
                                                       const Sum32 *__restrict__ sums, const Sum64 *__restrict__ starts,
                                                       RawOut o, int64_t *__restrict__ result) {
    __shared__ Sum32 s_w[RAW_WAVES];
    __shared__ uint32_t s_bad[RAW_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t w[RAW_ITEMS];
    const int64_t first = (int64_t)blockIdx.x * RAW_CHUNK + (int64_t)threadIdx.x * RAW_ITEMS;
    const int nv = load_words<FMT>(base32, half, first, n, w);
    const Sum32 mine = lane_summary<FMT>(w, nv);
    const Sum32 incl = wave_scan_sum<FMT>(mine);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    Sum32 before = {};
#pragma unroll
    for (int k = 0; k < RAW_WAVES; ++k)
        if (k < wave) before = combine<FMT>(before, s_w[k]);
    Sum32 excl = shfl_up_sum(incl, 1);
    if (lane == 0) excl = Sum32{};
    const Sum64 chunk = starts[blockIdx.x];
    const Sum64 start = combine<FMT>(chunk, combine<FMT>(before, excl));
    o.total = result[0];
    uint32_t bad = 0;
    if constexpr (!STAGED) {
        DirectSink<SECONDS> sink = {o, 0};
        Lane<int64_t> l = lane_start<int64_t>(start, start.post);
#pragma unroll
        for (int k = 0; k < RAW_ITEMS; ++k)
            if (k < nv) Format<FMT>::walk_word(l, w[k], sink);
        bad = sink.bad;
    } else {
        // rounds of RAW_STAGE events through LDS, so that the column stores of a round are contiguous; a lane walks its words in
        // every round its events reach into
        __shared__ Stage stage;
        const int64_t out0 = chunk.post, out1 = combine<FMT>(chunk, sums[blockIdx.x]).post;
        const int64_t my0 = start.post, my1 = combine<FMT>(start, mine).post;
        for (int64_t r0 = out0; r0 < out1; r0 += RAW_STAGE) {
            if (my0 < r0 + RAW_STAGE && my1 > r0) {
                StageSink sink = {stage};
                Lane<int> l = lane_start<int>(start, (int)(my0 - r0));     // (a lane holds at most 12 RAW_ITEMS events)
#pragma unroll
                for (int k = 0; k < RAW_ITEMS; ++k)
                    if (k < nv) Format<FMT>::walk_word(l, w[k], sink);
            }
            __syncthreads();
            const int64_t left = (out1 < o.total ? out1 : o.total) - r0;
            const int cnt = left < RAW_STAGE ? (int)left : RAW_STAGE;
            for (int k = threadIdx.x; k < cnt; k += EVK_BLOCK)
                bad += store_event<SECONDS>(o, r0 + k, (uint16_t)stage.x[k], (uint16_t)stage.y[k], stage.t[k], stage.p[k]);
            __syncthreads();
        }
    }
    if (o.w) {                                       // (uniform) one atomic per workgroup
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
        if (lane == 0) s_bad[wave] = bad;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
#pragma unroll
            for (int k = 0; k < RAW_WAVES; ++k) t += s_bad[k];
            if (t) __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(result + 5), (unsigned long long)t,
                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

static int64_t raw_chunks(int64_t n) { return (n + RAW_CHUNK - 1) / RAW_CHUNK; }
static int64_t raw_sums_bytes(int64_t nc) { return ((int64_t)sizeof(Sum32) * nc + 255) / 256 * 256; }

struct RawCol {
    const uint32_t *base32;
    int half;
};
// the column's dword-rounded start; false when it is not aligned to its words
static bool raw_column(const void *words, int format, RawCol &c) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(words);
    if (a & (format == EVK_RAW_EVT3 ? 1u : 3u)) return false;
    c.base32 = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    c.half = (int)((a & 2u) >> 1);
    return true;
}

template <int FMT>
static void raw_plan(const RawCol &c, int64_t n, const int64_t *state_in, Sum32 *sums, Sum64 *starts, int64_t *result,
                     int64_t *state_out, hipStream_t s) {
    const int64_t nc = raw_chunks(n);
    if (nc) k_raw_sum<FMT><<<(unsigned)nc, EVK_BLOCK, 0, s>>>(c.base32, c.half, n, sums);
    k_raw_scan<FMT><<<1, EVK_BLOCK, 0, s>>>(sums, nc, state_in, starts, result, state_out);
}

template <int FMT, bool SECONDS>
static void raw_write(const RawCol &c, int64_t n, const Sum32 *sums, const Sum64 *starts, const RawOut &o, int64_t *result,
                      bool direct, hipStream_t s) {
    const unsigned nc = (unsigned)raw_chunks(n);
    if (direct) k_raw_write<FMT, SECONDS, false><<<nc, EVK_BLOCK, 0, s>>>(c.base32, c.half, n, sums, starts, o, result);
    else k_raw_write<FMT, SECONDS, true><<<nc, EVK_BLOCK, 0, s>>>(c.base32, c.half, n, sums, starts, o, result);
}

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_raw_decode_scratch_bytes(int64_t n_words) {
    if (n_words < 0 || n_words > EVK_RAW_MAX_WORDS) return EVK_EINVAL;
    const int64_t nc = raw_chunks(n_words);
    return raw_sums_bytes(nc) + (int64_t)sizeof(Sum64) * nc + 256;
}

static bool raw_head_ok(const void *words, int64_t n, int format, void *scratch, int64_t scratch_bytes, RawCol &c, int &rc) {
    rc = EVK_EINVAL;
    if (n < 0 || n > EVK_RAW_MAX_WORDS || (n > 0 && !words) || !scratch || (format != EVK_RAW_EVT3 && format != EVK_RAW_EVT2) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15u))
        return false;
    c = RawCol{nullptr, 0};
    if (n > 0 && !raw_column(words, format, c)) return false;
    rc = EVK_ESCRATCH;
    return scratch_bytes >= evk_raw_decode_scratch_bytes(n);
}

extern "C" int evk_raw_decode_plan(const void *words, int64_t n_words, int format, const int64_t *state_in, void *scratch,
                                   int64_t scratch_bytes, int64_t *result, int64_t *state_out, void *stream) {
    RawCol c;
    int rc;
    if (!result || !state_out) return EVK_EINVAL;
    if (!raw_head_ok(words, n_words, format, scratch, scratch_bytes, c, rc)) return rc;
    Sum32 *sums = static_cast<Sum32 *>(scratch);
    Sum64 *starts = reinterpret_cast<Sum64 *>(static_cast<char *>(scratch) + raw_sums_bytes(raw_chunks(n_words)));
    hipStream_t s = (hipStream_t)stream;
    if (format == EVK_RAW_EVT3) raw_plan<EVK_RAW_EVT3>(c, n_words, state_in, sums, starts, result, state_out, s);
    else raw_plan<EVK_RAW_EVT2>(c, n_words, state_in, sums, starts, result, state_out, s);
    return launch_status();
}

extern "C" int evk_raw_decode_write(const void *words, int64_t n_words, int format, void *scratch, int64_t scratch_bytes,
                                    int64_t *result, int16_t *xs, int16_t *ys, void *ts, uint8_t *ps, int ts_kind, int sensor_h,
                                    int sensor_w, uint32_t flags, void *stream) {
    RawCol c;
    int rc;
    if (!result || (ts_kind != EVK_RAW_TS_US && ts_kind != EVK_RAW_TS_SECONDS) || sensor_h < 0 || sensor_w < 0 ||
        sensor_h > 65535 || sensor_w > 65535 || (sensor_h == 0) != (sensor_w == 0) || (flags & ~(uint32_t)EVK_RAW_DIRECT_STORES))
        return EVK_EINVAL;
    if (!raw_head_ok(words, n_words, format, scratch, scratch_bytes, c, rc)) return rc;
    if (n_words == 0) return EVK_OK;
    // (with no event the output columns may be NULL: no position below the total exists)
    const Sum32 *sums = static_cast<const Sum32 *>(scratch);
    const Sum64 *starts = reinterpret_cast<const Sum64 *>(static_cast<const char *>(scratch) + raw_sums_bytes(raw_chunks(n_words)));
    const RawOut o = {xs, ys, ts, ps, 0, (uint32_t)sensor_w, (uint32_t)sensor_h};
    const bool direct = flags & EVK_RAW_DIRECT_STORES;
    hipStream_t s = (hipStream_t)stream;
    if (format == EVK_RAW_EVT3) {
        if (ts_kind == EVK_RAW_TS_US) raw_write<EVK_RAW_EVT3, false>(c, n_words, sums, starts, o, result, direct, s);
        else raw_write<EVK_RAW_EVT3, true>(c, n_words, sums, starts, o, result, direct, s);
    } else {
        if (ts_kind == EVK_RAW_TS_US) raw_write<EVK_RAW_EVT2, false>(c, n_words, sums, starts, o, result, direct, s);
        else raw_write<EVK_RAW_EVT2, true>(c, n_words, sums, starts, o, result, direct, s);
    }
    return launch_status();
}
