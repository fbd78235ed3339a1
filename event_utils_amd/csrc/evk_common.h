// Shared device helpers for libevk (gfx950 / CDNA4 only; wavefront = 64).
// Build flags that matter for parity (see csrc/build.py): -ffp-contract=off (the reference evaluates
// x - dt*v, w*(1-dx)*(1-dy), ... as separate roundings; a fused multiply-add would change per-event values) and
// -munsafe-fp-atomics (hardware global_atomic_add_f32/f64 and ds_add_f32 instead of CAS loops; the outputs are
// ordinary hipMalloc'ed device memory, never fine-grained host memory).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/evk.h"

#define EVK_WAVE 64
#define EVK_BLOCK 256
#define EVK_NUM_CU 256

namespace evk {

__device__ __forceinline__ void atomic_add(float *p, float v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void atomic_add(double *p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void atomic_add(int32_t *p, int32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void count_oob(uint32_t *oob) {
    if (oob) __hip_atomic_fetch_add(oob, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Wave scans on DPP: the adds read their neighbour lane through the VALU's data-parallel-primitive path -- no LDS
// instruction, where __shfl_up is a ds_bpermute_b32 and a wait for the LDS queue per step.  ALL 64 LANES MUST BE ACTIVE at
// the call (wave-uniform control flow): a lane whose source lane is switched off adds 0 instead of that lane's value.  Call
// sites inside divergent code keep __shfl.  (old = 0, bound_ctrl = false: a lane without a source -- the first lanes of a
// row, a row left out by the row mask -- adds 0.)
#define EVK_DPP_ADD(v, ctrl, rows) ((v) + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rows), 0xf, false))
// inclusive scan over the rows of 16 lanes: lanes 16 r .. 16 r + 15 each hold a scan of their own
__device__ __forceinline__ uint32_t wave_incl_scan16_u32(uint32_t v) {
    v = EVK_DPP_ADD(v, 0x111, 0xf);   // row_shr:1
    v = EVK_DPP_ADD(v, 0x112, 0xf);   // row_shr:2
    v = EVK_DPP_ADD(v, 0x114, 0xf);   // row_shr:4
    v = EVK_DPP_ADD(v, 0x118, 0xf);   // row_shr:8
    return v;
}
// inclusive scan over the 64 lanes
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
    v = wave_incl_scan16_u32(v);
    v = EVK_DPP_ADD(v, 0x142, 0xa);   // row_bcast:15 into rows 1 and 3: the total of the row below
    v = EVK_DPP_ADD(v, 0x143, 0xc);   // row_bcast:31 into rows 2 and 3: the total of lanes 0..31
    return v;
}
// lane `l`'s value to every lane, through a scalar register; `l` a constant or wave-uniform (made so with
// __builtin_amdgcn_readfirstlane where the compiler cannot see it, e.g. the wave's number threadIdx.x >> 6)
__device__ __forceinline__ uint32_t wave_bcast_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// 4 consecutive elements of a column, as one (float) or two (double) 16-byte loads per lane.
template <typename T>
struct Vec4 {
    T v[4];
};
template <typename T>
__device__ __forceinline__ Vec4<T> load4(const T *p, int64_t i4) {
    Vec4<T> r;
    if constexpr (sizeof(T) == 4) {
        const uint4 q = reinterpret_cast<const uint4 *>(p)[i4];
        uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) r.v[k] = __builtin_bit_cast(T, u[k]);
    } else {
        const double2 a = reinterpret_cast<const double2 *>(p)[2 * i4];
        const double2 b = reinterpret_cast<const double2 *>(p)[2 * i4 + 1];
        double d[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
        for (int k = 0; k < 4; ++k) r.v[k] = __builtin_bit_cast(T, d[k]);
    }
    return r;
}

// A column of one of the five EVK_SELECT_* kinds (evk.h).  Host: f(the typed pointer), f a generic lambda -- the one switch
// behind every launcher that is a template of the column's element type.  Device: element i as a double (exact for every kind
// but int64 beyond 2^53), a switch on the wave-uniform kind.
template <class F>
static void with_time_kind(int kind, const void *t, F f) {
    switch (kind) {
        case EVK_SELECT_I16: f(static_cast<const int16_t *>(t)); break;
        case EVK_SELECT_I32: f(static_cast<const int32_t *>(t)); break;
        case EVK_SELECT_I64: f(static_cast<const int64_t *>(t)); break;
        case EVK_SELECT_F32: f(static_cast<const float *>(t)); break;
        default: f(static_cast<const double *>(t)); break;
    }
}
__device__ __forceinline__ double ts_time(const void *t, int kind, uint32_t i) {
    switch (kind) {
        case EVK_SELECT_I16: return (double)static_cast<const int16_t *>(t)[i];
        case EVK_SELECT_I32: return (double)static_cast<const int32_t *>(t)[i];
        case EVK_SELECT_I64: return (double)static_cast<const int64_t *>(t)[i];
        case EVK_SELECT_F32: return (double)static_cast<const float *>(t)[i];
        default: return static_cast<const double *>(t)[i];
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// columns of the one-pass entry points: 16-byte aligned, or -- with EVK_COLUMNS_UNALIGNED (evk.h) in `flags` -- aligned to their
// element (4 bytes; 8 for int64 pixels): the kernels' 16-byte loads are dword-aligned loads (evk_part.h, load_col16)
inline bool column_ok(const void *p, int flags, unsigned elem = 4) {
    return (reinterpret_cast<uintptr_t>(p) & ((flags & EVK_COLUMNS_UNALIGNED) ? elem - 1u : 15u)) == 0;
}

// Streaming launch shape: enough 256-thread blocks to fill 256 CUs x 8 blocks, grid-stride beyond that.
inline int stream_grid(int64_t work_items, int per_thread = 1) {
    int64_t blocks = (work_items + (int64_t)EVK_BLOCK * per_thread - 1) / ((int64_t)EVK_BLOCK * per_thread);
    if (blocks < 1) blocks = 1;
    const int64_t cap = (int64_t)EVK_NUM_CU * 8;
    return (int)(blocks < cap ? blocks : cap);
}

inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? EVK_OK : (int)e;
}

}  // namespace evk
