// The fence-free hand-over between the workgroups of ONE launch, stated once: the partition's ticket (evk_part2.h), the pieces
// of a cut tile (evk_voxel2.hip, evk_image2.hip, evk_tiled.hip), the host publish of a result.
//
//   every workgroup:  agent-scope stores / atomics of what it hands over
//                     EVK_HANDOVER_DRAIN()          every wave waits for its own (vmcnt(0)), workgroup barrier
//                     last_arriver(counter, ..)     one lane takes a relaxed agent-scope ticket, barrier
//   the last arriver: reads what the others wrote with agent-scope loads (sum_pieces)
//
// There is NO release / acquire fence in it: everything the receiving side reads was written with agent- (or system-) scope
// atomics, which on gfx950 are performed at the level all XCDs share and complete -- vmcnt -- only then, and are never served
// from a stale line of the reader's L2; every wave has drained its own before the workgroup's ticket.  A fence there is a
// write-back (and an invalidate) of the XCD's whole L2 with everything the other workgroups have just stored in it: 4.5 us of
// the 47 us partition kernel, 48.7 -> 46.3 us for the tile kernel on the blob scene (DESIGN.md section 3, K1').
// It is correct only AS A WHOLE -- the ticket behind the drain, the payload and its reads agent-scope on both sides, the
// counter back at zero before the next launch -- and only on gfx9-family memory pipelines (one counter, vmcnt, covering loads,
// stores and atomics): refuse to compile the device code for anything else.  -DEVK_SAFE_HANDOVER puts the textbook fences back
// (release before the ticket, acquire after it) so that the parity tests can be run with both forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "libevk's fence-free hand-overs assume a gfx9-family memory pipeline (built and validated for gfx950 only)"
#endif
#ifdef EVK_SAFE_HANDOVER
#define EVK_HANDOVER_RELEASE() __atomic_thread_fence(__ATOMIC_RELEASE)   /* (HIP: agent scope) */
#define EVK_HANDOVER_ACQUIRE() __atomic_thread_fence(__ATOMIC_ACQUIRE)
#else
#define EVK_HANDOVER_RELEASE() do {} while (0)
#define EVK_HANDOVER_ACQUIRE() do {} while (0)
#endif
// every wave drains its own stores / atomics, [fence], workgroup barrier: what precedes a ticket.  (A call of its own, so that
// a workgroup can still store a word -- the partition's live progress -- between the drain and its ticket.)
#define EVK_HANDOVER_DRAIN()                              \
    do {                                                  \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  \
        EVK_HANDOVER_RELEASE();                           \
        __syncthreads();                                  \
    } while (0)

namespace evk {

// The ticket: true, in every thread of the workgroup, for the last of the `expected` workgroups to arrive at `counter`
// (whole workgroup, behind EVK_HANDOVER_DRAIN).  `expected`: a number, or a callable giving it, which only the lane with the
// ticket evaluates, behind its atomic (the partition passes gridDim.x so: a kernel argument load that need not be waited for
// ahead of the ticket).  `reset`: the last arriver leaves the counter zero for the next launch; a caller that passes false
// does so itself, later.
template <typename Count>
__device__ __forceinline__ bool last_arriver(uint32_t *counter, Count expected, bool reset) {
    __shared__ int is_last;
    if (threadIdx.x == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (std::is_integral<Count>::value) is_last = (prev == expected - 1);
        else is_last = (prev == expected() - 1);
        if (reset && is_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (is_last) EVK_HANDOVER_ACQUIRE();
    return is_last != 0;
}

// Cell `c` of a cut tile: the sum of its `nparts` pieces, `stride` elements apart, IN PART ORDER -- a float sum then does
// not depend on which piece arrived last -- with agent-scope loads (above).  seen(v) looks at every piece's value.
template <typename T, typename Seen>
__device__ __forceinline__ T sum_pieces(const T *parts, int64_t stride, uint32_t nparts, int64_t c, Seen seen) {
    T sum = 0;
    for (uint32_t p = 0; p < nparts; ++p) {
        const T v = __hip_atomic_load(parts + (int64_t)p * stride + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seen(v);
        sum += v;
    }
    return sum;
}
template <typename T>
__device__ __forceinline__ T sum_pieces(const T *parts, int64_t stride, uint32_t nparts, int64_t c) {
    return sum_pieces(parts, stride, nparts, c, [](T) {});
}

}  // namespace evk
