// Arrival protocol of a hub row split over P parts (agg.hip's hub blocks, agg_stream.hip's hub waves; part table and counters: gm_agg_schedule).
//
// Every part writes its partial row to its own row of the scratch matrix with agg_hub_publish -- write-through (sc1) 16-byte stores, acknowledged by
// the writer's L2 -- and drains them (agg_hub_drain, every wave that published).  Then ONE lane per part takes a relaxed agent-scope ticket
// (agg_hub_arrive).  Only the last part to arrive goes on: it puts the counter back to 0 for the next launch, does one agent-scope acquire and reads
// the P partial rows with plain loads, summing them in part order (deterministic whatever the arrival order).  Correct wherever the parts run; the
// schedules keep the parts of a row on one XCD because that is faster, and the protocol has only ever been exercised that way.
// What orders the publishing waves before the ticket and hands the result to the other lanes is the caller's: __syncthreads and an LDS flag for a
// block of several waves, readfirstlane for a single wave.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void agg_hub_publish(float* dst, const float4 v) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v val = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(dst), "v"(val) : "memory");
}
__device__ __forceinline__ void agg_hub_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// one lane per part; true: this part is the last of the row's P to arrive (the partial rows of all P are visible to the caller's loads)
__device__ __forceinline__ bool agg_hub_arrive(int* ctr, const int P) {
    const int old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == P - 1) {
        __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    return old == P - 1;
}
