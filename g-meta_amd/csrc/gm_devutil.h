// Small device helpers that more than one translation unit needs bit for bit: the hash and salt behind every random word of the library (extract.hip's node
// sampling, negatives.hip's candidate stream), the search of a sorted list of pair keys (negatives.hip, holdout.hip) and the word access of a membership bitmap that lives in LDS or in HBM (extract.hip, candidates.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// oracle.lowbias32 / oracle.sample_salt
__host__ __device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ uint32_t sample_salt(uint64_t seed, int g, int i, int j) {
    uint32_t s = lowbias32((uint32_t)(seed & 0xffffffffu) ^ 0x9E3779B9u);
    s = lowbias32(s ^ (uint32_t)(seed >> 32));
    s = lowbias32(s + (uint32_t)g * 0x85EBCA6Bu);
    s = lowbias32(s ^ (uint32_t)i);
    s = lowbias32(s + (uint32_t)(j + 1) * 0xC2B2AE35u);
    return s;
}

// key in the ascending list keys[0 .. n) of canonical pair keys u * N + v (int64): the exclusion list of negatives.hip, the removal lists of holdout.hip
__device__ __forceinline__ bool gm_key_listed(const int64_t* keys, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t x = keys[mid];
        if (x == key) return true;
        if (x < key) lo = mid + 1; else hi = mid;
    }
    return false;
}

// Bitmap words live in LDS (G = false) or, for parent graphs too large for it, in a per-workgroup slab of global memory
// (G = true).  In the global case every word access is an agent-scope relaxed atomic: the bits are set with L2 atomics, and a
// CU's L1 is not coherent with those, so plain loads could return stale words.
template <bool G> __device__ __forceinline__ uint32_t wld(const uint32_t* p) {
    if (G) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool G> __device__ __forceinline__ void wst(uint32_t* p, uint32_t v) {
    if (G) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
