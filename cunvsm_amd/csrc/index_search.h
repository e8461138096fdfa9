// The binary search of the postings kernels (index.hip, sdm.hip): a term's documents ascend, a posting's positions ascend.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cunvsm {

// first index in [lo, hi) whose value is >= key; hi when there is none
template <typename T, typename K>
__device__ __forceinline__ int64_t index_lower_bound(const T* __restrict__ a, int64_t lo, int64_t hi, K key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (static_cast<K>(a[mid]) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace cunvsm
