// Grow-only device arrays of the host code (pm_context.hip, pm_flatten.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace pm {

// Room for `need` elements at *p: kept when it is there, else the old buffer is released FIRST (hipFree waits for the device:
// nothing is using it any more) and `want` elements are allocated.  After a failed allocation there is no buffer and no capacity.
template <typename T>
hipError_t Grow(T **p, size_t *cap, size_t need, size_t want) {
    if (need <= *cap && *p) return hipSuccess;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc(p, want * sizeof(T));
    if (e == hipSuccess) *cap = want;
    return e;
}
// ... with a quarter of headroom: what grows once tends to grow again
template <typename T>
hipError_t Grow(T **p, size_t *cap, size_t need) {
    return Grow(p, cap, need, need + (need >> 2) + 16);
}

template <typename T>
struct DevArray {
    T *p = nullptr;
    size_t cap = 0;  // elements
    hipError_t Reserve(size_t need) { return Grow(&p, &cap, need); }
    hipError_t Reserve(size_t need, size_t want) { return Grow(&p, &cap, need, want); }
    void Free() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace pm
