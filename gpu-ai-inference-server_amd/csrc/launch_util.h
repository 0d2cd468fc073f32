// Host-side helpers that more than one kernel file's launcher or eligibility check needs (kernels.h stays the interface to the executor).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "kernels.h"

namespace ie {

inline bool Aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// A map the 16-byte channel-vector kernels can address (V = 4 floats / 8 halfs): channels contiguous, whole vectors per pixel, every
// pitch a multiple of the vector, the base 16-byte aligned.  A kernel that needs more (dense rows, a single row) adds it at its call site.
inline bool VecViewOk(const TensorArg& t, int V) {
    return t.sc == 1 && t.c % V == 0 && t.sw % V == 0 && t.sh % V == 0 && t.sn % V == 0 && Aligned16(t.p);
}

// No gap between the pixel rows of an image nor between images: the n * h * w pixels lie one pitch (sw) apart through the whole tensor
inline bool RowsDense(const TensorArg& t) { return t.sh == int64_t(t.w) * t.sw && t.sn == int64_t(t.h) * t.sh; }

// Compute units of the current device, cached per device id (ids past the array are queried every time); 0: the query failed.
inline int DeviceCus() {
    static std::atomic<int> cache[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    const bool cached = dev >= 0 && dev < int(sizeof(cache) / sizeof(cache[0]));
    int cus = cached ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (cus == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        cus = prop.multiProcessorCount;
        if (cached) cache[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

}  // namespace ie
