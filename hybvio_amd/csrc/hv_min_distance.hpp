// The distance test of FeatureDetector::applyMinDistance (feature_detector_legacy.cpp:177-213), shared by detect_tail.hip (GPU-GFTT
// tail, applyMinDistance on lists) and fast.hip (FAST tail), and wave_sync(), the in-wave ordering of detect_tail.hip's ballot walks.
// fast.hip deliberately does not call wave_sync(): its wavefront-private LDS exchanges (queue, counters, accepted list) go through
// volatile pointers with a wave_barrier, because the fences below also wait for the global stores its loops keep in flight.
#pragma once
#include <hip/hip_runtime.h>

namespace hv {

// the reference's binary32 expression, two rounded products and one rounded sum, strict `<` against (float)(r * r): the library is
// built with -ffp-contract=off and the function also switches contraction off itself
__device__ __forceinline__ bool within(float ax, float ay, float bx, float by, float r2)
{
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by;
    const float xx = dx * dx, yy = dy * dy;
    return xx + yy < r2;
}

// orders the LDS accesses of one wavefront (the hardware runs them in issue order; this keeps the compiler from moving them)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace hv
