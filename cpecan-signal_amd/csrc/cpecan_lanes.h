/*
 * cpecan_lanes.h -- the lane-level helpers the two families of throughput kernels (cpecan_kernel_wave.hip,
 * cpecan_kernel_systolic.hip) have in common.  File-local in each of them, like their other helpers: a sweep file
 * includes this once, and no name of a build's device code depends on which file a helper was typed in.
 */
#ifndef CPECAN_LANES_H_
#define CPECAN_LANES_H_

#include "cpecan_device.h"

namespace {

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uni64(long long v) {
    const unsigned lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) v);
    const int hi = __builtin_amdgcn_readfirstlane((int) (v >> 32));
    return ((long long) hi << 32) | lo;
}
__device__ __forceinline__ double bcast(double v, int srcLane) { /* srcLane wave-uniform */
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), srcLane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), srcLane);
    return __hiloint2double(hi, lo);
}

/* a load that cannot be served from a line this CU cached before another wave (or an earlier phase
 * of the same workgroup) rewrote it */
template <typename V> __device__ __forceinline__ V ld_agent(V *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* the four cubics [c3,c2,c1,c0] of lookup() (impl/pairwiseAligner.c:238-249: d <= 1, <= 2.5, <= 4.5, else), float
 * literals as there; a sweep's init_coef spreads them over the LDS table its ladd reads by n = ceil(2d) */
#define CP_LOOKUP_CUBICS                                                                            \
    { -0.009350833524763f, 0.130659527668286f, 0.498799810682272f, 0.693203116424741f,              \
      -0.014532321752540f, 0.139942324101744f, 0.495635523139337f, 0.692140569840976f,              \
      -0.004605031767994f, 0.063427417320019f, 0.695956496475118f, 0.514272634594009f,              \
      -0.000458661602210f, 0.009695946122598f, 0.930734667215156f, 0.168037164329057f }

/* log N(x; mu, sd) = K + (-0.5*a*a), a = (x-mu)/sd (impl/stateMachine.c:333-343); the quotient is
 * q + fma(-q, sd, t) * rsd with q = t*rsd, rsd = RN(1/sd): Markstein's correction step, which
 * rounds to the same double as the division.  sd == 0 rows carry rsd = 0, K = -inf => -inf. */
__device__ __forceinline__ double lgauss(double x, double mu, double sd, double rsd, double K) {
    const double t = x - mu;
    const double q = t * rsd;
    const double rem = __fma_rn(-q, sd, t);
    const double a = __fma_rn(rem, rsd, q);
    return K + (-0.5 * a * a);
}

/* where an alignment's results go, and how many there are so far */
struct ItemOut {
    long long *pairs;
    double *logp;
    long long pairCap;
    long long *totXay;
    double *totVal;
    long long totCap;
    long long nPairs, nTot;
};

} // namespace

#endif
