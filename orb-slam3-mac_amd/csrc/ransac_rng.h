// The counter-based generator behind the device-drawn RANSAC sets (tvr_kernels.hip, sim3solver_kernels.hip): a splitmix64 finaliser
// keyed by (seed, pair, iteration, draw) and a draw of floor(u * avail) from its upper 32 bits.  No state: a pair draws the same sets
// alone and inside a batch.
#ifndef ORBHIP_RANSAC_RNG_H
#define ORBHIP_RANSAC_RNG_H
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long ransac_mix(unsigned long long x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// draw j of iteration it of pair `pair`: uniform in [0, avail)
__device__ __forceinline__ int ransac_draw(unsigned long long seed, int pair, int it, int j, unsigned avail)
{
    const unsigned long long h = ransac_mix(ransac_mix(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(pair + 1)) +
                                            0xD1B54A32D192ED03ull * (unsigned long long)(it + 1) + 0x8CB92BA72F3D8DD7ull * (unsigned long long)(j + 1));
    return (int)(((h >> 32) * (unsigned long long)avail) >> 32);
}
#endif
