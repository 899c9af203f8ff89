// ransac_common.h -- what the three hypothesise-and-verify solvers (tvr_kernels.hip, sim3solver_kernels.hip, mlpnp_kernels.hip) share:
//   ransac_mix / ransac_draw      the counter-based generator behind the device-drawn sets: a splitmix64 finaliser keyed by (seed, item,
//                                 iteration, draw) and a draw of floor(u * avail) from its upper 32 bits.  No state: an item draws the same
//                                 sets alone and inside a batch
//   ransac_draw_set<K>            K draws without replacement from 0..n-1 (the reference's swap-with-last on its index vector)
//   ransac_iteration_budget       mRansacMaxIts of SetRansacParameters (Sim3Solver.cc:126-150, MLPnPsolver.cpp:229-248), saturated at the cap
//   ransac_wave_count             inliers among n items counted by a whole wave: ballot + popcount
//   RansacCam / ransac_cam        GeometricCamera::mvParameters in float, from an orbhip_sim3_camera
//   ransac_check_capacity         the size rule of the three device entry points
// The first four are host + device (RANSAC_HD, as mlpnp_core.h's MLPNP_HD) so that tests/ransac_common_check.cc can build them into a
// stand-alone CPU program; what needs the wave or the library's own headers is compiled by hipcc only.
#ifndef ORBHIP_RANSAC_COMMON_H
#define ORBHIP_RANSAC_COMMON_H
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RANSAC_HD __host__ __device__ __forceinline__
#define RANSAC_UNROLL _Pragma("unroll")
#else
#define RANSAC_HD inline
#define RANSAC_UNROLL
#endif

RANSAC_HD unsigned long long ransac_mix(unsigned long long x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// draw j of iteration it of pair `pair`: uniform in [0, avail)
RANSAC_HD int ransac_draw(unsigned long long seed, int pair, int it, int j, unsigned avail)
{
    const unsigned long long h = ransac_mix(ransac_mix(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(pair + 1)) +
                                            0xD1B54A32D192ED03ull * (unsigned long long)(it + 1) + 0x8CB92BA72F3D8DD7ull * (unsigned long long)(j + 1));
    return (int)(((h >> 32) * (unsigned long long)avail) >> 32);
}

// set[0..K) of iteration `it` of item `item`: K draws without replacement from 0..n-1, the drawn slot refilled with the last one (a partial
// Fisher-Yates).  Only the (at most K) moved slots are held: pos[k] is a slot whose content is no longer its own index, val[k] what it
// holds; -1 marks an entry that a later draw of the same slot has superseded.  n < K: no set can be drawn, K times -1.
template <int K>
RANSAC_HD void ransac_draw_set(unsigned long long seed, int item, int it, int n, int32_t *set)
{
    if (n < K) {
        RANSAC_UNROLL
        for (int j = 0; j < K; j++) set[j] = -1;
        return;
    }
    int pos[K], val[K];
    RANSAC_UNROLL
    for (int j = 0; j < K; j++) {
        const unsigned avail = (unsigned)(n - j);
        const int r = ransac_draw(seed, item, it, j, avail);
        const int last = (int)avail - 1;
        int v = r, lv = last;
        RANSAC_UNROLL
        for (int k = 0; k < j; k++) { if (pos[k] == r) v = val[k]; if (pos[k] == last) lv = val[k]; }
        set[j] = v;
        bool found = false;
        RANSAC_UNROLL
        for (int k = 0; k < j; k++) if (pos[k] == r) { val[k] = lv; found = true; }
        pos[j] = found ? -1 : r; val[j] = lv;
    }
}

// mRansacMaxIts for n items of which nmin must be inliers: 0 for n < nmin (iterate() answers bNoMore at once), 1 for n == nmin, else
// ceil(log(1 - p) / log(1 - epsilon^3)) in [1, cap].  epsilon is a float and its cube a double, as in the reference; the reference converts
// the quotient to int unchecked, beyond the cap it saturates here.
RANSAC_HD int ransac_iteration_budget(int n, int nmin, float epsilon, double probability, int cap)
{
    int budget = 0;
    if (n >= nmin) {
        if (nmin == n) budget = 1;
        else {
            const double q = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
            budget = q < (double)cap ? (int)q : cap;
        }
        budget = budget < cap ? budget : cap;
        budget = budget > 1 ? budget : 1;
    }
    return budget;
}

#ifdef __HIPCC__
#include "ctx_internal.h"

// how many of the items 0..n-1 satisfy pred(i), counted by the whole wave (lane = 0..63); FLAGS: also written to flags_row[]
template <bool FLAGS, class Pred>
__device__ __forceinline__ int ransac_wave_count(int n, int lane, uint8_t *flags_row, Pred pred)
{
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            in = pred(i);
            if (FLAGS) flags_row[i] = in ? 1 : 0;
        }
        cnt += (int)__popcll(__ballot(in));
    }
    return cnt;
}

// fx fy cx cy k1 k2 k3 k4 as tri_project / tri_unproject (cam_project_f32.h) take them; type 0 Pinhole, 1 KannalaBrandt8
struct RansacCam { float p[8]; int type; };
inline RansacCam ransac_cam(const orbhip_sim3_camera &c)                       // mvParameters are float
{
    RansacCam r;
    r.p[0] = (float)c.fx; r.p[1] = (float)c.fy; r.p[2] = (float)c.cx; r.p[3] = (float)c.cy;
    for (int k = 0; k < 4; k++) r.p[4 + k] = c.camera_model ? (float)c.kb[k] : 0.f;
    r.type = c.camera_model;
    return r;
}

// the capacity rule of the three solvers: at most 8192 items per row and 1024 iterations (k_s3s_decide packs (count, iteration) as
// count * 1024 + iteration).  `msg` is RANSAC_CAPACITY_MSG(entry point, what max_n counts): the last error when the rule fails
#define RANSAC_CAPACITY_MSG(fn, what) fn ": at most 8192 " what " and 1024 iterations"
inline int ransac_check_capacity(int max_n, int iterations, const char *msg)
{
    if (max_n <= 8192 && iterations <= 1024) return ORBHIP_OK;
    orbhip_set_last_error_internal(msg);
    return ORBHIP_E_CAPACITY;
}
#endif
#endif
