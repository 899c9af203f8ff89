// match_common.h -- the rules every ORBmatcher search shares (reference src/ORBmatcher.cc): the two constants, the rotation-consistency
// check (the `rot` / `bin` lines of every search and ComputeThreeMaxima, :2307-2348) and the FeatureVector of a frame as the kernels
// read it.  Included by search_init_kernels.hip, match_kernels.hip (SearchByProjection), bow_kernels.hip and tri_kernels.hip.  The functions are
// force-inlined device code; what a kernel clears when a bin is dropped, and its barriers, stay in the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TH_LOW 50             // ORBmatcher::TH_LOW  (ORBmatcher.cc:41)
#define HISTO_LENGTH 30       // ORBmatcher::HISTO_LENGTH (ORBmatcher.cc:42)

// Histogram bin of the rotation between two matched keypoints: rot = a - b, + 360 when negative, bin = round(rot * (1 / HISTO_LENGTH)),
// bin HISTO_LENGTH wraps to 0.  One rounding per operation, whatever contraction the including file has set.
__device__ __forceinline__ int rot_bin(float angle_a, float angle_b)
{
    float rot = __fsub_rn(angle_a, angle_b);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, 1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ComputeThreeMaxima (ORBmatcher.cc:2307-2348) over the bin counts: keep[0..2] = the three fullest bins, the first of equal counts
// ahead; the second and third are dropped (-1) when they hold less than a tenth of the first.  One thread executes it.
// This and rot_kept are macros, not functions: the compiler simplifies and unrolls a function on its own before it inlines it, and the
// kernels then come out 10 to 12 instructions longer with their registers allocated differently; expanded in place they compile to the
// instruction stream they had when each kernel wrote the scan out itself (profiles/refactor_match_streams.txt).
#define rot_three_maxima(hist, keep) do { \
    int max1_ = 0, max2_ = 0, max3_ = 0, ind1_ = -1, ind2_ = -1, ind3_ = -1; \
    for (int i_ = 0; i_ < HISTO_LENGTH; i_++) { \
        const int sz_ = (hist)[i_]; \
        if (sz_ > max1_) { max3_ = max2_; max2_ = max1_; max1_ = sz_; ind3_ = ind2_; ind2_ = ind1_; ind1_ = i_; } \
        else if (sz_ > max2_) { max3_ = max2_; max2_ = sz_; ind3_ = ind2_; ind2_ = i_; } \
        else if (sz_ > max3_) { max3_ = sz_; ind3_ = i_; } \
    } \
    if ((float)max2_ < __fmul_rn(0.1f, (float)max1_)) { ind2_ = -1; ind3_ = -1; } \
    else if ((float)max3_ < __fmul_rn(0.1f, (float)max1_)) ind3_ = -1; \
    (keep)[0] = ind1_; (keep)[1] = ind2_; (keep)[2] = ind3_; \
} while (0)

// does a match of this bin survive the check?  (bin: a plain variable, it is read three times)
#define rot_kept(bin, keep) ((bin) == (keep)[0] || (bin) == (keep)[1] || (bin) == (keep)[2])

// DBoW2 FeatureVector of the frames of a batch, flattened: per frame the node ids ascending [max_nodes], the first entry of every
// node in feat [max_nodes + 1], the feature indices node by node [max_n], and the number of nodes.
struct FeatVec { const int32_t *node_ids, *node_start, *feat, *nnodes; };

// std::lower_bound of a node id in a frame's ascending node list (FeatureVector::lower_bound, ORBmatcher.cc:435-442): the first
// position whose id is not below nid, n when there is none
__device__ __forceinline__ int node_lower_bound(const int32_t *ids, int n, int nid)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < nid) lo = mid + 1; else hi = mid; }
    return lo;
}
