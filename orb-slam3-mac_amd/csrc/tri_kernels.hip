// tri_kernels.hip -- ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:969-1210) for EVERY camera combination the
// reference supports: single Pinhole or KannalaBrandt8 cameras and two-camera rigs (mpCamera2 != 0: TUM-VI stereo-fisheye, BASELINE
// config #5).  k_search_triangulation is the Pinhole / single-camera fast path; k_search_triangulation_general is its sibling for the rest:
//   * rig keyframes: keypoints mvKeys | mvKeysRight, bRight = index >= NLeft, the relative pose and the camera pair of a candidate
//     picked from {ll, lr, rl, rr} (ORBmatcher.cc:994-1008, 1101-1130), no epipole test and no stereo keypoints (:1044, :1091);
//   * GeometricCamera::epipolarConstrain per camera type: Pinhole.cpp:122-144 (distance to the epipolar line of
//     F12 = K1^-T [t12]x R12 K2^-1, host-built per combination) or KannalaBrandt8.cpp:235-238 -> TriangulateMatches (:334-401):
//     ray parallax, linear triangulation through the SVD of a 4x4 float system (cv::SVD::compute = one-sided Jacobi, restated from
//     OpenCV 3.4.1 lapack.cpp JacobiSVDImpl_<float>: parity unpinned), positive depths, reprojection errors in both cameras.
// One thread per KF1 keypoint as in the fast path (this fork never sets vbMatched2: KF1 keypoints are independent); the Jacobi sweeps
// run in the thread's registers.  Every float expression is evaluated op by op (-ffp-contract=off) in the oracle's order; libm calls
// whose results differ between platforms are replaced on BOTH sides by fixed double sequences rounded to float (tanf, cosf, sinf:
// Cody-Waite + fdlibm kernels; atan2f: double atan2; hypot: sqrt(p^2 + beta^2)) -- the deviation DESIGN 2 states for orb_sincos.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "svd4.h"
#include "cam_project_f32.h"
#include "match_common.h"
#include <cfloat>
#include <cstring>

namespace {

// KannalaBrandt8::TriangulateMatches (KannalaBrandt8.cpp:334-401) > 0.0001f.  P3D (Frame::ComputeStereoFishEyeMatches): the depth z1 and
// p3D (left-camera point) of an accepted match go to z1_out / p3D; P3D = false (SearchForTriangulation's epipolar test, :235-238) writes
// nothing.  One template rather than a core plus a bool wrapper: the wrapper's extra call level took k_search_triangulation_general from
// 168 to 184 VGPRs (occupancy 3 -> 2, tools/kernel_resources.py).
template <bool P3D>
__device__ bool tri_kb8_triangulate(int type1, const float *cam1, int type2, const float *cam2, float u1, float v1, float u2, float v2,
                                    const float *R12, const float *t12, float sigmaLevel, float unc, float *z1_out, float *p3D)
{
    float r1[3], r2[3], r21[3];
    tri_unproject(type1, cam1, u1, v1, r1);
    tri_unproject(type2, cam2, u2, v2, r2);
#pragma unroll
    for (int i = 0; i < 3; i++) r21[i] = (float)((double)R12[3 * i] * r2[0] + (double)R12[3 * i + 1] * r2[1] + (double)R12[3 * i + 2] * r2[2]);
    const double dot = (double)r1[0] * r21[0] + (double)r1[1] * r21[1] + (double)r1[2] * r21[2];
    const double n1 = sqrt((double)r1[0] * r1[0] + (double)r1[1] * r1[1] + (double)r1[2] * r1[2]);
    const double n2 = sqrt((double)r21[0] * r21[0] + (double)r21[1] * r21[1] + (double)r21[2] * r21[2]);
    const float cosParallaxRays = (float)(dot / (n1 * n2));
    if ((double)cosParallaxRays > 0.9998) return false;
    float R21[9], t21[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R21[3 * i + j] = R12[3 * j + i];
#pragma unroll
    for (int i = 0; i < 3; i++) t21[i] = (float)(-1.0 * ((double)R21[3 * i] * t12[0] + (double)R21[3 * i + 1] * t12[1] + (double)R21[3 * i + 2] * t12[2]));
    // A (KannalaBrandt8.cpp:426-429) with Tcw1 = [I | 0], Tcw2 = [R21 | t21]; stored transposed: At[j] = column j of A
    float At[4][4], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float T1r0 = j == 0 ? 1.f : 0.f, T1r1 = j == 1 ? 1.f : 0.f, T1r2 = j == 2 ? 1.f : 0.f;
        const float T2r0 = j < 3 ? R21[j] : t21[0], T2r1 = j < 3 ? R21[3 + j] : t21[1], T2r2 = j < 3 ? R21[6 + j] : t21[2];
        At[j][0] = r1[0] * T1r2 - T1r0;
        At[j][1] = r1[1] * T1r2 - T1r1;
        At[j][2] = r2[0] * T2r2 - T2r0;
        At[j][3] = r2[1] * T2r2 - T2r1;
    }
    tri_svd4_null(At, v);
    const float inv = (float)(1.0 / (double)v[3]);
    const float x3D[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
    const float z1 = x3D[2];
    if (!(z1 > 0.f)) return false;
    const float z2 = (float)((double)R21[6] * x3D[0] + (double)R21[7] * x3D[1] + (double)R21[8] * x3D[2] + (double)t21[2]);
    if (z2 <= 0.f) return false;
    float uv1[2], uv2[2], x3D2[3];
    tri_project(type1, cam1, x3D, uv1);
    const float errX1 = uv1[0] - u1, errY1 = uv1[1] - v1;
    if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaLevel) return false;
#pragma unroll
    for (int i = 0; i < 3; i++)
        x3D2[i] = (float)((double)R21[3 * i] * x3D[0] + (double)R21[3 * i + 1] * x3D[1] + (double)R21[3 * i + 2] * x3D[2] + (double)t21[i]);
    tri_project(type2, cam2, x3D2, uv2);
    const float errX2 = uv2[0] - u2, errY2 = uv2[1] - v2;
    if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)unc) return false;
    if (P3D) { *z1_out = z1; p3D[0] = x3D[0]; p3D[1] = x3D[1]; p3D[2] = x3D[2]; }
    return z1 > 0.0001f;
}
// KannalaBrandt8::matchAndtriangulate (KannalaBrandt8.cpp:240-332): the candidate test of the SearchForTriangulation overload that
// returns the triangulated points (ORBmatcher.cc:1212-1402).  T1 / T2 = rows 0..2 of Tcw1 / Tcw2 (world -> camera, row-major 3x4) of
// the cameras the two keypoints were seen by; the first camera is a KannalaBrandt8 (the virtual call is made on it), the second any.
// Differences from TriangulateMatches: absolute poses in the linear system, no z1 > 1e-4 test, x3D is a WORLD point.
__device__ bool tri_kb8_match_and_triangulate(const float *cam1, int type2, const float *cam2, float u1, float v1, float u2, float v2,
                                              const float *T1, const float *T2, float sigmaLevel1, float sigmaLevel2, float *x3D_out)
{
    float r1[3], r2[3], ray1[3], ray2[3];
    tri_unproject(1, cam1, u1, v1, r1);
    tri_unproject(type2, cam2, u2, v2, r2);
#pragma unroll
    for (int i = 0; i < 3; i++) {                                              // Rwc = Rcw.t(); ray = Rwc * r
        ray1[i] = (float)((double)T1[i] * r1[0] + (double)T1[4 + i] * r1[1] + (double)T1[8 + i] * r1[2]);
        ray2[i] = (float)((double)T2[i] * r2[0] + (double)T2[4 + i] * r2[1] + (double)T2[8 + i] * r2[2]);
    }
    const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
    const double n1 = sqrt((double)ray1[0] * ray1[0] + (double)ray1[1] * ray1[1] + (double)ray1[2] * ray1[2]);
    const double n2 = sqrt((double)ray2[0] * ray2[0] + (double)ray2[1] * ray2[1] + (double)ray2[2] * ray2[2]);
    const float cosParallaxRays = (float)(dot / (n1 * n2));
    if ((double)cosParallaxRays > 0.9998) return false;
    // Triangulate(p11, p22, Tcw1, Tcw2, x3D) (KannalaBrandt8.cpp:422-435); stored transposed: At[j] = column j of A
    float At[4][4], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        At[j][0] = r1[0] * T1[8 + j] - T1[j];
        At[j][1] = r1[1] * T1[8 + j] - T1[4 + j];
        At[j][2] = r2[0] * T2[8 + j] - T2[j];
        At[j][3] = r2[1] * T2[8 + j] - T2[4 + j];
    }
    tri_svd4_null(At, v);
    const float inv = (float)(1.0 / (double)v[3]);
    const float x3D[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
    const float z1 = (float)((double)T1[8] * x3D[0] + (double)T1[9] * x3D[1] + (double)T1[10] * x3D[2] + (double)T1[11]);
    if (!(z1 > 0.f)) return false;
    const float z2 = (float)((double)T2[8] * x3D[0] + (double)T2[9] * x3D[1] + (double)T2[10] * x3D[2] + (double)T2[11]);
    if (!(z2 > 0.f)) return false;
    float uv1[2], uv2[2], xc[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        xc[i] = (float)((double)T1[4 * i] * x3D[0] + (double)T1[4 * i + 1] * x3D[1] + (double)T1[4 * i + 2] * x3D[2] + (double)T1[4 * i + 3]);
    tri_project(1, cam1, xc, uv1);
    const float errX1 = uv1[0] - u1, errY1 = uv1[1] - v1;
    if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaLevel1) return false;
#pragma unroll
    for (int i = 0; i < 3; i++)
        xc[i] = (float)((double)T2[4 * i] * x3D[0] + (double)T2[4 * i + 1] * x3D[1] + (double)T2[4 * i + 2] * x3D[2] + (double)T2[4 * i + 3]);
    tri_project(type2, cam2, xc, uv2);
    const float errX2 = uv2[0] - u2, errY2 = uv2[1] - v2;
    if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaLevel2) return false;
    x3D_out[0] = x3D[0]; x3D_out[1] = x3D[1]; x3D_out[2] = x3D[2];
    return true;
}

// ORBmatcher::SearchForTriangulation (ORBmatcher.cc:969-1210; Pinhole, mpCamera2 == 0) -- the matcher of
// LocalMapping::CreateNewMapPoints.  This fork never sets vbMatched2, so every KF1 keypoint is independent: one block per
// keyframe pair, one thread per KF1 keypoint, KF2's descriptors and flags LDS-resident.
struct TriLevels { float scale[16], sigma2[16]; };
#define TRI_THREADS 256
__global__ __launch_bounds__(TRI_THREADS) void k_search_triangulation(const int32_t *nid1_, const uint8_t *mp1_, const orbhip_keypoint *kp1_,
        const uint8_t *desc1_, const float *ur1_, const int32_t *n1_, FeatVec S2, const uint8_t *mp2_, const orbhip_keypoint *kp2_,
        const uint8_t *desc2_, const float *ur2_, const int32_t *n2_, const orbhip_tri_pair *geom_, int max_nodes, int max_n,
        size_t kp_stride, TriLevels lv, int check_ori, int cap_n, int32_t *matches12_, int32_t *nmatches_, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t tri_lds[];
    uint4 *dlds = reinterpret_cast<uint4 *>(tri_lds);                        // [cap_n][2] KF2 descriptors
    uint8_t *flag2 = reinterpret_cast<uint8_t *>(dlds + 2 * (size_t)cap_n);  // [cap_n] bit0: has a map point, bit1: stereo
    int8_t *bin1 = reinterpret_cast<int8_t *>(flag2 + cap_n);                // [cap_n] rotation bin of KF1 keypoint i's match
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    __shared__ int s_cnt;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n1 = n1_[pair], n2 = n2_[pair], nn2 = S2.nnodes[pair];
    int32_t *matches12 = matches12_ + (size_t)pair * max_n;
    if (n1 > cap_n || n2 > cap_n || n1 > max_n || n2 > max_n || nn2 > max_nodes) {
        if (tid == 0) { atomicExch(status, ORBHIP_E_CAPACITY); nmatches_[pair] = 0; }
        return;
    }
    const int32_t *nid1 = nid1_ + (size_t)pair * max_n;
    const uint8_t *mp1 = mp1_ + (size_t)pair * max_n, *mp2 = mp2_ + (size_t)pair * max_n;
    const float *ur1 = ur1_ ? ur1_ + (size_t)pair * max_n : nullptr, *ur2 = ur2_ ? ur2_ + (size_t)pair * max_n : nullptr;
    const int32_t *ids2 = S2.node_ids + (size_t)pair * max_nodes, *st2 = S2.node_start + (size_t)pair * (max_nodes + 1), *fe2 = S2.feat + (size_t)pair * max_n;
    const orbhip_keypoint *kp1 = kp1_ + (size_t)pair * kp_stride, *kp2 = kp2_ + (size_t)pair * kp_stride;
    const uint4 *d1 = reinterpret_cast<const uint4 *>(desc1_ + (size_t)pair * kp_stride * 32);
    const uint4 *d2 = reinterpret_cast<const uint4 *>(desc2_ + (size_t)pair * kp_stride * 32);
    const orbhip_tri_pair g = geom_[pair];
    for (int i = tid; i < HISTO_LENGTH; i += TRI_THREADS) hist[i] = 0;
    if (tid == 0) s_cnt = 0;
    for (int j = tid; j < n2; j += TRI_THREADS) {
        dlds[2 * j] = d2[2 * j]; dlds[2 * j + 1] = d2[2 * j + 1];
        flag2[j] = (uint8_t)((mp2[j] ? 1 : 0) | ((ur2 && ur2[j] >= 0.0f) ? 2 : 0));
    }
    __syncthreads();
    int mine = 0;
    for (int idx1 = tid; idx1 < n1; idx1 += TRI_THREADS) {
        int best_idx = -1;
        bin1[idx1] = -1;
        const bool st1 = ur1 && ur1[idx1] >= 0.0f;
        if (!mp1[idx1] && !(g.only_stereo && !st1)) {                        // :1039-1048
            const int nid = nid1[idx1];
            const int lo = node_lower_bound(ids2, nn2, nid);
            if (lo < nn2 && ids2[lo] == nid) {
                const uint4 a0 = d1[2 * idx1], a1 = d1[2 * idx1 + 1];
                const float x1 = kp1[idx1].x, y1 = kp1[idx1].y;
                // epipolar line in the second image, Pinhole.cpp:130-132
                const float la = __fadd_rn(__fadd_rn(__fmul_rn(x1, g.F12[0]), __fmul_rn(y1, g.F12[3])), g.F12[6]);
                const float lb = __fadd_rn(__fadd_rn(__fmul_rn(x1, g.F12[1]), __fmul_rn(y1, g.F12[4])), g.F12[7]);
                const float lc = __fadd_rn(__fadd_rn(__fmul_rn(x1, g.F12[2]), __fmul_rn(y1, g.F12[5])), g.F12[8]);
                const float den = __fadd_rn(__fmul_rn(la, la), __fmul_rn(lb, lb));
                int best = TH_LOW;
                for (int j = st2[lo]; j < st2[lo + 1]; j++) {                // :1062-1143
                    const int idx2 = fe2[j];
                    const int fl = flag2[idx2];
                    if ((fl & 1) || (g.only_stereo && !(fl & 2))) continue;
                    const int dist = hamming256(a0, a1, dlds[2 * idx2], dlds[2 * idx2 + 1]);
                    if (dist > best) continue;                               // :1073 (best <= TH_LOW always)
                    const orbhip_keypoint k2 = kp2[idx2];
                    if (!st1 && !(fl & 2)) {                                 // :1083-1091
                        const float ex = __fsub_rn(g.ep_x, k2.x), ey = __fsub_rn(g.ep_y, k2.y);
                        if (__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) < __fmul_rn(100.0f, lv.scale[k2.octave & 15])) continue;
                    }
                    bool ok = g.coarse != 0;
                    if (!ok && den != 0.0f) {                                // Pinhole.cpp:134-143
                        const float num = __fadd_rn(__fadd_rn(__fmul_rn(la, k2.x), __fmul_rn(lb, k2.y)), lc);
                        const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
                        ok = (double)dsqr < 3.84 * (double)lv.sigma2[k2.octave & 15];
                    }
                    if (ok) { best_idx = idx2; best = dist; }
                }
            }
        }
        if (best_idx >= 0) {
            mine++;
            if (check_ori) {                                                 // :1154-1164
                const int bin = rot_bin(kp1[idx1].angle, kp2[best_idx].angle);
                atomicAdd(&hist[bin], 1); bin1[idx1] = (int8_t)bin;
            }
        }
        matches12[idx1] = best_idx;
    }
    __syncthreads();
    if (check_ori) {                                                         // :1171-1189
        if (tid == 0) rot_three_maxima(hist, s_keep);
        __syncthreads();
        for (int i = tid; i < n1; i += TRI_THREADS) {
            const int b = bin1[i];
            if (b < 0 || rot_kept(b, s_keep)) continue;
            matches12[i] = -1; mine--;
        }
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (tid == 0) nmatches_[pair] = s_cnt;
}

struct TriLevelsG { float sigma2_1[16], scale2[16], sigma2_2[16]; };
#define TRIG_THREADS 128

// BIG (round 4): keyframes of more than 4096 keypoints (to 16384) read KF2's descriptors from global memory instead of LDS.
// MT (round 4): the overload that also returns the triangulated points (ORBmatcher.cc:1212-1402): the candidate test is
// GeometricCamera::matchAndtriangulate with the absolute poses of the two cameras (poses_), no stereo / epipole gates (bOnlyStereo is
// not read there), and the world point of every kept match goes to points12_ [pairs][max_n][3].
template <bool BIG, bool MT>
__global__ __launch_bounds__(TRIG_THREADS) void k_search_triangulation_general(const int32_t *nid1_, const uint8_t *mp1_, const orbhip_keypoint *kp1_,
        const uint8_t *desc1_, const float *ur1_, const int32_t *n1_, FeatVec S2, const uint8_t *mp2_, const orbhip_keypoint *kp2_,
        const uint8_t *desc2_, const float *ur2_, const int32_t *n2_, const orbhip_tri_pair_general *geom_, int max_nodes, int max_n,
        size_t kp_stride, TriLevelsG lv, int check_ori, int cap_n, int32_t *matches12_, int32_t *nmatches_, int32_t *status,
        const orbhip_tri_pair_poses *poses_, float *points12_)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t trig_lds[];
    uint4 *dlds = reinterpret_cast<uint4 *>(trig_lds);                        // [cap_n][2] KF2 descriptors (BIG: absent)
    uint8_t *flag2 = reinterpret_cast<uint8_t *>(dlds + (BIG ? 0 : 2 * (size_t)cap_n));   // [cap_n] bit0: has a map point, bit1: stereo
    int8_t *bin1 = reinterpret_cast<int8_t *>(flag2 + cap_n);                 // [cap_n] rotation bin of KF1 keypoint i's match
    __shared__ orbhip_tri_pair_general g;
    __shared__ orbhip_tri_pair_poses P;
    __shared__ int hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    __shared__ int s_cnt;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n1 = n1_[pair], n2 = n2_[pair], nn2 = S2.nnodes[pair];
    int32_t *matches12 = matches12_ + (size_t)pair * max_n;
    if (n1 > cap_n || n2 > cap_n || n1 > max_n || n2 > max_n || nn2 > max_nodes) {
        if (tid == 0) { atomicExch(status, ORBHIP_E_CAPACITY); nmatches_[pair] = 0; }
        return;
    }
    const int32_t *nid1 = nid1_ + (size_t)pair * max_n;
    const uint8_t *mp1 = mp1_ + (size_t)pair * max_n, *mp2 = mp2_ + (size_t)pair * max_n;
    const float *ur1 = ur1_ ? ur1_ + (size_t)pair * max_n : nullptr, *ur2 = ur2_ ? ur2_ + (size_t)pair * max_n : nullptr;
    const int32_t *ids2 = S2.node_ids + (size_t)pair * max_nodes, *st2 = S2.node_start + (size_t)pair * (max_nodes + 1), *fe2 = S2.feat + (size_t)pair * max_n;
    const orbhip_keypoint *kp1 = kp1_ + (size_t)pair * kp_stride, *kp2 = kp2_ + (size_t)pair * kp_stride;
    const uint4 *d1 = reinterpret_cast<const uint4 *>(desc1_ + (size_t)pair * kp_stride * 32);
    const uint4 *d2 = reinterpret_cast<const uint4 *>(desc2_ + (size_t)pair * kp_stride * 32);
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(geom_ + pair);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&g);
        for (int i = tid; i < (int)(sizeof(orbhip_tri_pair_general) / 4); i += TRIG_THREADS) dst[i] = src[i];
        if (MT) {
            const uint32_t *psrc = reinterpret_cast<const uint32_t *>(poses_ + pair);
            uint32_t *pdst = reinterpret_cast<uint32_t *>(&P);
            for (int i = tid; i < (int)(sizeof(orbhip_tri_pair_poses) / 4); i += TRIG_THREADS) pdst[i] = psrc[i];
        }
    }
    for (int i = tid; i < HISTO_LENGTH; i += TRIG_THREADS) hist[i] = 0;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const bool cam2nd1 = g.nleft1 != -1, cam2nd2 = g.nleft2 != -1;           // pKF->mpCamera2 != 0
    for (int j = tid; j < n2; j += TRIG_THREADS) {
        if (!BIG) { dlds[2 * j] = d2[2 * j]; dlds[2 * j + 1] = d2[2 * j + 1]; }
        flag2[j] = (uint8_t)((mp2[j] ? 1 : 0) | ((!cam2nd2 && ur2 && ur2[j] >= 0.0f) ? 2 : 0));      // :1073
    }
    __syncthreads();
    int mine = 0;
    for (int idx1 = tid; idx1 < n1; idx1 += TRIG_THREADS) {
        int best_idx = -1;
        float best_pt[3] = {0.f, 0.f, 0.f};
        bin1[idx1] = -1;
        const bool st1 = !cam2nd1 && ur1 && ur1[idx1] >= 0.0f;                // :1044
        if (!mp1[idx1] && (MT || !(g.only_stereo && !st1))) {                 // (:1264-1265: only the map-point test)
            const int nid = nid1[idx1];
            const int lo = node_lower_bound(ids2, nn2, nid);
            if (lo < nn2 && ids2[lo] == nid) {
                const uint4 a0 = d1[2 * idx1], a1 = d1[2 * idx1 + 1];
                const orbhip_keypoint k1 = kp1[idx1];
                const int bRight1 = !(g.nleft1 == -1 || idx1 < g.nleft1);    // :1055-1056
                const float s1 = lv.sigma2_1[k1.octave & 15];
                int best = TH_LOW;
                for (int j = st2[lo]; j < st2[lo + 1]; j++) {
                    const int idx2 = fe2[j];
                    const int fl = flag2[idx2];
                    if ((fl & 1) || (!MT && g.only_stereo && !(fl & 2))) continue;
                    const int dist = BIG ? hamming256(a0, a1, d2[2 * idx2], d2[2 * idx2 + 1]) : hamming256(a0, a1, dlds[2 * idx2], dlds[2 * idx2 + 1]);
                    if (dist > best) continue;                                // :1082 (best <= TH_LOW always)
                    const orbhip_keypoint k2 = kp2[idx2];
                    const int bRight2 = !(g.nleft2 == -1 || idx2 < g.nleft2);
                    if (!MT && !st1 && !(fl & 2) && !cam2nd1) {               // :1091-1099
                        const float ex = g.ep_x - k2.x, ey = g.ep_y - k2.y;
                        if (ex * ex + ey * ey < 100.0f * lv.scale2[k2.octave & 15]) continue;
                    }
                    const bool both = cam2nd1 && cam2nd2;                     // :1101-1130
                    const int c = both ? 2 * bRight1 + bRight2 : 0, ci1 = both ? bRight1 : 0, ci2 = both ? bRight2 : 0;
                    const float s2 = lv.sigma2_2[k2.octave & 15];
                    bool ok = !MT && g.coarse != 0;
                    if (MT) {                                                 // :1307-1324: camera and pose by bRight; Pinhole::matchAndtriangulate is
                        float pt[3];                                          // { return false; } (Pinhole.h:91-94)
                        if (g.cam1_type[bRight1] == 1 &&
                            tri_kb8_match_and_triangulate(g.cam1[bRight1], g.cam2_type[bRight2], g.cam2[bRight2], k1.x, k1.y, k2.x, k2.y, P.Tcw1[bRight1],
                                                          P.Tcw2[bRight2], s1, s2, pt)) {
                            ok = true; best_pt[0] = pt[0]; best_pt[1] = pt[1]; best_pt[2] = pt[2];
                        }
                    } else if (!ok) {
                        if (g.cam1_type[ci1] == 0) {                          // Pinhole.cpp:129-143
                            const float *F = g.F12[c];
                            const float la = k1.x * F[0] + k1.y * F[3] + F[6];
                            const float lb = k1.x * F[1] + k1.y * F[4] + F[7];
                            const float lc = k1.x * F[2] + k1.y * F[5] + F[8];
                            const float num = la * k2.x + lb * k2.y + lc;
                            const float den = la * la + lb * lb;
                            if (den != 0.0f) { const float dsqr = num * num / den; ok = (double)dsqr < 3.84 * (double)s2; }
                        } else
                            ok = tri_kb8_triangulate<false>(1, g.cam1[ci1], g.cam2_type[ci2], g.cam2[ci2], k1.x, k1.y, k2.x, k2.y, g.R12[c], g.t12[c], s1, s2, nullptr, nullptr);
                    }
                    if (ok) { best_idx = idx2; best = dist; }
                }
            }
        }
        if (best_idx >= 0) {
            mine++;
            if (check_ori) {                                                  // :1154-1164
                const int bin = rot_bin(kp1[idx1].angle, kp2[best_idx].angle);
                atomicAdd(&hist[bin], 1); bin1[idx1] = (int8_t)bin;
            }
        }
        matches12[idx1] = best_idx;
        if (MT) {
            float *pt = points12_ + ((size_t)pair * max_n + idx1) * 3;
            pt[0] = best_pt[0]; pt[1] = best_pt[1]; pt[2] = best_pt[2];
        }
    }
    __syncthreads();
    if (check_ori) {                                                          // :1171-1189
        if (tid == 0) rot_three_maxima(hist, s_keep);
        __syncthreads();
        for (int i = tid; i < n1; i += TRIG_THREADS) {
            const int b = bin1[i];
            if (b < 0 || rot_kept(b, s_keep)) continue;
            matches12[i] = -1; mine--;
        }
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (tid == 0) nmatches_[pair] = s_cnt;
}

// Frame::ComputeStereoFishEyeMatches (Frame.cc:1128-1168) after the 2-NN on the lapping slices: one thread per left keypoint i of frame f
// (row i of mvKeys; the rows below monoLeft and above Nleft only take the reset values).  Lapping row q = i - monoLeft: Lowe's test on
// the 2-NN pair (:1153, size() >= 2 included), TriangulateMatches(mpCamera2, kpL, kpR, mRlr, mtlr, sigma2[kpL.octave],
// sigma2[kpR.octave]) (:1158-1159), depth > 0.0001f (:1160).  mvRightToLeftMatch keeps the highest left index of a right keypoint (the
// reference loop overwrites in query order): atomicMax on a table the caller has set to -1.
struct FeArgs {
    const orbhip_keypoint *kpL, *kpR;
    const int32_t *nL, *nR, *monoL, *monoR;
    size_t strideL, strideR;
    int max_n, type1, type2;
    float cam1[8], cam2[8], R12[9], t12[3], sigma2[16];
    const int32_t *idx2;
    const uint8_t *accept;
    int32_t *l2r, *r2l, *n_matches, *status;
    float *depth, *x3d;
};
#define FE_THREADS 256
__global__ __launch_bounds__(FE_THREADS) void k_stereo_fisheye_tri(FeArgs A)
{
    const int f = blockIdx.y, i = blockIdx.x * FE_THREADS + threadIdx.x;
    const int nL = A.nL[f], nR = A.nR[f];
    const bool over = nL > A.max_n || nR > A.max_n;
    if (over && i == 0) atomicExch(A.status, ORBHIP_E_CAPACITY);
    const int mL = min(max(A.monoL[f], 0), max(nL, 0)), mR = min(max(A.monoR[f], 0), max(nR, 0));
    int l2r = -1;
    float depth = -1.f, x[3] = {0.f, 0.f, 0.f};
    if (!over && i >= mL && i < nL) {
        const size_t o = (size_t)f * A.max_n + (i - mL);
        const int t0 = A.idx2[2 * o], t1 = A.idx2[2 * o + 1];
        if (A.accept[o] && t0 >= 0 && t1 >= 0) {
            const orbhip_keypoint kL = A.kpL[(size_t)f * A.strideL + i], kR = A.kpR[(size_t)f * A.strideR + mR + t0];
            float z, p[3];
            if (tri_kb8_triangulate<true>(A.type1, A.cam1, A.type2, A.cam2, kL.x, kL.y, kR.x, kR.y, A.R12, A.t12, A.sigma2[kL.octave & 15],
                                          A.sigma2[kR.octave & 15], &z, p)) {
                l2r = mR + t0; depth = z; x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
                atomicMax(&A.r2l[(size_t)f * A.max_n + l2r], i);
            }
        }
    }
    if (i < A.max_n) {
        const size_t o = (size_t)f * A.max_n + i;
        A.l2r[o] = l2r; A.depth[o] = depth;
        A.x3d[3 * o] = x[0]; A.x3d[3 * o + 1] = x[1]; A.x3d[3 * o + 2] = x[2];
    }
    const unsigned long long hit = __ballot(l2r >= 0);
    if ((threadIdx.x & 63) == 0 && hit) atomicAdd(&A.n_matches[f], (int)__popcll(hit));
}

}  // namespace

// Two launches and two memsets on the context's stream: the 2-NN (matrix-core kernel from 64 rows) into a scratch arena, then the
// triangulation.  Kept apart: the Jacobi sweeps' registers would cut the matcher's occupancy.
extern "C" int orbhip_compute_stereo_fisheye_matches_device(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kpL, const uint8_t *d_descL, const int32_t *d_nL, const int32_t *d_monoL, size_t strideL,
        const orbhip_keypoint *d_kpR, const uint8_t *d_descR, const int32_t *d_nR, const int32_t *d_monoR, size_t strideR,
        int batch, int max_n, int cam1_type, const float *cam1, int cam2_type, const float *cam2, const float *Rlr, const float *tlr,
        const float *level_sigma2, int nlevels,
        int32_t *d_l2r, int32_t *d_r2l, float *d_depth, float *d_x3d, int32_t *d_n_matches)
{
    if (!ctx || !d_kpL || !d_descL || !d_nL || !d_monoL || !d_kpR || !d_descR || !d_nR || !d_monoR || batch <= 0 || max_n <= 0 || max_n > 65535 ||
        strideL < (size_t)max_n || strideR < (size_t)max_n || (cam1_type != 0 && cam1_type != 1) || (cam2_type != 0 && cam2_type != 1) || !cam1 ||
        !cam2 || !Rlr || !tlr || !level_sigma2 || nlevels <= 0 || nlevels > 16 || !d_l2r || !d_r2l || !d_depth || !d_x3d || !d_n_matches)
        return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    const size_t rows = (size_t)batch * max_n;
    uint8_t *w = (uint8_t *)orbhip_ctx_scratch_internal(ctx, 17 * rows + 256);
    if (!w) return ORBHIP_E_HIP;
    int32_t *d_idx2 = (int32_t *)w, *d_dist2 = d_idx2 + 2 * rows;
    uint8_t *d_accept = (uint8_t *)(d_dist2 + 2 * rows);
    hipStream_t st = orbhip_ctx_stream_internal(ctx);
    if (hipMemsetAsync(d_r2l, 0xFF, 4 * rows, st) != hipSuccess || hipMemsetAsync(d_n_matches, 0, 4 * (size_t)batch, st) != hipSuccess) return ORBHIP_E_HIP;
    int rc = orbhip_bf2nn_slices_internal(ctx, d_descL, d_nL, d_monoL, strideL * 32, d_descR, d_nR, d_monoR, strideR * 32, batch, max_n, 0.7,
                                          d_idx2, d_dist2, d_accept);
    if (rc) return rc;
    FeArgs A;
    memset(&A, 0, sizeof(A));
    A.kpL = d_kpL; A.kpR = d_kpR; A.nL = d_nL; A.nR = d_nR; A.monoL = d_monoL; A.monoR = d_monoR; A.strideL = strideL; A.strideR = strideR;
    A.max_n = max_n; A.type1 = cam1_type; A.type2 = cam2_type;
    for (int k = 0; k < 8; k++) { A.cam1[k] = cam1[k]; A.cam2[k] = cam2[k]; }
    for (int k = 0; k < 9; k++) A.R12[k] = Rlr[k];
    for (int k = 0; k < 3; k++) A.t12[k] = tlr[k];
    for (int l = 0; l < nlevels; l++) A.sigma2[l] = level_sigma2[l];
    A.idx2 = d_idx2; A.accept = d_accept; A.l2r = d_l2r; A.r2l = d_r2l; A.n_matches = d_n_matches; A.status = orbhip_ctx_status_internal(ctx);
    A.depth = d_depth; A.x3d = d_x3d;
    hipLaunchKernelGGL(k_stereo_fisheye_tri, dim3((max_n + FE_THREADS - 1) / FE_THREADS, batch), dim3(FE_THREADS), 0, st, A);
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

extern "C" int orbhip_search_for_triangulation_device(orbhip_ctx *ctx,
        const int32_t *d_nid1, const uint8_t *d_has_mp1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const float *d_u_right1,
        const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_has_mp2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const float *d_u_right2, const int32_t *d_n2,
        const orbhip_tri_pair *d_pair, int pairs, int max_nodes, int max_n, size_t frame_stride_kp,
        const float *scale_factors, const float *level_sigma2, int nlevels, int check_orientation,
        int32_t *d_matches12, int32_t *d_nmatches)
{
    if (!ctx || !d_nid1 || !d_has_mp1 || !d_kp1 || !d_desc1 || !d_n1 || !d_node_ids2 || !d_node_start2 || !d_feat2 || !d_nnodes2 ||
        !d_has_mp2 || !d_kp2 || !d_desc2 || !d_n2 || !d_pair || pairs <= 0 || max_nodes <= 0 || max_n <= 0 || !scale_factors ||
        !level_sigma2 || nlevels <= 0 || nlevels > 16 || !d_matches12 || !d_nmatches) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    TriLevels lv;
    for (int l = 0; l < 16; l++) { lv.scale[l] = l < nlevels ? scale_factors[l] : 0.0f; lv.sigma2[l] = l < nlevels ? level_sigma2[l] : 0.0f; }
    const int cap_n = ((max_n < 4096 ? max_n : 4096) + 15) & ~15;
    const size_t lds = (size_t)cap_n * (32 + 1 + 1) + 16;
    if (orb_lds_optin(reinterpret_cast<const void *>(k_search_triangulation), orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    FeatVec S2 = {d_node_ids2, d_node_start2, d_feat2, d_nnodes2};
    hipLaunchKernelGGL(k_search_triangulation, dim3(pairs), dim3(TRI_THREADS), lds, orbhip_ctx_stream_internal(ctx), d_nid1, d_has_mp1, d_kp1,
                       d_desc1, d_u_right1, d_n1, S2, d_has_mp2, d_kp2, d_desc2, d_u_right2, d_n2, d_pair, max_nodes, max_n, frame_stride_kp, lv,
                       check_orientation, cap_n, d_matches12, d_nmatches, orbhip_ctx_status_internal(ctx));
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}

namespace {
int tri_general_launch(orbhip_ctx *ctx,
        const int32_t *d_nid1, const uint8_t *d_has_mp1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const float *d_u_right1,
        const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_has_mp2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const float *d_u_right2, const int32_t *d_n2,
        const orbhip_tri_pair_general *d_pair, const orbhip_tri_pair_poses *d_poses, int pairs, int max_nodes, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *scale_factors2, const float *level_sigma2_2, int nlevels, int check_orientation,
        int32_t *d_matches12, float *d_points12, int32_t *d_nmatches)
{
    if (!ctx || !d_nid1 || !d_has_mp1 || !d_kp1 || !d_desc1 || !d_n1 || !d_node_ids2 || !d_node_start2 || !d_feat2 || !d_nnodes2 ||
        !d_has_mp2 || !d_kp2 || !d_desc2 || !d_n2 || !d_pair || pairs <= 0 || max_nodes <= 0 || max_n <= 0 || !level_sigma2_1 || !scale_factors2 ||
        !level_sigma2_2 || nlevels <= 0 || nlevels > 16 || !d_matches12 || !d_nmatches || (d_poses != nullptr) != (d_points12 != nullptr)) return ORBHIP_E_BADARG;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) return ORBHIP_E_HIP;
    TriLevelsG lv;
    for (int l = 0; l < 16; l++) {
        lv.sigma2_1[l] = l < nlevels ? level_sigma2_1[l] : 0.0f; lv.scale2[l] = l < nlevels ? scale_factors2[l] : 0.0f;
        lv.sigma2_2[l] = l < nlevels ? level_sigma2_2[l] : 0.0f;
    }
    // up to 4096 keypoints KF2's descriptors live in LDS; beyond (to 16384: the 5 x nFeatures keypoints of a monocular map's first keyframes,
    // Tracking.cc:210) they are read from global memory and only the per-keypoint flags stay in LDS
    const bool big = max_n > 4096, mt = d_poses != nullptr;
    const int lim = big ? 16384 : 4096;
    const int cap_n = ((max_n < lim ? max_n : lim) + 15) & ~15;
    const size_t lds = (size_t)cap_n * (big ? (1 + 1) : (32 + 1 + 1)) + 16;
    typedef void (*kern_t)(const int32_t *, const uint8_t *, const orbhip_keypoint *, const uint8_t *, const float *, const int32_t *, FeatVec, const uint8_t *,
                           const orbhip_keypoint *, const uint8_t *, const float *, const int32_t *, const orbhip_tri_pair_general *, int, int, size_t, TriLevelsG, int,
                           int, int32_t *, int32_t *, int32_t *, const orbhip_tri_pair_poses *, float *);
    const kern_t kern = mt ? (big ? k_search_triangulation_general<true, true> : k_search_triangulation_general<false, true>)
                           : (big ? k_search_triangulation_general<true, false> : k_search_triangulation_general<false, false>);
    if (orb_lds_optin(reinterpret_cast<const void *>(kern), orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    FeatVec S2 = {d_node_ids2, d_node_start2, d_feat2, d_nnodes2};
    hipLaunchKernelGGL(kern, dim3(pairs), dim3(TRIG_THREADS), lds, orbhip_ctx_stream_internal(ctx), d_nid1, d_has_mp1, d_kp1, d_desc1, d_u_right1, d_n1, S2,
                       d_has_mp2, d_kp2, d_desc2, d_u_right2, d_n2, d_pair, max_nodes, max_n, frame_stride_kp, lv, check_orientation, cap_n, d_matches12,
                       d_nmatches, orbhip_ctx_status_internal(ctx), d_poses, d_points12);
    return hipGetLastError() == hipSuccess ? ORBHIP_OK : ORBHIP_E_HIP;
}
}  // namespace

extern "C" int orbhip_search_for_triangulation_general_device(orbhip_ctx *ctx,
        const int32_t *d_nid1, const uint8_t *d_has_mp1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const float *d_u_right1,
        const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_has_mp2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const float *d_u_right2, const int32_t *d_n2,
        const orbhip_tri_pair_general *d_pair, int pairs, int max_nodes, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *scale_factors2, const float *level_sigma2_2, int nlevels, int check_orientation,
        int32_t *d_matches12, int32_t *d_nmatches)
{
    return tri_general_launch(ctx, d_nid1, d_has_mp1, d_kp1, d_desc1, d_u_right1, d_n1, d_node_ids2, d_node_start2, d_feat2, d_nnodes2, d_has_mp2, d_kp2, d_desc2,
                              d_u_right2, d_n2, d_pair, nullptr, pairs, max_nodes, max_n, frame_stride_kp, level_sigma2_1, scale_factors2, level_sigma2_2, nlevels,
                              check_orientation, d_matches12, nullptr, d_nmatches);
}

extern "C" int orbhip_match_and_triangulate_device(orbhip_ctx *ctx,
        const int32_t *d_nid1, const uint8_t *d_has_mp1, const orbhip_keypoint *d_kp1, const uint8_t *d_desc1, const int32_t *d_n1,
        const int32_t *d_node_ids2, const int32_t *d_node_start2, const int32_t *d_feat2, const int32_t *d_nnodes2,
        const uint8_t *d_has_mp2, const orbhip_keypoint *d_kp2, const uint8_t *d_desc2, const int32_t *d_n2,
        const orbhip_tri_pair_general *d_pair, const orbhip_tri_pair_poses *d_poses, int pairs, int max_nodes, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *level_sigma2_2, int nlevels, int check_orientation,
        int32_t *d_matches12, float *d_points12, int32_t *d_nmatches)
{
    if (!d_poses || !d_points12) return ORBHIP_E_BADARG;
    return tri_general_launch(ctx, d_nid1, d_has_mp1, d_kp1, d_desc1, nullptr, d_n1, d_node_ids2, d_node_start2, d_feat2, d_nnodes2, d_has_mp2, d_kp2, d_desc2,
                              nullptr, d_n2, d_pair, d_poses, pairs, max_nodes, max_n, frame_stride_kp, level_sigma2_1, level_sigma2_2, level_sigma2_2, nlevels,
                              check_orientation, d_matches12, d_points12, d_nmatches);
}
