// newpoints_kernels.hip -- the per-match loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:479-724) on what
// SearchForTriangulation leaves on the device: d_matches12 [pairs][max_n] (idx2 or -1 per KF1 keypoint).  Per match, in the reference's
// order: keypoint / bStereo / bRight selection (:486-501), pose and camera among ll / lr / rl / rr for rig pairs (:503-568), ray parallax
// against stereo parallax (:571-587), linear triangulation by the SVD of a 4x4 system or KeyFrame::UnprojectStereo (:590-623,
// KeyFrame.cc:821-837), both depths (:629-635), reprojection in both keyframes (:638-688), distances and scale consistency (:691-707).
// The kernel ends where the reference says `new MapPoint` (:710): it writes the world point and an outcome code per KF1 keypoint, counts the
// created points per pair and, when the caller hands it writable flag rows, marks idx1 / idx2 of every created point -- what
// AddMapPoint (:715-716) does to the next neighbour's SearchForTriangulation (ORBmatcher.cc:1039, :1067).
//
// Matches are sparse among KF1's keypoints (10-30 %), and a match costs up to 30 Jacobi sweeps: a workgroup walks its slice of the row
// 256 keypoints at a time, appends the (i, matches12[i]) with a match to a queue in LDS (wave ballot + prefix) and runs the per-match work
// on 256 dense queue entries whenever that many are waiting, so that the sweeps run in full waves.  Results go back to index i.
//
// Arithmetic as tri_kernels.hip: -ffp-contract=off, every float expression op by op in the reference's order, cv::Mat products that
// tri_kb8_match_and_triangulate (the same linear system with absolute poses) spells out keep its rounding points (sums in double, rounded
// once), Twc.R * x3Dc + Twc.t of UnprojectStereo keeps host/cvmath.h's mul_add (no transposed operand: float sum, then one rounding of
// the double t + c), libm calls are the library's fixed sequences (tri_atan2f, tri_sincos_signed).  Parity against an OpenCV build unpinned.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "svd4.h"
#include "cam_project_f32.h"
#include <cstring>

namespace {

struct NpLevels { float sigma2_1[16], scale1[16], sigma2_2[16], scale2[16]; };

enum {
    NP_NONE = 0, NP_TRIANGULATED = 1, NP_STEREO1 = 2, NP_STEREO2 = 3, NP_LOW_PARALLAX = 4, NP_W_ZERO = 5, NP_EMPTY_STEREO = 6, NP_Z1 = 7, NP_Z2 = 8,
    NP_REPROJ1 = 9, NP_REPROJ2 = 10, NP_ZERO_DIST = 11, NP_FAR = 12, NP_SCALE = 13
};

// cos(2*atan2(mb/2, mvDepth[idx])) (:583, :585).  mb and mvDepth[] are float, so with <cmath> in scope the reference's call resolves to
// std::atan2(float, float) = atan2f, `2 * float` stays float, and cos resolves to std::cos(float) = cosf: a float chain, restated here
// with the library's stand-ins for atan2f and cosf.
__device__ float np_cos_stereo(float mb, float depth)
{
    const float a = tri_atan2f(mb / 2, depth);
    const float t = 2 * a;
    double s, c;
    tri_sincos_signed((double)t, s, c);
    return (float)c;
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:821-837): reads mvKeys (the RAW keypoint, not mvKeysUn), the keyframe's cx cy invfx invfy and Twc
// (rows 0..2, row-major 3x4).  false = the empty cv::Mat of a depth that is not positive.
__device__ bool np_unproject_stereo(const float *cam, const float *Twc, float u, float v, float z, float *x3D)
{
    if (!(z > 0)) return false;
    const float invfx = 1.0f / cam[0], invfy = 1.0f / cam[1];
    const float x = (u - cam[2]) * z * invfx;
    const float y = (v - cam[3]) * z * invfy;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float t = Twc[4 * i] * x + Twc[4 * i + 1] * y + Twc[4 * i + 2] * z;
        x3D[i] = (float)((double)t + (double)Twc[4 * i + 3]);
    }
    return true;
}

// Rcw.row(r).dot(x3Dt) + tcw.at<float>(r): Mat::dot accumulates in double, the float translation is added in double, the result narrows once
__device__ __forceinline__ float np_row_dot(const float *T, int r, const float *x)
{
    return (float)((double)T[4 * r] * x[0] + (double)T[4 * r + 1] * x[1] + (double)T[4 * r + 2] * x[2] + (double)T[4 * r + 3]);
}

// (:638-688) false = the reprojection test of this keyframe rejects.  cam: the camera the keypoint was seen by; kfcam: mpCamera of the
// keyframe, whose fx fy cx cy the stereo formula reads; mbf: mpCurrentKeyFrame->mbf for BOTH keyframes (:656, :681).
__device__ bool np_reproject(bool stereo, int type, const float *cam, const float *kfcam, float mbf, const float *T, const float *x3D, float z,
                             float u, float v, float ur, float sigma2)
{
    const float x = np_row_dot(T, 0, x3D), y = np_row_dot(T, 1, x3D);
    const float invz = (float)(1.0 / (double)z);
    if (!stereo) {
        const float P[3] = {x, y, z};
        float uv[2];
        tri_project(type, cam, P, uv);
        const float errX = uv[0] - u, errY = uv[1] - v;
        return !((double)(errX * errX + errY * errY) > 5.991 * (double)sigma2);
    }
    const float u1 = kfcam[0] * x * invz + kfcam[2];
    const float u1_r = u1 - mbf * invz;
    const float v1 = kfcam[1] * y * invz + kfcam[3];
    const float errX = u1 - u, errY = v1 - v, errX_r = u1_r - ur;
    return !((double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)sigma2);
}

// cv::norm(x3D - Ow): the difference in float, the norm accumulated in double
__device__ __forceinline__ float np_dist(const float *x, const float *O)
{
    const float a = x[0] - O[0], b = x[1] - O[1], c = x[2] - O[2];
    return (float)sqrt((double)a * a + (double)b * b + (double)c * c);
}

// One match (:483-707).  g lives in LDS: its arrays are picked with run-time indices, which a private copy could not be.  k1 / k2: the
// keypoint the loop reads (mvKeysUn, or mvKeys | mvKeysRight of a rig keyframe); raw1 / raw2: mvKeys[idx] for UnprojectStereo.
__device__ int np_match(const orbhip_newpoints_pair &g, const NpLevels &lv, int idx1, int idx2, const orbhip_keypoint &k1, float raw1x, float raw1y,
                        float ur1, float depth1, const orbhip_keypoint &k2, float raw2x, float raw2y, float ur2, float depth2, float *x3D)
{
    const bool rig1 = g.nleft1 != -1, rig2 = g.nleft2 != -1;                  // mpCamera2 != 0
    const bool bStereo1 = !rig1 && ur1 >= 0, bStereo2 = !rig2 && ur2 >= 0;    // :490, :499
    const bool both = rig1 && rig2;                                           // :503 (mixed pairs are refused by the entry point)
    const int c1 = both && idx1 >= g.nleft1 ? 1 : 0, c2 = both && idx2 >= g.nleft2 ? 1 : 0;
    const float *T1 = g.Tcw1[c1], *T2 = g.Tcw2[c2], *cam1 = g.cam1[c1], *cam2 = g.cam2[c2];
    const int type1 = g.cam1_type[c1], type2 = g.cam2_type[c2];

    float xn1[3], xn2[3], ray1[3], ray2[3];
    tri_unproject(type1, cam1, k1.x, k1.y, xn1);                              // :571-572
    tri_unproject(type2, cam2, k2.x, k2.y, xn2);
#pragma unroll
    for (int i = 0; i < 3; i++) {                                             // Rwc = Rcw.t(); ray = Rwc * xn (:574-575)
        ray1[i] = (float)((double)T1[i] * xn1[0] + (double)T1[4 + i] * xn1[1] + (double)T1[8 + i] * xn1[2]);
        ray2[i] = (float)((double)T2[i] * xn2[0] + (double)T2[4 + i] * xn2[1] + (double)T2[8 + i] * xn2[2]);
    }
    const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
    const double n1 = sqrt((double)ray1[0] * ray1[0] + (double)ray1[1] * ray1[1] + (double)ray1[2] * ray1[2]);
    const double n2 = sqrt((double)ray2[0] * ray2[0] + (double)ray2[1] * ray2[1] + (double)ray2[2] * ray2[2]);
    const float cosParallaxRays = (float)(dot / (n1 * n2));                   // :576

    float cosParallaxStereo = cosParallaxRays + 1;                            // :578-587
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = np_cos_stereo(g.mb1, depth1);
    else if (bStereo2) cosParallaxStereo2 = np_cos_stereo(g.mb2, depth2);     // the reference's `else if`: KF2's only when KF1's is not stereo
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min

    int code;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {   // :590-591
        float At[4][4], v[4];                                                 // :594-598, stored transposed: At[j] = column j of A
#pragma unroll
        for (int j = 0; j < 4; j++) {
            At[j][0] = xn1[0] * T1[8 + j] - T1[j];
            At[j][1] = xn1[1] * T1[8 + j] - T1[4 + j];
            At[j][2] = xn2[0] * T2[8 + j] - T2[j];
            At[j][3] = xn2[1] * T2[8 + j] - T2[4 + j];
        }
        tri_svd4_null(At, v);
        if (v[3] == 0) return NP_W_ZERO;                                      // :605
        const float inv = (float)(1.0 / (double)v[3]);                        // :609, as tri_kb8_match_and_triangulate
        x3D[0] = v[0] * inv; x3D[1] = v[1] * inv; x3D[2] = v[2] * inv;
        code = NP_TRIANGULATED;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {         // :612-615
        if (!np_unproject_stereo(g.cam1[0], g.Twc1, raw1x, raw1y, depth1, x3D)) return NP_EMPTY_STEREO;
        code = NP_STEREO1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {         // :616-619
        if (!np_unproject_stereo(g.cam2[0], g.Twc2, raw2x, raw2y, depth2, x3D)) return NP_EMPTY_STEREO;
        code = NP_STEREO2;
    } else
        return NP_LOW_PARALLAX;                                               // :622

    const float z1 = np_row_dot(T1, 2, x3D);                                  // :629-635
    if (z1 <= 0) return NP_Z1;
    const float z2 = np_row_dot(T2, 2, x3D);
    if (z2 <= 0) return NP_Z2;
    if (!np_reproject(bStereo1, type1, cam1, g.cam1[0], g.mbf, T1, x3D, z1, k1.x, k1.y, ur1, lv.sigma2_1[k1.octave & 15])) return NP_REPROJ1;
    if (!np_reproject(bStereo2, type2, cam2, g.cam2[0], g.mbf, T2, x3D, z2, k2.x, k2.y, ur2, lv.sigma2_2[k2.octave & 15])) return NP_REPROJ2;

    const float dist1 = np_dist(x3D, g.Ow1[c1]), dist2 = np_dist(x3D, g.Ow2[c2]);      // :691-707
    if (dist1 == 0 || dist2 == 0) return NP_ZERO_DIST;
    if (g.far_points && (dist1 >= g.th_far_points || dist2 >= g.th_far_points)) return NP_FAR;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = lv.scale1[k1.octave & 15] / lv.scale2[k2.octave & 15];
    if (ratioDist * g.ratio_factor < ratioOctave || ratioDist > ratioOctave * g.ratio_factor) return NP_SCALE;
    return code;
}

#define NP_THREADS 256
#define NP_WAVES (NP_THREADS / 64)
#define NP_SLICE 2048          // KF1 keypoints per workgroup: a 16384-keypoint keyframe is served by 8 workgroups

struct NpArgs {
    const orbhip_keypoint *kp1, *kp1_raw, *kp2, *kp2_raw;
    const float *ur1, *ur2, *depth1, *depth2;
    const int32_t *n1, *n2, *matches12;
    const orbhip_newpoints_pair *pair;
    uint8_t *mp1, *mp2, *outcome;
    float *x3D;
    int32_t *n_created, *status;
    size_t kp_stride;
    int max_n;
};

__global__ __launch_bounds__(NP_THREADS) void k_create_new_points(NpArgs a, NpLevels lv)
{
    __shared__ orbhip_newpoints_pair g;
    __shared__ int q_i[2 * NP_THREADS], q_m[2 * NP_THREADS];                  // the queue: never more than 255 waiting + 256 appended
    __shared__ int s_wc[NP_WAVES], s_qn, s_created;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = a.n1[pair], n2 = a.n2[pair];
    if (n1 < 0 || n2 < 0 || n1 > a.max_n || n2 > a.max_n) {                   // status word; the pair's rows stay untouched
        if (tid == 0 && blockIdx.y == 0) atomicExch(a.status, ORBHIP_E_CAPACITY);
        return;
    }
    const int lo = blockIdx.y * NP_SLICE, hi = min(n1, lo + NP_SLICE);
    if (lo >= n1) return;                                                     // (n_created was zeroed by the launcher)
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.pair + pair);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&g);
        for (int i = tid; i < (int)(sizeof(orbhip_newpoints_pair) / 4); i += NP_THREADS) dst[i] = src[i];
    }
    if (tid == 0) { s_qn = 0; s_created = 0; }
    __syncthreads();
    const size_t row = (size_t)pair * a.max_n, krow = (size_t)pair * a.kp_stride;
    const int32_t *matches12 = a.matches12 + row;
    const orbhip_keypoint *kp1 = a.kp1 + krow, *kp2 = a.kp2 + krow;
    const orbhip_keypoint *raw1 = a.kp1_raw ? a.kp1_raw + krow : kp1, *raw2 = a.kp2_raw ? a.kp2_raw + krow : kp2;
    const float *ur1 = a.ur1 ? a.ur1 + row : nullptr, *ur2 = a.ur2 ? a.ur2 + row : nullptr;
    const float *depth1 = a.depth1 ? a.depth1 + row : nullptr, *depth2 = a.depth2 ? a.depth2 + row : nullptr;
    uint8_t *outcome = a.outcome + row, *mp1 = a.mp1 ? a.mp1 + row : nullptr, *mp2 = a.mp2 ? a.mp2 + row : nullptr;
    float *x3D_out = a.x3D + row * 3;
    int mine = 0;
    for (int tile = lo; tile < hi; tile += NP_THREADS) {
        const int i = tile + tid;
        int m = -1;
        if (i < hi) {
            m = matches12[i];
            if (m < 0 || m >= n2) {                                           // no match (an index past KF2's keypoints is none either)
                m = -1;
                outcome[i] = NP_NONE;
                x3D_out[3 * i] = 0.f; x3D_out[3 * i + 1] = 0.f; x3D_out[3 * i + 2] = 0.f;
            }
        }
        const unsigned long long hit = __ballot(m >= 0);
        if (lane == 0) s_wc[wave] = (int)__popcll(hit);
        __syncthreads();
        int base = s_qn, total = 0;
#pragma unroll
        for (int w = 0; w < NP_WAVES; w++) { const int c = s_wc[w]; if (w < wave) base += c; total += c; }
        if (m >= 0) {
            const int slot = base + (int)__popcll(hit & ((1ull << lane) - 1));
            q_i[slot] = i; q_m[slot] = m;
        }
        int qn = s_qn + total;
        __syncthreads();
        const bool last = tile + NP_THREADS >= hi;
        while (qn >= NP_THREADS || (last && qn > 0)) {                        // uniform: qn is the same in every lane
            const int cnt = min(qn, NP_THREADS);
            const int slot = qn - cnt + tid;
            if (tid < cnt) {
                const int idx1 = q_i[slot], idx2 = q_m[slot];
                const orbhip_keypoint k1 = kp1[idx1], k2 = kp2[idx2];
                const float u1r = ur1 ? ur1[idx1] : -1.f, u2r = ur2 ? ur2[idx2] : -1.f;
                const float dp1 = depth1 ? depth1[idx1] : -1.f, dp2 = depth2 ? depth2[idx2] : -1.f;
                float x3D[3] = {0.f, 0.f, 0.f};
                const int code = np_match(g, lv, idx1, idx2, k1, raw1[idx1].x, raw1[idx1].y, u1r, dp1, k2, raw2[idx2].x, raw2[idx2].y, u2r, dp2, x3D);
                const bool created = code >= NP_TRIANGULATED && code <= NP_STEREO2;
                outcome[idx1] = (uint8_t)code;
                x3D_out[3 * idx1] = created ? x3D[0] : 0.f; x3D_out[3 * idx1 + 1] = created ? x3D[1] : 0.f; x3D_out[3 * idx1 + 2] = created ? x3D[2] : 0.f;
                if (created) {
                    mine++;
                    if (mp1) mp1[idx1] = 1;                                   // AddMapPoint (:715-716); equal idx2 of two matches: the same byte twice
                    if (mp2) mp2[idx2] = 1;
                }
            }
            qn -= cnt;
        }
        __syncthreads();                                                      // the queue is read out before the next tile appends to it
        if (tid == 0) s_qn = qn;
    }
    if (mine) atomicAdd(&s_created, mine);
    __syncthreads();
    if (tid == 0 && s_created) atomicAdd(&a.n_created[pair], s_created);
}

}  // namespace

// the checks both entry points make on the HOST records before anything is launched
int orbhip_newpoints_check_internal(const orbhip_newpoints_pair *pair, int pairs, int max_n, int nlevels)
{
    if (pairs <= 0) { orbhip_set_last_error_internal("create_new_map_points: pairs < 1"); return ORBHIP_E_BADARG; }
    if (max_n <= 0) { orbhip_set_last_error_internal("create_new_map_points: max_n < 1"); return ORBHIP_E_BADARG; }
    if (max_n > 16384) { orbhip_set_last_error_internal("create_new_map_points: max_n above 16384 features per keyframe"); return ORBHIP_E_CAPACITY; }
    if (nlevels <= 0 || nlevels > 16) { orbhip_set_last_error_internal("create_new_map_points: nlevels outside 1..16"); return ORBHIP_E_BADARG; }
    for (int p = 0; p < pairs; p++) {
        if ((pair[p].nleft1 == -1) != (pair[p].nleft2 == -1)) {               // the reference would reuse the matrices of an earlier match
            orbhip_set_last_error_internal("create_new_map_points: nleft1 / nleft2: one rig and one single-camera keyframe");
            return ORBHIP_E_BADARG;
        }
        if (pair[p].nleft1 < -1 || pair[p].nleft2 < -1) { orbhip_set_last_error_internal("create_new_map_points: nleft < -1"); return ORBHIP_E_BADARG; }
        for (int c = 0; c < 2; c++)
            if ((pair[p].cam1_type[c] | 1) != 1 || (pair[p].cam2_type[c] | 1) != 1) {
                orbhip_set_last_error_internal("create_new_map_points: cam_type is neither 0 (Pinhole) nor 1 (KannalaBrandt8)");
                return ORBHIP_E_BADARG;
            }
    }
    return ORBHIP_OK;
}

// the launch: d_pair on the DEVICE, already checked; level arrays on the host
int orbhip_newpoints_launch_internal(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kp1, const orbhip_keypoint *d_kp1_raw, const float *d_u_right1, const float *d_depth1, const int32_t *d_n1,
        const orbhip_keypoint *d_kp2, const orbhip_keypoint *d_kp2_raw, const float *d_u_right2, const float *d_depth2, const int32_t *d_n2,
        const int32_t *d_matches12, const orbhip_newpoints_pair *d_pair, int pairs, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *scale_factors1, const float *level_sigma2_2, const float *scale_factors2, int nlevels,
        uint8_t *d_has_mp1, uint8_t *d_has_mp2, float *d_x3D, uint8_t *d_outcome, int32_t *d_n_created)
{
    hipStream_t stream = orbhip_ctx_stream_internal(ctx);
    ORB_HIP_TRY(hipMemsetAsync(d_n_created, 0, sizeof(int32_t) * (size_t)pairs, stream));
    NpLevels lv;
    for (int l = 0; l < 16; l++) {
        lv.sigma2_1[l] = l < nlevels ? level_sigma2_1[l] : 0.0f; lv.scale1[l] = l < nlevels ? scale_factors1[l] : 0.0f;
        lv.sigma2_2[l] = l < nlevels ? level_sigma2_2[l] : 0.0f; lv.scale2[l] = l < nlevels ? scale_factors2[l] : 0.0f;
    }
    NpArgs a;
    a.kp1 = d_kp1; a.kp1_raw = d_kp1_raw; a.kp2 = d_kp2; a.kp2_raw = d_kp2_raw;
    a.ur1 = d_u_right1; a.ur2 = d_u_right2; a.depth1 = d_depth1; a.depth2 = d_depth2;
    a.n1 = d_n1; a.n2 = d_n2; a.matches12 = d_matches12; a.pair = d_pair;
    a.mp1 = d_has_mp1; a.mp2 = d_has_mp2; a.outcome = d_outcome; a.x3D = d_x3D;
    a.n_created = d_n_created; a.status = orbhip_ctx_status_internal(ctx);
    a.kp_stride = frame_stride_kp; a.max_n = max_n;
    hipLaunchKernelGGL(k_create_new_points, dim3(pairs, (max_n + NP_SLICE - 1) / NP_SLICE), dim3(NP_THREADS), 0, stream, a, lv);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("k_create_new_points launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}

extern "C" int orbhip_create_new_map_points_device(orbhip_ctx *ctx,
        const orbhip_keypoint *d_kp1, const orbhip_keypoint *d_kp1_raw, const float *d_u_right1, const float *d_depth1, const int32_t *d_n1,
        const orbhip_keypoint *d_kp2, const orbhip_keypoint *d_kp2_raw, const float *d_u_right2, const float *d_depth2, const int32_t *d_n2,
        const int32_t *d_matches12, const orbhip_newpoints_pair *pair, int pairs, int max_n, size_t frame_stride_kp,
        const float *level_sigma2_1, const float *scale_factors1, const float *level_sigma2_2, const float *scale_factors2, int nlevels,
        uint8_t *d_has_mp1, uint8_t *d_has_mp2, float *d_x3D, uint8_t *d_outcome, int32_t *d_n_created)
{
    if (!ctx || !d_kp1 || !d_n1 || !d_kp2 || !d_n2 || !d_matches12 || !pair || !level_sigma2_1 || !scale_factors1 || !level_sigma2_2 ||
        !scale_factors2 || !d_x3D || !d_outcome || !d_n_created) {
        orbhip_set_last_error_internal("orbhip_create_new_map_points_device: a required pointer is NULL");
        return ORBHIP_E_BADARG;
    }
    if (int rc = orbhip_newpoints_check_internal(pair, pairs, max_n, nlevels)) return rc;
    if (frame_stride_kp < (size_t)max_n) { orbhip_set_last_error_internal("orbhip_create_new_map_points_device: frame_stride_kp < max_n"); return ORBHIP_E_BADARG; }
    if ((d_u_right1 != nullptr) != (d_depth1 != nullptr) || (d_u_right2 != nullptr) != (d_depth2 != nullptr)) {
        orbhip_set_last_error_internal("orbhip_create_new_map_points_device: d_u_right and d_depth of a keyframe go together");
        return ORBHIP_E_BADARG;
    }
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    // the per-pair records go to the context's work arena (grow-only: a warmed-up context allocates nothing here).  The copy is ordered
    // on the stream behind an earlier call's kernel, which has read its own records by then; the caller's array is free on return
    const size_t bytes = (size_t)pairs * sizeof(orbhip_newpoints_pair);
    orbhip_newpoints_pair *d_pair = (orbhip_newpoints_pair *)orbhip_ctx_work_internal(ctx, align256(bytes));
    if (!d_pair) return ORBHIP_E_HIP;
    ORB_HIP_TRY(hipMemcpyAsync(d_pair, pair, bytes, hipMemcpyHostToDevice, orbhip_ctx_stream_internal(ctx)));
    return orbhip_newpoints_launch_internal(ctx, d_kp1, d_kp1_raw, d_u_right1, d_depth1, d_n1, d_kp2, d_kp2_raw, d_u_right2, d_depth2, d_n2, d_matches12,
                                            d_pair, pairs, max_n, frame_stride_kp, level_sigma2_1, scale_factors1, level_sigma2_2, scale_factors2, nlevels,
                                            d_has_mp1, d_has_mp2, d_x3D, d_outcome, d_n_created);
}
