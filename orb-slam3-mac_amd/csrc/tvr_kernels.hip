// tvr_kernels.hip -- TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc:39-933), batched over frame pairs: the
// consumer of SearchForInitialization's vnMatches12 (src/Tracking.cc:1522 through GeometricCamera::ReconstructWithTwoViews).
// Four launches per call, every pair of the batch in each:
//   k_tvr_prepare      compaction of vnMatches12 into the match list in index order (:53-62), Normalize of both frames over ALL their
//                      keypoints (:753-799), the RANSAC sets (:81-96, ransac_common.h) when the caller asks for them, reset of the outputs
//   k_tvr_hyp          ComputeH21 / ComputeF21 (:231-308) per (pair, iteration, model), one lane per hypothesis: the 9x9 Gram matrix
//                      of the 16x9 / 8x9 system accumulated in double, cyclic Jacobi on it with the matrix and the rotation in LDS
//                      ([element][lane]: no bank conflicts, no scratch), the eigenvector of the smallest eigenvalue, denormalisation
//   k_tvr_score        CheckHomography / CheckFundamental (:310-473) for every hypothesis over the pair's matches staged in LDS: float
//                      arithmetic in the reference's operation order (-ffp-contract=off), one wave per (iteration, model)
//   k_tvr_reconstruct  the argmax with the reference's tie rule (:170, :221), RH (:111-126), DecomposeE / the Faugeras decomposition,
//                      CheckRT (:802-911) for the 4 / 8 motion hypotheses x matches, the decision rules of ReconstructF / ReconstructH
// OpenCV's SVD bits are not reproduced (for the 8x9 system they cannot be: FULL_UV completes vt from a random generator); every
// decomposition here is a Jacobi iteration in double.  The numbering of the motion hypotheses follows this file's sign conventions for
// the singular vectors (the SET of hypotheses does not depend on them).
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "svd4.h"
#include "ransac_common.h"
#include <cfloat>
#include <cstring>

namespace {

#define TVR_THREADS 256
#define TVR_HYP_STRIDE 28         // floats per (pair, iteration): H21 [9], H12 [9], F21 [9], valid
#define TVR_SCORE_ITERS 32        // iterations per k_tvr_score workgroup

struct TvrArgs {
    const orbhip_keypoint *kp1, *kp2;
    const int32_t *n1, *n2, *matches12;
    size_t kp_stride;
    int pairs, max_n, iters, draw_sets;
    unsigned long long seed;
    float fx, fy, cx, cy;
    float sigma, rh_threshold, min_parallax;
    int min_triangulated;
    // work arena
    int32_t *w_n;                 // [pairs] N
    float *w_norm;                // [pairs][8] sX1 sY1 meanX1 meanY1 sX2 sY2 meanX2 meanY2
    float4 *w_pts;                // [pairs][max_n] (u1, v1, u2, v2) of match i
    int32_t *w_idx1;              // [pairs][max_n] first keypoint index of match i
    float *w_hyp;                 // [pairs][iters][TVR_HYP_STRIDE]
    float *w_scores;              // [pairs][iters][2]
    // caller arrays
    int32_t *sets;
    uint8_t *ok, *tri;
    float *R21, *t21, *P3D;
    orbhip_tvr_stats *stats;
    float *hyp_scores, *hyp_mats;
    int32_t *status;
};

__device__ __forceinline__ float tvr_wave_sum_f32(float v)
{
#define TVR_STEP(CTRL, RM) v += __builtin_bit_cast(float, dpp_mov<CTRL, RM>(0, __builtin_bit_cast(int, v)))
    TVR_STEP(ORB_DPP_ROW_SHR(1), 0xF); TVR_STEP(ORB_DPP_ROW_SHR(2), 0xF); TVR_STEP(ORB_DPP_ROW_SHR(4), 0xF); TVR_STEP(ORB_DPP_ROW_SHR(8), 0xF);
    TVR_STEP(ORB_DPP_ROW_BCAST15, 0xA); TVR_STEP(ORB_DPP_ROW_BCAST31, 0xC);
#undef TVR_STEP
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// sum of a double over the workgroup (TVR_THREADS lanes), fixed association; every lane gets the result
__device__ double tvr_block_sum_f64(double v, double *s_w)
{
    const double w = wave_sum_f64_dpp(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = w;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// Normalize (:753-799) of one frame: sums in double over a fixed tree, the rest in float as there
__device__ void tvr_normalize(const orbhip_keypoint *kp, int n, double *s_w, float *out4)
{
    double sx = 0, sy = 0;
    for (int i = threadIdx.x; i < n; i += TVR_THREADS) { sx += (double)kp[i].x; sy += (double)kp[i].y; }
    sx = tvr_block_sum_f64(sx, s_w); sy = tvr_block_sum_f64(sy, s_w);
    const float meanX = (float)(sx / (double)n), meanY = (float)(sy / (double)n);
    double dx = 0, dy = 0;
    for (int i = threadIdx.x; i < n; i += TVR_THREADS) { dx += (double)fabsf(kp[i].x - meanX); dy += (double)fabsf(kp[i].y - meanY); }
    dx = tvr_block_sum_f64(dx, s_w); dy = tvr_block_sum_f64(dy, s_w);
    const float meanDevX = (float)(dx / (double)n), meanDevY = (float)(dy / (double)n);
    if (threadIdx.x == 0) { out4[0] = 1.0f / meanDevX; out4[1] = 1.0f / meanDevY; out4[2] = meanX; out4[3] = meanY; }
}

__global__ __launch_bounds__(TVR_THREADS) void k_tvr_prepare(TvrArgs a)
{
    __shared__ double s_w[4];
    __shared__ int s_wc[4];
    __shared__ int s_base;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n1 = a.n1[pair], n2 = a.n2[pair];
    if (n1 > a.max_n || n2 > a.max_n) {
        if (tid == 0) atomicExch(a.status, ORBHIP_E_CAPACITY);
        n1 = 0; n2 = 0;
    }
    if (n1 < 0) n1 = 0;
    if (n2 < 0) n2 = 0;
    const orbhip_keypoint *kp1 = a.kp1 + (size_t)pair * a.kp_stride, *kp2 = a.kp2 + (size_t)pair * a.kp_stride;
    const int32_t *m12 = a.matches12 + (size_t)pair * a.max_n;
    float4 *pts = a.w_pts + (size_t)pair * a.max_n;
    int32_t *idx1 = a.w_idx1 + (size_t)pair * a.max_n;
    // reset of the outputs: what a failed Reconstruct leaves (R21 / t21 empty, nothing triangulated)
    for (int i = tid; i < n1; i += TVR_THREADS) {
        float *p = a.P3D + ((size_t)pair * a.max_n + i) * 3;
        p[0] = 0.f; p[1] = 0.f; p[2] = 0.f;
        a.tri[(size_t)pair * a.max_n + i] = 0;
    }
    if (tid < 9) a.R21[(size_t)pair * 9 + tid] = 0.f;
    if (tid < 3) a.t21[(size_t)pair * 3 + tid] = 0.f;
    if (tid == 0) { a.ok[pair] = 0; s_base = 0; }
    __syncthreads();
    // mvMatches12 (:53-62): the matched first-frame keypoints in index order.  An entry that points beyond the second frame is no match.
    for (int start = 0; start < n1; start += TVR_THREADS) {
        const int i = start + tid;
        int m = -1;
        if (i < n1) { m = m12[i]; if (m >= n2) m = -1; }
        const unsigned long long b = __ballot(m >= 0);
        if (lane == 0) s_wc[wave] = (int)__popcll(b);
        __syncthreads();
        int off = s_base + (int)__popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) off += s_wc[w];
        if (m >= 0) {
            const orbhip_keypoint k1 = kp1[i], k2 = kp2[m];
            pts[off] = make_float4(k1.x, k1.y, k2.x, k2.y);
            idx1[off] = i;
        }
        __syncthreads();
        if (tid == 0) s_base += s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
        __syncthreads();
    }
    const int N = s_base;
    if (tid == 0) a.w_n[pair] = N;
    if (n1 > 0) tvr_normalize(kp1, n1, s_w, a.w_norm + (size_t)pair * 8);
    if (n2 > 0) tvr_normalize(kp2, n2, s_w, a.w_norm + (size_t)pair * 8 + 4);
    if (!a.draw_sets) return;
    // mvSets (:81-96): per iteration 8 draws without replacement, swap-with-last on 0..N-1
    for (int it = tid; it < a.iters; it += TVR_THREADS) ransac_draw_set<8>(a.seed, pair, it, N, a.sets + ((size_t)pair * a.iters + it) * 8);
}

// ------------------------------------------------------------------------------------------------ 3x3 decompositions (double, registers)
// A = U diag(w) V^T, w descending, one-sided Jacobi on the columns.  Row-major 3x3 arrays.  A rank-deficient A gets its missing left
// vectors from cross products, so U is always orthonormal.
__device__ void tvr_svd3(const double *A, double *U, double *w, double *V)
{
    double a[3][3], v[3][3];                  // a[j] = column j of A V, v[j] = column j of V
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) { a[j][i] = A[3 * i + j]; v[j][i] = i == j ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < 40; sweep++) {
        bool rot = false;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = i + 1; j < 3; j++) {
                const double al = a[i][0] * a[i][0] + a[i][1] * a[i][1] + a[i][2] * a[i][2];
                const double be = a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2];
                const double ga = a[i][0] * a[j][0] + a[i][1] * a[j][1] + a[i][2] * a[j][2];
                if (!(fabs(ga) > 1e-16 * sqrt(al * be))) continue;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double x = a[i][k], y = a[j][k];
                    a[i][k] = c * x - s * y; a[j][k] = s * x + c * y;
                    const double p = v[i][k], q = v[j][k];
                    v[i][k] = c * p - s * q; v[j][k] = s * p + c * q;
                }
                rot = true;
            }
        if (!rot) break;
    }
    double n[3];
#pragma unroll
    for (int j = 0; j < 3; j++) n[j] = sqrt(a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2]);
#define TVR_CSWAP(I, J) if (n[I] < n[J]) { double t_ = n[I]; n[I] = n[J]; n[J] = t_; \
        for (int k = 0; k < 3; k++) { t_ = a[I][k]; a[I][k] = a[J][k]; a[J][k] = t_; t_ = v[I][k]; v[I][k] = v[J][k]; v[J][k] = t_; } }
    TVR_CSWAP(0, 1) TVR_CSWAP(0, 2) TVR_CSWAP(1, 2)
#undef TVR_CSWAP
    double u[3][3];
    const double tiny = 1e-13 * n[0];
    if (n[0] > 0) { u[0][0] = a[0][0] / n[0]; u[0][1] = a[0][1] / n[0]; u[0][2] = a[0][2] / n[0]; }
    else { u[0][0] = 1; u[0][1] = 0; u[0][2] = 0; }
    if (n[1] > tiny) { u[1][0] = a[1][0] / n[1]; u[1][1] = a[1][1] / n[1]; u[1][2] = a[1][2] / n[1]; }
    else {                                      // any unit vector orthogonal to u0: cross with the axis of its smallest component
        const double ax = fabs(u[0][0]), ay = fabs(u[0][1]), az = fabs(u[0][2]);
        double e0 = 0, e1 = 0, e2 = 0;
        if (ax <= ay && ax <= az) e0 = 1; else if (ay <= az) e1 = 1; else e2 = 1;
        double c0 = u[0][1] * e2 - u[0][2] * e1, c1 = u[0][2] * e0 - u[0][0] * e2, c2 = u[0][0] * e1 - u[0][1] * e0;
        const double cn = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
        u[1][0] = c0 / cn; u[1][1] = c1 / cn; u[1][2] = c2 / cn;
    }
    if (n[2] > tiny) { u[2][0] = a[2][0] / n[2]; u[2][1] = a[2][1] / n[2]; u[2][2] = a[2][2] / n[2]; }
    else {
        u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
        u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
        u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        w[j] = n[j];
#pragma unroll
        for (int i = 0; i < 3; i++) { U[3 * i + j] = u[j][i]; V[3 * i + j] = v[j][i]; }
    }
}
__device__ __forceinline__ double tvr_det3(const double *M)
{
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
// (not geom3.h's mm3 / mtm3: those are contracted to FMAs and go through a temporary; this file compiles un-contracted and writes in place)
__device__ __forceinline__ void tvr_mul3(const double *A, const double *B, double *C)        // C = A B
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void tvr_mul3t(const double *A, const double *B, double *C)       // C = A B^T
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
// cv::invert of a 3x3 CV_32F matrix: cofactors and determinant in double, each entry rounded once
__device__ void tvr_inv3f(const float *S, float *T)
{
#define S_(i, j) ((double)S[3 * (i) + (j)])
    double d = S_(0, 0) * (S_(1, 1) * S_(2, 2) - S_(1, 2) * S_(2, 1)) - S_(0, 1) * (S_(1, 0) * S_(2, 2) - S_(1, 2) * S_(2, 0)) +
               S_(0, 2) * (S_(1, 0) * S_(2, 1) - S_(1, 1) * S_(2, 0));
    if (d == 0.0) {
#pragma unroll
        for (int k = 0; k < 9; k++) T[k] = 0.f;
        return;
    }
    d = 1.0 / d;
    T[0] = (float)((S_(1, 1) * S_(2, 2) - S_(1, 2) * S_(2, 1)) * d);
    T[1] = (float)((S_(0, 2) * S_(2, 1) - S_(0, 1) * S_(2, 2)) * d);
    T[2] = (float)((S_(0, 1) * S_(1, 2) - S_(0, 2) * S_(1, 1)) * d);
    T[3] = (float)((S_(1, 2) * S_(2, 0) - S_(1, 0) * S_(2, 2)) * d);
    T[4] = (float)((S_(0, 0) * S_(2, 2) - S_(0, 2) * S_(2, 0)) * d);
    T[5] = (float)((S_(0, 2) * S_(1, 0) - S_(0, 0) * S_(1, 2)) * d);
    T[6] = (float)((S_(1, 0) * S_(2, 1) - S_(1, 1) * S_(2, 0)) * d);
    T[7] = (float)((S_(0, 1) * S_(2, 0) - S_(0, 0) * S_(2, 1)) * d);
    T[8] = (float)((S_(0, 0) * S_(1, 1) - S_(0, 1) * S_(1, 0)) * d);
#undef S_
}

// ------------------------------------------------------------------------------------------------ hypotheses
// One lane per (pair, iteration); blockIdx.y = model (0 H, 1 F).  LDS: the upper triangle of G [45][64] and V [81][64] doubles,
// lane-interleaved: 63 KB per wave, so two waves share a CU's 160 KB (the full G would be 81 KB: one).
#define TVR_HYP_LANES 64
#define TVR_HYP_LDS ((45 + 81) * TVR_HYP_LANES * sizeof(double))
__global__ __launch_bounds__(TVR_HYP_LANES) void k_tvr_hyp(TvrArgs a)
{
    extern __shared__ double tvr_hyp_lds[];
    double *G = tvr_hyp_lds + threadIdx.x, *V = G + 45 * TVR_HYP_LANES;
#define GU(r, c) G[((r) * 9 - ((r) * ((r) - 1)) / 2 + ((c) - (r))) * TVR_HYP_LANES]        // r <= c
#define GE(r, c) GU(min(r, c), max(r, c))
#define VE(r, c) V[((r) * 9 + (c)) * TVR_HYP_LANES]
    const int model = blockIdx.y;
    const long long gid = (long long)blockIdx.x * TVR_HYP_LANES + threadIdx.x, total = (long long)a.pairs * a.iters;
    const bool in_range = gid < total;
    const int pair = in_range ? (int)(gid / a.iters) : 0, it = in_range ? (int)(gid % a.iters) : 0;
    const int N = a.w_n[pair];
    const int32_t *set = a.sets + ((size_t)pair * a.iters + it) * 8;
    bool act = in_range && N >= 8;
    int sidx[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { sidx[j] = act ? set[j] : 0; if (sidx[j] < 0 || sidx[j] >= N) { act = false; sidx[j] = 0; } }
    const float *nrm = a.w_norm + (size_t)pair * 8;
    const float sX1 = nrm[0], sY1 = nrm[1], mX1 = nrm[2], mY1 = nrm[3], sX2 = nrm[4], sY2 = nrm[5], mX2 = nrm[6], mY2 = nrm[7];
    const float4 *pts = a.w_pts + (size_t)pair * a.max_n;
    double g[45];
#pragma unroll
    for (int k = 0; k < 45; k++) g[k] = 0.0;
    if (act) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float4 p = pts[sidx[j]];
            const float u1 = (p.x - mX1) * sX1, v1 = (p.y - mY1) * sY1, u2 = (p.z - mX2) * sX2, v2 = (p.w - mY2) * sY2;
            float r0[9], r1[9];
            if (model == 0) {                                                  // ComputeH21 (:244-262)
                r0[0] = 0.f; r0[1] = 0.f; r0[2] = 0.f; r0[3] = -u1; r0[4] = -v1; r0[5] = -1.f; r0[6] = v2 * u1; r0[7] = v2 * v1; r0[8] = v2;
                r1[0] = u1; r1[1] = v1; r1[2] = 1.f; r1[3] = 0.f; r1[4] = 0.f; r1[5] = 0.f; r1[6] = -u2 * u1; r1[7] = -u2 * v1; r1[8] = -u2;
            } else {                                                           // ComputeF21 (:286-294)
                r0[0] = u2 * u1; r0[1] = u2 * v1; r0[2] = u2; r0[3] = v2 * u1; r0[4] = v2 * v1; r0[5] = v2; r0[6] = u1; r0[7] = v1; r0[8] = 1.f;
#pragma unroll
                for (int k = 0; k < 9; k++) r1[k] = 0.f;
            }
            int e = 0;
#pragma unroll
            for (int r = 0; r < 9; r++)
#pragma unroll
                for (int c = r; c < 9; c++) { g[e] += (double)r0[r] * (double)r0[c] + (double)r1[r] * (double)r1[c]; e++; }
        }
    }
    double trace = 0;
    {
        int e = 0;
#pragma unroll
        for (int r = 0; r < 9; r++)
#pragma unroll
            for (int c = r; c < 9; c++) {
                G[e * TVR_HYP_LANES] = g[e];
                VE(r, c) = r == c ? 1.0 : 0.0; VE(c, r) = r == c ? 1.0 : 0.0;
                if (r == c) trace += g[e];
                e++;
            }
    }
    const double thr = 1e-17 * trace;
#pragma unroll 1
    for (int sweep = 0; sweep < 24; sweep++) {
        bool rot = false;
#pragma unroll 1
        for (int p = 0; p < 8; p++)
#pragma unroll 1
            for (int q = p + 1; q < 9; q++) {
                const double gpq = GE(p, q);
                if (!(act && fabs(gpq) > thr)) continue;
                const double gpp = GE(p, p), gqq = GE(q, q);
                const double theta = (gqq - gpp) / (2.0 * gpq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const double vkp = VE(k, p), vkq = VE(k, q);
                    VE(k, p) = c * vkp - s * vkq; VE(k, q) = s * vkp + c * vkq;
                    if (k == p || k == q) continue;
                    const double gkp = GE(k, p), gkq = GE(k, q);
                    const double np_ = c * gkp - s * gkq, nq_ = s * gkp + c * gkq;
                    GE(k, p) = np_; GE(k, q) = nq_;
                }
                GE(p, p) = gpp - t * gpq; GE(q, q) = gqq + t * gpq; GE(p, q) = 0.0;
                rot = true;
            }
        if (!__any(rot)) break;
    }
    if (!in_range) return;
    float *out = a.w_hyp + ((size_t)pair * a.iters + it) * TVR_HYP_STRIDE;
    float *mats = a.hyp_mats ? a.hyp_mats + (((size_t)pair * a.iters + it) * 2 + model) * 9 : nullptr;
    if (!act) {
        if (model == 0) {
#pragma unroll
            for (int k = 0; k < 18; k++) out[k] = 0.f;
            out[27] = 0.f;
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) out[18 + k] = 0.f;
        }
        if (mats) {
#pragma unroll
            for (int k = 0; k < 9; k++) mats[k] = 0.f;
        }
        return;
    }
    int m = 0;
    double dmin = GE(0, 0);
#pragma unroll 1
    for (int k = 1; k < 9; k++) { const double d = GE(k, k); if (d < dmin) { dmin = d; m = k; } }
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = V[(k * 9 + m) * TVR_HYP_LANES];
    // T1 (:794-798), float entries as there
    const double t1x = (double)(-mX1 * sX1), t1y = (double)(-mY1 * sY1);
    if (model == 0) {
        // H21i = T2inv * Hn * T1 (:165)
        float H21[9], H12[9];
        double M[9];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            M[3 * r] = h[3 * r] * (double)sX1; M[3 * r + 1] = h[3 * r + 1] * (double)sY1;
            M[3 * r + 2] = h[3 * r] * t1x + h[3 * r + 1] * t1y + h[3 * r + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            H21[c] = (float)(M[c] / (double)sX2 + (double)mX2 * M[6 + c]);
            H21[3 + c] = (float)(M[3 + c] / (double)sY2 + (double)mY2 * M[6 + c]);
            H21[6 + c] = (float)M[6 + c];
        }
        tvr_inv3f(H21, H12);                                                   // H12i = H21i.inv() (:166)
#pragma unroll
        for (int k = 0; k < 9; k++) { out[k] = H21[k]; out[9 + k] = H12[k]; if (mats) mats[k] = H21[k]; }
        out[27] = 1.f;
    } else {
        // rank 2 (:301-307), then F21i = T2t * Fn * T1 (:217)
        double U[9], w[3], Vv[9], UW[9], Fn[9], M[9];
        tvr_svd3(h, U, w, Vv);
#pragma unroll
        for (int i = 0; i < 3; i++) { UW[3 * i] = U[3 * i] * w[0]; UW[3 * i + 1] = U[3 * i + 1] * w[1]; UW[3 * i + 2] = 0.0; }
        tvr_mul3t(UW, Vv, Fn);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            M[3 * r] = Fn[3 * r] * (double)sX1; M[3 * r + 1] = Fn[3 * r + 1] * (double)sY1;
            M[3 * r + 2] = Fn[3 * r] * t1x + Fn[3 * r + 1] * t1y + Fn[3 * r + 2];
        }
        const double t2x = (double)(-mX2 * sX2), t2y = (double)(-mY2 * sY2);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float f0 = (float)((double)sX2 * M[c]), f1 = (float)((double)sY2 * M[3 + c]);
            const float f2 = (float)(t2x * M[c] + t2y * M[3 + c] + M[6 + c]);
            out[18 + c] = f0; out[21 + c] = f1; out[24 + c] = f2;
            if (mats) { mats[c] = f0; mats[3 + c] = f1; mats[6 + c] = f2; }
        }
    }
#undef GE
#undef GU
#undef VE
}

// ------------------------------------------------------------------------------------------------ scoring
// CheckHomography (:342-390), one match: adds to score, returns bIn
__device__ __forceinline__ bool tvr_check_h(const float *H, const float *Hi, float u1, float v1, float u2, float v2, float invSigmaSquare, float &score)
{
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = 1.0f / (Hi[6] * u2 + Hi[7] * v2 + Hi[8]);
    const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
    const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false; else score += th - chiSquare1;
    const float w1in2inv = 1.0f / (H[6] * u1 + H[7] * v1 + H[8]);
    const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
    const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false; else score += th - chiSquare2;
    return bIn;
}
// CheckFundamental (:418-470)
__device__ __forceinline__ bool tvr_check_f(const float *F, float u1, float v1, float u2, float v2, float invSigmaSquare, float &score)
{
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false; else score += thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false; else score += thScore - chiSquare2;
    return bIn;
}

__global__ __launch_bounds__(TVR_THREADS) void k_tvr_score(TvrArgs a)
{
    extern __shared__ float4 tvr_score_pts[];                                  // [max_n]
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.w_n[pair];
    const float4 *pts = a.w_pts + (size_t)pair * a.max_n;
    for (int i = tid; i < N; i += TVR_THREADS) tvr_score_pts[i] = pts[i];
    __syncthreads();
    const float invSigmaSquare = 1.0f / (a.sigma * a.sigma);
    const int it0 = blockIdx.y * TVR_SCORE_ITERS;
    for (int task = wave; task < 2 * TVR_SCORE_ITERS; task += TVR_THREADS / 64) {
        const int it = it0 + (task >> 1), model = task & 1;
        if (it >= a.iters) break;
        const float *hp = a.w_hyp + ((size_t)pair * a.iters + it) * TVR_HYP_STRIDE;
        const bool valid = N >= 8 && hp[27] != 0.f;
        float sc = 0.f;
        if (valid) {
            float M[18];
            if (model == 0) {
#pragma unroll
                for (int k = 0; k < 18; k++) M[k] = hp[k];
                for (int i = lane; i < N; i += 64) {
                    const float4 p = tvr_score_pts[i];
                    tvr_check_h(M, M + 9, p.x, p.y, p.z, p.w, invSigmaSquare, sc);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 9; k++) M[k] = hp[18 + k];
                for (int i = lane; i < N; i += 64) {
                    const float4 p = tvr_score_pts[i];
                    tvr_check_f(M, p.x, p.y, p.z, p.w, invSigmaSquare, sc);
                }
            }
        }
        sc = tvr_wave_sum_f32(sc);
        if (lane == 0) {
            const size_t o = ((size_t)pair * a.iters + it) * 2 + model;
            a.w_scores[o] = sc;
            if (a.hyp_scores) a.hyp_scores[o] = sc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ reconstruction
struct TvrHypRT { float R[9], t[3], P2[12], O2[3]; };

// one match of CheckRT (:834-898) for motion hypothesis h.  Returns 0 rejected, 1 counted (nGood), 3 counted and vbGood.
__device__ int tvr_check_rt_one(const TvrHypRT &h, float fx, float fy, float cx, float cy, float4 p, float th2, float &cos_out, float *X)
{
    // Triangulate (:738-751): A rows from P1 = K [I | 0] and P2 = K [R | t]; At[j] = column j of A
    float At[4][4], v[4];
    const float P1r0[4] = {fx, 0.f, cx, 0.f}, P1r1[4] = {0.f, fy, cy, 0.f}, P1r2[4] = {0.f, 0.f, 1.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        At[j][0] = p.x * P1r2[j] - P1r0[j];
        At[j][1] = p.y * P1r2[j] - P1r1[j];
        At[j][2] = p.z * h.P2[8 + j] - h.P2[j];
        At[j][3] = p.w * h.P2[8 + j] - h.P2[4 + j];
    }
    tri_svd4_null(At, v);
    const float x0 = v[0] / v[3], x1 = v[1] / v[3], x2 = v[2] / v[3];
    if (!isfinite(x0) || !isfinite(x1) || !isfinite(x2)) return 0;
    // parallax (:852-858): cv::norm and Mat::dot return doubles
    const float dist1 = (float)sqrt((double)x0 * x0 + (double)x1 * x1 + (double)x2 * x2);
    const float n2x = x0 - h.O2[0], n2y = x1 - h.O2[1], n2z = x2 - h.O2[2];
    const float dist2 = (float)sqrt((double)n2x * n2x + (double)n2y * n2y + (double)n2z * n2z);
    const float cosParallax = (float)(((double)x0 * n2x + (double)x1 * n2y + (double)x2 * n2z) / (double)(dist1 * dist2));
    if (x2 <= 0.f && (double)cosParallax < 0.99998) return 0;
    const float y0 = (float)((double)h.R[0] * x0 + (double)h.R[1] * x1 + (double)h.R[2] * x2) + h.t[0];
    const float y1 = (float)((double)h.R[3] * x0 + (double)h.R[4] * x1 + (double)h.R[5] * x2) + h.t[1];
    const float y2 = (float)((double)h.R[6] * x0 + (double)h.R[7] * x1 + (double)h.R[8] * x2) + h.t[2];
    if (y2 <= 0.f && (double)cosParallax < 0.99998) return 0;
    const float invZ1 = 1.0f / x2;
    const float im1x = fx * x0 * invZ1 + cx, im1y = fy * x1 * invZ1 + cy;
    const float squareError1 = (im1x - p.x) * (im1x - p.x) + (im1y - p.y) * (im1y - p.y);
    if (squareError1 > th2) return 0;
    const float invZ2 = 1.0f / y2;
    const float im2x = fx * y0 * invZ2 + cx, im2y = fy * y1 * invZ2 + cy;
    const float squareError2 = (im2x - p.z) * (im2x - p.z) + (im2y - p.w) * (im2y - p.w);
    if (squareError2 > th2) return 0;
    cos_out = cosParallax; X[0] = x0; X[1] = x1; X[2] = x2;
    return (double)cosParallax < 0.99998 ? 3 : 1;
}

__device__ void tvr_fill_hyp(TvrHypRT &h, const double *R, const double *t, float fx, float fy, float cx, float cy)
{
#pragma unroll
    for (int k = 0; k < 9; k++) h.R[k] = (float)R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) h.t[k] = (float)t[k];
#pragma unroll
    for (int j = 0; j < 4; j++) {                                              // P2 = K * [R | t] (:825-828)
        const double r0 = j < 3 ? (double)h.R[j] : (double)h.t[0], r1 = j < 3 ? (double)h.R[3 + j] : (double)h.t[1], r2 = j < 3 ? (double)h.R[6 + j] : (double)h.t[2];
        h.P2[j] = (float)((double)fx * r0 + (double)cx * r2);
        h.P2[4 + j] = (float)((double)fy * r1 + (double)cy * r2);
        h.P2[8 + j] = (float)r2;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)                                                // O2 = -R.t() * t (:830)
        h.O2[i] = -(float)((double)h.R[i] * h.t[0] + (double)h.R[3 + i] * h.t[1] + (double)h.R[6 + i] * h.t[2]);
}

__device__ __forceinline__ unsigned tvr_sort_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float tvr_key_float(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__global__ __launch_bounds__(TVR_THREADS) void k_tvr_reconstruct(TvrArgs a)
{
    extern __shared__ float tvr_rec_lds[];
    float *cosv = tvr_rec_lds;                                                 // [max_n] cosParallax of the taken hypothesis' good points
    uint8_t *inl = reinterpret_cast<uint8_t *>(cosv + a.max_n);               // [max_n] vbMatchesInliers of the model taken
    __shared__ float s_sc[2][TVR_THREADS];
    __shared__ int s_ix[2][TVR_THREADS];
    __shared__ TvrHypRT s_h[8];
    __shared__ float s_M[18];
    __shared__ int s_good[8];
    __shared__ int s_model, s_nhyp, s_ninl, s_sel, s_cnt, s_c, s_pre;
    __shared__ orbhip_tvr_stats s_st;
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int N = a.w_n[pair];
    const float4 *pts = a.w_pts + (size_t)pair * a.max_n;
    const int32_t *idx1 = a.w_idx1 + (size_t)pair * a.max_n;
    const float *scores = a.w_scores + (size_t)pair * a.iters * 2;
    // the argmax of :170 / :221: strictly greater wins, so the lowest iteration among equal scores; a score of 0 (or NaN) never wins
    {
        float bh = 0.f, bf = 0.f;
        int ih = -1, jf = -1;
        for (int it = tid; it < a.iters; it += TVR_THREADS) {
            const float sh = scores[2 * it], sf = scores[2 * it + 1];
            if (sh > bh) { bh = sh; ih = it; }
            if (sf > bf) { bf = sf; jf = it; }
        }
        s_sc[0][tid] = bh; s_ix[0][tid] = ih; s_sc[1][tid] = bf; s_ix[1][tid] = jf;
    }
    if (tid < 8) s_good[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        float best[2] = {0.f, 0.f};
        int bi[2] = {-1, -1};
        for (int m = 0; m < 2; m++)
            for (int k = 0; k < TVR_THREADS; k++) {
                const float s = s_sc[m][k];
                const int i = s_ix[m][k];
                if (i >= 0 && (s > best[m] || (s == best[m] && i < bi[m]))) { best[m] = s; bi[m] = i; }
            }
        const float SH = best[0], SF = best[1];
        memset(&s_st, 0, sizeof(s_st));
        s_st.n_matches = N; s_st.score_h = SH; s_st.score_f = SF; s_st.iter_h = bi[0]; s_st.iter_f = bi[1]; s_st.hyp_index = -1;
        int model = 0;
        if (SH + SF != 0.f) {                                                  // :111-126
            const float RH = SH / (SH + SF);
            model = RH > a.rh_threshold ? 1 : 2;
            if ((model == 1 && bi[0] < 0) || (model == 2 && bi[1] < 0)) model = 0;       // no matrix of that model: the reference has none to decompose
        }
        s_st.model = model;
        int nhyp = 0;
        if (model) {
            const float *hp = a.w_hyp + ((size_t)pair * a.iters + bi[model - 1]) * TVR_HYP_STRIDE;
            if (model == 1) { for (int k = 0; k < 18; k++) s_M[k] = hp[k]; }
            else { for (int k = 0; k < 9; k++) s_M[k] = hp[18 + k]; }
            const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
            double U[9], w[3], V[9];
            if (model == 2) {
                // E21 = K.t() * F21 * K (:484), DecomposeE (:913-933)
                double E[9];
                const double F0 = s_M[0], F1 = s_M[1], F2 = s_M[2], F3 = s_M[3], F4 = s_M[4], F5 = s_M[5], F6 = s_M[6], F7 = s_M[7], F8 = s_M[8];
                const double FK[9] = {F0 * fx, F1 * fy, F0 * cx + F1 * cy + F2, F3 * fx, F4 * fy, F3 * cx + F4 * cy + F5, F6 * fx, F7 * fy, F6 * cx + F7 * cy + F8};
                for (int c = 0; c < 3; c++) { E[c] = fx * FK[c]; E[3 + c] = fy * FK[3 + c]; E[6 + c] = cx * FK[c] + cy * FK[3 + c] + FK[6 + c]; }
                for (int k = 0; k < 9; k++) E[k] = (double)(float)E[k];
                tvr_svd3(E, U, w, V);
                double t[3] = {U[2], U[5], U[8]};
                const double tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
                for (int k = 0; k < 3; k++) t[k] /= tn;
                const double W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
                double UW[9], R1[9], R2[9];
                tvr_mul3(U, W, UW); tvr_mul3t(UW, V, R1);
                if (tvr_det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = -R1[k];
                tvr_mul3(U, Wt, UW); tvr_mul3t(UW, V, R2);
                if (tvr_det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = -R2[k];
                const double t2[3] = {-t[0], -t[1], -t[2]};
                tvr_fill_hyp(s_h[0], R1, t, a.fx, a.fy, a.cx, a.cy); tvr_fill_hyp(s_h[1], R2, t, a.fx, a.fy, a.cx, a.cy);
                tvr_fill_hyp(s_h[2], R1, t2, a.fx, a.fy, a.cx, a.cy); tvr_fill_hyp(s_h[3], R2, t2, a.fx, a.fy, a.cx, a.cy);
                nhyp = 4;
            } else {
                // A = invK * H21 * K (:588-589), Faugeras (:591-690)
                double H[9], HK[9], A[9];
                for (int k = 0; k < 9; k++) H[k] = s_M[k];
                for (int r = 0; r < 3; r++) { HK[3 * r] = H[3 * r] * fx; HK[3 * r + 1] = H[3 * r + 1] * fy; HK[3 * r + 2] = H[3 * r] * cx + H[3 * r + 1] * cy + H[3 * r + 2]; }
                for (int c = 0; c < 3; c++) { A[c] = (HK[c] - cx * HK[6 + c]) / fx; A[3 + c] = (HK[3 + c] - cy * HK[6 + c]) / fy; A[6 + c] = HK[6 + c]; }
                for (int k = 0; k < 9; k++) A[k] = (double)(float)A[k];
                tvr_svd3(A, U, w, V);
                double Vt[9];
                for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Vt[3 * i + j] = V[3 * j + i];
                const float s = (float)(tvr_det3(U) * tvr_det3(Vt));
                const float d1 = (float)w[0], d2 = (float)w[1], d3 = (float)w[2];
                if (!(d1 / d2 < 1.00001f || d2 / d3 < 1.00001f) && isfinite(d1 / d2) && isfinite(d2 / d3)) {
                    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
                    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
                    const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
                    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
                    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
                    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
                    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
                    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
                    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
                    for (int i = 0; i < 8; i++) {
                        double Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tp[3];
                        if (i < 4) {
                            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
                            tp[0] = x1[i] * (d1 - d3); tp[1] = 0; tp[2] = -x3[i] * (d1 - d3);
                        } else {
                            Rp[0] = cphi; Rp[2] = sphi[i - 4]; Rp[4] = -1; Rp[6] = sphi[i - 4]; Rp[8] = -cphi;
                            tp[0] = x1[i - 4] * (d1 + d3); tp[1] = 0; tp[2] = x3[i - 4] * (d1 + d3);
                        }
                        double URp[9], R[9], t[3];
                        tvr_mul3(U, Rp, URp); tvr_mul3(URp, Vt, R);
                        for (int k = 0; k < 9; k++) R[k] *= (double)s;
                        for (int k = 0; k < 3; k++) t[k] = U[3 * k] * tp[0] + U[3 * k + 1] * tp[1] + U[3 * k + 2] * tp[2];
                        const double tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
                        for (int k = 0; k < 3; k++) t[k] /= tn;
                        tvr_fill_hyp(s_h[i], R, t, a.fx, a.fy, a.cx, a.cy);
                    }
                    nhyp = 8;
                }
            }
        }
        s_model = model; s_nhyp = nhyp; s_ninl = 0; s_sel = -1; s_cnt = 0; s_pre = 0;
        s_st.n_hyp = nhyp;
    }
    __syncthreads();
    const int model = s_model, nhyp = s_nhyp;
    if (model) {
        // vbMatchesInliers of the winner: the same arithmetic as the scoring pass
        const float invSigmaSquare = 1.0f / (a.sigma * a.sigma);
        int mine = 0;
        for (int i = tid; i < N; i += TVR_THREADS) {
            const float4 p = pts[i];
            float dummy = 0.f;
            const bool in = model == 1 ? tvr_check_h(s_M, s_M + 9, p.x, p.y, p.z, p.w, invSigmaSquare, dummy)
                                       : tvr_check_f(s_M, p.x, p.y, p.z, p.w, invSigmaSquare, dummy);
            inl[i] = in ? 1 : 0;
            mine += in ? 1 : 0;
        }
        if (mine) atomicAdd(&s_ninl, mine);
    }
    __syncthreads();
    const float th2 = (float)(4.0 * (double)(a.sigma * a.sigma));
    if (nhyp) {
        // CheckRT, counting pass: nGood of every motion hypothesis
        const int tasks = nhyp * N;
        for (int t = tid; t < tasks; t += TVR_THREADS) {
            const int h = t / N, i = t - h * N;
            if (!inl[i]) continue;
            float c, X[3];
            if (tvr_check_rt_one(s_h[h], a.fx, a.fy, a.cx, a.cy, pts[i], th2, c, X)) atomicAdd(&s_good[h], 1);
        }
    }
    __syncthreads();
    if (tid == 0 && nhyp) {
        const int Nin = s_ninl;
        int sel = -1, pre = 0;
        if (model == 2) {                                                      // ReconstructF :504-525
            const int g1 = s_good[0], g2 = s_good[1], g3 = s_good[2], g4 = s_good[3];
            const int maxGood = max(g1, max(g2, max(g3, g4)));
            const int nMinGood = max((int)(0.9 * Nin), a.min_triangulated);
            int nsimilar = 0;
            if (g1 > 0.7 * maxGood) nsimilar++;
            if (g2 > 0.7 * maxGood) nsimilar++;
            if (g3 > 0.7 * maxGood) nsimilar++;
            if (g4 > 0.7 * maxGood) nsimilar++;
            if (!(maxGood < nMinGood || nsimilar > 1)) {
                pre = 1;
                sel = maxGood == g1 ? 0 : maxGood == g2 ? 1 : maxGood == g3 ? 2 : 3;
            }
        } else {                                                               // ReconstructH :693-722
            int bestGood = 0, secondBestGood = 0, bestIdx = -1;
            for (int i = 0; i < 8; i++) {
                const int nGood = s_good[i];
                if (nGood > bestGood) { secondBestGood = bestGood; bestGood = nGood; bestIdx = i; }
                else if (nGood > secondBestGood) secondBestGood = nGood;
            }
            sel = bestIdx;
            pre = (secondBestGood < 0.75 * bestGood && bestGood > a.min_triangulated && bestGood > 0.9 * Nin) ? 1 : 0;
        }
        s_sel = sel; s_pre = pre;
    }
    __syncthreads();
    const int sel = s_sel;
    float *P3D = a.P3D + (size_t)pair * a.max_n * 3;
    uint8_t *tri = a.tri + (size_t)pair * a.max_n;
    if (sel >= 0) {
        // CheckRT of the hypothesis whose parallax decides: vP3D / vbGood by FIRST keypoint index (:893-897), the cosines for the selection
        for (int i = tid; i < N; i += TVR_THREADS) {
            if (!inl[i]) continue;
            float c, X[3];
            const int r = tvr_check_rt_one(s_h[sel], a.fx, a.fy, a.cx, a.cy, pts[i], th2, c, X);
            if (!r) continue;
            cosv[atomicAdd(&s_cnt, 1)] = c;
            const int k1 = idx1[i];
            P3D[3 * k1] = X[0]; P3D[3 * k1 + 1] = X[1]; P3D[3 * k1 + 2] = X[2];
            tri[k1] = r == 3 ? 1 : 0;
        }
    }
    __syncthreads();
    float parallax = 0.f;
    if (sel >= 0 && s_cnt > 0) {
        // sorted vCosParallax[min(50, n - 1)] (:902-905): the largest key with at most idx keys below it
        const int n = s_cnt, idx = min(50, n - 1);
        unsigned K = 0;
        for (int b = 31; b >= 0; b--) {
            const unsigned trial = K | (1u << b);
            if (tid == 0) s_c = 0;
            __syncthreads();
            int c = 0;
            for (int i = tid; i < n; i += TVR_THREADS) c += tvr_sort_key(cosv[i]) < trial ? 1 : 0;
            if (c) atomicAdd(&s_c, c);
            __syncthreads();
            if (s_c <= idx) K = trial;
            __syncthreads();
        }
        parallax = (float)((double)(acosf(tvr_key_float(K)) * 180.f) / 3.1415926535897932384626433832795);
    }
    bool okk = false;
    if (sel >= 0 && s_pre)
        okk = model == 2 ? parallax > a.min_parallax : parallax >= a.min_parallax;     // :530 (>) and :725 (>=)
    if (sel >= 0 && !okk) {
        // a rejected reconstruction leaves vP3D / vbTriangulated as they were: back to the reset values
        for (int i = tid; i < N; i += TVR_THREADS) {
            if (!inl[i]) continue;
            const int k1 = idx1[i];
            P3D[3 * k1] = 0.f; P3D[3 * k1 + 1] = 0.f; P3D[3 * k1 + 2] = 0.f; tri[k1] = 0;
        }
    }
    if (tid == 0) {
        if (okk) {
            for (int k = 0; k < 9; k++) a.R21[(size_t)pair * 9 + k] = s_h[sel].R[k];
            for (int k = 0; k < 3; k++) a.t21[(size_t)pair * 3 + k] = s_h[sel].t[k];
            a.ok[pair] = 1;
        }
        if (a.stats) {
            s_st.n_inliers = model ? s_ninl : 0;
            for (int k = 0; k < 8; k++) s_st.n_good[k] = k < nhyp ? s_good[k] : 0;
            s_st.hyp_index = sel; s_st.parallax = parallax;
            a.stats[pair] = s_st;
        }
    }
}

}  // namespace

extern "C" void orbhip_tvr_default_params(orbhip_tvr_params *p)
{
    if (!p) return;
    p->sigma = 1.0f; p->iterations = 200; p->rh_threshold = 0.50f; p->min_parallax = 1.0f; p->min_triangulated = 50;
    p->draw_sets = 1; p->seed = 0;
}

extern "C" int orbhip_two_view_reconstruct_device(orbhip_ctx *ctx, const orbhip_keypoint *d_kp1, const int32_t *d_n1, const orbhip_keypoint *d_kp2,
        const int32_t *d_n2, size_t frame_stride_kp, const int32_t *d_matches12, int pairs, int max_n, float fx, float fy, float cx, float cy,
        const orbhip_tvr_params *p, int32_t *d_sets, uint8_t *d_ok, float *d_R21, float *d_t21, float *d_P3D, uint8_t *d_triangulated,
        orbhip_tvr_stats *d_stats, float *d_hyp_scores, float *d_hyp_mats)
{
    if (!ctx || !d_kp1 || !d_n1 || !d_kp2 || !d_n2 || !d_matches12 || !p || !d_sets || !d_ok || !d_R21 || !d_t21 || !d_P3D || !d_triangulated ||
        pairs <= 0 || max_n <= 0 || frame_stride_kp < (size_t)max_n || p->iterations <= 0 || !(p->sigma > 0.f) || !(fx != 0.f) || !(fy != 0.f)) {
        orbhip_set_last_error_internal("orbhip_two_view_reconstruct_device: bad argument");
        return ORBHIP_E_BADARG;
    }
    if (int rc = ransac_check_capacity(max_n, p->iterations, RANSAC_CAPACITY_MSG("orbhip_two_view_reconstruct_device", "keypoints per frame"))) return rc;
    const int device = orbhip_ctx_device_internal(ctx);
    if (hipSetDevice(device) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    const int iters = p->iterations;
    const size_t P = (size_t)pairs;
    TvrArgs a;
    memset(&a, 0, sizeof(a));
    size_t bytes = 0;
    for (int pass = 0; pass < 2; pass++) {                                     // the arena's size, then its pointers
        Carve c{pass ? (char *)orbhip_ctx_work_internal(ctx, bytes + 256) : nullptr};
        if (pass && !c.base) return ORBHIP_E_HIP;
        a.w_n = c.take<int32_t>(P); a.w_norm = c.take<float>(8 * P); a.w_pts = c.take<float4>(P * max_n); a.w_idx1 = c.take<int32_t>(P * max_n);
        a.w_hyp = c.take<float>(P * iters * TVR_HYP_STRIDE); a.w_scores = c.take<float>(2 * P * iters);
        bytes = c.off;
    }
    a.kp1 = d_kp1; a.kp2 = d_kp2; a.n1 = d_n1; a.n2 = d_n2; a.matches12 = d_matches12; a.kp_stride = frame_stride_kp;
    a.pairs = pairs; a.max_n = max_n; a.iters = iters; a.draw_sets = p->draw_sets ? 1 : 0; a.seed = p->seed;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.sigma = p->sigma; a.rh_threshold = p->rh_threshold; a.min_parallax = p->min_parallax;
    a.min_triangulated = p->min_triangulated;
    a.sets = d_sets; a.ok = d_ok; a.tri = d_triangulated; a.R21 = d_R21; a.t21 = d_t21; a.P3D = d_P3D; a.stats = d_stats;
    a.hyp_scores = d_hyp_scores; a.hyp_mats = d_hyp_mats; a.status = orbhip_ctx_status_internal(ctx);
    const size_t lds_score = 16 * (size_t)max_n, lds_rec = 5 * (size_t)max_n + 16;
    if (orb_lds_optin(reinterpret_cast<const void *>(k_tvr_hyp), device, TVR_HYP_LDS) ||
        orb_lds_optin(reinterpret_cast<const void *>(k_tvr_score), device, lds_score) ||
        orb_lds_optin(reinterpret_cast<const void *>(k_tvr_reconstruct), device, lds_rec)) return ORBHIP_E_HIP;
    hipStream_t st = orbhip_ctx_stream_internal(ctx);
    hipLaunchKernelGGL(k_tvr_prepare, dim3(pairs), dim3(TVR_THREADS), 0, st, a);
    const long long total = (long long)pairs * iters;
    hipLaunchKernelGGL(k_tvr_hyp, dim3((unsigned)((total + TVR_HYP_LANES - 1) / TVR_HYP_LANES), 2), dim3(TVR_HYP_LANES), TVR_HYP_LDS, st, a);
    hipLaunchKernelGGL(k_tvr_score, dim3(pairs, (iters + TVR_SCORE_ITERS - 1) / TVR_SCORE_ITERS), dim3(TVR_THREADS), lds_score, st, a);
    hipLaunchKernelGGL(k_tvr_reconstruct, dim3(pairs), dim3(TVR_THREADS), lds_rec, st, a);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("two-view reconstruction launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
