// sim3solver_kernels.hip -- Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc:35-506), batched over loop candidates: the
// step between SearchByBoW and SearchByProjection / OptimizeSim3 in LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:673-684).
// A pair is one candidate (its correspondences X1c / X2c in the two cameras with their truncated thresholds); blockIdx.x carries the pair.
// Four launches per call, every pair of the batch in each; no workgroup waits on another:
//   k_s3s_prepare   FromCameraToImage (:492-506: mvP1im1 / mvP2im2, no z test), the 12 floats of a correspondence packed for the scoring
//                   passes, the iteration budget of SetRansacParameters (:126-150) in double, the RANSAC sets (:178-189) when the
//                   caller asks for them (both from ransac_common.h), reset of the outputs
//   k_s3s_hyp       ComputeSim3 (:316-427) per (pair, iteration), one lane per hypothesis: horn_sim3.h -- Horn in double on the float
//                   inputs, the 4x4 eigenproblem by cyclic Jacobi in registers, T12 / T21 / R12 / s12 rounded once to float
//   k_s3s_score     CheckInliers (:430-454) for every hypothesis, one wave per (pair, iteration), lanes striding the correspondences:
//                   Project (:472-490) as OpenCV's small-matrix gemm (host/cvmath.h mul_add) then GeometricCamera::project, float in
//                   the reference's operation order (-ffp-contract=off), the squared distance as Mat::dot (double sum, one rounding),
//                   `err < max` against the truncated threshold, counted by ballot + popcount (ransac_wave_count)
//   k_s3s_decide    one wave per pair: the scan rule of iterate() (:170-213) over count[] -- the first iteration with more than
//                   min_inliers converges, else the LAST arg-max (>= updates the best) --, the winner re-scored with the same device
//                   function (so the inlier flags carry the counted bits), the outputs
// A pair's correspondences are staged in LDS for scoring while they fit: 3 float4 each (X1c max1 | X2c max2 | p1 p2), at most
// S3S_LDS_MAX = 3072 of them = 144 KB of the 160 KB a workgroup can have, the rest left to the runtime; a longer pair is read
// through L2 by the same code (every wave of a workgroup walks the same rows at the same time).
// A hypothesis with a NaN entry (coincident points, |v| = 0) counts 0 inliers: every comparison with NaN is false, nothing traps.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "cam_project_f32.h"
#include "ransac_common.h"
#include "horn_sim3.h"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

#define S3S_THREADS 256
#define S3S_HYP_STRIDE 36         // floats per (pair, iteration): sR12 [9] t12 [3] sR21 [9] t21 [3] R12 [9] s12, valid, pad
#define S3S_SCORE_ITERS 32        // iterations per k_s3s_score workgroup
#define S3S_LDS_MAX 3072          // correspondences of a pair that k_s3s_score keeps in LDS (48 bytes each)

struct S3sArgs {
    const float *X1c, *X2c, *max1, *max2;
    const int32_t *n;
    int pairs, max_n, iters, min_inliers, fix_scale, draw_sets;
    double probability;
    unsigned long long seed;
    RansacCam c1, c2;
    // work arena
    int32_t *w_n;                 // [pairs] n, -1 for a pair whose count is out of range
    int32_t *w_budget;            // [pairs] mRansacMaxIts, 0 for n < min_inliers
    float4 *w_a, *w_b, *w_c;      // [pairs][max_n] (X1c, max1), (X2c, max2), (p1, p2)
    float *w_hyp;                 // [pairs][iters][S3S_HYP_STRIDE]
    int32_t *w_counts;            // [pairs][iters]
    // caller arrays
    int32_t *sets;
    uint8_t *converged, *inlier;
    float *R12, *t12, *s12;
    int32_t *n_inliers, *stats, *counts, *status;
};

// Rcw * X + tcw on CV_32F (cv::gemm's small-matrix path, host/cvmath.h mul_add): the row's products summed in float, then
// (float)(sum * 1.0 + t * 1.0) with the scalars double
__device__ __forceinline__ void s3s_gemm_add(const float *R, const float *t, float x, float y, float z, float *P)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float s = R[3 * i] * x + R[3 * i + 1] * y + R[3 * i + 2] * z;
        P[i] = (float)((double)s * 1.0 + (double)t[i] * 1.0);
    }
}
// one correspondence of CheckInliers (:438-452) under T = (sR12 t12 sR21 t21)
__device__ __forceinline__ bool s3s_inlier(const RansacCam &c1, const RansacCam &c2, const float *T, float4 a, float4 b, float4 c)
{
    float P[3], uv[2];
    s3s_gemm_add(T, T + 9, b.x, b.y, b.z, P);                                  // vP2im1 = project(cam1, T12 * X2c)
    tri_project(c1.type, c1.p, P, uv);
    const float d1x = c.x - uv[0], d1y = c.y - uv[1];                          // dist1 = mvP1im1[i] - vP2im1[i]
    const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
    s3s_gemm_add(T + 12, T + 21, a.x, a.y, a.z, P);                            // vP1im2 = project(cam2, T21 * X1c)
    tri_project(c2.type, c2.p, P, uv);
    const float d2x = uv[0] - c.z, d2y = uv[1] - c.w;                          // dist2 = vP1im2[i] - mvP2im2[i]
    const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
    return err1 < a.w && err2 < b.w;
}

__global__ __launch_bounds__(S3S_THREADS) void k_s3s_prepare(S3sArgs a)
{
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = a.n[pair];
    if (n < 0 || n > a.max_n) {                                                // status word; nothing of its rows is written
        if (tid == 0) {
            atomicExch(a.status, ORBHIP_E_CAPACITY);
            a.w_n[pair] = -1; a.w_budget[pair] = 0; a.converged[pair] = 0; a.n_inliers[pair] = 0;
            if (a.stats) { a.stats[3 * pair] = 0; a.stats[3 * pair + 1] = -1; a.stats[3 * pair + 2] = 0; }
        }
        return;
    }
    const size_t row = (size_t)pair * a.max_n;
    for (int i = tid; i < n; i += S3S_THREADS) {
        const float *x1 = a.X1c + (row + i) * 3, *x2 = a.X2c + (row + i) * 3;
        const float P1[3] = {x1[0], x1[1], x1[2]}, P2[3] = {x2[0], x2[1], x2[2]};
        float uv1[2], uv2[2];
        tri_project(a.c1.type, a.c1.p, P1, uv1);
        tri_project(a.c2.type, a.c2.p, P2, uv2);
        a.w_a[row + i] = make_float4(P1[0], P1[1], P1[2], a.max1[row + i]);
        a.w_b[row + i] = make_float4(P2[0], P2[1], P2[2], a.max2[row + i]);
        a.w_c[row + i] = make_float4(uv1[0], uv1[1], uv2[0], uv2[1]);
        a.inlier[row + i] = 0;
    }
    // SetRansacParameters (:126-150): epsilon = mRansacMinInliers / N in float
    const int budget = ransac_iteration_budget(n, a.min_inliers, (float)a.min_inliers / n, a.probability, a.iters);
    if (tid == 0) {
        a.w_n[pair] = n; a.w_budget[pair] = budget; a.converged[pair] = 0; a.n_inliers[pair] = 0;
    }
    if (!a.draw_sets) return;
    // :178-189: per iteration 3 draws without replacement, the drawn slot refilled with the last one
    for (int it = tid; it < a.iters; it += S3S_THREADS) ransac_draw_set<3>(a.seed, pair, it, n, a.sets + ((size_t)pair * a.iters + it) * 3);
}

__global__ __launch_bounds__(64) void k_s3s_hyp(S3sArgs a)
{
    const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (long long)a.pairs * a.iters) return;
    const int pair = (int)(gid / a.iters), it = (int)(gid % a.iters);
    const int n = a.w_n[pair];
    if (it >= a.w_budget[pair]) return;
    const int32_t *set = a.sets + ((size_t)pair * a.iters + it) * 3;
    const size_t row = (size_t)pair * a.max_n;
    float *out = a.w_hyp + ((size_t)pair * a.iters + it) * S3S_HYP_STRIDE;
    bool ok = true;
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        int s = set[j];
        if (s < 0 || s >= n) { ok = false; s = 0; }
        const float4 x1 = n > 0 ? a.w_a[row + s] : make_float4(0.f, 0.f, 0.f, 0.f), x2 = n > 0 ? a.w_b[row + s] : make_float4(0.f, 0.f, 0.f, 0.f);
        P1[j][0] = x1.x; P1[j][1] = x1.y; P1[j][2] = x1.z; P2[j][0] = x2.x; P2[j][1] = x2.y; P2[j][2] = x2.z;
    }
    HornSim3f h;
    horn_sim3(P1, P2, a.fix_scale != 0, h);
    const float nanv = __uint_as_float(0x7FC00000u);                           // a set with an index outside [0, n): no hypothesis
#pragma unroll
    for (int k = 0; k < 9; k++) { out[k] = ok ? h.sR12[k] : nanv; out[12 + k] = ok ? h.sR21[k] : nanv; out[24 + k] = ok ? h.R12[k] : nanv; }
#pragma unroll
    for (int k = 0; k < 3; k++) { out[9 + k] = ok ? h.t12[k] : nanv; out[21 + k] = ok ? h.t21[k] : nanv; }
    out[33] = ok ? h.s12 : nanv; out[34] = ok ? 1.f : 0.f; out[35] = 0.f;
}

// inliers of hypothesis T among the pair's n correspondences, counted by the whole wave; FLAGS: also written to row[]
template <bool FLAGS>
__device__ __forceinline__ int s3s_count(const RansacCam &c1, const RansacCam &c2, const float *T, const float4 *pa, const float4 *pb, const float4 *pc,
                                         int n, int lane, uint8_t *row)
{
    return ransac_wave_count<FLAGS>(n, lane, row, [&](int i) { return s3s_inlier(c1, c2, T, pa[i], pb[i], pc[i]); });
}

__global__ __launch_bounds__(S3S_THREADS) void k_s3s_score(S3sArgs a)
{
    extern __shared__ float4 s3s_lds[];                                        // [3][cap], cap = min(max_n, S3S_LDS_MAX)
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.w_n[pair], budget = a.w_budget[pair];
    const int it0 = blockIdx.y * S3S_SCORE_ITERS;
    if (n < 0) return;
    int32_t *counts = a.w_counts + (size_t)pair * a.iters, *ccounts = a.counts ? a.counts + (size_t)pair * a.iters : nullptr;
    if (it0 >= budget) {                                                       // iterations the budget leaves out: -1
        for (int k = tid; k < S3S_SCORE_ITERS && it0 + k < a.iters; k += S3S_THREADS) { counts[it0 + k] = -1; if (ccounts) ccounts[it0 + k] = -1; }
        return;
    }
    const size_t row = (size_t)pair * a.max_n;
    const int cap = min(a.max_n, S3S_LDS_MAX);
    const bool resident = n <= cap;
    if (resident) {
        for (int i = tid; i < n; i += S3S_THREADS) { s3s_lds[i] = a.w_a[row + i]; s3s_lds[cap + i] = a.w_b[row + i]; s3s_lds[2 * cap + i] = a.w_c[row + i]; }
    }
    __syncthreads();
    for (int k = wave; k < S3S_SCORE_ITERS; k += S3S_THREADS / 64) {
        const int it = it0 + k;
        if (it >= a.iters) break;
        int cnt = -1;
        if (it < budget) {
            const float *hp = a.w_hyp + ((size_t)pair * a.iters + it) * S3S_HYP_STRIDE;
            float T[24];
#pragma unroll
            for (int j = 0; j < 24; j++) T[j] = hp[j];
            cnt = resident ? s3s_count<false>(a.c1, a.c2, T, s3s_lds, s3s_lds + cap, s3s_lds + 2 * cap, n, lane, nullptr)
                           : s3s_count<false>(a.c1, a.c2, T, a.w_a + row, a.w_b + row, a.w_c + row, n, lane, nullptr);
        }
        if (lane == 0) { counts[it] = cnt; if (ccounts) ccounts[it] = cnt; }
    }
}

__global__ __launch_bounds__(64) void k_s3s_decide(S3sArgs a)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int n = a.w_n[pair], budget = a.w_budget[pair];
    if (n < 0) return;
    if (budget == 0) {                                                         // N < mRansacMinInliers: bNoMore, nothing estimated
        if (lane == 0 && a.stats) { a.stats[3 * pair] = 0; a.stats[3 * pair + 1] = -1; a.stats[3 * pair + 2] = 0; }
        return;
    }
    const int32_t *counts = a.w_counts + (size_t)pair * a.iters;
    uint32_t first = 0xFFFFFFFFu;
    for (int k = lane; k < budget; k += 64) if (counts[k] > a.min_inliers) first = min(first, (uint32_t)k);
    first = wave_min_u32_dpp(first);
    const bool converged = first != 0xFFFFFFFFu;
    const int end = converged ? (int)first + 1 : budget;
    int key = (int)0x80000000;                                                 // (count, iteration): the largest count, then the LATEST iteration
    for (int k = lane; k < end; k += 64) key = max(key, counts[k] * 1024 + k);
    key = wave_max_dpp(key);
    const int winner = key & 1023, best = key >> 10;
    const float *hp = a.w_hyp + ((size_t)pair * a.iters + winner) * S3S_HYP_STRIDE;
    int nin = 0;
    __shared__ float s_T[24];                                                  // through LDS: 24 wave-uniform loads would sit in (and spill) SGPRs
    if (lane < 24) s_T[lane] = hp[lane];
    __syncthreads();
    if (converged) {
        const size_t row = (size_t)pair * a.max_n;
        float T[24];
#pragma unroll
        for (int j = 0; j < 24; j++) T[j] = s_T[j];
        nin = s3s_count<true>(a.c1, a.c2, T, a.w_a + row, a.w_b + row, a.w_c + row, n, lane, a.inlier + row);
    }
    if (lane < 9) a.R12[(size_t)pair * 9 + lane] = hp[24 + lane];
    if (lane < 3) a.t12[(size_t)pair * 3 + lane] = hp[9 + lane];
    if (lane == 0) {
        a.s12[pair] = hp[33];
        a.converged[pair] = converged ? 1 : 0;
        a.n_inliers[pair] = nin;
        if (a.stats) { a.stats[3 * pair] = budget; a.stats[3 * pair + 1] = winner; a.stats[3 * pair + 2] = best; }
    }
}

}  // namespace

extern "C" void orbhip_sim3solver_default_params(orbhip_sim3solver_params *p)
{
    if (!p) return;
    p->probability = 0.99; p->min_inliers = 6; p->max_iterations = 300; p->fix_scale = 0; p->draw_sets = 1; p->seed = 0;
}

extern "C" int orbhip_sim3_solver_device(orbhip_ctx *ctx, const float *d_X1c, const float *d_X2c, const float *d_max_err1, const float *d_max_err2,
        const int32_t *d_n, int pairs, int max_n, const orbhip_sim3_camera *cam1, const orbhip_sim3_camera *cam2,
        const orbhip_sim3solver_params *p, int32_t *d_sets, uint8_t *d_converged, float *d_R12, float *d_t12, float *d_s12,
        int32_t *d_n_inliers, uint8_t *d_inlier, int32_t *d_stats, int32_t *d_counts)
{
    if (!ctx || !d_X1c || !d_X2c || !d_max_err1 || !d_max_err2 || !d_n || pairs <= 0 || max_n <= 0 || !cam1 || !cam2 || !p || !d_sets ||
        !d_converged || !d_R12 || !d_t12 || !d_s12 || !d_n_inliers || !d_inlier || (cam1->camera_model != 0 && cam1->camera_model != 1) ||
        (cam2->camera_model != 0 && cam2->camera_model != 1)) {
        orbhip_set_last_error_internal("orbhip_sim3_solver_device: bad argument");
        return ORBHIP_E_BADARG;
    }
    if (p->min_inliers < 1) { orbhip_set_last_error_internal("orbhip_sim3_solver_device: min_inliers < 1"); return ORBHIP_E_BADARG; }
    if (p->max_iterations < 1) { orbhip_set_last_error_internal("orbhip_sim3_solver_device: max_iterations < 1"); return ORBHIP_E_BADARG; }
    if (!(p->probability > 0.0 && p->probability < 1.0)) { orbhip_set_last_error_internal("orbhip_sim3_solver_device: probability outside (0, 1)"); return ORBHIP_E_BADARG; }
    if (int rc = ransac_check_capacity(max_n, p->max_iterations, RANSAC_CAPACITY_MSG("orbhip_sim3_solver_device", "correspondences per pair"))) return rc;
    const int device = orbhip_ctx_device_internal(ctx);
    if (hipSetDevice(device) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    const int iters = p->max_iterations;
    const size_t P = (size_t)pairs;
    S3sArgs a;
    memset(&a, 0, sizeof(a));
    size_t bytes = 0;
    for (int pass = 0; pass < 2; pass++) {                                     // the arena's size, then its pointers
        Carve c{pass ? (char *)orbhip_ctx_work_internal(ctx, bytes + 256) : nullptr};
        if (pass && !c.base) return ORBHIP_E_HIP;
        a.w_n = c.take<int32_t>(P); a.w_budget = c.take<int32_t>(P);
        a.w_a = c.take<float4>(P * max_n); a.w_b = c.take<float4>(P * max_n); a.w_c = c.take<float4>(P * max_n);
        a.w_hyp = c.take<float>(P * iters * S3S_HYP_STRIDE); a.w_counts = c.take<int32_t>(P * iters);
        bytes = c.off;
    }
    a.X1c = d_X1c; a.X2c = d_X2c; a.max1 = d_max_err1; a.max2 = d_max_err2; a.n = d_n;
    a.pairs = pairs; a.max_n = max_n; a.iters = iters; a.min_inliers = p->min_inliers; a.fix_scale = p->fix_scale ? 1 : 0;
    a.draw_sets = p->draw_sets ? 1 : 0; a.probability = p->probability; a.seed = p->seed;
    a.c1 = ransac_cam(*cam1); a.c2 = ransac_cam(*cam2);
    a.sets = d_sets; a.converged = d_converged; a.inlier = d_inlier; a.R12 = d_R12; a.t12 = d_t12; a.s12 = d_s12; a.n_inliers = d_n_inliers;
    a.stats = d_stats; a.counts = d_counts; a.status = orbhip_ctx_status_internal(ctx);
    const size_t lds_score = 48 * (size_t)(max_n < S3S_LDS_MAX ? max_n : S3S_LDS_MAX);
    if (orb_lds_optin(reinterpret_cast<const void *>(k_s3s_score), device, lds_score)) return ORBHIP_E_HIP;
    hipStream_t st = orbhip_ctx_stream_internal(ctx);
    hipLaunchKernelGGL(k_s3s_prepare, dim3(pairs), dim3(S3S_THREADS), 0, st, a);
    const long long total = (long long)pairs * iters;
    hipLaunchKernelGGL(k_s3s_hyp, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_s3s_score, dim3(pairs, (iters + S3S_SCORE_ITERS - 1) / S3S_SCORE_ITERS), dim3(S3S_THREADS), lds_score, st, a);
    hipLaunchKernelGGL(k_s3s_decide, dim3(pairs), dim3(64), 0, st, a);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("Sim3Solver launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
