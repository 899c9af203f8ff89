// mlpnp_kernels.hip -- MLPnPsolver (reference include/MLPnPsolver.h, src/MLPnPsolver.cpp:54-1010), batched over relocalisation
// candidates: the step between SearchByBoW and PoseOptimization / SearchByProjection in Tracking::Relocalization (src/Tracking.cc:2644-2760).
// A candidate is one keyframe's matches (world point, undistorted keypoint, sigma2 of its octave); blockIdx.x carries the candidate.
// Four launches per call, every candidate of the batch in each; no workgroup waits on another:
//   k_pnp_prepare   the bearing of every keypoint (GeometricCamera::unproject in float, divided by its z: :77-78), mvMaxError = sigma2 * th2
//                   in float (:250-252), nMin / epsilon / the iteration budget of SetRansacParameters (:229-248) in the reference's types,
//                   the 6-point sets (:126-138) when the caller asks for them (budget and sets from ransac_common.h), reset of the outputs
//   k_pnp_hyp       computePose (:345-651) per (candidate, iteration) on its 6 points, one lane per hypothesis: mlpnp_core.h in double.
//                   The 12x12 (9x9 planar) A^T A and its eigenvectors live in LDS, element k of a lane's matrices at [k][lane] -- as
//                   private arrays indexed by the Jacobi rotation they would be scratch; 2 x 144 doubles per lane, 144 KB a workgroup
//   k_pnp_score     CheckInliers (:255-286) for every hypothesis, one wave per (candidate, iteration), lanes striding the matches:
//                   the camera point as the double sums of :264-266 rounded to float, GeometricCamera::project in float in the
//                   reference's operation order (-ffp-contract=off), `error2 < mvMaxError`, counted by ballot + popcount (ransac_wave_count)
//   k_pnp_decide    one wave per candidate: the scan of iterate() (:113-213) over count[] with Refine() (:288-342) as the reference
//                   writes it -- its N-point solve is discarded there, it scores the current hypothesis again, so the first iteration
//                   with count > nMin returns its own hypothesis --, the winner re-scored with the device function that counted (the
//                   flags carry the counted bits), the outputs
// A candidate's matches are staged in LDS for scoring while they fit: 2 float4 each (Xw max_err | u v bx by), at most PNP_LDS_MAX = 4096
// of them = 128 KB; a longer candidate is read through L2 by the same code.
// A hypothesis with a NaN entry counts 0, and so does a set with an index outside [0, n) or with one index twice (the reference cannot
// draw either): every comparison with NaN is false, nothing traps.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "cam_project_f32.h"
#include "ransac_common.h"
#include "mlpnp_core.h"
#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

#define PNP_THREADS 256
#define PNP_SCORE_ITERS 32        // iterations per k_pnp_score workgroup
#define PNP_LDS_MAX 4096          // matches of a candidate that k_pnp_score keeps in LDS (32 bytes each)
#define PNP_MAT 144               // elements of one 12 x 12 matrix
#define PNP_HYP_LDS (2 * PNP_MAT * 64 * sizeof(double))

struct PnpArgs {
    const float *Xw, *p2d, *sigma2;
    const int32_t *n;
    int cands, max_n, iters, min_inliers, min_set, first_call, resume_at, draw_sets;
    float epsilon, th2;
    double probability;
    unsigned long long seed;
    RansacCam cam;
    // work arena
    int32_t *w_n;                 // [cands] n, -1 for a candidate whose count is out of range
    int32_t *w_nmin;              // [cands] mRansacMinInliers after SetRansacParameters
    int32_t *w_budget;            // [cands] mRansacMaxIts, 0 for n < nMin
    int32_t *w_exec;              // [cands] iterations this call runs: max(budget, first_call) capped at iters, 0 for n < nMin
    float4 *w_pt, *w_ob;          // [cands][max_n] (Xw, max_err), (u, v, bearing x, bearing y); the bearing's z is 1
    double *w_hyp;                // [cands][iters][12] mRi row-major, mti
    int32_t *w_counts;            // [cands][iters]
    // caller arrays
    int32_t *sets;
    uint8_t *outcome, *inlier;
    float *Tcw;
    int32_t *n_inliers, *stats, *counts, *status;
};

// one match of CheckInliers (:260-284) under T = (mRi row-major, mti), both double as the reference keeps them
__device__ __forceinline__ bool pnp_inlier(const RansacCam &c, const double *T, float4 pt, float4 ob)
{
    float P[3], uv[2];
#pragma unroll
    for (int i = 0; i < 3; i++)
        P[i] = (float)(T[3 * i] * (double)pt.x + T[3 * i + 1] * (double)pt.y + T[3 * i + 2] * (double)pt.z + T[9 + i]);
    tri_project(c.type, c.p, P, uv);
    const float dx = ob.x - uv[0], dy = ob.y - uv[1];
    const float e2 = dx * dx + dy * dy;
    return e2 < pt.w;
}

// inliers of T among the candidate's n matches, counted by the whole wave; FLAGS: also written to row[]
template <bool FLAGS>
__device__ __forceinline__ int pnp_count(const RansacCam &c, const double *T, const float4 *pt, const float4 *ob, int n, int lane, uint8_t *row)
{
    bool nan = false;
#pragma unroll
    for (int j = 0; j < 12; j++) nan |= T[j] != T[j];
    return ransac_wave_count<FLAGS>(n, lane, row, [&](int i) { return !nan && pnp_inlier(c, T, pt[i], ob[i]); });
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_prepare(PnpArgs a)
{
    const int cand = blockIdx.x, tid = threadIdx.x;
    const int n = a.n[cand];
    if (n < 0 || n > a.max_n) {                                                // status word; nothing of its rows is written
        if (tid == 0) {
            atomicExch(a.status, ORBHIP_E_CAPACITY);
            a.w_n[cand] = -1; a.w_nmin[cand] = 0; a.w_budget[cand] = 0; a.w_exec[cand] = 0; a.outcome[cand] = 0; a.n_inliers[cand] = 0;
            if (a.stats) { a.stats[4 * cand] = 0; a.stats[4 * cand + 1] = -1; a.stats[4 * cand + 2] = 0; a.stats[4 * cand + 3] = 0; }
        }
        return;
    }
    const size_t row = (size_t)cand * a.max_n;
    for (int i = tid; i < n; i += PNP_THREADS) {
        const float *x = a.Xw + (row + i) * 3, *p = a.p2d + (row + i) * 2;
        float ray[3];
        tri_unproject(a.cam.type, a.cam.p, p[0], p[1], ray);
        a.w_pt[row + i] = make_float4(x[0], x[1], x[2], a.sigma2[row + i] * a.th2);
        a.w_ob[row + i] = make_float4(p[0], p[1], ray[0] / ray[2], ray[1] / ray[2]);
        a.inlier[row + i] = 0;
    }
    // SetRansacParameters (:229-248): int(N * epsilon) is a float product, epsilon a float, pow(epsilon, 3) a double
    int nmin = (int)((float)n * a.epsilon);
    nmin = max(nmin, max(a.min_inliers, a.min_set));
    const int budget = ransac_iteration_budget(n, nmin, fmaxf(a.epsilon, (float)nmin / (float)n), a.probability, a.iters);
    const int exec = budget ? min(a.iters, max(budget, a.first_call)) : 0;
    if (tid == 0) {
        a.w_n[cand] = n; a.w_nmin[cand] = nmin; a.w_budget[cand] = budget; a.w_exec[cand] = exec; a.outcome[cand] = 0; a.n_inliers[cand] = 0;
    }
    if (!a.draw_sets) return;
    // :126-138: per iteration 6 draws without replacement, the drawn slot refilled with the last one
    for (int it = tid; it < a.iters; it += PNP_THREADS) ransac_draw_set<6>(a.seed, cand, it, n, a.sets + ((size_t)cand * a.iters + it) * 6);
}

// correspondence i of a list of indices into a candidate's rows
struct PnpListAcc {
    const float4 *pt, *ob;
    const int32_t *idx;
    __device__ __forceinline__ void operator()(int i, double f[3], double X[3]) const
    {
        const int j = idx[i];
        const float4 p = pt[j], o = ob[j];
        f[0] = (double)o.z; f[1] = (double)o.w; f[2] = 1.0; X[0] = (double)p.x; X[1] = (double)p.y; X[2] = (double)p.z;
    }
};

__global__ __launch_bounds__(64) void k_pnp_hyp(PnpArgs a)
{
    extern __shared__ double pnp_lds[];                                        // A [144][64], V [144][64]
    const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (long long)a.cands * a.iters) return;
    const int cand = (int)(gid / a.iters), it = (int)(gid % a.iters);
    const int n = a.w_n[cand];
    if (it >= a.w_exec[cand]) return;
    const int32_t *set = a.sets + ((size_t)cand * a.iters + it) * 6;
    const size_t row = (size_t)cand * a.max_n;
    double *out = a.w_hyp + ((size_t)cand * a.iters + it) * 12;
    bool ok = true;
    int s[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        s[j] = set[j];
        if (s[j] < 0 || s[j] >= n) ok = false;
#pragma unroll
        for (int k = 0; k < j; k++) if (s[k] == s[j]) ok = false;
    }
    if (!ok) {                                                                 // no hypothesis
        const double nanv = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
        for (int k = 0; k < 12; k++) out[k] = nanv;
        return;
    }
    PnpListAcc acc = {a.w_pt + row, a.w_ob + row, set};
    double T[12];
    mlpnp_compute_pose(acc, 6, pnp_lds + threadIdx.x, pnp_lds + PNP_MAT * 64 + threadIdx.x, 64, T);
#pragma unroll
    for (int k = 0; k < 12; k++) out[k] = T[k];
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_score(PnpArgs a)
{
    extern __shared__ float4 pnp_lds4[];                                       // [2][cap], cap = min(max_n, PNP_LDS_MAX)
    const int cand = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.w_n[cand], exec = a.w_exec[cand];
    const int it0 = blockIdx.y * PNP_SCORE_ITERS;
    if (n < 0) return;
    int32_t *counts = a.w_counts + (size_t)cand * a.iters, *ccounts = a.counts ? a.counts + (size_t)cand * a.iters : nullptr;
    if (it0 >= exec) {                                                         // iterations this call does not run: -1
        for (int k = tid; k < PNP_SCORE_ITERS && it0 + k < a.iters; k += PNP_THREADS) { counts[it0 + k] = -1; if (ccounts) ccounts[it0 + k] = -1; }
        return;
    }
    const size_t row = (size_t)cand * a.max_n;
    const int cap = min(a.max_n, PNP_LDS_MAX);
    const bool resident = n <= cap;
    if (resident) {
        for (int i = tid; i < n; i += PNP_THREADS) { pnp_lds4[i] = a.w_pt[row + i]; pnp_lds4[cap + i] = a.w_ob[row + i]; }
    }
    __syncthreads();
    for (int k = wave; k < PNP_SCORE_ITERS; k += PNP_THREADS / 64) {
        const int it = it0 + k;
        if (it >= a.iters) break;
        int cnt = -1;
        if (it < exec) {
            const double *hp = a.w_hyp + ((size_t)cand * a.iters + it) * 12;
            double T[12];
#pragma unroll
            for (int j = 0; j < 12; j++) T[j] = hp[j];
            cnt = resident ? pnp_count<false>(a.cam, T, pnp_lds4, pnp_lds4 + cap, n, lane, nullptr)
                           : pnp_count<false>(a.cam, T, a.w_pt + row, a.w_ob + row, n, lane, nullptr);
        }
        if (lane == 0) { counts[it] = cnt; if (ccounts) ccounts[it] = cnt; }
    }
}

// iterate()'s loop (:113-213) over count[].  Refine() (:288-342) as the reference writes it: computePose on the best's inliers fills a local
// `result` that is never copied into mRi / mti, so its CheckInliers() scores the CURRENT iteration's hypothesis again and mRefinedTcw is
// that hypothesis.  What decides is therefore count[k] alone: the call returns at the first iteration k >= resume_at with count[k] > nMin,
// with hypothesis k, its flags and its count; the N-point solve changes nothing the caller can see and is not run.
__global__ __launch_bounds__(64) void k_pnp_decide(PnpArgs a)
{
    __shared__ double s_T[12];                                                 // through LDS: 12 wave-uniform loads would sit in SGPRs
    const int cand = blockIdx.x, lane = threadIdx.x;
    const int n = a.w_n[cand], exec = a.w_exec[cand], nmin = a.w_nmin[cand], budget = a.w_budget[cand];
    if (n < 0) return;
    if (exec == 0) {                                                           // N < mRansacMinInliers: bNoMore, nothing estimated
        if (lane == 0 && a.stats) { a.stats[4 * cand] = 0; a.stats[4 * cand + 1] = -1; a.stats[4 * cand + 2] = 0; a.stats[4 * cand + 3] = 0; }
        return;
    }
    const size_t row = (size_t)cand * a.max_n;
    const int32_t *counts = a.w_counts + (size_t)cand * a.iters;
    uint8_t *flags = a.inlier + row;
    int best = 0, bestk = -1, nref = 0, ret = -1;
#pragma unroll 1
    for (int k = 0; k < exec; k++) {                                           // counts[k] is the same in every lane
        const int c = counts[k];
        if (c < nmin) continue;                                                // :167
        if (c > best) { best = c; bestk = k; }                                 // :170-182: a strictly larger count is the new best
        nref++;                                                                // :184: Refine() is called
        if (c > nmin && k >= a.resume_at) { ret = k; break; }                  // :329 on the current hypothesis' count
    }
    const int at = ret >= 0 ? ret : bestk;
    const int outcome = ret >= 0 ? 1 : (bestk >= 0 ? 2 : 0);                   // :186-193 | :199-212 | nothing
    int nin = 0;
    if (outcome) {
        if (lane < 12) s_T[lane] = a.w_hyp[((size_t)cand * a.iters + at) * 12 + lane];
        __syncthreads();
        double T[12];
#pragma unroll
        for (int j = 0; j < 12; j++) T[j] = s_T[j];
        nin = pnp_count<true>(a.cam, T, a.w_pt + row, a.w_ob + row, n, lane, flags);       // the function that counted: the same bits
        if (lane < 12) a.Tcw[(size_t)cand * 12 + lane] = (float)T[lane];
    } else {
        for (int i = lane; i < n; i += 64) flags[i] = 0;
    }
    if (lane == 0) {
        a.outcome[cand] = (uint8_t)outcome;
        a.n_inliers[cand] = nin;
        if (a.stats) { a.stats[4 * cand] = budget; a.stats[4 * cand + 1] = at; a.stats[4 * cand + 2] = at >= 0 ? counts[at] : 0; a.stats[4 * cand + 3] = nref; }
    }
}

}  // namespace

extern "C" void orbhip_mlpnp_default_params(orbhip_mlpnp_params *p)
{
    if (!p) return;
    p->probability = 0.99; p->min_inliers = 8; p->max_iterations = 300; p->min_set = 6; p->epsilon = 0.4f; p->th2 = 5.991f;
    p->first_call_iterations = 0; p->resume_at = 0; p->draw_sets = 1; p->seed = 0;
}

// the parameter and capacity rules of both forms, each failure named; ORBHIP_OK when they hold
extern "C" int orbhip_mlpnp_check_params_internal(const orbhip_mlpnp_params *p, int max_n)
{
    if (p->min_set != 6) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: min_set must be 6"); return ORBHIP_E_BADARG; }
    if (p->min_inliers < 1) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: min_inliers < 1"); return ORBHIP_E_BADARG; }
    if (p->max_iterations < 1) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: max_iterations < 1"); return ORBHIP_E_BADARG; }
    if (!(p->probability > 0.0 && p->probability < 1.0)) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: probability outside (0, 1)"); return ORBHIP_E_BADARG; }
    if (!(p->epsilon > 0.f && p->epsilon <= 1.f)) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: epsilon outside (0, 1]"); return ORBHIP_E_BADARG; }
    if (!(p->th2 > 0.f)) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: th2 <= 0"); return ORBHIP_E_BADARG; }
    if (p->first_call_iterations < 0) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: first_call_iterations < 0"); return ORBHIP_E_BADARG; }
    if (p->resume_at < 0) { orbhip_set_last_error_internal("orbhip_mlpnp_solver: resume_at < 0"); return ORBHIP_E_BADARG; }
    return ransac_check_capacity(max_n, p->max_iterations, RANSAC_CAPACITY_MSG("orbhip_mlpnp_solver", "matches per candidate"));
}

extern "C" int orbhip_mlpnp_solver_device(orbhip_ctx *ctx, const float *d_Xw, const float *d_p2d, const float *d_sigma2, const int32_t *d_n,
        int candidates, int max_n, const orbhip_sim3_camera *cam, const orbhip_mlpnp_params *p, int32_t *d_sets, uint8_t *d_outcome,
        float *d_Tcw, int32_t *d_n_inliers, uint8_t *d_inlier, int32_t *d_stats, int32_t *d_counts)
{
    if (!ctx || !d_Xw || !d_p2d || !d_sigma2 || !d_n || candidates <= 0 || max_n <= 0 || !cam || !p || !d_sets || !d_outcome || !d_Tcw ||
        !d_n_inliers || !d_inlier || (cam->camera_model != 0 && cam->camera_model != 1)) {
        orbhip_set_last_error_internal("orbhip_mlpnp_solver_device: bad argument");
        return ORBHIP_E_BADARG;
    }
    if (int rc = orbhip_mlpnp_check_params_internal(p, max_n)) return rc;
    const int device = orbhip_ctx_device_internal(ctx);
    if (hipSetDevice(device) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    const int iters = p->max_iterations;
    const size_t C = (size_t)candidates;
    PnpArgs a;
    memset(&a, 0, sizeof(a));
    size_t bytes = 0;
    for (int pass = 0; pass < 2; pass++) {                                     // the arena's size, then its pointers
        Carve c{pass ? (char *)orbhip_ctx_work_internal(ctx, bytes + 256) : nullptr};
        if (pass && !c.base) return ORBHIP_E_HIP;
        a.w_n = c.take<int32_t>(C); a.w_nmin = c.take<int32_t>(C); a.w_budget = c.take<int32_t>(C); a.w_exec = c.take<int32_t>(C);
        a.w_pt = c.take<float4>(C * max_n); a.w_ob = c.take<float4>(C * max_n);
        a.w_hyp = c.take<double>(C * iters * 12); a.w_counts = c.take<int32_t>(C * iters);
        bytes = c.off;
    }
    a.Xw = d_Xw; a.p2d = d_p2d; a.sigma2 = d_sigma2; a.n = d_n;
    a.cands = candidates; a.max_n = max_n; a.iters = iters; a.min_inliers = p->min_inliers; a.min_set = p->min_set;
    a.first_call = p->first_call_iterations; a.resume_at = p->resume_at; a.draw_sets = p->draw_sets ? 1 : 0;
    a.epsilon = p->epsilon; a.th2 = p->th2; a.probability = p->probability; a.seed = p->seed;
    a.cam = ransac_cam(*cam);
    a.sets = d_sets; a.outcome = d_outcome; a.inlier = d_inlier; a.Tcw = d_Tcw; a.n_inliers = d_n_inliers;
    a.stats = d_stats; a.counts = d_counts; a.status = orbhip_ctx_status_internal(ctx);
    const size_t lds_score = 32 * (size_t)(max_n < PNP_LDS_MAX ? max_n : PNP_LDS_MAX);
    if (orb_lds_optin(reinterpret_cast<const void *>(k_pnp_score), device, lds_score)) return ORBHIP_E_HIP;
    if (orb_lds_optin(reinterpret_cast<const void *>(k_pnp_hyp), device, PNP_HYP_LDS)) return ORBHIP_E_HIP;
    hipStream_t st = orbhip_ctx_stream_internal(ctx);
    hipLaunchKernelGGL(k_pnp_prepare, dim3(candidates), dim3(PNP_THREADS), 0, st, a);
    const long long total = (long long)candidates * iters;
    hipLaunchKernelGGL(k_pnp_hyp, dim3((unsigned)((total + 63) / 64)), dim3(64), PNP_HYP_LDS, st, a);
    hipLaunchKernelGGL(k_pnp_score, dim3(candidates, (iters + PNP_SCORE_ITERS - 1) / PNP_SCORE_ITERS), dim3(PNP_THREADS), lds_score, st, a);
    hipLaunchKernelGGL(k_pnp_decide, dim3(candidates), dim3(64), 0, st, a);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("MLPnPsolver launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
