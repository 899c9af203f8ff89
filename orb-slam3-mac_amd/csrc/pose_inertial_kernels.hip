// pose_inertial_kernels.hip -- the inertial pose-only optimisations on gfx950: k_pose_inertial and its device-resident C entry point
// (orbhip_pose_inertial_optimization_host, host_entry.hip, packs one frame and calls it).  The cameras, the visual edges and
// EdgeInertial are iba_edges.h's, shared with the inertial BA (iba_kernels.hip).  A module of its own, with cam_pose and visual_jac
// force-inlined: left to the inliner, their form in this kernel depends on what else the module holds, and the kernel was 0.9 % slower
// alone than beside k_iba_solve; force-inlined it is 0.7 % faster than it was there (DESIGN.md 3b has the measurements).
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#define IBA_EDGES_FORCE_INLINE
#include "iba_edges.h"        // + geom3.h, so3_f64.h, imu_layout.h, iba_pack.h (IbaWin, IBA_KF, IBA_PRE)
#include <cmath>
#include <cstring>
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with their models to rounding, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)

// Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:7479-7872, mode 0) and ...LastFrame (:7874-8299, mode 1): the
// current frame's 15 IMU unknowns (+ the previous frame's 15 in mode 1), unary EdgeMonoOnlyPose / EdgeStereoOnlyPose edges, one
// EdgeInertial + EdgeGyroRW + EdgeAccRW (+ EdgePriorPoseImu), g2o Gauss-Newton with a dense LDL^T, 4 rounds x 10 iterations with the
// outlier classification after each, the recovery, the new prior's Hessian, Marginalize and ConstraintPoseImu -- one workgroup per
// frame, the whole schedule in one launch.  The visual edges are strided over the 256 threads; every per-thread sum is reduced in a
// fixed order (DPP inside a wave, then the 4 waves in index order), so that a run is reproducible bit for bit.  The 30 x 30 system,
// the IMU edges and the two 15 x 15 eigen-decompositions live in LDS.  tests/pose_inertial_model.py is the specification.
#define PIM_THREADS 256
#define PIM_WAVES (PIM_THREADS / 64)
#define PIM_PRIOR (ORBHIP_IBA_KF + 225)
struct PimArgs {
    IbaWin W;                                   // the rig (camera fields only)
    const double *Xw, *obs, *is2;               // [F][max_edges][3], [F][max_edges][3], [F][max_edges]
    const uint8_t *kind, *close;                // [F][max_edges]
    const int32_t *n_edges;
    const double *prev, *preint, *info, *info_g, *info_a, *prior;   // [F][21], [F][67], [F][81], [F][9], [F][9], [F][21 + 225]
    double *state; uint8_t *outlier; int32_t *ret; double *H_out; int32_t *stats;
    int frames, max_edges, mode, rec_init;
};
namespace {
struct PimLds {
    IbaWin W;
    double s[IBA_KF], p[IBA_KF], sl[IBA_KF], pl[IBA_KF], cam[24], caml[24], pre[IBA_PRE];
    double om[81 + 9 + 9 + 225];               // block-diagonal information of the IMU-side rows: inertial, gyro RW, acc RW, prior
    double J[30 * 30], OJ[30 * 30], e[30], Oe[30], Ji[216];
    double H[30 * 30], b[30], x[30], A[30 * 30], V[16 * 16], w[16];
    double red[PIM_WAVES * 28];
    double wprior;
    int fail, nbad, ninl;
};

__device__ __forceinline__ void pim_update(double *s, const double *dx)     // ImuCamPose::Update (G2oTypes.cc:192-220) + the "+=" vertices
{
    double t[3], E[9];
    mv3(s + K_R, dx + 3, t);
    for (int i = 0; i < 3; i++) s[K_T + i] += t[i];
    so3_exp(dx, E, 1e-5, true);
    mm3(s + K_R, E, s + K_R);
    for (int i = 0; i < 9; i++) s[K_V + i] += dx[6 + i];
}

// visual pass: robust (0 = raw Omega) normal-equation sums of the edges with use[e] (level 0 / inliers) at the cameras in L.cam
__device__ void pim_visual_sums(PimLds &L, const PimArgs &A, int f, int n, bool robust, double *out27)
{
    const int tid = threadIdx.x;
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0.0;
    const size_t base = (size_t)f * A.max_edges;
    for (int e = tid; e < n; e += PIM_THREADS) {
        if (A.outlier[base + e]) continue;
        const int kind = A.kind[base + e];
        const double *X = A.Xw + 3 * (base + e), *ob = A.obs + 3 * (base + e);
        const double is2 = A.is2[base + e];
        const int ci = kind == 2 ? 1 : 0;
        const CamView V = cam_view(L.W, ci);
        double er[3], Xc[3], Jx[9], Jp[18];
        visual_error(L.W, V, L.cam + 12 * ci, X, ob, kind, er, Xc);
        visual_jac(L.W, V, L.cam + 12 * ci, Xc, kind, Jx, Jp);
        double ww = is2;
        if (robust) {
            const double chi2 = is2 * (er[0] * er[0] + er[1] * er[1] + er[2] * er[2]);
            const double delta = kind == 1 ? (double)sqrtf(7.815f) : (double)sqrtf(5.991f);
            double r0, r1;
            huber(chi2, delta, delta * delta, &r0, &r1);
            ww = r1 * is2;
        }
        if (kind != 1) { er[2] = 0; for (int a = 0; a < 6; a++) Jp[12 + a] = 0; }
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int c = a; c < 6; c++) acc[k++] += ww * (Jp[a] * Jp[c] + Jp[6 + a] * Jp[6 + c] + Jp[12 + a] * Jp[12 + c]);
        }
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] -= ww * (Jp[a] * er[0] + Jp[6 + a] * er[1] + Jp[12 + a] * er[2]);
    }
    const int wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < 27; k++) {
        const double v = wave_sum_f64_dpp(acc[k]);
        if ((tid & 63) == 0) L.red[28 * wv + k] = v;
    }
    __syncthreads();
    if (tid < 27) {
        double v = 0;
        for (int w = 0; w < PIM_WAVES; w++) v += L.red[28 * w + tid];
        out27[tid] = v;
    }
    __syncthreads();
}

// the IMU-side rows (EdgeInertial 9, EdgeGyroRW 3, EdgeAccRW 3, EdgePriorPoseImu 15) at the states in L.s / L.p, and H += J^T W Omega J,
// b -= J^T W Omega e over them; vis27 = the visual sums on the current pose block.  robust: Huber(5) on the prior.
__device__ void pim_system(PimLds &L, const PimArgs &A, int f, int n, const double *vis27, bool robust)
{
    const int tid = threadIdx.x;
    const bool lf = A.mode == 1;
    const int rows = lf ? 30 : 15;
    for (int i = tid; i < rows * n; i += PIM_THREADS) L.J[i] = 0.0;
    __syncthreads();
    if (tid == 0) {
        const double *s1 = lf ? L.p : A.prev + (size_t)f * IBA_KF;
        __builtin_amdgcn_sched_barrier(0);          // keeps the EdgeInertial body's schedule to itself: fewer registers live at its peak
        inertial_edge_body(s1, L.s, L.pre, L.e, L.Ji);
        __builtin_amdgcn_sched_barrier(0);
        for (int i = 0; i < 3; i++) {
            L.e[9 + i] = L.s[K_BG + i] - s1[K_BG + i]; L.J[n * (9 + i) + 9 + i] = 1.0;
            L.e[12 + i] = L.s[K_BA + i] - s1[K_BA + i]; L.J[n * (12 + i) + 12 + i] = 1.0;
            if (lf) { L.J[n * (9 + i) + 24 + i] = -1.0; L.J[n * (12 + i) + 27 + i] = -1.0; }
        }
        if (lf) {                                           // EdgePriorPoseImu (G2oTypes.cc:940-969)
            const double *pr = A.prior + (size_t)f * PIM_PRIOR;
            double RR[9], er[3], IJ[9];
            mtm3(pr + K_R, L.p + K_R, RR);
            so3_log(RR, er);
            double d[3] = {L.p[K_T] - pr[K_T], L.p[K_T + 1] - pr[K_T + 1], L.p[K_T + 2] - pr[K_T + 2]}, et[3];
            mtv3(pr + K_R, d, et);
            so3_inv_right_jac(er, IJ);
            for (int i = 0; i < 3; i++) {
                L.e[15 + i] = er[i]; L.e[18 + i] = et[i];
                for (int j = 0; j < 3; j++) { L.J[n * (15 + i) + 15 + j] = IJ[3 * i + j]; L.J[n * (18 + i) + 18 + j] = RR[3 * i + j]; }
            }
            for (int i = 0; i < 9; i++) { L.e[21 + i] = L.p[K_V + i] - pr[K_V + i]; L.J[n * (21 + i) + 21 + i] = 1.0; }
        }
    }
    __syncthreads();
    for (int i = tid; i < 9 * 24; i += PIM_THREADS) {       // EdgeInertial columns: pose1 v1 bg1 ba1 (previous) | pose2 v2 (current)
        const int r = i / 24, c = i % 24;
        const int col = c >= 15 ? c - 15 : (lf ? c + 15 : -1);
        if (col >= 0) L.J[n * r + col] = L.Ji[i];
    }
    __syncthreads();
    // Omega e (unweighted), then the prior's Huber weight
    for (int r = tid; r < rows; r += PIM_THREADS) {
        int r0, k; const double *Om;
        if (r < 9) { r0 = 0; k = 9; Om = L.om; } else if (r < 12) { r0 = 9; k = 3; Om = L.om + 81; }
        else if (r < 15) { r0 = 12; k = 3; Om = L.om + 90; } else { r0 = 15; k = 15; Om = L.om + 99; }
        double v = 0;
        for (int j = 0; j < k; j++) v += Om[k * (r - r0) + j] * L.e[r0 + j];
        L.Oe[r] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double w = 1.0;
        if (lf && robust) {
            double chi2 = 0, r0, r1;
            for (int i = 0; i < 15; i++) chi2 += L.e[15 + i] * L.Oe[15 + i];
            huber(chi2, 5.0, 25.0, &r0, &r1);
            w = r1;
        }
        L.wprior = w;
    }
    __syncthreads();
    const double wp = L.wprior;
    for (int i = tid; i < rows * n; i += PIM_THREADS) {
        const int r = i / n, c = i % n;
        int r0, k; const double *Om; double w = 1.0;
        if (r < 9) { r0 = 0; k = 9; Om = L.om; } else if (r < 12) { r0 = 9; k = 3; Om = L.om + 81; }
        else if (r < 15) { r0 = 12; k = 3; Om = L.om + 90; } else { r0 = 15; k = 15; Om = L.om + 99; w = wp; }
        double v = 0;
        for (int j = 0; j < k; j++) v += Om[k * (r - r0) + j] * L.J[n * (r0 + j) + c];
        L.OJ[i] = w * v;
    }
    __syncthreads();
    for (int i = tid; i < n * n; i += PIM_THREADS) {
        const int a = i / n, c = i % n;
        if (c < a) continue;
        double v = 0;
        for (int r = 0; r < rows; r++) v += L.J[n * r + a] * L.OJ[n * r + c];
        if (c < 6) v += vis27[a * 6 - a * (a - 1) / 2 + (c - a)];
        L.H[n * a + c] = v; L.H[n * c + a] = v;
    }
    for (int a = tid; a < n; a += PIM_THREADS) {
        double v = 0;
        for (int r = 0; r < rows; r++) v -= L.J[n * r + a] * (r >= 15 ? wp : 1.0) * L.Oe[r];
        if (a < 6) v += vis27[21 + a];
        L.b[a] = v;
    }
    __syncthreads();
}

// dense LDL^T (no pivoting) of L.H into L.A and the solve into x (wave 0); returns false when a pivot is <= 0 or not finite
__device__ bool pim_ldlt(PimLds &L, int n, double *x)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < n * n; i += PIM_THREADS) L.A[i] = L.H[i];
    __syncthreads();
    for (int k = 0; k < n; k++) {
        const double d = L.A[n * k + k];
        if (!(d > 0.0) || !isfinite(d)) { __syncthreads(); return false; }
        const int m = n - k - 1;
        for (int idx = tid; idx < m * m; idx += PIM_THREADS) {
            const int i = k + 1 + idx / m, j = k + 1 + idx % m;
            if (j <= i) L.A[n * i + j] -= L.A[n * i + k] * L.A[n * j + k] / d;
        }
        __syncthreads();
    }
    if (tid < 64) {
        const int i = tid;
        double y = i < n ? L.b[i] : 0.0;
        for (int k = 0; k < n; k++) {                         // L y = b
            const double yk = __shfl(y, k);
            if (i > k && i < n) y -= L.A[n * i + k] / L.A[n * k + k] * yk;
        }
        double z = i < n ? y / L.A[n * i + i] : 0.0;
        for (int k = n - 1; k >= 0; k--) {                    // L^T x = D^-1 y
            const double zk = __shfl(z, k);
            if (i < k) z -= L.A[n * k + i] / L.A[n * i + i] * zk;
        }
        if (i < n) x[i] = z;
    }
    __syncthreads();
    return true;
}

// cyclic Jacobi eigen-decomposition of the symmetric 15 x 15 in L.V's companion L.A (stride 16, lower triangle read): eigenvalues in
// L.w, eigenvectors the columns of L.V
__device__ void pim_eig15(PimLds &L)
{
    const int tid = threadIdx.x, N = 15;
    if (tid < N * N) {
        const int i = tid / N, j = tid % N;
        if (j > i) L.A[16 * i + j] = L.A[16 * j + i];
        L.V[16 * i + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int sweep = 0; sweep < 16; sweep++) {
        double off = 0, dia = 0;
        for (int i = 0; i < N; i++) {
            dia += L.A[17 * i] * L.A[17 * i];
            for (int j = i + 1; j < N; j++) off += L.A[16 * i + j] * L.A[16 * i + j];
        }
        if (off <= 1e-30 * dia || off == 0.0) break;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const double apq = L.A[16 * p + q], app = L.A[17 * p], aqq = L.A[17 * q];
                double akp = 0, akq = 0, vkp = 0, vkq = 0;
                if (tid < N) { akp = L.A[16 * tid + p]; akq = L.A[16 * tid + q]; vkp = L.V[16 * tid + p]; vkq = L.V[16 * tid + q]; }
                __syncthreads();
                if (apq != 0.0) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                    if (tid < N) {
                        if (tid != p && tid != q) {
                            const double np = c * akp - s * akq, nq = s * akp + c * akq;
                            L.A[16 * tid + p] = np; L.A[16 * p + tid] = np; L.A[16 * tid + q] = nq; L.A[16 * q + tid] = nq;
                        }
                        L.V[16 * tid + p] = c * vkp - s * vkq; L.V[16 * tid + q] = s * vkp + c * vkq;
                    }
                    if (tid == 0) { L.A[17 * p] = app - t * apq; L.A[17 * q] = aqq + t * apq; L.A[16 * p + q] = 0.0; L.A[16 * q + p] = 0.0; }
                }
                __syncthreads();
            }
    }
    if (tid < N) L.w[tid] = L.A[17 * tid];
    __syncthreads();
}

// visual chi2 of edge ge at the cameras `cams` (computeError)
__device__ __forceinline__ double pim_chi2(const PimLds &L, const PimArgs &A, size_t ge, const double *cams)
{
    const int kind = A.kind[ge], ci = kind == 2 ? 1 : 0;
    const CamView V = cam_view(L.W, ci);
    double er[3], Xc[3];
    visual_error(L.W, V, cams + 12 * ci, A.Xw + 3 * ge, A.obs + 3 * ge, kind, er, Xc);
    return A.is2[ge] * (er[0] * er[0] + er[1] * er[1] + er[2] * er[2]);
}
}  // namespace

__global__ __launch_bounds__(PIM_THREADS) void k_pose_inertial(PimArgs A)
{
    __shared__ PimLds L;
    const int f = blockIdx.x, tid = threadIdx.x;
    const bool lf = A.mode == 1;
    const int nx = lf ? 30 : 15;
    const size_t base = (size_t)f * A.max_edges;
    const int n = min(max(A.n_edges[f], 0), A.max_edges);
    if (tid == 0) L.W = A.W;
    if (tid < 24) { L.cam[tid] = 0.0; L.caml[tid] = 0.0; }     // camera 1 stays zero without a second camera
    if (tid < IBA_KF) {
        L.s[tid] = A.state[(size_t)f * IBA_KF + tid];
        L.p[tid] = lf ? A.prev[(size_t)f * IBA_KF + tid] : 0.0;
    }
    if (tid < IBA_PRE) L.pre[tid] = A.preint[(size_t)f * IBA_PRE + tid];
    if (tid < 81) L.om[tid] = A.info[(size_t)f * 81 + tid];
    if (tid < 9) { L.om[81 + tid] = A.info_g[(size_t)f * 9 + tid]; L.om[90 + tid] = A.info_a[(size_t)f * 9 + tid]; }
    if (lf && tid < 225) L.om[99 + tid] = A.prior[(size_t)f * PIM_PRIOR + IBA_KF + tid];
    if (tid < 30) L.x[tid] = 0.0;
    for (int e = tid; e < n; e += PIM_THREADS) A.outlier[base + e] = 0;
    __syncthreads();
    __shared__ double vis[27];
    int rounds = 0, iters = 0, fails = 0, nbad = 0, ninl = 0;
    bool robust = true;
    for (int it = 0; it < 4; it++) {
        rounds++;
        for (int k = 0; k < 10; k++) {
            if (tid < IBA_KF) { L.sl[tid] = L.s[tid]; L.pl[tid] = L.p[tid]; }
            if (tid == 0) cam_pose(L.W, L.s, L.cam);
            __syncthreads();
            pim_visual_sums(L, A, f, n, robust, vis);
            pim_system(L, A, f, nx, vis, true);
            const bool ok = pim_ldlt(L, nx, L.Oe);       // the step lands in L.Oe (free after pim_system)
            iters++;
            if (!ok) fails++;
            if (tid == 0) {
                if (ok) for (int i = 0; i < nx; i++) L.x[i] = L.Oe[i];
                pim_update(L.s, L.x);
                if (lf) pim_update(L.p, L.x + 15);
            }
            __syncthreads();
            if (!ok) break;
        }
        // classification (:7720-7790 / :8129-8198): active edges keep the chi2 of the last computeActiveErrors (L.sl)
        if (tid == 0) { cam_pose(L.W, L.s, L.cam); cam_pose(L.W, L.sl, L.caml); L.nbad = 0; }
        __syncthreads();
        const float gm = (lf || it >= 2) ? 5.991f : (it == 0 ? 12.f : 7.5f), gclose = (float)(1.5 * (double)gm);
        const float gs = it == 0 ? 15.6f : (it == 1 ? 9.8f : 7.815f);
        int bad = 0;
        for (int e = tid; e < n; e += PIM_THREADS) {
            const size_t ge = base + e;
            const bool was_out = A.outlier[ge] != 0;
            const float chi2 = (float)pim_chi2(L, A, ge, was_out ? L.cam : L.caml);
            const double *c = L.cam + (A.kind[ge] == 2 ? 12 : 0), *X = A.Xw + 3 * ge;
            const double depth = c[6] * X[0] + c[7] * X[1] + c[8] * X[2] + c[11];          // isDepthPositive at the current estimate
            bool out;
            if (A.kind[ge] == 1) out = chi2 > gs;
            else {
                const bool close = A.close && A.close[ge];
                out = (chi2 > gm && !close) || (close && chi2 > gclose) || !(depth > 0.0);
            }
            A.outlier[ge] = out ? 1 : 0;
            bad += out ? 1 : 0;
        }
        if (bad) atomicAdd(&L.nbad, bad);
        __syncthreads();
        nbad = L.nbad; ninl = n - nbad;
        if (it == 2) robust = false;
        __syncthreads();
        if (n + (lf ? 4 : 3) < 10) break;
    }
    if (ninl < 30 && !A.rec_init) {                      // recovery (:7795-7822 / :8202-8230)
        if (tid == 0) L.nbad = 0;
        __syncthreads();
        int bad = 0;
        for (int e = tid; e < n; e += PIM_THREADS) {
            const size_t ge = base + e;
            const double chi2 = pim_chi2(L, A, ge, L.cam);
            if (chi2 < (A.kind[ge] == 1 ? 24.0 : 18.0)) A.outlier[ge] = 0;
            else bad++;
        }
        if (bad) atomicAdd(&L.nbad, bad);
        __syncthreads();
        nbad = L.nbad;
    }
    // the new prior (:7831-7869 / :8242-8296): raw information, inlier visual edges, the final estimate
    pim_visual_sums(L, A, f, n, false, vis);
    pim_system(L, A, f, nx, vis, false);
    if (lf) {                                            // Marginalize(H, 0, 14): the previous frame's block (15..29 here)
        if (tid < 225) { const int i = tid / 15, j = tid % 15; L.A[16 * i + j] = L.H[30 * (15 + i) + 15 + j]; }
        __syncthreads();
        pim_eig15(L);
        if (tid < 225) {                                 // pinv: sum v v^T / lambda over |lambda| > 1e-6 (JacobiSVD of a symmetric block)
            const int i = tid / 15, j = tid % 15;
            double v = 0;
            for (int k = 0; k < 15; k++) if (fabs(L.w[k]) > 1e-6) v += L.V[16 * i + k] * L.V[16 * j + k] / L.w[k];
            L.J[15 * i + j] = v;
        }
        __syncthreads();
        if (tid < 225) {                                 // M = H_cb pinv
            const int i = tid / 15, j = tid % 15;
            double v = 0;
            for (int k = 0; k < 15; k++) v += L.H[30 * i + 15 + k] * L.J[15 * k + j];
            L.OJ[15 * i + j] = v;
        }
        __syncthreads();
        if (tid < 225) {
            const int i = tid / 15, j = tid % 15;
            double v = 0;
            for (int k = 0; k < 15; k++) v += L.OJ[15 * i + k] * L.H[30 * (15 + k) + j];
            L.A[16 * i + j] = L.H[30 * i + j] - v;
        }
        __syncthreads();
    } else {
        if (tid < 225) { const int i = tid / 15, j = tid % 15; L.A[16 * i + j] = L.H[15 * i + j]; }
        __syncthreads();
    }
    // ConstraintPoseImu (include/G2oTypes.h:708-719): H = (H + H) / 2, eigenvalues < 1e-12 -> 0, reassembled
    if (tid < 225) { const int i = tid / 15, j = tid % 15; L.A[16 * i + j] = (L.A[16 * i + j] + L.A[16 * i + j]) / 2; }
    __syncthreads();
    pim_eig15(L);
    if (tid < 225) {
        const int i = tid / 15, j = tid % 15;
        double v = 0;
        for (int k = 0; k < 15; k++) { const double w = L.w[k] < 1e-12 ? 0.0 : L.w[k]; v += L.V[16 * i + k] * w * L.V[16 * j + k]; }
        A.H_out[(size_t)f * 225 + tid] = v;
    }
    if (tid < IBA_KF) A.state[(size_t)f * IBA_KF + tid] = L.s[tid];
    if (tid == 0) {
        A.ret[f] = n - nbad;
        if (A.stats) { int32_t *st = A.stats + 4 * (size_t)f; st[0] = rounds; st[1] = iters; st[2] = fails; st[3] = nbad; }
    }
}

extern "C" int orbhip_pose_inertial_optimization_device(orbhip_ctx *ctx, int mode, int rec_init, const orbhip_pim_rig *rig, int frames,
        int max_edges, const double *d_Xw, const double *d_obs, const double *d_inv_sigma2, const uint8_t *d_kind, const uint8_t *d_close,
        const int32_t *d_n_edges, const double *d_prev, const double *d_preint, const double *d_info, const double *d_info_g,
        const double *d_info_a, const double *d_prior, double *d_state, uint8_t *d_outlier, int32_t *d_ret, double *d_H_out,
        int32_t *d_stats)
{
    if (!ctx || !rig || (mode != 0 && mode != 1) || frames < 0 || max_edges < 0 || (rig->camera_model != 0 && rig->camera_model != 1) ||
        (rig->has_cam2 && rig->camera2_model != 0 && rig->camera2_model != 1))
        return ORBHIP_E_BADARG;
    if (frames == 0) return ORBHIP_OK;
    if ((max_edges && (!d_Xw || !d_obs || !d_inv_sigma2 || !d_kind || !d_outlier)) || !d_n_edges || !d_prev || !d_preint || !d_info ||
        !d_info_g || !d_info_a || (mode == 1 && !d_prior) || !d_state || !d_ret || !d_H_out)
        return ORBHIP_E_BADARG;
    PimArgs a;
    memset(&a, 0, sizeof(a));
    IbaWin &W = a.W;
    for (int i = 0; i < 9; i++) W.Rcb[i] = rig->Rcb[i];
    for (int i = 0; i < 3; i++) W.tcb[i] = rig->tcb[i];
    W.fx = rig->fx; W.fy = rig->fy; W.cx = rig->cx; W.cy = rig->cy; W.bf = rig->bf; W.cam_model = rig->camera_model;
    for (int i = 0; i < 4; i++) { W.kb[i] = rig->kb[i]; W.kb2[i] = rig->kb2[i]; }
    W.has_cam2 = rig->has_cam2 ? 1 : 0;
    if (W.has_cam2) {                                    // Rcb[1] = Rrl Rcb[0], tcb[1] = Rrl tcb[0] + trl (G2oTypes.cc:57-67)
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) W.Rcb2[3 * r + c] = rig->Trl[4 * r] * rig->Rcb[c] + rig->Trl[4 * r + 1] * rig->Rcb[3 + c] + rig->Trl[4 * r + 2] * rig->Rcb[6 + c];
            W.tcb2[r] = rig->Trl[4 * r] * rig->tcb[0] + rig->Trl[4 * r + 1] * rig->tcb[1] + rig->Trl[4 * r + 2] * rig->tcb[2] + rig->Trl[4 * r + 3];
        }
        W.fx2 = rig->fx2; W.fy2 = rig->fy2; W.cx2 = rig->cx2; W.cy2 = rig->cy2; W.cam2_model = rig->camera2_model;
    }
    a.Xw = d_Xw; a.obs = d_obs; a.is2 = d_inv_sigma2; a.kind = d_kind; a.close = d_close; a.n_edges = d_n_edges;
    a.prev = d_prev; a.preint = d_preint; a.info = d_info; a.info_g = d_info_g; a.info_a = d_info_a; a.prior = d_prior;
    a.state = d_state; a.outlier = d_outlier; a.ret = d_ret; a.H_out = d_H_out; a.stats = d_stats;
    a.frames = frames; a.max_edges = max_edges; a.mode = mode; a.rec_init = rec_init ? 1 : 0;
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    hipLaunchKernelGGL(k_pose_inertial, dim3(frames), dim3(PIM_THREADS), 0, orbhip_ctx_stream_internal(ctx), a);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("k_pose_inertial launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
