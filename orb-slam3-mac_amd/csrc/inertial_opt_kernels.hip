// inertial_opt_kernels.hip -- Optimizer::InertialOptimization (src/Optimizer.cc:5303-5908, all four overloads) on the device: the
// inertial-only solve for gravity direction, scale, one gyro / accelerometer bias and the keyframe velocities that LocalMapping::
// InitializeIMU, ScaleRefinement and the inertial map merge call.  ONE workgroup solves ONE map from start to end (no team grid, no
// device-wide barrier, no cooperative launch); a batch is `maps` independent workgroups.  All FP64.
//
// Graph: one EdgeInertialGS (src/G2oTypes.cc:802-927) per keyframe with a link to its predecessor, EdgePriorAcc / EdgePriorGyro on the
// biases, g2o's Levenberg-Marquardt (the fork's: tau 1e-50, 100 trials, Raul's three-bad-iterations stop) or Gauss-Newton.
// System: an arrowhead -- a block-tridiagonal chain of 3x3 velocity blocks and a dense border of up to 9 columns (gyro bias 3,
// accelerometer bias 3, gravity direction 2, scale 1).  It is solved as one: block elimination along the chain (one wave; lane c
// carries border column c, lane 9 the right-hand side), the border's Schur complement (<= 9x9, LDL^T without pivoting), back
// substitution.  A fixed unknown is absent from the system.  A block pivot that is not positive (or not finite) is "solver failed".
// Every sum (chi2, the border blocks, LM's scale term) has a fixed order: two runs of the same inputs agree byte for byte.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "geom3.h"
#include "so3_f64.h"
#include "imu_layout.h"        // K_* state and P_* preintegration offsets, IMU_GRAVITY
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#pragma clang fp contract(fast)

#define IO_THREADS 256
#define IO_KF ORBHIP_IBA_KF
#define IO_PRE ORBHIP_IBA_PREINT
#define IO_MAX_KF 4096
// chain record of a keyframe, in doubles: D[6] (symmetric 3x3: 00 01 02 11 12 22; after the sweep the eliminated block), O[9] (the block
// to the predecessor, rows = predecessor; after the sweep G = D~(k-1)^-1 O), B[27] ([3][9] border rows; after the sweep D~^-1 B~), r[3]
// (likewise), r0[3] (the pristine right-hand side), x[3] (the step), v[3] (the velocity estimate), vt[3] (the trial's)
#define IO_CH 57
enum { C_D = 0, C_O = 6, C_B = 15, C_R = 42, C_R0 = 45, C_X = 48, C_V = 51, C_VT = 54 };
// per-edge border contributions in the call's workspace: C[45] (symmetric 9x9), rhs[9], chi2
#define IO_WS 56
// global state of a map: Rwg[9], scale, bg[3], ba[3]
enum { G_R = 0, G_S = 9, G_BG = 10, G_BA = 13 };

namespace {

struct IoArgs {
    const int32_t *kf_off; double *kf; const uint8_t *link; const double *preint; const double *info;
    double *global; double *stats; double *trace; double *ws_edge; double *ws_chain;
    int fvb, fgd, fsc, gn, iterations, max_trials, lds_kf, prof;
    double lambda_init, prior_g, prior_a;
};

__host__ __device__ constexpr int sym3(int a, int b) { return a * 3 - a * (a - 1) / 2 + (b - a); }
__host__ __device__ constexpr int sym9(int a, int b) { return a * 9 - a * (a - 1) / 2 + (b - a); }

// sum over the workgroup in a fixed association; the result is uniform
__device__ __forceinline__ double io_block_sum(double v, double *red)
{
    const double w = wave_sum_f64_dpp(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// EdgeInertialGS::computeError at (kf1, v1) -> (kf2, v2) with the map's state gs; the pieces linearizeOplus needs come back too
struct IoGeom { double e[9], Rbw1[9], eR[9], w[3], dvel[3], dpos[3]; };
__device__ __forceinline__ void io_edge_error(const double *kf1, const double *kf2, const double *v1, const double *v2, const double *pi,
                                              const double *gs, IoGeom &Q)
{
    const double dt = pi[P_DT], s = gs[G_S];
    double dbg[3], dba[3], E[9], dR[9], dV[3], dP[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { dbg[i] = gs[G_BG + i] - pi[P_BG + i]; dba[i] = gs[G_BA + i] - pi[P_BA + i]; }
    mv3(pi + P_JRG, dbg, Q.w);
    so3_exp(Q.w, E, 1e-4, false);                        // Preintegrated::GetDeltaRotation (ImuTypes.cc:357-363)
    mm3(pi + P_DR, E, dR);
    so3_normalize(dR);
    mv3(pi + P_JVG, dbg, dV); mv3(pi + P_JVA, dba, t);
#pragma unroll
    for (int i = 0; i < 3; i++) dV[i] = pi[P_DV + i] + dV[i] + t[i];
    mv3(pi + P_JPG, dbg, dP); mv3(pi + P_JPA, dba, t);
#pragma unroll
    for (int i = 0; i < 3; i++) dP[i] = pi[P_DP + i] + dP[i] + t[i];
    double R12[9], er[3], a[3], b[3], va[3], vb[3];
    mtm3(kf1 + K_R, kf2 + K_R, R12);
    mtm3(dR, R12, Q.eR);
    so3_log(Q.eR, er);
    const double g[3] = {-IMU_GRAVITY * gs[G_R + 2], -IMU_GRAVITY * gs[G_R + 5], -IMU_GRAVITY * gs[G_R + 8]};     // Rwg (0, 0, -G)
#pragma unroll
    for (int i = 0; i < 3; i++) {
        Q.dvel[i] = v2[i] - v1[i];
        Q.dpos[i] = kf2[K_T + i] - kf1[K_T + i] - v1[i] * dt;
        a[i] = s * Q.dvel[i] - g[i] * dt;
        b[i] = s * Q.dpos[i] - g[i] * dt * dt / 2;
    }
    mtv3(kf1 + K_R, a, va); mtv3(kf1 + K_R, b, vb);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        Q.e[i] = er[i]; Q.e[3 + i] = va[i] - dV[i]; Q.e[6 + i] = vb[i] - dP[i];
#pragma unroll
        for (int j = 0; j < 3; j++) Q.Rbw1[3 * i + j] = kf1[K_R + 3 * j + i];
    }
}

// the information, read as its upper triangle (the reference's is symmetric to rounding: (Info + Info^T) / 2, then an eigen clean-up)
__device__ __forceinline__ void io_load_info(const double *info, double *om)
{
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = i; j < 9; j++) om[sym9(i, j)] = info[9 * i + j];
}
__device__ __forceinline__ double io_weigh(const double *om, const double *e, double *oe)
{
    double chi = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        double acc = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) acc += om[i <= j ? sym9(i, j) : sym9(j, i)] * e[j];
        oe[i] = acc;
        chi += e[i] * acc;
    }
    return chi;
}

// chi2 of one edge
__device__ __forceinline__ double io_edge_chi(const double *kf1, const double *kf2, const double *v1, const double *v2, const double *pi,
                                              const double *info, const double *gs)
{
    IoGeom Q;
    io_edge_error(kf1, kf2, v1, v2, pi, gs, Q);
    double om[45], oe[9];
    io_load_info(info, om);
    return io_weigh(om, Q.e, oe);
}

// One edge into the normal equations.  Columns: v1 0:3, v2 3:6, gyro bias 6:9, accelerometer bias 9:12, gravity direction 12:14, scale 14;
// rows 0:3 (rotation) are non-zero in the gyro-bias columns only (T), rows 3:9 are J6.  R = the chain record of keyframe 2, P1 = of
// keyframe 1, Ew = the edge's border row in the workspace.  FVB: velocities and biases are free.
template <bool FVB>
__device__ __forceinline__ void io_edge_build(const double *kf1, const double *kf2, const double *v1, const double *v2, const double *pi,
                                              const double *info, const double *gs, bool fgd, bool fsc, double *R, double *P1, double *Ew)
{
    IoGeom Q;
    io_edge_error(kf1, kf2, v1, v2, pi, gs, Q);
    const double dt = pi[P_DT], s = gs[G_S];
    double J6[6 * 15], T[9];
#pragma unroll
    for (int i = 0; i < 90; i++) J6[i] = 0.0;
    if (FVB) {
        double er[3] = {Q.e[0], Q.e[1], Q.e[2]}, invJr[9], RJ[9], eRt[9], M[9];
        so3_inv_right_jac(er, invJr);
        so3_right_jac(Q.w, RJ);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) eRt[3 * i + j] = Q.eR[3 * j + i];
        mm3(invJr, eRt, M); mm3(M, RJ, M); mm3(M, pi + P_JRG, M);
#pragma unroll
        for (int i = 0; i < 9; i++) T[i] = -M[i];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                J6[i * 15 + j] = -s * Q.Rbw1[3 * i + j];                  // velocity rows, v1
                J6[(3 + i) * 15 + j] = -s * Q.Rbw1[3 * i + j] * dt;       // position rows, v1
                J6[i * 15 + 3 + j] = s * Q.Rbw1[3 * i + j];               // velocity rows, v2
                J6[i * 15 + 6 + j] = -pi[P_JVG + 3 * i + j];
                J6[(3 + i) * 15 + 6 + j] = -pi[P_JPG + 3 * i + j];
                J6[i * 15 + 9 + j] = -pi[P_JVA + 3 * i + j];
                J6[(3 + i) * 15 + 9 + j] = -pi[P_JPA + 3 * i + j];
            }
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) T[i] = 0.0;
    }
    if (fgd) {                                               // dGdTheta = Rwg Gm, Gm = [0 -G; G 0; 0 0]
        double c0[3] = {IMU_GRAVITY * gs[G_R + 1], IMU_GRAVITY * gs[G_R + 4], IMU_GRAVITY * gs[G_R + 7]};
        double c1[3] = {-IMU_GRAVITY * gs[G_R + 0], -IMU_GRAVITY * gs[G_R + 3], -IMU_GRAVITY * gs[G_R + 6]};
        double a0[3], a1[3];
        mv3(Q.Rbw1, c0, a0); mv3(Q.Rbw1, c1, a1);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            J6[i * 15 + 12] = -a0[i] * dt; J6[i * 15 + 13] = -a1[i] * dt;
            J6[(3 + i) * 15 + 12] = -0.5 * a0[i] * dt * dt; J6[(3 + i) * 15 + 13] = -0.5 * a1[i] * dt * dt;
        }
    }
    if (fsc) {
        double a0[3], a1[3];
        mv3(Q.Rbw1, Q.dvel, a0); mv3(Q.Rbw1, Q.dpos, a1);
#pragma unroll
        for (int i = 0; i < 3; i++) { J6[i * 15 + 14] = a0[i]; J6[(3 + i) * 15 + 14] = a1[i]; }
    }
    double om[45], oe[9];
    io_load_info(info, om);
    Ew[54] = io_weigh(om, Q.e, oe);
    if (!FVB) {
#pragma unroll
        for (int i = 0; i < 54; i++) Ew[i] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < 15; c++) {
        if (!FVB && c < 12) continue;
        const bool cg = FVB && c >= 6 && c < 9;              // a gyro-bias column: rotation rows too
        double t[9];
#pragma unroll
        for (int i = 0; i < 9; i++) {
            double acc = 0;
#pragma unroll
            for (int j = 3; j < 9; j++) acc += om[i <= j ? sym9(i, j) : sym9(j, i)] * J6[(j - 3) * 15 + c];
            if (cg) {
#pragma unroll
                for (int j = 0; j < 3; j++) acc += om[i <= j ? sym9(i, j) : sym9(j, i)] * T[3 * j + (c - 6)];
            }
            t[i] = acc;
        }
        double gc = 0;
#pragma unroll
        for (int j = 3; j < 9; j++) gc += J6[(j - 3) * 15 + c] * oe[j];
        if (cg) {
#pragma unroll
            for (int j = 0; j < 3; j++) gc += T[3 * j + (c - 6)] * oe[j];
        }
        if (c < 3) P1[C_R + c] -= gc;
        else if (c < 6) R[C_R + c - 3] -= gc;
        else Ew[45 + c - 6] = -gc;
#pragma unroll
        for (int cp = 0; cp <= c; cp++) {
            if (!FVB && cp < 12) continue;
            double h = 0;
#pragma unroll
            for (int j = 3; j < 9; j++) h += J6[(j - 3) * 15 + cp] * t[j];
            if (FVB && cp >= 6 && cp < 9) {
#pragma unroll
                for (int j = 0; j < 3; j++) h += T[3 * j + (cp - 6)] * t[j];
            }
            if (c < 3) P1[C_D + sym3(cp, c)] += h;
            else if (c < 6) { if (cp < 3) R[C_O + 3 * cp + c - 3] = h; else R[C_D + sym3(cp - 3, c - 3)] += h; }
            else if (cp < 3) P1[C_B + cp * 9 + c - 6] += h;
            else if (cp < 6) R[C_B + (cp - 3) * 9 + c - 6] += h;
            else Ew[sym9(cp - 6, c - 6)] = h;
        }
    }
}

struct IoMap {
    int n; const double *kf; const uint8_t *link; const double *preint, *info;
    double *ch, *ws; bool fvb, fgd, fsc; double prior_g, prior_a;
};

// chi2 of the map at the state gs with the velocities at record offset voff
__device__ __forceinline__ double io_chi2(const IoMap &M, int voff, const double *gs, double *red)
{
    double acc = 0;
    for (int k = 1 + threadIdx.x; k < M.n; k += IO_THREADS)
        if (M.link[k])
            acc += io_edge_chi(M.kf + (size_t)(k - 1) * IO_KF, M.kf + (size_t)k * IO_KF, M.ch + (size_t)(k - 1) * IO_CH + voff,
                               M.ch + (size_t)k * IO_CH + voff, M.preint + (size_t)k * IO_PRE, M.info + (size_t)k * 81, gs);
    double chi = io_block_sum(acc, red);
    if (!M.fvb) return chi;                                  // fixed biases: the prior edges have only fixed vertices and are not active in g2o
    chi += M.prior_g * (gs[G_BG] * gs[G_BG] + gs[G_BG + 1] * gs[G_BG + 1] + gs[G_BG + 2] * gs[G_BG + 2]);
    chi += M.prior_a * (gs[G_BA] * gs[G_BA] + gs[G_BA + 1] * gs[G_BA + 1] + gs[G_BA + 2] * gs[G_BA + 2]);
    return chi;
}

// the normal equations at (v, gs): chain records D O B r, the border sums acc[0:45] = C, acc[45:54] = rhs, acc[54] = chi2 (priors included)
__device__ __forceinline__ void io_build(const IoMap &M, const double *gs, double *acc, double *red2)
{
    const int tid = threadIdx.x, n = M.n;
    if (M.fvb)
        for (int i = tid; i < n * C_R0; i += IO_THREADS) M.ch[(size_t)(i / C_R0) * IO_CH + i % C_R0] = 0.0;
    for (int i = tid; i < n * IO_WS; i += IO_THREADS) {
        const int k = i / IO_WS;
        if (k == 0 || !M.link[k]) M.ws[i] = 0.0;
    }
    __syncthreads();
    for (int parity = 0; parity < 2; parity++) {             // even edges, then odd ones: no two edges of a pass share a keyframe
        for (int k = 2 * tid + parity; k < n; k += 2 * IO_THREADS) {
            if (k < 1 || !M.link[k]) continue;
            double *R = M.ch + (size_t)k * IO_CH, *P1 = R - IO_CH;
            if (M.fvb) io_edge_build<true>(M.kf + (size_t)(k - 1) * IO_KF, M.kf + (size_t)k * IO_KF, P1 + C_V, R + C_V, M.preint + (size_t)k * IO_PRE,
                                           M.info + (size_t)k * 81, gs, M.fgd, M.fsc, R, P1, M.ws + (size_t)k * IO_WS);
            else io_edge_build<false>(M.kf + (size_t)(k - 1) * IO_KF, M.kf + (size_t)k * IO_KF, P1 + C_V, R + C_V, M.preint + (size_t)k * IO_PRE,
                                      M.info + (size_t)k * 81, gs, M.fgd, M.fsc, R, P1, M.ws + (size_t)k * IO_WS);
        }
        __syncthreads();
    }
    // border sums: entry j over the keyframes in index order, four contiguous parts combined in order
    {
        const int j = tid & 63, part = tid >> 6;
        const int k0 = (int)((long long)n * part / 4), k1 = (int)((long long)n * (part + 1) / 4);
        double sum = 0;
        if (j < 55)
            for (int k = k0; k < k1; k++) sum += M.ws[(size_t)k * IO_WS + j];
        red2[part * 64 + j] = sum;
        __syncthreads();
        if (tid < 55) {
            double v = ((red2[tid] + red2[64 + tid]) + red2[128 + tid]) + red2[192 + tid];
            if (tid == 54 && M.fvb) {
                v += M.prior_g * (gs[G_BG] * gs[G_BG] + gs[G_BG + 1] * gs[G_BG + 1] + gs[G_BG + 2] * gs[G_BG + 2]);
                v += M.prior_a * (gs[G_BA] * gs[G_BA] + gs[G_BA + 1] * gs[G_BA + 1] + gs[G_BA + 2] * gs[G_BA + 2]);
            }
            if (M.fvb) {                                     // EdgePriorGyro / EdgePriorAcc: e = 0 - b, the Jacobian +I as G2oTypes.cc:971-983 sets it
                if (tid == sym9(0, 0) || tid == sym9(1, 1) || tid == sym9(2, 2)) v += M.prior_g;
                if (tid == sym9(3, 3) || tid == sym9(4, 4) || tid == sym9(5, 5)) v += M.prior_a;
                if (tid >= 45 && tid < 48) v += M.prior_g * gs[G_BG + tid - 45];
                if (tid >= 48 && tid < 51) v += M.prior_a * gs[G_BA + tid - 48];
            }
            acc[tid] = v;
        }
        __syncthreads();
    }
}

// L.x etc. live in LDS
struct IoLds {
    double st[16], stt[16];      // the map's state and the trial's
    double acc[56];              // border C, rhs, chi2 of the last build
    double S[54];                // the border's Schur complement and right-hand side, full width
    double A[81], ar[9];         // the free columns' system
    double xb[9];                // the border's step, full width (fixed columns 0)
    double red[4], red2[256];
    int fidx[9], nb, ok;
    long long prof[2];           // ORBHIP_IO_PROF: thread 0's cycles in the chain elimination / in the border solve + back substitution
};

// the arrowhead solve with lambda on the diagonal; false = a pivot was not positive.  On success x is in the records and L.xb.
__device__ __forceinline__ bool io_solve(const IoMap &M, IoLds &L, double lam)
{
    const int tid = threadIdx.x, n = M.n;
    if (tid == 0) L.ok = 1;
    if (M.fvb) {
        // inactive keyframes (no edge) become identity blocks: their step is zero; lambda on the others; keep the right-hand side
        for (int k = tid; k < n; k += IO_THREADS) {
            double *R = M.ch + (size_t)k * IO_CH;
            const bool active = (k > 0 && M.link[k]) || (k + 1 < n && M.link[k + 1]);
            if (active) { R[C_D + 0] += lam; R[C_D + 3] += lam; R[C_D + 5] += lam; }
            else { R[C_D + 0] = 1.0; R[C_D + 3] = 1.0; R[C_D + 5] = 1.0; }
            R[C_R0 + 0] = R[C_R + 0]; R[C_R0 + 1] = R[C_R + 1]; R[C_R0 + 2] = R[C_R + 2];
        }
        __syncthreads();
        const long long t_sweep = tid == 0 ? clock64() : 0;
        if (tid < 64) {                                      // the sweep: every lane repeats the 3x3 recursion, lane c < 9 carries border column c, lane 9 the rhs
            const int lane = tid;
            bool ok = true;
            double Di[6] = {0, 0, 0, 0, 0, 0}, pc[3] = {0, 0, 0};
            for (int k = 0; k < n && ok; k++) {
                double *R = M.ch + (size_t)k * IO_CH;
                double D[6], c3[3] = {0, 0, 0};
#pragma unroll
                for (int i = 0; i < 6; i++) D[i] = R[C_D + i];
                if (lane < 9) { c3[0] = R[C_B + lane]; c3[1] = R[C_B + 9 + lane]; c3[2] = R[C_B + 18 + lane]; }
                else if (lane == 9) { c3[0] = R[C_R]; c3[1] = R[C_R + 1]; c3[2] = R[C_R + 2]; }
                if (k > 0 && M.link[k]) {
                    double O[9], G[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) O[i] = R[C_O + i];
#pragma unroll
                    for (int b = 0; b < 3; b++) {            // G = D~(k-1)^-1 O
                        G[b] = Di[0] * O[b] + Di[1] * O[3 + b] + Di[2] * O[6 + b];
                        G[3 + b] = Di[1] * O[b] + Di[3] * O[3 + b] + Di[4] * O[6 + b];
                        G[6 + b] = Di[2] * O[b] + Di[4] * O[3 + b] + Di[5] * O[6 + b];
                    }
#pragma unroll
                    for (int a = 0; a < 3; a++) {
#pragma unroll
                        for (int b = a; b < 3; b++) D[sym3(a, b)] -= G[a] * O[b] + G[3 + a] * O[3 + b] + G[6 + a] * O[6 + b];
                        c3[a] -= G[a] * pc[0] + G[3 + a] * pc[1] + G[6 + a] * pc[2];
                    }
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < 9; i++) R[C_O + i] = G[i];
                    }
                }
                // LDL^T of the block without pivoting, its inverse from the factors
                const double d0 = D[0], l10 = D[1] / d0, l20 = D[2] / d0;
                const double d1 = D[3] - l10 * D[1], t21 = D[4] - l20 * D[1], l21 = t21 / d1;
                const double d2 = D[5] - l20 * D[2] - l21 * t21;
                ok = d0 > 0 && d1 > 0 && d2 > 0 && isfinite(d0) && isfinite(d1) && isfinite(d2);
                const double m20 = l10 * l21 - l20, i0 = 1.0 / d0, i1 = 1.0 / d1, i2 = 1.0 / d2;
                Di[5] = i2; Di[4] = -l21 * i2; Di[2] = m20 * i2;
                Di[3] = i1 + l21 * l21 * i2; Di[1] = -l10 * i1 - l21 * m20 * i2;
                Di[0] = i0 + l10 * l10 * i1 + m20 * m20 * i2;
                const double w0 = Di[0] * c3[0] + Di[1] * c3[1] + Di[2] * c3[2], w1 = Di[1] * c3[0] + Di[3] * c3[1] + Di[4] * c3[2],
                             w2 = Di[2] * c3[0] + Di[4] * c3[1] + Di[5] * c3[2];
                if (lane < 9) { R[C_B + lane] = w0; R[C_B + 9 + lane] = w1; R[C_B + 18 + lane] = w2; }
                else if (lane == 9) { R[C_R] = w0; R[C_R + 1] = w1; R[C_R + 2] = w2; }
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 6; i++) R[C_D + i] = D[i];
                }
                pc[0] = c3[0]; pc[1] = c3[1]; pc[2] = c3[2];
            }
            if (lane == 0 && !ok) L.ok = 0;
            if (lane == 0) L.prof[0] += clock64() - t_sweep;
        }
        __syncthreads();
        if (!L.ok) return false;
        // Schur complement of the chain in the border: S = C - sum_k W^T D~ W, entry j over k in order, four parts combined in order
        {
            const int j = tid & 63, part = tid >> 6;
            const int k0 = (int)((long long)n * part / 4), k1 = (int)((long long)n * (part + 1) / 4);
            double sum = 0;
            if (j < 54) {
                int ci = 0, cj;
                if (j < 45) { int rem = j; while (rem >= 9 - ci) { rem -= 9 - ci; ci++; } cj = ci + rem; }
                else { ci = j - 45; cj = 9; }
                for (int k = k0; k < k1; k++) {
                    const double *R = M.ch + (size_t)k * IO_CH;
                    const double a0 = R[C_B + ci], a1 = R[C_B + 9 + ci], a2 = R[C_B + 18 + ci];
                    const double b0 = cj < 9 ? R[C_B + cj] : R[C_R], b1 = cj < 9 ? R[C_B + 9 + cj] : R[C_R + 1], b2 = cj < 9 ? R[C_B + 18 + cj] : R[C_R + 2];
                    sum += a0 * (R[0] * b0 + R[1] * b1 + R[2] * b2) + a1 * (R[1] * b0 + R[3] * b1 + R[4] * b2) + a2 * (R[2] * b0 + R[4] * b1 + R[5] * b2);
                }
            }
            L.red2[part * 64 + j] = sum;
            __syncthreads();
            if (tid < 54) L.S[tid] = L.acc[tid] - (((L.red2[tid] + L.red2[64 + tid]) + L.red2[128 + tid]) + L.red2[192 + tid]);
        }
    } else if (tid < 54) L.S[tid] = L.acc[tid];
    __syncthreads();
    if (tid == 0) {                                          // the free columns: LDL^T without pivoting
        const long long t_b = clock64();
        const int nb = L.nb;
        bool ok = true;
        for (int a = 0; a < nb; a++) {
            for (int b = 0; b < nb; b++) {
                const int fa = L.fidx[a], fb = L.fidx[b];
                L.A[9 * a + b] = L.S[fa <= fb ? sym9(fa, fb) : sym9(fb, fa)] + (a == b ? lam : 0.0);
            }
            L.ar[a] = L.S[45 + L.fidx[a]];
        }
        for (int j = 0; j < nb && ok; j++) {                 // A[i][j] (i > j) <- L, A[j][j] <- d
            double d = L.A[9 * j + j];
            for (int p = 0; p < j; p++) d -= L.A[9 * j + p] * L.A[9 * j + p] * L.A[9 * p + p];
            ok = d > 0 && isfinite(d);
            L.A[9 * j + j] = d;
            for (int i = j + 1; i < nb; i++) {
                double v = L.A[9 * i + j];
                for (int p = 0; p < j; p++) v -= L.A[9 * i + p] * L.A[9 * j + p] * L.A[9 * p + p];
                L.A[9 * i + j] = v / d;
            }
        }
        if (ok) {
            for (int i = 0; i < nb; i++) { double v = L.ar[i]; for (int p = 0; p < i; p++) v -= L.A[9 * i + p] * L.ar[p]; L.ar[i] = v; }
            for (int i = 0; i < nb; i++) L.ar[i] /= L.A[9 * i + i];
            for (int i = nb - 1; i >= 0; i--) { double v = L.ar[i]; for (int p = i + 1; p < nb; p++) v -= L.A[9 * p + i] * L.ar[p]; L.ar[i] = v; }
            for (int c = 0; c < 9; c++) L.xb[c] = 0.0;
            for (int a = 0; a < nb; a++) L.xb[L.fidx[a]] = L.ar[a];
        } else L.ok = 0;
        L.prof[1] += clock64() - t_b;
    }
    __syncthreads();
    if (!L.ok) return false;
    if (M.fvb) {                                             // back substitution: y = W_r - W_B xb for every keyframe, then the chain from its end
        for (int k = tid; k < n; k += IO_THREADS) {
            double *R = M.ch + (size_t)k * IO_CH;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                double v = R[C_R + a];
                for (int c = 0; c < 9; c++) v -= R[C_B + 9 * a + c] * L.xb[c];
                R[C_X + a] = v;
            }
        }
        __syncthreads();
        if (tid == 0) {
            const long long t_b = clock64();
            double x0 = 0, x1 = 0, x2 = 0;
            bool coupled = false;                            // keyframe k + 1 is linked to k
            for (int k = n - 1; k >= 0; k--) {
                double *R = M.ch + (size_t)k * IO_CH;
                double y0 = R[C_X], y1 = R[C_X + 1], y2 = R[C_X + 2];
                if (coupled) {
                    const double *G = R + IO_CH + C_O;
                    y0 -= G[0] * x0 + G[1] * x1 + G[2] * x2; y1 -= G[3] * x0 + G[4] * x1 + G[5] * x2; y2 -= G[6] * x0 + G[7] * x1 + G[8] * x2;
                    R[C_X] = y0; R[C_X + 1] = y1; R[C_X + 2] = y2;
                }
                x0 = y0; x1 = y1; x2 = y2;
                coupled = k > 0 && M.link[k];
            }
            L.prof[1] += clock64() - t_b;
        }
        __syncthreads();
    }
    return true;
}

// the state after the step (records' x, L.xb): velocities into record offset voff_out, the map's state into go
__device__ __forceinline__ void io_apply(const IoMap &M, IoLds &L, const double *gi, double *go, int voff_out)
{
    const int tid = threadIdx.x;
    if (M.fvb)
        for (int k = tid; k < M.n; k += IO_THREADS) {
            double *R = M.ch + (size_t)k * IO_CH;
            R[voff_out] = R[C_V] + R[C_X]; R[voff_out + 1] = R[C_V + 1] + R[C_X + 1]; R[voff_out + 2] = R[C_V + 2] + R[C_X + 2];
        }
    if (tid == 0) {
        double t[16];
#pragma unroll
        for (int i = 0; i < 16; i++) t[i] = gi[i];
        if (M.fvb) {
#pragma unroll
            for (int i = 0; i < 6; i++) t[G_BG + i] = gi[G_BG + i] + L.xb[i];
        }
        if (M.fgd) {                                         // GDirection::Update: Rwg <- Rwg ExpSO3(d0, d1, 0)
            const double w[3] = {L.xb[6], L.xb[7], 0.0};
            double E[9], Rn[9];
            so3_exp(w, E, 1e-5, true);
            mm3(gi + G_R, E, Rn);
#pragma unroll
            for (int i = 0; i < 9; i++) t[G_R + i] = Rn[i];
        }
        if (M.fsc) t[G_S] = gi[G_S] * exp(L.xb[8]);            // VertexScale::oplusImpl
#pragma unroll
        for (int i = 0; i < 16; i++) go[i] = t[i];
    }
    __syncthreads();
}

__global__ __launch_bounds__(IO_THREADS) void k_inertial_opt(IoArgs A)
{
    extern __shared__ double io_dyn[];
    __shared__ IoLds L;
    const int m = blockIdx.x, tid = threadIdx.x;
    const int k_begin = A.kf_off[m], n = A.kf_off[m + 1] - k_begin;
    IoMap M;
    M.n = n; M.kf = A.kf + (size_t)k_begin * IO_KF; M.link = A.link + k_begin;
    M.preint = A.preint + (size_t)k_begin * IO_PRE; M.info = A.info + (size_t)k_begin * 81;
    M.ch = n <= A.lds_kf ? io_dyn : A.ws_chain + (size_t)k_begin * IO_CH;
    M.ws = A.ws_edge + (size_t)k_begin * IO_WS;
    M.fvb = A.fvb != 0; M.fgd = A.fgd != 0; M.fsc = A.fsc != 0; M.prior_g = A.prior_g; M.prior_a = A.prior_a;
    double *glob = A.global + (size_t)m * ORBHIP_IO_GLOBAL;
    if (tid < 16) L.st[tid] = glob[tid];
    if (tid < 9) L.xb[tid] = 0.0;
    const long long t_begin = tid == 0 ? clock64() : 0;
    if (tid == 0) { L.prof[0] = 0; L.prof[1] = 0; }
    if (tid == 0) {
        int nb = 0;
        if (M.fvb) for (int c = 0; c < 6; c++) L.fidx[nb++] = c;
        if (M.fgd) { L.fidx[nb++] = 6; L.fidx[nb++] = 7; }
        if (M.fsc) L.fidx[nb++] = 8;
        L.nb = nb;
    }
    for (int k = tid; k < n; k += IO_THREADS) {
        double *R = M.ch + (size_t)k * IO_CH;
#pragma unroll
        for (int a = 0; a < 3; a++) { R[C_V + a] = M.kf[(size_t)k * IO_KF + K_V + a]; R[C_VT + a] = R[C_V + a]; R[C_X + a] = 0.0; }
    }
    __syncthreads();

    int iters = 0, trials = 0, reason = 0;
    double lam = A.gn ? 0.0 : A.lambda_init, ni = 2.0, chi_first = 0, chi_cur = 0;
    int nbad = 0;
    if (A.gn) {
        for (int it = 0; it < A.iterations; it++) {
            io_build(M, L.st, L.acc, L.red2);
            chi_cur = L.acc[54];
            if (it == 0) chi_first = chi_cur;
            if (!isfinite(chi_cur)) { reason = 3; break; }
            iters++;
            const bool ok = io_solve(M, L, 0.0);
            // OptimizationAlgorithmGaussNewton::solve updates with the solver's x whether or not the factorisation succeeded: after a
            // failure x is still the last successful step (zero before the first), and optimize() stops
            io_apply(M, L, L.st, L.stt, C_V);
            if (tid < 16) L.st[tid] = L.stt[tid];
            __syncthreads();
            if (A.trace && tid == 0) { double *tr = A.trace + ((size_t)m * A.iterations + it) * 2; tr[0] = chi_cur; tr[1] = 0.0; }
            if (!ok) { reason = 2; break; }
        }
        chi_cur = io_chi2(M, C_V, L.st, L.red);
    } else {
        chi_cur = io_chi2(M, C_V, L.st, L.red);
        chi_first = chi_cur;
        for (int it = 0; it < A.iterations; it++) {
            if (!isfinite(chi_cur) || !isfinite(lam)) { reason = 3; break; }
            iters++;
            const double ini_chi = chi_cur;
            double rho = 0;
            int q = 0;
            while (q < A.max_trials) {
                io_build(M, L.st, L.acc, L.red2);
                if (it == 0 && q == 0 && !(A.lambda_init > 0)) {      // computeLambdaInit: tau * the largest diagonal entry
                    double mx = 0;
                    if (M.fvb)
                        for (int k = tid; k < n; k += IO_THREADS) {
                            const double *R = M.ch + (size_t)k * IO_CH;
                            mx = fmax(mx, fmax(fabs(R[C_D]), fmax(fabs(R[C_D + 3]), fabs(R[C_D + 5]))));
                        }
                    L.red2[tid] = mx;
                    __syncthreads();
                    mx = 0;
                    for (int i = 0; i < IO_THREADS; i++) mx = fmax(mx, L.red2[i]);
                    for (int a = 0; a < L.nb; a++) mx = fmax(mx, fabs(L.acc[sym9(L.fidx[a], L.fidx[a])]));
                    __syncthreads();
                    lam = 1e-50 * mx;
                }
                const bool ok = io_solve(M, L, lam);
                trials++;
                bool good = false;
                if (ok) {
                    io_apply(M, L, L.st, L.stt, C_VT);
                    const double chi_t = io_chi2(M, C_VT, L.stt, L.red);
                    double part = 0;                          // computeScale: sum x (lambda x + b)
                    if (M.fvb)
                        for (int k = tid; k < n; k += IO_THREADS) {
                            const double *R = M.ch + (size_t)k * IO_CH;
#pragma unroll
                            for (int a = 0; a < 3; a++) part += R[C_X + a] * (lam * R[C_X + a] + R[C_R0 + a]);
                        }
                    double scale = io_block_sum(part, L.red);
                    for (int a = 0; a < L.nb; a++) { const int c = L.fidx[a]; scale += L.xb[c] * (lam * L.xb[c] + L.acc[45 + c]); }
                    scale += 1e-3;
                    rho = (chi_cur - chi_t) / scale;
                    good = rho > 0 && isfinite(chi_t);
                    if (good) {
                        double alpha = 1. - pow(2 * rho - 1, 3);
                        alpha = fmin(alpha, 2. / 3.);
                        lam *= fmax(1. / 3., alpha);
                        ni = 2;
                        chi_cur = chi_t;
                        __syncthreads();
                        if (M.fvb)
                            for (int k = tid; k < n; k += IO_THREADS) {
                                double *R = M.ch + (size_t)k * IO_CH;
                                R[C_V] = R[C_VT]; R[C_V + 1] = R[C_VT + 1]; R[C_V + 2] = R[C_VT + 2];
                            }
                        if (tid < 16) L.st[tid] = L.stt[tid];
                        __syncthreads();
                    }
                } else rho = -1.0;                            // a failed factorisation is a failed trial
                if (!good) { lam *= ni; ni *= 2; }
                q++;
                if (!(rho < 0)) break;
            }
            if (A.trace && tid == 0) { double *tr = A.trace + ((size_t)m * A.iterations + it) * 2; tr[0] = chi_cur; tr[1] = lam; }
            if (q == A.max_trials || rho == 0) { reason = 1; break; }
            if ((ini_chi - chi_cur) * 1e3 < ini_chi) nbad++; else nbad = 0;      // the fork's stop criterion
            if (nbad >= 3) { reason = 1; break; }
        }
    }
    __syncthreads();
    if (M.fvb)
        for (int k = tid; k < n; k += IO_THREADS) {
            double *s = A.kf + (size_t)(k_begin + k) * IO_KF;
            const double *R = M.ch + (size_t)k * IO_CH;
            s[K_V] = R[C_V]; s[K_V + 1] = R[C_V + 1]; s[K_V + 2] = R[C_V + 2];
#pragma unroll
            for (int i = 0; i < 6; i++) s[K_BG + i] = L.st[G_BG + i];         // SetNewBias(b)
        }
    if (tid < 16) glob[tid] = L.st[tid];
    if (A.stats && tid == 0) {
        double *st = A.stats + (size_t)m * 8;
        int ne = 0;
        for (int k = 1; k < n; k++) ne += M.link[k] ? 1 : 0;
        st[0] = iters; st[1] = trials; st[2] = reason; st[3] = chi_first; st[4] = chi_cur; st[5] = lam; st[6] = ne; st[7] = 0.0;
        if (A.prof) {                                        // diagnostics: shares of the kernel's cycles (thread 0's clock)
            const double total = (double)(clock64() - t_begin);
            st[6] = (double)L.prof[1] / total; st[7] = (double)L.prof[0] / total;
        }
    }
}

}  // namespace

extern "C" int orbhip_inertial_opt_lds_keyframes(void) { return ORBHIP_IO_LDS_KEYFRAMES; }

extern "C" void orbhip_inertial_opt_default_params(orbhip_inertial_opt_params *p, int overload, int mono, int fixed_vel, float priorG, float priorA)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_trials = 100;
    if (overload == 3) {                                     // (Map*, Rwg, scale): Gauss-Newton on direction and scale
        p->free_gdir = 1; p->free_scale = 1; p->gauss_newton = 1; p->iterations = 10;
        return;
    }
    p->iterations = 200;
    p->prior_g = priorG; p->prior_a = priorA;
    if (overload == 0) {
        p->free_vel_bias = fixed_vel ? 0 : 1; p->free_gdir = 1; p->free_scale = mono ? 1 : 0;
        p->lambda_init = priorG != 0.f ? 1e3 : 0.0;
    } else {                                                 // (b), (c): Rwg = I and scale = 1 stay fixed
        p->free_vel_bias = 1;
        p->lambda_init = 1e3;
    }
}

extern "C" int orbhip_inertial_optimization_device(orbhip_ctx *ctx, const orbhip_inertial_opt_params *p, int maps, const int32_t *d_kf_off,
        double *d_kf, const uint8_t *d_link, const double *d_preint, const double *d_info, double *d_global, double *d_stats, double *d_trace)
{
    if (!ctx || !p || maps < 0) return ORBHIP_E_BADARG;
    if (!p->free_vel_bias && !p->free_gdir && !p->free_scale) { orbhip_set_last_error_internal("inertial optimisation: nothing is free"); return ORBHIP_E_BADARG; }
    if (p->iterations < 0 || p->max_trials < 1) { orbhip_set_last_error_internal("inertial optimisation: iterations / max_trials"); return ORBHIP_E_BADARG; }
    if (maps == 0) return ORBHIP_OK;
    if (!d_kf_off || !d_global) return ORBHIP_E_BADARG;
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    // the offsets come back once (maps + 1 words): they are checked here and size the workspace; the solve itself is not waited for
    std::vector<int32_t> off((size_t)maps + 1);
    ORB_HIP_TRY(hipMemcpyAsync(off.data(), d_kf_off, sizeof(int32_t) * off.size(), hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));
    int max_n = 0;
    if (off[0] < 0) { orbhip_set_last_error_internal("inertial optimisation: d_kf_off"); return ORBHIP_E_BADARG; }
    for (int m = 0; m < maps; m++) {
        const long long n = (long long)off[m + 1] - off[m];
        if (n < 0) { orbhip_set_last_error_internal("inertial optimisation: d_kf_off is not monotone"); return ORBHIP_E_BADARG; }
        if (n > IO_MAX_KF) { orbhip_set_last_error_internal("inertial optimisation: more than 4096 keyframes in a map"); return ORBHIP_E_BADARG; }
        if (n > max_n) max_n = (int)n;
    }
    const size_t K = (size_t)off[maps];
    if (K && (!d_kf || !d_link || !d_preint || !d_info)) return ORBHIP_E_BADARG;
    const size_t ws_edge = align256(sizeof(double) * IO_WS * (K + 1)), ws_chain = align256(sizeof(double) * IO_CH * (K + 1));
    uint8_t *work = (uint8_t *)orbhip_ctx_work_internal(ctx, ws_edge + ws_chain);
    if (!work) return ORBHIP_E_HIP;
    IoArgs a;
    a.kf_off = d_kf_off; a.kf = d_kf; a.link = d_link; a.preint = d_preint; a.info = d_info; a.global = d_global; a.stats = d_stats; a.trace = d_trace;
    a.ws_edge = (double *)work; a.ws_chain = (double *)(work + ws_edge);
    a.fvb = p->free_vel_bias ? 1 : 0; a.fgd = p->free_gdir ? 1 : 0; a.fsc = p->free_scale ? 1 : 0; a.gn = p->gauss_newton ? 1 : 0;
    a.iterations = p->iterations; a.max_trials = p->max_trials; a.lds_kf = ORBHIP_IO_LDS_KEYFRAMES;
    { const char *e = getenv("ORBHIP_IO_PROF"); a.prof = e && atoi(e) != 0; }
    a.lambda_init = p->lambda_init; a.prior_g = p->prior_g; a.prior_a = p->prior_a;
    const size_t lds = sizeof(double) * IO_CH * (size_t)(max_n < ORBHIP_IO_LDS_KEYFRAMES ? (max_n > 0 ? max_n : 1) : ORBHIP_IO_LDS_KEYFRAMES);
    if (orb_lds_optin(reinterpret_cast<const void *>(k_inertial_opt), orbhip_ctx_device_internal(ctx), lds)) return ORBHIP_E_HIP;
    hipLaunchKernelGGL(k_inertial_opt, dim3(maps), dim3(IO_THREADS), lds, s, a);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("k_inertial_opt launch"); return ORBHIP_E_HIP; }
    return ORBHIP_OK;
}
