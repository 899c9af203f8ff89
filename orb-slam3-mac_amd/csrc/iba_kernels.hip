// iba_kernels.hip -- Optimizer::LocalInertialBA's numerical core on gfx950 (reference src/Optimizer.cc:4574-5187; vertices and
// edges include/G2oTypes.h + src/G2oTypes.cc: ImuCamPose :25-220, EdgeMono / EdgeStereo :349-482, EdgeInertial :693-800,
// EdgeGyroRW / EdgeAccRW G2oTypes.h:632-700; bias-corrected preintegration src/ImuTypes.cc:351-378; g2o Levenberg-Marquardt
// with the landmark Schur complement as in ba_kernels.hip).
//
// Shape of the problem: <= 25 keyframes with 15 unknowns each (pose 6, velocity 3, gyro bias 3, accelerometer bias 3), up to 200
// fixed keyframes, a few thousand landmarks, a chain of <= 25 inertial edges.  The reduced system is at most 375 x 375 and every
// LM trial is a short dependent chain (errors -> Schur -> LDL^T -> update -> errors), so ONE workgroup of 512 threads owns a
// window for the whole optimisation: no host round trips, no inter-workgroup synchronisation, all LM decisions taken redundantly
// by every thread from block-uniform sums.  A batch of windows is a grid of such workgroups (256 CUs = 256 windows in flight).
// Every sum has a fixed order (per-thread sequential, DPP tree inside a wave, waves in index order): results are deterministic.
//
// Scratch (Jacobian blocks W, H, S ...) lives in global memory and stays L2-resident (a window's working set is < 4 MB); the
// LDL^T panel is the only LDS user (ba_ldlt.h).
#include "orb_internal.h"
#include "ctx_internal.h"
#include "wave_dpp.h"
#include "ba_ldlt.h"
#include "geom3.h"
#include "ba_camera.h"
#include "iba_pack.h"          // IbaWin, the IBA_* sizes and modes, and the host packing (HIP-free)
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>
#include <thread>
#include <functional>
#include <mutex>
#include <fcntl.h>
#include <errno.h>
#include <unistd.h>
#include <sys/file.h>
#include <sys/stat.h>


#define IBA_WAVES (IBA_THREADS / 64)
#define IBA_STAGE 544          // doubles of LDS a wave of workgroup 0 stages an inertial edge in (9 x 24 Jacobian, its Omega-weighted copy, Omega e at 432, the 9 x 9 information at 448)
#define IBA_MAXG 32
enum { K_R = 0, K_T = 9, K_V = 12, K_BG = 15, K_BA = 18 };
enum { P_DT = 0, P_DR = 1, P_DV = 10, P_DP = 13, P_JRG = 16, P_JVG = 25, P_JVA = 34, P_JPG = 43, P_JPA = 52, P_BG = 61, P_BA = 64 };

// Pointers into global memory carry their address space in the TYPE on the device side: the phase functions are not inlined (register
// pressure) and reach IbaArgs through a pointer, where a plain `double *` loaded from memory is a generic pointer and every access
// through it a FLAT instruction (1100 of them in the round-3 kernel: slower than global ones, and counted on BOTH wait counters, so that
// they serialise with the LDS traffic).  gen() hands out the generic pointer the code computes with; the backend's address-space
// inference sees the cast from the global space and emits global instructions.  Same layout on the host, which fills the struct.
#if defined(__HIP_DEVICE_COMPILE__)
#define GPTR(...) __attribute__((address_space(1))) __VA_ARGS__ *
#else
#define GPTR(...) __VA_ARGS__ *
#endif
static_assert(sizeof(IbaInt4) == sizeof(int4) && alignof(IbaInt4) == alignof(int4) && sizeof(IbaInt2) == sizeof(int2) && alignof(IbaInt2) == alignof(int2),
              "iba_pack.h's four-int and two-int structs must be HIP's int4 and int2");
struct IbaArgs {
    GPTR(const IbaWin) win;
    GPTR(const int) kf_xoff;                 // [sumKF] first unknown of the keyframe's block, -1 = fixed
    GPTR(const uint8_t) kf_imu;
    GPTR(const int) free_kf;                 // [sumFree] keyframe of free block f
    GPTR(const int) edge_kf; GPTR(const int) edge_point;    // [sumE] window-local indices
    GPTR(const double) edge_obs; GPTR(const double) edge_is2;
    GPTR(const uint8_t) edge_stereo; GPTR(const uint8_t) edge_close;
    GPTR(const int) pt_start;                // per window L + 1 entries
    GPTR(const int) kf_edges;                // the visual edges of every free keyframe, keyframe by keyframe
    GPTR(const int4) kf_task;                // {free block f, first, end (into kf_edges), 0}: chunks of <= IBA_KF_CHUNK edges
    GPTR(const int) kf_task_start;           // per window nfree + 1: the chunks of block f
    GPTR(const int2) pair_ent;               // {edge of block i, edge of block j} of every landmark both see, pair by pair (i <= j, row-major)
    GPTR(const int4) pair_task;              // {pair, first, end (into pair_ent), i == j}: chunks of <= IBA_PAIR_CHUNK entries
    GPTR(const int) pair_task_start;         // per window npairs + 1
    GPTR(const int) in_kf1; GPTR(const int) in_kf2; GPTR(const int) in_color; GPTR(const uint8_t) in_robust;
    GPTR(const double) in_pre; GPTR(const double) in_info; GPTR(const double) in_info_g; GPTR(const double) in_info_a;
    GPTR(double) kfs; GPTR(double) cam; GPTR(double) pts;            // estimates, two buffers each: [2][sumKF][21], [2][sumKF][2 cameras][12] (Rcw, tcw), [2][sumL][3]
    long long kfs_stride, cam_stride, pts_stride;
    GPTR(double) err; GPTR(double) chi2; GPTR(double) W; GPTR(double) Hll; GPTR(double) bl; GPTR(double) Dinv; GPTR(double) db; GPTR(double) xl;
    GPTR(double) ierr; GPTR(double) ichi2; GPTR(double) Jb; GPTR(double) OJ; GPTR(double) Oe;
    GPTR(double) H; GPTR(double) S; GPTR(double) b; GPTR(double) bs; GPTR(double) x;
    GPTR(double) kpart; GPTR(double) ppart;              // [kf tasks][27], [pair tasks][42] partial sums
    GPTR(unsigned) counters; GPTR(int) fail; GPTR(int) okflag;   // per window: team barrier counter, barrier time-out flag, LDL^T status
    GPTR(double) wpart;                      // per window [2][IBA_MAXG][2]
    int G, n_windows;                   // workgroups per window
    GPTR(uint8_t) outlier;
    GPTR(orbhip_iba_stats) stats;
    int iterations, max_trials, large, max_n;
    double lambda_init;
    GPTR(long long) prof;                    // optional [windows][16] shader-clock cycles per phase (ORBHIP_IBA_PROF=1): errors, build, prep+Schur, LDL^T, update
    // FullInertialBA only (k_fiba_solve; k_iba_solve reads none of these)
    GPTR(double) sbias;                      // [2][windows][6] the shared gyro / accelerometer bias estimate, double buffered like kfs
    GPTR(double) spart;                      // [sumM][42] per-edge parts of the shared 6x6 block and its right-hand side
    GPTR(orbhip_fiba_stats) fstats;
    double prior_g, prior_a;
};

#if defined(__HIP_DEVICE_COMPILE__)
template <class T>
__device__ __forceinline__ T *gen(__attribute__((address_space(1))) T *p) { return (T *)p; }
#else
template <class T>
__host__ __device__ inline T *gen(T *p) { return p; }      // (the host pass only parses the device functions)
#endif
#define GA(f) gen(A.f)
// ------------------------------------------------------------------ small dense helpers (row-major 3x3; the products and huber: geom3.h)
namespace {
__device__ __forceinline__ void skew3(const double *w, double *W)
{
    W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
__device__ __forceinline__ void inv3(const double *A, double *I)
{
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double id = 1.0 / (A[0] * c0 + A[1] * c1 + A[2] * c2);
    I[0] = c0 * id; I[1] = (A[2] * A[7] - A[1] * A[8]) * id; I[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    I[3] = c1 * id; I[4] = (A[0] * A[8] - A[2] * A[6]) * id; I[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    I[6] = c2 * id; I[7] = (A[1] * A[6] - A[0] * A[7]) * id; I[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}
// nearest rotation (IMU::NormalizeRotation, ImuTypes.cc:30-36, takes U V^T of an SVD): two Newton polar steps
__device__ __forceinline__ void normalize_rotation(double *R)
{
    for (int it = 0; it < 2; it++) {
        double I[9];
        inv3(R, I);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[3 * i + j] = 0.5 * (R[3 * i + j] + I[3 * j + i]);
    }
}
__device__ __forceinline__ void rodrigues(const double *w, double a, double b, double *R)     // I + a W + b W W
{
    double W[9], W2[9];
    skew3(w, W); mm3(W, W, W2);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = a * W[i] + b * W2[i];
    R[0] += 1; R[4] += 1; R[8] += 1;
}
__device__ void exp_so3(const double *w, double *R, double eps, bool normalize)     // G2oTypes.cc:991-1008 (1e-5, normalised) / ImuTypes.cc:48-60 (1e-4)
{
    const double d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], d = sqrt(d2);
    if (d < eps) rodrigues(w, 1.0, 0.5, R);
    else rodrigues(w, sin(d) / d, (1.0 - cos(d)) / d2, R);
    if (normalize) normalize_rotation(R);
}
__device__ void log_so3(const double *R, double *w)     // G2oTypes.cc:1010-1025
{
    const double tr = R[0] + R[4] + R[8];
    w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5;
    if (costheta > 1 || costheta < -1) return;
    const double theta = acos(costheta), s = sin(theta);
    if (fabs(s) < 1e-5) return;
    for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}
__device__ void inv_right_jac(const double *v, double *J)     // G2oTypes.cc:1032-1044
{
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
    if (d < 1e-5) { for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    rodrigues(v, 0.5, 1.0 / d2 - (1.0 + cos(d)) / (2.0 * d * sin(d)), J);
}
__device__ void right_jac(const double *v, double *J)         // G2oTypes.cc:1046-1061
{
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
    if (d < 1e-5) { for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    rodrigues(v, -(1.0 - cos(d)) / d2, (d - sin(d)) / (d2 * d), J);
}
// camera `idx` of the rig: extrinsics w.r.t. the body (G2oTypes.cc:49-52, 57-67) and intrinsics
struct CamView { const double *Rcb, *tcb, *kb; double fx, fy, cx, cy; int model; };
__device__ __forceinline__ CamView cam_view(const IbaWin &W, int idx)
{
    CamView V;
    if (idx == 0) { V.Rcb = W.Rcb; V.tcb = W.tcb; V.kb = W.kb; V.fx = W.fx; V.fy = W.fy; V.cx = W.cx; V.cy = W.cy; V.model = W.cam_model; }
    else { V.Rcb = W.Rcb2; V.tcb = W.tcb2; V.kb = W.kb2; V.fx = W.fx2; V.fy = W.fy2; V.cx = W.cx2; V.cy = W.cy2; V.model = W.cam2_model; }
    return V;
}
// Rcw = Rcb Rbw, tcw = Rcb tbw + tcb for every camera of the keyframe (ImuCamPose::Update, G2oTypes.cc:212-219); c: [2][12]
__device__ void cam_pose(const IbaWin &W, const double *s, double *c)
{
    double Rbw[9], tbw[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rbw[3 * i + j] = s[K_R + 3 * j + i];
    mv3(Rbw, s + K_T, tbw);
    for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
    for (int cam = 0; cam <= W.has_cam2; cam++) {
        const CamView V = cam_view(W, cam);
        double R[9], t[3];
        mm3(V.Rcb, Rbw, R);
        mv3(V.Rcb, tbw, t);
        for (int i = 0; i < 9; i++) c[12 * cam + i] = R[i];
        for (int i = 0; i < 3; i++) c[12 * cam + 9 + i] = t[i] + V.tcb[i];
    }
}

// EdgeMono / EdgeStereo::computeError (G2oTypes.h:350-355, G2oTypes.cc:170-185); type 0 EdgeMono(0), 1 EdgeStereo(0), 2 EdgeMono(1);
// c = the pose of the edge's camera
__device__ __forceinline__ void visual_error(const IbaWin &W, const CamView &V, const double *c, const double *X, const double *obs, int type, double *er, double *Xc)
{
    mv3(c, X, Xc);
    Xc[0] += c[9]; Xc[1] += c[10]; Xc[2] += c[11];
    double uv[2];
    cam_project(V.fx, V.fy, V.cx, V.cy, V.model, V.kb, Xc, uv);
    er[0] = obs[0] - uv[0]; er[1] = obs[1] - uv[1];
    er[2] = type == 1 ? obs[2] - (uv[0] - W.bf * (1 / Xc[2])) : 0.0;
}

// linearizeOplus (G2oTypes.cc:349-373, :397-423): Jx [3][3], Jp [3][6]; row 2 zero when mono
__device__ void visual_jac(const IbaWin &W, const CamView &V, const double *c, const double *Xc, int type, double *Jx, double *Jp)
{
    double pj[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    cam_project_jac(V.fx, V.fy, V.model, V.kb, Xc, pj);
    if (type == 1) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + W.bf * (1.0 / (Xc[2] * Xc[2])); }
#pragma unroll
    for (int d = 0; d < 3; d++)
#pragma unroll
        for (int j = 0; j < 3; j++) Jx[3 * d + j] = -(pj[3 * d] * c[j] + pj[3 * d + 1] * c[3 + j] + pj[3 * d + 2] * c[6 + j]);
    double Xb[3];
    const double d0[3] = {Xc[0] - V.tcb[0], Xc[1] - V.tcb[1], Xc[2] - V.tcb[2]};
    mtv3(V.Rcb, d0, Xb);
    double PR[9];
    mm3(pj, V.Rcb, PR);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double p0 = PR[3 * d], p1 = PR[3 * d + 1], p2 = PR[3 * d + 2];
        Jp[6 * d + 0] = p1 * -Xb[2] + p2 * Xb[1];            // SE3deriv columns: (0,-z,y) (z,0,-x) (-y,x,0) | I
        Jp[6 * d + 1] = p0 * Xb[2] + p2 * -Xb[0];
        Jp[6 * d + 2] = p0 * -Xb[1] + p1 * Xb[0];
        Jp[6 * d + 3] = p0; Jp[6 * d + 4] = p1; Jp[6 * d + 5] = p2;
    }
}

// EdgeInertial::computeError (+ linearizeOplus into J [9][24] when J != nullptr), G2oTypes.cc:720-800.  The body is inlined where a
// kernel must stay free of calls (a call's frame is scratch); inertial_edge is the out-of-line form the local BA calls.
__device__ __forceinline__ void inertial_edge_body(const double *s1, const double *s2, const double *pi, double *err, double *J)
{
    const double dt = pi[P_DT];
    const double g[3] = {0, 0, -(double)9.81f};
    double dbg[3], dba[3], w[3], E[9], dR[9], dV[3], dP[3], t[3];
    for (int i = 0; i < 3; i++) { dbg[i] = s1[K_BG + i] - pi[P_BG + i]; dba[i] = s1[K_BA + i] - pi[P_BA + i]; }
    mv3(pi + P_JRG, dbg, w);
    exp_so3(w, E, 1e-4, false);
    mm3(pi + P_DR, E, dR);
    normalize_rotation(dR);
    mv3(pi + P_JVG, dbg, dV); mv3(pi + P_JVA, dba, t);
    for (int i = 0; i < 3; i++) dV[i] = pi[P_DV + i] + dV[i] + t[i];
    mv3(pi + P_JPG, dbg, dP); mv3(pi + P_JPA, dba, t);
    for (int i = 0; i < 3; i++) dP[i] = pi[P_DP + i] + dP[i] + t[i];
    double R12[9], eR[9], er[3], a[3], b[3], va[3], vb[3];
    mtm3(s1 + K_R, s2 + K_R, R12);
    mtm3(dR, R12, eR);
    log_so3(eR, er);
    for (int i = 0; i < 3; i++) {
        a[i] = s2[K_V + i] - s1[K_V + i] - g[i] * dt;
        b[i] = s2[K_T + i] - s1[K_T + i] - s1[K_V + i] * dt - g[i] * dt * dt / 2;
    }
    mtv3(s1 + K_R, a, va); mtv3(s1 + K_R, b, vb);
    for (int i = 0; i < 3; i++) { err[i] = er[i]; err[3 + i] = va[i] - dV[i]; err[6 + i] = vb[i] - dP[i]; }
    if (!J) return;
    for (int i = 0; i < 216; i++) J[i] = 0.0;
    double invJr[9], T[9], S[9];
    inv_right_jac(er, invJr);
#define SETB(r0, c0, M, sgn) for (int i_ = 0; i_ < 3; i_++) for (int j_ = 0; j_ < 3; j_++) J[24 * ((r0) + i_) + (c0) + j_] = (sgn) * (M)[3 * i_ + j_]
    mtm3(s2 + K_R, s1 + K_R, T); mm3(invJr, T, T); SETB(0, 0, T, -1.0);
    skew3(va, S); SETB(3, 0, S, 1.0);
    skew3(vb, S); SETB(6, 0, S, 1.0);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    SETB(6, 3, I3, -1.0);
    double Rbw1[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rbw1[3 * i + j] = s1[K_R + 3 * j + i];
    SETB(3, 6, Rbw1, -1.0);
    SETB(6, 6, Rbw1, -dt);
    double RJ[9], eRt[9];
    right_jac(w, RJ);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) eRt[3 * i + j] = eR[3 * j + i];
    mm3(invJr, eRt, T); mm3(T, RJ, T); mm3(T, pi + P_JRG, T); SETB(0, 9, T, -1.0);
    SETB(3, 9, pi + P_JVG, -1.0);
    SETB(6, 9, pi + P_JPG, -1.0);
    SETB(3, 12, pi + P_JVA, -1.0);
    SETB(6, 12, pi + P_JPA, -1.0);
    SETB(0, 15, invJr, 1.0);
    SETB(6, 18, R12, 1.0);
    SETB(3, 21, Rbw1, 1.0);
#undef SETB
}
__device__ __noinline__ void inertial_edge(const double *s1, const double *s2, const double *pi, double *err, double *J)
{
    inertial_edge_body(s1, s2, pi, err, J);
}

// ------------------------------------------------------------------ a window's team of workgroups
// G workgroups work on one window (G = 1 for big batches: plain __syncthreads semantics).  team_sync is a monotonic-counter
// barrier (MI355X_MICROARCH.md "barrier-counter": lane-0 agent release fence + drained vmcnt before the arrive, relaxed polls
// with s_sleep, agent acquire fence after); the grid is sized by the host so that all workgroups are resident (cooperative
// launch), and every spin is bounded: a barrier that does not complete sets *fail and lets the kernel run out.
struct Team {
    int w, g, G, gtid, gsize, gwave, gwaves;
    unsigned *counter;          // per window, zeroed by the host
    unsigned epoch;             // barriers passed so far (uniform)
    double *wpart;              // [2][IBA_MAXG][2] cross-workgroup partial sums, double buffered
    int slot;
    int *fail;                  // per window
};

__device__ __forceinline__ void team_sync(Team &T)
{
    __syncthreads();
    if (T.G > 1) {
        T.epoch++;
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(T.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned target = T.epoch * (unsigned)T.G;
            long long spins = 0;
            while (__hip_atomic_load(T.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > (1ll << 22) || __hip_atomic_load(T.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {       // seconds: never in a resident grid
                    __hip_atomic_store(T.fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
    }
}

// team-uniform sums of two per-thread values: DPP tree inside each wave, the 16 wave sums in index order, then the G workgroup
// sums in index order (fixed association for a given G)
__device__ __forceinline__ void team_sum2(Team &T, double &a, double &b, double *red)
{
    a = wave_sum_f64_dpp(a); b = wave_sum_f64_dpp(b);
    __syncthreads();                                         // red may still be read by the previous call
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = a; red[2 * (threadIdx.x >> 6) + 1] = b; }
    __syncthreads();
    double sa = 0, sb = 0;
#pragma unroll
    for (int w = 0; w < IBA_WAVES; w++) { sa += red[2 * w]; sb += red[2 * w + 1]; }
    if (T.G > 1) {
        double *wp = T.wpart + (size_t)T.slot * IBA_MAXG * 2;
        if (threadIdx.x == 0) { wp[2 * T.g] = sa; wp[2 * T.g + 1] = sb; }
        team_sync(T);
        sa = 0; sb = 0;
        for (int g = 0; g < T.G; g++) { sa += wp[2 * g]; sb += wp[2 * g + 1]; }
        T.slot ^= 1;
    }
    a = sa; b = sb;
}

struct IbaCtx {            // per-window views (all threads hold the same values)
    GPTR(const IbaWin) W;
    GPTR(const IbaArgs) A;
    double delta_m, dsqr_m, delta_s, dsqr_s, delta_i, dsqr_i;
};

// computeActiveErrors at estimate buffer `buf`: per-edge errors / chi2 to global memory; returns this THREAD's share of
// activeRobustChi2 (the caller sums over the team)
template <bool SHARED>
__device__ __noinline__ double iba_errors(const IbaCtx &C, const Team &T, int buf)
{
    const IbaWin &W = *gen(C.W); const IbaArgs &A = *gen(C.A);
    const double *cam = GA(cam) + buf * A.cam_stride + (size_t)W.kf_off * 24;
    const double *pts = GA(pts) + buf * A.pts_stride + (size_t)W.pt_off * 3;
    const double *kfs = GA(kfs) + buf * A.kfs_stride + (size_t)W.kf_off * IBA_KF;
    double part = 0.0;
    for (int e = T.gtid; e < W.E; e += T.gsize) {
        const size_t ge = (size_t)W.e_off + e;
        const int type = GA(edge_stereo)[ge], st = type == 1;
        double er[3], Xc[3];
        visual_error(W, cam_view(W, type == 2), cam + 24 * GA(edge_kf)[ge] + 12 * (type == 2), pts + 3 * GA(edge_point)[ge], GA(edge_obs) + 3 * ge, type, er, Xc);
        const double chi = (er[0] * er[0] + er[1] * er[1] + er[2] * er[2]) * GA(edge_is2)[ge];
        GA(err)[3 * ge] = er[0]; GA(err)[3 * ge + 1] = er[1]; GA(err)[3 * ge + 2] = er[2];
        GA(chi2)[ge] = chi;
        double r0, r1;
        huber(chi, st ? C.delta_s : C.delta_m, st ? C.dsqr_s : C.dsqr_m, &r0, &r1);
        part += r0;
    }
    // inertial edges: the last threads of the team (the first ones carry the most visual edges)
    const int m = T.gsize - 1 - T.gtid;
    if (m < W.M) {
        const size_t gm = (size_t)W.m_off + m;
        const double *s1 = kfs + IBA_KF * GA(in_kf1)[gm], *s2 = kfs + IBA_KF * GA(in_kf2)[gm];
        double er[15];
        inertial_edge(s1, s2, GA(in_pre) + IBA_PRE * gm, er, nullptr);
        for (int i = 0; i < 3; i++) { er[9 + i] = s2[K_BG + i] - s1[K_BG + i]; er[12 + i] = s2[K_BA + i] - s1[K_BA + i]; }
        const double *I9 = GA(in_info) + 81 * gm;
        double c9 = 0, cg = 0, ca = 0;
        for (int i = 0; i < 9; i++) { double r = 0; for (int j = 0; j < 9; j++) r += I9[9 * i + j] * er[j]; c9 += er[i] * r; }
        if constexpr (!SHARED) {                                  // (shared biases: no EdgeGyroRW / EdgeAccRW)
            const double *Ig = GA(in_info_g) + 9 * gm, *Ia = GA(in_info_a) + 9 * gm;
            for (int i = 0; i < 3; i++) {
                double r = 0, q = 0;
                for (int j = 0; j < 3; j++) { r += Ig[3 * i + j] * er[9 + j]; q += Ia[3 * i + j] * er[12 + j]; }
                cg += er[9 + i] * r; ca += er[12 + i] * q;
            }
        }
        for (int i = 0; i < 15; i++) GA(ierr)[15 * gm + i] = er[i];
        GA(ichi2)[3 * gm] = c9; GA(ichi2)[3 * gm + 1] = cg; GA(ichi2)[3 * gm + 2] = ca;
        double r0 = c9, r1;
        if (GA(in_robust)[gm]) huber(c9, C.delta_i, C.dsqr_i, &r0, &r1);
        part += r0 + cg + ca;
    }
    if constexpr (SHARED) {
        // EdgePriorGyro / EdgePriorAcc (error 0 - b, information prior I, no robust kernel): one thread of the team
        if (T.gtid == 0) {
            const double *sb = GA(sbias) + ((size_t)buf * A.n_windows + T.w) * 6;
            part += A.prior_g * (sb[0] * sb[0] + sb[1] * sb[1] + sb[2] * sb[2]) + A.prior_a * (sb[3] * sb[3] + sb[4] * sb[4] + sb[5] * sb[5]);
        }
    }
    return part;
}

// One chunk of a free keyframe's visual edges -> partial sums of its 6x6 pose block (lower triangle, 21) and right-hand side (6).
// HALF 0: rows 0..3 of the block (10 entries) + the right-hand side; HALF 1: rows 4, 5 (11 entries): two waves per chunk keep the
// accumulators + the 3x6 Jacobian inside the 128-VGPR budget of a 16-wave workgroup.
template <int HALF>
__device__ __forceinline__ void kf_block_task(const IbaCtx &C, const double *cam, const double *pts, int4 task, double *out)
{
    const IbaWin &W = *gen(C.W); const IbaArgs &A = *gen(C.A);
    constexpr int A0 = HALF ? 4 : 0, A1 = HALF ? 6 : 4, Q0 = HALF ? 10 : 0, NQ = HALF ? 11 : 10, NB = HALF ? 0 : 6;
    const int lane = threadIdx.x & 63;
    const int k = GA(free_kf)[W.free_off + task.x];
    const int *kf_edges = GA(kf_edges) + W.kfe_off;
    double acc[NQ + NB + 1];
#pragma unroll
    for (int i = 0; i < NQ + NB; i++) acc[i] = 0.0;
    for (int j = task.y + lane; j < task.z; j += 64) {
        const size_t ge = (size_t)W.e_off + kf_edges[j];
        const int type = GA(edge_stereo)[ge], st = type == 1;
        const double *c = cam + 24 * k + 12 * (type == 2);
        const double *X = pts + 3 * GA(edge_point)[ge];
        double Xc[3], Jx[9], Jp[18], r0, r1;
        mv3(c, X, Xc); Xc[0] += c[9]; Xc[1] += c[10]; Xc[2] += c[11];
        visual_jac(W, cam_view(W, type == 2), c, Xc, type, Jx, Jp);
        huber(GA(chi2)[ge], st ? C.delta_s : C.delta_m, st ? C.dsqr_s : C.dsqr_m, &r0, &r1);
        const double w = r1 * GA(edge_is2)[ge];
        int q = 0;
#pragma unroll
        for (int a = A0; a < A1; a++)
#pragma unroll
            for (int cc = 0; cc <= a; cc++, q++)
                acc[q] += Jp[a] * w * Jp[cc] + Jp[6 + a] * w * Jp[6 + cc] + Jp[12 + a] * w * Jp[12 + cc];      // row 2 of Jp is zero when mono
        if (!HALF) {
            const double e0 = -w * GA(err)[3 * ge], e1 = -w * GA(err)[3 * ge + 1], e2 = st ? -w * GA(err)[3 * ge + 2] : 0.0;
#pragma unroll
            for (int a = 0; a < 6; a++) acc[NQ + a] += Jp[a] * e0 + Jp[6 + a] * e1 + Jp[12 + a] * e2;
        }
    }
#pragma unroll
    for (int i = 0; i < NQ + NB; i++) acc[i] = wave_sum_f64_dpp(acc[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NQ; i++) out[Q0 + i] = acc[i];
#pragma unroll
        for (int i = 0; i < NB; i++) out[21 + i] = acc[NQ + i];
    }
}

// buildSystem at buffer `buf` from the stored errors.  Team: Hll, bl and the pose-landmark blocks W per landmark; per-chunk partial
// pose blocks; the Omega-weighted inertial Jacobians.  Workgroup 0 then assembles H (dense, both triangles) and b.
template <bool SHARED>
__device__ __noinline__ void iba_build(const IbaCtx &C, Team &T, int buf)
{
    const IbaWin &W = *gen(C.W); const IbaArgs &A = *gen(C.A);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = W.n;
    const double *cam = GA(cam) + buf * A.cam_stride + (size_t)W.kf_off * 24;
    const double *pts = GA(pts) + buf * A.pts_stride + (size_t)W.pt_off * 3;
    const double *kfs = GA(kfs) + buf * A.kfs_stride + (size_t)W.kf_off * IBA_KF;
    double *H = GA(H) + W.h_off, *b = GA(b) + W.x_off;
    const bool bprof = GA(prof) && T.g == 0 && tid == 0;
    long long *bpf = GA(prof) ? GA(prof) + 16 * T.w + 8 : nullptr;
    long long tb = bprof ? clock64() : 0;
#define BPROF(k) do { if (bprof) { const long long t_ = clock64(); bpf[k] += t_ - tb; tb = t_; } } while (0)
    if (T.g == 0) {
        for (int i = tid; i < n * n; i += IBA_THREADS) H[i] = 0.0;
        for (int i = tid; i < n; i += IBA_THREADS) b[i] = 0.0;
    }
    // (1) inertial Jacobians (the last threads of the team, as in iba_errors)
    {
        const int m = T.gsize - 1 - T.gtid;
        if (m < W.M) {
            const size_t gm = (size_t)W.m_off + m;
            double er[9];
            inertial_edge(kfs + IBA_KF * GA(in_kf1)[gm], kfs + IBA_KF * GA(in_kf2)[gm], GA(in_pre) + IBA_PRE * gm, er, GA(Jb) + 216 * gm);
        }
    }
    BPROF(0);
    // (2) landmarks: Hll, bl and the pose-landmark blocks; 8 lanes share a landmark's edges
    const int *pt_start = GA(pt_start) + W.ptstart_off;
    const int sub = tid & 7;
    for (int l0 = (T.gtid >> 3); l0 < ((W.L + 7) & ~7); l0 += (T.gsize >> 3)) {      // whole waves stay in the loop (DPP reductions)
        const int l = min(l0, W.L - 1);
        double h[6] = {0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
        const double *X = pts + 3 * l;
        const int e_end = l0 < W.L ? pt_start[l + 1] : 0;
        for (int e = pt_start[l] + sub; e < e_end; e += 8) {
            const size_t ge = (size_t)W.e_off + e;
            const int type = GA(edge_stereo)[ge], st = type == 1, k = GA(edge_kf)[ge];
            const double *c = cam + 24 * k + 12 * (type == 2);
            double Xc[3], Jx[9], Jp[18], r0, r1;
            mv3(c, X, Xc); Xc[0] += c[9]; Xc[1] += c[10]; Xc[2] += c[11];
            visual_jac(W, cam_view(W, type == 2), c, Xc, type, Jx, Jp);
            huber(GA(chi2)[ge], st ? C.delta_s : C.delta_m, st ? C.dsqr_s : C.dsqr_m, &r0, &r1);
            const double w = r1 * GA(edge_is2)[ge];
            const double es[3] = {-w * GA(err)[3 * ge], -w * GA(err)[3 * ge + 1], st ? -w * GA(err)[3 * ge + 2] : 0.0};
            int q = 0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                bl[a] += Jx[a] * es[0] + Jx[3 + a] * es[1] + Jx[6 + a] * es[2];      // row 2 of Jx is zero when mono
#pragma unroll
                for (int cc = 0; cc <= a; cc++, q++) h[q] += Jx[a] * w * Jx[cc] + Jx[3 + a] * w * Jx[3 + cc] + Jx[6 + a] * w * Jx[6 + cc];
            }
            if (GA(kf_xoff)[W.kf_off + k] >= 0) {
                double *Wd = GA(W) + 18 * ge;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int cc = 0; cc < 3; cc++) Wd[3 * a + cc] = Jp[a] * w * Jx[cc] + Jp[6 + a] * w * Jx[3 + cc] + Jp[12 + a] * w * Jx[6 + cc];
            }
        }
#pragma unroll
        for (int i = 0; i < 6; i++) h[i] = oct_allreduce_f64_dpp(h[i]);
#pragma unroll
        for (int i = 0; i < 3; i++) bl[i] = oct_allreduce_f64_dpp(bl[i]);
        if (sub == 0 && l0 < W.L) {
            double *Hl = GA(Hll) + 6 * ((size_t)W.pt_off + l), *Bl = GA(bl) + 3 * ((size_t)W.pt_off + l);
            for (int i = 0; i < 6; i++) Hl[i] = h[i];
            for (int i = 0; i < 3; i++) Bl[i] = bl[i];
        }
    }
    BPROF(1);
    // (3) per-chunk partial pose blocks, two waves per chunk
    {
        const int4 *kf_task = GA(kf_task) + W.ktask_off;
        double *kpart = GA(kpart) + 27 * (size_t)W.ktask_off;
        for (int t = T.gwave; t < 2 * W.nktask; t += T.gwaves) {
            const int4 task = kf_task[t >> 1];
            if (t & 1) kf_block_task<1>(C, cam, pts, task, kpart + 27 * (size_t)(t >> 1));
            else kf_block_task<0>(C, cam, pts, task, kpart + 27 * (size_t)(t >> 1));
        }
    }
    BPROF(2);
    team_sync(T);                      // Jb, kpart complete
    BPROF(3);
    if (T.g != 0) return;
    BPROF(4);
    // ---- workgroup 0: pose blocks: the chunks of every keyframe summed in order
    {
        const int *kts = GA(kf_task_start) + W.ktstart_off;
        const double *kpart = GA(kpart) + 27 * (size_t)W.ktask_off;
        for (int idx = tid; idx < W.nfree * 27; idx += IBA_THREADS) {
            const int f = idx / 27, q = idx - 27 * f;
            const int o = GA(kf_xoff)[W.kf_off + GA(free_kf)[W.free_off + f]];
            double s = 0;
            for (int t = kts[f]; t < kts[f + 1]; t++) s += kpart[27 * (size_t)t + q];
            if (q >= 21) b[o + q - 21] = s;
            else {
                int a = 0, rem = q;
                while (rem > a) { rem -= a + 1; a++; }          // q -> (a, cc) of the lower triangle
                H[(size_t)(o + a) * n + o + rem] = s; H[(size_t)(o + rem) * n + o + a] = s;
            }
        }
    }
    // what the colour loop needs to know about an edge, fetched for all edges at once (colour, first unknowns of its two keyframes or -1,
    // robust flag): inside the loop these were four dependent L2 round trips per edge
    extern __shared__ double iba_dyn_lds[];
    typedef __attribute__((address_space(3))) int lds_i32;
    lds_i32 *recs = (lds_i32 *)((lds_f64 *)iba_dyn_lds + (size_t)IBA_WAVES * IBA_STAGE);
    for (int m = tid; m < W.M; m += IBA_THREADS) {
        const size_t gm = (size_t)W.m_off + m;
        const int *kx = GA(kf_xoff) + W.kf_off;
        recs[4 * m] = GA(in_color)[gm]; recs[4 * m + 1] = kx[GA(in_kf1)[gm]]; recs[4 * m + 2] = kx[GA(in_kf2)[gm]]; recs[4 * m + 3] = GA(in_robust)[gm];
    }
    __syncthreads();
    BPROF(5);
    // inertial + random-walk edges into H / b: edges of one colour share no keyframe, colours run one after the other.  A wave takes an
    // edge and keeps it in LDS (the solver's panel area is idle during the build): Jacobian, information and error are fetched in ONE
    // round trip, the Omega-weighted copies (Huber weight x information x J, -weight x information x error) are formed in LDS -- round 3
    // wrote them to global memory in a pass of its own, one L2 round trip per output -- and the 24 x 24 products read LDS only; the
    // entries of H a lane updates are read together before and written together after.  Same expressions, same order of sums.
    lds_f64 *sw = (lds_f64 *)iba_dyn_lds + (size_t)wave * IBA_STAGE;      // J [9][24] | Omega J [9][24] at 216 | Omega e [9] at 432 | information [9][9] at 448 | error [15] at 529
    if constexpr (SHARED) {
        // Shared biases: columns 9..14 of every edge's Jacobian belong to the ONE block at n - 6.  Border entries (shared x keyframe)
        // are touched by the edges of that keyframe only, which the colouring keeps apart; the shared 6x6 block and its right-hand
        // side are touched by every edge: each edge stores its part, the parts are summed in edge order afterwards.
        const int os = n - 6;
        double *spart = GA(spart) + 42 * (size_t)W.m_off;
        for (int col = 0; col < W.ncolors; col++) {
            for (int m = 0; m < W.M; m++) {
                const int cr = recs[4 * m];
                if ((cr & 255) != col || ((cr >> 8) % IBA_WAVES) != wave) continue;
                const size_t gm = (size_t)W.m_off + m;
                const int o1 = recs[4 * m + 1], o2 = recs[4 * m + 2];
                const double *Jg = GA(Jb) + 216 * gm, *Ig = GA(in_info) + 81 * gm, *erg = GA(ierr) + 15 * gm;
                double jv[4], iv[2];
#pragma unroll
                for (int t = 0; t < 4; t++) jv[t] = lane + 64 * t < 216 ? Jg[lane + 64 * t] : 0.0;
                iv[0] = Ig[lane]; iv[1] = lane + 64 < 81 ? Ig[lane + 64] : 0.0;
                const double erv = lane < 9 ? erg[lane] : 0.0;
                const double chi_i = GA(ichi2)[3 * gm];
#pragma unroll
                for (int t = 0; t < 4; t++) if (lane + 64 * t < 216) sw[lane + 64 * t] = jv[t];
                sw[448 + lane] = iv[0];
                if (lane + 64 < 81) sw[448 + 64 + lane] = iv[1];
                if (lane < 9) sw[529 + lane] = erv;
                double r0, r1 = 1.0;
                if (recs[4 * m + 3]) huber(chi_i, C.delta_i, C.dsqr_i, &r0, &r1);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (int idx = lane; idx < 216; idx += 64) {
                    const int i = idx / 24, c = idx - i * 24;
                    double s = 0;
                    for (int k = 0; k < 9; k++) s += r1 * sw[448 + 9 * i + k] * sw[24 * k + c];
                    sw[216 + idx] = s;
                }
                if (lane < 9) {
                    double q = 0;
                    for (int k = 0; k < 9; k++) q += sw[448 + 9 * lane + k] * sw[529 + k];
                    sw[432 + lane] = -r1 * q;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // column a of the 9 x 24 Jacobian -> unknown: pose1 + velocity1 | shared biases | pose2 + velocity2; -1 = fixed
                auto col_of = [&](int a) { return a < 9 ? (o1 < 0 ? -1 : o1 + a) : a < 15 ? os + a - 9 : (o2 < 0 ? -1 : o2 + a - 15); };
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    const int idx = lane + 64 * j, a = idx / 24, c = idx - a * 24;
                    double s = 0;
                    for (int k = 0; k < 9; k++) s += sw[24 * k + a] * sw[216 + 24 * k + c];
                    const bool sa = a >= 9 && a < 15, sc = c >= 9 && c < 15;
                    if (sa && sc) spart[42 * (size_t)m + 6 * (a - 9) + (c - 9)] = s;
                    else {
                        const int ga = col_of(a), gc = col_of(c);
                        if (ga >= 0 && gc >= 0) H[(size_t)ga * n + gc] += s;
                    }
                }
                if (lane < 24) {
                    double s = 0;
                    for (int k = 0; k < 9; k++) s += sw[24 * k + lane] * sw[432 + k];
                    if (lane >= 9 && lane < 15) spart[42 * (size_t)m + 36 + lane - 9] = s;
                    else { const int ga = col_of(lane); if (ga >= 0) b[ga] += s; }
                }
                __builtin_amdgcn_wave_barrier();                     // (the next edge of this wave restages sw)
            }
            __syncthreads();
        }
        // the shared block: per-edge parts in edge order, then the two prior edges (J = +I: H += prior I, b += -J^T Omega e = prior b)
        if (tid < 42) {
            double s = 0;
            for (int m = 0; m < W.M; m++) s += spart[42 * (size_t)m + tid];
            const double *sb = GA(sbias) + ((size_t)buf * A.n_windows + T.w) * 6;
            if (tid < 36) {
                const int r = tid / 6, c = tid - 6 * r;
                if (r == c) s += r < 3 ? A.prior_g : A.prior_a;
                H[(size_t)(os + r) * n + os + c] = s;
            } else {
                const int r = tid - 36;
                s += (r < 3 ? A.prior_g : A.prior_a) * sb[r];
                b[os + r] = s;
            }
        }
        __syncthreads();
        BPROF(6);
        return;
    }
    for (int col = 0; col < W.ncolors; col++) {
        for (int m = 0; m < W.M; m++) {                             // (M is small: every wave scans the records, in LDS)
            const int cr = recs[4 * m];
            if ((cr & 255) != col || ((cr >> 8) % IBA_WAVES) != wave) continue;
            const size_t gm = (size_t)W.m_off + m;
            const int o1 = recs[4 * m + 1], o2 = recs[4 * m + 2];
            const double *Jg = GA(Jb) + 216 * gm, *Ig = GA(in_info) + 81 * gm, *erg = GA(ierr) + 15 * gm;
            double jv[4], iv[2];
#pragma unroll
            for (int t = 0; t < 4; t++) jv[t] = lane + 64 * t < 216 ? Jg[lane + 64 * t] : 0.0;
            iv[0] = Ig[lane]; iv[1] = lane + 64 < 81 ? Ig[lane + 64] : 0.0;
            const double erv = lane < 15 ? erg[lane] : 0.0;
            const double chi_i = GA(ichi2)[3 * gm];
            // EdgeGyroRW / EdgeAccRW (G2oTypes.h:648-651, J = [-I, I]): lanes 32..49 = 2 edges x 3 x 3 of H, lanes 50..55 = 2 x 3 of b
            double rwv = 0.0, rw0 = 0.0, rw1 = 0.0, rw2 = 0.0;
            if (lane >= 32 && lane < 50) { const int t = lane - 32, which = t / 9; rwv = ((which ? GA(in_info_a) : GA(in_info_g)) + 9 * gm)[t % 9]; }
            if (lane >= 50 && lane < 56) {
                const int t = lane - 50, which = t / 3, r = t % 3;
                const double *If = (which ? GA(in_info_a) : GA(in_info_g)) + 9 * gm;
                rw0 = If[3 * r]; rw1 = If[3 * r + 1]; rw2 = If[3 * r + 2];
            }
#pragma unroll
            for (int t = 0; t < 4; t++) if (lane + 64 * t < 216) sw[lane + 64 * t] = jv[t];
            sw[448 + lane] = iv[0];
            if (lane + 64 < 81) sw[448 + 64 + lane] = iv[1];
            if (lane < 15) sw[529 + lane] = erv;
            double r0, r1 = 1.0;
            if (recs[4 * m + 3]) huber(chi_i, C.delta_i, C.dsqr_i, &r0, &r1);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int idx = lane; idx < 216; idx += 64) {
                const int i = idx / 24, c = idx - i * 24;
                double s = 0;
                for (int k = 0; k < 9; k++) s += r1 * sw[448 + 9 * i + k] * sw[24 * k + c];
                sw[216 + idx] = s;
            }
            if (lane < 9) {
                double q = 0;
                for (int k = 0; k < 9; k++) q += sw[448 + 9 * lane + k] * sw[529 + k];
                sw[432 + lane] = -r1 * q;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            {
                double hv[9]; size_t ad[9];
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    const int idx = lane + 64 * j, a = idx / 24, c = idx - a * 24;
                    const int ga = a < 15 ? (o1 < 0 ? -1 : o1 + a) : (o2 < 0 ? -1 : o2 + a - 15);
                    const int gc = c < 15 ? (o1 < 0 ? -1 : o1 + c) : (o2 < 0 ? -1 : o2 + c - 15);
                    ad[j] = (ga < 0 || gc < 0) ? (size_t)-1 : (size_t)ga * n + gc;
                    hv[j] = ad[j] != (size_t)-1 ? H[ad[j]] : 0.0;
                }
                // the right-hand side entry of lanes 0..23 and the random-walk entries travel with the same round trip
                const int ba_ = lane < 24 ? (lane < 15 ? (o1 < 0 ? -1 : o1 + lane) : (o2 < 0 ? -1 : o2 + lane - 15)) : -1;
                double bv = ba_ >= 0 ? b[ba_] : 0.0;
                size_t a11 = 0, a22 = 0, a12 = 0, a21 = 0;
                int rb1 = -1, rb2 = -1;
                if (lane >= 32 && lane < 50) {
                    const int t = lane - 32, which = t / 9, r = (t % 9) / 3, c = t % 3, base = which ? 12 : 9;
                    if (o1 >= 0) a11 = (size_t)(o1 + base + r) * n + o1 + base + c;
                    if (o2 >= 0) a22 = (size_t)(o2 + base + r) * n + o2 + base + c;
                    if (o1 >= 0 && o2 >= 0) { a12 = (size_t)(o1 + base + r) * n + o2 + base + c; a21 = (size_t)(o2 + base + r) * n + o1 + base + c; }
                }
                if (lane >= 50 && lane < 56) {
                    const int t = lane - 50, which = t / 3, r = t % 3, base = which ? 12 : 9;
                    if (o1 >= 0) rb1 = o1 + base + r;
                    if (o2 >= 0) rb2 = o2 + base + r;
                }
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    const int idx = lane + 64 * j, a = idx / 24, c = idx - a * 24;
                    double s = 0;
                    for (int k = 0; k < 9; k++) s += sw[24 * k + a] * sw[216 + 24 * k + c];
                    if (ad[j] != (size_t)-1) H[ad[j]] = hv[j] + s;
                }
                if (ba_ >= 0) {
                    double s = 0;
                    for (int k = 0; k < 9; k++) s += sw[24 * k + lane] * sw[432 + k];
                    b[ba_] = bv + s;
                }
                // the random-walk entries are addresses OTHER lanes have just written (blocks 9..14 of both keyframes): those stores are
                // waited for before they are read back (the inertial sums go in first, as in round 3)
                __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0)
                __builtin_amdgcn_wave_barrier();
                if (lane >= 32 && lane < 50) {
                    if (o1 >= 0) H[a11] += rwv;
                    if (o2 >= 0) H[a22] += rwv;
                    if (o1 >= 0 && o2 >= 0) { H[a12] -= rwv; H[a21] -= rwv; }
                }
                if (lane >= 50 && lane < 56) {
                    const int t = lane - 50, which = t / 3;
                    const double v = rw0 * sw[529 + (which ? 12 : 9)] + rw1 * sw[529 + (which ? 12 : 9) + 1] + rw2 * sw[529 + (which ? 12 : 9) + 2];
                    if (rb1 >= 0) b[rb1] += v;                   // J1 = -I: b1 += -J1^T (-Omega e) = +Omega e
                    if (rb2 >= 0) b[rb2] -= v;
                }
            }
            __builtin_amdgcn_wave_barrier();                     // (the next edge of this wave restages sw)
        }
        __syncthreads();
    }
    BPROF(6);
#undef BPROF
}

// One chunk of one keyframe pair's shared landmarks -> partial W_j D^-1 W_i^T (6x6) and, on the diagonal pairs, W_i D^-1 b_l.
// HALF 0: rows 0..2 + the right-hand side, HALF 1: rows 3..5.
template <int HALF>
__device__ __forceinline__ void pair_task(const IbaCtx &C, int4 task, bool diag, double *out)
{
    const IbaWin &W = *gen(C.W); const IbaArgs &A = *gen(C.A);
    const int lane = threadIdx.x & 63;
    const int2 *pair_ent = GA(pair_ent) + W.pent_off;
    constexpr int NB = HALF ? 0 : 6;
    double acc[18 + NB + 1];
#pragma unroll
    for (int q = 0; q < 18 + NB; q++) acc[q] = 0.0;
    // (round 4: entries that also carry their landmark -- one dependent L2 round trip fewer per 64 entries -- took 0.4 % off the kernel and
    // DOUBLED the host packing of a one-shot batch, whose scattered 16-byte stores are its hot loop: 5.2 -> 13.9 ms per 32 windows; undone)
    for (int t = task.y + lane; t < task.z; t += 64) {
        const int2 en = pair_ent[t];
        const size_t gi = (size_t)W.e_off + en.x, gj = (size_t)W.e_off + en.y;
        const size_t gl = (size_t)W.pt_off + GA(edge_point)[gi];
        const double *Wi = GA(W) + 18 * gi, *Wj = GA(W) + 18 * gj + 9 * HALF, *Di = GA(Dinv) + 6 * gl;
        const double d00 = Di[0], d10 = Di[1], d11 = Di[2], d20 = Di[3], d21 = Di[4], d22 = Di[5];
        double wi[18];
#pragma unroll
        for (int q = 0; q < 18; q++) wi[q] = Wi[q];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double w0 = Wj[3 * a], w1 = Wj[3 * a + 1], w2 = Wj[3 * a + 2];
            const double y0 = w0 * d00 + w1 * d10 + w2 * d20, y1 = w0 * d10 + w1 * d11 + w2 * d21, y2 = w0 * d20 + w1 * d21 + w2 * d22;
#pragma unroll
            for (int c = 0; c < 6; c++) acc[6 * a + c] += y0 * wi[3 * c] + y1 * wi[3 * c + 1] + y2 * wi[3 * c + 2];
        }
        if (!HALF && diag && en.x == en.y) {                  // W db once per edge (a keyframe's left / right twin edges also pair with each other)
            const double *db = GA(db) + 3 * gl;
#pragma unroll
            for (int a = 0; a < 6; a++) acc[18 + a] += wi[3 * a] * db[0] + wi[3 * a + 1] * db[1] + wi[3 * a + 2] * db[2];
        }
    }
#pragma unroll
    for (int q = 0; q < 18 + NB; q++) acc[q] = wave_sum_f64_dpp(acc[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 18; q++) out[18 * HALF + q] = acc[q];
#pragma unroll
        for (int q = 0; q < NB; q++) out[36 + q] = acc[18 + q];
    }
}

// One LM trial: (Hll + lambda)^-1, S = H + lambda I - sum W D^-1 W^T, LDL^T, landmark back-substitution, oplus into buffer buf^1.
// Returns (team-uniform) ok of the linear solve; the return value of *scale_part is this THREAD's share of computeScale's sum
// (levenberg.cpp:187-194).
template <bool SHARED>
__device__ __noinline__ bool iba_trial(const IbaCtx &C, Team &T, int buf, double lambda, double *scale_part)
{
    const IbaWin &W = *gen(C.W); const IbaArgs &A = *gen(C.A);
    const long long t_begin = clock64();
    const int tid = threadIdx.x, n = W.n;
    double *H = GA(H) + W.h_off, *S = GA(S) + W.h_off, *b = GA(b) + W.x_off, *bs = GA(bs) + W.x_off, *x = GA(x) + W.x_off;
    const int *pt_start = GA(pt_start) + W.ptstart_off;
    for (int l = (T.gtid >> 3); l < W.L && (tid & 7) == 0; l += (T.gsize >> 3)) {          // the lane that wrote Hll / bl in iba_build
        const size_t gl = (size_t)W.pt_off + l;
        double *Di = GA(Dinv) + 6 * gl, *db = GA(db) + 3 * gl;
        if (pt_start[l + 1] == pt_start[l]) { for (int i = 0; i < 6; i++) Di[i] = 0.0; for (int i = 0; i < 3; i++) db[i] = 0.0; continue; }
        const double *h = GA(Hll) + 6 * gl, *bl = GA(bl) + 3 * gl;
        const double D[9] = {h[0] + lambda, h[1], h[3], h[1], h[2] + lambda, h[4], h[3], h[4], h[5] + lambda};
        double I[9];
        inv3(D, I);
        Di[0] = I[0]; Di[1] = I[3]; Di[2] = I[4]; Di[3] = I[6]; Di[4] = I[7]; Di[5] = I[8];       // lower triangle of the inverse
        mv3(I, bl, db);
    }
    if (T.g == 0) {
        // (four independent loads in flight per thread: one at a time this copy was 44 dependent L2 round trips per trial at n = 150)
        const int nn = n * n;
        for (int i0 = tid; i0 < nn; i0 += 4 * IBA_THREADS) {
            double h[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int i = i0 + u * IBA_THREADS; h[u] = i < nn ? H[i] : 0.0; }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u * IBA_THREADS;
                if (i < nn) { const int r = i / n, c = i - r * n; S[i] = h[u] + (r == c ? lambda : 0.0); }
            }
        }
        for (int i = tid; i < n; i += IBA_THREADS) bs[i] = b[i];
    }
    team_sync(T);
    // Schur complement partials: (pair of free keyframes i <= j, chunk of the landmarks both see), two waves per chunk
    {
        const int4 *ptask = GA(pair_task) + W.ptask_off;
        double *ppart = GA(ppart) + 42 * (size_t)W.ptask_off;
        const int nf = W.nfree;
        for (int t = T.gwave; t < 2 * W.nptask; t += T.gwaves) {
            const int4 task = ptask[t >> 1];
            const bool diag = task.w != 0;
            if (t & 1) pair_task<1>(C, task, diag, ppart + 42 * (size_t)(t >> 1));
            else pair_task<0>(C, task, diag, ppart + 42 * (size_t)(t >> 1));
        }
        (void)nf;
    }
    team_sync(T);
    bool ok = true;
    long long t_schur = 0, t_ldlt = 0;
    if (T.g == 0) {
        // combine: block (j, i) of the lower triangle -= sum of the pair's chunks, in order
        const int *pts_ = GA(pair_task_start) + W.ptstart2_off;
        const double *ppart = GA(ppart) + 42 * (size_t)W.ptask_off;
        const int nf = W.nfree;
        for (int idx = tid; idx < W.npairs * 42; idx += IBA_THREADS) {
            const int p = idx / 42, q = idx - 42 * p;
            if (pts_[p + 1] == pts_[p]) continue;
            int i = 0, rem = p;
            while (rem >= nf - i) { rem -= nf - i; i++; }
            const int j = i + rem;
            if (q >= 36 && i != j) continue;
            double s = 0;
            for (int t = pts_[p]; t < pts_[p + 1]; t++) s += ppart[42 * (size_t)t + q];
            const int oi = GA(kf_xoff)[W.kf_off + GA(free_kf)[W.free_off + i]], oj = GA(kf_xoff)[W.kf_off + GA(free_kf)[W.free_off + j]];
            if (q >= 36) bs[oi + q - 36] -= s;
            else { const int a = q / 6, c = q - 6 * a; S[(size_t)(oj + a) * n + oi + c] -= s; }
        }
        __syncthreads();
        t_schur = clock64();
        ok = n > 0 ? ldlt_solve_wg(S, n, n, bs, x, A.max_n) : true;
        if (tid == 0) GA(okflag)[T.w] = ok ? 1 : 0;
        t_ldlt = clock64();
    }
    team_sync(T);
    ok = GA(okflag)[T.w] != 0;
    const double *cur_pts = GA(pts) + buf * A.pts_stride + (size_t)W.pt_off * 3;
    double *new_pts = GA(pts) + (buf ^ 1) * A.pts_stride + (size_t)W.pt_off * 3;
    double part = 0.0;
    for (int l0 = (T.gtid >> 3); l0 < ((W.L + 7) & ~7); l0 += (T.gsize >> 3)) {      // 8 lanes per landmark, whole waves stay in the loop
        const int l = min(l0, W.L - 1), sub = tid & 7;
        const size_t gl = (size_t)W.pt_off + l;
        double *xl = GA(xl) + 3 * gl;
        const bool active = l0 < W.L && pt_start[l + 1] > pt_start[l];
        double cl[3] = {0, 0, 0};
        if (ok && active) {                                        // block_solver.hpp:461-481 (skipped when the pose solve failed: x stays stale)
            for (int e = pt_start[l] + sub; e < pt_start[l + 1]; e += 8) {
                const size_t ge = (size_t)W.e_off + e;
                const int o = GA(kf_xoff)[W.kf_off + GA(edge_kf)[ge]];
                if (o < 0) continue;
                const double *We = GA(W) + 18 * ge, *xp = x + o;
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int a = 0; a < 6; a++) cl[c] -= We[3 * a + c] * xp[a];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) cl[c] = oct_allreduce_f64_dpp(cl[c]);
        if (sub != 0 || l0 >= W.L) continue;
        if (ok && active) {
            const double *bl = GA(bl) + 3 * gl, *Di = GA(Dinv) + 6 * gl;
            cl[0] += bl[0]; cl[1] += bl[1]; cl[2] += bl[2];
            xl[0] = Di[0] * cl[0] + Di[1] * cl[1] + Di[3] * cl[2];
            xl[1] = Di[1] * cl[0] + Di[2] * cl[1] + Di[4] * cl[2];
            xl[2] = Di[3] * cl[0] + Di[4] * cl[1] + Di[5] * cl[2];
        }
        for (int a = 0; a < 3; a++) {
            const double dx = active ? xl[a] : 0.0;
            new_pts[3 * l + a] = cur_pts[3 * l + a] + dx;
            if (active) part += dx * (lambda * dx + GA(bl)[3 * gl + a]);
        }
    }
    if (T.g == 0) for (int i = tid; i < n; i += IBA_THREADS) part += x[i] * (lambda * x[i] + b[i]);
    // oplus on the keyframe vertices (ImuCamPose::Update, G2oTypes.cc:192-220; the velocity / bias vertices add)
    const double *cur_kf = GA(kfs) + buf * A.kfs_stride + (size_t)W.kf_off * IBA_KF;
    double *new_kf = GA(kfs) + (buf ^ 1) * A.kfs_stride + (size_t)W.kf_off * IBA_KF;
    double *new_cam = GA(cam) + (buf ^ 1) * A.cam_stride + (size_t)W.kf_off * 24;
    for (int k = T.gsize - 1 - T.gtid; k < W.n_kf; k += T.gsize) {
        double s[IBA_KF];
        for (int i = 0; i < IBA_KF; i++) s[i] = cur_kf[IBA_KF * k + i];
        const int o = GA(kf_xoff)[W.kf_off + k];
        if (o >= 0) {
            const double *dx = x + o;
            double t[3], E[9];
            mv3(s + K_R, dx + 3, t);
            for (int i = 0; i < 3; i++) s[K_T + i] += t[i];
            exp_so3(dx, E, 1e-5, true);
            mm3(s + K_R, E, s + K_R);
            if constexpr (SHARED) { if (GA(kf_imu)[W.kf_off + k]) for (int i = 0; i < 3; i++) s[K_V + i] += dx[6 + i]; }
            else if (GA(kf_imu)[W.kf_off + k]) for (int i = 0; i < 9; i++) s[K_V + i] += dx[6 + i];
        }
        if constexpr (SHARED) {
            // every keyframe with IMU states, fixed ones too, carries a copy of the shared biases: EdgeInertial reads them there
            if (GA(kf_imu)[W.kf_off + k]) {
                const double *sb = GA(sbias) + ((size_t)buf * A.n_windows + T.w) * 6;
                for (int i = 0; i < 6; i++) s[K_BG + i] = sb[i] + x[n - 6 + i];
            }
        }
        for (int i = 0; i < IBA_KF; i++) new_kf[IBA_KF * k + i] = s[i];
        cam_pose(W, s, new_cam + 24 * k);
    }
    if constexpr (SHARED) {
        if (T.gtid == 0) {
            const double *sb = GA(sbias) + ((size_t)buf * A.n_windows + T.w) * 6;
            double *sn = GA(sbias) + ((size_t)(buf ^ 1) * A.n_windows + T.w) * 6;
            for (int i = 0; i < 6; i++) sn[i] = sb[i] + x[n - 6 + i];
        }
    }
    team_sync(T);                              // the new estimates are complete
    *scale_part = part;
    if (GA(prof) && T.g == 0 && threadIdx.x == 0) {
        long long *pf = GA(prof) + 16 * T.w;
        pf[2] += t_schur - t_begin; pf[3] += t_ldlt - t_schur; pf[4] += clock64() - t_ldlt;
    }
    return ok;
}
}  // namespace

__global__ __launch_bounds__(IBA_THREADS) void k_iba_solve(const IbaArgs *Ap)      // the argument block sits in global memory: the phase functions read it through a pointer
{
    const IbaArgs &A = *Ap;
    __shared__ double red[2 * IBA_WAVES];
    // blockIdx -> (window, member): with G > 1 the members of a team sit on ONE XCD (workgroups are dealt round-robin over the 8
    // XCDs), so that the team's scratch stays in that XCD's L2; correctness does not depend on it (agent-scope fences)
    int w, g;
    if (A.G == 1) { w = blockIdx.x; g = 0; }
    else { const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3; w = xcd + 8 * (slot / A.G); g = slot % A.G; }
    if (w >= A.n_windows) return;
    const IbaWin &W = GA(win)[w];
    const int tid = threadIdx.x;
    Team T;
    T.w = w; T.g = g; T.G = A.G; T.gtid = g * IBA_THREADS + tid; T.gsize = A.G * IBA_THREADS; T.gwave = g * IBA_WAVES + (tid >> 6); T.gwaves = A.G * IBA_WAVES;
    T.counter = GA(counters) + w; T.epoch = 0; T.wpart = GA(wpart) + (size_t)w * 2 * IBA_MAXG * 2; T.slot = 0; T.fail = GA(fail) + w;
    IbaCtx C;
    C.W = (GPTR(const IbaWin))&W; C.A = (GPTR(const IbaArgs))Ap;
    C.delta_m = (double)sqrtf(5.991f); C.dsqr_m = C.delta_m * C.delta_m;        // thHuberMono etc. are floats (Optimizer.cc:4893-4896)
    C.delta_s = (double)sqrtf(7.815f); C.dsqr_s = C.delta_s * C.delta_s;
    C.delta_i = sqrt(16.92); C.dsqr_i = C.delta_i * C.delta_i;                  // :4838
    int cur = 0;
    {
        const double *kf0 = GA(kfs) + (size_t)W.kf_off * IBA_KF;
        double *cam0 = GA(cam) + (size_t)W.kf_off * 24;
        for (int k = T.gtid; k < W.n_kf; k += T.gsize) cam_pose(W, kf0 + IBA_KF * k, cam0 + 24 * k);
    }
    team_sync(T);
    long long t_err = 0, t_build = 0;
    const long long t_k0 = clock64();
    double chi = iba_errors<false>(C, T, cur), zero = 0.0;        // computeActiveErrors + activeRobustChi2 (:5046-5047)
    team_sum2(T, chi, zero, red);
    t_err += clock64() - t_k0;
    const double err0 = chi;
    double lambda = A.lambda_init, ni = 2.0, last_chi = chi;
    int nbad = 0, trials = 0, its = 0;
    bool errors_current = true;
    for (int it = 0; it < A.iterations; it++) {            // SparseOptimizer::optimize -> OptimizationAlgorithmLevenberg::solve
        long long t0 = clock64();
        // levenberg.cpp:71 computeActiveErrors: after an ACCEPTED trial the stored errors already are those of the current
        // estimate (same inputs, same code: recomputing gives the same bits), only a rejected trial leaves stale ones behind
        if (it > 0 && !errors_current) { chi = iba_errors<false>(C, T, cur); zero = 0.0; team_sum2(T, chi, zero, red); }
        double current_chi = chi;
        const double ini_chi = chi;
        long long t1 = clock64();
        iba_build<false>(C, T, cur);
        t_err += t1 - t0; t_build += clock64() - t1;
        if (it == 0) { lambda = A.lambda_init; ni = 2.0; nbad = 0; }
        double rho = 0.0;
        int qmax = 0;
        do {
            double scale;
            const bool ok = iba_trial<false>(C, T, cur, lambda, &scale);
            t0 = clock64();
            double tmp = iba_errors<false>(C, T, cur ^ 1);
            team_sum2(T, tmp, scale, red);
            t_err += clock64() - t0;
            last_chi = tmp;
            if (!ok) tmp = DBL_MAX;
            rho = (current_chi - tmp) / (scale + 1e-3);
            if (rho > 0 && isfinite(tmp)) {
                double alpha = 1. - pow(2 * rho - 1, 3);
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha); ni = 2.0; current_chi = tmp;
                cur ^= 1;
                errors_current = true; chi = tmp;
            } else {
                lambda *= ni; ni *= 2;
                errors_current = false;
            }
            qmax++; trials++;
        } while (rho < 0 && qmax < A.max_trials && !__hip_atomic_load(T.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        its++;
        if (qmax == A.max_trials || rho == 0 || __hip_atomic_load(T.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        if ((ini_chi - current_chi) * 1e3 < ini_chi) nbad++; else nbad = 0;
        if (nbad >= 3) break;
    }
    // outlier gates on the stored chi2, depth of the final estimates (Optimizer.cc:5056-5088)
    const double *cam = GA(cam) + cur * A.cam_stride + (size_t)W.kf_off * 24;
    const double *pts = GA(pts) + cur * A.pts_stride + (size_t)W.pt_off * 3;
    double nout = 0.0;
    for (int e = T.gtid; e < W.E; e += T.gsize) {
        const size_t ge = (size_t)W.e_off + e;
        const double c2 = GA(chi2)[ge];
        bool out;
        if (GA(edge_stereo)[ge] == 1) out = c2 > (double)7.815f;
        else {
            const double *c = cam + 24 * GA(edge_kf)[ge] + 12 * (GA(edge_stereo)[ge] == 2), *X = pts + 3 * GA(edge_point)[ge];
            const bool depth_pos = (c[6] * X[0] + c[7] * X[1] + c[8] * X[2] + c[11]) > 0.0;
            const bool close = GA(edge_close)[ge] != 0;
            out = (c2 > (double)5.991f && !close) || (c2 > (double)(1.5f * 5.991f) && close) || !depth_pos;
        }
        GA(outlier)[ge] = out ? 1 : 0;
        nout += out ? 1.0 : 0.0;
    }
    zero = 0.0;
    team_sum2(T, nout, zero, red);
    if (cur == 1) {                                         // results are read from buffer 0
        double *k0 = GA(kfs) + (size_t)W.kf_off * IBA_KF, *p0 = GA(pts) + (size_t)W.pt_off * 3;
        const double *k1 = k0 + A.kfs_stride, *p1 = p0 + A.pts_stride;
        for (int i = T.gtid; i < W.n_kf * IBA_KF; i += T.gsize) k0[i] = k1[i];
        for (int i = T.gtid; i < W.L * 3; i += T.gsize) p0[i] = p1[i];
    }
    if (GA(prof) && g == 0 && tid == 0) { long long *pf = GA(prof) + 16 * w; pf[0] = t_err; pf[1] = t_build; pf[5] = clock64() - t_k0; }
    if (g == 0 && tid == 0) {
        orbhip_iba_stats &st = GA(stats)[w];
        st.iterations_run = its; st.lm_trials = trials; st.n_outliers = (int)nout;
        st.err = err0; st.err_end = last_chi;
        const float fe = (float)err0, fl = (float)last_chi;
        st.failed = ((2 * fe < fl || isnan(fe) || isnan(fl)) && !A.large) ? 1 : 0;        // :5096
    }
}

// Optimizer::FullInertialBA's optimize(its) (reference src/Optimizer.cc:420-851): the graph of a whole map through the phase functions
// above.  SHARED (bInit): one gyro / accelerometer bias pair for the map, last in x, with its two prior edges; a keyframe with IMU
// states has 9 unknowns.  !SHARED: the 15-blocks and random-walk edges of the local window.  The LM loop is k_iba_solve's; after it
// there are no outlier gates and no fail check.  One workgroup per map: the shared block's ordered sum runs in workgroup 0 alone.
template <bool SHARED>
__global__ __launch_bounds__(IBA_THREADS) void k_fiba_solve(const IbaArgs *Ap)
{
    const IbaArgs &A = *Ap;
    __shared__ double red[2 * IBA_WAVES];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (w >= A.n_windows) return;
    const IbaWin &W = GA(win)[w];
    Team T;
    T.w = w; T.g = 0; T.G = 1; T.gtid = tid; T.gsize = IBA_THREADS; T.gwave = tid >> 6; T.gwaves = IBA_WAVES;
    T.counter = GA(counters) + w; T.epoch = 0; T.wpart = GA(wpart) + (size_t)w * 2 * IBA_MAXG * 2; T.slot = 0; T.fail = GA(fail) + w;
    IbaCtx C;
    C.W = (GPTR(const IbaWin))&W; C.A = (GPTR(const IbaArgs))Ap;
    C.delta_m = (double)sqrtf(5.991f); C.dsqr_m = C.delta_m * C.delta_m;        // thHuberMono / thHuberStereo are floats (:629-630)
    C.delta_s = (double)sqrtf(7.815f); C.dsqr_s = C.delta_s * C.delta_s;
    C.delta_i = sqrt(16.92); C.dsqr_i = C.delta_i * C.delta_i;                  // :572
    int cur = 0;
    {
        const double *kf0 = GA(kfs) + (size_t)W.kf_off * IBA_KF;
        double *cam0 = GA(cam) + (size_t)W.kf_off * 24;
        for (int k = tid; k < W.n_kf; k += IBA_THREADS) cam_pose(W, kf0 + IBA_KF * k, cam0 + 24 * k);
    }
    team_sync(T);
    double chi = iba_errors<SHARED>(C, T, cur), zero = 0.0;
    team_sum2(T, chi, zero, red);
    const double err0 = chi;
    double lambda = A.lambda_init, ni = 2.0;
    int nbad = 0, trials = 0, its = 0, reason = ORBHIP_FIBA_END_ITERATIONS;
    bool errors_current = true;
    for (int it = 0; it < A.iterations; it++) {            // SparseOptimizer::optimize -> OptimizationAlgorithmLevenberg::solve
        if (it > 0 && !errors_current) { chi = iba_errors<SHARED>(C, T, cur); zero = 0.0; team_sum2(T, chi, zero, red); }
        double current_chi = chi;
        const double ini_chi = chi;
        iba_build<SHARED>(C, T, cur);
        if (it == 0) { lambda = A.lambda_init; ni = 2.0; nbad = 0; }
        double rho = 0.0;
        int qmax = 0;
        do {
            double scale;
            const bool ok = iba_trial<SHARED>(C, T, cur, lambda, &scale);
            double tmp = iba_errors<SHARED>(C, T, cur ^ 1);
            team_sum2(T, tmp, scale, red);
            if (!ok) tmp = DBL_MAX;
            rho = (current_chi - tmp) / (scale + 1e-3);
            if (rho > 0 && isfinite(tmp)) {
                double alpha = 1. - pow(2 * rho - 1, 3);
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha); ni = 2.0; current_chi = tmp;
                cur ^= 1;
                errors_current = true; chi = tmp;
            } else {
                lambda *= ni; ni *= 2;
                errors_current = false;
            }
            qmax++; trials++;
        } while (rho < 0 && qmax < A.max_trials);
        its++;
        if (qmax == A.max_trials || rho == 0) { reason = ORBHIP_FIBA_END_TRIALS; break; }
        if ((ini_chi - current_chi) * 1e3 < ini_chi) nbad++; else nbad = 0;
        if (nbad >= 3) { reason = ORBHIP_FIBA_END_NBAD; break; }
    }
    if (cur == 1) {                                         // results are read from buffer 0
        double *k0 = GA(kfs) + (size_t)W.kf_off * IBA_KF, *p0 = GA(pts) + (size_t)W.pt_off * 3;
        const double *k1 = k0 + A.kfs_stride, *p1 = p0 + A.pts_stride;
        for (int i = tid; i < W.n_kf * IBA_KF; i += IBA_THREADS) k0[i] = k1[i];
        for (int i = tid; i < W.L * 3; i += IBA_THREADS) p0[i] = p1[i];
        if (SHARED && tid < 6) GA(sbias)[(size_t)w * 6 + tid] = GA(sbias)[((size_t)A.n_windows + w) * 6 + tid];
    }
    if (tid == 0) {
        orbhip_fiba_stats &st = GA(fstats)[w];
        st.iterations_run = its; st.lm_trials = trials; st.end_reason = reason; st.n_unknowns = W.n;
        st.chi2_first = err0; st.chi2_last = chi; st.lambda = lambda;
    }
}

// ------------------------------------------------------------------ host side
extern "C" void orbhip_iba_default_params(orbhip_iba_params *p, int large)
{
    if (!p) return;
    p->iterations = large ? 4 : 10;
    p->lambda_init = large ? 1e-2 : 1.0;
    p->large = large ? 1 : 0;
    p->max_trials = 100;
}

namespace {
// One TEAM grid per device at a time.  The team barrier needs every workgroup of the grid resident; the grid is sized for an otherwise
// empty device, so two team grids in flight (two contexts / threads / processes) could each hold compute units the other waits for.
// A solve that wants teams takes this lock without blocking -- an in-process mutex per device plus an advisory file lock for other
// processes of this library -- from launch to completion; a solve that does not get it runs one workgroup per window (G = 1: the
// barrier is a __syncthreads, no residency assumption).  Kernels WITHOUT spin barriers running beside a team grid only delay it: they
// finish on their own and free their compute units (the bounded spin, seconds long, is the last line of defence).
static thread_local int g_iba_last_team = 0;
extern "C" int orbhip_inertial_ba_last_team_size(void) { return g_iba_last_team; }

struct IbaTeamLock {
    int device = -1, fd = -1; bool held = false;
    static std::mutex &mu(int device) { static std::mutex m[64]; return m[device & 63]; }
    bool try_acquire(int dev)
    {
        if (!mu(dev).try_lock()) return false;
        char path[64];
        snprintf(path, sizeof(path), "/tmp/.orbhip_team_gpu%d.lock", dev);
        // flock works on a read-only descriptor, so processes of OTHER users can take part whatever the creator's umask left of the
        // mode (fchmod by the creator widens it to 0666 anyway); O_NOFOLLOW: the name is predictable in a world-writable directory.
        fd = open(path, O_RDONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0666);
        if (fd >= 0) (void)fchmod(fd, 0666);
        else if (errno == EEXIST) fd = open(path, O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
        if (fd < 0) {
            // only a file system that cannot hold the file at all leaves the in-process mutex as the whole lock; anything else
            // (EACCES, ELOOP: somebody else's file / a symlink planted there) means "lock not acquired": the caller runs G = 1
            if (errno == EROFS || errno == ENOENT) { device = dev; held = true; return true; }
            mu(dev).unlock();
            return false;
        }
        if (flock(fd, LOCK_EX | LOCK_NB) != 0) { close(fd); fd = -1; mu(dev).unlock(); return false; }
        device = dev; held = true;
        return true;
    }
    ~IbaTeamLock()
    {
        if (!held) return;
        if (fd >= 0) { flock(fd, LOCK_UN); close(fd); }
        mu(device).unlock();
    }
};
}  // namespace

// A batch of windows resident on the device: the constant part (topology, task lists, preintegrations: everything the host packs) is
// built and uploaded ONCE, a solve only uploads the initial states and launches -- the one-shot entry point below is create + solve +
// download on the context's arena.  (Host packing was 0.5 ms per 13 k-edge window against 60 us of device time.)
struct orbhip_iba_batch {
    orbhip_ctx *ctx;
    int n_windows, max_n;
    bool own;                               // device memory owned by the batch (hipMalloc) or the context's scratch arena (one-shot call)
    uint8_t *d;
    size_t bytes;
    std::vector<IbaWin> hw;
    std::vector<double> kfs, pts;           // initial states, concatenated (host): a solve starts from them
    std::vector<uint8_t> blob;              // host image of the constant part while its upload may still be in flight (one-shot call)
    size_t sumKF, sumL, sumE, sumM, sumX, sumH;
    size_t w_kfs, w_pts, w_xl, w_x, w_W, w_sync, w_stats, w_out, w_prof, w_args;
    size_t w_sbias, w_fstats;               // FullInertialBA
    IbaArgs A;                              // kernel argument, iteration parameters filled per solve
    double pack_ms;
};

static int iba_create_impl(orbhip_ctx *ctx, const orbhip_iba_window *wins, int n_windows, double *const *kf_state_inout, double *const *points_inout,
                           bool own, orbhip_iba_batch **out, int mode = IBA_LOCAL)
{
    const auto t_host0 = std::chrono::steady_clock::now();
    // ---- packing (iba_pack.h): chunks of windows on host threads, then one layout pass
    int nthr = (int)std::thread::hardware_concurrency();
    if (const char *ev = getenv("ORBHIP_IBA_HOST_THREADS")) nthr = atoi(ev);
    nthr = std::max(1, std::min(std::min(nthr, 16), n_windows / 2));
    IbaPacked P;
    const int prc = iba_pack_windows(wins, n_windows, kf_state_inout, points_inout, mode, nthr, P);
    if (prc != ORBHIP_OK) { if (!P.err.empty()) orbhip_set_last_error_internal(P.err.c_str()); return prc; }
    const IbaBlobOffsets &O = P.o;
    const size_t sumKF = P.sumKF, sumL = P.sumL, sumE = P.sumE, sumM = P.sumM, sumX = P.sumX, sumH = P.sumH, n_kftask = P.n_kftask, n_pairtask = P.n_pairtask;
    const size_t constant_bytes = align256(P.blob.size());
    // work area
    size_t off = constant_bytes;
    auto take = [&](size_t bytes) { const size_t o = off; off = align256(off + std::max<size_t>(bytes, 8)); return o; };
    const size_t w_kfs = take(16 * IBA_KF * sumKF), w_cam = take(16 * 24 * sumKF), w_pts = take(16 * 3 * sumL), w_err = take(24 * sumE), w_chi = take(8 * sumE),
                 w_W = take(144 * sumE), w_Hll = take(48 * sumL), w_bl = take(24 * sumL), w_Di = take(48 * sumL), w_db = take(24 * sumL), w_xl = take(24 * sumL),
                 w_ierr = take(120 * sumM), w_ichi = take(24 * sumM), w_Jb = take(1728 * sumM), w_OJ = take(1728 * sumM), w_Oe = take(120 * sumM),
                 w_H = take(8 * sumH), w_S = take(8 * sumH), w_b = take(8 * sumX), w_bs = take(8 * sumX), w_x = take(8 * sumX), w_out = take(sumE),
                 w_kpart = take(27 * 8 * n_kftask), w_ppart = take(42 * 8 * n_pairtask),
                 w_stats = take(sizeof(orbhip_iba_stats) * n_windows), w_prof = take(128 * (size_t)n_windows),
                 w_sync = take((4 + 4 + 4) * (size_t)n_windows), w_wpart = take(8 * 2 * IBA_MAXG * 2 * (size_t)n_windows), w_args = take(sizeof(IbaArgs));
    const bool full = mode != IBA_LOCAL;
    const size_t w_sbias = take(full ? 8 * 2 * 6 * (size_t)n_windows : 0), w_spart = take(full ? 8 * 42 * sumM : 0),
                 w_fstats = take(full ? sizeof(orbhip_fiba_stats) * (size_t)n_windows : 0);
    ORB_HIP_TRY(hipSetDevice(orbhip_ctx_device_internal(ctx)));
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    uint8_t *d = nullptr;
    if (own) { if (hipMalloc((void **)&d, off) != hipSuccess) { orbhip_set_last_error_internal("hipMalloc(inertial BA batch)"); return ORBHIP_E_HIP; } }
    else d = (uint8_t *)orbhip_ctx_scratch_internal(ctx, off);
    if (!d) return ORBHIP_E_HIP;
    orbhip_iba_batch *b = new orbhip_iba_batch();
    b->ctx = ctx; b->n_windows = n_windows; b->own = own; b->d = d; b->bytes = off; b->hw = std::move(P.hw); b->kfs = std::move(P.kfs); b->pts = std::move(P.pts);
    b->sumKF = sumKF; b->sumL = sumL; b->sumE = sumE; b->sumM = sumM; b->sumX = sumX; b->sumH = sumH;
    b->w_kfs = w_kfs; b->w_pts = w_pts; b->w_xl = w_xl; b->w_x = w_x; b->w_W = w_W; b->w_sync = w_sync; b->w_stats = w_stats; b->w_out = w_out; b->w_prof = w_prof; b->w_args = w_args;
    b->w_sbias = w_sbias; b->w_fstats = w_fstats;
    b->max_n = std::max(P.max_n, 32);
    b->blob = std::move(P.blob);                                   // stays alive until the copy has been waited for
    if (hipMemcpyAsync(d, b->blob.data(), b->blob.size(), hipMemcpyHostToDevice, s) != hipSuccess || (own && hipStreamSynchronize(s) != hipSuccess)) {
        if (own) (void)hipFree(d);
        delete b; orbhip_set_last_error_internal("upload of the inertial BA batch"); return ORBHIP_E_HIP;
    }
    if (own) std::vector<uint8_t>().swap(b->blob);                   // a persistent batch keeps no host copy
    IbaArgs &A = b->A;
    memset(&A, 0, sizeof(A));
#define CP(T, o) (GPTR(const T))(d + (o))
#define WP(T, o) (GPTR(T))(d + (o))
    A.win = CP(IbaWin, O.win); A.kf_xoff = CP(int, O.kf_xoff); A.kf_imu = CP(uint8_t, O.kf_imu); A.free_kf = CP(int, O.free_kf);
    A.edge_kf = CP(int, O.edge_kf); A.edge_point = CP(int, O.edge_point); A.edge_obs = CP(double, O.edge_obs); A.edge_is2 = CP(double, O.edge_is2);
    A.edge_stereo = CP(uint8_t, O.edge_stereo); A.edge_close = CP(uint8_t, O.edge_close); A.pt_start = CP(int, O.pt_start);
    A.kf_edges = CP(int, O.kf_edges); A.pair_ent = CP(int2, O.pair_ent); A.kf_task = CP(int4, O.kf_task); A.kf_task_start = CP(int, O.kf_task_start);
    A.pair_task = CP(int4, O.pair_task); A.pair_task_start = CP(int, O.pair_task_start); A.in_kf1 = CP(int, O.in_kf1); A.in_kf2 = CP(int, O.in_kf2);
    A.in_color = CP(int, O.in_color); A.in_robust = CP(uint8_t, O.in_robust); A.in_pre = CP(double, O.in_pre); A.in_info = CP(double, O.in_info);
    A.in_info_g = CP(double, O.in_info_g); A.in_info_a = CP(double, O.in_info_a);
    A.kfs = WP(double, w_kfs); A.cam = WP(double, w_cam); A.pts = WP(double, w_pts);
    A.kfs_stride = (long long)IBA_KF * sumKF; A.cam_stride = 24 * (long long)sumKF; A.pts_stride = 3 * (long long)sumL;
    A.err = WP(double, w_err); A.chi2 = WP(double, w_chi); A.W = WP(double, w_W); A.Hll = WP(double, w_Hll); A.bl = WP(double, w_bl);
    A.Dinv = WP(double, w_Di); A.db = WP(double, w_db); A.xl = WP(double, w_xl); A.ierr = WP(double, w_ierr); A.ichi2 = WP(double, w_ichi);
    A.Jb = WP(double, w_Jb); A.OJ = WP(double, w_OJ); A.Oe = WP(double, w_Oe); A.H = WP(double, w_H); A.S = WP(double, w_S);
    A.b = WP(double, w_b); A.bs = WP(double, w_bs); A.x = WP(double, w_x); A.outlier = WP(uint8_t, w_out); A.stats = WP(orbhip_iba_stats, w_stats);
    A.kpart = WP(double, w_kpart); A.ppart = WP(double, w_ppart);
    A.counters = WP(unsigned, w_sync); A.fail = WP(int, w_sync + 4 * (size_t)n_windows); A.okflag = WP(int, w_sync + 8 * (size_t)n_windows);
    A.wpart = WP(double, w_wpart);
    if (full) { A.sbias = WP(double, w_sbias); A.spart = WP(double, w_spart); A.fstats = WP(orbhip_fiba_stats, w_fstats); }
#undef CP
#undef WP
    A.max_n = b->max_n;
    A.n_windows = n_windows;
    b->pack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    *out = b;
    return ORBHIP_OK;
}

static void iba_destroy_impl(orbhip_iba_batch *b)
{
    if (!b) return;
    if (b->own && b->d) { (void)hipStreamSynchronize(orbhip_ctx_stream_internal(b->ctx)); (void)hipFree(b->d); }
    delete b;
}

static int iba_solve_impl(orbhip_iba_batch *b, const orbhip_iba_params *params)
{
    orbhip_ctx *ctx = b->ctx;
    const int n_windows = b->n_windows;
    uint8_t *d = b->d;
    const size_t sumL = b->sumL, sumE = b->sumE, sumX = b->sumX;
    const bool want_prof = getenv("ORBHIP_IBA_PROF") != nullptr;
    const auto t_host1 = std::chrono::steady_clock::now();
    ORB_HIP_TRY(hipSetDevice(orbhip_ctx_device_internal(ctx)));
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    ORB_HIP_TRY(hipMemcpyAsync(d + b->w_kfs, b->kfs.data(), 8 * b->kfs.size(), hipMemcpyHostToDevice, s));
    if (!b->pts.empty()) ORB_HIP_TRY(hipMemcpyAsync(d + b->w_pts, b->pts.data(), 8 * b->pts.size(), hipMemcpyHostToDevice, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_xl, 0, 24 * sumL + 8, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_x, 0, 8 * sumX + 8, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_W, 0, 144 * sumE + 8, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_sync, 0, 12 * (size_t)n_windows, s));
    IbaArgs A = b->A;
    if (want_prof) { ORB_HIP_TRY(hipMemsetAsync(d + b->w_prof, 0, 128 * (size_t)n_windows, s)); A.prof = (GPTR(long long))(d + b->w_prof); }
    A.iterations = params->iterations; A.max_trials = params->max_trials; A.large = params->large; A.lambda_init = params->lambda_init;
    const int device = orbhip_ctx_device_internal(ctx);
    const size_t lds = std::max(ba_ldlt_lds_bytes(A.max_n), sizeof(double) * (size_t)IBA_WAVES * IBA_STAGE + 16 * (size_t)IBA_THREADS);      // the solver's panel area; the build stages inertial edges (and their records) in it
    if (orb_lds_optin((const void *)k_iba_solve, device, lds) != 0) return ORBHIP_E_HIP;
    // team size: every workgroup of a team must be resident (the barrier spins), so teams are only used while the whole grid fits
    // the device at one 512-thread workgroup per CU; bigger batches run one workgroup per window
    int cus = 0, per_cu = 0;
    ORB_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    ORB_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_iba_solve, IBA_THREADS, lds));
    const int forced = getenv("ORBHIP_IBA_TEAM") ? atoi(getenv("ORBHIP_IBA_TEAM")) : 0;
    const int slots_per_xcd = std::max(1, (cus / 8) * std::min(per_cu, 1));          // co-resident workgroups per XCD we rely on
    const int win_per_xcd = (n_windows + 7) / 8;
    int G = std::min(IBA_MAXG, slots_per_xcd / win_per_xcd);
    if (forced > 0) G = std::min(forced, G);
    if (G < 2 || per_cu < 1) G = 1;
    IbaTeamLock team_lock;                                           // released when this (synchronous) call returns
    if (G > 1 && !team_lock.try_acquire(device)) G = 1;              // another team grid is in flight on this device
    A.G = G;
    g_iba_last_team = G;
    // the argument block goes to the device (the kernel's phase functions read it through a global pointer; a by-value kernel argument
    // whose address is taken is copied to scratch by every thread)
    const IbaArgs *d_args = reinterpret_cast<const IbaArgs *>(d + b->w_args);
    ORB_HIP_TRY(hipMemcpyAsync(d + b->w_args, &A, sizeof(IbaArgs), hipMemcpyHostToDevice, s));
    if (G == 1) {
        hipLaunchKernelGGL(k_iba_solve, dim3(n_windows), dim3(IBA_THREADS), lds, s, d_args);
        ORB_HIP_TRY(hipGetLastError());
    } else {
        // the whole grid must be resident (the team barrier spins): a plain launch has the same residency as a cooperative one
        // (MI355X_MICROARCH.md), so the size rule is checked here instead of by hipLaunchCooperativeKernel (whose launches rocprofv3
        // cannot trace without crashing in the runtime's exit handler on this image: profiles/r03_iba_coop_exit_crash.txt)
        if (8 * G * win_per_xcd > cus * per_cu) { orbhip_set_last_error_internal("inertial BA: team grid larger than the device"); return ORBHIP_E_HIP; }
        hipLaunchKernelGGL(k_iba_solve, dim3(8 * G * win_per_xcd), dim3(IBA_THREADS), lds, s, d_args);
        ORB_HIP_TRY(hipGetLastError());
    }
    std::vector<int> failv(n_windows);
    ORB_HIP_TRY(hipMemcpyAsync(failv.data(), d + b->w_sync + 4 * (size_t)n_windows, 4 * (size_t)n_windows, hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));
    for (int w = 0; w < n_windows; w++)
        if (failv[w]) { orbhip_set_last_error_internal("inertial BA: a team barrier did not complete (workgroups not co-resident)"); return ORBHIP_E_HIP; }
#ifdef LDLT_PROF
    {
        long long lp[8];
        ORB_HIP_TRY(hipMemcpyFromSymbol(lp, HIP_SYMBOL(g_ldlt_prof), sizeof(lp)));
        fprintf(stderr, "[orbhip iba] LDLT cycles (cumulative): load %lld diag %lld rows %lld trailing %lld backsub %lld\n", lp[0], lp[1], lp[2], lp[3], lp[4]);
    }
#endif
    if (want_prof) {
        const auto t_host2 = std::chrono::steady_clock::now();
        fprintf(stderr, "[orbhip iba] %d windows: host packing %.3f ms (at creation), state upload + kernel %.3f ms (%zu B on the device)\n", n_windows, b->pack_ms,
                std::chrono::duration<double, std::milli>(t_host2 - t_host1).count(), b->bytes);
        long long pf[16];
        ORB_HIP_TRY(hipMemcpy(pf, d + b->w_prof, 128, hipMemcpyDeviceToHost));
        fprintf(stderr, "[orbhip iba] build phases (workgroup 0, cycles): inertial Jacobians %lld, landmarks %lld, pose chunks %lld, team barrier %lld, Omega J %lld, pose blocks %lld, colours %lld\n",
                pf[8], pf[9], pf[10], pf[11], pf[12], pf[13], pf[14]);
        fprintf(stderr, "[orbhip iba] G=%d window 0 shader cycles: errors %lld, build %lld, prep+schur %lld, ldlt %lld, update %lld, total %lld\n", G, pf[0], pf[1], pf[2], pf[3], pf[4], pf[5]);
    }
    return ORBHIP_OK;
}

static int iba_download_impl(orbhip_iba_batch *b, double *const *kf_state_out, double *const *points_out, uint8_t *const *edge_outlier_out,
                             orbhip_iba_stats *stats_out)
{
    const int n_windows = b->n_windows;
    uint8_t *d = b->d;
    hipStream_t s = orbhip_ctx_stream_internal(b->ctx);
    ORB_HIP_TRY(hipSetDevice(orbhip_ctx_device_internal(b->ctx)));
    std::vector<orbhip_iba_stats> st(n_windows);
    std::vector<double> kfo((size_t)IBA_KF * b->sumKF), pto(3 * b->sumL);
    std::vector<uint8_t> outl(b->sumE);
    ORB_HIP_TRY(hipMemcpyAsync(st.data(), d + b->w_stats, sizeof(orbhip_iba_stats) * n_windows, hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipMemcpyAsync(kfo.data(), d + b->w_kfs, 8 * kfo.size(), hipMemcpyDeviceToHost, s));
    if (b->sumL) ORB_HIP_TRY(hipMemcpyAsync(pto.data(), d + b->w_pts, 8 * pto.size(), hipMemcpyDeviceToHost, s));
    if (b->sumE) ORB_HIP_TRY(hipMemcpyAsync(outl.data(), d + b->w_out, b->sumE, hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));
    for (int w = 0; w < n_windows; w++) {
        const IbaWin &W = b->hw[w];
        if (!st[w].failed) {                               // "FAIL LOCAL-INERTIAL BA": the reference returns before any write-back (Optimizer.cc:5096-5100)
            if (kf_state_out && kf_state_out[w]) memcpy(kf_state_out[w], kfo.data() + (size_t)W.kf_off * IBA_KF, 8 * (size_t)IBA_KF * W.n_kf);
            if (W.L && points_out && points_out[w]) memcpy(points_out[w], pto.data() + (size_t)W.pt_off * 3, 24 * (size_t)W.L);
        }
        if (edge_outlier_out && edge_outlier_out[w] && W.E) memcpy(edge_outlier_out[w], outl.data() + W.e_off, W.E);
        if (stats_out) stats_out[w] = st[w];
    }
    return ORBHIP_OK;
}

static bool iba_params_ok(const orbhip_iba_params *p) { return p && p->iterations >= 0 && p->max_trials >= 1 && p->lambda_init > 0; }

extern "C" int orbhip_inertial_ba_solve_batch(orbhip_ctx *ctx, const orbhip_iba_window *wins, int n_windows, const orbhip_iba_params *params,
                                              double *const *kf_state_inout, double *const *points_inout, uint8_t *const *edge_outlier_out,
                                              orbhip_iba_stats *stats_out)
{
    if (!ctx || n_windows < 0 || (n_windows && (!wins || !kf_state_inout || !points_inout)) || !params) return ORBHIP_E_BADARG;
    if (n_windows == 0) return ORBHIP_OK;
    if (!iba_params_ok(params)) return ORBHIP_E_BADARG;
    orbhip_iba_batch *b = nullptr;
    int rc = iba_create_impl(ctx, wins, n_windows, kf_state_inout, points_inout, false, &b);
    if (rc != ORBHIP_OK) return rc;
    rc = iba_solve_impl(b, params);
    if (rc == ORBHIP_OK) rc = iba_download_impl(b, kf_state_inout, points_inout, edge_outlier_out, stats_out);
    iba_destroy_impl(b);
    return rc;
}

extern "C" int orbhip_iba_batch_create(orbhip_ctx *ctx, const orbhip_iba_window *wins, int n_windows, double *const *kf_states, double *const *points,
                                       orbhip_iba_batch **out)
{
    if (!ctx || n_windows <= 0 || !wins || !kf_states || !points || !out) return ORBHIP_E_BADARG;
    return iba_create_impl(ctx, wins, n_windows, kf_states, points, true, out);
}
extern "C" int orbhip_iba_batch_set_states(orbhip_iba_batch *b, double *const *kf_states, double *const *points)
{
    if (!b || !kf_states || !points) return ORBHIP_E_BADARG;
    for (int w = 0; w < b->n_windows; w++) {
        const IbaWin &W = b->hw[w];
        if (!kf_states[w] || (W.L && !points[w])) return ORBHIP_E_BADARG;
        memcpy(b->kfs.data() + (size_t)W.kf_off * IBA_KF, kf_states[w], 8 * (size_t)IBA_KF * W.n_kf);
        if (W.L) memcpy(b->pts.data() + (size_t)W.pt_off * 3, points[w], 24 * (size_t)W.L);
    }
    return ORBHIP_OK;
}
extern "C" int orbhip_iba_batch_solve(orbhip_iba_batch *b, const orbhip_iba_params *params)
{
    if (!b || !iba_params_ok(params)) return ORBHIP_E_BADARG;
    return iba_solve_impl(b, params);
}
extern "C" int orbhip_iba_batch_download(orbhip_iba_batch *b, double *const *kf_states_out, double *const *points_out, uint8_t *const *edge_outlier_out,
                                         orbhip_iba_stats *stats_out)
{
    if (!b) return ORBHIP_E_BADARG;
    return iba_download_impl(b, kf_states_out, points_out, edge_outlier_out, stats_out);
}
extern "C" void orbhip_iba_batch_destroy(orbhip_iba_batch *b) { iba_destroy_impl(b); }

// ================================================================== full inertial BA
extern "C" void orbhip_fiba_default_params(orbhip_fiba_params *p, int its, int bInit, double priorG, double priorA)
{
    if (!p) return;
    p->iterations = its;
    p->lambda_init = 1e-5;                   // setUserLambdaInit(1e-5), Optimizer.cc:435
    p->max_trials = 100;
    p->shared_bias = bInit ? 1 : 0;
    p->prior_g = priorG; p->prior_a = priorA;
}

extern "C" int orbhip_full_inertial_ba_solve_batch(orbhip_ctx *ctx, const orbhip_iba_window *maps, int n_maps, const orbhip_fiba_params *params,
                                                   const volatile uint8_t *stop, double *const *kf_state_inout, double *const *points_inout,
                                                   double *shared_bias_inout, orbhip_fiba_stats *stats_out)
{
    if (!ctx || n_maps < 0 || (n_maps && (!maps || !kf_state_inout || !points_inout)) || !params) return ORBHIP_E_BADARG;
    if (params->iterations < 0 || params->max_trials < 1 || !(params->lambda_init > 0) || !(params->prior_g >= 0) || !(params->prior_a >= 0)) {
        orbhip_set_last_error_internal("full inertial BA: iterations < 0, max_trials < 1, lambda_init <= 0 or a negative prior");
        return ORBHIP_E_BADARG;
    }
    const bool shared = params->shared_bias != 0;
    if (shared && n_maps && !shared_bias_inout) { orbhip_set_last_error_internal("full inertial BA: shared_bias_inout is NULL"); return ORBHIP_E_BADARG; }
    if (stop && *stop) return ORBHIP_E_ABORTED;                  // Optimizer.cc:758-760
    // maps that hold something, filtered
    std::vector<int> idx;
    for (int m = 0; m < n_maps; m++) {
        if (maps[m].n_kf == 0) { if (stats_out) memset(&stats_out[m], 0, sizeof(orbhip_fiba_stats)); continue; }
        idx.push_back(m);
    }
    const int nm = (int)idx.size();
    if (nm == 0) return ORBHIP_OK;
    std::vector<FibaMap> F(nm);
    std::vector<orbhip_iba_window> wins(nm);
    std::vector<std::vector<double>> kf0(nm);
    std::vector<double *> kfp(nm), ptp(nm);
    for (int i = 0; i < nm; i++) {
        const orbhip_iba_window &g = maps[idx[i]];
        if (!kf_state_inout[idx[i]] || (g.n_points > 0 && !points_inout[idx[i]])) return ORBHIP_E_BADARG;
        const int rc = fiba_filter(g, shared, F[i], wins[i]);
        if (rc != ORBHIP_OK) return rc;
        kf0[i].assign(kf_state_inout[idx[i]], kf_state_inout[idx[i]] + (size_t)IBA_KF * g.n_kf);
        if (shared)                                              // every keyframe with IMU states carries a copy of the shared biases
            for (int k = 0; k < g.n_kf; k++)
                if (g.kf_imu[k]) memcpy(kf0[i].data() + (size_t)IBA_KF * k + K_BG, shared_bias_inout + 6 * (size_t)idx[i], 48);
        kfp[i] = kf0[i].data(); ptp[i] = points_inout[idx[i]];
    }
    orbhip_iba_batch *b = nullptr;
    int rc = iba_create_impl(ctx, wins.data(), nm, kfp.data(), ptp.data(), false, &b, shared ? IBA_FULL_SHARED : IBA_FULL);
    if (rc != ORBHIP_OK) return rc;
    struct Guard { orbhip_iba_batch *b; ~Guard() { iba_destroy_impl(b); } } guard{b};
    uint8_t *d = b->d;
    ORB_HIP_TRY(hipSetDevice(orbhip_ctx_device_internal(ctx)));
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    ORB_HIP_TRY(hipMemcpyAsync(d + b->w_kfs, b->kfs.data(), 8 * b->kfs.size(), hipMemcpyHostToDevice, s));
    if (!b->pts.empty()) ORB_HIP_TRY(hipMemcpyAsync(d + b->w_pts, b->pts.data(), 8 * b->pts.size(), hipMemcpyHostToDevice, s));
    std::vector<double> sb(12 * (size_t)nm, 0.0);
    if (shared) for (int i = 0; i < nm; i++) memcpy(sb.data() + 6 * (size_t)i, shared_bias_inout + 6 * (size_t)idx[i], 48);
    ORB_HIP_TRY(hipMemcpyAsync(d + b->w_sbias, sb.data(), 8 * sb.size(), hipMemcpyHostToDevice, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_xl, 0, 24 * b->sumL + 8, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_x, 0, 8 * b->sumX + 8, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_W, 0, 144 * b->sumE + 8, s));
    ORB_HIP_TRY(hipMemsetAsync(d + b->w_sync, 0, 12 * (size_t)nm, s));
    IbaArgs A = b->A;
    A.iterations = params->iterations; A.max_trials = params->max_trials; A.large = 1; A.lambda_init = params->lambda_init;
    A.prior_g = shared ? params->prior_g : 0.0; A.prior_a = shared ? params->prior_a : 0.0;
    A.G = 1;
    const int device = orbhip_ctx_device_internal(ctx);
    const size_t lds = std::max(ba_ldlt_lds_bytes(A.max_n), sizeof(double) * (size_t)IBA_WAVES * IBA_STAGE + 16 * (size_t)IBA_THREADS);
    const void *kern = shared ? (const void *)k_fiba_solve<true> : (const void *)k_fiba_solve<false>;
    if (orb_lds_optin(kern, device, lds) != 0) return ORBHIP_E_HIP;
    const IbaArgs *d_args = reinterpret_cast<const IbaArgs *>(d + b->w_args);
    ORB_HIP_TRY(hipMemcpyAsync(d + b->w_args, &A, sizeof(IbaArgs), hipMemcpyHostToDevice, s));
    if (shared) hipLaunchKernelGGL(k_fiba_solve<true>, dim3(nm), dim3(IBA_THREADS), lds, s, d_args);
    else hipLaunchKernelGGL(k_fiba_solve<false>, dim3(nm), dim3(IBA_THREADS), lds, s, d_args);
    ORB_HIP_TRY(hipGetLastError());
    std::vector<orbhip_fiba_stats> st(nm);
    std::vector<double> kfo((size_t)IBA_KF * b->sumKF), pto(3 * b->sumL);
    ORB_HIP_TRY(hipMemcpyAsync(st.data(), d + b->w_fstats, sizeof(orbhip_fiba_stats) * nm, hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipMemcpyAsync(kfo.data(), d + b->w_kfs, 8 * kfo.size(), hipMemcpyDeviceToHost, s));
    if (b->sumL) ORB_HIP_TRY(hipMemcpyAsync(pto.data(), d + b->w_pts, 8 * pto.size(), hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipMemcpyAsync(sb.data(), d + b->w_sbias, 8 * 6 * (size_t)nm, hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < nm; i++) {
        const IbaWin &W = b->hw[i];
        memcpy(kf_state_inout[idx[i]], kfo.data() + (size_t)W.kf_off * IBA_KF, 8 * (size_t)IBA_KF * W.n_kf);
        if (W.L) memcpy(points_inout[idx[i]], pto.data() + (size_t)W.pt_off * 3, 24 * (size_t)W.L);
        if (shared) memcpy(shared_bias_inout + 6 * (size_t)idx[i], sb.data() + 6 * (size_t)i, 48);
        if (stats_out) stats_out[idx[i]] = st[i];
    }
    return ORBHIP_OK;
}

// ================================================================== inertial pose-only optimisation
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
    exp_so3(dx, E, 1e-5, true);
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
            log_so3(RR, er);
            double d[3] = {L.p[K_T] - pr[K_T], L.p[K_T + 1] - pr[K_T + 1], L.p[K_T + 2] - pr[K_T + 2]}, et[3];
            mtv3(pr + K_R, d, et);
            inv_right_jac(er, IJ);
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
