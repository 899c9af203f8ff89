// iba_kernels.hip -- Optimizer::LocalInertialBA's numerical core on gfx950 (reference src/Optimizer.cc:4574-5187; vertices and
// edges include/G2oTypes.h + src/G2oTypes.cc: ImuCamPose :25-220, EdgeMono / EdgeStereo :349-482, EdgeInertial :693-800,
// EdgeGyroRW / EdgeAccRW G2oTypes.h:632-700; bias-corrected preintegration src/ImuTypes.cc:351-378; g2o Levenberg-Marquardt
// with the landmark Schur complement as in the local BA, ba_kernels.hip and its device files).
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
#include "iba_pack.h"          // IbaWin, the IBA_* sizes and modes, and the host packing (HIP-free)
#include "iba_edges.h"         // the cameras, the visual edges and EdgeInertial (+ geom3.h, so3_f64.h, ba_camera.h, imu_layout.h)
// The library is built with -ffp-contract=off for the bit-exact integer / float ORB paths.  The double-precision optimisers are
// compared with the oracle to 1e-4, not bit for bit: let a * b + c contract to v_fma_f64 here (half the FP64 instructions).
#pragma clang fp contract(fast)
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <thread>              // hardware_concurrency (the packing threads themselves: iba_pack.h)
#include <mutex>               // IbaTeamLock, as the five below
#include <fcntl.h>
#include <errno.h>
#include <unistd.h>
#include <sys/file.h>
#include <sys/stat.h>

#define IBA_WAVES (IBA_THREADS / 64)
#define IBA_STAGE 544          // doubles of LDS a wave of workgroup 0 stages an inertial edge in (9 x 24 Jacobian, its Omega-weighted copy, Omega e at 432, the 9 x 9 information at 448)
#define IBA_MAXG 32

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
namespace {
// EdgeInertial out of line, as the BA kernels call it (iba_edges.h has the body; 3x3 products and huber: geom3.h, SO(3): so3_f64.h)
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
        so3_inv3(D, I);
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
            so3_exp(dx, E, 1e-5, true);
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
