// preint_kernels.hip -- IMU::Preintegrated on the device: Initialize / IntegrateNewMeasurement (src/ImuTypes.cc:225-310) for a batch of
// independent chains, and the edge information the inertial optimisers take from the covariance.  The arithmetic is csrc/preint_core.h
// (float throughout, the reference's update order); this file holds how it is spread over the machine, in two forms chosen by the
// number of chains:
//   k_preint_lane  one lane per chain, the whole state (45 Jacobian entries, 81 covariance entries, 22 others) in registers, the
//                  measurements streamed from the chain's running offset: a map-wide Reintegrate of tens to hundreds of chains.
//   k_preint_wave  one wave per chain, for the few-chain calls whose length is a latency chain.  64 measurements at a time: (A) each
//                  lane takes one measurement: acc, accW, deltaR, rightJ dt, into LDS; (B) the rotation chain dR_k, which nothing can
//                  shorten, runs alone (every lane carries a copy, lane 0 files dR_k); (C) each lane takes one measurement again and
//                  builds, from dR_k, the blocks F, G, dR dt, 0.5 dR dt^2, dR acc and the 81 entries of B Nga B^T; (D) the recursion:
//                  lanes 0-8 hold one row of C each (two products with A and a transposition through LDS per step), lanes 9-11 a column
//                  of (JRg; JVg; JPg), lanes 12-14 a column of (0; JVa; JPa) (one product), lanes 16-51 one entry of the walk block;
//                  dT, dV, dP, avgA, avgW are carried by every lane.  Per step the serial path is two 33-multiply products and one LDS
//                  round trip instead of the lane form's 24 products, 9 noise rows and the trigonometry.
// Both forms run the same functions on the same values in the same order; the compiler contracts multiply-adds differently in the two
// kernels, so their results differ in last bits.  What is promised (and tested) is byte equality within one form: of reruns, and of a
// continued chain with the chain integrated in one go.
//   k_preint_info  one lane per chain, in double: optc::inertial_information (host/Optimizer_LocalInertialBA.cc:57-74: symmetrise, cyclic
//                  Jacobi, drop eigenvalues <= 9e-7 wmax, clamp inverses below 1e-12, reassemble) and the two inv3_block of the walk
//                  block, rounded through float.  Every rotation is unrolled: A and V (162 doubles) stay in registers.
#include "orb_internal.h"
#include "ctx_internal.h"
#include "imu_layout.h"
#include "preint_core.h"
#include "wave_dpp.h"
#include <cstring>
#include <vector>

namespace {

struct PreintArgs {
    const int32_t *meas_off; const float *meas; const uint8_t *cont;
    double *record; float *cov, *avg;
    int chains;
    float nga[36], walk[36];
};

__device__ __forceinline__ void load_bias(const double *rec, float *bg, float *ba)
{
#pragma unroll
    for (int i = 0; i < 3; i++) { bg[i] = (float)rec[P_BG + i]; ba[i] = (float)rec[P_BA + i]; }
}

// ---------------------------------------------------------------------------------------------------------------- lane form
__global__ __launch_bounds__(64) void k_preint_lane(const PreintArgs a)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= a.chains) return;
    const int m0 = a.meas_off[ch], n = a.meas_off[ch + 1] - m0;
    const bool cont = a.cont && a.cont[ch];
    double *rec = a.record + (size_t)ORBHIP_IBA_PREINT * ch;
    float *cov = a.cov + (size_t)225 * ch, *avg = a.avg + (size_t)6 * ch;
    float bg[3], ba[3];
    load_bias(rec, bg, ba);
    PreintState S;
    preint_initialize(S);
    if (cont) {
        S.dT = (float)rec[P_DT];
#pragma unroll
        for (int i = 0; i < 9; i++) S.dR[i] = (float)rec[P_DR + i];
#pragma unroll
        for (int i = 0; i < 3; i++) { S.dV[i] = (float)rec[P_DV + i]; S.dP[i] = (float)rec[P_DP + i]; S.avgA[i] = avg[i]; S.avgW[i] = avg[3 + i]; }
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                S.Jg[j][i] = (float)rec[P_JRG + 3 * i + j]; S.Jg[j][3 + i] = (float)rec[P_JVG + 3 * i + j]; S.Jg[j][6 + i] = (float)rec[P_JPG + 3 * i + j];
                S.Ja[j][3 + i] = (float)rec[P_JVA + 3 * i + j]; S.Ja[j][6 + i] = (float)rec[P_JPA + 3 * i + j];
            }
#pragma unroll
        for (int c = 0; c < 9; c++)
#pragma unroll
            for (int r = 0; r < 9; r++) S.C[c][r] = cov[15 * c + r];
    }
    const float *m = a.meas + (size_t)7 * m0;
    for (int k = 0; k < n; k++, m += 7) {
        float mk[7];
#pragma unroll
        for (int i = 0; i < 7; i++) mk[i] = m[i];
        preint_step(S, bg, ba, mk, a.nga);
    }
    rec[P_DT] = (double)S.dT;
#pragma unroll
    for (int i = 0; i < 9; i++) rec[P_DR + i] = (double)S.dR[i];
#pragma unroll
    for (int i = 0; i < 3; i++) { rec[P_DV + i] = (double)S.dV[i]; rec[P_DP + i] = (double)S.dP[i]; avg[i] = S.avgA[i]; avg[3 + i] = S.avgW[i]; }
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            rec[P_JRG + 3 * i + j] = (double)S.Jg[j][i]; rec[P_JVG + 3 * i + j] = (double)S.Jg[j][3 + i]; rec[P_JPG + 3 * i + j] = (double)S.Jg[j][6 + i];
            rec[P_JVA + 3 * i + j] = (double)S.Ja[j][3 + i]; rec[P_JPA + 3 * i + j] = (double)S.Ja[j][6 + i];
        }
#pragma unroll
    for (int c = 0; c < 9; c++) {
#pragma unroll
        for (int r = 0; r < 9; r++) cov[15 * c + r] = S.C[c][r];
#pragma unroll
        for (int j = 9; j < 15; j++) { cov[15 * c + j] = 0.f; cov[15 * j + c] = 0.f; }
    }
    // C(9:15, 9:15) += NgaWalk per measurement (:303): a plain add, kept out of the loop above to keep its registers free
    for (int e = 0; e < 36; e++) {
        float *p = cov + 15 * (9 + e / 6) + 9 + e % 6;
        float v = cont ? *p : 0.f;
        const float w = a.walk[e];
        for (int k = 0; k < n; k++) v += w;
        *p = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- wave form
enum { S_ACC = 0, S_ACCW = 3, S_DT = 6, S_E = 7, S_JDT = 16, S_DR = 25, S_F = 34, S_G = 43, S_B2 = 52, S_B3 = 61, S_RACC = 70, S_Q = 73,
       S_STRIDE = 155 };        // floats per measurement; the odd stride spreads the lanes of phases A and C over the banks

__global__ __launch_bounds__(64) void k_preint_wave(const PreintArgs a)
{
    __shared__ float slot[64 * S_STRIDE];
    __shared__ float tr[81];
    const int ch = blockIdx.x, lane = threadIdx.x;
    const int m0 = a.meas_off[ch], n = a.meas_off[ch + 1] - m0;
    const bool cont = a.cont && a.cont[ch];
    double *rec = a.record + (size_t)ORBHIP_IBA_PREINT * ch;
    float *cov = a.cov + (size_t)225 * ch, *avg = a.avg + (size_t)6 * ch;
    float bg[3], ba[3];
    load_bias(rec, bg, ba);
    const bool isC = lane < 9, isG = lane >= 9 && lane < 12, isA = lane >= 12 && lane < 15, isW = lane >= 16 && lane < 52;
    const int col = isG ? lane - 9 : (isA ? lane - 12 : 0);
    float *wp = cov + 15 * (9 + (isW ? (lane - 16) / 6 : 0)) + 9 + (isW ? (lane - 16) % 6 : 0);
    const float wv = isW ? a.walk[lane - 16] : 0.f;

    float dT = 0.f, dR[9], dV[3], dP[3], avgA[3], avgW[3], x[9], cw = 0.f;
#pragma unroll
    for (int i = 0; i < 9; i++) { dR[i] = (i % 4 == 0) ? 1.f : 0.f; x[i] = 0.f; }
#pragma unroll
    for (int i = 0; i < 3; i++) { dV[i] = 0.f; dP[i] = 0.f; avgA[i] = 0.f; avgW[i] = 0.f; }
    if (cont) {
        dT = (float)rec[P_DT];
#pragma unroll
        for (int i = 0; i < 9; i++) dR[i] = (float)rec[P_DR + i];
#pragma unroll
        for (int i = 0; i < 3; i++) { dV[i] = (float)rec[P_DV + i]; dP[i] = (float)rec[P_DP + i]; avgA[i] = avg[i]; avgW[i] = avg[3 + i]; }
        if (isC) {
#pragma unroll
            for (int r = 0; r < 9; r++) x[r] = cov[15 * lane + r];
        } else if (isG) {
#pragma unroll
            for (int i = 0; i < 3; i++) { x[i] = (float)rec[P_JRG + 3 * i + col]; x[3 + i] = (float)rec[P_JVG + 3 * i + col]; x[6 + i] = (float)rec[P_JPG + 3 * i + col]; }
        } else if (isA) {
#pragma unroll
            for (int i = 0; i < 3; i++) { x[3 + i] = (float)rec[P_JVA + 3 * i + col]; x[6 + i] = (float)rec[P_JPA + 3 * i + col]; }
        }
        if (isW) cw = *wp;
    }

    for (int base = 0; base < n; base += 64) {
        const int cnt = n - base < 64 ? n - base : 64;
        float *mine = slot + lane * S_STRIDE;
        wave_lds_sync();                                    // the chunk before is read to its end
        if (lane < cnt) {                                   // (A) what one measurement alone decides
            const float *m = a.meas + (size_t)7 * (m0 + base + lane);
            float mk[7];
#pragma unroll
            for (int i = 0; i < 7; i++) mk[i] = m[i];
            PreintMeas M;
            preint_measure(bg, ba, mk, M);
#pragma unroll
            for (int i = 0; i < 3; i++) { mine[S_ACC + i] = M.acc[i]; mine[S_ACCW + i] = M.accW[i]; }
            mine[S_DT] = M.dt;
#pragma unroll
            for (int i = 0; i < 9; i++) { mine[S_E + i] = M.E[i]; mine[S_JDT + i] = M.Jdt[i]; }
        }
        wave_lds_sync();
        for (int k = 0; k < cnt; k++) {                     // (B) the rotation chain; dR_k is the rotation BEFORE measurement k
            float *s = slot + k * S_STRIDE;
            float E[9];
#pragma unroll
            for (int i = 0; i < 9; i++) E[i] = s[S_E + i];
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 9; i++) s[S_DR + i] = dR[i];
            }
            preint_rotate(dR, E);
        }
        wave_lds_sync();
        if (lane < cnt) {                                   // (C) what measurement k and dR_k decide
            float acc[3], Jdt[9], R[9], q[9];
#pragma unroll
            for (int i = 0; i < 3; i++) acc[i] = mine[S_ACC + i];
#pragma unroll
            for (int i = 0; i < 9; i++) { Jdt[i] = mine[S_JDT + i]; R[i] = mine[S_DR + i]; }
            PreintBlocks K;
            preint_blocks(R, acc, mine[S_DT], K);
#pragma unroll
            for (int i = 0; i < 9; i++) { mine[S_F + i] = K.F[i]; mine[S_G + i] = K.G[i]; mine[S_B2 + i] = K.B2[i]; mine[S_B3 + i] = K.B3[i]; }
#pragma unroll
            for (int i = 0; i < 3; i++) mine[S_RACC + i] = K.Racc[i];
#pragma unroll
            for (int c = 0; c < 9; c++) {
                preint_noise_row(c, Jdt, K.B2, K.B3, a.nga, q);
#pragma unroll
                for (int r = 0; r < 9; r++) mine[S_Q + 9 * c + r] = q[r];
            }
        }
        wave_lds_sync();
        for (int k = 0; k < cnt; k++) {                     // (D) the recursion
            const float *s = slot + k * S_STRIDE;
            float E[9], F[9], G[9], y[9], Racc[3], accW[3];
            const float dt = s[S_DT];
#pragma unroll
            for (int i = 0; i < 9; i++) { E[i] = s[S_E + i]; F[i] = s[S_F + i]; G[i] = s[S_G + i]; }
#pragma unroll
            for (int i = 0; i < 3; i++) { Racc[i] = s[S_RACC + i]; accW[i] = s[S_ACCW + i]; }
            preint_vectors(dT, dV, dP, avgA, avgW, Racc, accW, dt);
            preint_apply(E, F, G, dt, x, y);
            if (isC) {                                      // lane c holds column c of A C; row c of it comes back
#pragma unroll
                for (int r = 0; r < 9; r++) tr[9 * r + lane] = y[r];
            }
            wave_lds_sync();
            if (isC) {
                float e[9], z[9];
#pragma unroll
                for (int r = 0; r < 9; r++) e[r] = tr[9 * lane + r];
                preint_apply(E, F, G, dt, e, z);
#pragma unroll
                for (int r = 0; r < 9; r++) x[r] = z[r] + s[S_Q + 9 * lane + r];
            } else {
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const float k0 = isG ? s[S_JDT + 3 * i + col] : 0.f, k1 = isA ? s[S_B2 + 3 * i + col] : 0.f, k2 = isA ? s[S_B3 + 3 * i + col] : 0.f;
                    x[i] = y[i] - k0; x[3 + i] = y[3 + i] - k1; x[6 + i] = y[6 + i] - k2;
                }
            }
            cw += wv;
        }
    }

    if (lane == 0) {
        rec[P_DT] = (double)dT;
#pragma unroll
        for (int i = 0; i < 9; i++) rec[P_DR + i] = (double)dR[i];
#pragma unroll
        for (int i = 0; i < 3; i++) { rec[P_DV + i] = (double)dV[i]; rec[P_DP + i] = (double)dP[i]; avg[i] = avgA[i]; avg[3 + i] = avgW[i]; }
    }
    if (isC) {
#pragma unroll
        for (int r = 0; r < 9; r++) cov[15 * lane + r] = x[r];
#pragma unroll
        for (int j = 9; j < 15; j++) { cov[15 * lane + j] = 0.f; cov[15 * j + lane] = 0.f; }
    } else if (isG) {
#pragma unroll
        for (int i = 0; i < 3; i++) { rec[P_JRG + 3 * i + col] = (double)x[i]; rec[P_JVG + 3 * i + col] = (double)x[3 + i]; rec[P_JPG + 3 * i + col] = (double)x[6 + i]; }
    } else if (isA) {
#pragma unroll
        for (int i = 0; i < 3; i++) { rec[P_JVA + 3 * i + col] = (double)x[3 + i]; rec[P_JPA + 3 * i + col] = (double)x[6 + i]; }
    }
    if (isW) *wp = cw;
}

// ---------------------------------------------------------------------------------------------------------------- information
// one Jacobi rotation of the pair (P, Q), as jacobi_eig writes it: columns of A, rows of A, columns of V
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double *A, double *V)
{
#pragma clang fp contract(off)
    if (A[9 * P + Q] == 0.0) return;
    const double theta = (A[9 * Q + Q] - A[9 * P + P]) / (2 * A[9 * P + Q]);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 9; k++) { const double u = A[9 * k + P], v = A[9 * k + Q]; A[9 * k + P] = c * u - s * v; A[9 * k + Q] = s * u + c * v; }
#pragma unroll
    for (int k = 0; k < 9; k++) { const double u = A[9 * P + k], v = A[9 * Q + k]; A[9 * P + k] = c * u - s * v; A[9 * Q + k] = s * u + c * v; }
#pragma unroll
    for (int k = 0; k < 9; k++) { const double u = V[9 * k + P], v = V[9 * k + Q]; V[9 * k + P] = c * u - s * v; V[9 * k + Q] = s * u + c * v; }
}
template <int P, int Q>
__device__ __forceinline__ void jacobi_row(double *A, double *V)
{
    jacobi_rotate<P, Q>(A, V);
    if constexpr (Q < 8) jacobi_row<P, Q + 1>(A, V);
}
template <int P>
__device__ __forceinline__ void jacobi_sweep(double *A, double *V)
{
    jacobi_row<P, P + 1>(A, V);
    if constexpr (P < 7) jacobi_sweep<P + 1>(A, V);
}

__device__ __forceinline__ void inv3_block_f(const float *cov, int o, double *out9)
{
#pragma clang fp contract(off)
    double A[9], I[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) A[3 * r + c] = (double)cov[15 * (o + r) + o + c];
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double id = 1.0 / (A[0] * c0 + A[1] * c1 + A[2] * c2);
    I[0] = c0 * id; I[1] = (A[2] * A[7] - A[1] * A[8]) * id; I[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    I[3] = c1 * id; I[4] = (A[0] * A[8] - A[2] * A[6]) * id; I[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    I[6] = c2 * id; I[7] = (A[1] * A[6] - A[0] * A[7]) * id; I[8] = (A[0] * A[4] - A[1] * A[3]) * id;
#pragma unroll
    for (int i = 0; i < 9; i++) out9[i] = (double)(float)I[i];
}

__global__ __launch_bounds__(64) void k_preint_info(const float *covs, int chains, double *info, double *info_g, double *info_a)
{
#pragma clang fp contract(off)
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= chains) return;
    const float *cov = covs + (size_t)225 * ch;
    double A[81], V[81];
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int c = 0; c < 9; c++) { A[9 * r + c] = 0.5 * ((double)cov[15 * r + c] + (double)cov[15 * c + r]); V[9 * r + c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0;
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = i + 1; j < 9; j++) off += A[9 * i + j] * A[9 * i + j];
        if (off < 1e-300) break;
        jacobi_sweep<0>(A, V);
    }
    double w[9], wmax = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) wmax = fmax(wmax, fabs(A[10 * i]));
#pragma unroll
    for (int i = 0; i < 9; i++) {
        double inv = (A[10 * i] > wmax * 1e-7 * 9) ? 1.0 / A[10 * i] : 0.0;
        if (inv < 1e-12) inv = 0.0;
        w[i] = inv;
    }
    double *out = info + (size_t)81 * ch;
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int c = 0; c < 9; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) s += V[9 * r + k] * w[k] * V[9 * c + k];
            out[9 * r + c] = s;
        }
    double b[9];
    inv3_block_f(cov, 9, b);
#pragma unroll
    for (int i = 0; i < 9; i++) info_g[(size_t)9 * ch + i] = b[i];
    inv3_block_f(cov, 12, b);
#pragma unroll
    for (int i = 0; i < 9; i++) info_a[(size_t)9 * ch + i] = b[i];
}

}  // namespace

extern "C" void orbhip_preint_default_params(orbhip_preint_params *p, float ng, float na, float ngw, float naw)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    const float ng2 = ng * ng, na2 = na * na, ngw2 = ngw * ngw, naw2 = naw * naw;      // IMU::Calib::Set, src/ImuTypes.cc:492-509
    for (int i = 0; i < 3; i++) {
        p->nga[7 * i] = ng2; p->nga[7 * (3 + i)] = na2;
        p->nga_walk[7 * i] = ngw2; p->nga_walk[7 * (3 + i)] = naw2;
    }
    p->force_form = ORBHIP_PREINT_FORM_AUTO;
    p->want_info = 1;
}

extern "C" int orbhip_preint_wave_max_chains(void) { return ORBHIP_PREINT_WAVE_MAX_CHAINS; }

// the launches alone: the arguments are checked already (host_entry.hip checks the offsets where they are, on the host)
int orbhip_preint_launch_internal(orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const int32_t *d_meas_off, const float *d_meas,
        const uint8_t *d_continue, double *d_record, float *d_cov, float *d_avg, double *d_info, double *d_info_g, double *d_info_a)
{
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    PreintArgs a;
    a.meas_off = d_meas_off; a.meas = d_meas; a.cont = d_continue; a.record = d_record; a.cov = d_cov; a.avg = d_avg; a.chains = chains;
    memcpy(a.nga, p->nga, sizeof(a.nga)); memcpy(a.walk, p->nga_walk, sizeof(a.walk));
    const bool wave = p->force_form == ORBHIP_PREINT_FORM_WAVE || (p->force_form == ORBHIP_PREINT_FORM_AUTO && chains < ORBHIP_PREINT_WAVE_MAX_CHAINS);
    if (wave) hipLaunchKernelGGL(k_preint_wave, dim3(chains), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_preint_lane, dim3((chains + 63) / 64), dim3(64), 0, s, a);
    if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("k_preint launch"); return ORBHIP_E_HIP; }
    if (p->want_info) {
        hipLaunchKernelGGL(k_preint_info, dim3((chains + 63) / 64), dim3(64), 0, s, d_cov, chains, d_info, d_info_g, d_info_a);
        if (hipGetLastError() != hipSuccess) { orbhip_set_last_error_internal("k_preint_info launch"); return ORBHIP_E_HIP; }
    }
    return ORBHIP_OK;
}

// the argument rules of both entries, one statement: before the offsets are at hand ...
int orbhip_preint_check_args_internal(const orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const void *meas_off, const void *record,
        const void *cov, const void *avg, const void *info, const void *info_g, const void *info_a)
{
    if (!ctx || !p || chains < 0) return ORBHIP_E_BADARG;
    if (p->force_form != ORBHIP_PREINT_FORM_AUTO && p->force_form != ORBHIP_PREINT_FORM_LANE && p->force_form != ORBHIP_PREINT_FORM_WAVE) {
        orbhip_set_last_error_internal("preintegration: force_form"); return ORBHIP_E_BADARG;
    }
    if (chains == 0) return ORBHIP_OK;
    if (!meas_off || !record || !cov || !avg || (p->want_info && (!info || !info_g || !info_a))) {
        orbhip_set_last_error_internal("preintegration: a required array is NULL"); return ORBHIP_E_BADARG;
    }
    return ORBHIP_OK;
}
// ... and on the offsets (HOST memory)
int orbhip_preint_check_offsets_internal(const int32_t *off, int chains, const void *meas)
{
    if (off[0] < 0) { orbhip_set_last_error_internal("preintegration: meas_off[0] < 0"); return ORBHIP_E_BADARG; }
    for (int c = 0; c < chains; c++)
        if (off[c + 1] < off[c]) { orbhip_set_last_error_internal("preintegration: meas_off decreases"); return ORBHIP_E_BADARG; }
    if (off[chains] > 0 && !meas) { orbhip_set_last_error_internal("preintegration: meas is NULL"); return ORBHIP_E_BADARG; }
    return ORBHIP_OK;
}

extern "C" int orbhip_preintegrate_device(orbhip_ctx *ctx, const orbhip_preint_params *p, int chains, const int32_t *d_meas_off,
        const float *d_meas, const uint8_t *d_continue, double *d_record, float *d_cov, float *d_avg, double *d_info, double *d_info_g,
        double *d_info_a)
{
    if (int rc = orbhip_preint_check_args_internal(ctx, p, chains, d_meas_off, d_record, d_cov, d_avg, d_info, d_info_g, d_info_a)) return rc;
    if (chains == 0) return ORBHIP_OK;
    hipStream_t s = orbhip_ctx_stream_internal(ctx);
    if (hipSetDevice(orbhip_ctx_device_internal(ctx)) != hipSuccess) { orbhip_set_last_error_internal("hipSetDevice"); return ORBHIP_E_HIP; }
    // the offsets come back once (chains + 1 words) and are checked before anything is written; the kernels are not waited for
    std::vector<int32_t> off((size_t)chains + 1);
    ORB_HIP_TRY(hipMemcpyAsync(off.data(), d_meas_off, sizeof(int32_t) * off.size(), hipMemcpyDeviceToHost, s));
    ORB_HIP_TRY(hipStreamSynchronize(s));
    if (int rc = orbhip_preint_check_offsets_internal(off.data(), chains, d_meas)) return rc;
    return orbhip_preint_launch_internal(ctx, p, chains, d_meas_off, d_meas, d_continue, d_record, d_cov, d_avg, d_info, d_info_g, d_info_a);
}
