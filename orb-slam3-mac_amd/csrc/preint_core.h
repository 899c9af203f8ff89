// preint_core.h -- IMU::Preintegrated::IntegrateNewMeasurement (src/ImuTypes.cc:255-310) with IntegratedRotation (:153-178) and
// NormalizeRotation (:30-36) restated in plain float, cut into the pieces both device forms (preint_kernels.hip) and the host class
// (host/ImuTypes.cc) put together: what depends on one measurement alone (preint_measure), the rotation chain (preint_rotate), what
// depends on the rotation before the measurement (preint_blocks, preint_noise) and the linear recursion (preint_apply).
//
// The recursion.  With deltaR / rightJ of the measurement, dR the rotation BEFORE it and Wacc the skew matrix of acc,
//     A = [[deltaR^T, 0, 0], [F, I, 0], [G, dt I, I]],   F = -dt (dR Wacc),   G = -0.5 dt^2 (dR Wacc),
//     B = [[rightJ dt, 0], [0, dR dt], [0, 0.5 dR dt^2]],
// the covariance goes C <- A C A^T + B Nga B^T, and the bias Jacobians obey the SAME map column by column: column j of
// (JRg; JVg; JPg) goes x <- A x - (rightJ dt; 0; 0)[:, j], column j of (0; JVa; JPa) goes x <- A x - (0; dR dt; 0.5 dR dt^2)[:, j]
// (:288-291, :306 written out).  So one 9-vector product with the block-structured A (preint_apply, 33 multiplies instead of 81) is
// the whole recursion: row c of C takes two of them (D = A C by columns, then row c of D A^T = A (row c of D)^T), a Jacobian column
// one.  No dense 9 x 9 x 9 product is formed.  C is carried as its 9 rows; it is symmetric up to rounding, as the reference's is,
// and since a row is fed in as if it were a column each step yields the transpose of the reference's product (see preint_step).
// Nga is read as the reference has it, a symmetric matrix.
// NormalizeRotation's U V^T of an SVD is two Newton steps of the polar iteration R <- (R + R^-T) / 2, the float version of
// so3_normalize (so3_f64.h): the argument is a product of two rotations, a rounding error away from one.
// OpenCV's gemm accumulates float products in double; this text accumulates in float.
// No HIP header is needed: a host compiler sees plain inline functions.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PREINT_FN __host__ __device__ __forceinline__
#else
#define PREINT_FN inline
#endif
// the device text contracts a * b + c (one rounding); a host compiler that does not know the pragma keeps them apart
#if defined(__clang__)
#define PREINT_CONTRACT _Pragma("clang fp contract(fast)")
#define PREINT_UNROLL _Pragma("unroll")
#else
#define PREINT_CONTRACT
#define PREINT_UNROLL
#endif

#define PREINT_EPS 1e-4f

// one measurement (ax, ay, az, wx, wy, wz, dt) at bias (bg[3], ba[3])
struct PreintMeas {
    float acc[3], accW[3], dt;
    float E[9];         // IntegratedRotation::deltaR
    float Jdt[9];       // IntegratedRotation::rightJ * dt
};
// what one step needs of the rotation before it
struct PreintBlocks {
    float F[9], G[9];   // A(3:6, 0:3), A(6:9, 0:3)
    float B2[9], B3[9]; // dR dt, 0.5 dR dt^2
    float Racc[3];      // dR acc
};
// the serial state: column j of (JRg; JVg; JPg) in Jg[j], of (0; JVa; JPa) in Ja[j], row c of C(0:9, 0:9) in C[c]
struct PreintState {
    float dT, dR[9], dV[3], dP[3], avgA[3], avgW[3];
    float Jg[3][9], Ja[3][9], C[9][9];
};

PREINT_FN void preint_mm3(const float *A, const float *B, float *C)
{
    PREINT_CONTRACT
    PREINT_UNROLL
    for (int i = 0; i < 3; i++)
        PREINT_UNROLL
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
PREINT_FN void preint_inv3(const float *A, float *I)
{
    PREINT_CONTRACT
    const float c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const float id = 1.0f / (A[0] * c0 + A[1] * c1 + A[2] * c2);
    I[0] = c0 * id; I[1] = (A[2] * A[7] - A[1] * A[8]) * id; I[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    I[3] = c1 * id; I[4] = (A[0] * A[8] - A[2] * A[6]) * id; I[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    I[6] = c2 * id; I[7] = (A[1] * A[6] - A[0] * A[7]) * id; I[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}
PREINT_FN void preint_normalize(float *R)
{
    PREINT_CONTRACT
    PREINT_UNROLL
    for (int it = 0; it < 2; it++) {
        float I[9];
        preint_inv3(R, I);
        PREINT_UNROLL
        for (int i = 0; i < 3; i++)
            PREINT_UNROLL
            for (int j = 0; j < 3; j++) R[3 * i + j] = 0.5f * (R[3 * i + j] + I[3 * j + i]);
    }
}

PREINT_FN void preint_measure(const float *bg, const float *ba, const float *m, PreintMeas &o)
{
    PREINT_CONTRACT
    PREINT_UNROLL
    for (int i = 0; i < 3; i++) { o.acc[i] = m[i] - ba[i]; o.accW[i] = m[3 + i] - bg[i]; }
    const float dt = m[6];
    o.dt = dt;
    const float x = o.accW[0] * dt, y = o.accW[1] * dt, z = o.accW[2] * dt;
    const float d2 = x * x + y * y + z * z, d = sqrtf(d2);
    const float W[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
    if (d < PREINT_EPS) {                                   // deltaR = I + W (no 0.5 W^2 here, :170), rightJ = I
        PREINT_UNROLL
        for (int i = 0; i < 9; i++) { o.E[i] = W[i]; o.Jdt[i] = 0.f; }
        o.E[0] += 1.f; o.E[4] += 1.f; o.E[8] += 1.f;
        o.Jdt[0] = dt; o.Jdt[4] = dt; o.Jdt[8] = dt;
    } else {
        float W2[9];
        preint_mm3(W, W, W2);
        const float s = sinf(d), c = cosf(d);
        const float a = s / d, b = (1.0f - c) / d2, e = (d - s) / (d2 * d);
        PREINT_UNROLL
        for (int i = 0; i < 9; i++) {
            const float id = (i % 4 == 0) ? 1.f : 0.f;
            o.E[i] = id + W[i] * a + W2[i] * b;
            o.Jdt[i] = (id - W[i] * b + W2[i] * e) * dt;
        }
    }
}

// dR <- NormalizeRotation(dR * deltaR)
PREINT_FN void preint_rotate(float *dR, const float *E)
{
    float R[9];
    preint_mm3(dR, E, R);
    preint_normalize(R);
    PREINT_UNROLL
    for (int i = 0; i < 9; i++) dR[i] = R[i];
}

PREINT_FN void preint_blocks(const float *dR, const float *acc, float dt, PreintBlocks &o)
{
    PREINT_CONTRACT
    const float hdt2 = 0.5f * dt * dt;
    PREINT_UNROLL
    for (int i = 0; i < 3; i++) {
        const float r0 = dR[3 * i], r1 = dR[3 * i + 1], r2 = dR[3 * i + 2];
        // row i of dR Wacc, Wacc = [[0, -a2, a1], [a2, 0, -a0], [-a1, a0, 0]]
        const float m0 = r1 * acc[2] - r2 * acc[1], m1 = r2 * acc[0] - r0 * acc[2], m2 = r0 * acc[1] - r1 * acc[0];
        o.F[3 * i] = -dt * m0; o.F[3 * i + 1] = -dt * m1; o.F[3 * i + 2] = -dt * m2;
        o.G[3 * i] = -hdt2 * m0; o.G[3 * i + 1] = -hdt2 * m1; o.G[3 * i + 2] = -hdt2 * m2;
        o.Racc[i] = r0 * acc[0] + r1 * acc[1] + r2 * acc[2];
    }
    PREINT_UNROLL
    for (int i = 0; i < 9; i++) { o.B2[i] = dR[i] * dt; o.B3[i] = dR[i] * hdt2; }
}

// row c of B Nga B^T (nga: 6 x 6 row-major); c is a compile-time constant wherever the caller unrolls
PREINT_FN void preint_noise_row(int c, const float *Jdt, const float *B2, const float *B3, const float *nga, float *q)
{
    PREINT_CONTRACT
    const float *Bc = c < 3 ? Jdt : (c < 6 ? B2 : B3);
    const int i = c % 3, o = c < 3 ? 0 : 3;
    float bn[6];
    PREINT_UNROLL
    for (int j = 0; j < 6; j++) bn[j] = Bc[3 * i] * nga[6 * o + j] + Bc[3 * i + 1] * nga[6 * (o + 1) + j] + Bc[3 * i + 2] * nga[6 * (o + 2) + j];
    PREINT_UNROLL
    for (int r = 0; r < 3; r++) {
        q[r] = Jdt[3 * r] * bn[0] + Jdt[3 * r + 1] * bn[1] + Jdt[3 * r + 2] * bn[2];
        q[3 + r] = B2[3 * r] * bn[3] + B2[3 * r + 1] * bn[4] + B2[3 * r + 2] * bn[5];
        q[6 + r] = B3[3 * r] * bn[3] + B3[3 * r + 1] * bn[4] + B3[3 * r + 2] * bn[5];
    }
}

// y = A x, A = [[E^T, 0, 0], [F, I, 0], [G, dt I, I]]
PREINT_FN void preint_apply(const float *E, const float *F, const float *G, float dt, const float *x, float *y)
{
    PREINT_CONTRACT
    PREINT_UNROLL
    for (int i = 0; i < 3; i++) {
        y[i] = E[i] * x[0] + E[3 + i] * x[1] + E[6 + i] * x[2];
        y[3 + i] = F[3 * i] * x[0] + F[3 * i + 1] * x[1] + F[3 * i + 2] * x[2] + x[3 + i];
        y[6 + i] = G[3 * i] * x[0] + G[3 * i + 1] * x[1] + G[3 * i + 2] * x[2] + dt * x[3 + i] + x[6 + i];
    }
}

// avgA, avgW, dP, dV, dT of one step (:270-275, :309), from the rotated acceleration dR acc
PREINT_FN void preint_vectors(float &dT, float *dV, float *dP, float *avgA, float *avgW, const float *Racc, const float *accW, float dt)
{
    PREINT_CONTRACT
    const float T = dT + dt;
    PREINT_UNROLL
    for (int i = 0; i < 3; i++) {
        const float ra = Racc[i] * dt;
        avgA[i] = (dT * avgA[i] + ra) / T;
        avgW[i] = (dT * avgW[i] + accW[i] * dt) / T;
        dP[i] = dP[i] + dV[i] * dt + 0.5f * Racc[i] * dt * dt;
        dV[i] = dV[i] + ra;
    }
    dT = T;
}

PREINT_FN void preint_initialize(PreintState &S)
{
    S.dT = 0.f;
    PREINT_UNROLL
    for (int i = 0; i < 9; i++) S.dR[i] = (i % 4 == 0) ? 1.f : 0.f;
    PREINT_UNROLL
    for (int i = 0; i < 3; i++) { S.dV[i] = 0.f; S.dP[i] = 0.f; S.avgA[i] = 0.f; S.avgW[i] = 0.f; }
    PREINT_UNROLL
    for (int j = 0; j < 3; j++)
        PREINT_UNROLL
        for (int i = 0; i < 9; i++) { S.Jg[j][i] = 0.f; S.Ja[j][i] = 0.f; }
    PREINT_UNROLL
    for (int c = 0; c < 9; c++)
        PREINT_UNROLL
        for (int r = 0; r < 9; r++) S.C[c][r] = 0.f;
}

// the whole of IntegrateNewMeasurement but the walk block (a plain add the callers do), in the reference's order: the vectors, the
// blocks of A and B and the position / velocity Jacobians from the old dR, then dR, then C, then JRg (one map with the others here)
PREINT_FN void preint_step(PreintState &S, const float *bg, const float *ba, const float *m, const float *nga)
{
    PreintMeas M;
    PreintBlocks K;
    preint_measure(bg, ba, m, M);
    preint_blocks(S.dR, M.acc, M.dt, K);
    preint_vectors(S.dT, S.dV, S.dP, S.avgA, S.avgW, K.Racc, M.accW, M.dt);
    PREINT_UNROLL
    for (int j = 0; j < 3; j++) {
        float y[9];
        preint_apply(M.E, K.F, K.G, M.dt, S.Jg[j], y);
        PREINT_UNROLL
        for (int i = 0; i < 3; i++) { S.Jg[j][i] = y[i] - M.Jdt[3 * i + j]; S.Jg[j][3 + i] = y[3 + i]; S.Jg[j][6 + i] = y[6 + i]; }
        preint_apply(M.E, K.F, K.G, M.dt, S.Ja[j], y);
        PREINT_UNROLL
        for (int i = 0; i < 3; i++) { S.Ja[j][i] = y[i]; S.Ja[j][3 + i] = y[3 + i] - K.B2[3 * i + j]; S.Ja[j][6 + i] = y[6 + i] - K.B3[3 * i + j]; }
    }
    preint_rotate(S.dR, M.E);
    // D[c] = A (row c of C): column c of A C for a symmetric C.  C is symmetric only up to rounding, so what is computed is
    // A C^T A^T, the transpose of the reference's product: the same products summed in the same order, entry (r, c) for (c, r)
    float D[9][9];
    PREINT_UNROLL
    for (int c = 0; c < 9; c++) preint_apply(M.E, K.F, K.G, M.dt, S.C[c], D[c]);
    PREINT_UNROLL
    for (int c = 0; c < 9; c++) {
        float e[9], y[9], q[9];
        PREINT_UNROLL
        for (int k = 0; k < 9; k++) e[k] = D[k][c];
        preint_apply(M.E, K.F, K.G, M.dt, e, y);
        preint_noise_row(c, M.Jdt, K.B2, K.B3, nga, q);
        PREINT_UNROLL
        for (int r = 0; r < 9; r++) S.C[c][r] = y[r] + q[r];
    }
}
