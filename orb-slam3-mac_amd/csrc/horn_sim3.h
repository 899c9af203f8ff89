// Sim3Solver::ComputeSim3 (reference src/Sim3Solver.cc:316-427): Horn's closed-form absolute orientation from THREE point pairs, in
// double on the float inputs.  The reference runs cv::eigen / cv::Rodrigues / cv::Mat products on CV_32F; here the 4x4 symmetric
// eigenproblem is a cyclic Jacobi iteration in registers (every index static: no scratch) and each output is rounded ONCE to float, the
// type the reference stores mR12i / mt12i / ms12i / mT12i / mT21i in.  One text for the device (sim3solver_kernels.hip, one lane per
// hypothesis) and for the host class (host/Sim3Solver.cc recomputes the best-so-far hypothesis of a chunk from its set).
// Nothing traps: coincident points give M = 0, the first unit vector as quaternion, |v| = 0 and NaN everywhere (as 0/0 does there).
#ifndef ORBHIP_HORN_SIM3_H
#define ORBHIP_HORN_SIM3_H
#include <cfloat>
#include <cmath>

#ifdef __HIPCC__
#define HORN_HD __host__ __device__ inline
#define HORN_UNROLL _Pragma("unroll")
#define HORN_NOUNROLL _Pragma("unroll 1")
#else
#define HORN_HD inline
#define HORN_UNROLL
#define HORN_NOUNROLL
#endif

// float views of one hypothesis: T12 = [sR12 | t12], T21 = [sR21 | t21] (what CheckInliers projects with), R12 / s12 for the getters
struct HornSim3f { float sR12[9], t12[3], sR21[9], t21[3], R12[9], s12; };

// eigenvector of the LARGEST eigenvalue of the symmetric A (destroyed); among equal eigenvalues the lowest index wins
HORN_HD void horn_eig4_max(double (&A)[4][4], double (&q)[4])
{
    double V[4][4];
    double fro = 0;
    HORN_UNROLL
    for (int i = 0; i < 4; i++) {
        HORN_UNROLL
        for (int j = 0; j < 4; j++) { V[i][j] = i == j ? 1.0 : 0.0; fro += A[i][j] * A[i][j]; }
    }
    const double thr = 1e-17 * sqrt(fro);
    HORN_NOUNROLL
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rot = false;
        HORN_UNROLL
        for (int p = 0; p < 3; p++) {
            HORN_UNROLL
            for (int r = p + 1; r < 4; r++) {
                const double apq = A[p][r];
                if (!(fabs(apq) > thr)) continue;
                const double app = A[p][p], aqq = A[r][r];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                HORN_UNROLL
                for (int k = 0; k < 4; k++) {
                    const double vkp = V[k][p], vkq = V[k][r];
                    V[k][p] = c * vkp - s * vkq; V[k][r] = s * vkp + c * vkq;
                    if (k == p || k == r) continue;
                    const double akp = A[k][p], akq = A[k][r];
                    const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                    A[k][p] = np_; A[p][k] = np_; A[k][r] = nq_; A[r][k] = nq_;
                }
                A[p][p] = app - t * apq; A[r][r] = aqq + t * apq; A[p][r] = 0.0; A[r][p] = 0.0;
                rot = true;
            }
        }
        if (!rot) break;
    }
    int m = 0;
    double best = A[0][0];
    if (A[1][1] > best) { best = A[1][1]; m = 1; }
    if (A[2][2] > best) { best = A[2][2]; m = 2; }
    if (A[3][3] > best) { best = A[3][3]; m = 3; }
    HORN_UNROLL
    for (int i = 0; i < 4; i++) q[i] = m == 0 ? V[i][0] : m == 1 ? V[i][1] : m == 2 ? V[i][2] : V[i][3];
}

// P1 / P2 [3 points][3]: the set's points in camera 1 / camera 2 (columns of P3Dc1i / P3Dc2i)
HORN_HD void horn_sim3(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, HornSim3f &o)
{
    // Step 1: centroids and relative coordinates (:321-329)
    double O1[3], O2[3], Pr1[3][3], Pr2[3][3];
    HORN_UNROLL
    for (int c = 0; c < 3; c++) {
        O1[c] = (((double)P1[0][c] + (double)P1[1][c]) + (double)P1[2][c]) / 3.0;
        O2[c] = (((double)P2[0][c] + (double)P2[1][c]) + (double)P2[2][c]) / 3.0;
        HORN_UNROLL
        for (int k = 0; k < 3; k++) { Pr1[k][c] = (double)P1[k][c] - O1[c]; Pr2[k][c] = (double)P2[k][c] - O2[c]; }
    }
    // Step 2: M = Pr2 * Pr1^T (:333)
    double M[3][3];
    HORN_UNROLL
    for (int i = 0; i < 3; i++) {
        HORN_UNROLL
        for (int j = 0; j < 3; j++) M[i][j] = (Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[2][i] * Pr1[2][j];
    }
    // Step 3: N (:337-355)
    const double N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
    const double N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
    const double N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
    double N[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    // Step 4: the quaternion = eigenvector of the highest eigenvalue, then angle-axis 2 atan2(|v|, q0) v / |v| and Rodrigues (:358-374)
    double q[4];
    horn_eig4_max(N, q);
    const double nv = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
    const double ang = atan2(nv, q[0]);
    const double rx = 2.0 * ang * q[1] / nv, ry = 2.0 * ang * q[2] / nv, rz = 2.0 * ang * q[3] / nv;
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    double R[9];
    if (theta < DBL_EPSILON) {
        HORN_UNROLL
        for (int k = 0; k < 9; k++) R[k] = k % 4 == 0 ? 1.0 : 0.0;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
        const double kx = rx * it, ky = ry * it, kz = rz * it;
        R[0] = c + c1 * kx * kx;      R[1] = c1 * kx * ky - s * kz; R[2] = c1 * kx * kz + s * ky;
        R[3] = c1 * kx * ky + s * kz; R[4] = c + c1 * ky * ky;      R[5] = c1 * ky * kz - s * kx;
        R[6] = c1 * kx * kz - s * ky; R[7] = c1 * ky * kz + s * kx; R[8] = c + c1 * kz * kz;
    }
    // Step 5 / 6: P3 = R * Pr2, scale = Pr1 . P3 / sum P3^2 (:378-401)
    double s12 = 1.0;
    if (!fix_scale) {
        double nom = 0, den = 0;
        HORN_UNROLL
        for (int k = 0; k < 3; k++) {
            HORN_UNROLL
            for (int i = 0; i < 3; i++) {
                const double p3 = (R[3 * i] * Pr2[k][0] + R[3 * i + 1] * Pr2[k][1]) + R[3 * i + 2] * Pr2[k][2];
                nom += Pr1[k][i] * p3; den += p3 * p3;
            }
        }
        s12 = nom / den;
    }
    // Step 7: t12 = O1 - s R O2 (:405-406); Step 8: T12 = [sR | t], T21 = [(1/s) R^T | -(1/s) R^T t] (:411-426)
    double t[3], sRi[9];
    const double is = 1.0 / s12;
    HORN_UNROLL
    for (int i = 0; i < 3; i++) t[i] = O1[i] - s12 * ((R[3 * i] * O2[0] + R[3 * i + 1] * O2[1]) + R[3 * i + 2] * O2[2]);
    HORN_UNROLL
    for (int i = 0; i < 3; i++) {
        HORN_UNROLL
        for (int j = 0; j < 3; j++) { sRi[3 * i + j] = is * R[3 * j + i]; o.sR12[3 * i + j] = (float)(s12 * R[3 * i + j]); o.R12[3 * i + j] = (float)R[3 * i + j]; }
    }
    HORN_UNROLL
    for (int i = 0; i < 3; i++) {
        o.t12[i] = (float)t[i];
        o.t21[i] = (float)(-((sRi[3 * i] * t[0] + sRi[3 * i + 1] * t[1]) + sRi[3 * i + 2] * t[2]));
    }
    HORN_UNROLL
    for (int k = 0; k < 9; k++) o.sR21[k] = (float)sRi[k];
    o.s12 = (float)s12;
}
#endif
