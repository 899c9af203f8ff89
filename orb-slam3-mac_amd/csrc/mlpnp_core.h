// MLPnPsolver::computePose (reference src/MLPnPsolver.cpp:345-651) with rot2rodrigues / rodrigues2rot (:653-685), mlpnp_gn (:687-752)
// and the residual with its Jacobian (:754-1010), in double, without the covariance branch (use_cov is always false there).  One text
// for the device (mlpnp_kernels.hip: a lane per 6-point hypothesis), the host and a stand-alone CPU program, for any number of
// correspondences.  A correspondence (bearing f with z = 1, world point X) is read through an accessor `acc(i, f, X)`; the
// per-correspondence pieces (null space, design rows, residual and Jacobian rows) are separate functions from the serial ones
// (eigenproblems, disambiguation, the 6x6 solve), so that a group of lanes could sum the former and run the latter once.
// Where the reference calls Eigen, this file has its own arithmetic; the pose does not depend on which basis or sign a decomposition
// returns (A^T A, J^T J and J^T r see only N N^T), so the agreement is a tolerance, not bits:
//   null space of f            closed form: f x e for the unit vector e least aligned with f, then f x (f x e), both normalised
//   last right singular vector the eigenvector of the smallest eigenvalue of the symmetric A^T A, cyclic Jacobi, at most
//                              MLPNP_MAX_SWEEPS sweeps (nothing loops forever; a NaN matrix ends the first sweep)
//   U V^T of the 3x3 SVD       tmp V diag(1 / sigma) V^T from the Jacobi eigenvectors of tmp^T tmp (equal for a nonsingular tmp; a
//                              singular one gives non-finite entries, a hypothesis that counts 0)
//   FullPivHouseholderQR::rank the same pivoting and the same rule (pivots above |largest pivot| * 3 * DBL_EPSILON) on the 3x3
//   LDLT of J^T J              without pivoting
// The matrices of the eigenproblems live where the caller puts them (element k at p[k * stride]): LDS on the device, an array on the host.
// The Jacobian is the exact derivative of N^T normalize(R(w) X + T) for Rodrigues' R(w), written from
//   d(R(w) X) / dw = -R [X]x (w w^T + (R^T - I) [w]x) / |w|^2     (Gallego and Yezzi, J. Math. Imaging Vis. 51, 2015, eq. III.7)
// which, like the reference's generated code, divides by |w|^2: w = 0 gives NaN rows and, through x -= dx, a NaN hypothesis.
#ifndef ORBHIP_MLPNP_CORE_H
#define ORBHIP_MLPNP_CORE_H
#include <cfloat>
#include <cmath>

#ifdef __HIPCC__
#define MLPNP_HD __host__ __device__ __forceinline__
#define MLPNP_UNROLL _Pragma("unroll")
#define MLPNP_NOUNROLL _Pragma("unroll 1")
#else
#define MLPNP_HD inline
#define MLPNP_UNROLL
#define MLPNP_NOUNROLL
#endif

#define MLPNP_MAX_SWEEPS 30
#define MLPNP_GN_STEPS 5          // maxIt (:711)

MLPNP_HD void mlpnp_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
MLPNP_HD double mlpnp_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
MLPNP_HD double mlpnp_norm(const double a[3]) { return sqrt(mlpnp_dot(a, a)); }
MLPNP_HD double mlpnp_det3(const double R[9])
{
    return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}
// y = R x (row-major) or R^T x
MLPNP_HD void mlpnp_mul(const double R[9], const double x[3], double y[3])
{
    MLPNP_UNROLL
    for (int i = 0; i < 3; i++) y[i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
}
MLPNP_HD void mlpnp_mul_t(const double R[9], const double x[3], double y[3])
{
    MLPNP_UNROLL
    for (int i = 0; i < 3; i++) y[i] = R[i] * x[0] + R[3 + i] * x[1] + R[6 + i] * x[2];
}

// :356-364: an orthonormal basis (r, s) of the plane orthogonal to f
MLPNP_HD void mlpnp_nullspace(const double f[3], double r[3], double s[3])
{
    const double ax = fabs(f[0]), ay = fabs(f[1]), az = fabs(f[2]);
    double e[3] = {0.0, 0.0, 0.0};
    if (ax <= ay && ax <= az) e[0] = 1.0; else if (ay <= az) e[1] = 1.0; else e[2] = 1.0;
    mlpnp_cross(f, e, r);
    const double nr = mlpnp_norm(r);
    r[0] /= nr; r[1] /= nr; r[2] /= nr;
    mlpnp_cross(f, r, s);
    const double ns = mlpnp_norm(s);
    s[0] /= ns; s[1] /= ns; s[2] /= ns;
}

// eigen-decomposition of the symmetric n x n matrix A (element (i, j) at A[(i * n + j) * st], destroyed: its diagonal holds the
// eigenvalues afterwards); the columns of V are the eigenvectors.  n is a multiple of 3 (3, 9 or 12 here).
MLPNP_HD void mlpnp_jacobi(double *A, double *V, int n, int st)
{
    MLPNP_NOUNROLL
    for (int i = 0; i < n; i++) {
        MLPNP_NOUNROLL
        for (int j = 0; j < n; j++) V[(i * n + j) * st] = i == j ? 1.0 : 0.0;
    }
    MLPNP_NOUNROLL
    for (int sweep = 0; sweep < MLPNP_MAX_SWEEPS; sweep++) {
        bool rot = false;
        MLPNP_NOUNROLL
        for (int p = 0; p < n - 1; p++) {
            MLPNP_NOUNROLL
            for (int q = p + 1; q < n; q++) {
                // a pair is left alone once |apq| <= eps sqrt(|app aqq|): the relative rule, which keeps the small eigenvalues (the one
                // wanted here is the smallest) as accurate as the large ones; measured against the norm, the last sweeps would turn
                // rounding noise until MLPNP_MAX_SWEEPS.  A NaN fails the test too.
                const double apq = A[(p * n + q) * st], app = A[(p * n + p) * st], aqq = A[(q * n + q) * st];
                if (!(apq * apq > (DBL_EPSILON * DBL_EPSILON) * fabs(app * aqq))) continue;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                // rows k of A and V are independent of each other: three at a time (n is 3, 9 or 12), every load before the first
                // store, so that the loads of a trip are in flight together -- one by one, each waits for the store before it
                MLPNP_NOUNROLL
                for (int k0 = 0; k0 < n; k0 += 3) {
                    double vkp[3], vkq[3], akp[3], akq[3];
                    MLPNP_UNROLL
                    for (int u = 0; u < 3; u++) {
                        const int k = k0 + u;
                        vkp[u] = V[(k * n + p) * st]; vkq[u] = V[(k * n + q) * st]; akp[u] = A[(k * n + p) * st]; akq[u] = A[(k * n + q) * st];
                    }
                    MLPNP_UNROLL
                    for (int u = 0; u < 3; u++) {
                        const int k = k0 + u;
                        V[(k * n + p) * st] = c * vkp[u] - s * vkq[u]; V[(k * n + q) * st] = s * vkp[u] + c * vkq[u];
                        if (k == p || k == q) continue;
                        const double np_ = c * akp[u] - s * akq[u], nq_ = s * akp[u] + c * akq[u];
                        A[(k * n + p) * st] = np_; A[(p * n + k) * st] = np_; A[(k * n + q) * st] = nq_; A[(q * n + k) * st] = nq_;
                    }
                }
                A[(p * n + p) * st] = app - t * apq; A[(q * n + q) * st] = aqq + t * apq; A[(p * n + q) * st] = 0.0; A[(q * n + p) * st] = 0.0;
                rot = true;
            }
        }
        if (!rot) break;
    }
}

// FullPivHouseholderQR<Matrix3d>::rank() of the symmetric M = sum p p^T (m = xx xy xz yy yz zz), :370-380
MLPNP_HD int mlpnp_rank3(const double m[6])
{
    double a0[3] = {m[0], m[1], m[2]}, a1[3] = {m[1], m[3], m[4]}, a2[3] = {m[2], m[4], m[5]};      // rows
    double piv[3] = {0.0, 0.0, 0.0};
    int nonzero = 3;
    double biggest = 0.0, maxpivot = 0.0;
    // step 0: the largest |entry| of the whole matrix to (0, 0)
    {
        double b = -1.0; int br = 0, bc = 0;
        MLPNP_UNROLL
        for (int c = 0; c < 3; c++) {
            if (fabs(a0[c]) > b) { b = fabs(a0[c]); br = 0; bc = c; }
        }
        MLPNP_UNROLL
        for (int c = 0; c < 3; c++) {
            if (fabs(a1[c]) > b) { b = fabs(a1[c]); br = 1; bc = c; }
        }
        MLPNP_UNROLL
        for (int c = 0; c < 3; c++) {
            if (fabs(a2[c]) > b) { b = fabs(a2[c]); br = 2; bc = c; }
        }
        biggest = b;
        if (!(b > 0.0)) return 0;                                                                   // a zero (or NaN) matrix
        MLPNP_UNROLL
        for (int c = 0; c < 3; c++) {
            if (br == 1) { const double t = a0[c]; a0[c] = a1[c]; a1[c] = t; }
            if (br == 2) { const double t = a0[c]; a0[c] = a2[c]; a2[c] = t; }
        }
        if (bc == 1) { double t = a0[0]; a0[0] = a0[1]; a0[1] = t; t = a1[0]; a1[0] = a1[1]; a1[1] = t; t = a2[0]; a2[0] = a2[1]; a2[1] = t; }
        if (bc == 2) { double t = a0[0]; a0[0] = a0[2]; a0[2] = t; t = a1[0]; a1[0] = a1[2]; a1[2] = t; t = a2[0]; a2[0] = a2[2]; a2[2] = t; }
        // Householder on column 0: v = x + sign(x0) |x| e0, the rest H = I - 2 v v^T / v^T v
        const double nx = sqrt(a0[0] * a0[0] + a1[0] * a1[0] + a2[0] * a2[0]);
        const double beta = a0[0] >= 0 ? -nx : nx;
        const double v0 = a0[0] - beta, v1 = a1[0], v2 = a2[0];
        const double vv = v0 * v0 + v1 * v1 + v2 * v2;
        if (vv > 0.0) {
            MLPNP_UNROLL
            for (int c = 1; c < 3; c++) {
                const double d = 2.0 * (v0 * a0[c] + v1 * a1[c] + v2 * a2[c]) / vv;
                a0[c] -= d * v0; a1[c] -= d * v1; a2[c] -= d * v2;
            }
        }
        piv[0] = beta; maxpivot = fabs(beta);
    }
    // step 1: the 2 x 2 corner
    {
        double b = fabs(a1[1]); int br = 1, bc = 1;
        if (fabs(a1[2]) > b) { b = fabs(a1[2]); br = 1; bc = 2; }
        if (fabs(a2[1]) > b) { b = fabs(a2[1]); br = 2; bc = 1; }
        if (fabs(a2[2]) > b) { b = fabs(a2[2]); br = 2; bc = 2; }
        if (b <= biggest * (DBL_EPSILON * 3.0)) nonzero = 1;
        else {
            if (br == 2) { double t = a1[1]; a1[1] = a2[1]; a2[1] = t; t = a1[2]; a1[2] = a2[2]; a2[2] = t; }
            if (bc == 2) { double t = a1[1]; a1[1] = a1[2]; a1[2] = t; t = a2[1]; a2[1] = a2[2]; a2[2] = t; }
            const double nx = sqrt(a1[1] * a1[1] + a2[1] * a2[1]);
            const double beta = a1[1] >= 0 ? -nx : nx;
            const double v1 = a1[1] - beta, v2 = a2[1];
            const double vv = v1 * v1 + v2 * v2;
            if (vv > 0.0) { const double d = 2.0 * (v1 * a1[2] + v2 * a2[2]) / vv; a1[2] -= d * v1; a2[2] -= d * v2; }
            piv[1] = beta; if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
            // step 2: the last entry
            if (fabs(a2[2]) <= biggest * (DBL_EPSILON * 3.0)) nonzero = 2;
            else { piv[2] = a2[2]; if (fabs(a2[2]) > maxpivot) maxpivot = fabs(a2[2]); }
        }
    }
    const double thr = maxpivot * (DBL_EPSILON * 3.0);
    int rank = 0;
    MLPNP_UNROLL
    for (int i = 0; i < 3; i++) if (i < nonzero && fabs(piv[i]) > thr) rank++;
    return rank;
}

// :380-390: planar when rank(sum p p^T) == 2; then E (row-major) has the eigenvectors of that matrix as ROWS, eigenvalues ascending
// (SelfAdjointEigenSolver's order; their signs are free).  A, V: 9 elements each at stride st.
MLPNP_HD bool mlpnp_planar_frame(const double m[6], double *A, double *V, int st, double E[9])
{
    MLPNP_UNROLL
    for (int k = 0; k < 9; k++) E[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    if (mlpnp_rank3(m) != 2) return false;
    A[0] = m[0]; A[st] = m[1]; A[2 * st] = m[2]; A[3 * st] = m[1]; A[4 * st] = m[3]; A[5 * st] = m[4]; A[6 * st] = m[2]; A[7 * st] = m[4]; A[8 * st] = m[5];
    mlpnp_jacobi(A, V, 3, st);
    const double l0 = A[0], l1 = A[4 * st], l2 = A[8 * st];
    int o0 = 0, o1 = 1, o2 = 2;                                                                     // stable sort of three
    if (l1 < l0) { o0 = 1; o1 = 0; }
    const double la = o0 == 0 ? l0 : l1, lb = o0 == 0 ? l1 : l0;
    if (l2 < la) { o2 = o1; o1 = o0; o0 = 2; } else if (l2 < lb) { o2 = o1; o1 = 2; }
    MLPNP_UNROLL
    for (int k = 0; k < 3; k++) { E[k] = V[(3 * k + o0) * st]; E[3 + k] = V[(3 * k + o1) * st]; E[6 + k] = V[(3 * k + o2) * st]; }
    return true;
}

// the two rows of the design matrix of one correspondence (:430-503) added to A^T A (cols x cols at stride st); Xe = E X
MLPNP_HD void mlpnp_design_add(double *A, int st, bool planar, const double r[3], const double s[3], const double Xe[3])
{
    double a[12], b[12];
    if (planar) {
        MLPNP_UNROLL
        for (int i = 0; i < 3; i++) { a[2 * i] = r[i] * Xe[1]; a[2 * i + 1] = r[i] * Xe[2]; a[6 + i] = r[i]; b[2 * i] = s[i] * Xe[1]; b[2 * i + 1] = s[i] * Xe[2]; b[6 + i] = s[i]; }
        MLPNP_UNROLL
        for (int i = 0; i < 9; i++) {
            MLPNP_UNROLL
            for (int j = 0; j < 9; j++) A[(i * 9 + j) * st] += a[i] * a[j] + b[i] * b[j];
        }
    } else {
        MLPNP_UNROLL
        for (int i = 0; i < 3; i++) {
            MLPNP_UNROLL
            for (int j = 0; j < 3; j++) { a[3 * i + j] = r[i] * Xe[j]; b[3 * i + j] = s[i] * Xe[j]; }
            a[9 + i] = r[i]; b[9 + i] = s[i];
        }
        MLPNP_UNROLL
        for (int i = 0; i < 12; i++) {
            MLPNP_UNROLL
            for (int j = 0; j < 12; j++) A[(i * 12 + j) * st] += a[i] * a[j] + b[i] * b[j];
        }
    }
}

// U V^T of the SVD of the 3x3 T (row-major), by the eigenvectors of T^T T; A, V: 9 elements each at stride st
MLPNP_HD void mlpnp_nearest_rotation(const double T[9], double *A, double *V, int st, double R[9])
{
    MLPNP_UNROLL
    for (int i = 0; i < 3; i++) {
        MLPNP_UNROLL
        for (int j = 0; j < 3; j++) A[(3 * i + j) * st] = T[i] * T[j] + T[3 + i] * T[3 + j] + T[6 + i] * T[6 + j];
    }
    mlpnp_jacobi(A, V, 3, st);
    double S[9];                                                                                    // V diag(1 / sigma) V^T
    const double i0 = 1.0 / sqrt(A[0]), i1 = 1.0 / sqrt(A[4 * st]), i2 = 1.0 / sqrt(A[8 * st]);
    MLPNP_UNROLL
    for (int i = 0; i < 3; i++) {
        MLPNP_UNROLL
        for (int j = 0; j < 3; j++)
            S[3 * i + j] = V[(3 * i) * st] * i0 * V[(3 * j) * st] + V[(3 * i + 1) * st] * i1 * V[(3 * j + 1) * st] + V[(3 * i + 2) * st] * i2 * V[(3 * j + 2) * st];
    }
    MLPNP_UNROLL
    for (int i = 0; i < 3; i++) {
        MLPNP_UNROLL
        for (int j = 0; j < 3; j++) R[3 * i + j] = T[3 * i] * S[j] + T[3 * i + 1] * S[3 + j] + T[3 * i + 2] * S[6 + j];
    }
}

// :653-668
MLPNP_HD void mlpnp_rodrigues2rot(const double w[3], double R[9])
{
    MLPNP_UNROLL
    for (int k = 0; k < 9; k++) R[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    const double n = mlpnp_norm(w);
    if (n > DBL_EPSILON) {
        const double a = sin(n) / n, b = (1 - cos(n)) / (n * n);
        const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
        MLPNP_UNROLL
        for (int i = 0; i < 3; i++) {
            MLPNP_UNROLL
            for (int j = 0; j < 3; j++)
                R[3 * i + j] = R[3 * i + j] + a * K[3 * i + j] + b * (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j]);
        }
    }
}
// :670-685: the test is false for a NaN angle too, so w stays 0 then
MLPNP_HD void mlpnp_rot2rodrigues(const double R[9], double w[3])
{
    w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
    const double trace = R[0] + R[4] + R[8] - 1.0;
    const double wnorm = acos(trace / 2.0);
    if (wnorm > DBL_EPSILON) {
        const double sc = wnorm / (2.0 * sin(wnorm));
        w[0] = (R[7] - R[5]) * sc; w[1] = (R[2] - R[6]) * sc; w[2] = (R[3] - R[1]) * sc;
    }
}

// :505-642 after A^T A is summed: the linear solution, scale, nearest rotation, disambiguation on the first 6 correspondences and the
// start x0 = (w, t) of Gauss-Newton.  A, V: cols x cols at stride st (A = A^T A, destroyed).
template <class Acc>
MLPNP_HD void mlpnp_linear_pose(double *A, double *V, int st, bool planar, const double E[9], const Acc &acc, double x0[6])
{
    const int cols = planar ? 9 : 12;
    mlpnp_jacobi(A, V, cols, st);
    int kmin = 0;
    double lmin = A[0];
    MLPNP_NOUNROLL
    for (int k = 1; k < cols; k++) { const double l = A[(k * cols + k) * st]; if (l < lmin) { lmin = l; kmin = k; } }
    double res[12];
    MLPNP_UNROLL
    for (int k = 0; k < 12; k++) res[k] = k < cols ? V[(k * cols + kmin) * st] : 0.0;
    double Rout[9], tout[3];
    if (planar) {                                                                                   // :524-586
        const double c1[3] = {res[0], res[2], res[4]}, c2[3] = {res[1], res[3], res[5]};
        double c0[3];
        mlpnp_cross(c1, c2, c0);
        const double T[9] = {c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]};        // after transposeInPlace: the columns became rows
        const double n1 = sqrt(T[1] * T[1] + T[4] * T[4] + T[7] * T[7]), n2 = sqrt(T[2] * T[2] + T[5] * T[5] + T[8] * T[8]);
        const double scale = 1.0 / sqrt(fabs(n1 * n2));
        double R1[9];
        mlpnp_nearest_rotation(T, A, V, st, R1);
        if (mlpnp_det3(R1) < 0) { MLPNP_UNROLL for (int k = 0; k < 9; k++) R1[k] = -R1[k]; }
        double Q[9];                                                                                // -(E^T R1)^T = -(R1^T E)
        MLPNP_UNROLL
        for (int i = 0; i < 3; i++) {
            MLPNP_UNROLL
            for (int j = 0; j < 3; j++) Q[3 * i + j] = -(R1[i] * E[j] + R1[3 + i] * E[3 + j] + R1[6 + i] * E[6 + j]);
        }
        if (mlpnp_det3(Q) < 0.0) { Q[2] = -Q[2]; Q[5] = -Q[5]; Q[8] = -Q[8]; }
        const double t[3] = {scale * res[6], scale * res[7], scale * res[8]};
        double best = 0.0;
        int ibest = 0;
        MLPNP_NOUNROLL
        for (int c = 0; c < 4; c++) {
            const double sr = c >= 2 ? -1.0 : 1.0, stt = (c & 1) ? -1.0 : 1.0;
            double norms = 0.0;
            MLPNP_NOUNROLL
            for (int p = 0; p < 6; p++) {
                double f[3], X[3], v[3];
                acc(p, f, X);
                MLPNP_UNROLL
                for (int i = 0; i < 3; i++) v[i] = sr * Q[3 * i] * X[0] + sr * Q[3 * i + 1] * X[1] + Q[3 * i + 2] * X[2] + stt * t[i];
                const double nv = mlpnp_norm(v);
                v[0] /= nv; v[1] /= nv; v[2] /= nv;
                norms += 1.0 - mlpnp_dot(v, f);
            }
            if (c == 0 || norms < best) { best = norms; ibest = c; }                               // std::min_element: the first minimum
        }
        const double sr = ibest >= 2 ? -1.0 : 1.0, stt = (ibest & 1) ? -1.0 : 1.0;
        MLPNP_UNROLL
        for (int i = 0; i < 3; i++) { Rout[3 * i] = sr * Q[3 * i]; Rout[3 * i + 1] = sr * Q[3 * i + 1]; Rout[3 * i + 2] = Q[3 * i + 2]; tout[i] = stt * t[i]; }
    } else {                                                                                        // :589-629
        const double T[9] = {res[0], res[3], res[6], res[1], res[4], res[7], res[2], res[5], res[8]};
        const double n0 = sqrt(T[0] * T[0] + T[3] * T[3] + T[6] * T[6]), n1 = sqrt(T[1] * T[1] + T[4] * T[4] + T[7] * T[7]),
                     n2 = sqrt(T[2] * T[2] + T[5] * T[5] + T[8] * T[8]);
        const double scale = 1.0 / pow(fabs(n0 * n1 * n2), 1.0 / 3.0);
        double R1[9];
        mlpnp_nearest_rotation(T, A, V, st, R1);
        if (mlpnp_det3(R1) < 0) { MLPNP_UNROLL for (int k = 0; k < 9; k++) R1[k] = -R1[k]; }
        const double ts[3] = {scale * res[9], scale * res[10], scale * res[11]};
        double t1[3], ti[3];
        mlpnp_mul(R1, ts, t1);
        mlpnp_mul_t(R1, t1, ti);                                                                    // the inverse of [R1 | +-t1] is [R1^T | -+R1^T t1]
        double err[2] = {0.0, 0.0};
        MLPNP_NOUNROLL
        for (int p = 0; p < 6; p++) {
            double f[3], X[3], y[3];
            acc(p, f, X);
            mlpnp_mul_t(R1, X, y);
            MLPNP_UNROLL
            for (int s = 0; s < 2; s++) {
                const double sg = s == 0 ? -1.0 : 1.0;
                double v[3] = {y[0] + sg * ti[0], y[1] + sg * ti[1], y[2] + sg * ti[2]};
                const double nv = mlpnp_norm(v);
                v[0] /= nv; v[1] /= nv; v[2] /= nv;
                err[s] += 1.0 - mlpnp_dot(v, f);
            }
        }
        const double sg = err[0] < err[1] ? -1.0 : 1.0;
        MLPNP_UNROLL
        for (int i = 0; i < 3; i++) { tout[i] = sg * ti[i]; Rout[3 * i] = R1[i]; Rout[3 * i + 1] = R1[3 + i]; Rout[3 * i + 2] = R1[6 + i]; }
    }
    mlpnp_rot2rodrigues(Rout, x0);
    x0[3] = tout[0]; x0[4] = tout[1]; x0[5] = tout[2];
}

// :754-1010 for one correspondence: res = (r, s)^T v / |v| with v = R(w) X + T, and its derivative by (w, T)
MLPNP_HD void mlpnp_res_jac(const double R[9], const double w[3], const double T[3], const double X[3], const double r[3], const double s[3],
                            double res[2], double J[2][6])
{
    double v[3];
    mlpnp_mul(R, X, v);
    v[0] += T[0]; v[1] += T[1]; v[2] += T[2];
    const double nv = mlpnp_norm(v);
    v[0] /= nv; v[1] /= nv; v[2] /= nv;
    const double th2 = mlpnp_dot(w, w);
    MLPNP_UNROLL
    for (int k = 0; k < 2; k++) {
        const double *nk = k == 0 ? r : s;
        const double d = mlpnp_dot(nk, v);
        res[k] = d;
        const double g[3] = {(nk[0] - d * v[0]) / nv, (nk[1] - d * v[1]) / nv, (nk[2] - d * v[2]) / nv};      // (I - v v^T) n / |v|
        double a[3], b[3], c[3], cw[3];
        mlpnp_mul_t(R, g, a);                                                                       // g^T R
        mlpnp_cross(X, a, b);                                                                       // -(g^T R [X]x)^T
        mlpnp_mul(R, b, c);
        c[0] -= b[0]; c[1] -= b[1]; c[2] -= b[2];                                                   // (R - I) b
        mlpnp_cross(c, w, cw);
        const double bw = mlpnp_dot(b, w);
        MLPNP_UNROLL
        for (int i = 0; i < 3; i++) { J[k][i] = (bw * w[i] + cw[i]) / th2; J[k][3 + i] = g[i]; }
    }
}
// the rows of one correspondence added to J^T J (upper triangle, row by row: 21) and J^T r (6)
MLPNP_HD void mlpnp_normal_add(const double res[2], const double J[2][6], double H[21], double g[6])
{
    int k = 0;
    MLPNP_UNROLL
    for (int i = 0; i < 6; i++) {
        MLPNP_UNROLL
        for (int j = i; j < 6; j++) H[k++] += J[0][i] * J[0][j] + J[1][i] * J[1][j];
        g[i] += J[0][i] * res[0] + J[1][i] * res[1];
    }
}
// dx = (J^T J)^-1 J^T r by L D L^T (:733-734)
MLPNP_HD void mlpnp_solve6(const double H[21], const double g[6], double dx[6])
{
    double L[6][6], D[6], y[6];
    int k = 0;
    MLPNP_UNROLL
    for (int i = 0; i < 6; i++) {
        MLPNP_UNROLL
        for (int j = i; j < 6; j++) L[j][i] = H[k++];                                              // lower triangle
    }
    MLPNP_UNROLL
    for (int j = 0; j < 6; j++) {
        double d = L[j][j];
        MLPNP_UNROLL
        for (int m = 0; m < j; m++) d -= L[j][m] * L[j][m] * D[m];
        D[j] = d;
        MLPNP_UNROLL
        for (int i = j + 1; i < 6; i++) {
            double v = L[i][j];
            MLPNP_UNROLL
            for (int m = 0; m < j; m++) v -= L[i][m] * L[j][m] * D[m];
            L[i][j] = v / d;
        }
    }
    MLPNP_UNROLL
    for (int i = 0; i < 6; i++) {
        double v = g[i];
        MLPNP_UNROLL
        for (int m = 0; m < i; m++) v -= L[i][m] * y[m];
        y[i] = v;
    }
    MLPNP_UNROLL
    for (int i = 5; i >= 0; i--) {
        double v = y[i] / D[i];
        MLPNP_UNROLL
        for (int m = i + 1; m < 6; m++) v -= L[m][i] * dx[m];
        dx[i] = v;
    }
}
// :738: `max|dx| > 5 || min|dx| > 1`, the extrema started from the first coefficient as Eigen's visitors do (a NaN there stays)
MLPNP_HD bool mlpnp_step_rejected(const double dx[6])
{
    double mx = fabs(dx[0]), mn = fabs(dx[0]);
    MLPNP_UNROLL
    for (int i = 1; i < 6; i++) { const double a = fabs(dx[i]); if (a > mx) mx = a; if (a < mn) mn = a; }
    return mx > 5.0 || mn > 1.0;
}
// max(|J dx|) over the two rows of one correspondence, folded into dl (:741-742); first: dl takes the first value whatever it is
MLPNP_HD void mlpnp_dl_fold(const double J[2][6], const double dx[6], bool first, double &dl)
{
    MLPNP_UNROLL
    for (int k = 0; k < 2; k++) {
        double v = 0.0;
        MLPNP_UNROLL
        for (int i = 0; i < 6; i++) v += J[k][i] * dx[i];
        v = fabs(v);
        if ((first && k == 0) || v > dl) dl = v;
    }
}

// computePose on the n correspondences of acc, one thread: out = R row-major [9], t [3].  A, V: 144 elements each at stride st.
template <class Acc>
MLPNP_HD void mlpnp_compute_pose(const Acc &acc, int n, double *A, double *V, int st, double out[12])
{
    double m[6] = {0, 0, 0, 0, 0, 0};
    MLPNP_NOUNROLL
    for (int i = 0; i < n; i++) {
        double f[3], X[3];
        acc(i, f, X);
        m[0] += X[0] * X[0]; m[1] += X[0] * X[1]; m[2] += X[0] * X[2]; m[3] += X[1] * X[1]; m[4] += X[1] * X[2]; m[5] += X[2] * X[2];
    }
    double E[9];
    const bool planar = mlpnp_planar_frame(m, A, V, st, E);
    const int cols = planar ? 9 : 12;
    MLPNP_NOUNROLL
    for (int k = 0; k < cols * cols; k++) A[k * st] = 0.0;
    MLPNP_NOUNROLL
    for (int i = 0; i < n; i++) {
        double f[3], X[3], r[3], s[3], Xe[3];
        acc(i, f, X);
        mlpnp_nullspace(f, r, s);
        mlpnp_mul(E, X, Xe);
        mlpnp_design_add(A, st, planar, r, s, Xe);
    }
    double x[6];
    mlpnp_linear_pose(A, V, st, planar, E, acc, x);
    MLPNP_NOUNROLL
    for (int it = 0; it < MLPNP_GN_STEPS; it++) {                                                   // mlpnp_gn, :717-750
        double R[9], H[21], g[6], dx[6];
        mlpnp_rodrigues2rot(x, R);
        MLPNP_UNROLL
        for (int k = 0; k < 21; k++) H[k] = 0.0;
        MLPNP_UNROLL
        for (int k = 0; k < 6; k++) g[k] = 0.0;
        MLPNP_NOUNROLL
        for (int i = 0; i < n; i++) {
            double f[3], X[3], r[3], s[3], res[2], J[2][6];
            acc(i, f, X);
            mlpnp_nullspace(f, r, s);
            mlpnp_res_jac(R, x, x + 3, X, r, s, res, J);
            mlpnp_normal_add(res, J, H, g);
        }
        mlpnp_solve6(H, g, dx);
        if (mlpnp_step_rejected(dx)) break;
        double dl = 0.0;
        MLPNP_NOUNROLL
        for (int i = 0; i < n; i++) {
            double f[3], X[3], r[3], s[3], res[2], J[2][6];
            acc(i, f, X);
            mlpnp_nullspace(f, r, s);
            mlpnp_res_jac(R, x, x + 3, X, r, s, res, J);
            mlpnp_dl_fold(J, dx, i == 0, dl);
        }
        MLPNP_UNROLL
        for (int k = 0; k < 6; k++) x[k] -= dx[k];
        if (dl < 1e-5) break;
    }
    mlpnp_rodrigues2rot(x, out);
    out[9] = x[3]; out[10] = x[4]; out[11] = x[5];
}
#endif
