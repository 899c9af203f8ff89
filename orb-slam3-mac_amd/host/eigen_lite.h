// eigen_lite.h -- the smallest part of Eigen that the host classes' signatures touch (fixed matrices, a dynamic matrix and vector that
// are only passed through, Quaterniond), written from the interfaces (Eigen/Dense).  Containers only.  slam_types.h and ImuTypes.h
// include it; with ORBHIP_WITH_ORBSLAM3 the real Eigen takes its place.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace Eigen {
template <typename T, int R, int C>
class Matrix {
public:
    Matrix() { setZero(); }
    void setZero() { for (int i = 0; i < R * C; i++) m[i] = T(0); }
    T &operator()(int i, int j) { return m[i * C + j]; }
    const T &operator()(int i, int j) const { return m[i * C + j]; }
    T &operator()(int i) { return m[i]; }                         // vectors
    const T &operator()(int i) const { return m[i]; }
    T &operator[](int i) { return m[i]; }
    const T &operator[](int i) const { return m[i]; }
    static Matrix Identity() { Matrix I; for (int i = 0; i < (R < C ? R : C); i++) I.m[i * C + i] = T(1); return I; }
    // the comma initialiser (`bg << 0., 0., 0.;`, src/LoopClosing.cc:2023-2024): row-major
    struct CommaInit { Matrix &M; int k; CommaInit &operator,(T v) { M.m[k++] = v; return *this; } };
    CommaInit operator<<(T v) { m[0] = v; return CommaInit{*this, 1}; }
private:
    T m[R * C];
};
typedef Matrix<double, 3, 3> Matrix3d;
typedef Matrix<double, 3, 1> Vector3d;
// a dynamic matrix: Optimizer::InertialOptimization takes LocalMapping::infoInertial by reference and never writes it
class MatrixXd {
public:
    MatrixXd() : r(0), c(0) {}
    MatrixXd(int rows_, int cols_) : r(rows_), c(cols_), m((size_t)rows_ * cols_, 0.0) {}
    int rows() const { return r; }
    int cols() const { return c; }
    double &operator()(int i, int j) { return m[(size_t)i * c + j]; }
    const double &operator()(int i, int j) const { return m[(size_t)i * c + j]; }
private:
    int r, c;
    std::vector<double> m;
};
// a dynamic vector: Optimizer::FullInertialBA takes a pointer to one (vSingVal) and never reads it
class VectorXd {
public:
    VectorXd() {}
    explicit VectorXd(int n) : m((size_t)n, 0.0) {}
    int size() const { return (int)m.size(); }
    double &operator()(int i) { return m[(size_t)i]; }
private:
    std::vector<double> m;
};
class Quaterniond {
public:
    Quaterniond() : q{0, 0, 0, 1} {}
    Quaterniond(double w, double x, double y, double z) : q{x, y, z, w} {}
    explicit Quaterniond(const Matrix3d &R)                        // the trace branch, else the largest diagonal element picks (i, j, k)
    {
        double t = R(0, 0) + R(1, 1) + R(2, 2);
        if (t > 0) {
            t = std::sqrt(t + 1.0);
            q[3] = 0.5 * t; t = 0.5 / t;
            q[0] = (R(2, 1) - R(1, 2)) * t; q[1] = (R(0, 2) - R(2, 0)) * t; q[2] = (R(1, 0) - R(0, 1)) * t;
        } else {
            int i = 0;
            if (R(1, 1) > R(0, 0)) i = 1;
            if (R(2, 2) > R(i, i)) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
            q[i] = 0.5 * t; t = 0.5 / t;
            q[3] = (R(k, j) - R(j, k)) * t; q[j] = (R(j, i) + R(i, j)) * t; q[k] = (R(k, i) + R(i, k)) * t;
        }
    }
    double x() const { return q[0]; }
    double y() const { return q[1]; }
    double z() const { return q[2]; }
    double w() const { return q[3]; }
    Quaterniond conjugate() const { return Quaterniond(q[3], -q[0], -q[1], -q[2]); }
    Quaterniond operator*(const Quaterniond &b) const
    {
        return Quaterniond(q[3] * b.q[3] - q[0] * b.q[0] - q[1] * b.q[1] - q[2] * b.q[2], q[3] * b.q[0] + q[0] * b.q[3] + q[1] * b.q[2] - q[2] * b.q[1],
                           q[3] * b.q[1] + q[1] * b.q[3] + q[2] * b.q[0] - q[0] * b.q[2], q[3] * b.q[2] + q[2] * b.q[3] + q[0] * b.q[1] - q[1] * b.q[0]);
    }
    Vector3d operator*(const Vector3d &v) const                    // v + w * (2 u x v) + u x (2 u x v)
    {
        const double a0 = 2 * (q[1] * v[2] - q[2] * v[1]), a1 = 2 * (q[2] * v[0] - q[0] * v[2]), a2 = 2 * (q[0] * v[1] - q[1] * v[0]);
        Vector3d o;
        o[0] = v[0] + q[3] * a0 + (q[1] * a2 - q[2] * a1);
        o[1] = v[1] + q[3] * a1 + (q[2] * a0 - q[0] * a2);
        o[2] = v[2] + q[3] * a2 + (q[0] * a1 - q[1] * a0);
        return o;
    }
    Matrix3d toRotationMatrix() const
    {
        const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2], twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
        const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
        Matrix3d R;
        R(0, 0) = 1 - (tyy + tzz); R(0, 1) = txy - twz; R(0, 2) = txz + twy;
        R(1, 0) = txy + twz; R(1, 1) = 1 - (txx + tzz); R(1, 2) = tyz - twx;
        R(2, 0) = txz - twy; R(2, 1) = tyz + twx; R(2, 2) = 1 - (txx + tyy);
        return R;
    }
private:
    double q[4];                                                   // x, y, z, w
};
}  // namespace Eigen
