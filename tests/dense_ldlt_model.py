"""Systems and yardsticks for tests/test_gpu_dense_ldlt.py: symmetric positive definite systems of a chosen condition number and the
unpivoted L D L^T solve (the elimination the device performs) in numpy at a chosen precision.  No GPU, no library."""
import functools

import numpy as np

LD = np.longdouble
COND = 1e6


def ldlt_solve(A, b, dtype):
    """x of A x = b by L D L^T without pivoting in `dtype`, and the pivots.  Only the lower triangle of A is read."""
    A = np.asarray(A, dtype); b = np.asarray(b, dtype)
    n = len(b)
    Lm = np.zeros((n, n), dtype); d = np.zeros(n, dtype)
    for j in range(n):
        v = Lm[j, :j] * d[:j]
        d[j] = A[j, j] - np.dot(Lm[j, :j], v)
        if j + 1 < n:
            Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j] @ v) / d[j]
    y = np.zeros(n, dtype)
    for i in range(n):
        y[i] = b[i] - np.dot(Lm[i, :i], y[:i])
    y /= d
    x = np.zeros(n, dtype)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - np.dot(Lm[i + 1:, i], x[i + 1:])
    return x, d


@functools.lru_cache(maxsize=None)
def system(n, seed=20240):
    """A = J^T J + mu I with J random [n + 8, n] and mu such that cond(A) = COND (mu is negative where J^T J alone is better conditioned;
    A stays positive definite: its smallest eigenvalue becomes lambda_max(A) / COND.  n = 1 has condition number 1 whatever mu is).
    -> dict(A, rhs, cond, x_ld, x_64): float64 A and rhs, the measured condition number, the longdouble and the float64 solutions."""
    rng = np.random.default_rng(seed + n)
    J = rng.standard_normal((n + 8, n))
    H = J.T @ J
    H = (H + H.T) / 2
    w = np.linalg.eigvalsh(H)
    mu = (w[-1] - COND * w[0]) / (COND - 1) if n > 1 else 0.0
    A = H + mu * np.eye(n)
    rhs = rng.standard_normal(n)
    wa = np.linalg.eigvalsh(A)
    assert wa[0] > 0
    x_ld, _ = ldlt_solve(A, rhs, LD)
    x_64, _ = ldlt_solve(A, rhs, np.float64)
    for a in (A, rhs, x_ld, x_64):
        a.setflags(write=False)
    return dict(A=A, rhs=rhs, cond=float(wa[-1] / wa[0]), x_ld=x_ld, x_64=x_64)


def zero_pivot_system(n, k, seed=7):
    """A well-conditioned system of size n whose row and column k are zero: the unpivoted elimination meets the pivot d_k = 0 exactly
    (every update of entry (k, k) subtracts l * d * l with l = 0 / d = 0)."""
    rng = np.random.default_rng(seed + 100 * n + k)
    J = rng.standard_normal((n + 8, n))
    A = J.T @ J + np.eye(n)
    A[k, :] = 0.0
    A[:, k] = 0.0
    return A, rng.standard_normal(n)
