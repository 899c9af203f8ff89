// Stand-alone CPU driver of csrc/mlpnp_core.h for tests/test_mlpnp_abi.py (built there with -fsanitize=address,undefined): reads
// problems from stdin -- a count, then per problem n and n rows `fx fy fz X Y Z` -- runs computePose on each with the matrices of the
// eigenproblems in exactly-sized heap arrays (so that an index past 144 elements is caught) and prints R row-major and t, 17 digits.
#include <cstdio>
#include <vector>
#include "mlpnp_core.h"

struct RowAcc {
    const double *rows;
    void operator()(int i, double f[3], double X[3]) const
    {
        for (int k = 0; k < 3; k++) { f[k] = rows[6 * i + k]; X[k] = rows[6 * i + 3 + k]; }
    }
};

int main()
{
    int problems = 0;
    if (scanf("%d", &problems) != 1) return 2;
    for (int p = 0; p < problems; p++) {
        int n = 0;
        if (scanf("%d", &n) != 1 || n < 6) return 2;
        std::vector<double> rows(6 * (size_t)n);
        for (double &v : rows) if (scanf("%lf", &v) != 1) return 2;
        std::vector<double> A(144), V(144);
        RowAcc acc = {rows.data()};
        double T[12];
        mlpnp_compute_pose(acc, n, A.data(), V.data(), 1, T);
        for (int k = 0; k < 12; k++) printf("%.17g%c", T[k], k == 11 ? '\n' : ' ');
    }
    return 0;
}
