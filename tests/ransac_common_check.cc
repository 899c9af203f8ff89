// Stand-alone CPU driver of csrc/ransac_common.h for tests/test_ransac_common.py (built there with -fsanitize=address,undefined): reads
// requests from stdin, one per line, and answers each on stdout:
//   S k seed item n iterations                 ransac_draw_set<k> (k = 3, 6, 8) of iterations 0..iterations-1, one line of k indices each;
//                                              every set is written into a heap array of exactly k ints (an index past it is caught)
//   B n min_inliers probability cap            the budget as k_s3s_prepare asks for it: epsilon = min_inliers / n in float
//   P n min_inliers epsilon probability cap    nMin and the budget as k_pnp_prepare asks for them (min_set = 6)
#include <algorithm>
#include <cstdio>
#include <vector>
#include "ransac_common.h"

template <int K>
static void sets(unsigned long long seed, int item, int n, int iterations)
{
    for (int it = 0; it < iterations; it++) {
        std::vector<int32_t> set(K);
        ransac_draw_set<K>(seed, item, it, n, set.data());
        for (int j = 0; j < K; j++) printf("%d%c", (int)set[j], j == K - 1 ? '\n' : ' ');
    }
}

int main()
{
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'S') {
            int k, item, n, iterations;
            unsigned long long seed;
            if (scanf("%d %llu %d %d %d", &k, &seed, &item, &n, &iterations) != 5) return 2;
            if (k == 3) sets<3>(seed, item, n, iterations);
            else if (k == 6) sets<6>(seed, item, n, iterations);
            else if (k == 8) sets<8>(seed, item, n, iterations);
            else return 2;
        } else if (what == 'B') {
            int n, min_inliers, cap;
            double probability;
            if (scanf("%d %d %lf %d", &n, &min_inliers, &probability, &cap) != 4 || n < 1) return 2;
            printf("%d\n", ransac_iteration_budget(n, min_inliers, (float)min_inliers / n, probability, cap));
        } else if (what == 'P') {
            int n, min_inliers, cap;
            float epsilon;
            double probability;
            if (scanf("%d %d %f %lf %d", &n, &min_inliers, &epsilon, &probability, &cap) != 5 || n < 1) return 2;
            const int nmin = std::max((int)((float)n * epsilon), std::max(min_inliers, 6));
            printf("%d %d\n", nmin, ransac_iteration_budget(n, nmin, std::max(epsilon, (float)nmin / (float)n), probability, cap));
        } else return 2;
    }
    return 0;
}
