// The host check of the matrix exponential's domain (phylo_treeset.h: pt2_q_norm1, pt2_check_expm_range) as a program of its own,
// for the host compiler's sanitizers (test_expm_contract_cpu.py): lengths either side of the limit, 0, -0, inf and NaN, a rate, the
// closed form's "no limit", the first offender's index and a short message buffer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "phylo_treeset.h"

static int failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            ++failed;                                                  \
            printf("line %d: %s\n", __LINE__, #cond);                 \
        }                                                              \
    } while (0)

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    char msg[240];
    int bad = -1;
    // the norm: the largest column sum of |q_ij|
    const double Q[16] = {-1.0, 0.25, 0.5, 0.25, 0.5, -1.0, 0.125, 0.375, 0.0, 0.25, -1.0, 0.75, 0.25, 0.75, 0.125, -1.125};
    EXPECT(pt2_q_norm1(Q) == 2.5);                          // column 3: 0.25 + 0.375 + 0.75 + 1.125
    const double zero[16] = {0};
    EXPECT(pt2_q_norm1(zero) == 0.0);
    EXPECT(PT2_EXPM_NORM_MAX == std::ldexp(5.371920351148152, PT2_EXPM_S_MAX));
    long checks = 0;
    const double norms[] = {1.0, 2.0, 2.5, 50.0, 1e-3};
    for (double qn : norms) {
        // the largest length the check lets through, and its neighbour above
        double top = PT2_EXPM_NORM_MAX / qn;
        while (qn * top > PT2_EXPM_NORM_MAX) top = std::nextafter(top, 0.0);
        while (qn * std::nextafter(top, inf) <= PT2_EXPM_NORM_MAX) top = std::nextafter(top, inf);
        const double over = std::nextafter(top, inf);
        const double fine[] = {0.0, -0.0, 5e-324, 1e-300, 1e-8, 1.0, 100.0, top, -top, 0.5 * top};
        for (double t : fine) {
            bad = -1;
            EXPECT(pt2_check_expm_range(qn, 1, &t, 1.0, &bad, msg, sizeof msg) == 0 && bad == -1);
            ++checks;
        }
        const double refused[] = {over, -over, 2.0 * top, 1e100, 1e300, std::numeric_limits<double>::max(), inf, -inf, nan};
        for (double t : refused) {
            bad = -1;
            msg[0] = 0;
            EXPECT(pt2_check_expm_range(qn, 1, &t, 1.0, &bad, msg, sizeof msg) == 1 && bad == 0);
            EXPECT(strstr(msg, "length") && strstr(msg, "above") && strlen(msg) < sizeof msg);
            ++checks;
        }
        // a rate: the rounded product rate * t is what is held against the limit
        const double half = 0.5 * top;
        EXPECT(pt2_check_expm_range(qn, 1, &half, 2.0, &bad, msg, sizeof msg) == 0);
        EXPECT(pt2_check_expm_range(qn, 1, &half, 2.0000001, &bad, msg, sizeof msg) == 1 && strstr(msg, "at rate"));
        EXPECT(pt2_check_expm_range(qn, 1, &over, 0.0, &bad, msg, sizeof msg) == 0);          // the invariant category
        EXPECT(pt2_check_expm_range(qn, 1, &over, 1e-30, &bad, msg, sizeof msg) == 0);
        // no limit under the closed form (q_norm1 = 0), whatever the length
        for (double t : refused) EXPECT(pt2_check_expm_range(0.0, 1, &t, 1.0, &bad, msg, sizeof msg) == 0);
        // many lengths: the first offender is named, nothing is read past n
        std::vector<double> ts(37, 0.1);
        EXPECT(pt2_check_expm_range(qn, (int)ts.size(), ts.data(), 1.0, &bad, msg, sizeof msg) == 0);
        ts[36] = over;
        ts[11] = 1e100;
        bad = -1;
        EXPECT(pt2_check_expm_range(qn, (int)ts.size(), ts.data(), 1.0, &bad, msg, sizeof msg) == 1 && bad == 11 && strstr(msg, "1e+100"));
        EXPECT(pt2_check_expm_range(qn, 11, ts.data(), 1.0, &bad, msg, sizeof msg) == 0);
        EXPECT(pt2_check_expm_range(qn, 0, nullptr, 1.0, &bad, msg, sizeof msg) == 0);
        char tiny[8];                                       // a short message buffer is not overrun
        EXPECT(pt2_check_expm_range(qn, (int)ts.size(), ts.data(), 1.0, &bad, tiny, sizeof tiny) == 1 && strlen(tiny) < sizeof tiny);
    }
    {   // a tree's rows still go through pt2_check_tree first: a valid tree with a long branch passes it, and is refused here
        const int32_t child[4] = {0, 1, 3, 2};
        const double blen[4] = {0.1, 0.2, 1e100, 0.0};
        int row = -1;
        EXPECT(pt2_check_tree(3, child, blen, &row, msg, sizeof msg) == 0);
        EXPECT(pt2_check_expm_range(2.0, 4, blen, 1.0, &bad, msg, sizeof msg) == 1 && bad / 2 == 1);
    }
    printf("%ld lengths; %d checks failed\n", checks, failed);
    return failed ? 1 : 0;
}
