// The speculative updates of the running site product (phylo_math.h: pm_lp_mul2_spec, pm_lp_mul2_spec_q, pm_lp_mul_spec,
// pm_lp_mul_normal) against pm_lp_mul2 / pm_lp_mul, on the host: built and run by tests/test_merge_fast_rows_cpu.py.
//   flag clear  =>  (p, E, extra) bit-equal to the reference update's
//   flag set   <=>  the reference took its fall-back, decided HERE with <cmath> alone (fpclassify and compares of doubles), not
//                   with the header's bit tests
// over a boundary grid of exponents x mantissa ends, the special values, and random triples weighted towards products that land
// within two binades of 2^-1022 and of overflow.  Every class is counted and must have occurred.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "phylo_math.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {                                    // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double make(unsigned e, uint64_t m) { return pm_from_bits(((uint64_t)e << 52) | (m & 0x000fffffffffffffull)); }
static bool pos_normal(double x) { return std::fpclassify(x) == FP_NORMAL && x > 0.0; }
static bool same(const pm_lp& a, const pm_lp& b) {
    return pm_bits(a.p) == pm_bits(b.p) && a.E == b.E && pm_bits(a.extra) == pm_bits(b.extra);
}

enum { KEPT, X1, X2, SMALL, INF, S_NORMAL, S_ZERO, S_SUBNORMAL, S_NEGATIVE, S_INF, S_NAN, Q_KEPT, Q_SMALL, Q_INF, NCLASS };
static const char* NAMES[NCLASS] = {"kept", "x1", "x2", "small", "inf", "single_normal", "single_zero", "single_subnormal",
                                    "single_negative", "single_inf", "single_nan", "q_kept", "q_small", "q_inf"};
static long counts[NCLASS];
static long failures = 0;

static void fail(const char* what, double p, double x1, double x2) {
    if (failures++ < 20) std::printf("FAIL %s: p=%a x1=%a x2=%a\n", what, p, x1, x2);
}

// the reference's branch, by its definition (phylo_math.h above pm_lp_mul2), in double arithmetic
static int pair_class(double p, double x1, double x2) {
    if (!pos_normal(x1)) return X1;
    if (!pos_normal(x2)) return X2;
    const volatile double t = p * x1;
    const volatile double q = t * x2;
    if (std::isinf((double)q)) return INF;
    if (!(q >= 0x1p-1021)) return SMALL;
    return KEPT;
}

static void pair(double p, int E, double x1, double x2) {
    const pm_lp a0 = {p, E, 0.25};
    pm_lp ref = a0, sp = a0;
    pm_lp_mul2(ref, x1, x2);
    pm_lp_flag f = pm_lp_flag_init();
    pm_lp_mul2_spec(sp, x1, x2, f);
    const int c = pair_class(p, x1, x2);
    ++counts[c];
    const bool set = pm_lp_flag_set(f);
    if (set != (c != KEPT)) fail("pair: flag <=> fall-back", p, x1, x2);
    if (!set && !same(ref, sp)) fail("pair: flag clear but fields differ", p, x1, x2);
    if (!(sp.p >= 1.0 && sp.p < 2.0)) fail("pair: p left [1, 2)", p, x1, x2);
    if (pos_normal(x1) && pos_normal(x2)) {                // the form that trusts its factors
        pm_lp sq = a0;
        pm_lp_flag g = pm_lp_flag_init();
        pm_lp_mul2_spec_q(sq, x1, x2, g);
        ++counts[c == KEPT ? Q_KEPT : c == SMALL ? Q_SMALL : Q_INF];
        if (pm_lp_flag_set(g) != (c != KEPT)) fail("pair_q: flag <=> fall-back", p, x1, x2);
        if (!pm_lp_flag_set(g) && !same(ref, sq)) fail("pair_q: flag clear but fields differ", p, x1, x2);
    }
}

static void single(double p, int E, double x) {
    const pm_lp a0 = {p, E, 0.25};
    pm_lp ref = a0, sp = a0;
    pm_lp_mul(ref, x);
    pm_lp_flag f = pm_lp_flag_init();
    pm_lp_mul_spec(sp, x, f);
    const int k = std::fpclassify(x);
    const int c = k == FP_NAN ? S_NAN : k == FP_ZERO ? S_ZERO : x < 0.0 ? S_NEGATIVE : k == FP_INFINITE ? S_INF
                  : k == FP_SUBNORMAL ? S_SUBNORMAL : S_NORMAL;
    ++counts[c];
    if (pm_lp_flag_set(f) != (c != S_NORMAL)) fail("single: flag <=> rare branch", p, x, 0.0);
    if (pm_lp_special(x) != (c != S_NORMAL)) fail("single: pm_lp_special", p, x, 0.0);
    if (c == S_NORMAL) {
        if (!same(ref, sp)) fail("single: flag clear but fields differ", p, x, 0.0);
        pm_lp n = a0;
        pm_lp_mul_normal(n, x);
        if (!same(ref, n)) fail("single: pm_lp_mul_normal", p, x, 0.0);
    }
    if (!(sp.p >= 1.0 && sp.p < 2.0)) fail("single: p left [1, 2)", p, x, 0.0);
}

// a column as a row loop walks it: one flag over all updates; clear => the fields of the reference chain
static void chain(const std::vector<double>& xs) {
    pm_lp ref = pm_lp_init(), sp = pm_lp_init();
    pm_lp_flag f = pm_lp_flag_init();
    bool any = false;
    size_t i = 0;
    for (; i + 1 < xs.size(); i += 2) {
        any = any || pair_class(ref.p, xs[i], xs[i + 1]) != KEPT;
        pm_lp_mul2(ref, xs[i], xs[i + 1]);
        pm_lp_mul2_spec(sp, xs[i], xs[i + 1], f);
    }
    if (i < xs.size()) {
        any = any || !pos_normal(xs[i]);
        pm_lp_mul(ref, xs[i]);
        pm_lp_mul_spec(sp, xs[i], f);
    }
    // (after a fall-back the two chains hold different p, so later pairs are classified on the reference's: `any` is the
    // reference's history, and the flag may only be set where it is)
    if (pm_lp_flag_set(f) && !any) fail("chain: flag set without a fall-back", xs[0], xs.size() > 1 ? xs[1] : 0.0, 0.0);
    if (!pm_lp_flag_set(f) && (any || !same(ref, sp))) fail("chain: flag clear", xs[0], xs.size() > 1 ? xs[1] : 0.0, 0.0);
}

int main() {
    const unsigned EXPS[] = {1, 2, 1021, 1022, 1023, 2045, 2046};
    const uint64_t MANTS[] = {0, 1, 0x0008000000000000ull, 0x000fffffffffffffull};
    const double PS[] = {1.0, make(1023, 1), 1.5, make(1023, 0x000fffffffffffffull)};
    std::vector<double> grid, specials;
    for (unsigned e : EXPS)
        for (uint64_t m : MANTS) grid.push_back(make(e, m));
    const double inf = pm_inf();
    const double sp[] = {0.0, -0.0, make(0, 1), make(0, 0x000fffffffffffffull), -1.0, -make(1, 0), -make(0, 1), inf, -inf, pm_nan(),
                         -pm_nan()};
    for (double v : sp) specials.push_back(v);
    for (double p : PS) {
        for (double x1 : grid)
            for (double x2 : grid) pair(p, 7, x1, x2);
        for (double s : specials) {
            for (double x : grid) { pair(p, -3, s, x); pair(p, -3, x, s); }
            for (double s2 : specials) pair(p, 0, s, s2);
            single(p, 11, s);
        }
        for (double x : grid) single(p, -1000, x);
    }
    // random triples: p in [1, 2); the product's exponent near the subnormal edge, near overflow, or anywhere
    const long NR = 1200000;
    for (long i = 0; i < NR; ++i) {
        const double p = make(1023, rnd());
        const unsigned e1 = 1 + (unsigned)(rnd() % 2046);
        const uint64_t r = rnd() % 10;
        long e2;
        if (r < 4) e2 = 1023 + 1 - (long)e1 + (long)(rnd() % 5) - 2;           // e1 + e2 - 1023 within two of 1
        else if (r < 8) e2 = 1023 + 2046 - (long)e1 + (long)(rnd() % 5) - 2;   // ... within two of 2046
        else e2 = 1 + (long)(rnd() % 2046);
        if (e2 < 1) e2 = 1;
        if (e2 > 2046) e2 = 2046;
        const double x1 = make(e1, rnd()), x2 = make((unsigned)e2, rnd());
        pair(p, (int)(rnd() % 4001) - 2000, x1, x2);
        if (i % 8 == 0) single(p, (int)(rnd() % 4001) - 2000, x1);
        if (i % 64 == 0) {                                  // a random special among ordinary factors
            const double s = specials[rnd() % specials.size()];
            pair(p, 0, rnd() & 1 ? s : x1, s);
        }
    }
    // columns: ordinary ones (flag clear), ones with an underflowing pair, ones with a special single
    for (int i = 0; i < 20000; ++i) {
        std::vector<double> xs;
        const int n = 1 + (int)(rnd() % 17);
        for (int j = 0; j < n; ++j) xs.push_back(make(1023 - (unsigned)(rnd() % 40), rnd()));
        const uint64_t kind = rnd() % 4;
        if (kind == 1 && n >= 2) { xs[0] = make(500, rnd()); xs[1] = make(500, rnd()); }
        if (kind == 2) xs[n - 1] = specials[rnd() % specials.size()];
        if (kind == 3 && n >= 2) xs[(size_t)(rnd() % (uint64_t)n)] = make(2046, rnd());
        chain(xs);
    }
    std::printf("classes:");
    bool all = true;
    for (int c = 0; c < NCLASS; ++c) {
        std::printf(" %s=%ld", NAMES[c], counts[c]);
        all = all && counts[c] > 0;
    }
    std::printf("\n%ld failures\n", failures);
    if (!all) std::printf("a class never occurred\n");
    return failures == 0 && all ? 0 : 1;
}
