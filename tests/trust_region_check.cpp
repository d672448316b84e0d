// tests/trust_region_check.cpp -- host check of lmono_amd/csrc/trust_region.hpp (built and run by tests/test_trust_region_cpu.py):
// TrustRegion driven by scripted sums (H 21 | g 6 | cost) through the branches that no scan pair and no map scene reaches.
// What each scenario must print follows from the rules of the loop; the arithmetic behind it is worked out in the test's docstring.
#include "../lmono_amd/csrc/trust_region.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
using namespace lmono;

// sums with H = h_diag on the diagonal and h_off off it, g = (0, 0, 0, g_tx, 0, 0): a gradient in the translation alone
static void sums(double *s, double h_diag, double h_off, double g_tx, double cost)
{
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) s[sym6(i, j)] = i == j ? h_diag : h_off;
    for (int i = 0; i < 6; i++) s[21 + i] = 0.0;
    s[21 + 3] = g_tx;
    s[27] = cost;
}

struct Run {
    double s_cur[28], s_sum[28], x[7] = { 0, 0, 0, 1, 0, 0, 0 }, cand[7] = { 0, 0, 0, 0, 0, 0, 0 };
    int takes = 0;
    bool x_is_cand() const { return std::memcmp(x, cand, sizeof x) == 0; }
    bool x_is_start() const { const double x0[7] = { 0, 0, 0, 1, 0, 0, 0 }; return std::memcmp(x, x0, sizeof x) == 0; }
};

// 1: the start's gradient is zero
static void start_gradient_zero()
{
    Run r;
    sums(r.s_cur, 1.0, 0.0, 0.0, 1.0);
    TrustRegion<false> tr(4);
    const bool go = tr.begin(r.s_cur, r.x);
    std::printf("1:begin=%d,iter=%d", (int)go, tr.iter);
}

// 2, 3: an indefinite H whose diagonal is not negative: every factorisation fails
template <bool kRecip>
static void invalid_steps(int scenario, int max_iter)
{
    Run r;
    sums(r.s_cur, 0.0, 1.0, 1.0, 1.0);
    TrustRegion<kRecip> tr(max_iter);
    const bool go = tr.begin(r.s_cur, r.x);
    const int ctl = go ? tr.propose(r.s_cur, r.x, r.cand) : -1;
    std::printf(" | %d<%d>:ctl=%d,iter=%d,invalid=%d,radius=%.17g", scenario, (int)kRecip, ctl, tr.iter, tr.invalid_steps, tr.radius);
}

// 4: every candidate costs more than the accepted pose
template <bool kRecip>
static void every_step_rejected()
{
    Run r;
    sums(r.s_cur, 1.0, 0.0, 1e26, 1.0);
    sums(r.s_sum, 1.0, 0.0, 1e26, 2.0);
    TrustRegion<kRecip> tr(64);
    auto take = [&]() { r.takes++; };
    bool radius_rule = true, reuse_rule = true, full_eval = true;
    int k = 0;
    if (tr.begin(r.s_cur, r.x))
        for (;;) {
            if (tr.reuse_diagonal != (k > 0)) reuse_rule = false;          // the first damping takes a fresh diagonal, the others reuse it
            if (tr.propose(r.s_cur, r.x, r.cand) != 0) { full_eval = false; break; }
            for (int i = 0; i < 6; i++) if (tr.diag[i] != 0.25) reuse_rule = false;      // H scale^2 = 1 / (1 + 1)^2
            const bool go = tr.judge(r.s_sum, r.s_cur, r.x, r.cand, take);
            k++;
            if (tr.radius != std::ldexp(1e4, -(k * (k + 1) / 2))) radius_rule = false;   // halved, quartered, ..: exact in binary
            if (!go) break;
        }
    std::printf(" | 4<%d>:rejects=%d,iter=%d,full_eval=%d,radius_rule=%d,reuse_rule=%d,takes=%d,x_kept=%d,below_min=%d,prev_above_min=%d", (int)kRecip, k, tr.iter,
                (int)full_eval, (int)radius_rule, (int)reuse_rule, r.takes, (int)r.x_is_start(), (int)(tr.radius <= 1e-32), (int)(tr.radius * std::ldexp(1.0, k) > 1e-32));
}

// 5 .. 8: one proposal from H = I, then one judgement of a scripted candidate
static void one_step(const char *tag, int max_iter, double g_tx, double x_cost, double cand_g_tx, double cand_cost)
{
    Run r;
    sums(r.s_cur, 1.0, 0.0, g_tx, x_cost);
    sums(r.s_sum, 1.0, 0.0, cand_g_tx, cand_cost);
    TrustRegion<false> tr(max_iter);
    auto take = [&]() { r.takes++; std::memcpy(r.s_cur, r.s_sum, sizeof r.s_cur); };
    const bool go = tr.begin(r.s_cur, r.x);
    const int ctl = go ? tr.propose(r.s_cur, r.x, r.cand) : -1;
    const bool on = ctl == 0 || ctl == 1 ? tr.judge(r.s_sum, r.s_cur, r.x, r.cand, take) : false;
    std::printf(" | %s:ctl=%d,judge=%d,takes=%d,x=%s,iter=%d,radius=%.6g", tag, ctl, (int)on, r.takes,
                r.x_is_cand() ? "cand" : r.x_is_start() ? "start" : "other", tr.iter, tr.radius);
}

int main()
{
    start_gradient_zero();
    invalid_steps<false>(2, 4); invalid_steps<true>(2, 4);
    invalid_steps<false>(3, 8); invalid_steps<true>(3, 8);
    every_step_rejected<false>(); every_step_rejected<true>();
    one_step("5", 1, 1.0, 0.5, 0.0, 0.0);             // accepted on the last iteration
    one_step("6", 4, 1.0, 0.5, 0.0, 0.0);             // accepted, the new gradient is zero
    one_step("6b", 4, 1.0, 0.5, 1e-3, 0.0);           // accepted, the new gradient is not: the loop goes on
    one_step("7", 4, 1e-9, 1.0, 1e-9, 0.5);           // a step of 1e-9: parameter tolerance
    one_step("8", 4, 1.0, 1.0, 1.0, 1.0 - 5e-7);      // a cost change of 5e-7 of the cost: function tolerance
    std::printf("\n");
    return 0;
}
