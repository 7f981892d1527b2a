// Stand-alone driver for the host simulation of the optimal-permutation kernels (csrc/assign.hip: sep_pair_gram_scratch_bytes, sep_pair_gram,
// sep_assign, sep_pair_assign, sep_pair_bwd): n in {1, 9, 64} at T = 1 and T = 2 SEP_PAIR_SLAB + 17, every buffer allocated to its exact size and
// pre-filled with NaN, checked against the contract of include/sepkernels.h restated here with plain double loops over the waveforms and a plain
// O(n^3) shortest-augmenting-path solver; matrices with NaN and +-Inf must come back with a valid permutation.  Built and run by
// tools/hostsim_hungarian.py, plain or with -fsanitize=address,undefined (a program of its own: the sanitizer's runtime is linked in, nothing
// is preloaded).  Exit status 0 = all within the bounds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "sepkernels.h"

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static double uniform() {      // (-1, 1)
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (double)(int32_t)(g_seed >> 16) / 2147483648.0;
}
static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                            \
    } while (0)

static const double EPS = 1e-12, TAU = 1e-3;
static const float FNAN = std::numeric_limits<float>::quiet_NaN();

// the measure of (estimate y, target x) from the waveforms, and d measure / d y[t] = ct x[t] + ce y[t]
static double measure(int kind, const float* y, const float* x, int T, double* ct, double* ce) {
    double tt = 0, a = 0, yy = 0;
    for (int t = 0; t < T; ++t) { tt += (double)x[t] * x[t]; a += (double)x[t] * y[t]; yy += (double)y[t] * y[t]; }
    const double K = 10.0 / std::log(10.0);
    if (kind == 0) {
        const double c = tt + EPS, alpha = a / c;
        double num = 0, den = 0;
        for (int t = 0; t < T; ++t) { const double p = alpha * x[t]; num += p * p; den += (p - y[t]) * (p - y[t]); }
        const double S = num + EPS, Nn = den + EPS;
        *ct = K * (2.0 * alpha * tt / (c * S) - ((2.0 * alpha * tt - 2.0 * a) / c - 2.0 * alpha) / Nn);
        *ce = K * (-2.0 / Nn);
        return 10.0 * std::log10(S / Nn);
    }
    double d = 0;
    for (int t = 0; t < T; ++t) d += ((double)x[t] - y[t]) * ((double)x[t] - y[t]);
    const double den = d + (kind == 2 ? TAU * tt : 0.0) + EPS;
    *ct = 2.0 * K / den;
    *ce = -2.0 * K / den;
    return 10.0 * std::log10((tt + EPS) / den);
}

// the textbook O(n^3) assignment (rows and columns from 1, column 0 the root) on finite costs: the minimum of sum_i C[i][perm[i]]
static double plain_assign(const std::vector<double>& C, int n) {
    const double INF = std::numeric_limits<double>::infinity();
    std::vector<double> u(n + 1, 0.0), v(n + 1, 0.0);
    std::vector<int> p(n + 1, 0), way(n + 1, 0);
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        std::vector<double> minv(n + 1, INF);
        std::vector<char> used(n + 1, 0);
        do {
            used[j0] = 1;
            const int i0 = p[j0];
            double delta = INF;
            int j1 = 0;
            for (int j = 1; j <= n; ++j)
                if (!used[j]) {
                    const double cur = C[(size_t)(i0 - 1) * n + j - 1] - u[i0] - v[j];
                    if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                    if (minv[j] < delta) { delta = minv[j]; j1 = j; }
                }
            for (int j = 0; j <= n; ++j)
                if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            j0 = j1;
        } while (p[j0] != 0);
        do { const int j1 = way[j0]; p[j0] = p[j1]; j0 = j1; } while (j0);
    }
    double s = 0;
    for (int j = 1; j <= n; ++j) s += C[(size_t)(p[j] - 1) * n + j - 1];
    return s;
}

static bool is_permutation(const int64_t* perm, int n) {
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n; ++i) {
        if (perm[i] < 0 || perm[i] >= n || seen[perm[i]]) return false;
        seen[perm[i]] = 1;
    }
    return true;
}

// sep_assign on an exactly-sized matrix; finite: the value against the plain solver and the certificate of the duals
static void assign_case(int B, int n, int maximize, int fill) {
    ++g_cases;
    const double INF = std::numeric_limits<double>::infinity(), QNAN = std::nan("");
    std::vector<double> cost((size_t)B * n * n), total(B, QNAN), duals((size_t)B * 2 * n, QNAN);
    for (auto& c : cost) c = 10.0 * uniform();
    if (fill == 1) for (size_t e = 0; e < cost.size(); e += 3) cost[e] = QNAN;              // some NaN
    if (fill == 2) for (auto& c : cost) c = QNAN;                                           // all NaN
    if (fill == 3) for (size_t e = 0; e < cost.size(); e += 2) cost[e] = (e % 4) ? INF : -INF;
    std::vector<int64_t> perm((size_t)B * n, -7);
    const int rc = sep_assign(cost.data(), B, n, maximize, perm.data(), total.data(), duals.data(), nullptr);
    CHECK(rc == 0, "case %d: assign: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    for (int b = 0; b < B; ++b) {
        CHECK(is_permutation(&perm[(size_t)b * n], n), "case %d (n=%d fill=%d): item %d is not matched by a permutation", g_cases, n, fill, b);
        if (fill != 0 || !is_permutation(&perm[(size_t)b * n], n)) continue;
        std::vector<double> C(cost.begin() + (size_t)b * n * n, cost.begin() + (size_t)(b + 1) * n * n);
        double big = 0, at = 0, su = 0;
        for (auto& c : C) { if (maximize) c = -c; big = std::fmax(big, std::fabs(c)); }
        const double tol = 64.0 * n * std::ldexp(1.0, -52) * big;
        for (int i = 0; i < n; ++i) at += C[(size_t)i * n + perm[(size_t)b * n + i]];
        for (int k = 0; k < 2 * n; ++k) su += duals[(size_t)b * 2 * n + k];
        CHECK(std::fabs(plain_assign(C, n) - at) <= tol, "case %d (n=%d): value %.17g, plain solver %.17g", g_cases, n, at, plain_assign(C, n));
        CHECK(std::fabs((maximize ? -total[b] : total[b]) - at) <= tol && std::fabs(su - at) <= tol, "case %d (n=%d): total %.17g, duals %.17g, at perm %.17g", g_cases, n,
              total[b], su, at);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                CHECK(duals[(size_t)b * 2 * n + i] + duals[(size_t)b * 2 * n + n + j] <= C[(size_t)i * n + j] + tol, "case %d (n=%d): u[%d] + v[%d] exceeds the cost", g_cases,
                      n, i, j);
    }
}

static void pair_case(int B, int n, int T) {
    ++g_cases;
    std::vector<float> est((size_t)B * n * T), tgt((size_t)B * n * T);
    for (auto& v : tgt) v = (float)uniform();
    for (int b = 0; b < B; ++b)                                   // estimate i belongs to target (i + b + 1) % n
        for (int i = 0; i < n; ++i)
            for (int t = 0; t < T; ++t) est[((size_t)b * n + i) * T + t] = (float)(0.8 * tgt[((size_t)b * n + (i + b + 1) % n) * T + t] + 0.3 * uniform());
    // ---- the inner products
    const size_t sbytes = sep_pair_gram_scratch_bytes(B, n, T);
    CHECK(sbytes == sizeof(double) * (size_t)B * ((T + SEP_PAIR_SLAB - 1) / SEP_PAIR_SLAB) * (n * n + 2 * n), "case %d: scratch size %zu", g_cases, sbytes);
    std::vector<double> scratch(sbytes / sizeof(double), std::nan("")), dots((size_t)B * n * n, std::nan("")), tt((size_t)B * n, std::nan("")), xx((size_t)B * n, std::nan(""));
    int rc = sep_pair_gram(est.data(), tgt.data(), dots.data(), tt.data(), xx.data(), scratch.data(), sbytes, B, n, T, nullptr);
    CHECK(rc == 0, "case %d: gram: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    for (int b = 0; b < B; ++b) {
        std::vector<double> ee(n, 0.0), ww(n, 0.0);
        for (int i = 0; i < n; ++i)
            for (int t = 0; t < T; ++t) {
                ee[i] += (double)est[((size_t)b * n + i) * T + t] * est[((size_t)b * n + i) * T + t];
                ww[i] += (double)tgt[((size_t)b * n + i) * T + t] * tgt[((size_t)b * n + i) * T + t];
            }
        for (int i = 0; i < n; ++i) {
            CHECK(std::fabs(xx[(size_t)b * n + i] - ee[i]) <= T * std::ldexp(1.0, -52) * ee[i], "case %d: xx[%d][%d] %.17g != %.17g", g_cases, b, i, xx[(size_t)b * n + i], ee[i]);
            CHECK(std::fabs(tt[(size_t)b * n + i] - ww[i]) <= T * std::ldexp(1.0, -52) * ww[i], "case %d: tt[%d][%d] %.17g != %.17g", g_cases, b, i, tt[(size_t)b * n + i], ww[i]);
            for (int j = 0; j < n; ++j) {
                double want = 0;
                for (int t = 0; t < T; ++t) want += (double)est[((size_t)b * n + i) * T + t] * tgt[((size_t)b * n + j) * T + t];
                const double got = dots[((size_t)b * n + i) * n + j];
                CHECK(std::fabs(got - want) <= T * std::ldexp(1.0, -52) * std::sqrt(ee[i] * ww[j]), "case %d: dots[%d][%d][%d] %.17g != %.17g", g_cases, b, i, j, got, want);
            }
        }
    }
    for (int kind = 0; kind < 3; ++kind) {
        // ---- the assignment, against the measures formed from the waveforms and the plain solver on them
        std::vector<float> best_val(B, FNAN), per_src((size_t)B * n, FNAN);
        std::vector<int64_t> perm((size_t)B * n, -7);
        std::vector<double> duals((size_t)B * 2 * n, std::nan(""));
        rc = sep_pair_assign(dots.data(), tt.data(), xx.data(), B, n, kind, 1, 1, EPS, TAU, best_val.data(), perm.data(), per_src.data(), kind == 1 ? nullptr : duals.data(),
                             nullptr);
        CHECK(rc == 0, "case %d: pair_assign: %s", g_cases, sep_last_error());
        if (rc != 0) return;
        // at T = 1 every estimate is a multiple of every target and the residual of SI-SDR is eps alone: the value rests on a difference that
        // cancels completely, so only T > 1 is held to the bound of the tests (1e-5 dB)
        const double tol = T > 1 ? 1e-5 : 1e-3;
        for (int b = 0; b < B; ++b) {
            const int64_t* pm = &perm[(size_t)b * n];
            CHECK(is_permutation(pm, n), "case %d kind %d: item %d is not matched by a permutation", g_cases, kind, b);
            if (!is_permutation(pm, n)) continue;
            std::vector<double> neg((size_t)n * n), cts((size_t)n * n), ces((size_t)n * n);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    neg[(size_t)i * n + j] = -measure(kind, &est[((size_t)b * n + i) * T], &tgt[((size_t)b * n + j) * T], T, &cts[(size_t)i * n + j], &ces[(size_t)i * n + j]);
            double at = 0;
            for (int i = 0; i < n; ++i) {
                at -= neg[(size_t)i * n + pm[i]];
                CHECK(std::fabs(-neg[(size_t)i * n + pm[i]] - per_src[(size_t)b * n + i]) <= tol, "case %d kind %d: per_src[%d][%d] %.9g != %.9g", g_cases, kind, b, i,
                      (double)per_src[(size_t)b * n + i], -neg[(size_t)i * n + pm[i]]);
            }
            CHECK(std::fabs(at / n - best_val[b]) <= tol, "case %d kind %d: best_val[%d] %.9g, from the waveforms %.9g", g_cases, kind, b, (double)best_val[b], at / n);
            if (T > 1) {
                CHECK(std::fabs(-plain_assign(neg, n) - at) <= 1e-6 * n, "case %d kind %d: the kernel's permutation scores %.12g, the optimum is %.12g", g_cases, kind, at,
                      -plain_assign(neg, n));
                for (int i = 0; i < n; ++i) CHECK(pm[i] == (i + b + 1) % n, "case %d kind %d: estimate %d of item %d went to %lld", g_cases, kind, i, b, (long long)pm[i]);
            }
            // ---- the gradient at the kernel's permutation
            std::vector<float> gw(1, 0.75f), d_est((size_t)n * T, FNAN);
            rc = sep_pair_bwd(&est[(size_t)b * n * T], &tgt[(size_t)b * n * T], &dots[(size_t)b * n * n], &tt[(size_t)b * n], &xx[(size_t)b * n], pm, gw.data(), d_est.data(), 1, n,
                              T, kind, EPS, TAU, nullptr);
            CHECK(rc == 0, "case %d: bwd: %s", g_cases, sep_last_error());
            if (rc != 0) return;
            for (int i = 0; i < n; ++i)
                for (int t = 0; t < T; ++t) {
                    const double ct = cts[(size_t)i * n + pm[i]], ce = ces[(size_t)i * n + pm[i]];
                    const double x = tgt[((size_t)b * n + pm[i]) * T + t], y = est[((size_t)b * n + i) * T + t];
                    const double want = 0.75 * (ct * x + ce * y), bound = 1e-5 * 0.75 * (std::fabs(ct * x) + std::fabs(ce * y));
                    CHECK(std::isfinite(d_est[(size_t)i * T + t]), "case %d kind %d: d_est[%d][%d][%d] was not written", g_cases, kind, b, i, t);
                    if (T > 1) CHECK(std::fabs(d_est[(size_t)i * T + t] - want) <= bound, "case %d kind %d: d_est[%d][%d][%d] %.9g != %.9g", g_cases, kind, b, i, t,
                                     (double)d_est[(size_t)i * T + t], want);
                }
        }
    }
}

// every refused call returns an error with a message before anything is launched (the outputs keep their NaN)
static void argument_errors() {
    ++g_cases;
    std::vector<float> x(64, 1.f), fo(64, FNAN);
    std::vector<double> g(64, 0.5), out(64, std::nan("")), scratch(64, 0.0);
    std::vector<int64_t> idx(4, 0);
    const size_t sb = scratch.size() * sizeof(double);
    double* o = out.data();
    CHECK(sep_pair_gram(nullptr, x.data(), o, o, o, scratch.data(), sb, 1, 1, 8, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null est");
    CHECK(sep_pair_gram(x.data(), x.data(), o, o, o, scratch.data(), sb, 1, 65, 1, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "n 65");
    CHECK(sep_pair_gram(x.data(), x.data(), o, o, o, scratch.data(), sb, 1, 0, 8, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "n 0");
    CHECK(sep_pair_gram(x.data(), x.data(), o, o, o, scratch.data(), sb, 1, 1, 0, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "T 0");
    CHECK(sep_pair_gram(x.data(), x.data(), o, o, o, scratch.data(), 23, 1, 1, 8, nullptr) < 0 && strstr(sep_last_error(), "scratch holds"), "scratch");
    CHECK(sep_assign(g.data(), 1, 65, 0, idx.data(), o, o, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "assign n 65");
    CHECK(sep_assign(g.data(), 1, 2, 0, idx.data(), o, nullptr, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "assign null duals");
    CHECK(sep_pair_assign(g.data(), g.data(), g.data(), 1, 2, 3, 1, 1, EPS, TAU, fo.data(), idx.data(), fo.data(), nullptr, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"),
          "kind 3");
    CHECK(sep_pair_assign(g.data(), g.data(), g.data(), 1, 2, 0, 1, 1, EPS, TAU, nullptr, idx.data(), fo.data(), nullptr, nullptr) < 0 && strstr(sep_last_error(), "null pointer"),
          "null best_val");
    CHECK(sep_pair_bwd(x.data(), x.data(), g.data(), g.data(), g.data(), idx.data(), nullptr, fo.data(), 1, 1, 8, 0, EPS, TAU, nullptr) < 0 && strstr(sep_last_error(), "null pointer"),
          "null gw");
    CHECK(sep_pair_bwd(x.data(), x.data(), g.data(), g.data(), g.data(), idx.data(), x.data(), fo.data(), 0, 1, 8, 0, EPS, TAU, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"),
          "B 0");
    CHECK(sep_pair_gram_scratch_bytes(1, 65, 8) == 0 && sep_pair_gram_scratch_bytes(0, 1, 8) == 0 && sep_pair_gram_scratch_bytes(70000, 1, 8) == 0, "scratch size of bad arguments");
    for (double v : out) CHECK(std::isnan(v), "a refused call wrote the output");
    for (float v : fo) CHECK(std::isnan(v), "a refused call wrote the output");
}

int main() {
    const int ns[3] = {1, 9, 64}, Ts[2] = {1, 2 * SEP_PAIR_SLAB + 17};
    for (int n : ns) {
        for (int T : Ts) pair_case(n == 64 ? 1 : 2, n, T);
        for (int maximize = 0; maximize < 2; ++maximize) assign_case(2, n, maximize, 0);
        for (int fill = 1; fill <= 3; ++fill) assign_case(1, n, 0, fill);          // NaN here and there, NaN everywhere, +-Inf
    }
    argument_errors();
    printf("hungarian host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
