// Stand-alone driver for the host simulation of the MixIT kernels (csrc/mixit.hip: sep_mixit_scratch_bytes, sep_mixit_gram, sep_mixit_search,
// sep_mixit_bwd): R = M + N in {2, 10, 24} at T = 1 and T = 2 SEP_MIXIT_SLAB + 17, every buffer allocated to its exact size and pre-filled with
// NaN, checked against the contract of include/sepkernels.h restated here with plain double loops over the waveforms (no Gram matrix on this
// side: every assignment's remix is formed sample by sample).  Built and run by tools/hostsim_mixit.py, plain or with
// -fsanitize=address,undefined (a program of its own: the sanitizer's runtime is linked in, nothing is preloaded).  Exit status 0 = all
// within the bounds.
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

// the measure of (remix y, mixture x) from the waveforms, and d measure / d y[t] = ct x[t] + ce y[t]
static double measure(int kind, const double* y, const double* x, int T, double* ct, double* ce) {
    double tt = 0, a = 0, yy = 0;
    for (int t = 0; t < T; ++t) { tt += x[t] * x[t]; a += x[t] * y[t]; yy += y[t] * y[t]; }
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
    for (int t = 0; t < T; ++t) d += (x[t] - y[t]) * (x[t] - y[t]);
    const double den = d + (kind == 2 ? TAU * tt : 0.0) + EPS;
    *ct = 2.0 * K / den;
    *ce = -2.0 * K / den;
    return 10.0 * std::log10((tt + EPS) / den);
}

// ncodes = N^M, or 0 where that is beyond what sep_mixit_search takes: the refusal is checked and the gradient is taken at a given code
static void mixit_case(int B, int M, int N, int T, int ncodes) {
    ++g_cases;
    const int R = M + N;
    std::vector<float> est((size_t)B * M * T), tgt((size_t)B * N * T);
    std::vector<float> src = est;
    for (auto& v : src) v = (float)uniform();
    for (size_t i = 0; i < est.size(); ++i) est[i] = (float)(0.8 * src[i] + 0.3 * uniform());
    for (int b = 0; b < B; ++b)                                   // estimate m belongs to mixture (m + b) % N
        for (int n = 0; n < N; ++n)
            for (int t = 0; t < T; ++t) {
                double s = 0.1 * uniform();
                for (int m = 0; m < M; ++m)
                    if ((m + b) % N == n) s += src[((size_t)b * M + m) * T + t];
                tgt[((size_t)b * N + n) * T + t] = (float)s;
            }
    // ---- the Gram matrix
    const size_t sbytes = sep_mixit_scratch_bytes(B, M, N, T);
    CHECK(sbytes == sizeof(double) * (size_t)B * ((T + SEP_MIXIT_SLAB - 1) / SEP_MIXIT_SLAB) * R * R, "case %d: scratch size %zu", g_cases, sbytes);
    std::vector<double> scratch(sbytes / sizeof(double), std::nan("")), gram((size_t)B * R * R, std::nan(""));
    int rc = sep_mixit_gram(est.data(), tgt.data(), gram.data(), scratch.data(), sbytes, B, M, N, T, nullptr);
    CHECK(rc == 0, "case %d: gram: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    auto row = [&](int b, int r) { return r < M ? &est[((size_t)b * M + r) * T] : &tgt[((size_t)b * N + (r - M)) * T]; };
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < R; ++j) {
                double want = 0, ii = 0, jj = 0;
                for (int t = 0; t < T; ++t) { want += (double)row(b, i)[t] * row(b, j)[t]; ii += (double)row(b, i)[t] * row(b, i)[t]; jj += (double)row(b, j)[t] * row(b, j)[t]; }
                const double got = gram[((size_t)b * R + i) * R + j];
                CHECK(std::fabs(got - want) <= 1e-12 * std::sqrt(ii * jj), "case %d: gram[%d][%d][%d] %.17g != %.17g", g_cases, b, i, j, got, want);
                CHECK(got == gram[((size_t)b * R + j) * R + i], "case %d: gram[%d] is not symmetric at (%d, %d)", g_cases, b, i, j);
            }
    for (int kind = 0; kind < 3; ++kind) {
        // ---- the search, against every remix formed from the waveforms
        std::vector<float> best_val(B, std::numeric_limits<float>::quiet_NaN()), per_mix((size_t)B * N, std::numeric_limits<float>::quiet_NaN());
        std::vector<int64_t> best_idx(B, -7);
        rc = sep_mixit_search(gram.data(), B, M, N, kind, 1, 1, EPS, TAU, best_val.data(), best_idx.data(), per_mix.data(), nullptr);
        if (ncodes == 0) {
            CHECK(rc < 0 && strstr(sep_last_error(), "exceeds") && best_idx[0] == -7, "case %d: the search took %d^%d assignments", g_cases, N, M);
            for (int b = 0; b < B; ++b) best_idx[b] = 54321 + b;
        } else {
            CHECK(rc == 0, "case %d: search: %s", g_cases, sep_last_error());
            if (rc != 0) return;
        }
        std::vector<double> y((size_t)N * T), x((size_t)N * T), cts(N), ces(N);
        auto score = [&](int b, int64_t code, std::vector<double>* per) {
            std::vector<int> asg(M);
            for (int m = M - 1; m >= 0; --m) { asg[m] = (int)(code % N); code /= N; }
            std::fill(y.begin(), y.end(), 0.0);
            for (int m = 0; m < M; ++m)
                for (int t = 0; t < T; ++t) y[(size_t)asg[m] * T + t] += est[((size_t)b * M + m) * T + t];
            double s = 0;
            for (int n = 0; n < N; ++n) {
                for (int t = 0; t < T; ++t) x[(size_t)n * T + t] = tgt[((size_t)b * N + n) * T + t];
                const double v = measure(kind, &y[(size_t)n * T], &x[(size_t)n * T], T, &cts[n], &ces[n]);
                if (per) (*per)[n] = v;
                s += v;
            }
            return s / N;
        };
        for (int b = 0; b < B; ++b) {
            CHECK(best_idx[b] >= 0, "case %d kind %d: best_idx[%d] = %lld", g_cases, kind, b, (long long)best_idx[b]);
            if (best_idx[b] < 0) continue;
            std::vector<double> per(N);
            const double at_best = score(b, best_idx[b], &per);
            // at T = 1 every remix is a multiple of its mixture and the residual of SI-SDR is eps alone: the value rests on a difference that
            // cancels completely, so only T > 1 is held to the bound of the tests (1e-5 dB; the fp32 store of a 30 dB value rounds by 2e-6)
            const double tol = T > 1 ? 1e-5 : 1e-3;
            if (ncodes > 0) {
                CHECK(std::fabs(at_best - best_val[b]) <= tol, "case %d kind %d: best_val[%d] %.9g, from the waveforms %.9g", g_cases, kind, b, (double)best_val[b], at_best);
                for (int n = 0; n < N; ++n)
                    CHECK(std::fabs(per[n] - per_mix[(size_t)b * N + n]) <= tol, "case %d kind %d: per_mix[%d][%d] %.9g != %.9g", g_cases, kind, b, n,
                          (double)per_mix[(size_t)b * N + n], per[n]);
            }
            if (T > 1)
                for (int64_t code = 0; code < ncodes; ++code)
                    CHECK(score(b, code, nullptr) <= at_best + 1e-9, "case %d kind %d: code %lld beats the kernel's best %lld", g_cases, kind, (long long)code,
                          (long long)best_idx[b]);
            // ---- the gradient at the kernel's best
            score(b, best_idx[b], nullptr);      // leaves y, x, cts, ces of this code
            std::vector<float> gw(1, 0.75f), d_est((size_t)M * T, std::numeric_limits<float>::quiet_NaN());
            rc = sep_mixit_bwd(&est[(size_t)b * M * T], &tgt[(size_t)b * N * T], &gram[(size_t)b * R * R], &best_idx[b], gw.data(), d_est.data(), 1, M, N, T, kind, EPS,
                               TAU, nullptr);
            CHECK(rc == 0, "case %d: bwd: %s", g_cases, sep_last_error());
            if (rc != 0) return;
            std::vector<int> asg(M);
            int64_t code = best_idx[b];
            for (int m = M - 1; m >= 0; --m) { asg[m] = (int)(code % N); code /= N; }
            double big = 0;
            std::vector<double> want((size_t)M * T);
            for (int m = 0; m < M; ++m)
                for (int t = 0; t < T; ++t) {
                    const int n = asg[m];
                    want[(size_t)m * T + t] = 0.75 * (cts[n] * x[(size_t)n * T + t] + ces[n] * y[(size_t)n * T + t]);
                    big = std::fmax(big, std::fabs(want[(size_t)m * T + t]));
                }
            if (T > 1)
                for (size_t i = 0; i < want.size(); ++i)
                    CHECK(std::fabs(d_est[i] - want[i]) <= 1e-5 * big, "case %d kind %d: d_est[%d][%zu] %.9g != %.9g", g_cases, kind, b, i, (double)d_est[i], want[i]);
            for (size_t i = 0; i < want.size(); ++i) CHECK(std::isfinite(d_est[i]), "case %d kind %d: d_est[%d][%zu] was not written", g_cases, kind, b, i);
        }
    }
}

// every refused call returns an error with a message before anything is launched (the outputs keep their NaN)
static void argument_errors() {
    ++g_cases;
    std::vector<float> x(64, 1.f), fo(64, std::numeric_limits<float>::quiet_NaN());
    std::vector<double> g(64, 0.5), out(64, std::nan("")), scratch(64, 0.0);
    std::vector<int64_t> idx(4, 0);
    const size_t sb = scratch.size() * sizeof(double);
    CHECK(sep_mixit_gram(nullptr, x.data(), out.data(), scratch.data(), sb, 1, 1, 1, 8, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null est");
    CHECK(sep_mixit_gram(x.data(), x.data(), out.data(), scratch.data(), sb, 1, 17, 1, 2, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "M 17");
    CHECK(sep_mixit_gram(x.data(), x.data(), out.data(), scratch.data(), sb, 1, 1, 9, 2, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "N 9");
    CHECK(sep_mixit_gram(x.data(), x.data(), out.data(), scratch.data(), sb, 1, 1, 1, 0, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "T 0");
    CHECK(sep_mixit_gram(x.data(), x.data(), out.data(), scratch.data(), 31, 1, 1, 1, 8, nullptr) < 0 && strstr(sep_last_error(), "scratch holds"), "scratch");
    CHECK(sep_mixit_search(g.data(), 1, 16, 3, 0, 1, 1, EPS, TAU, fo.data(), idx.data(), fo.data(), nullptr) < 0 && strstr(sep_last_error(), "exceeds"), "3^16");
    CHECK(sep_mixit_search(g.data(), 1, 2, 2, 3, 1, 1, EPS, TAU, fo.data(), idx.data(), fo.data(), nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "kind 3");
    CHECK(sep_mixit_search(g.data(), 1, 2, 2, 0, 1, 1, EPS, TAU, nullptr, idx.data(), fo.data(), nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null best_val");
    CHECK(sep_mixit_bwd(x.data(), x.data(), g.data(), idx.data(), nullptr, fo.data(), 1, 1, 1, 8, 0, EPS, TAU, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null gw");
    CHECK(sep_mixit_bwd(x.data(), x.data(), g.data(), idx.data(), x.data(), fo.data(), 0, 1, 1, 8, 0, EPS, TAU, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "B 0");
    CHECK(sep_mixit_scratch_bytes(1, 17, 1, 8) == 0 && sep_mixit_scratch_bytes(0, 1, 1, 8) == 0 && sep_mixit_scratch_bytes(70000, 1, 1, 8) == 0, "scratch size of bad arguments");
    for (double v : out) CHECK(std::isnan(v), "a refused call wrote the output");
    for (float v : fo) CHECK(std::isnan(v), "a refused call wrote the output");
}

int main() {
    const int Ts[2] = {1, 2 * SEP_MIXIT_SLAB + 17};
    for (int T : Ts) {
        mixit_case(2, 1, 1, T, 1);              // R = 2
        mixit_case(2, 8, 2, T, 256);            // R = 10: every code is scored on this side
        mixit_case(1, 16, 8, T, 0);             // R = 24: the Gram matrix, the refusal of 8^16 assignments, the gradient at a given code
    }
    argument_errors();
    printf("mixit host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
