// Stand-alone driver for the host simulation of the BSS-eval kernels (csrc/bss.hip: sep_bss_scratch_bytes, sep_bss_xcorr, sep_bss_energies):
// the kernel cases of tests/test_bss_eval_gpu.py on buffers allocated to their exact sizes, checked against the contract of
// include/sepkernels.h restated here with plain double loops, at 1e-12 relative.  Samples beyond a row's length hold NaN: reading one shows in
// the result.  Built and run by tools/hostsim_bss.py, plain or with -fsanitize=address,undefined (a program of its own: the
// sanitizer's runtime is linked in, nothing is preloaded).  Exit status 0 = all within the bound.
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

// rows of a first-order recursion x[t] = u[t] + 0.9 x[t-1], rounded to fp32; NaN at and beyond the row's length
static std::vector<float> audio(int B, int n, int T, const std::vector<int32_t>& lengths) {
    std::vector<float> x((size_t)B * n * T);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < n; ++i) {
            float* r = &x[((size_t)b * n + i) * T];
            const int Tb = lengths.empty() ? T : lengths[b];
            double prev = 0.0;
            for (int t = 0; t < T; ++t) {
                prev = uniform() + 0.9 * prev;
                r[t] = t < Tb ? (float)prev : std::numeric_limits<float>::quiet_NaN();
            }
        }
    return x;
}

static void xcorr_case(int B, int n, int m, int T, int flen, const std::vector<int32_t>& lengths) {
    ++g_cases;
    const std::vector<float> a = audio(B, n, T, lengths), c = audio(B, m, T, lengths);
    const int nm = n > m ? n : m;
    const size_t sbytes = sep_bss_scratch_bytes(B, nm, nm, T, flen);
    CHECK(sbytes > 0, "xcorr case %d: no scratch size", g_cases);
    const int uses[2][2] = {{-(flen - 1), 2 * flen - 1}, {0, flen}};
    for (const auto& use : uses) {
        const int lag_lo = use[0], nlag = use[1];
        const size_t exact = sizeof(double) * (size_t)B * n * m * ((T + 2047) / 2048) * nlag;      // what this one call needs: the buffer holds no more
        CHECK(exact <= sbytes, "xcorr case %d: the helper's size %zu is below the call's need %zu", g_cases, sbytes, exact);
        std::vector<double> scratch(exact / sizeof(double), std::nan("")), out((size_t)B * n * m * nlag, std::nan(""));
        const int rc = sep_bss_xcorr(a.data(), c.data(), lengths.empty() ? nullptr : lengths.data(), out.data(), scratch.data(), exact, B, n, m, T, lag_lo,
                                     nlag, nullptr);
        CHECK(rc == 0, "xcorr case %d: %s", g_cases, sep_last_error());
        if (rc != 0) continue;
        for (int b = 0; b < B; ++b) {
            const int Tb = lengths.empty() ? T : lengths[b];
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < m; ++k) {
                    const float* ar = &a[((size_t)b * n + i) * T];
                    const float* cr = &c[((size_t)b * m + k) * T];
                    double aa = 0.0, cc = 0.0;
                    for (int t = 0; t < Tb; ++t) { aa += (double)ar[t] * ar[t]; cc += (double)cr[t] * cr[t]; }
                    for (int l = 0; l < nlag; ++l) {
                        double want = 0.0;
                        bool any = false;
                        for (int t = 0; t < Tb; ++t) {
                            const long u = (long)t + lag_lo + l;
                            if (u >= 0 && u < Tb) { want += (double)ar[t] * (double)cr[u]; any = true; }
                        }
                        const double got = out[(((size_t)b * n + i) * m + k) * nlag + l];
                        CHECK(std::fabs(got - want) <= 1e-12 * std::sqrt(aa * cc), "xcorr case %d (b %d, pair %d %d, lag %d): %.17g != %.17g", g_cases, b, i, k,
                              lag_lo + l, got, want);
                        CHECK(any || (got == 0.0 && !std::signbit(got)), "xcorr case %d: lag %d has no overlap and is %.17g", g_cases, lag_lo + l, got);
                    }
                }
        }
    }
}

static void energies_case(int B, int n, int m, int T, int flen, const std::vector<int32_t>& lengths) {
    ++g_cases;
    const std::vector<float> ref = audio(B, n, T, lengths), est = audio(B, m, T, lengths);
    std::vector<double> fa((size_t)B * m * n * flen), fo(fa.size());
    for (auto& v : fa) v = uniform() / std::sqrt((double)flen);
    for (auto& v : fo) v = uniform() / std::sqrt((double)flen);
    const size_t exact = 40 * (size_t)B * n * m * (((size_t)T + flen - 1 + 1023) / 1024);
    CHECK(exact <= sep_bss_scratch_bytes(B, n, m, T, flen), "energies case %d: the helper's size is below the call's need", g_cases);
    std::vector<double> scratch(exact / sizeof(double), std::nan("")), out((size_t)B * m * n * 5, std::nan(""));
    const int rc = sep_bss_energies(ref.data(), est.data(), fa.data(), fo.data(), lengths.empty() ? nullptr : lengths.data(), out.data(), scratch.data(), exact,
                                    B, n, m, T, flen, nullptr);
    CHECK(rc == 0, "energies case %d: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    for (int b = 0; b < B; ++b) {
        const int Tb = lengths.empty() ? T : lengths[b], Tx = Tb + flen - 1;
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < n; ++i) {
                double want[5] = {0, 0, 0, 0, 0};
                for (int t = 0; t < Tx; ++t) {
                    double pall = 0.0, s = 0.0;
                    for (int k = 0; k < n; ++k)
                        for (int tau = 0; tau < flen; ++tau)
                            if (t - tau >= 0 && t - tau < Tb) pall += fa[(((size_t)b * m + j) * n + k) * flen + tau] * (double)ref[((size_t)b * n + k) * T + t - tau];
                    for (int tau = 0; tau < flen; ++tau)
                        if (t - tau >= 0 && t - tau < Tb) s += fo[(((size_t)b * m + j) * n + i) * flen + tau] * (double)ref[((size_t)b * n + i) * T + t - tau];
                    const double e = t < Tb ? (double)est[((size_t)b * m + j) * T + t] : 0.0, interf = pall - s, artif = e - pall;
                    const double v[5] = {s, interf, artif, interf + artif, s + interf};
                    for (int q = 0; q < 5; ++q) want[q] += v[q] * v[q];
                }
                for (int q = 0; q < 5; ++q) {
                    const double got = out[(((size_t)b * m + j) * n + i) * 5 + q];
                    CHECK(std::fabs(got - want[q]) <= 1e-12 * want[q], "energies case %d (b %d, estimate %d, reference %d, sum %d): %.17g != %.17g", g_cases, b, j,
                          i, q, got, want[q]);
                }
            }
    }
}

// every refused call returns an error with a message before anything is launched (the output keeps its NaN)
static void argument_errors() {
    ++g_cases;
    std::vector<float> x(64, 1.f);
    std::vector<double> f(64, 0.5), out(64, std::nan("")), scratch(64, 0.0);
    const size_t sb = scratch.size() * sizeof(double);
    CHECK(sep_bss_xcorr(nullptr, x.data(), nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 0, 4, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null a");
    CHECK(sep_bss_xcorr(x.data(), x.data(), nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 0, 0, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "nlag 0");
    CHECK(sep_bss_xcorr(x.data(), x.data(), nullptr, out.data(), scratch.data(), sb, 1, 0, 1, 8, 0, 4, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "n 0");
    CHECK(sep_bss_xcorr(x.data(), x.data(), nullptr, out.data(), scratch.data(), 8, 1, 1, 1, 8, 0, 4, nullptr) < 0 && strstr(sep_last_error(), "scratch holds"), "scratch");
    CHECK(sep_bss_xcorr(x.data(), x.data(), nullptr, out.data(), scratch.data(), sb, 70000, 1, 1, 8, 0, 4, nullptr) < 0 && strstr(sep_last_error(), "grid limit"), "B");
    CHECK(sep_bss_energies(x.data(), x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 0, nullptr) < 0 &&
              strstr(sep_last_error(), "bad arguments"), "flen 0");
    CHECK(sep_bss_energies(x.data(), x.data(), f.data(), nullptr, nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 4, nullptr) < 0 &&
              strstr(sep_last_error(), "null pointer"), "null filter");
    CHECK(sep_bss_energies(x.data(), x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), 32, 1, 1, 1, 8, 4, nullptr) < 0 &&
              strstr(sep_last_error(), "scratch holds"), "scratch");
    CHECK(sep_bss_scratch_bytes(1, 1, 1, 8, 0) == 0 && sep_bss_scratch_bytes(0, 1, 1, 8, 4) == 0 && sep_bss_scratch_bytes(70000, 1, 1, 8, 4) == 0, "scratch size of bad arguments");
    for (double v : out) CHECK(std::isnan(v), "a refused call wrote the output");
}

int main() {
    xcorr_case(2, 2, 2, 700, 32, {});
    xcorr_case(2, 2, 2, 700, 32, {700, 131});
    xcorr_case(1, 1, 1, 20, 32, {});
    xcorr_case(1, 2, 2, 2049, 16, {});
    xcorr_case(1, 2, 3, 300, 8, {});
    xcorr_case(1, 1, 1, 600, 200, {});
    energies_case(2, 2, 2, 700, 32, {});
    energies_case(2, 2, 2, 700, 32, {700, 131});
    energies_case(1, 2, 2, 1010, 16, {});
    energies_case(1, 1, 2, 300, 300, {});
    argument_errors();
    printf("bss-eval host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
