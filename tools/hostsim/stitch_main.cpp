// Stand-alone driver for the host simulation of the stitching kernels (csrc/stitch.hip: sep_stitch_cost, sep_stitch_chain, sep_stitch_ola; sep_assign
// of csrc/assign.hip between them): window geometries around the wave width and the 16-byte paths, n in {1, 3, 9, 20, 64}, every buffer allocated to its
// exact size and pre-filled with NaN (or -7), checked against the contract of include/sepkernels.h restated here with plain double loops.  Built
// and run by tools/hostsim_stitch.py, plain or with -fsanitize=address,undefined (a program of its own: the sanitizer's runtime is linked in,
// nothing is preloaded).  Exit status 0 = all within the bounds.
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

static const float FNAN = std::numeric_limits<float>::quiet_NaN();

static void shuffle(std::vector<int64_t>& p) {
    for (size_t i = 0; i < p.size(); ++i) p[i] = (int64_t)i;
    for (size_t i = p.size(); i > 1; --i) {
        const size_t j = (size_t)((uniform() * 0.5 + 0.5) * (double)i) % i;
        const int64_t tmp = p[i - 1];
        p[i - 1] = p[j];
        p[j] = tmp;
    }
}

// sep_stitch_cost on exactly-sized buffers: every entry against the plain sum, a planted pair of identical rows at exactly 0, two runs the same bits
static void cost_case(int B, int W, int n, int win, int hop) {
    ++g_cases;
    const int O = win - hop;
    std::vector<float> est((size_t)B * W * n * win);
    for (auto& v : est) v = (float)uniform();
    auto row = [&](int b, int w, int i) { return &est[(((size_t)b * W + w) * n + i) * win]; };
    if (W > 1) memcpy(row(B - 1, 1, 0), row(B - 1, 0, n - 1) + hop, sizeof(float) * O);
    std::vector<double> cost((size_t)B * (W - 1) * n * n, std::nan("")), again(cost);
    int rc = sep_stitch_cost(est.data(), cost.data(), B, W, n, win, hop, nullptr);
    CHECK(rc == 0, "case %d: cost: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    rc = sep_stitch_cost(est.data(), again.data(), B, W, n, win, hop, nullptr);
    CHECK(rc == 0 && memcmp(cost.data(), again.data(), sizeof(double) * cost.size()) == 0, "case %d: two runs differ", g_cases);
    for (int b = 0; b < B; ++b)
        for (int w = 0; w + 1 < W; ++w)
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    double want = 0;
                    for (int t = 0; t < O; ++t) {
                        const double d = (double)row(b, w, i)[hop + t] - (double)row(b, w + 1, j)[t];
                        want += d * d;
                    }
                    const double got = cost[(((size_t)b * (W - 1) + w) * n + i) * n + j];
                    CHECK(std::fabs(got - want) <= 1e-12 * want, "case %d (n=%d win=%d hop=%d): cost[%d][%d][%d][%d] %.17g != %.17g", g_cases, n, win, hop, b, w, i, j, got, want);
                }
    if (W > 1) CHECK(cost[(((size_t)(B - 1) * (W - 1)) * n + n - 1) * n] == 0.0, "case %d: identical rows do not cost 0", g_cases);
}

// sep_stitch_chain against the loop, entries outside [0, n) included
static void chain_case(int B, int W, int n, bool bad) {
    ++g_cases;
    std::vector<int64_t> local((size_t)B * (W - 1) * n), one(n), abs_((size_t)B * W * n, -7);
    for (int r = 0; r < B * (W - 1); ++r) {
        shuffle(one);
        memcpy(&local[(size_t)r * n], one.data(), sizeof(int64_t) * n);
    }
    if (bad && W > 1) {
        local[0] = -1;
        local[local.size() - 1] = n;
    }
    const int rc = sep_stitch_chain(W > 1 ? local.data() : nullptr, abs_.data(), B, W, n, nullptr);
    CHECK(rc == 0, "case %d: chain: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    for (int b = 0; b < B; ++b) {
        std::vector<int64_t> cur(n);
        for (int s = 0; s < n; ++s) cur[s] = s;
        for (int w = 0; w < W; ++w)
            for (int s = 0; s < n; ++s) {
                CHECK(abs_[((size_t)b * W + w) * n + s] == cur[s], "case %d (W=%d n=%d): perm_abs[%d][%d][%d] %lld != %lld", g_cases, W, n, b, w, s,
                      (long long)abs_[((size_t)b * W + w) * n + s], (long long)cur[s]);
                if (w + 1 < W) {
                    const int64_t v = local[((size_t)b * (W - 1) + w) * n + cur[s]];
                    cur[s] = v < 0 || v >= n ? 0 : v;
                }
            }
    }
}

// sep_stitch_ola at the four lengths of the tests: copies bit for bit, cross-fades within 1e-6 max|est|, every element written
static void ola_case(int B, int W, int n, int win, int hop) {
    const int O = win - hop, Ts[4] = {win, win + 1, (W - 1) * hop + 1, (W - 1) * hop + win};
    std::vector<float> est((size_t)B * W * n * win);
    double big = 0;
    for (auto& v : est) { v = (float)uniform(); big = std::fmax(big, std::fabs((double)v)); }
    std::vector<int64_t> perm((size_t)B * W * n), one(n);
    for (int r = 0; r < B * W; ++r) {
        shuffle(one);
        memcpy(&perm[(size_t)r * n], one.data(), sizeof(int64_t) * n);
    }
    for (int T : Ts) {
        ++g_cases;
        std::vector<float> out((size_t)B * n * T, FNAN);
        const int rc = sep_stitch_ola(est.data(), perm.data(), out.data(), B, W, n, win, hop, T, nullptr);
        CHECK(rc == 0, "case %d: ola: %s", g_cases, sep_last_error());
        if (rc != 0) return;
        for (int b = 0; b < B; ++b)
            for (int s = 0; s < n; ++s)
                for (int t = 0; t < T; ++t) {
                    const int w = t / hop < W - 1 ? t / hop : W - 1, k = t - w * hop;
                    const float c = est[(((size_t)b * W + w) * n + perm[((size_t)b * W + w) * n + s]) * win + k], got = out[((size_t)b * n + s) * T + t];
                    if (w >= 1 && k < O) {
                        const double a = est[(((size_t)b * W + w - 1) * n + perm[((size_t)b * W + w - 1) * n + s]) * win + hop + k];
                        const double want = a + (k + 0.5) / O * ((double)c - a);
                        CHECK(std::fabs((double)got - want) <= 1e-6 * big, "case %d (win=%d hop=%d T=%d): out[%d][%d][%d] %.9g != %.9g", g_cases, win, hop, T, b, s, t, (double)got, want);
                    } else {
                        CHECK(memcmp(&got, &c, sizeof(float)) == 0, "case %d (win=%d hop=%d T=%d): out[%d][%d][%d] is not a copy", g_cases, win, hop, T, b, s, t);
                    }
                }
    }
}

// the four launches in a row on windows cut from n long tracks with scrambled rows and a little noise: every window comes back in the order
// of the first, the tracks come back within the noise
static void pipeline_case(int W, int n, int win, int hop) {
    ++g_cases;
    const int cover = (W - 1) * hop + win, T = cover - 3;
    std::vector<float> tracks((size_t)n * cover), est((size_t)W * n * win);
    for (auto& v : tracks) v = (float)uniform();
    std::vector<int64_t> scramble((size_t)W * n), one(n);
    for (int w = 0; w < W; ++w) {
        shuffle(one);
        memcpy(&scramble[(size_t)w * n], one.data(), sizeof(int64_t) * n);
        for (int r = 0; r < n; ++r)
            for (int k = 0; k < win; ++k) est[((size_t)w * n + r) * win + k] = tracks[(size_t)one[r] * cover + w * hop + k] + (float)(0.01 * uniform());
    }
    std::vector<double> cost((size_t)(W - 1) * n * n, std::nan("")), total(W - 1, std::nan("")), duals((size_t)(W - 1) * 2 * n, std::nan(""));
    std::vector<int64_t> local((size_t)(W - 1) * n, -7), abs_((size_t)W * n, -7);
    std::vector<float> out((size_t)n * T, FNAN);
    int rc = sep_stitch_cost(est.data(), cost.data(), 1, W, n, win, hop, nullptr);
    if (rc == 0) rc = sep_assign(cost.data(), W - 1, n, 0, local.data(), total.data(), duals.data(), nullptr);
    if (rc == 0) rc = sep_stitch_chain(local.data(), abs_.data(), 1, W, n, nullptr);
    if (rc == 0) rc = sep_stitch_ola(est.data(), abs_.data(), out.data(), 1, W, n, win, hop, T, nullptr);
    CHECK(rc == 0, "case %d: pipeline: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    for (int w = 0; w < W; ++w)
        for (int s = 0; s < n; ++s) {
            const int64_t r = abs_[(size_t)w * n + s];
            CHECK(r >= 0 && r < n && scramble[(size_t)w * n + r] == scramble[s], "case %d (n=%d): window %d continues track %d in row %lld", g_cases, n, w, s, (long long)r);
        }
    for (int s = 0; s < n; ++s)
        for (int t = 0; t < T; ++t)
            CHECK(std::fabs(out[(size_t)s * T + t] - tracks[(size_t)scramble[s] * cover + t]) <= 0.0101, "case %d (n=%d): out[%d][%d] is off its track", g_cases, n, s, t);
}

// every refused call returns an error with a message before anything is launched (the outputs keep their NaN)
static void argument_errors() {
    ++g_cases;
    std::vector<float> x(64, 1.f), fo(64, FNAN);
    std::vector<double> out(64, std::nan(""));
    std::vector<int64_t> idx(16, 0), io(16, -7);
    CHECK(sep_stitch_cost(nullptr, out.data(), 1, 2, 2, 8, 4, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null est");
    CHECK(sep_stitch_cost(x.data(), nullptr, 1, 2, 2, 8, 4, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null cost");
    CHECK(sep_stitch_cost(x.data(), nullptr, 1, 1, 2, 8, 4, nullptr) == 0, "one window is no error");
    CHECK(sep_stitch_cost(x.data(), out.data(), 1, 2, 2, 8, 3, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "hop 3 of 8");
    CHECK(sep_stitch_cost(x.data(), out.data(), 1, 2, 2, 8, 8, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "hop 8 of 8");
    CHECK(sep_stitch_cost(x.data(), out.data(), 1, 2, 65, 8, 4, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "n 65");
    CHECK(sep_stitch_cost(x.data(), out.data(), 1, 2, 0, 8, 4, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "n 0");
    CHECK(sep_stitch_cost(x.data(), out.data(), 0, 2, 2, 8, 4, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "B 0");
    CHECK(sep_stitch_chain(idx.data(), nullptr, 1, 2, 2, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null perm_abs");
    CHECK(sep_stitch_chain(nullptr, io.data(), 1, 2, 2, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null perm_local");
    CHECK(sep_stitch_chain(idx.data(), io.data(), 1, 2, 65, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "chain n 65");
    CHECK(sep_stitch_chain(idx.data(), io.data(), 1, 0, 2, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "chain W 0");
    CHECK(sep_stitch_ola(x.data(), idx.data(), nullptr, 1, 2, 2, 8, 4, 12, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null out");
    CHECK(sep_stitch_ola(x.data(), idx.data(), fo.data(), 1, 2, 2, 8, 4, 13, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "T beyond the windows");
    CHECK(sep_stitch_ola(x.data(), idx.data(), fo.data(), 1, 2, 2, 8, 4, 0, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "T 0");
    CHECK(sep_stitch_ola(x.data(), idx.data(), fo.data(), 1, 2, 2, 8, 3, 8, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "ola hop 3 of 8");
    CHECK(sep_stitch_ola(x.data(), idx.data(), fo.data(), 70000, 2, 2, 8, 4, 8, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "ola B 70000");
    for (double v : out) CHECK(std::isnan(v), "a refused call wrote the output");
    for (float v : fo) CHECK(std::isnan(v), "a refused call wrote the output");
    for (int64_t v : io) CHECK(v == -7, "a refused call wrote the output");
}

int main() {
    const int geoms[6][2] = {{2, 1}, {128, 65}, {130, 65}, {1100, 571}, {128, 64}, {2200, 1140}};
    for (const auto& g : geoms) {
        for (int n : {1, 3, 9}) cost_case(2, 3, n, g[0], g[1]);
        ola_case(2, 3, 3, g[0], g[1]);
    }
    cost_case(1, 2, 64, 130, 65);
    ola_case(1, 2, 64, 130, 65);
    for (int W : {1, 2, 300})
        for (int n : {1, 2, 64}) {
            chain_case(2, W, n, false);
            chain_case(2, W, n, true);
        }
    for (int n : {2, 9, 20}) pipeline_case(4, n, 130, 65);
    pipeline_case(4, 5, 128, 64);
    argument_errors();
    printf("stitch host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
