// Stand-alone driver for the host simulation of the resampling kernels (csrc/resample.hip: sep_resample_fwd, sep_resample_stream_fwd): the rate
// pairs and lengths of tests/test_resample_gpu.py, every buffer allocated to its exact size and pre-filled with NaN, checked against the definition
// of include/sepkernels.h restated here with plain double loops over the FULL table of K taps.  Built and run by tools/hostsim_resample.py, plain
// or with -fsanitize=address,undefined (a program of its own: the sanitizer's runtime is linked in, nothing is preloaded).  Exit status 0 = all
// within the bounds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
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
static const double PI = 3.14159265358979323846;

// the filter of a conversion (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) and its compact form
struct Filter {
    int o, u, width, K, Kc, D, H;
    std::vector<double> h;             // (u, K)
    std::vector<float> table;          // (Kc, u)
    std::vector<int32_t> first;        // (u)
    Filter(int orig, int nw) {
        const int g = std::gcd(orig, nw);
        o = orig / g;
        u = nw / g;
        const double lpw = 6, base = (o < u ? o : u) * 0.99;
        width = (int)std::ceil(lpw * o / base);
        K = 2 * width + o;
        h.resize((size_t)u * K);
        std::vector<int> lo(u), hi(u);
        Kc = 1;
        for (int p = 0; p < u; ++p) {
            double big = 0;
            for (int k = 0; k < K; ++k) {
                double t = ((double)(k - width) / o - (double)p / u) * base;
                t = t < -lpw ? -lpw : t > lpw ? lpw : t;
                const double w = std::cos(t * PI / lpw / 2), a = t * PI;
                h[(size_t)p * K + k] = (a == 0 ? 1.0 : std::sin(a) / a) * w * w * base / o;
                big = std::fmax(big, std::fabs(h[(size_t)p * K + k]));
            }
            lo[p] = 0;
            hi[p] = K - 1;
            while (std::fabs(h[(size_t)p * K + lo[p]]) < std::ldexp(big, -60)) ++lo[p];
            while (std::fabs(h[(size_t)p * K + hi[p]]) < std::ldexp(big, -60)) --hi[p];
            if (hi[p] - lo[p] + 1 > Kc) Kc = hi[p] - lo[p] + 1;
        }
        first.resize(u);
        table.resize((size_t)Kc * u);
        for (int p = 0; p < u; ++p) {
            first[p] = lo[p] < K - Kc ? lo[p] : K - Kc;
            for (int j = 0; j < Kc; ++j) table[(size_t)j * u + p] = (float)h[(size_t)p * K + first[p] + j];
        }
        D = (width + o - 1) / o * o;
        H = width + D;
    }
    // y[t] of the definition on x (T samples, zero outside), and the sum of |h| |x| behind it
    double at(const float* x, int64_t T, int64_t t, double* mag) const {
        const int64_t i = t / u;
        const int p = (int)(t % u);
        double acc = 0, m = 0;
        for (int k = 0; k < K; ++k) {
            const int64_t s = i * o + k - width;
            if (s < 0 || s >= T) continue;
            acc += h[(size_t)p * K + k] * (double)x[s];
            m += std::fabs(h[(size_t)p * K + k] * (double)x[s]);
        }
        *mag = m;
        return acc;
    }
    double tol(double mag) const { return (Kc + 3) * std::ldexp(1.0, -24) * mag + 1e-30; }
};

// sep_resample_fwd on exactly-sized buffers with pitches of their own: every element below T_out against the double loop, the elements between
// T_out and the pitch untouched, two runs the same bits
static void offline_case(const Filter& f, int R, int64_t T, int extra) {
    ++g_cases;
    const int64_t T_out = (T * f.u + f.o - 1) / f.o, xp = T + extra, yp = T_out + extra;
    std::vector<float> x((size_t)(R * xp)), y((size_t)(R * yp), FNAN), again(y);
    for (int r = 0; r < R; ++r)
        for (int64_t t = 0; t < xp; ++t) x[(size_t)(r * xp + t)] = t < T ? (float)(uniform() * std::ldexp(1.0, r % 13 - 6)) : FNAN;
    int rc = sep_resample_fwd(x.data(), xp, f.table.data(), f.first.data(), y.data(), yp, R, T, T_out, f.o, f.u, f.width, f.Kc, nullptr);
    CHECK(rc == 0, "case %d: fwd: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    rc = sep_resample_fwd(x.data(), xp, f.table.data(), f.first.data(), again.data(), yp, R, T, T_out, f.o, f.u, f.width, f.Kc, nullptr);
    CHECK(rc == 0 && memcmp(y.data(), again.data(), sizeof(float) * y.size()) == 0, "case %d: two runs differ", g_cases);
    for (int r = 0; r < R; ++r)
        for (int64_t t = 0; t < yp; ++t) {
            const float got = y[(size_t)(r * yp + t)];
            if (t >= T_out) {
                CHECK(std::isnan(got), "case %d (o=%d u=%d T=%lld): y[%d][%lld] beyond T_out was written", g_cases, f.o, f.u, (long long)T, r, (long long)t);
                continue;
            }
            double mag;
            const double want = f.at(&x[(size_t)(r * xp)], T, t, &mag);
            CHECK(std::fabs((double)got - want) <= f.tol(mag), "case %d (o=%d u=%d T=%lld): y[%d][%lld] %.9g != %.9g", g_cases, f.o, f.u, (long long)T, r,
                  (long long)t, (double)got, want);
        }
}

// sep_resample_stream_fwd: `streams` slots, a plan of chunk lengths in units of o, the calls naming the slots in reverse order; every slot's pieces
// plus its flush bit for bit sep_resample_fwd of [D zeros | its samples]; a slot that is never named keeps its (NaN) history
static void stream_case(const Filter& f, int streams, const std::vector<int>& plan) {
    ++g_cases;
    int n = 0;
    for (int m : plan) n += m;
    const int64_t T = (int64_t)n * f.o, Tp = T + f.D, T_out = (Tp * f.u + f.o - 1) / f.o;
    const int A = streams > 1 ? streams - 1 : 1;               // the last slot is left out when there is more than one
    std::vector<float> padded((size_t)(A * Tp), 0.f), want((size_t)(A * T_out), FNAN), got((size_t)(A * T_out), FNAN);
    for (int a = 0; a < A; ++a)
        for (int64_t t = 0; t < T; ++t) padded[(size_t)(a * Tp + f.D + t)] = (float)(uniform() * std::ldexp(1.0, a - 2));
    int rc = sep_resample_fwd(padded.data(), Tp, f.table.data(), f.first.data(), want.data(), T_out, A, Tp, T_out, f.o, f.u, f.width, f.Kc, nullptr);
    CHECK(rc == 0, "case %d: fwd: %s", g_cases, sep_last_error());
    std::vector<float> history((size_t)streams * f.H, 0.f);
    for (int e = 0; e < f.H && streams > 1; ++e) history[(size_t)(streams - 1) * f.H + e] = FNAN;
    std::vector<int32_t> slots(A);
    for (int a = 0; a < A; ++a) slots[a] = A - 1 - a;           // row a of a call is slot A - 1 - a
    int64_t pos = 0;
    std::vector<int> calls(plan);
    calls.push_back(f.D / f.o);                                 // the flush: D zero samples
    for (size_t c = 0; c < calls.size(); ++c) {
        const int m = calls[c];
        std::vector<float> chunk((size_t)A * m * f.o, 0.f), y((size_t)A * m * f.u, FNAN);
        if (c + 1 < calls.size())
            for (int a = 0; a < A; ++a) memcpy(&chunk[(size_t)a * m * f.o], &padded[(size_t)(slots[a] * Tp + f.D + pos * f.o)], sizeof(float) * m * f.o);
        rc = sep_resample_stream_fwd(chunk.data(), f.table.data(), f.first.data(), history.data(), y.data(), streams > 1 ? slots.data() : nullptr, A, streams > 1 ? streams : 1, m, f.o,
                                     f.u, f.width, f.Kc, nullptr);
        CHECK(rc == 0, "case %d: stream: %s", g_cases, sep_last_error());
        if (rc != 0) return;
        for (int a = 0; a < A; ++a) memcpy(&got[(size_t)(slots[a] * T_out + pos * f.u)], &y[(size_t)a * m * f.u], sizeof(float) * m * f.u);
        pos += m;
    }
    CHECK(pos * f.u == T_out, "case %d: %lld frames of %d outputs are not T_out = %lld", g_cases, (long long)pos, f.u, (long long)T_out);
    CHECK(memcmp(got.data(), want.data(), sizeof(float) * got.size()) == 0, "case %d (o=%d u=%d streams=%d): the stream is not sep_resample_fwd of the padded signal bit for bit",
          g_cases, f.o, f.u, streams);
    for (int e = 0; e < f.H && streams > 1; ++e) CHECK(std::isnan(history[(size_t)(streams - 1) * f.H + e]), "case %d: the history of a slot that was not named was written", g_cases);
}

// every refused call returns an error with a message before anything is launched (the output keeps its NaN)
static void argument_errors() {
    ++g_cases;
    const Filter f(16000, 8000);
    std::vector<float> x(64, 1.f), y(64, FNAN), hist(64, 0.f);
    const float* tb = f.table.data();
    const int32_t* fi = f.first.data();
    CHECK(sep_resample_fwd(nullptr, 8, tb, fi, y.data(), 4, 1, 8, 4, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null x");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, nullptr, 4, 1, 8, 4, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null y");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 5, 1, 8, 5, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "T_out = ceil"), "T_out 5 of 4");
    CHECK(sep_resample_fwd(x.data(), 7, tb, fi, y.data(), 4, 1, 8, 4, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "x_pitch 7 of 8");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 3, 1, 8, 4, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "y_pitch 3 of 4");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 4, 0, 8, 4, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "R 0");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 4, 1, 0, 0, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "T 0");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 4, 1, 8, 4, 2, 1, 13, 29, nullptr) < 0 && strstr(sep_last_error(), "refused"), "Kc 29 of K 28");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 4, 1, 8, 4, 2, 1, 13, 0, nullptr) < 0 && strstr(sep_last_error(), "refused"), "Kc 0");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 4, 1, 8, 4, 0, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "refused"), "o 0");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 4, 1, 8, 4, 2, 1, 4096, 25, nullptr) < 0 && strstr(sep_last_error(), "staged span"), "width 4096");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 8 * 1025 / 2, 1, 8, 8 * 1025 / 2, 2, 1025, 13, 5, nullptr) < 0 && strstr(sep_last_error(), "more phases"), "u 1025");
    CHECK(sep_resample_fwd(x.data(), 8, tb, fi, y.data(), 8 * 1000 / 2, 1, 8, 8 * 1000 / 2, 2, 1000, 13, 7, nullptr) < 0 && strstr(sep_last_error(), "exceeds the kernels' LDS"), "Kc u 7000");
    CHECK(sep_resample_stream_fwd(x.data(), tb, fi, nullptr, y.data(), nullptr, 1, 1, 2, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null history");
    CHECK(sep_resample_stream_fwd(x.data(), tb, fi, hist.data(), y.data(), nullptr, 1, 2, 2, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "a subset without slots");
    CHECK(sep_resample_stream_fwd(x.data(), tb, fi, hist.data(), y.data(), nullptr, 2, 1, 2, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "A 2 of 1");
    CHECK(sep_resample_stream_fwd(x.data(), tb, fi, hist.data(), y.data(), nullptr, 1, 1, 0, 2, 1, 13, 25, nullptr) < 0 && strstr(sep_last_error(), "bad arguments"), "m 0");
    CHECK(sep_resample_stream_fwd(x.data(), tb, fi, hist.data(), y.data(), nullptr, 1, 1, 1, 2000, 1, 1500, 25, nullptr) < 0 && strstr(sep_last_error(), "history"), "H 3500");
    CHECK(sep_resample_stream_fwd(x.data(), tb, fi, hist.data(), y.data(), nullptr, 1, 1, 5, 1, 1000, 7, 6, nullptr) < 0 && strstr(sep_last_error(), "shorter than the history"), "tiles of 2 frames, H 14");
    for (float v : y) CHECK(std::isnan(v), "a refused call wrote the output");
}

int main() {
    const int pairs[9][2] = {{8000, 16000}, {16000, 8000}, {32000, 16000}, {48000, 8000}, {3, 2}, {2, 3}, {48000, 44100}, {44100, 8000}, {44100, 16000}};
    for (const auto& pr : pairs) {
        const Filter f(pr[0], pr[1]);
        const int by_span = (8192 - f.K) / f.o + 1, by_out = f.u <= 3 ? 2048 : 2048 / f.u, ft = by_span < by_out ? by_span : by_out;      // frames per tile (csrc/resample.hip)
        std::vector<int64_t> Ts;
        if (f.o == 441) Ts = {1, 440, 441, 1000, 4411, (int64_t)ft * f.o + 1};
        else Ts = {1, f.width - 1, f.width, f.width + 1, 3 * f.o - 1, 3 * f.o, 3 * f.o + 1, (int64_t)ft * f.o + 1};
        for (int64_t T : Ts)
            if (T >= 1) offline_case(f, T > 3000 ? 1 : 3, T, T % 3);
    }
    const int spairs[4][2] = {{16000, 8000}, {8000, 16000}, {48000, 44100}, {44100, 8000}};
    for (const auto& pr : spairs) {
        const Filter f(pr[0], pr[1]);
        for (int streams : {1, 3}) {
            stream_case(f, streams, {1});
            stream_case(f, streams, {1, 3, 7, 29});
            if (f.o == 441) stream_case(f, streams, {1, 2, 1});
        }
    }
    stream_case(Filter(8000, 16000), 2, {2100, 1});            // a chunk of two tiles: only the first one touches the history
    argument_errors();
    printf("resample host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
