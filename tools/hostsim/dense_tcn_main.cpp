// Stand-alone driver for the host simulation of the dilated unfold kernels (csrc/causal.hip: sep_unfold_dilated, sep_fold_dilated;
// csrc/online.hip: sep_online_unfold_fwd, _sel, _rag): the shapes of tests/test_dense_tcn_gpu.py on buffers allocated to their exact sizes,
// checked against plain loops written from the contracts of include/sepkernels.h.  Built and run by tools/hostsim_dense.py, plain or with
// -fsanitize=address / thread (a program of its own: the sanitizer's runtime is linked in, nothing is preloaded).  Exit status 0 = all equal.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sepkernels.h"

static unsigned g_seed = 12345u;
static float rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((g_seed >> 8) & 0xffff) / 32768.f - 1.f;
}
static int g_bad = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                 \
    } while (0)

static void offline_case(int B, int C, int T, int ldt, int P, int dil, int pad) {
    const size_t nx = (size_t)B * C * ldt, nc = nx * P;
    std::vector<float> x(nx), cols(nc, NAN), dcols(nc), dx(nx, NAN);
    for (size_t i = 0; i < nx; ++i) x[i] = (int)(i % ldt) < T ? rnd() : NAN;
    for (size_t i = 0; i < nc; ++i) dcols[i] = (int)(i % ldt) < T ? rnd() : NAN;
    CHECK(sep_unfold_dilated(x.data(), cols.data(), B, C, T, ldt, P, dil, pad, nullptr) == 0, "sep_unfold_dilated: %s", sep_last_error());
    CHECK(sep_fold_dilated(dcols.data(), dx.data(), B, C, T, ldt, P, dil, pad, nullptr) == 0, "sep_fold_dilated: %s", sep_last_error());
    for (int r = 0; r < B * C; ++r) {
        for (int p = 0; p < P; ++p)
            for (int t = 0; t < ldt; ++t) {
                const int i = t + p * dil - pad;
                const float want = (t < T && i >= 0 && i < T) ? x[(size_t)r * ldt + i] : 0.f;
                const float got = cols[((size_t)r * P + p) * ldt + t];
                CHECK(got == want, "unfold (%d %d %d %d %d %d %d): row %d tap %d frame %d: %g != %g", B, C, T, ldt, P, dil, pad, r, p, t, got, want);
            }
        for (int u = 0; u < ldt; ++u) {
            double want = 0.0, mag = 0.0;
            for (int p = 0; p < P && u < T; ++p) {
                const int i = u - p * dil + pad;
                if (i >= 0 && i < T) { want += dcols[((size_t)r * P + p) * ldt + i]; mag += std::fabs(dcols[((size_t)r * P + p) * ldt + i]); }
            }
            const float got = dx[(size_t)r * ldt + u];
            CHECK(std::fabs(got - want) <= P * std::ldexp(1.0, -24) * mag && !(u >= T && got != 0.f), "fold (%d %d %d %d %d %d %d): row %d frame %d: %g != %g",
                  B, C, T, ldt, P, dil, pad, r, u, got, want);
        }
    }
}

// form 0 plain, 1 _sel, 2 _rag; `calls` calls of A blocks, block j of call k bringing len[k * A + j] frames
static void online_case(int form, int Bs, const std::vector<int>& sel, int C, int calls, const std::vector<int>& len, int P, int d) {
    const int A = (int)sel.size(), D = (P - 1) * d;
    const int64_t stride = (int64_t)C * D + 9, off = 5;
    std::vector<float> ring((size_t)Bs * stride, 7.f);
    for (int j = 0; j < A; ++j)
        for (int64_t i = 0; i < stride; ++i) ring[(size_t)sel[j] * stride + i] = 0.f;
    const std::vector<float> ring0 = ring;
    std::vector<std::vector<float>> seen(A);                    // per stream and channel: every frame so far, behind D zeros
    for (int j = 0; j < A; ++j) seen[j].assign((size_t)C * D, 0.f);
    std::vector<int> count(A, 0);
    std::vector<int32_t> slots(sel.begin(), sel.end());
    for (int k = 0; k < calls; ++k) {
        std::vector<int32_t> offs(A + 1, 0);
        int cap = 0;
        for (int j = 0; j < A; ++j) { offs[j + 1] = offs[j] + len[k * A + j]; cap = len[k * A + j] > cap ? len[k * A + j] : cap; }
        const int used = offs[A], ldt = (used + 127) / 128 * 128;
        std::vector<float> x((size_t)C * ldt, NAN), cols((size_t)C * P * ldt, NAN);
        std::vector<std::vector<float>> ext(A);                 // [history D | chunk n] per channel
        for (int j = 0; j < A; ++j) {
            const int n = len[k * A + j];
            ext[j].resize((size_t)C * (D + n));
            for (int c = 0; c < C; ++c) {
                for (int i = 0; i < D; ++i) ext[j][(size_t)c * (D + n) + i] = seen[j][(size_t)c * D + i];
                for (int f = 0; f < n; ++f) ext[j][(size_t)c * (D + n) + D + f] = x[(size_t)c * ldt + offs[j] + f] = rnd();
            }
        }
        float* rg = ring.data() + off;
        int rc;
        if (form == 0) rc = sep_online_unfold_fwd(x.data(), rg, stride, cols.data(), A, C, cap, ldt, P, d, nullptr);
        else if (form == 1) rc = sep_online_unfold_fwd_sel(x.data(), rg, stride, cols.data(), A, C, cap, ldt, P, d, slots.data(), nullptr);
        else rc = sep_online_unfold_fwd_rag(x.data(), rg, stride, cols.data(), A, C, cap + k % 2, ldt, P, d, slots.data(), offs.data(), nullptr);
        CHECK(rc == 0, "sep_online_unfold_fwd form %d: %s", form, sep_last_error());
        for (int j = 0; j < A; ++j) {
            const int n = len[k * A + j];
            for (int c = 0; c < C; ++c) {
                for (int p = 0; p < P; ++p)
                    for (int f = 0; f < n; ++f)
                        CHECK(cols[((size_t)c * P + p) * ldt + offs[j] + f] == ext[j][(size_t)c * (D + n) + f + p * d], "online unfold form %d call %d block %d", form, k, j);
                for (int i = 0; i < D; ++i) seen[j][(size_t)c * D + i] = ext[j][(size_t)c * (D + n) + n + i];
            }
        }
        for (int r = 0; r < C * P; ++r)
            for (int t = used; t < ldt; ++t) CHECK(cols[(size_t)r * ldt + t] == 0.f, "online unfold form %d call %d: dead column %d not zero", form, k, t);
    }
    for (int s = 0; s < Bs; ++s) {
        int j = -1;
        for (int q = 0; q < A; ++q) if (sel[q] == s) j = q;
        for (int64_t i = 0; i < stride; ++i) {
            const float got = ring[(size_t)s * stride + i];
            float want = ring0[(size_t)s * stride + i];
            if (j >= 0 && i >= off && i < off + (int64_t)C * D) want = seen[j][(size_t)(i - off)];
            CHECK(got == want, "online unfold form %d: ring of slot %d word %lld: %g != %g", form, s, (long long)i, got, want);
        }
    }
}

int main() {
    offline_case(2, 16, 203, 256, 3, 1, 2);
    offline_case(1, 32, 130, 256, 3, 64, 128);
    offline_case(2, 16, 37, 128, 5, 16, 64);
    offline_case(1, 48, 1030, 1152, 3, 4, 8);
    offline_case(1, 16, 100, 128, 2, 8, 4);
    online_case(0, 3, {0, 1, 2}, 16, 2, {5, 5, 5, 5, 5, 5}, 3, 4);
    online_case(0, 2, {0, 1}, 16, 3, {11, 11, 11, 11, 3, 3}, 3, 4);
    online_case(0, 2, {0, 1}, 32, 2, {70, 70, 70, 70}, 5, 16);
    online_case(1, 5, {3, 0}, 16, 2, {6, 6, 6, 6}, 3, 8);
    online_case(1, 4, {2}, 16, 2, {130, 130}, 2, 1);
    online_case(2, 5, {4, 1, 2}, 16, 3, {1, 7, 3, 1, 7, 3, 6, 1, 20}, 3, 2);
    online_case(2, 3, {2, 0, 1}, 16, 2, {1, 7, 3, 40, 2, 90}, 5, 8);
    printf("dense-tcn host cases: %d mismatches\n", g_bad);
    return g_bad ? 1 : 0;
}
