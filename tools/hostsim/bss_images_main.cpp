// Stand-alone driver for the host simulation of the BSS-eval v4 ("images") kernel (csrc/bss.hip: sep_bss_image_scratch_bytes,
// sep_bss_image_energies): the shapes of tests/test_bss_images_gpu.py on buffers allocated to their exact sizes, two rows of different
// lengths, checked against the contract of include/sepkernels.h restated here with plain double loops, at 1e-12 relative.  Samples beyond a
// row's length hold NaN: reading one shows in the result.  Built and run by tools/hostsim_bss_images.py, plain or with
// -fsanitize=address,undefined (a program of its own: the sanitizer's runtime is linked in, nothing is preloaded).  Exit status 0 = all
// within the bound.
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

static int frames_of(int Tb, int W, int H) { return Tb < W ? 0 : (Tb - W + H) / H; }

// rows of noise rounded to fp32; NaN at and beyond the row's length
static std::vector<float> audio(int B, int rows, int T, const std::vector<int32_t>& lengths) {
    std::vector<float> x((size_t)B * rows * T);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < rows; ++i)
            for (int t = 0; t < T; ++t) {
                const double u = uniform();
                x[((size_t)b * rows + i) * T + t] = t < lengths[b] ? (float)u : std::numeric_limits<float>::quiet_NaN();
            }
    return x;
}

static void image_case(int n, int C, int T, int F, int W, int H) {
    ++g_cases;
    const int B = 2, nc = n * C;
    const std::vector<int32_t> lengths = {T, T - H - 1};
    std::vector<float> ref = audio(B, nc, T, lengths), est = audio(B, nc, T, lengths);
    for (int c = 0; c < C; ++c)
        for (int t = H; t < H + 3 && t < T; ++t) ref[(size_t)c * T + t] = 0.f;        // row 0, source 0: three samples of silence
    if (C == 2)
        for (int t = 0; t < 7; ++t) est[(size_t)(nc + 1) * T + t] = -est[(size_t)nc * T + t];   // row 1, source 0: L = -R on seven samples
    std::vector<double> fa((size_t)B * n * C * nc * F), fo((size_t)B * n * C * C * F);
    for (auto& v : fa) v = uniform() / std::sqrt((double)F * nc);
    for (auto& v : fo) v = uniform() / std::sqrt((double)F * C);
    const int nwin = frames_of(T, W, H) + 1, Wx = W + F - 1;
    const size_t exact = 72 * (size_t)B * n * nwin * ((Wx + 1023) / 1024);
    CHECK(sep_bss_image_scratch_bytes(B, n, C, F, W, nwin) == exact, "case %d: the helper's size is not the call's need", g_cases);
    std::vector<double> scratch(exact / sizeof(double), std::nan("")), out((size_t)B * n * nwin * 9, std::nan(""));
    const int rc = sep_bss_image_energies(ref.data(), est.data(), fa.data(), fo.data(), lengths.data(), out.data(), scratch.data(), exact, B, n, C, T, F, W, H,
                                          nwin, nullptr);
    CHECK(rc == 0, "case %d: %s", g_cases, sep_last_error());
    if (rc != 0) return;
    std::vector<double> pall(Wx), pj(Wx);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < n; ++j)
            for (int w = 0; w < nwin; ++w) {
                double want[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (w < frames_of(lengths[b], W, H)) {
                    const float* rb = &ref[(size_t)b * nc * T + (size_t)w * H];
                    const float* eb = &est[((size_t)b * n + j) * C * T + (size_t)w * H];
                    for (int c = 0; c < C; ++c) {
                        for (int t = 0; t < Wx; ++t) {
                            double a = 0.0, o = 0.0;
                            for (int kc = 0; kc < nc; ++kc)
                                for (int tau = 0; tau < F; ++tau)
                                    if (t - tau >= 0 && t - tau < W) a += fa[((((size_t)b * n + j) * C + c) * nc + kc) * F + tau] * (double)rb[(size_t)kc * T + t - tau];
                            for (int c2 = 0; c2 < C; ++c2)
                                for (int tau = 0; tau < F; ++tau)
                                    if (t - tau >= 0 && t - tau < W)
                                        o += fo[((((size_t)b * n + j) * C + c) * C + c2) * F + tau] * (double)rb[((size_t)j * C + c2) * T + t - tau];
                            pall[t] = a;
                            pj[t] = o;
                        }
                        for (int t = 0; t < Wx; ++t) {
                            const double s = t < W ? (double)rb[((size_t)j * C + c) * T + t] : 0.0, e = t < W ? (double)eb[(size_t)c * T + t] : 0.0;
                            const double v[7] = {s, e - s, pj[t] - s, pj[t], pall[t] - pj[t], pall[t], e - pall[t]};
                            for (int q = 0; q < 7; ++q) want[q] += v[q] * v[q];
                        }
                    }
                    for (int t = 0; t < W; ++t) {
                        double rs = 0.0, es = 0.0;
                        for (int c = 0; c < C; ++c) { rs += (double)rb[((size_t)j * C + c) * T + t]; es += (double)eb[(size_t)c * T + t]; }
                        want[7] += rs != 0.0;
                        want[8] += es != 0.0;
                    }
                }
                for (int q = 0; q < 9; ++q) {
                    const double got = out[(((size_t)b * n + j) * nwin + w) * 9 + q];
                    CHECK(q < 7 ? std::fabs(got - want[q]) <= 1e-12 * want[q] : got == want[q], "case %d (b %d, source %d, frame %d, sum %d): %.17g != %.17g", g_cases,
                          b, j, w, q, got, want[q]);
                }
            }
}

// every refused call returns an error with a message before anything is launched (the output keeps its NaN)
static void argument_errors() {
    ++g_cases;
    std::vector<float> x(64, 1.f);
    std::vector<double> f(64, 0.5), out(64, std::nan("")), scratch(64, 0.0);
    const size_t sb = scratch.size() * sizeof(double);
    CHECK(sep_bss_image_energies(nullptr, x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 4, 4, 4, 2, nullptr) < 0 &&
              strstr(sep_last_error(), "null pointer"), "null ref");
    CHECK(sep_bss_image_energies(x.data(), x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 0, 4, 4, 2, nullptr) < 0 &&
              strstr(sep_last_error(), "bad arguments"), "flen 0");
    CHECK(sep_bss_image_energies(x.data(), x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 4, 4, 0, 2, nullptr) < 0 &&
              strstr(sep_last_error(), "bad arguments"), "hop 0");
    CHECK(sep_bss_image_energies(x.data(), x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), sb, 1, 1, 1, 8, 4, 4, 4, 0, nullptr) < 0 &&
              strstr(sep_last_error(), "bad arguments"), "nwin 0");
    CHECK(sep_bss_image_energies(x.data(), x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), sb, 70000, 1, 1, 8, 4, 4, 4, 2, nullptr) < 0 &&
              strstr(sep_last_error(), "grid limit"), "B");
    CHECK(sep_bss_image_energies(x.data(), x.data(), f.data(), f.data(), nullptr, out.data(), scratch.data(), 72 * 2 - 1, 1, 1, 1, 8, 4, 4, 4, 2, nullptr) < 0 &&
              strstr(sep_last_error(), "scratch holds"), "scratch");
    CHECK(sep_bss_image_scratch_bytes(1, 1, 1, 0, 4, 2) == 0 && sep_bss_image_scratch_bytes(0, 1, 1, 4, 4, 2) == 0 && sep_bss_image_scratch_bytes(70000, 1, 1, 4, 4, 2) == 0,
          "scratch size of bad arguments");
    for (double v : out) CHECK(std::isnan(v), "a refused call wrote the output");
}

int main() {
    image_case(2, 2, 300, 8, 100, 100);
    image_case(3, 1, 257, 16, 64, 48);
    image_case(4, 2, 1100, 32, 256, 256);
    image_case(2, 2, 600, 64, 40, 40);
    image_case(2, 2, 4000, 512, 1500, 1500);
    argument_errors();
    printf("bss-eval images host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
