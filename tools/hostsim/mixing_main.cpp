// Stand-alone driver for the host simulation of the dynamic-mixing kernels (csrc/mixing.hip: sep_mix_draw, sep_mix_render): the test corpus of
// tests/test_dynamic_mixing_gpu.py (3 speakers, 7 utterances of 1, 5, 8, 31, 64, 100, 257 samples) in both sample kinds, every buffer allocated to
// its exact size and pre-filled with NaN, checked bit for bit against the rule of include/sepkernels.h restated here in plain loops; the known
// answers of the header; and HOSTILE plans (an utterance index out of range either way, start >= len, lead negative or >= T, NaN gains), which
// run only on the host.  Built and run by tools/hostsim_mixing.py, plain or with -fsanitize=address,undefined (a program of its own: the
// sanitizer's runtime is linked in, nothing is preloaded).  Exit status 0 = no mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "sepkernels.h"

#pragma clang fp contract(off)

static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                            \
    } while (0)

static const float FNAN = std::numeric_limits<float>::quiet_NaN();
static const int GUARD = SEP_MIX_GUARD;

// ---- the rule, restated ---------------------------------------------------------------------------------------------------------------------
static uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t word(uint64_t seed, uint64_t item, uint64_t k) { return mix64(mix64(seed + 0x9E3779B97F4A7C15ull * (item + 1)) + k); }
static uint64_t below(uint64_t w, uint64_t m) { return ((w >> 32) * m) >> 32; }

template <typename P>
struct Corpus {
    std::vector<P> samples;              // exactly GUARD + total + GUARD elements
    std::vector<int64_t> offsets;
    std::vector<int32_t> spk_first;
    std::vector<float> level;
    int U() const { return (int)offsets.size() - 1; }
    int S() const { return (int)spk_first.size() - 1; }
    int64_t len(int64_t u) const { return offsets[u + 1] - offsets[u]; }
};

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static int32_t rnd16() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (int32_t)((g_rng >> 20) & 0xffff) - 32768;
}

template <typename P>
static Corpus<P> make_corpus(const std::vector<int>& lengths, const std::vector<int32_t>& spk_first) {
    Corpus<P> c;
    c.spk_first = spk_first;
    int64_t pos = GUARD;
    c.offsets.push_back(pos);
    for (int l : lengths) c.offsets.push_back(pos += l);
    c.samples.assign((size_t)(pos + GUARD), (P)0);
    for (size_t u = 0; u < lengths.size(); ++u) {
        for (int64_t e = c.offsets[u]; e < c.offsets[u + 1]; ++e)
            c.samples[(size_t)e] = sizeof(P) == 2 ? (P)rnd16() : (P)std::ldexp((double)rnd16() / 32768.0, (int)(u * 2) - 6);      // fp32: a magnitude per utterance, 2^-6 .. 2^6
        c.level.push_back(0.25f + 0.125f * (float)u);
    }
    return c;
}

struct Row { int64_t s, u, start, lead, g; };
template <typename P>
static Row place(const Corpus<P>& c, int64_t u, int T, uint64_t wpos, uint64_t wgain, int G) {
    const int64_t len = c.len(u);
    Row r{0, u, 0, 0, (int64_t)below(wgain, (uint64_t)G)};
    if (len >= T) r.start = (int64_t)below(wpos, (uint64_t)(len - T + 1));
    else r.lead = (int64_t)below(wpos, (uint64_t)(T - len + 1));
    return r;
}
template <typename P>
static std::vector<Row> draw_item(const Corpus<P>& c, const Corpus<P>* noise, uint64_t seed, uint64_t item, int n, int T, int G, int G_noise) {
    std::vector<Row> rows;
    std::vector<int64_t> chosen;
    for (int i = 0; i < n; ++i) {
        int64_t r = (int64_t)below(word(seed, item, i), (uint64_t)(c.S() - i));
        size_t pos = 0;
        for (size_t q = 0; q < chosen.size(); ++q)
            if (r >= chosen[q]) { ++r; pos = q + 1; }
        chosen.insert(chosen.begin() + pos, r);
        const int64_t u = c.spk_first[r] + (int64_t)below(word(seed, item, n + i), (uint64_t)(c.spk_first[r + 1] - c.spk_first[r]));
        Row row = place(c, u, T, word(seed, item, 2 * n + i), word(seed, item, 3 * n + i), G);
        row.s = r;
        rows.push_back(row);
    }
    if (noise) {
        const int64_t u = (int64_t)below(word(seed, item, 4 * n), (uint64_t)noise->U());
        rows.push_back(place(*noise, u, T, word(seed, item, 4 * n + 1), word(seed, item, 4 * n + 2), G_noise));
    }
    return rows;
}

static std::vector<float> table_of(double lo, double hi, int G) {
    std::vector<float> t(G);
    for (int j = 0; j < G; ++j) t[j] = (float)std::pow(10.0, (G > 1 ? lo + (hi - lo) * j / (G - 1) : lo) / 20.0);
    return t;
}

// the render formula with its clamps and its predicate, the differences formed in 128 bits so that no plan overflows THIS side
template <typename P>
static float render_at(const Corpus<P>& c, const int64_t* row, float g, int64_t t) {
    int64_t u = row[0];
    u = u < 0 ? 0 : u >= c.U() ? c.U() - 1 : u;
    const int64_t len = c.len(u);
    int64_t start = row[1];
    start = start > len - 1 ? len - 1 : start;
    start = start < 0 ? 0 : start;
    const __int128 d = (__int128)t - (__int128)row[2];
    if (d < 0 || d >= (__int128)(len - start)) return 0.f;
    const float scale = sizeof(P) == 2 ? 0x1p-15f : 1.f;
    return g * ((float)c.samples[(size_t)(c.offsets[u] + start + (int64_t)d)] * scale);
}
static bool same_bits(float a, float b) { return (std::isnan(a) && std::isnan(b)) || memcmp(&a, &b, 4) == 0; }

// ---- cases ----------------------------------------------------------------------------------------------------------------------------------
static void known_answers() {
    ++g_cases;
    CHECK(word(1234, 0, 0) == 0x2851ddd6c202938bull && word(1234, 0, 1) == 0xf344a9a461c929aaull && word(1234, 1, 0) == 0xc4c7e6b923620b24ull &&
              word(1234, 1, 1) == 0x22531db8ef59e66full && word(0, 0, 0) == 0x48218226ff3cd4bfull &&
              word(1ull << 63, (1ull << 40) + 3, 31) == 0x568966ec49cd65d1ull,
          "the known answers of word()");
    const Corpus<int16_t> c = make_corpus<int16_t>({1, 5, 8, 31, 64, 100, 257}, {0, 2, 3, 7});
    const int64_t want0[2][5] = {{0, 0, 0, 53, 11}, {2, 6, 66, 0, 177}}, want7[3][5] = {{2, 4, 0, 0, 28}, {0, 0, 0, 49, 49}, {1, 2, 0, 25, 35}};
    const std::vector<Row> r0 = draw_item<int16_t>(c, nullptr, 1234, 0, 2, 64, 256, 0), r7 = draw_item<int16_t>(c, nullptr, 1234, 7, 3, 64, 256, 0);
    for (int i = 0; i < 2; ++i)
        CHECK(r0[i].s == want0[i][0] && r0[i].u == want0[i][1] && r0[i].start == want0[i][2] && r0[i].lead == want0[i][3] && r0[i].g == want0[i][4], "item 0 row %d", i);
    for (int i = 0; i < 3; ++i)
        CHECK(r7[i].s == want7[i][0] && r7[i].u == want7[i][1] && r7[i].start == want7[i][2] && r7[i].lead == want7[i][3] && r7[i].g == want7[i][4], "item 7 row %d", i);
}

// sep_mix_draw for steps step0 .. step0 + 2 against the restatement; the counter advances by one per call
template <typename P>
static void draw_case(const Corpus<P>& c, const Corpus<P>* noise, int B, int n, int T, int64_t step0, int rank, int world, uint64_t seed) {
    ++g_cases;
    const int R = n + (noise ? 1 : 0), G = 256, Gn = 5;
    const std::vector<float> table = table_of(-2.5, 2.5, G), ntable = table_of(-6, 3, Gn);
    std::vector<int64_t> counter(1, step0), plan((size_t)B * R * 4, -777);
    std::vector<float> gain((size_t)B * R, FNAN);
    for (int call = 0; call < 3; ++call) {
        const int rc = sep_mix_draw(c.offsets.data(), c.spk_first.data(), c.U(), c.S(), noise ? noise->offsets.data() : nullptr, noise ? noise->U() : 0, c.level.data(),
                                    table.data(), G, noise ? noise->level.data() : nullptr, noise ? ntable.data() : nullptr, noise ? Gn : 0, counter.data(), (int64_t)seed,
                                    (int64_t)B * world, (int64_t)rank * B, B, n, T, plan.data(), gain.data(), nullptr);
        CHECK(rc == 0, "case %d: draw: %s", g_cases, sep_last_error());
        if (rc != 0) return;
        CHECK(counter[0] == step0 + call + 1, "case %d: the counter holds %lld after call %d from %lld", g_cases, (long long)counter[0], call, (long long)step0);
        for (int b = 0; b < B; ++b) {
            const uint64_t item = (uint64_t)(step0 + call) * (uint64_t)((int64_t)B * world) + (uint64_t)((int64_t)rank * B) + (uint64_t)b;
            const std::vector<Row> rows = draw_item(c, noise, seed, item, n, T, G, Gn);
            for (int i = 0; i < R; ++i) {
                const int64_t* p = &plan[((size_t)b * R + i) * 4];
                const float want = i < n ? c.level[rows[i].u] * table[rows[i].g] : noise->level[rows[i].u] * ntable[rows[i].g];
                CHECK(p[0] == rows[i].u && p[1] == rows[i].start && p[2] == rows[i].lead && p[3] == rows[i].g && same_bits(gain[(size_t)b * R + i], want),
                      "case %d (B=%d n=%d T=%d step %lld): item %d row %d is (%lld, %lld, %lld, %lld), the rule says (%lld, %lld, %lld, %lld)", g_cases, B, n, T,
                      (long long)(step0 + call), b, i, (long long)p[0], (long long)p[1], (long long)p[2], (long long)p[3], (long long)rows[i].u, (long long)rows[i].start,
                      (long long)rows[i].lead, (long long)rows[i].g);
            }
        }
    }
}

// sep_mix_render of `plan` on exactly-sized outputs (`shift` floats into a larger allocation: 0 keeps malloc's alignment, 1 forces the scalar form)
template <typename P>
static void render_case(const Corpus<P>& c, const Corpus<P>* noise, const std::vector<int64_t>& plan, const std::vector<float>& gain, int B, int n, int T, int shift,
                        const char* instance, const char* what) {
    ++g_cases;
    const int R = n + (noise ? 1 : 0);
    std::vector<float> src((size_t)B * n * T + shift, FNAN), mix((size_t)B * T + shift, FNAN), nz(noise ? (size_t)B * T + shift : 0, FNAN), src2(src), mix2(mix), nz2(nz);
    const int kind = sizeof(P) == 2 ? SEP_MIX_INT16 : SEP_MIX_F32;
    const std::vector<P> before(c.samples);
    for (int run = 0; run < 2; ++run) {
        float* s = (run ? src2 : src).data() + shift;
        float* m = (run ? mix2 : mix).data() + shift;
        float* z = noise ? (run ? nz2 : nz).data() + shift : nullptr;
        const int rc = sep_mix_render(c.samples.data(), kind, c.offsets.data(), c.U(), noise ? noise->samples.data() : nullptr, noise ? noise->offsets.data() : nullptr,
                                      noise ? noise->U() : 0, plan.data(), gain.data(), B, n, T, s, m, z, nullptr);
        CHECK(rc == 0, "case %d (%s): render: %s", g_cases, what, sep_last_error());
        if (rc != 0) return;
        CHECK(strcmp(sep_last_kernel(), instance) == 0, "case %d (%s): instance %s, expected %s", g_cases, what, sep_last_kernel(), instance);
    }
    CHECK(memcmp(src.data() + shift, src2.data() + shift, 4 * (size_t)B * n * T) == 0 && memcmp(mix.data() + shift, mix2.data() + shift, 4 * (size_t)B * T) == 0,
          "case %d (%s): two runs differ", g_cases, what);
    CHECK(before == c.samples, "case %d (%s): the corpus was changed", g_cases, what);
    for (int k = 0; k < shift; ++k) CHECK(std::isnan(src[k]) && std::isnan(mix[k]), "case %d (%s): an element in front of an output was written", g_cases, what);
    for (int b = 0; b < B; ++b)
        for (int64_t t = 0; t < T; ++t) {
            float acc = 0.f;
            for (int i = 0; i < R; ++i) {
                const size_t e = (size_t)b * R + i;
                const float want = i < n ? render_at(c, &plan[4 * e], gain[e], t) : render_at(*noise, &plan[4 * e], gain[e], t);
                const float got = i < n ? src[shift + ((size_t)b * n + i) * T + t] : nz[shift + (size_t)b * T + t];
                acc = i == 0 ? want : acc + want;
                CHECK(same_bits(got, want), "case %d (%s): item %d row %d sample %lld is %.9g, the formula says %.9g", g_cases, what, b, i, (long long)t, (double)got, (double)want);
            }
            CHECK(same_bits(mix[shift + (size_t)b * T + t], acc), "case %d (%s): mixture of item %d at %lld is %.9g, the ascending sum %.9g", g_cases, what, b, (long long)t,
                  (double)mix[shift + (size_t)b * T + t], (double)acc);
        }
}

template <typename P>
static void kind_cases(const char* vec_name, const char* scalar_name) {
    const Corpus<P> c = make_corpus<P>({1, 5, 8, 31, 64, 100, 257}, {0, 2, 3, 7});
    const Corpus<P> noise = make_corpus<P>({3, 40, 129}, {0, 3});
    const int BN[3][2] = {{1, 1}, {5, 2}, {3, 3}};
    for (const auto& bn : BN)
        for (int T : {16, 64, 300}) {
            draw_case<P>(c, nullptr, bn[0], bn[1], T, 0, 0, 1, 1234);
            draw_case<P>(c, nullptr, bn[0], bn[1], T, 13, 1, 2, 1234);
            draw_case<P>(c, &noise, bn[0], bn[1], T, 5, 0, 1, 1ull << 63);
        }
    draw_case<P>(c, nullptr, 300, 2, 64, 0, 0, 1, 7);              // more items than threads
    // plans of the rule itself, rendered
    for (int T : {16, 64, 30, 300})
        for (int with_noise = 0; with_noise < 2; ++with_noise) {
            const int B = 5, n = 2 + with_noise, R = n + with_noise;
            std::vector<int64_t> plan;
            std::vector<float> gain;
            const std::vector<float> table = table_of(-2.5, 2.5, 256), ntable = table_of(-6, 3, 5);
            for (int b = 0; b < B; ++b) {
                const std::vector<Row> rows = draw_item(c, with_noise ? &noise : nullptr, 99, (uint64_t)b, n, T, 256, 5);
                for (int i = 0; i < R; ++i) {
                    plan.insert(plan.end(), {rows[i].u, rows[i].start, rows[i].lead, rows[i].g});
                    gain.push_back(i < n ? c.level[rows[i].u] * table[rows[i].g] : noise.level[rows[i].u] * ntable[rows[i].g]);
                }
            }
            const bool vec = T % 4 == 0;
            render_case<P>(c, with_noise ? &noise : nullptr, plan, gain, B, n, T, 0, vec ? vec_name : scalar_name, "drawn plan");
            render_case<P>(c, with_noise ? &noise : nullptr, plan, gain, B, n, T, 1, scalar_name, "drawn plan, outputs offset by one float");
        }
    // every misalignment: start = 0 .. 7 on the last utterance, the last read ends on the last sample of the storage's utterances
    {
        std::vector<int64_t> plan;
        std::vector<float> gain;
        for (int64_t s = 0; s < 8; ++s) {
            plan.insert(plan.end(), {6, 257 - 64 - s, 0, 0});
            plan.insert(plan.end(), {6, 257 - 16 + s - 7, 9 - s, 0});        // (a short tail behind a lead: start + avail ends on the last sample)
            gain.push_back(1.f);
            gain.push_back(-0.5f);
        }
        render_case<P>(c, nullptr, plan, gain, 8, 2, 64, 0, vec_name, "start 0 .. 7 on the last utterance");
        render_case<P>(c, nullptr, plan, gain, 8, 2, 62, 0, scalar_name, "start 0 .. 7 on the last utterance, T = 62");
        for (int64_t s = 0; s < 8; ++s) plan[8 * s + 1] = s;                  // ... and on the first samples of it
        render_case<P>(c, nullptr, plan, gain, 8, 2, 64, 0, vec_name, "start 0 .. 7 from the first sample");
    }
    // hostile plans: the clamp-and-predicate rule, nothing outside the storage is touched (the sanitizer watches)
    {
        const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
        const int64_t rows[][4] = {{-1, 0, 0, 0},      {7, 0, 0, 0},       {big, 3, 0, 0},   {small, 3, 0, 0}, {6, 257, 0, 0},  {6, big, 0, 0},  {6, -5, 0, 0},   {6, small, 0, 0},
                                   {5, 10, -3, 0},     {5, 10, -1000, 0},  {5, 0, small, 0}, {5, 0, big, 0},   {5, 0, 64, 0},   {5, 0, 63, 0},   {0, 0, 17, 0},   {0, 5, -1, 0},
                                   {6, 250, 3, 0},     {6, 256, 0, 0},     {2, 7, 60, 0},    {3, 30, 1, 0},    {4, 63, 62, 0},  {1, 4, 33, 0},   {6, 1, -250, 0}, {6, 0, small + 5, 0}};
        const int B = (int)(sizeof(rows) / sizeof(rows[0])) / 2;
        std::vector<int64_t> plan;
        std::vector<float> gain;
        for (int e = 0; e < 2 * B; ++e) {
            plan.insert(plan.end(), rows[e], rows[e] + 4);
            gain.push_back(e % 5 == 4 ? FNAN : e % 3 == 0 ? -2.f : 0.75f);
        }
        render_case<P>(c, nullptr, plan, gain, B, 2, 64, 0, vec_name, "hostile plan");
        render_case<P>(c, nullptr, plan, gain, B, 2, 63, 0, scalar_name, "hostile plan, T = 63");
        std::vector<int64_t> with_noise;
        std::vector<float> gain3;
        for (int b = 0; b < B; ++b) {
            with_noise.insert(with_noise.end(), plan.begin() + 8 * b, plan.begin() + 8 * b + 8);
            with_noise.insert(with_noise.end(), rows[(2 * b + 5) % (2 * B)], rows[(2 * b + 5) % (2 * B)] + 4);
            gain3.insert(gain3.end(), {gain[2 * b], gain[2 * b + 1], b % 4 == 3 ? FNAN : 1.5f});
        }
        render_case<P>(c, &noise, with_noise, gain3, B, 2, 64, 0, vec_name, "hostile plan with a noise row");
    }
}

// every refused call returns an error with a message before anything is launched
static void argument_errors() {
    ++g_cases;
    const Corpus<int16_t> c = make_corpus<int16_t>({1, 5, 8, 31, 64, 100, 257}, {0, 2, 3, 7});
    const std::vector<float> table = table_of(0, 0, 1);
    std::vector<int64_t> counter(1, 0), plan(64, -777);
    std::vector<float> gain(16, FNAN), out(4 * 64, FNAN);
    auto draw = [&](const int64_t* offsets, int U, int S, const int64_t* noff, int Un, const float* nlev, int G, int B, int n, int T) {
        return sep_mix_draw(offsets, c.spk_first.data(), U, S, noff, Un, c.level.data(), table.data(), G, nlev, table.data(), 1, counter.data(), 1, 2, 0, B, n, T, plan.data(),
                            gain.data(), nullptr);
    };
    const int64_t* off = c.offsets.data();
    CHECK(draw(nullptr, 7, 3, nullptr, 0, nullptr, 1, 2, 2, 16) < 0 && strstr(sep_last_error(), "null pointer"), "null offsets");
    CHECK(draw(off, 7, 3, nullptr, 0, nullptr, 1, 2, 0, 16) < 0 && strstr(sep_last_error(), "n=0"), "n 0");
    CHECK(draw(off, 7, 3, nullptr, 0, nullptr, 1, 2, 9, 16) < 0 && strstr(sep_last_error(), "n=9"), "n 9");
    CHECK(draw(off, 7, 3, nullptr, 0, nullptr, 1, 2, 4, 16) < 0 && strstr(sep_last_error(), "n <= S"), "n 4 of S 3");
    CHECK(draw(off, 2, 3, nullptr, 0, nullptr, 1, 2, 2, 16) < 0 && strstr(sep_last_error(), "S <= U"), "S 3 of U 2");
    CHECK(draw(off, 7, 3, nullptr, 0, nullptr, 0, 2, 2, 16) < 0 && strstr(sep_last_error(), "G >= 1"), "G 0");
    CHECK(draw(off, 7, 3, nullptr, 0, nullptr, 1, 0, 2, 16) < 0 && strstr(sep_last_error(), "B=0"), "B 0");
    CHECK(draw(off, 7, 3, nullptr, 0, nullptr, 1, 65536, 2, 16) < 0 && strstr(sep_last_error(), "65535"), "B 65536");
    CHECK(draw(off, 7, 3, nullptr, 0, nullptr, 1, 2, 2, 0) < 0 && strstr(sep_last_error(), "T=0"), "T 0");
    CHECK(draw(off, 7, 3, off, 0, c.level.data(), 1, 2, 2, 16) < 0 && strstr(sep_last_error(), "noise index"), "a noise index of 0 utterances");
    CHECK(draw(off, 7, 3, off, 7, nullptr, 1, 2, 2, 16) < 0 && strstr(sep_last_error(), "noise index"), "a noise index without levels");
    CHECK(counter[0] == 0 && plan[0] == -777, "a refused draw wrote");
    auto render = [&](const void* samples, int kind, const void* ns, const int64_t* noff, int Un, int B, int n, int T, float* noise) {
        return sep_mix_render(samples, kind, off, 7, ns, noff, Un, plan.data(), gain.data(), B, n, T, out.data(), out.data() + 64, noise, nullptr);
    };
    const void* sm = c.samples.data();
    CHECK(render(nullptr, 0, nullptr, nullptr, 0, 1, 2, 16, nullptr) < 0 && strstr(sep_last_error(), "null pointer"), "null samples");
    CHECK(render(sm, 2, nullptr, nullptr, 0, 1, 2, 16, nullptr) < 0 && strstr(sep_last_error(), "kind=2"), "kind 2");
    CHECK(render(sm, 0, nullptr, nullptr, 0, 1, 9, 16, nullptr) < 0 && strstr(sep_last_error(), "n=9"), "n 9");
    CHECK(render(sm, 0, nullptr, nullptr, 0, 0, 2, 16, nullptr) < 0 && strstr(sep_last_error(), "B=0"), "B 0");
    CHECK(render(sm, 0, nullptr, nullptr, 0, 1, 2, 0, nullptr) < 0 && strstr(sep_last_error(), "T=0"), "T 0");
    CHECK(render(sm, 0, nullptr, nullptr, 0, 1, 2, 16, out.data() + 128) < 0 && strstr(sep_last_error(), "come together"), "a noise row without a noise corpus");
    CHECK(render(sm, 0, sm, off, 7, 1, 2, 16, nullptr) < 0 && strstr(sep_last_error(), "come together"), "a noise corpus without a noise row");
    for (float v : out) CHECK(std::isnan(v), "a refused call wrote the output");
}

int main() {
    known_answers();
    kind_cases<int16_t>("mix_render_vec<int16,8>", "mix_render_scalar<int16>");
    kind_cases<float>("mix_render_vec<float,4>", "mix_render_scalar<float>");
    argument_errors();
    printf("mixing host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
