// Stand-alone driver for the host simulation of the speed-perturbation entry points of csrc/mixing.hip (sep_mix_draw_speed, sep_mix_render_speed):
// the test corpus of tests/test_dynamic_mixing_gpu.py in both sample kinds, every buffer allocated to its exact size and pre-filled with NaN, checked
// bit for bit against the definition of include/sepkernels.h restated here in plain loops.  The filters are Hann-windowed sincs built here with the
// header's limits in mind (any table is a filter to the kernel: the definition reads table, first, Kc and width, whatever they hold); they are laid
// out as the header says.  HOSTILE inputs, which run only on the host: a speed index out of range either way, start >= len', lead negative or >= T, a
// one-sample utterance, descriptor fields and offsets out of bounds.  Built and run by tools/hostsim_mixing.py --speed, plain or with
// -fsanitize=address,undefined (a program of its own: the sanitizer's runtime is linked in, nothing is preloaded).  Exit status 0 = no mismatch.
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
            c.samples[(size_t)e] = sizeof(P) == 2 ? (P)rnd16() : (P)std::ldexp((double)rnd16() / 32768.0, (int)(u * 2) - 6);
        c.level.push_back(0.25f + 0.125f * (float)u);
    }
    return c;
}

// ---- speeds: descriptors and filter buffers as include/sepkernels.h lays them out -----------------------------------------------------------
struct Speeds {
    std::vector<int32_t> desc, first;       // exactly J * SEP_MIX_SPEED_DESC and sum of u entries
    std::vector<float> table;               // exactly sum of Kc u floats
    int J() const { return (int)desc.size() / SEP_MIX_SPEED_DESC; }
    const int32_t* d(int j) const { return &desc[(size_t)j * SEP_MIX_SPEED_DESC]; }
};
static int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }
static Speeds make_speeds(const std::vector<int>& percent) {
    Speeds s;
    const double PI = 3.14159265358979323846;
    for (int P : percent) {
        const int g = gcd(P, 100), o = P / g, u = 100 / g;
        if (o == u) {
            s.desc.insert(s.desc.end(), {1, 1, 0, 1, 0, 0, 100, 0});
            continue;
        }
        const double base = (o < u ? o : u) * 0.99;
        const int width = (int)std::ceil(6.0 * o / base), K = 2 * width + o, Kc = K < 25 ? K : (o > u ? 25 : 13);
        s.desc.insert(s.desc.end(), {o, u, width, Kc, (int32_t)s.table.size(), (int32_t)s.first.size(), P, 0});
        std::vector<int> first(u);
        for (int p = 0; p < u; ++p) {
            const int centre = width + (int)std::floor((double)p * o / u);        // the tap nearest t = 0
            int f = centre - Kc / 2;
            first[p] = f < 0 ? 0 : f > K - Kc ? K - Kc : f;
            s.first.push_back(first[p]);
        }
        const size_t t0 = s.table.size();
        s.table.resize(t0 + (size_t)Kc * u);
        for (int k = 0; k < Kc; ++k)
            for (int p = 0; p < u; ++p) {
                double t = ((double)(first[p] + k - width) / o - (double)p / u) * base;
                t = t < -6 ? -6 : t > 6 ? 6 : t;
                const double w = std::cos(t * PI / 12.0), x = t * PI;
                s.table[t0 + (size_t)k * u + p] = (float)((x == 0 ? 1.0 : std::sin(x) / x) * w * w * base / o);
            }
    }
    return s;
}
static int64_t speed_length(const int32_t* d, int64_t len) {
    const int64_t lp = ((int64_t)d[1] * len + d[0] - 1) / d[0];
    return lp < 1 ? 1 : lp > 0x7fffffff ? 0x7fffffff : lp;
}

struct Row { int64_t u, start, lead, g; int j; };
template <typename P>
static std::vector<Row> draw_item(const Corpus<P>& c, const Corpus<P>* noise, const Speeds& sp, uint64_t seed, uint64_t item, int n, int T, int G, int G_noise) {
    std::vector<Row> rows;
    std::vector<int64_t> chosen;
    auto place = [&](int64_t u, int64_t len, uint64_t wpos, uint64_t wgain, int GG, int j) {
        Row r{u, 0, 0, (int64_t)below(wgain, (uint64_t)GG), j};
        if (len >= T) r.start = (int64_t)below(wpos, (uint64_t)(len - T + 1));
        else r.lead = (int64_t)below(wpos, (uint64_t)(T - len + 1));
        return r;
    };
    for (int i = 0; i < n; ++i) {
        int64_t r = (int64_t)below(word(seed, item, i), (uint64_t)(c.S() - i));
        size_t pos = 0;
        for (size_t q = 0; q < chosen.size(); ++q)
            if (r >= chosen[q]) { ++r; pos = q + 1; }
        chosen.insert(chosen.begin() + pos, r);
        const int64_t u = c.spk_first[r] + (int64_t)below(word(seed, item, n + i), (uint64_t)(c.spk_first[r + 1] - c.spk_first[r]));
        const int j = (int)below(word(seed, item, 4 * n + 3 + i), (uint64_t)sp.J());
        rows.push_back(place(u, speed_length(sp.d(j), c.len(u)), word(seed, item, 2 * n + i), word(seed, item, 3 * n + i), G, j));
    }
    if (noise) {
        const int64_t u = (int64_t)below(word(seed, item, 4 * n), (uint64_t)noise->U());
        rows.push_back(place(u, noise->len(u), word(seed, item, 4 * n + 1), word(seed, item, 4 * n + 2), G_noise, -1));
    }
    return rows;
}

static std::vector<float> table_of(double lo, double hi, int G) {
    std::vector<float> t(G);
    for (int j = 0; j < G; ++j) t[j] = (float)std::pow(10.0, (G > 1 ? lo + (hi - lo) * j / (G - 1) : lo) / 20.0);
    return t;
}

// one sample of one row by the definition, with its clamps and its predicate (differences in 128 bits: no plan overflows THIS side)
template <typename P>
static float render_at(const Corpus<P>& c, const Speeds& sp, const int64_t* row, float g, int j, int64_t t) {
    int64_t u = row[0];
    u = u < 0 ? 0 : u >= c.U() ? c.U() - 1 : u;
    const int64_t len = c.len(u);
    const float scale = sizeof(P) == 2 ? 0x1p-15f : 1.f;
    j = j < -1 ? -1 : j >= sp.J() ? sp.J() - 1 : j;
    const int32_t* d = j >= 0 ? sp.d(j) : nullptr;
    const bool copy = !d || d[0] == d[1];
    const int64_t lenp = copy ? len : speed_length(d, len);
    int64_t start = row[1];
    start = start > lenp - 1 ? lenp - 1 : start;
    start = start < 0 ? 0 : start;
    const __int128 dd = (__int128)t - (__int128)row[2];
    if (dd < 0 || dd >= (__int128)(lenp - start)) return 0.f;
    if (copy) return g * ((float)c.samples[(size_t)(c.offsets[u] + start + (int64_t)dd)] * scale);
    const int o = d[0], uu = d[1], width = d[2], Kc = d[3];
    const int64_t m = start + (int64_t)dd, i = m / uu, p = m % uu;
    double acc = 0.0;
    for (int k = 0; k < Kc; ++k) {
        const int64_t e = i * o + sp.first[(size_t)(d[5] + p)] + k - width;
        const double x = e >= 0 && e < len ? (double)c.samples[(size_t)(c.offsets[u] + e)] : 0.0;
        acc = acc + (double)sp.table[(size_t)(d[4] + (int64_t)k * uu + p)] * x;
    }
    return g * ((float)acc * scale);
}
static bool same_bits(float a, float b) { return (std::isnan(a) && std::isnan(b)) || memcmp(&a, &b, 4) == 0; }

// ---- cases ----------------------------------------------------------------------------------------------------------------------------------
static void known_answers() {
    ++g_cases;
    CHECK(word(1234, 0, 11) == 0x718ad7f33aef0177ull && word(1234, 0, 12) == 0x0de521a7eba82090ull && word(1234, 1, 11) == 0x5f314ef19e801a70ull &&
              word(0, 0, 7) == 0x915f11bbbfb2963dull && word(1ull << 63, (1ull << 40) + 3, 42) == 0xd90fbd8340eb6aa8ull,
          "the known answers of word()");
    CHECK(below(word(1234, 0, 11), 3) == 1 && below(word(1234, 0, 12), 3) == 0 && below(word(1234, 1, 11), 3) == 1 && below(word(0, 0, 7), 3) == 1 &&
              below(word(1ull << 63, (1ull << 40) + 3, 42), 3) == 2,
          "the known speed indices");
}

template <typename P>
static void draw_case(const Corpus<P>& c, const Corpus<P>* noise, const Speeds& sp, int B, int n, int T, int64_t step0, int rank, int world, uint64_t seed) {
    ++g_cases;
    const int R = n + (noise ? 1 : 0), G = 256, Gn = 5;
    const std::vector<float> table = table_of(-2.5, 2.5, G), ntable = table_of(-6, 3, Gn);
    std::vector<int64_t> counter(1, step0), plan((size_t)B * R * 4, -777);
    std::vector<float> gain((size_t)B * R, FNAN);
    std::vector<int32_t> speed((size_t)B * R, -777);
    for (int call = 0; call < 3; ++call) {
        const int rc = sep_mix_draw_speed(c.offsets.data(), c.spk_first.data(), c.U(), c.S(), noise ? noise->offsets.data() : nullptr, noise ? noise->U() : 0, c.level.data(),
                                          table.data(), G, noise ? noise->level.data() : nullptr, noise ? ntable.data() : nullptr, noise ? Gn : 0, counter.data(), (int64_t)seed,
                                          (int64_t)B * world, (int64_t)rank * B, B, n, T, sp.desc.data(), sp.J(), plan.data(), gain.data(), speed.data(), nullptr);
        CHECK(rc == 0, "case %d: draw: %s", g_cases, sep_last_error());
        if (rc != 0) return;
        CHECK(counter[0] == step0 + call + 1, "case %d: the counter holds %lld after call %d from %lld", g_cases, (long long)counter[0], call, (long long)step0);
        for (int b = 0; b < B; ++b) {
            const uint64_t item = (uint64_t)(step0 + call) * (uint64_t)((int64_t)B * world) + (uint64_t)((int64_t)rank * B) + (uint64_t)b;
            const std::vector<Row> rows = draw_item(c, noise, sp, seed, item, n, T, G, Gn);
            for (int i = 0; i < R; ++i) {
                const size_t e = (size_t)b * R + i;
                const int64_t* p = &plan[e * 4];
                const float want = i < n ? c.level[rows[i].u] * table[rows[i].g] : noise->level[rows[i].u] * ntable[rows[i].g];
                CHECK(p[0] == rows[i].u && p[1] == rows[i].start && p[2] == rows[i].lead && p[3] == rows[i].g && speed[e] == rows[i].j && same_bits(gain[e], want),
                      "case %d (B=%d n=%d T=%d step %lld): item %d row %d is (%lld, %lld, %lld, %lld; %d), the rule says (%lld, %lld, %lld, %lld; %d)", g_cases, B, n, T,
                      (long long)(step0 + call), b, i, (long long)p[0], (long long)p[1], (long long)p[2], (long long)p[3], speed[e], (long long)rows[i].u,
                      (long long)rows[i].start, (long long)rows[i].lead, (long long)rows[i].g, rows[i].j);
            }
        }
    }
}

// sep_mix_render_speed on exactly-sized outputs (`shift` floats into a larger allocation: 0 keeps malloc's alignment, 1 forces the scalar stores).
// `ref` = the speeds the expected values are formed with (the same as `sp` unless the descriptors are hostile: then only the sanitizer judges, ref = NULL)
template <typename P>
static void render_case(const Corpus<P>& c, const Corpus<P>* noise, const Speeds& sp, const Speeds* ref, const std::vector<int64_t>& plan, const std::vector<float>& gain,
                        const std::vector<int32_t>& speed, int B, int n, int T, int shift, const char* instance, const char* what) {
    ++g_cases;
    const int R = n + (noise ? 1 : 0);
    std::vector<float> src((size_t)B * n * T + shift, FNAN), mix((size_t)B * T + shift, FNAN), nz(noise ? (size_t)B * T + shift : 0, FNAN), src2(src), mix2(mix), nz2(nz);
    const int kind = sizeof(P) == 2 ? SEP_MIX_INT16 : SEP_MIX_F32;
    const std::vector<P> before(c.samples);
    const std::vector<float> table_before(sp.table);
    for (int run = 0; run < 2; ++run) {
        float* s = (run ? src2 : src).data() + shift;
        float* m = (run ? mix2 : mix).data() + shift;
        float* z = noise ? (run ? nz2 : nz).data() + shift : nullptr;
        const int rc = sep_mix_render_speed(c.samples.data(), kind, c.offsets.data(), c.U(), noise ? noise->samples.data() : nullptr, noise ? noise->offsets.data() : nullptr,
                                            noise ? noise->U() : 0, plan.data(), gain.data(), speed.data(), sp.desc.data(), sp.J(), sp.table.data(), (int64_t)sp.table.size(),
                                            sp.first.data(), (int64_t)sp.first.size(), B, n, T, s, m, z, nullptr);
        CHECK(rc == 0, "case %d (%s): render: %s", g_cases, what, sep_last_error());
        if (rc != 0) return;
        CHECK(strcmp(sep_last_kernel(), instance) == 0, "case %d (%s): instance %s, expected %s", g_cases, what, sep_last_kernel(), instance);
    }
    CHECK(memcmp(src.data() + shift, src2.data() + shift, 4 * (size_t)B * n * T) == 0 && memcmp(mix.data() + shift, mix2.data() + shift, 4 * (size_t)B * T) == 0,
          "case %d (%s): two runs differ", g_cases, what);
    CHECK(before == c.samples && table_before == sp.table, "case %d (%s): an input was changed", g_cases, what);
    for (int k = 0; k < shift; ++k) CHECK(std::isnan(src[k]) && std::isnan(mix[k]), "case %d (%s): an element in front of an output was written", g_cases, what);
    if (!ref) return;          // hostile descriptors: no expected values, the sanitizer judges
    for (int b = 0; b < B; ++b)
        for (int64_t t = 0; t < T; ++t) {
            float acc = 0.f;
            for (int i = 0; i < R; ++i) {
                const size_t e = (size_t)b * R + i;
                const float want = i < n ? render_at(c, *ref, &plan[4 * e], gain[e], speed[e], t) : render_at(*noise, *ref, &plan[4 * e], gain[e], -1, t);
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
    const Speeds near = make_speeds({95, 100, 105}), far = make_speeds({50, 97, 200}), one = make_speeds({100});
    const int BN[3][2] = {{1, 1}, {5, 2}, {3, 3}};
    for (const Speeds* sp : {&near, &far})
        for (const auto& bn : BN)
            for (int T : {16, 64, 300}) {
                draw_case<P>(c, nullptr, *sp, bn[0], bn[1], T, 0, 0, 1, 1234);
                draw_case<P>(c, &noise, *sp, bn[0], bn[1], T, 5, 1, 2, 1ull << 63);
            }
    draw_case<P>(c, nullptr, one, 300, 2, 64, 0, 0, 1, 7);              // more items than threads; one identity speed
    // plans of the rule itself, rendered
    for (const Speeds* sp : {&near, &far})
        for (int T : {16, 64, 30, 300})
            for (int with_noise = 0; with_noise < 2; ++with_noise) {
                const int B = 5, n = 2 + with_noise, R = n + with_noise;
                std::vector<int64_t> plan;
                std::vector<float> gain;
                std::vector<int32_t> speed;
                const std::vector<float> table = table_of(-2.5, 2.5, 256), ntable = table_of(-6, 3, 5);
                for (int b = 0; b < B; ++b) {
                    const std::vector<Row> rows = draw_item(c, with_noise ? &noise : nullptr, *sp, 99, (uint64_t)b, n, T, 256, 5);
                    for (int i = 0; i < R; ++i) {
                        plan.insert(plan.end(), {rows[i].u, rows[i].start, rows[i].lead, rows[i].g});
                        gain.push_back(i < n ? c.level[rows[i].u] * table[rows[i].g] : noise.level[rows[i].u] * ntable[rows[i].g]);
                        speed.push_back(rows[i].j);
                    }
                }
                render_case<P>(c, with_noise ? &noise : nullptr, *sp, sp, plan, gain, speed, B, n, T, 0, T % 4 == 0 ? vec_name : scalar_name, "drawn plan");
                render_case<P>(c, with_noise ? &noise : nullptr, *sp, sp, plan, gain, speed, B, n, T, 1, scalar_name, "drawn plan, outputs offset by one float");
            }
    // every phase and both edges of the longest utterance, the one-sample utterance, a row across the tile boundary
    {
        std::vector<int64_t> plan;
        std::vector<float> gain;
        std::vector<int32_t> speed;
        for (int j = 0; j < 3; ++j) {
            plan.insert(plan.end(), {6, 0, 0, 0, 6, (int64_t)j, 2040 - 7 * j, 0, 0, 0, 1021 + j, 0});
            gain.insert(gain.end(), {1.f, -0.5f, 2.f});
            speed.insert(speed.end(), {j, j, j});
        }
        render_case<P>(c, nullptr, far, &far, plan, gain, speed, 3, 3, 2560, 0, vec_name, "every phase, the one-sample utterance, across the tile boundary");
        render_case<P>(c, nullptr, far, &far, plan, gain, speed, 3, 3, 2559, 0, scalar_name, "the same, T = 2559");
        render_case<P>(c, nullptr, near, &near, plan, gain, speed, 3, 3, 2560, 0, vec_name, "the same at 95, 100, 105");
    }
    // hostile plans and speed indices: the clamp-and-predicate rule, nothing outside the storage is touched (the sanitizer watches)
    {
        const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
        const int64_t rows[][4] = {{-1, 0, 0, 0},      {7, 0, 0, 0},       {big, 3, 0, 0},   {small, 3, 0, 0}, {6, 514, 0, 0},  {6, big, 0, 0},  {6, -5, 0, 0},   {6, small, 0, 0},
                                   {5, 10, -3, 0},     {5, 10, -1000, 0},  {5, 0, small, 0}, {5, 0, big, 0},   {5, 0, 64, 0},   {5, 0, 63, 0},   {0, 0, 17, 0},   {0, 5, -1, 0},
                                   {6, 250, 3, 0},     {6, 513, 0, 0},     {2, 7, 60, 0},    {3, 30, 1, 0},    {4, 63, 62, 0},  {0, 1, 33, 0},   {6, 1, -250, 0}, {6, 0, small + 5, 0}};
        const int32_t picks[] = {0, 1, 2, -1, 3, 100, -2, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max(), 0, 1, 2};
        const int B = (int)(sizeof(rows) / sizeof(rows[0])) / 2;
        std::vector<int64_t> plan;
        std::vector<float> gain;
        std::vector<int32_t> speed;
        for (int e = 0; e < 2 * B; ++e) {
            plan.insert(plan.end(), rows[e], rows[e] + 4);
            gain.push_back(e % 5 == 4 ? FNAN : e % 3 == 0 ? -2.f : 0.75f);
            speed.push_back(picks[(e * 5) % 12]);
        }
        for (const Speeds* sp : {&near, &far}) {
            render_case<P>(c, nullptr, *sp, sp, plan, gain, speed, B, 2, 64, 0, vec_name, "hostile plan");
            render_case<P>(c, nullptr, *sp, sp, plan, gain, speed, B, 2, 63, 0, scalar_name, "hostile plan, T = 63");
        }
        std::vector<int64_t> with_noise;
        std::vector<float> gain3;
        std::vector<int32_t> speed3;
        for (int b = 0; b < B; ++b) {
            with_noise.insert(with_noise.end(), plan.begin() + 8 * b, plan.begin() + 8 * b + 8);
            with_noise.insert(with_noise.end(), rows[(2 * b + 5) % (2 * B)], rows[(2 * b + 5) % (2 * B)] + 4);
            gain3.insert(gain3.end(), {gain[2 * b], gain[2 * b + 1], b % 4 == 3 ? FNAN : 1.5f});
            speed3.insert(speed3.end(), {speed[2 * b], speed[2 * b + 1], 1});          // a speed index on the noise row is not read
        }
        render_case<P>(c, &noise, far, &far, with_noise, gain3, speed3, B, 2, 64, 0, vec_name, "hostile plan with a noise row");
        // hostile descriptors: every field out of bounds in turn, on exactly-sized filter buffers; no expected values, the sanitizer judges
        const int32_t lo = std::numeric_limits<int32_t>::min(), hi = std::numeric_limits<int32_t>::max();
        for (int field = 0; field < 6; ++field)
            for (int32_t value : {lo, -1, 0, 1, 33, 101, 201, 4607, 4608, 100000, hi}) {
                Speeds bad = far;
                for (int j = 0; j < bad.J(); ++j) bad.desc[(size_t)j * SEP_MIX_SPEED_DESC + field] = value;
                render_case<P>(c, nullptr, bad, nullptr, plan, gain, speed, B, 2, 64, 0, vec_name, "hostile descriptors");
            }
        Speeds wild = far;
        for (auto& f : wild.first) f = (&f - wild.first.data()) % 2 ? hi : lo;
        render_case<P>(c, nullptr, wild, nullptr, plan, gain, speed, B, 2, 2560, 0, vec_name, "hostile first[]");
        Speeds tall = far;                                                      // u = 1 with o = 200 over a long row: the span would be 200 samples per output
        for (int j = 0; j < tall.J(); ++j) { tall.desc[(size_t)j * SEP_MIX_SPEED_DESC] = 1; tall.desc[(size_t)j * SEP_MIX_SPEED_DESC + 1] = 100; }
        render_case<P>(c, nullptr, tall, nullptr, plan, gain, speed, B, 2, 2560, 0, vec_name, "descriptors that stretch an utterance a hundredfold");
        for (int j = 0; j < tall.J(); ++j) { tall.desc[(size_t)j * SEP_MIX_SPEED_DESC] = 200; tall.desc[(size_t)j * SEP_MIX_SPEED_DESC + 1] = 1; }
        const Corpus<P> longc = make_corpus<P>({6000, 9}, {0, 1, 2});          // len' = 30 outputs, 200 samples apart: a span of 6026 samples
        std::vector<int64_t> long_rows;
        for (int e = 0; e < 2 * B; ++e) long_rows.insert(long_rows.end(), {0, 0, (int64_t)(e % 7), 0});
        render_case<P>(longc, nullptr, tall, nullptr, long_rows, gain, speed, B, 2, 64, 0, vec_name, "descriptors whose span outgrows the LDS");
    }
}

// every refused call returns an error with a message before anything is launched
static void argument_errors() {
    ++g_cases;
    const Corpus<int16_t> c = make_corpus<int16_t>({1, 5, 8, 31, 64, 100, 257}, {0, 2, 3, 7});
    const Speeds sp = make_speeds({95, 100, 105});
    const std::vector<float> table = table_of(0, 0, 1);
    std::vector<int64_t> counter(1, 0), plan(64, -777);
    std::vector<float> gain(16, FNAN), out(4 * 64, FNAN);
    std::vector<int32_t> speed(16, -777);
    auto draw = [&](const int32_t* desc, int J, int32_t* spd, int n, int B) {
        return sep_mix_draw_speed(c.offsets.data(), c.spk_first.data(), 7, 3, nullptr, 0, c.level.data(), table.data(), 1, nullptr, nullptr, 0, counter.data(), 1, 2, 0, B, n, 16,
                                  desc, J, plan.data(), gain.data(), spd, nullptr);
    };
    CHECK(draw(nullptr, 3, speed.data(), 2, 2) < 0 && strstr(sep_last_error(), "null pointer"), "null descriptors");
    CHECK(draw(sp.desc.data(), 3, nullptr, 2, 2) < 0 && strstr(sep_last_error(), "null pointer"), "null speed");
    CHECK(draw(sp.desc.data(), 0, speed.data(), 2, 2) < 0 && strstr(sep_last_error(), "J=0"), "J 0");
    CHECK(draw(sp.desc.data(), 17, speed.data(), 2, 2) < 0 && strstr(sep_last_error(), "J=17"), "J 17");
    CHECK(draw(sp.desc.data(), 3, speed.data(), 9, 2) < 0 && strstr(sep_last_error(), "n=9"), "n 9");
    CHECK(draw(sp.desc.data(), 3, speed.data(), 2, 0) < 0 && strstr(sep_last_error(), "B=0"), "B 0");
    CHECK(counter[0] == 0 && plan[0] == -777 && speed[0] == -777, "a refused draw wrote");
    auto render = [&](const void* samples, const int32_t* spd, const int32_t* desc, int J, const float* ft, int64_t nt, const int32_t* ff, int64_t nf, int kind, int T) {
        return sep_mix_render_speed(samples, kind, c.offsets.data(), 7, nullptr, nullptr, 0, plan.data(), gain.data(), spd, desc, J, ft, nt, ff, nf, 1, 2, T, out.data(),
                                    out.data() + 64, nullptr, nullptr);
    };
    const void* sm = c.samples.data();
    const int64_t nt = (int64_t)sp.table.size(), nf = (int64_t)sp.first.size();
    CHECK(render(nullptr, speed.data(), sp.desc.data(), 3, sp.table.data(), nt, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "null pointer"), "null samples");
    CHECK(render(sm, nullptr, sp.desc.data(), 3, sp.table.data(), nt, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "null pointer"), "null speed");
    CHECK(render(sm, speed.data(), nullptr, 3, sp.table.data(), nt, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "null pointer"), "null descriptors");
    CHECK(render(sm, speed.data(), sp.desc.data(), 3, nullptr, nt, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "null pointer"), "null table");
    CHECK(render(sm, speed.data(), sp.desc.data(), 0, sp.table.data(), nt, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "J=0"), "J 0");
    CHECK(render(sm, speed.data(), sp.desc.data(), 17, sp.table.data(), nt, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "J=17"), "J 17");
    CHECK(render(sm, speed.data(), sp.desc.data(), 3, sp.table.data(), 0, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "table_numel=0"), "an empty table");
    CHECK(render(sm, speed.data(), sp.desc.data(), 3, sp.table.data(), 16 * 32 * 100 + 1, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "table_numel"), "a table beyond the limits");
    CHECK(render(sm, speed.data(), sp.desc.data(), 3, sp.table.data(), nt, sp.first.data(), 1601, 0, 16) < 0 && strstr(sep_last_error(), "first_numel=1601"), "first beyond the limits");
    CHECK(render(sm, speed.data(), sp.desc.data(), 3, sp.table.data(), nt, sp.first.data(), nf, 2, 16) < 0 && strstr(sep_last_error(), "kind=2"), "kind 2");
    CHECK(render(sm, speed.data(), sp.desc.data(), 3, sp.table.data(), nt, sp.first.data(), nf, 0, 0) < 0 && strstr(sep_last_error(), "T=0"), "T 0");
    CHECK(render((const char*)sm + 1, speed.data(), sp.desc.data(), 3, sp.table.data(), nt, sp.first.data(), nf, 0, 16) < 0 && strstr(sep_last_error(), "aligned"), "odd samples");
    for (float v : out) CHECK(std::isnan(v), "a refused call wrote the output");
}

int main() {
    known_answers();
    kind_cases<int16_t>("mix_render_speed<int16>", "mix_render_speed_scalar<int16>");
    kind_cases<float>("mix_render_speed<float>", "mix_render_speed_scalar<float>");
    argument_errors();
    printf("mixing speed host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
