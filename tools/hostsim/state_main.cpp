// Stand-alone driver for the host simulation of the state export / import kernels (csrc/online.hip: sep_online_state_row_bytes,
// sep_online_state_export, sep_online_state_import): the kernel cases of tests/test_online_state_gpu.py on buffers allocated to their exact
// sizes, checked byte for byte against the row format (version 1) as include/sepkernels.h documents it, restated here with plain loops.
// Built and run by tools/hostsim_state.py, plain or with -fsanitize=address / thread (a program of its own: the sanitizer's runtime is linked
// in, nothing is preloaded).  Exit status 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sepkernels.h"

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t word() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (uint32_t)(g_seed >> 16);
}
static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (g_bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                            \
    } while (0)

// 16-byte aligned storage of exactly `bytes` bytes (the sanitizer sees the first byte beyond it)
struct blob_t {
    unsigned char* p;
    size_t bytes;
    explicit blob_t(size_t n, int fill) : p(nullptr), bytes(n) {
        if (posix_memalign((void**)&p, 16, n ? n : 16) != 0) abort();
        memset(p, fill, n);
    }
    ~blob_t() { free(p); }
};

struct state_t {
    int Bs, cl, sl, tl;
    int64_t rl;
    std::vector<int64_t> frames;
    std::vector<double> sums;
    std::vector<float> carry, rings, tail;
    state_t(int Bs_, int cl_, int sl_, int64_t rl_, int tl_, bool random) : Bs(Bs_), cl(cl_), sl(sl_), tl(tl_), rl(rl_) {
        frames.resize(Bs);
        sums.resize((size_t)Bs * sl);
        carry.resize((size_t)Bs * cl);
        rings.resize((size_t)Bs * rl);
        tail.resize((size_t)Bs * tl);
        static const uint32_t special[6] = {0x7fc00001u, 0xffa5a5a5u, 0x7f800001u, 0x00000001u, 0x807fffffu, 0x80000000u};
        for (int s = 0; s < Bs; ++s) frames[s] = random ? (int64_t)((1ull << 33) + word()) : 1000 + s;
        for (size_t i = 0; i < sums.size(); ++i) sums[i] = random ? (double)(int32_t)word() / 1024.0 : 77.0 + (double)i;
        std::vector<float>* secs[3] = {&carry, &rings, &tail};
        for (auto* v : secs)
            for (size_t i = 0; i < v->size(); ++i) {
                const uint32_t w = random ? (i < 6 ? special[i] : word()) : 0x40400000u + (uint32_t)(i & 0xffff);      // sentinels: finite, near 3
                memcpy(&(*v)[i], &w, 4);
            }
    }
    float* or_null(std::vector<float>& v) { return v.empty() ? nullptr : v.data(); }
};

static int64_t round16(int64_t a) { return (a + 15) / 16 * 16; }

// the documented row of slot s, into out (row_bytes bytes)
static void pack_row(const state_t& st, int s, unsigned char* out, int64_t rb) {
    memset(out, 0, (size_t)rb);
    memcpy(out, &st.frames[s], 8);
    if (st.sl) memcpy(out + 8, &st.sums[(size_t)s * st.sl], 8 * (size_t)st.sl);
    int64_t at = round16(8 + 8 * (int64_t)st.sl);
    if (st.rl) memcpy(out + at, &st.rings[(size_t)s * st.rl], 4 * (size_t)st.rl);
    at += 4 * st.rl;
    if (st.cl) memcpy(out + at, &st.carry[(size_t)s * st.cl], 4 * (size_t)st.cl);
    at += 4 * (int64_t)st.cl;
    if (st.tl) memcpy(out + at, &st.tail[(size_t)s * st.tl], 4 * (size_t)st.tl);
}

static int do_export(state_t& st, const std::vector<int32_t>& slots, void* blob, int64_t pitch) {
    return sep_online_state_export(slots.data(), (int)slots.size(), st.frames.data(), st.or_null(st.carry), st.cl, st.sums.empty() ? nullptr : st.sums.data(),
                                   st.sl, st.or_null(st.rings), st.rl, st.or_null(st.tail), st.tl, blob, pitch, nullptr);
}
static int do_import(state_t& st, const std::vector<int32_t>& slots, const void* blob, int64_t pitch) {
    return sep_online_state_import(slots.data(), (int)slots.size(), st.frames.data(), st.or_null(st.carry), st.cl, st.sums.empty() ? nullptr : st.sums.data(),
                                   st.sl, st.or_null(st.rings), st.rl, st.or_null(st.tail), st.tl, blob, pitch, nullptr);
}

template <class T>
static bool same_slot(const std::vector<T>& a, int sa, const std::vector<T>& b, int sb, int64_t n) {
    return n == 0 || memcmp(&a[(size_t)sa * n], &b[(size_t)sb * n], sizeof(T) * (size_t)n) == 0;
}

static void state_case(int Bs, const std::vector<int32_t>& slots, int cl, int sl, int64_t rl, int tl) {
    ++g_cases;
    const int A = (int)slots.size();
    const int64_t rb = (int64_t)sep_online_state_row_bytes(cl, sl, rl, tl);
    const int64_t want_rb = round16(round16(8 + 8 * (int64_t)sl) + 4 * (rl + cl + tl));
    CHECK(rb == want_rb && rb % 16 == 0, "row_bytes (%d %d %lld %d): %lld != %lld", cl, sl, (long long)rl, tl, (long long)rb, (long long)want_rb);
    state_t src(Bs, cl, sl, rl, tl, true);
    const state_t src0 = src;
    std::vector<unsigned char> want((size_t)rb);
    // (a) export, rows side by side and with a pitch beyond row_bytes
    blob_t tight((size_t)A * rb, 0xA5);
    for (int64_t pitch : {rb, rb + 32}) {
        blob_t wide((size_t)A * pitch, 0xA5);
        blob_t& b = pitch == rb ? tight : wide;
        CHECK(do_export(src, slots, b.p, pitch) == 0, "export: %s", sep_last_error());
        for (int j = 0; j < A; ++j) {
            pack_row(src0, slots[j], want.data(), rb);
            CHECK(memcmp(b.p + (size_t)j * pitch, want.data(), (size_t)rb) == 0, "export case %d pitch %lld: row %d is not the documented format", g_cases,
                  (long long)pitch, j);
            for (int64_t i = rb; i < pitch; ++i) CHECK(b.p[(size_t)j * pitch + i] == 0xA5, "export case %d: byte %lld beyond row_bytes written", g_cases, (long long)i);
        }
    }
    for (int s = 0; s < Bs; ++s)
        CHECK(src.frames[s] == src0.frames[s] && same_slot(src.sums, s, src0.sums, s, sl) && same_slot(src.rings, s, src0.rings, s, rl) &&
                  same_slot(src.carry, s, src0.carry, s, cl) && same_slot(src.tail, s, src0.tail, s, tl), "export case %d changed slot %d", g_cases, s);
    // (b) import into buffers of another size under another slot list, (c) the other slots keep their sentinels
    const int Bs2 = Bs + 2;
    std::vector<int32_t> slots2;
    for (int j = A - 1; j >= 0; --j) slots2.push_back(slots[j] + 1);
    state_t dst(Bs2, cl, sl, rl, tl, false);
    const state_t dst0 = dst;
    CHECK(do_import(dst, slots2, tight.p, rb) == 0, "import: %s", sep_last_error());
    for (int s = 0; s < Bs2; ++s) {
        int j = -1;
        for (int q = 0; q < A; ++q) if (slots2[q] == s) j = q;
        const state_t& from = j >= 0 ? src0 : dst0;
        const int fs = j >= 0 ? slots[j] : s;
        CHECK(dst.frames[s] == from.frames[fs] && same_slot(dst.sums, s, from.sums, fs, sl) && same_slot(dst.rings, s, from.rings, fs, rl) &&
                  same_slot(dst.carry, s, from.carry, fs, cl) && same_slot(dst.tail, s, from.tail, fs, tl), "import case %d: slot %d (%s) is wrong", g_cases, s,
              j >= 0 ? "named" : "not named");
    }
    // (d) round trip
    blob_t again((size_t)A * rb, 0x5A);
    CHECK(do_export(dst, slots2, again.p, rb) == 0, "export: %s", sep_last_error());
    CHECK(memcmp(again.p, tight.p, (size_t)A * rb) == 0, "case %d: export -> import -> export differs", g_cases);
}

// (e) every refused call returns an error with a message and leaves blob and state alone
static void argument_errors() {
    ++g_cases;
    const std::vector<int32_t> slots = {2, 0};
    state_t st(3, 8, 6, 32, 16, true);
    const state_t st0 = st;
    const int64_t rb = (int64_t)sep_online_state_row_bytes(8, 6, 32, 16);
    blob_t blob(2 * (size_t)(rb + 16), 0xA5);
    const struct { void* b; int64_t pitch; const char* words; } bad[3] = {{nullptr, rb, "bad arguments"}, {blob.p, rb - 16, "row_pitch"}, {blob.p, rb + 8, "multiple of 16"}};
    for (const auto& c : bad)
        for (int imp = 0; imp < 2; ++imp) {
            const int rc = imp ? do_import(st, slots, c.b, c.pitch) : do_export(st, slots, c.b, c.pitch);
            CHECK(rc < 0 && strstr(sep_last_error(), c.words), "a call with %s returned %d: %s", c.words, rc, sep_last_error());
        }
    for (size_t i = 0; i < blob.bytes; ++i) CHECK(blob.p[i] == 0xA5, "a refused call wrote the blob");
    CHECK(st.frames == st0.frames && memcmp(st.rings.data(), st0.rings.data(), 4 * st.rings.size()) == 0, "a refused call wrote the state");
}

int main() {
    state_case(5, {4, 0, 2}, 8, 6, 96, 16);
    state_case(257, {256, 0}, 10, 2, 0, 20);
    state_case(2, {1}, 0, 14, 16, 0);
    state_case(3, {0, 1, 2}, 8, 98, 49152, 24);
    state_case(1, {0}, 3, 2, 16, 3);
    argument_errors();
    printf("online-state host cases: %d cases, %d mismatches\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
