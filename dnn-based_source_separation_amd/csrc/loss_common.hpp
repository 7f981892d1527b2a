// What more than one of the criterion files uses (loss.hip, bss.hip, mixit.hip, assign.hip), defined once:
//   SdrTerms / sdr_terms   the terms of SI-SDR from three inner products (loss.hip's kernels, pair_measure)
//   pair_measure           a measure in dB and the coefficients of its gradient from the same three (mixit.hip, assign.hip)
//   slab_count, BSS_MAX_T  the FIXED-size time slabs of the deterministic two-stage sums and the longest row they take (bss.hip, mixit.hip, assign.hip)
//   sep_bss_reduce         the launch of bss.hip's second stage, for the one caller outside that file (mixit.hip: sep_mixit_gram)
#pragma once
#include "common.hpp"

struct SdrTerms { double alpha, c, S, Nn; };
__device__ __forceinline__ SdrTerms sdr_terms(double a, double ttv, double xxv, double eps) {
    SdrTerms r;
    r.c = ttv + eps;
    r.alpha = a / r.c;
    r.S = r.alpha * r.alpha * ttv + eps;
    double nn = r.alpha * r.alpha * ttv - 2.0 * r.alpha * a + xxv;   // |alpha t - x|^2
    if (nn < 0.0) nn = 0.0;
    r.Nn = nn + eps;
    return r;
}

// the measure of one mixture in dB and the coefficients of d measure / d y = cT x + cE y
__device__ __forceinline__ double pair_measure(const int kind, const double a, const double ttv, const double yy, const double eps, const double tau,
                                               double* cT, double* cE) {
    const double K = 10.0 / log(10.0);
    if (kind == 0) {
        const SdrTerms r = sdr_terms(a, ttv, yy, eps);
        if (cT) {   // sisdr_bwd_kernel's expressions with xx = yy
            *cT = K * (2.0 * r.alpha * ttv / (r.c * r.S) - ((2.0 * r.alpha * ttv - 2.0 * a) / r.c - 2.0 * r.alpha) / r.Nn);
            *cE = K * (-2.0 / r.Nn);
        }
        return 10.0 * log10(r.S / r.Nn);
    }
    double nn = ttv - 2.0 * a + yy;          // |x - y|^2
    if (nn < 0.0) nn = 0.0;
    const double den = nn + (kind == 2 ? tau * ttv : 0.0) + eps;
    if (cT) {
        *cT = 2.0 * K / den;
        *cE = -2.0 * K / den;
    }
    return 10.0 * log10((ttv + eps) / den);
}

constexpr int BSS_MAX_T = 1 << 30;

static inline int64_t slab_count(const int64_t len, const int slab) { return (len + slab - 1) / slab; }

// bss.hip: out[o][r] = part[o][0][r] + part[o][1][r] + ... by bss_reduce_kernel (checks and name: the caller's)
void sep_bss_reduce(const double* part, double* out, int nslab, int inner, int64_t total, hipStream_t stream);
