// The fixed-order sum the ensemble metrics share ("Fixed-order sums": the scheme and the two write policies): what makes a
// plane's sums the same bits whatever else rides in the launch.  No atomics, no tree, no reassociation: every sum below is sequential
// from +0.0.  A thread keeps N double accumulators; stash, barrier, fold_groups, barrier, fold_total, and the metric's own phase stores
// the entry through the policy it names; fold_parts adds a plane's chunks or tiles in a second launch (ordered_sum_launch.h).
// For host and device: the qualifiers come through C2W_HD (core_side.h: empty for the host).  No __global__ code.
#ifndef C2W_ORDERED_SUM_H
#define C2W_ORDERED_SUM_H

#include "core_side.h"

namespace ordered_sum {

constexpr int THREADS = 256;
constexpr int GROUP = 16;  // threads whose accumulators are added in one go; THREADS / GROUP group totals follow
constexpr int GROUPS = THREADS / GROUP;
template <int N>  // doubles of LDS for N sums a thread: the accumulators [N][THREADS], then the group totals [N][GROUPS]
constexpr int lds_doubles() { return N * (THREADS + GROUPS); }

static C2W_HD inline double nan_if_nan(double t) { return t != t ? (double)__builtin_nanf("") : t; }  // +-inf stays
static C2W_HD inline double nan_if_not_finite(double t) { return t - t == 0.0 ? t : (double)__builtin_nanf(""); }

template <int N>  // lds[s THREADS + tid] = sum s of thread tid
static C2W_HD inline void stash(double* lds, const double (&acc)[N], int tid) {
#pragma unroll
    for (int s = 0; s < N; ++s) lds[s * THREADS + tid] = acc[s];
}

template <int N>  // thread s GROUPS + g adds sum s of the threads g GROUP .. g GROUP + GROUP - 1, in thread order
static C2W_HD inline void fold_groups(double* lds, int tid) {
    if (tid >= N * GROUPS) return;
    const double* p = lds + (tid / GROUPS) * THREADS + (tid % GROUPS) * GROUP;
    double t = 0.0;
    for (int j = 0; j < GROUP; ++j) t += p[j];
    lds[N * THREADS + tid] = t;
}

template <int N>  // thread tid < N adds the group totals of sum tid, in group order
static C2W_HD inline double fold_total(const double* lds, int tid) {
    const double* p = lds + N * THREADS + tid * GROUPS;
    double t = 0.0;
    for (int g = 0; g < GROUPS; ++g) t += p[g];
    return t;
}

static C2W_HD inline double fold_strided(const double* p, long long parts, long long stride) {  // p[0] + p[stride] + ..
    double t = 0.0;
    for (long long c = 0; c < parts; ++c) t += p[c * stride];
    return t;
}

// partial [outer][parts][inner] -> entry = o inner + i of [outer][inner]; kde, which has o and i apart, calls fold_strided itself
static C2W_HD inline double fold_parts(const double* partial, long long entry, long long parts, long long inner) {
    return fold_strided(partial + (entry / inner) * parts * inner + entry % inner, parts, inner);
}

}  // namespace ordered_sum
#endif
