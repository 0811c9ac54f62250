// Temporal increments of an ensemble: the index maps and the arithmetic of temporal.hip, written as barrier-separated phases over
// "thread tid of a workgroup", as crps_core.h and escore_core.h are.  Compiled for the host (core_side.h) the same phases run one
// thread after the other over a record per thread: tests/host_temporal_main.cpp checks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_tincr_terms).  The rows are r_0 = y when a truth is given, then r_1 .. r_n = x, each [T][F][hw] fp32 read
// as exact numbers.  For row d, anchor t, variable f and lag tau = 1 .. L with t + tau < T, over the hw cells c of the plane
//   dx_c = r_d[t + tau][f][c] - r_d[t][f][c],   dy_c the same increment of the truth
//   S[d][t][f][tau - 1][0..2] = (sum |dx_c|, sum dx_c^2, sum (dx_c - dy_c)^2)
// +0.0 in all three where t + tau >= T, +0.0 in the third without a truth.  The truth's own row goes the same way as every other: its
// e = dx - dx is +0.0 in every cell.  A NaN or an infinity in one of the two planes of an entry makes the entry NaN, in the truth's
// planes the third column of every row; the kernel finds that on the result -- every term is >= 0 and an increment with a non-finite
// end is infinite or NaN, so a sum is non-finite exactly then, and a non-finite sum is written as NaN.  (A dx^2 that overflows fp32 --
// increments beyond 1.8e19 -- ends as NaN too.)
//
// tincr_terms: a workgroup of 256 owns one (d, t, f) anchor plane, or one chunk of CHUNK cells of it (a function of hw alone).  The
// lags go in passes of BATCH = 4 (a pass hands 12 sums to the fixed-order sum of ordered_sum.h, which serves at most 16).  In a pass a
// thread walks the rounds of its chunk; in a round it loads 4 adjacent anchor cells, the same cells of the pass's four later planes and,
// with a truth, of the truth's five planes: ten 16-byte loads in a straight line.  A lag of the pass past L or past the end of the series
// reads plane T - 1 again (the address is clamped, nothing is read out of bounds), forms no term and is +0.0 or nothing at the store.  dx = b - a, |dx|, dx * dx,
// e = dx - dy, e * e are fp32, no multiply fused with an add; every fp32 term joins its double accumulator at once, cells in ascending
// order -- no fp32 chain is kept.  The workgroup folds (N = 12, nan_if_not_finite) and thread s < 12 writes sum s of the pass: to S if
// the plane is one chunk, else to partial[plane][chunk][L][3], which the shared fold kernel (ordered_sum_launch.h) adds in chunk order.
// A pass none of whose lags has a pair writes its zeros without a fold.  No atomics: an entry's bits are fixed by hw alone.
#ifndef C2W_TEMPORAL_CORE_H
#define C2W_TEMPORAL_CORE_H

#include "core_side.h"

#if defined(__clang__)
#define TINCR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TINCR_NO_CONTRACT
#endif

#ifndef TINCR_VISIT  // the host driver counts the (cell, lag) pairs of every anchor here
#define TINCR_VISIT(plane, cell, tau)
#endif
#include "ordered_sum.h"

namespace tincr {

constexpr int THREADS = 256;
constexpr int MAX_L = 24;
constexpr int CHUNK = 4096;       // cells a workgroup owns: 4 rounds of 256 threads, 4 cells each
constexpr int BATCH = 4;          // lags between two folds
constexpr int SUMS = 3 * BATCH;   // sums a thread hands to one fold
constexpr int LDS_DOUBLES = ordered_sum::lds_doubles<SUMS>();
static_assert(THREADS == ordered_sum::THREADS, "the workgroup the fixed-order sum is written for");
static_assert(SUMS * ordered_sum::GROUPS <= THREADS, "fold_groups has a thread per (sum, group)");
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of rounds");
using ordered_sum::nan_if_not_finite;  // the write policy: the kernel finds a non-finite input on the result

typedef float F4 __attribute__((vector_size(16)));  // 16 bytes a load

static C2W_BOTH inline bool supported(int hw, int L) { return hw >= 4 && hw % 4 == 0 && L >= 1 && L <= MAX_L; }

// ---------------------------------------------------------------------------------------------------------------- maps

static C2W_BOTH inline int chunks(int hw) { return (hw + CHUNK - 1) / CHUNK; }
static C2W_BOTH inline int chunk_begin(int c) { return c * CHUNK; }
static C2W_BOTH inline int chunk_end(int hw, int c) { return (c + 1) * CHUNK < hw ? (c + 1) * CHUNK : hw; }
// rounds of the workgroup over chunk c, and the first of the 4 cells thread tid owns in round `it`
static C2W_BOTH inline int rounds(int hw, int c) { return (chunk_end(hw, c) - chunk_begin(c) + 4 * THREADS - 1) / (4 * THREADS); }
static C2W_BOTH inline int cell_of(int c, int it, int tid) { return chunk_begin(c) + (it * THREADS + tid) * 4; }
static C2W_BOTH inline int passes(int L) { return (L + BATCH - 1) / BATCH; }
// lags of anchor t that have a pair
static C2W_BOTH inline int lags_of(int T, int t, int L) { return T - 1 - t < L ? T - 1 - t : L; }
// bytes of partial sums: none while a plane is one chunk
static C2W_BOTH inline long long scratch_bytes(long long rows, long long T, long long F, int hw, int L) {
    return chunks(hw) > 1 ? rows * T * F * chunks(hw) * 3 * L * (long long)sizeof(double) : 0;
}

// ---------------------------------------------------------------------------------------------------------------- phases

struct View {
    const float* x;   // [n_rep][T][F][hw]
    const float* y;   // [T][F][hw] or null
    double* out;      // S [rows T F][L][3] (one chunk a plane) or partial [rows T F][chunks][L][3]
    long long plane;  // (d T + t) F + f
    int chunk;
    int T, F, hw, L;
    double* lds;  // LDS_DOUBLES
};

struct Thread {
    double acc[SUMS];  // [lag of the pass][column]
};

static C2W_HD inline int anchor_of(const View& v) { return (int)((v.plane / v.F) % v.T); }
// plane (t, f) of the row this workgroup owns, and of the truth
static C2W_HD inline const float* own_plane(const View& v, int t) {
    const long long d = v.plane / ((long long)v.T * v.F), f = v.plane % v.F;
    const float* row = v.y ? (d == 0 ? v.y : v.x + (d - 1) * v.T * v.F * v.hw) : v.x + d * v.T * v.F * v.hw;
    return row + ((long long)t * v.F + f) * v.hw;
}
static C2W_HD inline const float* truth_plane(const View& v, int t) { return v.y + ((long long)t * v.F + v.plane % v.F) * v.hw; }

static C2W_HD inline void t_init(Thread& th) {
#pragma unroll
    for (int s = 0; s < SUMS; ++s) th.acc[s] = 0.0;
}

// round `it` of pass `pass`: the lags pass BATCH + 1 .. pass BATCH + BATCH of the thread's 4 cells
template <bool HAS_Y>
static C2W_HD inline void t_round(const View& v, Thread& th, int tid, int pass, int it) {
    TINCR_NO_CONTRACT
    const int cell = cell_of(v.chunk, it, tid);
    if (cell >= chunk_end(v.hw, v.chunk)) return;
    const int t = anchor_of(v), last = v.T - 1;
    F4 b[BATCH], yb[BATCH];
    const F4 a = *(const F4*)(own_plane(v, t) + cell);
#pragma unroll
    for (int k = 0; k < BATCH; ++k) {
        const int tb = t + pass * BATCH + k + 1;
        b[k] = *(const F4*)(own_plane(v, tb < last ? tb : last) + cell);
    }
    F4 ya = {0.f, 0.f, 0.f, 0.f};
    if constexpr (HAS_Y) {
        ya = *(const F4*)(truth_plane(v, t) + cell);
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            const int tb = t + pass * BATCH + k + 1;
            yb[k] = *(const F4*)(truth_plane(v, tb < last ? tb : last) + cell);
        }
    }
#pragma unroll
    for (int k = 0; k < BATCH; ++k) {
        if (pass * BATCH + k + 1 > lags_of(v.T, t, v.L)) break;  // the same for the whole workgroup: its loads were clamped, its sums stay +0.0
        TINCR_VISIT(v.plane, cell, pass * BATCH + k + 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float dx = b[k][c] - a[c];
            const float sq = dx * dx;
            th.acc[k * 3 + 0] += (double)__builtin_fabsf(dx);
            th.acc[k * 3 + 1] += (double)sq;
            if constexpr (HAS_Y) {
                const float dy = yb[k][c] - ya[c];
                const float e = dx - dy;
                const float ee = e * e;
                th.acc[k * 3 + 2] += (double)ee;
            }
        }
    }
}

// the three phases of ordered_sum.h at N = 12: thread s writes sum s of the pass -- lag pass BATCH + s / 3 + 1, column s % 3 -- if the
// lag is one of the L; +0.0 where the lag has no pair and, without a truth, in the third column
static C2W_HD inline void t_stash(const View& v, const Thread& th, int tid) { ordered_sum::stash<SUMS>(v.lds, th.acc, tid); }
static C2W_HD inline void t_fold_groups(const View& v, int tid) { ordered_sum::fold_groups<SUMS>(v.lds, tid); }
static C2W_HD inline void t_store(const View& v, int tid, int pass, bool folded) {
    if (tid >= SUMS) return;
    const int tau = pass * BATCH + tid / 3 + 1, col = tid % 3;
    if (tau > v.L) return;
    double s = 0.0;
    if (folded && tau <= lags_of(v.T, anchor_of(v), v.L) && (col < 2 || v.y)) s = nan_if_not_finite(ordered_sum::fold_total<SUMS>(v.lds, tid));
    v.out[((v.plane * chunks(v.hw) + v.chunk) * v.L + (tau - 1)) * 3 + col] = s;
}
// whether pass `pass` of this anchor has a lag with a pair: the same for the whole workgroup
static C2W_HD inline bool pass_has_pairs(const View& v, int pass) { return pass * BATCH + 1 <= lags_of(v.T, anchor_of(v), v.L); }
static C2W_HD inline void f_fold(const double* partial, double* S, long long entry, int nc, int L) {
    S[entry] = nan_if_not_finite(ordered_sum::fold_parts(partial, entry, nc, 3 * L));
}

}  // namespace tincr
#endif
