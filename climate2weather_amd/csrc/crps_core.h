// Ensemble CRPS and spread-skill: the index maps and the arithmetic of crps.hip, written as barrier-separated phases over "thread tid of
// a workgroup", as kde_core.h is.  Compiled for the host (core_side.h) the same phases run one thread after the other over a record
// per thread: tests/host_crps_main.cpp checks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_crps_terms).  One cell (t, f, c) has the members x_1 .. x_M = x[m][t][f][c] and the truth y = y[t][f][c];
// four non-negative terms per cell
//   A = (1 / M) sum_m |x_m - y|        B = sum_{m < m'} |x_m - x_m'| = sum_{k = 1}^{M - 1} k (M - k) (x_(k + 1) - x_(k))
//   E = (mean_m x_m - y)^2             V = sum_m (x_m - mean x)^2 / (M - 1)      (M = 1: NaN)
// and sums[t][f] = the sum of each over the hw cells of the plane, in double.  A member or a truth that is NaN or infinite makes the
// four terms of its cell, and with them the four sums of its plane, NaN; nothing else.
//
// crps_terms: a workgroup of 256 owns one plane, or one chunk of CHUNK cells of it (a function of hw alone).  A thread owns V
// adjacent cells at a time and holds their K x V member values in registers, K = M rounded up to 8, 16, 32 or 64, (K, V) one of
// (8, 4), (16, 4), (32, 2), (64, 1); the K loads are issued in a straight line (row i reads member min(i, M - 1)) and rows M .. K - 1
// are then set to +inf.  Non-finite values are found ON THE LOADED VALUES (min and max drop a NaN).  The K rows are sorted by Batcher's odd-even merge network of min / max pairs with static indices; the pads end up behind the
// members and every sum below runs over the first M rows only.  Only differences of nearby numbers and sums of non-negative terms are
// formed (a pressure field lies at 101325 and its members differ by 0.05):
//   B from the neighbour gaps x_(k + 1) - x_(k) times the exact weights k (M - k);
//   p = x_(M / 2) the pivot, e_i = x_(i) - p, ebar = (sum e) / M, V = sum (e_i - ebar)^2 / (M - 1), E = ((p - y) + ebar)^2;
//   A = sum |x_(i) - y| / M.
// No multiply is fused with an add (the host run and the NumPy restatement give the same bits).  Identical members give B = V = 0.
// The fp32 terms of a cell join the thread's four double accumulators in cell order; the workgroup folds them by the fixed-order sum
// of ordered_sum.h (N = 4, nan_if_nan) and writes four doubles: to sums if the plane is one chunk, to partial[plane][chunk][4]
// otherwise, which the shared fold kernel adds in chunk order.  No atomics: a plane's bits are fixed by (M, hw).
#ifndef C2W_CRPS_CORE_H
#define C2W_CRPS_CORE_H

#include "core_side.h"

#if defined(__clang__)
#define CRPS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CRPS_NO_CONTRACT
#endif
#include "ordered_sum.h"

namespace crps {

constexpr int THREADS = 256;
constexpr int MAX_M = 64;
constexpr int CHUNK = 4096;             // cells a workgroup owns: 4, 8 or 16 rounds of 256 threads at V = 4, 2, 1
constexpr int LDS_DOUBLES = ordered_sum::lds_doubles<4>();
static_assert(THREADS == ordered_sum::THREADS, "the workgroup the fixed-order sum is written for");
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of rounds at every V");

template <int V>
struct alignas(4 * V) Pack {
    float v[V];
};

static C2W_BOTH inline bool supported(int hw, int M) { return hw >= 4 && hw % 4 == 0 && M >= 1 && M <= MAX_M; }

// ---------------------------------------------------------------------------------------------------------------- maps

static C2W_BOTH inline int rows_of(int M) { return M <= 8 ? 8 : M <= 16 ? 16 : M <= 32 ? 32 : 64; }
static C2W_BOTH inline int cells_per_thread(int K) { return K <= 16 ? 4 : K == 32 ? 2 : 1; }
static C2W_BOTH inline int chunks(int hw) { return (hw + CHUNK - 1) / CHUNK; }
static C2W_BOTH inline int chunk_begin(int c) { return c * CHUNK; }
static C2W_BOTH inline int chunk_end(int hw, int c) { return (c + 1) * CHUNK < hw ? (c + 1) * CHUNK : hw; }
// rounds of the workgroup over chunk c, and the first of the V cells thread tid owns in round `it`
static C2W_BOTH inline int rounds(int hw, int c, int V) { return (chunk_end(hw, c) - chunk_begin(c) + V * THREADS - 1) / (V * THREADS); }
static C2W_BOTH inline int cell_of(int c, int it, int tid, int V) { return chunk_begin(c) + (it * THREADS + tid) * V; }
// bytes of partial sums: none while a plane is one chunk
static C2W_BOTH inline long long scratch_bytes(long long T, long long F, int hw) {
    return chunks(hw) > 1 ? T * F * chunks(hw) * 4 * (long long)sizeof(double) : 0;
}

// ---------------------------------------------------------------------------------------------------------------- phases

struct View {
    const float* x;   // [M][T][F][hw]
    const float* y;   // [T][F][hw]
    double* out;      // sums [T F][4] (one chunk a plane) or partial [T F][chunks][4]
    float* cells;     // [4][T][F][hw] or null
    long long plane;  // t F + f
    int chunk;
    int M, T, F, hw;
    double* lds;  // LDS_DOUBLES
};

template <int K, int V>
struct Thread {
    float s[K][V];
    float y[V];
    double acc[4];
    float rM, rM1;
    int cell, has, bad[V];
};

template <int K, int V>
static C2W_HD inline void t_init(const View& v, Thread<K, V>& th) {
    th.rM = (float)(1.0 / (double)v.M);
    th.rM1 = v.M > 1 ? (float)(1.0 / (double)(v.M - 1)) : 0.f;
    th.acc[0] = th.acc[1] = th.acc[2] = th.acc[3] = 0.0;
}

static C2W_HD inline int not_finite(float a) { return !(__builtin_fabsf(a) < __builtin_inff()); }

// fn(Row<I>) for I = 0 .. min(M, K) - 1: unrolled at compile time, so a row index is never data (a register array indexed by a
// variable would go to scratch memory), left at row M by a branch (M is the same for the whole launch)
template <int I>
struct Row {
    static constexpr int i = I;
};
template <int I, int K, typename Fn>
static C2W_HD inline void rows_from(int M, Fn&& fn) {
    if constexpr (I < K) {
        if (I >= M) return;
        fn(Row<I>{});
        rows_from<I + 1, K>(M, fn);
    }
}
// On the device M goes through an empty asm statement first: every walk then compares rows with a scalar of its own, right where it
// branches.  Without it the compiler computes the K comparisons once per kernel, keeps them as K lane masks in scalar registers and
// spills those (seen: 263 spilled scalar registers and 722 lane reads at K = 64).
#ifdef C2W_CORE_HOST
static inline int own_scalar(int m) { return m; }
static inline long long own_scalar(long long m) { return m; }
#else
static C2W_HD inline int own_scalar(int m) {
    asm volatile("" : "+s"(m));
    return m;
}
static C2W_HD inline long long own_scalar(long long m) {
    asm volatile("" : "+s"(m));
    return m;
}
#endif
template <int I, int K, typename Fn>
static C2W_HD inline void rows_below(int M, Fn&& fn) {
    rows_from<I, K>(own_scalar(M), fn);
}
// the same rows, each behind a branch of its own and none left early: for a walk that fills registers, where leaving early would
// make every later register a value with K + 1 possible origins
template <int I, int K, typename Fn>
static C2W_HD inline void rows_each_from(int M, Fn&& fn) {
    if constexpr (I < K) {
        if (I < M) fn(Row<I>{});
        rows_each_from<I + 1, K>(M, fn);
    }
}
template <int I, int K, typename Fn>
static C2W_HD inline void rows_each(int M, Fn&& fn) {
    rows_each_from<I, K>(own_scalar(M), fn);
}
#define CRPS_ROW(r) [&](auto r) __attribute__((always_inline))

// the thread's V cells of round `it`: the truth and all M members, as wide as V allows; nothing is used before all are asked for
template <int K, int V>
static C2W_HD inline void t_fetch(const View& v, Thread<K, V>& th, int tid, int it) {
    th.cell = cell_of(v.chunk, it, tid, V);
    th.has = th.cell < chunk_end(v.hw, v.chunk);
    if (!th.has) return;
    const long long member = (long long)v.T * v.F * v.hw;
    const Pack<V> g = *(const Pack<V>*)(v.y + v.plane * v.hw + (unsigned)th.cell);
    // K loads in a straight line, none behind a branch (a load that had to be merged with the +inf of an absent row right where it
    // is issued would be waited for there, one load at a time): row i reads member min(i, M - 1), so the rows from M on ask again for
    // the line the last member's load has just brought in, and are replaced by +inf below.  The address is a scalar base of this
    // round's own, one member further per row, and a 32-bit offset per thread: K bases kept for the whole kernel, or K addresses of
    // 64 bits per thread, would fill the register files.
    const int members = own_scalar(v.M);
    const float* row = v.x + own_scalar(v.plane * v.hw);
    Pack<V> q[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        q[i] = *(const Pack<V>*)(row + (unsigned)th.cell);
        row += i + 1 < members ? member : 0;
    }
#pragma unroll
    for (int c = 0; c < V; ++c) th.y[c] = g.v[c], th.bad[c] = not_finite(g.v[c]);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int c = 0; c < V; ++c) th.s[i][c] = __builtin_inff();
    rows_each<0, K>(v.M, CRPS_ROW(r) {
#pragma unroll
        for (int c = 0; c < V; ++c) th.s[r.i][c] = q[r.i].v[c], th.bad[c] |= not_finite(q[r.i].v[c]);
    });
}

// Batcher's odd-even merge sort of the K rows, every one of the V columns at once: 19, 63, 191, 543 pairs at K = 8, 16, 32, 64
template <int K, int V>
static C2W_HD inline void t_sort(Thread<K, V>& th) {
#pragma unroll
    for (int p = 1; p < K; p *= 2)
#pragma unroll
        for (int k = p; k >= 1; k /= 2)
#pragma unroll
            for (int j = k % p; j + k < K; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; ++i)
                    if (i + j + k < K && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
#pragma unroll
                        for (int c = 0; c < V; ++c) {
                            const float a = th.s[i + j][c], b = th.s[i + j + k][c];
                            th.s[i + j][c] = __builtin_fminf(a, b), th.s[i + j + k][c] = __builtin_fmaxf(a, b);
                        }
                    }
}

// the four terms of every column from its sorted rows
template <int K, int V>
static C2W_HD inline void t_terms(const Thread<K, V>& th, int M, float (&o)[4][V]) {
    CRPS_NO_CONTRACT
    float a[V], b[V], es[V], ss[V], p[V], ebar[V];
#pragma unroll
    for (int c = 0; c < V; ++c) a[c] = b[c] = es[c] = ss[c] = 0.f, p[c] = th.s[0][c];
    rows_below<0, K>(M, CRPS_ROW(r) {
        CRPS_NO_CONTRACT
        const float w = (float)(r.i * (M - r.i));
#pragma unroll
        for (int c = 0; c < V; ++c) {
            a[c] += __builtin_fabsf(th.s[r.i][c] - th.y[c]);
            if constexpr (r.i > 0) {
                const float gap = th.s[r.i][c] - th.s[r.i - 1][c];
                const float term = w * gap;
                b[c] += term;
            }
        }
    });
    rows_below<0, K / 2 + 1>(M / 2 + 1, CRPS_ROW(r) {
#pragma unroll
        for (int c = 0; c < V; ++c) p[c] = th.s[r.i][c];
    });
    rows_below<0, K>(M, CRPS_ROW(r) {
#pragma unroll
        for (int c = 0; c < V; ++c) es[c] += th.s[r.i][c] - p[c];
    });
#pragma unroll
    for (int c = 0; c < V; ++c) ebar[c] = es[c] * th.rM;
    rows_below<0, K>(M, CRPS_ROW(r) {
        CRPS_NO_CONTRACT
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const float d = (th.s[r.i][c] - p[c]) - ebar[c];
            const float sq = d * d;
            ss[c] += sq;
        }
    });
#pragma unroll
    for (int c = 0; c < V; ++c) {
        const float t = (p[c] - th.y[c]) + ebar[c];
        o[0][c] = a[c] * th.rM, o[1][c] = b[c], o[2][c] = t * t, o[3][c] = M > 1 ? ss[c] * th.rM1 : __builtin_nanf("");
        if (th.bad[c]) o[0][c] = o[1][c] = o[2][c] = o[3][c] = __builtin_nanf("");
    }
}

template <int K, int V>
static C2W_HD inline void t_cells(const View& v, Thread<K, V>& th) {
    if (!th.has) return;
    t_sort(th);
    float o[4][V];
    t_terms(th, v.M, o);
    Pack<V> out[4];
#pragma unroll
    for (int c = 0; c < V; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s) out[s].v[c] = o[s][c], th.acc[s] += (double)o[s][c];
    if (v.cells) {
        const long long field = (long long)v.T * v.F * v.hw, at = v.plane * v.hw + th.cell;
#pragma unroll
        for (int s = 0; s < 4; ++s) *(Pack<V>*)(v.cells + s * field + at) = out[s];
    }
}

// the three phases of ordered_sum.h at N = 4: thread s writes the workgroup's entry of sum s, an infinite sum stays; f_fold then
// writes sums[entry], entry = plane 4 + s, from the chunks in index order
template <int K, int V>
static C2W_HD inline void t_stash(const View& v, const Thread<K, V>& th, int tid) { ordered_sum::stash<4>(v.lds, th.acc, tid); }
static C2W_HD inline void t_fold_groups(const View& v, int tid) { ordered_sum::fold_groups<4>(v.lds, tid); }
static C2W_HD inline void t_fold_store(const View& v, int tid) {
    if (tid >= 4) return;
    const double t = ordered_sum::fold_total<4>(v.lds, tid);
    const int nc = chunks(v.hw);
    v.out[(v.plane * nc + v.chunk) * 4 + tid] = ordered_sum::nan_if_nan(t);
}
static C2W_HD inline void f_fold(const double* partial, double* sums, long long entry, int nc) {
    sums[entry] = ordered_sum::nan_if_nan(ordered_sum::fold_parts(partial, entry, nc, 4));
}

}  // namespace crps
#endif
