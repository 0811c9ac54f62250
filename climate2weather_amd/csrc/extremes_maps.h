// Extremes of an ensemble: the index maps and the arithmetic of extremes.hip, written as phases over "thread tid of a workgroup", as
// spells_core.h and crps_core.h are.  Compiled for the host (core_side.h) the same phases run one thread after the other:
// tests/host_extremes_main.cpp walks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_block_extremes_update, c2w_lmoments).  The rows are d = 0 the truth when one is given, then the M members;
// D rows in all.  A SERIES is one (d, f, cell) over time, dir[F] says per variable whether maxima (1) or minima (0) are taken, block b
// holds the absolute hours [b block, (b + 1) block).
//
// THE KEY.  key_of (quantile_core.h) maps the fp32 bit pattern to an unsigned whose order is the order of the values, -0.0 just below
// +0.0, the infinities ordinary values.  dkey = key_of(bits) ^ flip, flip = 0 for maxima and ~0 for minima, turns either direction into
// an unsigned MAXIMUM.  Every non-NaN value has 0x007FFFFF <= key_of <= 0xFF800000 (key_of(-inf) and key_of(+inf)), and so has its
// complement: NONE = 0, the "no value yet" key, is below every dkey of every value in both directions.  A NaN hour contributes NONE, an
// all-NaN block ends as NONE and is stored as the one pattern NAN_BITS.  Integer maxima commute: no bit depends on any order or on how
// the time axis was cut into calls.
//
// block_extremes: a workgroup of 256 owns (row d, variable f, chunk of CHUNK = 1024 cells).  A thread owns 4 adjacent cells: it loads
// their open keys (16 bytes), walks the call's T planes in order with one 16-byte load a plane, UNROLL = 8 loads in flight in a straight
// line -- a step past the end reads plane T - 1 again (the address is clamped) and forms no term --, and where hour t0 + t is the last
// of its block stores the block's four extremes with one 16-byte store at table[d][f][(t0 + t) / block][cell] and starts over from
// NONE.  At the end it stores the open keys where it loaded them.  A block is written exactly once, by the call that holds its last
// hour.  The NaN hours go through one LDS int to one 64-bit add per workgroup.
//
// lmoments: a thread owns V adjacent cells of one row r = d F + f and holds their K x V block extremes in registers, K = n rounded up
// to 8, 16, 32 or 64, (K, V) as crps::cells_per_thread; NaN extremes and the pad rows become +inf and n' counts the rest, the rows are
// sorted by crps::t_sort (crps_core.h is included for it, nothing is copied): the first n' sorted rows are the valid extremes.
//
// THE ARITHMETIC of the sample L-moments, all in double on exactly converted fp32 values, no multiply fused with an add:
//   p = x_(n' / 2)                       the pivot, the middle order statistic
//   e_j = x_(j) - p                      exact while the exponents of the two lie within 2^29 of each other, else one rounding
//   S_r = sum_{j < n'} N_r(j) e_j        ascending j; N_0 = 1, N_1 = j, N_2 = j (j - 1), N_3 = j (j - 1)(j - 2): exact integers
//   b_r = S_r / D_r                      D_0 = n', D_r = n' (n' - 1) .. (n' - r): an exact integer below 2^53, ONE division
//   l1 = p + b_0    l2 = 2 b_1 - b_0    l3 = (6 b_2 - 6 b_1) + b_0    l4 = ((20 b_3 - 30 b_2) + 12 b_1) - b_0
// The weights of l2 .. l4 sum to zero, so b_r of e is b_r of x there and only l1 adds the pivot back.  l_r is NaN where n' < r.
//
// THE BOUND.  u = 2^-53, A = sum_{j < n'} |x_(j) - p|, and (k + 1) u stands for k u / (1 - k u) (k < 10^7).  A term of S_r carries the
// rounding of e_j, of its product and of at most n' - 1 adds, and b_r one division more: n' + 2 roundings, and N_r(j) / D_r <= 1 / n',
// so  |b_r^ - b_r| <= E = (n' + 3) u A / n'  and  |b_r| <= A / n'.  The combinations carry the weights 1, 3, 13, 63 on E and round
// intermediates of at most 1, 3, 13, 63 times A / n' (l2: the difference, 3; l3: two products and two sums, 6 + 6 + 12 + 13 = 37; l4:
// 20 + 30 + 12 + 50 + 62 + 63 = 237), one more unit each for the second-order terms:
//   |l_r^ - l_r| <= c_r(n') u A + [r = 1] u |l1|,   c_r(n') = (W_r (n' + 3) + Q_r) / n',   W = 1, 3, 13, 63,   Q = 1, 4, 38, 240
// (bound_weight / bound_rounds below).  The test takes A and l_r from rational arithmetic, so the kernel's error is the only error.
#ifndef C2W_EXTREMES_MAPS_H
#define C2W_EXTREMES_MAPS_H

#include "core_side.h"

#ifndef EX_VISIT_READ  // the host driver counts here: four cell-hours read; four table entries stored; four open keys loaded / stored;
#define EX_VISIT_READ(d, f, t, cell)  // `cells` block extremes loaded by the L-moment kernel (used: the row is one of the n)
#define EX_VISIT_TABLE(at)
#define EX_VISIT_OPEN_LOAD(at)
#define EX_VISIT_OPEN_STORE(at)
#define EX_VISIT_TABLE_READ(at, cells, used)
#endif
#include "crps_core.h"      // t_sort and the static row walks
#include "events_core.h"    // the LDS and global adds
#include "quantile_core.h"  // key_of: the total order on fp32 bit patterns

namespace extremes {

using events::global_add;
using events::lds_add;
using qnt::bits_of;
using qnt::is_nan_bits;
using qnt::key_of;

constexpr int THREADS = 256;
constexpr int CELLS = 4;                // adjacent cells a thread of the update owns: 16 bytes a load
constexpr int CHUNK = THREADS * CELLS;  // 1024 cells a workgroup of the update owns
constexpr int UNROLL = 8;               // planes loaded in a straight line
constexpr int MAX_BLOCK = 1 << 20, MAX_B = 4096, MAX_T = 1 << 20, MAX_N = 64;
constexpr unsigned NONE = 0u;           // no value yet
constexpr unsigned NAN_BITS = 0x7FC00000u;  // the extreme of a block without a value
static_assert((long long)CHUNK * MAX_T < (1LL << 31), "the NaN count of a workgroup fits its LDS int");
static_assert(MAX_N == crps::MAX_M, "the sorting network's sizes");

typedef float F4 __attribute__((vector_size(16)));
typedef unsigned U4 __attribute__((vector_size(16)));

// ---------------------------------------------------------------------------------------------------------------- the key

static C2W_BOTH inline unsigned flip_of(int maxima) { return maxima ? 0u : 0xFFFFFFFFu; }
static C2W_BOTH inline unsigned dkey_of(unsigned bits, unsigned flip) { return is_nan_bits(bits) ? NONE : key_of(bits) ^ flip; }
static C2W_BOTH inline unsigned extreme_bits(unsigned dkey, unsigned flip) { return dkey == NONE ? NAN_BITS : bits_of(dkey ^ flip); }
static C2W_BOTH inline unsigned bits_of_float(float v) { return __builtin_bit_cast(unsigned, v); }

// ---------------------------------------------------------------------------------------------------------------- block extremes

static C2W_BOTH inline bool update_supported(int hw, int block, int B) {
    return hw >= 4 && hw % 4 == 0 && block >= 1 && block <= MAX_BLOCK && B >= 1 && B <= MAX_B;
}
static C2W_BOTH inline int chunks(int hw) { return (hw + CHUNK - 1) / CHUNK; }
static C2W_BOTH inline int cell_of(int chunk, int tid) { return chunk * CHUNK + tid * CELLS; }
// the blocks whose last hour lies in [t0, t0 + T): [first_closed, end_closed)
static C2W_BOTH inline long long first_closed(long long t0, int block) { return t0 / block; }
static C2W_BOTH inline long long end_closed(long long t0, int T, int block) { return (t0 + T) / block; }

struct BView {
    const float* x;      // [M][T][F][hw]
    const float* y;      // [T][F][hw] or null
    const int* dir;      // [F]
    unsigned* open;      // [D][F][hw]
    float* table;        // [D][F][B][hw]
    long long* invalid;  // [D][F]
    int d, f, chunk;     // what this workgroup owns
    int D, T, F, hw, B, block;
    long long t0;
    int* lds;            // 1 int
};

static C2W_HD inline long long open_at(const BView& v, int cell) { return ((long long)v.d * v.F + v.f) * v.hw + cell; }
static C2W_HD inline long long table_at(const BView& v, long long b, int cell) { return (((long long)v.d * v.F + v.f) * v.B + b) * v.hw + cell; }
static C2W_HD inline const float* row_of(const BView& v) {
    const long long member = (long long)v.T * v.F * v.hw;
    const float* row = v.y ? (v.d == 0 ? v.y : v.x + (v.d - 1) * member) : v.x + v.d * member;
    return row + (long long)v.f * v.hw;
}

static C2W_HD inline void b_zero(const BView& v, int tid) {
    if (tid == 0) v.lds[0] = 0;
}

static C2W_HD inline void b_walk(const BView& v, int tid) {
    const int cell = cell_of(v.chunk, tid);
    if (cell >= v.hw) return;  // hw is a multiple of 4: a thread has its four cells or none
    const unsigned flip = flip_of(v.dir[v.f]);
    EX_VISIT_OPEN_LOAD(open_at(v, cell));
    U4 cur = *(const U4*)(v.open + open_at(v, cell));
    const float* row = row_of(v) + cell;
    const long long stride = (long long)v.F * v.hw;
    const int last = v.T - 1;
    long long b = v.t0 / v.block;
    int left = v.block - (int)(v.t0 % v.block);  // hours to the end of the open block, this one included
    int n_invalid = 0;
    for (int tb = 0; tb < v.T; tb += UNROLL) {
        F4 a[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) a[u] = *(const F4*)(row + (long long)(tb + u < last ? tb + u : last) * stride);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (tb + u > last) break;  // the same for the whole workgroup: its load was clamped, it forms no term
            EX_VISIT_READ(v.d, v.f, tb + u, cell);
#pragma unroll
            for (int c = 0; c < CELLS; ++c) {
                const unsigned bits = bits_of_float(a[u][c]);
                const unsigned k = dkey_of(bits, flip);
                n_invalid += is_nan_bits(bits) ? 1 : 0;
                cur[c] = k > cur[c] ? k : cur[c];
            }
            if (--left == 0) {  // the same for the whole workgroup: the block's last hour
                U4 o;
#pragma unroll
                for (int c = 0; c < CELLS; ++c) o[c] = extreme_bits(cur[c], flip), cur[c] = NONE;
                EX_VISIT_TABLE(table_at(v, b, cell));
                *(U4*)(v.table + table_at(v, b, cell)) = o;
                left = v.block, ++b;
            }
        }
    }
    EX_VISIT_OPEN_STORE(open_at(v, cell));
    *(U4*)(v.open + open_at(v, cell)) = cur;
    if (n_invalid) lds_add(v.lds, n_invalid);
}

static C2W_HD inline void b_flush(const BView& v, int tid) {
    if (tid == 0 && v.lds[0]) global_add(v.invalid + (long long)v.d * v.F + v.f, (long long)v.lds[0]);
}

// ---------------------------------------------------------------------------------------------------------------- L-moments

static C2W_BOTH inline bool lmoments_supported(int hw, int n) { return hw >= 4 && hw % 4 == 0 && n >= 1 && n <= MAX_N; }
static C2W_BOTH inline int rows_of(int n) { return crps::rows_of(n); }
static C2W_BOTH inline int cells_per_thread(int K) { return crps::cells_per_thread(K); }
template <int K>
constexpr int V_OF = K <= 16 ? 4 : K == 32 ? 2 : 1;  // cells_per_thread as a template argument (the host driver holds the two together)
static C2W_BOTH inline int lchunks(int hw, int V) { return (hw + THREADS * V - 1) / (THREADS * V); }
static C2W_BOTH inline int lcell_of(int chunk, int tid, int V) { return (chunk * THREADS + tid) * V; }

// the bound of the header's comment: |l_r^ - l_r| <= (bound_weight(r) (n' + 3) + bound_rounds(r)) / n' * 2^-53 * A  (+ 2^-53 |l1| at r = 1)
static C2W_BOTH inline int bound_weight(int r) { return r == 1 ? 1 : r == 2 ? 3 : r == 3 ? 13 : 63; }
static C2W_BOTH inline int bound_rounds(int r) { return r == 1 ? 1 : r == 2 ? 4 : r == 3 ? 38 : 240; }

struct LView {
    const float* table;  // [R][n][hw]
    double* lmom;        // [R][4][hw]
    int* n_valid;        // [R][hw]
    long long row;       // r
    int chunk;
    int n, hw;
};

// the four moments of one column from its sums: the last lines of THE ARITHMETIC
static C2W_HD inline void moments_of(double p, const double (&S)[4], int nv, double (&l)[4]) {
    CRPS_NO_CONTRACT
    const long long m = nv;
    const double nan = (double)__builtin_nanf("");
    const double d0 = (double)m, d1 = (double)(m * (m - 1)), d2 = (double)(m * (m - 1) * (m - 2)), d3 = (double)(m * (m - 1) * (m - 2) * (m - 3));
    const double b0 = S[0] / d0, b1 = S[1] / d1, b2 = S[2] / d2, b3 = S[3] / d3;
    const double two_b1 = 2.0 * b1, six_b2 = 6.0 * b2, six_b1 = 6.0 * b1, t20 = 20.0 * b3, t30 = 30.0 * b2, t12 = 12.0 * b1;
    const double l3a = six_b2 - six_b1, l4a = t20 - t30, l4b = l4a + t12;
    l[0] = nv >= 1 ? p + b0 : nan;
    l[1] = nv >= 2 ? two_b1 - b0 : nan;
    l[2] = nv >= 3 ? l3a + b0 : nan;
    l[3] = nv >= 4 ? l4b - b0 : nan;
}

template <int K, int V>
static C2W_HD inline void l_cells(const LView& v, int tid) {
    using crps::Pack;
    const int cell = lcell_of(v.chunk, tid, V);
    if (cell >= v.hw) return;  // hw is a multiple of 4 and V divides 4: a thread has its V cells or none
    // K loads in a straight line, as crps::t_fetch issues them: row i reads block min(i, n - 1); the rows from n on ask again for the
    // line the last block's load has just brought in and are replaced by +inf below
    const int n = crps::own_scalar(v.n);
    const float* row = v.table + crps::own_scalar(v.row * v.n * v.hw);
    Pack<V> q[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        EX_VISIT_TABLE_READ(row - v.table + cell, V, i < n);
        q[i] = *(const Pack<V>*)(row + (unsigned)cell);
        row += i + 1 < n ? v.hw : 0;
    }
    crps::Thread<K, V> th;
    int nv[V];
#pragma unroll
    for (int c = 0; c < V; ++c) nv[c] = 0;
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int c = 0; c < V; ++c) th.s[i][c] = __builtin_inff();
    crps::rows_each<0, K>(v.n, CRPS_ROW(r) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const float val = q[r.i].v[c];
            const bool isnan = val != val;
            nv[c] += isnan ? 0 : 1;
            th.s[r.i][c] = isnan ? __builtin_inff() : val;
        }
    });
    crps::t_sort(th);  // the pads and the NaNs, all +inf, end up behind the n' values
    double p[V], S[4][V];
#pragma unroll
    for (int c = 0; c < V; ++c) p[c] = (double)th.s[0][c], S[0][c] = S[1][c] = S[2][c] = S[3][c] = 0.0;
    crps::rows_below<0, K / 2 + 1>(v.n / 2 + 1, CRPS_ROW(r) {
#pragma unroll
        for (int c = 0; c < V; ++c) p[c] = r.i == nv[c] / 2 ? (double)th.s[r.i][c] : p[c];
    });
    crps::rows_below<0, K>(v.n, CRPS_ROW(r) {
        CRPS_NO_CONTRACT
        constexpr double w1 = (double)r.i, w2 = (double)(r.i * (r.i - 1)), w3 = (double)(r.i * (r.i - 1) * (r.i - 2));
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const double diff = (double)th.s[r.i][c] - p[c];
            const double e = r.i < nv[c] ? diff : 0.0;  // a row behind the n' values adds an exact zero
            const double t1 = w1 * e, t2 = w2 * e, t3 = w3 * e;
            S[0][c] += e, S[1][c] += t1, S[2][c] += t2, S[3][c] += t3;
        }
    });
#pragma unroll
    for (int c = 0; c < V; ++c) {
        double l[4];
        const double Sc[4] = {S[0][c], S[1][c], S[2][c], S[3][c]};
        moments_of(p[c], Sc, nv[c], l);
#pragma unroll
        for (int o = 0; o < 4; ++o) v.lmom[(v.row * 4 + o) * v.hw + cell + c] = l[o];
        v.n_valid[v.row * v.hw + cell + c] = nv[c];
    }
}

// K = rows_of(n) picks the instance (host code on either side)
template <typename Fn>
static inline void by_rows(int n, Fn&& fn) {
    const int K = rows_of(n);
    if (K == 8) fn(crps::Row<8>{});
    else if (K == 16) fn(crps::Row<16>{});
    else if (K == 32) fn(crps::Row<32>{});
    else fn(crps::Row<64>{});
}

}  // namespace extremes
#endif
