// Block moments at the observation grid: the index maps and the arithmetic of blockmoments.hip, written as phases over "thread tid of
// a workgroup", as comoments_maps.h and extremes_maps.h are.  Compiled for the host (core_side.h) the same phases run one thread after
// the other: tests/host_blockmoments_main.cpp walks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_block_moments).  The rows are d = 0 the truth when one is given, then the M members; D rows in all.  A
// PLANE is one (d, t, f) field of H x W cells, a BLOCK one of its h x w = (H / S) x (W / S) tiles of S x S cells x[r][c].
//
// PIVOT.  P = x[0][0] of the block, the fp32 value kept as its bits; with a truth PT is the same cell of the truth's block.
//
// SUMS.  e[r][c] = (double)x[r][c] - (double)P and eT[r][c] = (double)y[r][c] - (double)PT: double subtractions of exactly converted
// fp32 values.  No multiply is fused with an add, every product is rounded on its own, every accumulator is a plain s = s + term
// that starts as +0.0:
//   column sums, rows in order     A_c = sum_r e[r][c]     Q_c = sum_r e[r][c] e[r][c]     X_c = sum_r e[r][c] eT[r][c]
//   block sums, columns in order   S1 = sum_c A_c          S2 = sum_c Q_c                  X = sum_c X_c
// NS = 3 entries (S1, S2, X) with a truth, 2 without.  Row 0 carries the truth against itself: eT = e, so X = S2.
//
// VALID.  n is the number of the block's cells whose fp32 bits are finite (exponent field not all ones; an infinity is invalid, not
// a value).  A block with n < S^2 writes the canonical NaN 0x7ff8000000000000 to S1 and S2; X is that NaN if the block or the
// truth's block is invalid.  n and the pivot's bits are written as they are.
//
// A sum is never -0.0 (it starts as +0.0, and round-to-nearest gives -0.0 only from (-0.0) + (-0.0)), but a TERM can be: x = -0.0
// against P = +0.0 gives e = -0.0.  So no route may start an accumulator with its first term instead of +0.0.
//
// BIT FOR BIT.  The order above is the whole definition: the kernel, the torch route (S vector adds over the rows, then S over the
// columns) and the NumPy reference give the same bits, at every position of a launch.
//
// block_moments<S, TRUTH>, S in {4, 8, 16, 32}.  An ITEM is (plane, block row, quad of 4 adjacent columns); the items of a row's T F
// planes are numbered flat, item = (plane (H / S) + block row) (W / 4) + quad, and a thread owns one.  It walks the item's S rows with
// 16-byte loads (and the truth's rows), GROUP = 8 rows at a time, all loads of a group issued before any use, and keeps the 4 x NS
// column accumulators and its finite counts in registers.  The pivot is one more 4-byte load of the block's first cell: a line the
// block's first quad reads anyway.  A workgroup of 256 takes 256 consecutive items.  A block's S / 4 quads are consecutive items and
// S / 4 divides 256 and W / 4, so no block straddles a workgroup and a ragged last workgroup is the only edge.  b_walk stashes the
// column sums and the counts in LDS ([NS][4][256] doubles and [2][256] ints: 26 KiB); after one barrier b_fold -- the first thread of
// each block -- adds the S columns in order and stores n, the pivot and the sums with plain stores.  No atomics, no scratch.
//
// WHY THE PIVOT.  It removes the field's magnitude before any product and any sum: at 101325 +- 0.5 Pa the terms are of size 0.25.
// An fp32 avg_pool2d of the same field is off by more than the field's standard deviation at S = 32.
//
// THE BOUND.  u = 2^-53, and (k + 1) u stands for k u / (1 - k u), as in comoments_maps.h.  Against exact rational arithmetic on the
// exact fp32 values, with e the EXACT differences: a term reaches its block sum through the chain of S adds of its column and the S
// adds over the columns, depth 2 S, of which the first add of either chain is exact (+0.0 + a): at most 2 S - 2 roundings.  The
// difference e is rounded once where the exponents of x and P are far apart (none within 2^29 of each other), so
//   |S1^ - S1| <= (2 S - 1 + 1) u sum |e|               = 2 S u sum |e|.
// A product carries the roundings of its two factors and its own: 2 S + 1 roundings,
//   |S2^ - S2| <= (2 S + 2) u sum |e e|,      |X^ - X| <= (2 S + 2) u sum |e eT|.
// Nothing underflows: a nonzero |e| is at least 2^-149, a nonzero product at least 2^-298.  (bound_rounds below.)
#ifndef C2W_BLOCKMOMENTS_MAPS_H
#define C2W_BLOCKMOMENTS_MAPS_H

#include "core_side.h"

#ifndef BM_VISIT_READ  // the host driver counts here: 4 cells of row d's plane read at cell index `at`; one block's outputs stored
#define BM_VISIT_READ(d, plane, at)
#define BM_VISIT_STORE(d, plane, block)
#endif

#if defined(__clang__)
#define BM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BM_NO_CONTRACT
#endif

namespace blockmoments {

constexpr int THREADS = 256;
constexpr int GROUP = 8;  // rows whose loads are issued before any use
constexpr unsigned long long CANONICAL_NAN = 0x7ff8000000000000ull;

static C2W_BOTH constexpr bool size_ok(int s) { return s == 4 || s == 8 || s == 16 || s == 32; }
static C2W_BOTH constexpr int entries(bool truth) { return truth ? 3 : 2; }
static C2W_BOTH constexpr int group_rows(int S) { return S < GROUP ? S : GROUP; }
static C2W_BOTH inline bool supported(int H, int W, int s) { return size_ok(s) && H >= s && W >= s && H % s == 0 && W % s == 0; }
static C2W_BOTH inline long long items_per_plane(int H, int W, int s) { return (long long)(H / s) * (W / 4); }
// the items of one row's planes, and the workgroups that take them
static C2W_BOTH inline long long row_items(long long planes, int H, int W, int s) { return planes * items_per_plane(H, W, s); }
static C2W_BOTH inline long long chunks(long long items) { return (items + THREADS - 1) / THREADS; }

// the bound of the header's comment, in units of u = 2^-53 times the sum of absolute terms
static C2W_BOTH inline long long bound_rounds(int s, bool product) { return 2 * s + (product ? 2 : 0); }

static C2W_BOTH inline bool finite_bits(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7F800000u) != 0x7F800000u; }

static C2W_HD inline float lane(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

struct View {
    const float* x;  // [M][planes][H][W]
    const float* y;  // [planes][H][W] or null
    int* n;          // [D][planes][h][w]
    float* pivot;    // [D][planes][h][w]
    double* sums;    // [D][planes][NS][h][w]
    int d, chunk;    // what this workgroup owns: a row and 256 consecutive items of it
    int planes;      // T F
    int items;       // planes h (W / 4): fits an int (the launcher checks)
    int H, W;
    double* lds_sums;  // [NS][4][THREADS]
    int* lds_count;    // [2][THREADS]: the finite cells of the item, of the truth's item
};

template <int S, bool TRUTH>
static C2W_HD inline void b_walk(const View& v, int tid) {
    BM_NO_CONTRACT
    constexpr int G = group_rows(S), NS = entries(TRUTH);
    const int item = v.chunk * THREADS + tid;
    if (item >= v.items) return;  // the ragged last workgroup; a block's quads are all there or none is
    const int W4 = v.W / 4, per_plane = (v.H / S) * W4;
    const int plane = item / per_plane, rem = item % per_plane, br = rem / W4, quad = rem % W4;
    const int col = quad / (S / 4) * S;  // the block's first column
    const long long hw = (long long)v.H * v.W, member = (long long)v.planes * hw;
    const long long at = plane * hw + (long long)br * S * v.W;  // the block row's first cell in its plane
    const float* row = (TRUTH ? (v.d == 0 ? v.y : v.x + (v.d - 1) * member) : v.x + v.d * member) + at;
    const float* tru = TRUTH ? v.y + at : row;
    const float P = row[col], PT = TRUTH ? tru[col] : P;
    const double p = (double)P, pt = (double)PT;
    double A[4], Q[4], X[4];
    int fin = 0, fin_t = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) A[c] = 0.0, Q[c] = 0.0, X[c] = 0.0;
    for (int r0 = 0; r0 < S; r0 += G) {
        float4 a[G], b[TRUTH ? G : 1];
#pragma unroll
        for (int r = 0; r < G; ++r) {
            BM_VISIT_READ(v.d, plane, (long long)(br * S + r0 + r) * v.W + 4 * quad);
            a[r] = *(const float4*)(row + (long long)(r0 + r) * v.W + 4 * quad);
            if (TRUTH) b[r] = *(const float4*)(tru + (long long)(r0 + r) * v.W + 4 * quad);
        }
#pragma unroll
        for (int r = 0; r < G; ++r) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float xv = lane(a[r], c);
                const double e = (double)xv - p;
                const double q = e * e;
                fin += finite_bits(xv) ? 1 : 0;
                A[c] = A[c] + e;
                Q[c] = Q[c] + q;
                if (TRUTH) {
                    const float yv = lane(b[TRUTH ? r : 0], c);
                    const double eT = (double)yv - pt;
                    const double x = e * eT;
                    fin_t += finite_bits(yv) ? 1 : 0;
                    X[c] = X[c] + x;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        v.lds_sums[(0 * 4 + c) * THREADS + tid] = A[c];
        v.lds_sums[(1 * 4 + c) * THREADS + tid] = Q[c];
        if (TRUTH) v.lds_sums[((NS - 1) * 4 + c) * THREADS + tid] = X[c];
    }
    v.lds_count[tid] = fin;
    v.lds_count[THREADS + tid] = TRUTH ? fin_t : fin;
}

template <int S, bool TRUTH>
static C2W_HD inline void b_fold(const View& v, int tid) {
    BM_NO_CONTRACT
    constexpr int NS = entries(TRUTH), QUADS = S / 4;
    const int item = v.chunk * THREADS + tid;
    if (item >= v.items || tid % QUADS != 0) return;  // the first thread of each block
    const int W4 = v.W / 4, h = v.H / S, w = v.W / S, per_plane = h * W4;
    const int plane = item / per_plane, rem = item % per_plane, br = rem / W4, bc = rem % W4 / QUADS;
    const long long hw = (long long)v.H * v.W, member = (long long)v.planes * hw;
    const float* row = (TRUTH ? (v.d == 0 ? v.y : v.x + (v.d - 1) * member) : v.x + v.d * member);
    const float P = row[plane * hw + (long long)br * S * v.W + bc * S];  // the bits the walk subtracted
    double s[NS];
    int n = 0, n_t = 0;
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
    for (int q = 0; q < QUADS; ++q) {
        n += v.lds_count[tid + q], n_t += v.lds_count[THREADS + tid + q];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < NS; ++k) s[k] = s[k] + v.lds_sums[(k * 4 + c) * THREADS + tid + q];
    }
    const double nan = __builtin_bit_cast(double, CANONICAL_NAN);
    const bool ok = n == S * S, ok_t = n_t == S * S;
    const long long cells = (long long)h * w, block = (long long)br * w + bc;
    const long long out = ((long long)v.d * v.planes + plane) * cells + block;
    const long long out_s = ((long long)v.d * v.planes + plane) * NS * cells + block;
    BM_VISIT_STORE(v.d, plane, block);
    v.n[out] = n;
    v.pivot[out] = P;
    v.sums[out_s] = ok ? s[0] : nan;
    v.sums[out_s + cells] = ok ? s[1] : nan;
    if (TRUTH) v.sums[out_s + 2 * cells] = ok && ok_t ? s[2] : nan;
}

// S picks the instance (host code on either side)
template <int I>
struct Size {
    static constexpr int i = I;
};
template <typename Fn>
static inline void by_size(int s, Fn&& fn) {
    switch (s) {
        case 4: fn(Size<4>{}); break;
        case 8: fn(Size<8>{}); break;
        case 16: fn(Size<16>{}); break;
        default: fn(Size<32>{}); break;
    }
}

}  // namespace blockmoments
#endif
