// Co-moments of an ensemble: the index maps and the arithmetic of comoments.hip, written as phases over "thread tid of a workgroup", as
// extremes_maps.h and spells_core.h are.  Compiled for the host (core_side.h) the same phases run one thread after the other:
// tests/host_comoments_main.cpp walks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_comoments_update).  The rows are d = 0 the truth when one is given, then the M members; D rows in all.  A
// SERIES is one (d, f, cell) over time, F the number of variables.
//
// VALID HOUR.  Hour t is valid for (d, cell) iff all F values of row d at that cell are finite and, with a truth, all F truth values at
// that cell are finite too.  Finite is decided on the bits: exponent field not all ones; an infinity is invalid, not a value.  An invalid
// hour adds nothing to any entry of (d, cell) and is counted in invalid[d], in cell-hours.
//
// PIVOTS.  At the first valid hour of (d, cell) P[d][f][cell] becomes the row's own fp32 value and, with a truth, PT[d][f][cell] the
// truth's fp32 value of that same hour; neither changes afterwards.  n[d][cell] counts the valid hours, n == 0 is "no pivot yet".
//
// SUMS.  e_f = (double)x_f - (double)P_f and eT_f = (double)y_f - (double)PT_f: double subtractions of exactly converted fp32 values.
// Per valid hour, in hour order, no multiply fused with an add, every accumulator a plain s = s + term:
//   S[f]      += e_f                       F entries
//   C[f, g]   += e_f * e_g   (f <= g)      F (F + 1) / 2 entries, in the order (0,0), (0,1) .. (0,F-1), (1,1) ..
//   ST[f]     += eT_f                      F entries   }
//   QT[f]     += eT_f * eT_f               F entries   }  with a truth only
//   X[f]      += e_f * eT_f                F entries   }
// NS = 4 F + F (F + 1) / 2 entries with a truth, F + F (F + 1) / 2 without.  Row 0 carries the same layout: there eT = e, so X = QT =
// C_ff.  sums[D][NS][hw] double, pivot[D][F][hw] and truth_pivot[D][F][hw] float, n[D][hw] int: the cell index is innermost, adjacent
// threads touch adjacent addresses.  The first valid hour contributes e = 0 exactly; a series that never has one keeps n = 0, zero
// sums and the pivot +0.0 it was made with.
//
// A sum is never -0.0: it starts as +0.0, and round-to-nearest gives -0.0 only from (-0.0) + (-0.0).  So "adds nothing" and "adds
// +0.0" are the same bits, and a route may do either.
//
// BIT FOR BIT.  Every accumulator receives its terms one at a time in hour order and the state carries the doubles themselves, so
// the tables are the same bits on the kernel, on the torch route, in the NumPy reference and for every cut of the hours into calls.
//
// comoments_update<F, TRUTH>: a workgroup of 256 owns one row d and a chunk of 256 V(F) cells; a thread owns V(F) adjacent cells,
// V = 4 for F = 1, 2 for F = 2, 1 above -- the state of a cell is 2 NS + 2 F + 1 registers, and no instance may spill.  The thread
// loads its state (n, the pivots, the NS doubles a cell), walks the call's T planes in order -- per hour the row's F planes and the
// truth's F planes, UNROLL = 4 hours loaded in a straight line; a step past the end reads plane T - 1 again (the address is clamped)
// and forms no term, as extremes::b_walk does --, and stores its state where it loaded it.  The invalid cell-hours go through one LDS
// int to one 64-bit add per workgroup.  Time is not split over workgroups; no atomics on floats, no scratch buffer.
//
// WHY THE PIVOT.  It removes the field's magnitude before any product: at 101325 +- 0.5 Pa the terms are of size 0.25, not 1e10, and
// the one-pass form sum xy - sum x sum y / n in float64 loses eight digits more (tests/test_dependence_cpu.py shows the miss).
//
// THE BOUND.  u = 2^-53, and (k + 1) u stands for k u / (1 - k u) (k < 10^7), one more unit for the second-order terms, as in
// extremes_maps.h.  Against exact rational arithmetic on the exact fp32 values, with e the EXACT differences and n the valid hours:
// a term of S_f carries the rounding of e_f (none while the exponents of x and P lie within 2^29 of each other) and of at most n - 1
// adds -- the first valid hour's term is an exact zero and the add that follows it is exact --: at most n roundings,
//   |S_f^ - S_f| <= (n + 1) u sum |e_f|  + 2^-1074.
// A term of a product sum carries the roundings of its two factors and of the product as well: at most n + 1 roundings, and every
// product sum (C, QT, X) is within
//   (n + 2) u sum |e_f e_g|  + 2^-1074
// of its exact value; ST is bounded as S.  The denormal is for a term that underflows.  (bound_rounds below.)
//
// MERGE (dependence.py: DependenceAccumulator.merge) adds another accumulator `o` over OTHER hours of the same cells to this one `s`
// by re-basing o's sums onto s's pivots in float64.  With d_f = (double)P_o,f - (double)P_s,f, m = (double)n_o, each line one rounding
// per operation, evaluated left to right:
//   S'_f  = S_o,f + m d_f                                    S_f  <- S_s,f + S'_f
//   C'_fg = ((C_o,fg + d_f S_o,g) + d_g S_o,f) + (m d_f) d_g   C_fg <- C_s,fg + C'_fg
// and the same with (dT, ST), (dT, dT, ST, ST, QT) and (d, dT, ST, S, X).  Exactly, C'_fg = sum_o (e_f + d_f)(e_g + d_g): o's sum about
// s's pivot.  The four parts may cancel, so the roundings are not small against that sum itself but against its majorant
//   A'_fg = sum_o (|e_f| + |d_f|)(|e_g| + |d_g|)   and   A'_f = sum_o (|e_f| + |d_f|).
// Roundings of the re-basing: C_o three adds and the last add, 4; d_f S_o,g: d_f, the product, three adds, the last, 6; d_g S_o,f 5;
// (m d_f) d_g: two differences, two products, one add, the last, 6; at most 7 u A'_fg by the convention, one more for the errors the
// parts inherit from o's own sums being multiplied by 1 + 4 u.  With o's own bound (n_o + 2) u A'_fg (C_o's, and |d| times S_o's):
//   |C_fg^ - C_fg| <= (n_s + 4) u A_s,fg + (n_o + 11) u A'_fg + 2 * 2^-1074        (s's bound, the last add on it and its value)
//   |S_f^  - S_f | <= (n_s + 3) u A_s,f  + (n_o +  6) u A'_f  + 2 * 2^-1074        (S_o: 2; m d_f: 4)
// (merge_rounds_self / merge_rounds_other below.)  A series with n_s = 0 takes o's state as it is, bit for bit.
#ifndef C2W_COMOMENTS_MAPS_H
#define C2W_COMOMENTS_MAPS_H

#include "core_side.h"

#ifndef CM_VISIT_READ  // the host driver counts here: V cell-hours of row d read (its F planes and the truth's); V entries of a state
#define CM_VISIT_READ(d, t, cell, cells)  // array (0 n, 1 pivot, 2 truth_pivot, 3 sums) loaded / stored at element `at`
#define CM_VISIT_LOAD(what, at, cells)
#define CM_VISIT_STORE(what, at, cells)
#endif
#include "events_core.h"  // the LDS and global adds

#if defined(__clang__)
#define CM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CM_NO_CONTRACT
#endif

namespace comoments {

using events::global_add;
using events::lds_add;

constexpr int THREADS = 256;
constexpr int UNROLL = 4;  // hours loaded in a straight line
constexpr int MAX_F = 8, MAX_T = 1 << 20;

static C2W_BOTH constexpr int cells_per_thread(int F) { return F <= 1 ? 4 : F <= 2 ? 2 : 1; }
static C2W_BOTH constexpr int chunk_cells(int F) { return THREADS * cells_per_thread(F); }
static C2W_BOTH constexpr int pairs(int F) { return F * (F + 1) / 2; }
static C2W_BOTH constexpr int entries(int F, bool truth) { return F + pairs(F) + (truth ? 3 * F : 0); }
// where the blocks of a series' NS entries begin
static C2W_BOTH constexpr int at_S(int) { return 0; }
static C2W_BOTH constexpr int at_C(int F) { return F; }
static C2W_BOTH constexpr int at_ST(int F) { return F + pairs(F); }
static C2W_BOTH constexpr int at_QT(int F) { return 2 * F + pairs(F); }
static C2W_BOTH constexpr int at_X(int F) { return 3 * F + pairs(F); }
static_assert((long long)chunk_cells(1) * MAX_T < (1LL << 31), "the invalid count of a workgroup fits its LDS int");

static C2W_BOTH inline bool supported(int hw, int F) { return hw >= 4 && hw % 4 == 0 && F >= 1 && F <= MAX_F; }
static C2W_BOTH inline int chunks(int hw, int F) { return (hw + chunk_cells(F) - 1) / chunk_cells(F); }
static C2W_BOTH inline int cell_of(int chunk, int tid, int F) { return (chunk * THREADS + tid) * cells_per_thread(F); }

// the bounds of the header's comment, in units of u = 2^-53 times the sum of absolute terms
static C2W_BOTH inline long long bound_rounds(long long n, bool product) { return n + (product ? 2 : 1); }
static C2W_BOTH inline long long merge_rounds_self(long long n_s, bool product) { return n_s + (product ? 4 : 3); }
static C2W_BOTH inline long long merge_rounds_other(long long n_o, bool product) { return n_o + (product ? 11 : 6); }

static C2W_BOTH inline bool finite_bits(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7F800000u) != 0x7F800000u; }

// V adjacent entries of a state array or of a plane: one load of at most 16 bytes each
template <typename E, int V>
struct alignas(sizeof(E) * V < 16 ? sizeof(E) * V : 16) Pack {
    E v[V];
};

struct View {
    const float* x;      // [M][T][F][hw]
    const float* y;      // [T][F][hw] or null
    int* n;              // [D][hw]
    float* pivot;        // [D][F][hw]
    float* truth_pivot;  // [D][F][hw], with a truth
    double* sums;        // [D][NS][hw]
    long long* invalid;  // [D]
    int d, chunk;        // what this workgroup owns
    int D, T, hw;
    int* lds;            // 1 int
};

static C2W_HD inline void u_zero(const View& v, int tid) {
    if (tid == 0) v.lds[0] = 0;
}

template <int F, bool TRUTH>
static C2W_HD inline void u_walk(const View& v, int tid) {
    CM_NO_CONTRACT
    constexpr int V = cells_per_thread(F), NP = pairs(F), NS = entries(F, TRUTH);
    const int cell = cell_of(v.chunk, tid, F);
    if (cell >= v.hw) return;  // hw is a multiple of 4 and V divides 4: a thread has its V cells or none
    const long long n_at = (long long)v.d * v.hw + cell, p_at = (long long)v.d * F * v.hw + cell, s_at = (long long)v.d * NS * v.hw + cell;
    // ---- the state, loaded once
    CM_VISIT_LOAD(0, n_at, V);
    Pack<int, V> n = *(const Pack<int, V>*)(v.n + n_at);
    Pack<float, V> P[F], PT[TRUTH ? F : 1];
    Pack<double, V> s[NS];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        CM_VISIT_LOAD(1, p_at + (long long)f * v.hw, V);
        P[f] = *(const Pack<float, V>*)(v.pivot + p_at + (long long)f * v.hw);
        if (TRUTH) {
            CM_VISIT_LOAD(2, p_at + (long long)f * v.hw, V);
            PT[f] = *(const Pack<float, V>*)(v.truth_pivot + p_at + (long long)f * v.hw);
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        CM_VISIT_LOAD(3, s_at + (long long)k * v.hw, V);
        s[k] = *(const Pack<double, V>*)(v.sums + s_at + (long long)k * v.hw);
    }
    // ---- the hours, in order
    const long long stride = (long long)F * v.hw, member = (long long)v.T * stride;
    const float* row = (TRUTH ? (v.d == 0 ? v.y : v.x + (v.d - 1) * member) : v.x + v.d * member) + cell;
    const float* truth = TRUTH ? v.y + cell : row;
    const int last = v.T - 1;
    int n_invalid = 0;
    for (int tb = 0; tb < v.T; tb += UNROLL) {
        Pack<float, V> a[UNROLL][F], b[UNROLL][TRUTH ? F : 1];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long long at = (long long)(tb + u < last ? tb + u : last) * stride;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                a[u][f] = *(const Pack<float, V>*)(row + at + (long long)f * v.hw);
                if (TRUTH) b[u][f] = *(const Pack<float, V>*)(truth + at + (long long)f * v.hw);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const bool live = tb + u <= last;  // the same for the whole workgroup: past the end the loads were clamped and form no term
            if (live) CM_VISIT_READ(v.d, tb + u, cell, V);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                bool valid = live;
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    valid = valid && finite_bits(a[u][f].v[c]);
                    if (TRUTH) valid = valid && finite_bits(b[u][f].v[c]);
                }
                // No branch: an hour that is not valid is walked with the pivot in the value's place.  A pivot is finite (a valid
                // hour's value, or the +0.0 the state was made with), so every e is P - P = +0.0, every product +0.0, and a sum
                // -- never -0.0 -- keeps its bits.
                const bool first = valid && n.v[c] == 0;
                n.v[c] += valid ? 1 : 0;
                n_invalid += live && !valid ? 1 : 0;
                double e[F], eT[TRUTH ? F : 1];
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    P[f].v[c] = first ? a[u][f].v[c] : P[f].v[c];
                    e[f] = (double)(valid ? a[u][f].v[c] : P[f].v[c]) - (double)P[f].v[c];
                    if (TRUTH) {
                        PT[f].v[c] = first ? b[u][f].v[c] : PT[f].v[c];
                        eT[f] = (double)(valid ? b[u][f].v[c] : PT[f].v[c]) - (double)PT[f].v[c];
                    }
                }
#pragma unroll
                for (int f = 0; f < F; ++f) s[at_S(F) + f].v[c] = s[at_S(F) + f].v[c] + e[f];
                int k = at_C(F);
#pragma unroll
                for (int f = 0; f < F; ++f)
#pragma unroll
                    for (int g = f; g < F; ++g, ++k) {
                        const double term = e[f] * e[g];
                        s[k].v[c] = s[k].v[c] + term;
                    }
                if (TRUTH) {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        const double q = eT[f] * eT[f], x = e[f] * eT[f];
                        s[at_ST(F) + f].v[c] = s[at_ST(F) + f].v[c] + eT[f];
                        s[at_QT(F) + f].v[c] = s[at_QT(F) + f].v[c] + q;
                        s[at_X(F) + f].v[c] = s[at_X(F) + f].v[c] + x;
                    }
                }
            }
        }
    }
    (void)NP;
    // ---- the state, stored where it was loaded
    CM_VISIT_STORE(0, n_at, V);
    *(Pack<int, V>*)(v.n + n_at) = n;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        CM_VISIT_STORE(1, p_at + (long long)f * v.hw, V);
        *(Pack<float, V>*)(v.pivot + p_at + (long long)f * v.hw) = P[f];
        if (TRUTH) {
            CM_VISIT_STORE(2, p_at + (long long)f * v.hw, V);
            *(Pack<float, V>*)(v.truth_pivot + p_at + (long long)f * v.hw) = PT[f];
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        CM_VISIT_STORE(3, s_at + (long long)k * v.hw, V);
        *(Pack<double, V>*)(v.sums + s_at + (long long)k * v.hw) = s[k];
    }
    if (n_invalid) lds_add(v.lds, n_invalid);
}

static C2W_HD inline void u_flush(const View& v, int tid) {
    if (tid == 0 && v.lds[0]) global_add(v.invalid + v.d, (long long)v.lds[0]);
}

// F picks the instance (host code on either side)
template <int I>
struct Variables {
    static constexpr int i = I;
};
template <typename Fn>
static inline void by_variables(int F, Fn&& fn) {
    switch (F) {
        case 1: fn(Variables<1>{}); break;
        case 2: fn(Variables<2>{}); break;
        case 3: fn(Variables<3>{}); break;
        case 4: fn(Variables<4>{}); break;
        case 5: fn(Variables<5>{}); break;
        case 6: fn(Variables<6>{}); break;
        case 7: fn(Variables<7>{}); break;
        default: fn(Variables<8>{}); break;
    }
}

}  // namespace comoments
#endif
