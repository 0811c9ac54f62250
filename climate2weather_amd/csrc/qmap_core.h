// Quantile mapping per cell: the index maps and the arithmetic of qmap.hip, written as barrier-separated phases over "thread tid of a
// workgroup", as wind_core.h and temporal_core.h are.  Compiled for the host (core_side.h) the same phases run one thread after the
// other: tests/host_qmap_main.cpp checks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_qmap_nodes, c2w_qmap_apply).  A series is the values of one variable at one cell over the times of one
// group.  The times of group g are tidx[goff[g] .. goff[g + 1]), n of them.
//   nodes   q[rep][g][f][c][k] = the quantile at level p_k of the series, by the definition of quantile_core.h: nv = #non-NaN,
//           rank_of / lerp_of of that file on the two order statistics (exact fp32), float64.  nv == 0 (an empty group included), or a
//           NaN where NaNs are not skipped, makes the K nodes NaN.  n_valid[rep][g][f][c] = nv.
//   apply   with xq / yq the K nodes of the model's / the reference's historical series of the cell and group, x fp32, in float64:
//           j = the last node with xq[j] <= x;  none: y = x + (yq[0] - xq[0]);  j = K - 1: y = x + (yq[K - 1] - xq[K - 1]);  else
//           v = yq[j] + (x - xq[j]) * ((yq[j + 1] - yq[j]) / (xq[j + 1] - xq[j])),  y = v > yq[j + 1] ? yq[j + 1] : v;
//           no multiply fused with an add; y rounded once to fp32.  A NaN x finds no node and x + .. is NaN; a NaN row finds no node
//           and .. + NaN is NaN.
//
// Node fit, two kernels over a block of cells [c0, c1):
//   qmap_gather  a tile of 64 list positions x 64 cells goes through LDS ([64][65] floats: both sides conflict-free) from the
//                time-major planes into scratch[row][cell - c0][position], row = rep F + f: a wave reads 64 adjacent cells of one plane
//                and writes 64 adjacent positions of one series, 256 contiguous bytes either way.  A series' groups lie one after the
//                other in its scratch row, because the list is sorted by group.
//   qmap_sort    a workgroup per (row, cell, group): the series' keys (quantile_core.h: key_of; a NaN, by its bits, and the padding
//                become TOP = 0xFFFFFFFF, the key no number has) are sorted in LDS by a bitonic network over N = the next power of
//                two; nv is the first position that holds TOP, found by bisection; thread k < K interpolates level k.
// Apply, one kernel: a workgroup of 512 per (group, variable, block of C adjacent cells, slab of the group's rows), C from K so that
// the {xq, yq} tables of its cells fit APPLY_LDS bytes, each table row padded to an odd number of doubles.  A row is a (rep, list
// position) pair; C / 4 lanes take one row with a 16-byte load each, LOADS rows in flight; the four values of a load are bisected in
// LDS side by side (count_le4: the comparisons of count_le, the four reads of a step in flight together) and mapped; the store goes to
// the position the load came from, so out may be x.
// Every number is a function of its own series alone: the same bits wherever the series lies in the launch.
#ifndef C2W_QMAP_CORE_H
#define C2W_QMAP_CORE_H

#include "core_side.h"

#if defined(__clang__)
#define QMAP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define QMAP_NO_CONTRACT
#endif

#ifndef QMAP_VISIT  // the host driver counts the elements the apply walk takes up here
#define QMAP_VISIT(index)
#endif

#include "quantile_core.h"

namespace qmap {

constexpr int THREADS = 256;             // gather workgroup
constexpr int APPLY_THREADS = 512;       // apply workgroup: eight waves share one staging of the tables
constexpr int MAX_K = 128;               // levels
constexpr int MAX_N = 16384;             // values of a series the LDS sort takes: 64 KiB of keys
constexpr int TILE = 64;                 // gather: list positions and cells of a tile
constexpr int TILE_LD = TILE + 1;        // its row stride in LDS, odd: rows and columns both hit 64 banks
constexpr int APPLY_LDS = 72 * 1024;     // bytes of tables an apply workgroup stages: two workgroups a compute unit
constexpr int MAX_CELLS = 64;            // cells of an apply workgroup at most
constexpr int LOADS = 4;                 // 16-byte loads an apply thread has in flight
constexpr int WG_PER_CU = 4;             // apply workgroups per compute unit the slab count aims at
constexpr unsigned TOP = 0xFFFFFFFFu;    // the key of a NaN and of the padding: key_of of no number (it is the key of the bits 0x7FFFFFFF)
static_assert(THREADS % TILE == 0 && APPLY_THREADS % (MAX_CELLS / 4) == 0, "whole rows per pass");

typedef float F4 __attribute__((vector_size(16)));  // 16 bytes a load

static C2W_BOTH inline bool supported(int hw, int K, int max_len) {
    return hw >= 4 && hw % 4 == 0 && K >= 2 && K <= MAX_K && max_len >= 0 && max_len <= MAX_N;
}

// ---------------------------------------------------------------------------------------------------------------- maps

static C2W_BOTH inline int padded(int n) {
    int N = 2;
    while (N < n) N <<= 1;
    return N;
}
static C2W_BOTH inline int sort_threads(int N) { return N <= 2048 ? 256 : 1024; }
static C2W_BOTH inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
static C2W_BOTH inline int tiles(int n) { return (n + TILE - 1) / TILE; }
// bytes of the series-major scratch of a block of `cells` cells: [rows][cells][Tu] fp32
static C2W_BOTH inline long long scratch_bytes(long long rows, int cells, int Tu) { return (rows * cells * Tu * 4 + 15) / 16 * 16; }
// doubles of one table row in LDS, odd
static C2W_BOTH inline int table_ld(int K) { return K | 1; }
// cells of an apply workgroup: the most of 64, 32 .. 4 whose two tables fit APPLY_LDS
static C2W_BOTH inline int cells_per_block(int K) {
    int C = MAX_CELLS;
    while (C > 4 && 2 * C * table_ld(K) * 8 > APPLY_LDS) C >>= 1;
    return C;
}
static C2W_BOTH inline int apply_lds_bytes(int K) { return 2 * cells_per_block(K) * table_ld(K) * 8; }
static C2W_BOTH inline int cell_blocks(int hw, int K) { return (hw + cells_per_block(K) - 1) / cells_per_block(K); }
// rows one pass of an apply workgroup covers
static C2W_BOTH inline int rows_per_pass(int K) { return APPLY_THREADS / (cells_per_block(K) / 4); }
// slabs per (group, variable, cell block): WG_PER_CU workgroups a compute unit, a slab no shorter than one round of LOADS passes
static C2W_BOTH inline int slab_count(long long blocks, long long max_rows, int K, int cus) {
    long long s = (long long)cus * WG_PER_CU / (blocks < 1 ? 1 : blocks);
    const long long most = (max_rows + LOADS * rows_per_pass(K) - 1) / (LOADS * rows_per_pass(K));
    s = s > most ? most : s;
    return (int)(s < 1 ? 1 : s);
}
static C2W_BOTH inline long long slab_begin(long long rows, int slabs, int s) { return rows * s / slabs; }

// ---------------------------------------------------------------------------------------------------------------- gather: phases

struct GView {
    const float* x;   // [n_rep][T][F][hw]
    const int* tidx;  // [Tu] times, sorted by group
    float* scratch;   // [rows][c1 - c0][Tu]
    long long row;    // rep F + f
    int ctile, ptile;
    int T, F, hw, Tu, c0, c1;
    float* tile;  // LDS: TILE * TILE_LD
};

static C2W_HD inline void g_load(const GView& v, int tid) {
    const int col = tid % TILE, c = v.c0 + v.ctile * TILE + col;
    const long long rep = v.row / v.F, f = v.row % v.F;
    for (int i = tid / TILE; i < TILE; i += THREADS / TILE) {
        const int p = v.ptile * TILE + i;
        if (p >= v.Tu || c >= v.c1) continue;
        const int t = clampi(v.tidx[p], 0, v.T - 1);
        v.tile[i * TILE_LD + col] = v.x[((rep * v.T + t) * v.F + f) * v.hw + c];
    }
}

static C2W_HD inline void g_store(const GView& v, int tid) {
    const int col = tid % TILE, p = v.ptile * TILE + col;
    for (int j = tid / TILE; j < TILE; j += THREADS / TILE) {
        const int cl = v.ctile * TILE + j;
        if (p >= v.Tu || v.c0 + cl >= v.c1) continue;
        v.scratch[(v.row * (v.c1 - v.c0) + cl) * v.Tu + p] = v.tile[col * TILE_LD + j];
    }
}

// ---------------------------------------------------------------------------------------------------------------- sort: phases

struct SView {
    const float* scratch;   // [rows][c1 - c0][Tu]
    const int* goff;        // [G + 1]
    const double* levels;   // [K]
    double* q;              // [n_rep][G][F][hw][K]
    long long* nvalid;      // [n_rep][G][F][hw]
    long long series;       // (row (c1 - c0) + cell - c0) G + g
    int F, hw, Tu, c0, c1, G, K, skipna, max_len;
    int nthr;
    unsigned* keys;  // LDS: padded(n)
};

static C2W_HD inline int group_of(const SView& v) { return (int)(v.series % v.G); }
static C2W_HD inline int first_of(const SView& v) { return clampi(v.goff[group_of(v)], 0, v.Tu); }
// the series' length, never beyond the list or what the launch has LDS for
static C2W_HD inline int length_of(const SView& v) {
    const int n = clampi(v.goff[group_of(v) + 1], 0, v.Tu) - first_of(v);
    return clampi(n, 0, v.max_len);
}

static C2W_HD inline void s_load(const SView& v, int tid) {
    const int n = length_of(v), N = padded(n);
    const float* s = v.scratch + (v.series / v.G) * v.Tu + first_of(v);
    for (int i = tid; i < N; i += v.nthr) {
        unsigned key = TOP;
        if (i < n) {
            const unsigned bits = __builtin_bit_cast(unsigned, s[i]);
            if (!qnt::is_nan_bits(bits)) key = qnt::key_of(bits);
        }
        v.keys[i] = key;
    }
}

// one stage of the bitonic network: pairs (l, l | j), ascending where l & k == 0
static C2W_HD inline void s_stage(const SView& v, int tid, int k, int j) {
    const int N = padded(length_of(v));
    for (int i = tid; i < N / 2; i += v.nthr) {
        const int l = 2 * i - (i & (j - 1)), r = l | j;
        const unsigned a = v.keys[l], b = v.keys[r];
        if ((a > b) == ((l & k) == 0)) v.keys[l] = b, v.keys[r] = a;
    }
}

// thread k < K: level k of the sorted series; thread 0 also the count
static C2W_HD inline void s_nodes(const SView& v, int tid) {
    if (tid >= v.K) return;
    const int n = length_of(v);
    int lo = 0, hi = n;  // the first position that holds TOP: the non-NaN values are below it
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v.keys[mid] != TOP) lo = mid + 1; else hi = mid;
    }
    const long long nv = lo;
    const long long at = v.series / v.G, row = at / (v.c1 - v.c0), c = v.c0 + at % (v.c1 - v.c0);
    const long long rep = row / v.F, f = row % v.F;
    const long long cell = ((rep * v.G + group_of(v)) * v.F + f) * v.hw + c;
    if (tid == 0) v.nvalid[cell] = nv;
    double res = (double)__builtin_nanf("");
    if (nv > 0 && (v.skipna || nv == n)) {
        const double p = v.levels[tid];
        const float a = qnt::float_of(qnt::bits_of(v.keys[qnt::rank_of(nv, p, 0)])), b = qnt::float_of(qnt::bits_of(v.keys[qnt::rank_of(nv, p, 1)]));
        res = qnt::lerp_of(nv, p, a, b);
    }
    v.q[cell * v.K + tid] = res;
}

// ---------------------------------------------------------------------------------------------------------------- apply: phases

struct AView {
    const float* x;    // [n_rep][T][F][hw]
    float* out;        // the same shape; may be x
    const double* xq;  // [G][F][hw][K]
    const double* yq;
    const int* tidx;
    const int* goff;
    long long n_rep;
    int g, f, cblock, slab, slabs;
    int T, F, hw, Tu, K;
    double* lds;  // 2 * cells_per_block(K) * table_ld(K)
};

static C2W_HD inline void a_stage(const AView& v, int tid) {
    const int C = cells_per_block(v.K), ld = table_ld(v.K);
    const long long base = (((long long)v.g * v.F + v.f) * v.hw + (long long)v.cblock * C) * v.K;
    for (int i = tid; i < C * v.K; i += APPLY_THREADS) {
        const int cl = i / v.K, k = i - cl * v.K;
        if (v.cblock * C + cl >= v.hw) break;  // i ascends with the cell
        v.lds[cl * ld + k] = v.xq[base + i];
        v.lds[(C + cl) * ld + k] = v.yq[base + i];
    }
}

// the nodes with xq <= x are [0, lo): a NaN x, or a NaN row, has none
static C2W_BOTH inline int count_le(const double* xq, int K, double x) {
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xq[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// steps after which the search over K nodes has ended: ceil(log2(K + 1))
static C2W_BOTH inline int search_steps(int K) {
    int s = 0;
    while ((1 << s) <= K) ++s;
    return s;
}
// count_le for the four cells of a quad, step by step side by side: the same comparisons, the four LDS reads of a step in flight together
static C2W_BOTH inline void count_le4(const double* xq, int ld, int K, const double* x, int* lo) {
    int hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) lo[e] = 0, hi[e] = K;
    for (int s = search_steps(K); s > 0; --s) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int mid = (lo[e] + hi[e]) >> 1;  // < K while lo < hi; a search that has ended reads node K - 1 at most and keeps its bounds
            const bool open = lo[e] < hi[e], le = xq[e * ld + (mid < K ? mid : K - 1)] <= x[e];
            lo[e] = open && le ? mid + 1 : lo[e];
            hi[e] = open && !le ? mid : hi[e];
        }
    }
}

// the definition, given lo = the number of nodes with xq <= x
static C2W_BOTH inline float map_at(const double* xq, const double* yq, int K, double x, int lo) {
    QMAP_NO_CONTRACT
    double y;
    if (lo == 0) {
        const double shift = yq[0] - xq[0];
        y = x + shift;
    } else if (lo == K) {
        const double shift = yq[K - 1] - xq[K - 1];
        y = x + shift;
    } else {
        const int j = lo - 1;
        const double slope = (yq[j + 1] - yq[j]) / (xq[j + 1] - xq[j]);
        const double step = (x - xq[j]) * slope;
        const double v = yq[j] + step;
        y = v > yq[j + 1] ? yq[j + 1] : v;
    }
    return (float)y;
}
static C2W_BOTH inline float map_one(const double* xq, const double* yq, int K, float xf) {
    return map_at(xq, yq, K, (double)xf, count_le(xq, K, (double)xf));
}

static C2W_HD inline void a_walk(const AView& v, int tid) {
    const int C = cells_per_block(v.K), ld = table_ld(v.K), lanes = C / 4, rpp = APPLY_THREADS / lanes;
    const int cl = 4 * (tid % lanes), c = v.cblock * C + cl;
    if (c >= v.hw) return;  // hw % 4 == 0: a quad is whole or absent
    const int first = clampi(v.goff[v.g], 0, v.Tu), n = clampi(v.goff[v.g + 1], 0, v.Tu) - first;
    if (n <= 0) return;
    const long long rows = v.n_rep * n, r0 = slab_begin(rows, v.slabs, v.slab), r1 = slab_begin(rows, v.slabs, v.slab + 1);
    for (long long rr = r0 + tid / lanes; rr < r1; rr += (long long)LOADS * rpp) {
        F4 b[LOADS];
        long long at[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const long long r = rr + (long long)u * rpp;
            if (r >= r1) continue;
            const long long rep = r / n;
            const int t = clampi(v.tidx[first + (int)(r - rep * n)], 0, v.T - 1);
            at[u] = ((rep * v.T + t) * v.F + v.f) * v.hw + c;
            b[u] = *(const F4*)(v.x + at[u]);
        }
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            if (rr + (long long)u * rpp >= r1) continue;
            QMAP_VISIT(at[u]);
            F4 y;
            double xd[4];
            int lo[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) xd[e] = (double)b[u][e];
            count_le4(v.lds + cl * ld, ld, v.K, xd, lo);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = map_at(v.lds + (cl + e) * ld, v.lds + (C + cl + e) * ld, v.K, xd[e], lo[e]);
            *(F4*)(v.out + at[u]) = y;
        }
    }
}

}  // namespace qmap
#endif
