// Energy and variogram scores of an ensemble: the index maps and the arithmetic of escore.hip, written as barrier-separated phases over
// "thread tid of a workgroup", as crps_core.h is.  Compiled for the host (core_side.h) the same phases run one thread after the other
// over a record per thread: tests/host_escore_main.cpp checks every map below without a GPU.
//
// Definitions (c2w_hip.h: c2w_escore_pairs, c2w_vario_terms).  One (t, f) plane has the rows r_0 = y (the truth) and r_1 .. r_M = x_m,
// each of hw = H W cells, fp32 read as exact numbers.
//   D2[t][f][p] = sum_c (r_i[c] - r_j[c])^2 for every pair i < j, p = i (2 (M + 1) - i - 1) / 2 + (j - i - 1), P = M (M + 1) / 2
//   V[t][f][o][0..2] = sum over the cell pairs (c, c + o) inside the field of ((g_y - g_x)^2, g_y, g_x),
//     g_y = |y_c - y_{c+o}|^p, g_x = (1 / M) sum_m |x_{m,c} - x_{m,c+o}|^p, o = (di, dj) the offsets of offset_of() below
// A row value that is NaN or infinite makes every D2 entry of its row, and every V entry one of whose pairs touches its cell, NaN (all
// three sums); nothing else.  The kernels find that on the result: a difference with a non-finite end is infinite or NaN, every term
// is >= 0, so the sum is non-finite exactly then, and a non-finite sum is written as NaN.  (A term that overflows fp32 -- differences
// beyond 1.8e19 -- ends as NaN too.)
//
// escore_pairs: a workgroup of 256 owns CHUNK = 256 cells of one plane.  It copies them, all M + 1 rows, from HBM to LDS once, 16 bytes
// a load (cells past the end of the plane are zeros: they add +0).  The rows go in blocks of 4; a thread owns one 4 x 4 tile of pairs
// (bi <= bj, row-major) and one slice s of the chunk's 64 groups of 4 cells -- groups s, s + S, s + 2 S .. with S = slices(M) threads a
// tile, so the lanes of a wave read adjacent 16-byte groups -- and keeps its 16 sums in double registers: d = a - b in fp32, d * d in
// fp32, not fused, added to the double, cells in ascending order.  The S threads of a tile then fold through LDS in thread order and
// the pairs i < j <= M of the tile are written: to D2 if the plane is one chunk, else to partial[plane][chunk][P], which the shared
// fold kernel (ordered_sum_launch.h) adds in chunk order.  A row block that ends past row M reads row M again and its pairs are dropped.
//
// vario_terms: a workgroup of 256 owns a tile of 8 x 32 cells of one plane and copies the tile with its halo -- R columns on either
// side, R rows below: the offsets lie in the half plane -- of all M + 1 rows to LDS.  Thread (tid / 32, tid % 32) owns one cell; the 32
// lanes of half a wave read 32 adjacent floats whatever the pitch.  It walks the offsets four at a time (O is a multiple of 4 at every
// R), the member loop innermost: g_y and every member term are fp32 (p = 0.5: the correctly rounded square root, p = 1: the absolute
// value, p = 2: a product), g_x is the fp32 chain of the M terms in member order times the fp32 1 / M, and
// ((double)g_y - (double)g_x)^2, g_y and g_x join the fold as doubles.  The 12 sums of the four offsets fold by the fixed-order sum of
// ordered_sum.h (N = 12, nan_if_not_finite) and go to V if the plane is one tile, else to partial[plane][tile][O][3], which the shared
// fold kernel adds in tile order.  No atomics anywhere: the bits of a plane are fixed by its shape.
#ifndef C2W_ESCORE_CORE_H
#define C2W_ESCORE_CORE_H

#include "core_side.h"

#if defined(__clang__)
#define ESC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ESC_NO_CONTRACT
#endif

#ifndef ESC_VISIT  // the host driver counts the cell pairs here
#define ESC_VISIT(plane, cell, offset)
#endif
#include "ordered_sum.h"

namespace escore {

constexpr int THREADS = 256;
static_assert(THREADS == ordered_sum::THREADS, "the workgroup the fixed-order sum is written for");
using ordered_sum::nan_if_not_finite;  // the write policy of every sum here: the kernels find a non-finite input on the result

typedef float F4 __attribute__((vector_size(16)));  // 16 bytes a load; a struct of four floats would be merged through memory

// ================================================================================================================ pairs

constexpr int P_MAX_M = 64;
constexpr int P_CHUNK = 256;           // cells a workgroup owns
constexpr int P_QUADS = P_CHUNK / 4;   // groups of 4 cells
constexpr int P_PITCH = P_CHUNK + 4;   // floats between two rows in LDS: row blocks start 16 banks apart
constexpr int P_FOLD_BYTES = 16 * THREADS * 8;

static C2W_BOTH inline bool p_supported(int hw, int M) { return hw >= 4 && hw % 4 == 0 && M >= 1 && M <= P_MAX_M; }
static C2W_BOTH inline int p_pairs(int M) { return M * (M + 1) / 2; }
static C2W_BOTH inline int p_pair_index(int M, int i, int j) { return i * (2 * (M + 1) - i - 1) / 2 + (j - i - 1); }
static C2W_BOTH inline int p_blocks(int M) { return (M + 1 + 3) / 4; }
static C2W_BOTH inline int p_tiles(int M) { return p_blocks(M) * (p_blocks(M) + 1) / 2; }
// threads a tile: the largest power of two with tiles * S <= 256, at most 64 (one group of cells a round at least)
static C2W_BOTH inline int p_slices(int M) {
    int s = 64;
    while (s * p_tiles(M) > THREADS) s /= 2;
    return s;
}
static C2W_BOTH inline int p_chunks(int hw) { return (hw + P_CHUNK - 1) / P_CHUNK; }
static C2W_BOTH inline int p_lds_bytes(int M) {
    const int stage = (M + 1) * P_PITCH * 4;
    return stage > P_FOLD_BYTES ? stage : P_FOLD_BYTES;
}
static C2W_BOTH inline long long p_scratch_bytes(long long planes, int hw, int M) {
    return p_chunks(hw) > 1 ? planes * p_chunks(hw) * p_pairs(M) * (long long)sizeof(double) : 0;
}
// tile k -> its row blocks (bi <= bj), row-major
static C2W_BOTH inline void p_tile_blocks(int M, int k, int& bi, int& bj) {
    const int nb = p_blocks(M);
    bi = 0;
    while (k >= nb - bi) k -= nb - bi, ++bi;
    bj = bi + k;
}

struct PView {
    const float* x;   // [M][planes][hw]
    const float* y;   // [planes][hw]
    double* out;      // D2 [planes][P] (one chunk a plane) or partial [planes][chunks][P]
    long long plane, planes;
    int chunk, M, hw;
    unsigned char* lds;  // p_lds_bytes(M): the rows [M + 1][P_PITCH] fp32, then (after a barrier) the sums [16][THREADS] double
};

struct PThread {
    double acc[16];
};

static C2W_HD inline const float* p_row(const PView& v, int r) {
    return r == 0 ? v.y + v.plane * v.hw : v.x + ((long long)(r - 1) * v.planes + v.plane) * v.hw;
}

// the chunk's cells of every row, HBM -> LDS, each value once
static C2W_HD inline void p_stage(const PView& v, int tid) {
    float* rows = (float*)v.lds;
    const int n = (v.M + 1) * P_QUADS;
    for (int e = tid; e < n; e += THREADS) {
        const int r = e / P_QUADS, q = e % P_QUADS, cell = v.chunk * P_CHUNK + q * 4;
        F4 g = {0.f, 0.f, 0.f, 0.f};
        if (cell < v.hw) g = *(const F4*)(p_row(v, r) + cell);
        *(F4*)(rows + r * P_PITCH + q * 4) = g;
    }
}

static C2W_HD inline void p_pairs_of_tile(const PView& v, PThread& th, int tid) {
    ESC_NO_CONTRACT
    const int S = p_slices(v.M), tile = tid / S, s = tid % S;
#pragma unroll
    for (int a = 0; a < 16; ++a) th.acc[a] = 0.0;
    if (tile >= p_tiles(v.M)) return;
    int bi, bj;
    p_tile_blocks(v.M, tile, bi, bj);
    const float* rows = (const float*)v.lds;
    // a row past M reads row M again (its pairs are dropped at the store); scalars, not an array: a row index is never data
    const int M = v.M, i0 = 4 * bi, j0 = 4 * bj;
    const int a0 = (i0 < M ? i0 : M) * P_PITCH, a1 = (i0 + 1 < M ? i0 + 1 : M) * P_PITCH, a2 = (i0 + 2 < M ? i0 + 2 : M) * P_PITCH,
              a3 = (i0 + 3 < M ? i0 + 3 : M) * P_PITCH;
    const int b0 = (j0 < M ? j0 : M) * P_PITCH, b1 = (j0 + 1 < M ? j0 + 1 : M) * P_PITCH, b2 = (j0 + 2 < M ? j0 + 2 : M) * P_PITCH,
              b3 = (j0 + 3 < M ? j0 + 3 : M) * P_PITCH;
    for (int q = s; q < P_QUADS; q += S) {
        const float* at = rows + q * 4;
        const F4 A[4] = {*(const F4*)(at + a0), *(const F4*)(at + a1), *(const F4*)(at + a2), *(const F4*)(at + a3)};
        const F4 B[4] = {*(const F4*)(at + b0), *(const F4*)(at + b1), *(const F4*)(at + b2), *(const F4*)(at + b3)};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float d = A[a][c] - B[b][c];
                    const float sq = d * d;
                    th.acc[a * 4 + b] += (double)sq;
                }
    }
}

// after a barrier: the rows are dead, the sums take their place
static C2W_HD inline void p_stash(const PView& v, const PThread& th, int tid) {
    double* fold = (double*)v.lds;
#pragma unroll
    for (int a = 0; a < 16; ++a) fold[a * THREADS + tid] = th.acc[a];
}

// sum a of tile k is entry k * 16 + a; the threads share the entries round robin: each adds the S threads of the tile in thread order
// and writes the pair if it is one; p_fold then writes D2[entry], entry = plane P + p, from the chunks in index order
static C2W_HD inline void p_fold_store(const PView& v, int tid) {
    const int S = p_slices(v.M), n = p_tiles(v.M) * 16;
    for (int e = tid; e < n; e += THREADS) {
        const int tile = e / 16, a = e % 16;
        int bi, bj;
        p_tile_blocks(v.M, tile, bi, bj);
        const int i = 4 * bi + a / 4, j = 4 * bj + a % 4;
        if (!(i < j && j <= v.M)) continue;
        const double* p = (const double*)v.lds + a * THREADS + tile * S;
        double t = 0.0;
        for (int s = 0; s < S; ++s) t += p[s];
        v.out[(v.plane * p_chunks(v.hw) + v.chunk) * p_pairs(v.M) + p_pair_index(v.M, i, j)] = nan_if_not_finite(t);
    }
}
static C2W_HD inline void p_fold(const double* partial, double* d2, long long entry, int nc, int P) {
    d2[entry] = nan_if_not_finite(ordered_sum::fold_parts(partial, entry, nc, P));
}

// ================================================================================================================ variogram

constexpr int V_MAX_M = 16;
constexpr int V_MAX_R = 8;
constexpr int V_TH = 8, V_TW = 32;  // the tile: one cell a thread, tid = ti * 32 + tj
constexpr int V_BATCH = 4;          // offsets between two folds
constexpr int V_SUMS = 3 * V_BATCH;  // sums a thread hands to one fold
constexpr int V_FOLD_DOUBLES = ordered_sum::lds_doubles<V_SUMS>();

// order2 = 2 p: 1, 2 or 4
static C2W_BOTH inline bool v_supported(int H, int W, int R, int M, int order2) {
    return H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && R >= 1 && R <= V_MAX_R && M >= 1 && M <= V_MAX_M &&
           (order2 == 1 || order2 == 2 || order2 == 4);
}
static C2W_BOTH inline int v_offsets(int R) { return ((2 * R + 1) * (2 * R + 1) - 1) / 2; }
// offset o -> (di, dj): di == 0 and dj = 1 .. R first, then di = 1 .. R with dj = -R .. R
static C2W_BOTH inline void v_offset_of(int R, int o, int& di, int& dj) {
    if (o < R) {
        di = 0, dj = o + 1;
    } else {
        di = 1 + (o - R) / (2 * R + 1), dj = (o - R) % (2 * R + 1) - R;
    }
}
static C2W_BOTH inline int v_tiles_w(int W) { return (W + V_TW - 1) / V_TW; }
static C2W_BOTH inline int v_tiles(int H, int W) { return (H / V_TH) * v_tiles_w(W); }
static C2W_BOTH inline int v_patch_h(int R) { return V_TH + R; }
static C2W_BOTH inline int v_patch_w(int R) { return V_TW + 2 * R; }
static C2W_BOTH inline int v_patch_floats(int R, int M) { return (M + 1) * v_patch_h(R) * v_patch_w(R); }
static C2W_BOTH inline int v_lds_bytes(int R, int M) { return (v_patch_floats(R, M) * 4 + 7) / 8 * 8 + V_FOLD_DOUBLES * 8; }
static C2W_BOTH inline long long v_scratch_bytes(long long planes, int H, int W, int R) {
    return v_tiles(H, W) > 1 ? planes * v_tiles(H, W) * v_offsets(R) * 3 * (long long)sizeof(double) : 0;
}

struct VView {
    const float* x;  // [M][planes][H][W]
    const float* y;  // [planes][H][W]
    double* out;     // V [planes][O][3] (one tile a plane) or partial [planes][tiles][O][3]
    long long plane, planes;
    int tile, M, H, W, R;
    unsigned char* lds;  // v_lds_bytes(R, M): the patch [M + 1][8 + R][32 + 2 R] fp32, then the fold's doubles
};

static C2W_HD inline double* v_fold_area(const VView& v) { return (double*)(v.lds + (v_patch_floats(v.R, v.M) * 4 + 7) / 8 * 8); }

// the tile and its halo of every row, HBM -> LDS; what lies outside the field is 0 and is never used
static C2W_HD inline void v_stage(const VView& v, int tid) {
    float* patch = (float*)v.lds;
    const int ph = v_patch_h(v.R), pw = v_patch_w(v.R), n = (v.M + 1) * ph * pw;
    const int i0 = (v.tile / v_tiles_w(v.W)) * V_TH, j0 = (v.tile % v_tiles_w(v.W)) * V_TW - v.R;
    const long long hw = (long long)v.H * v.W;
    for (int e = tid; e < n; e += THREADS) {
        const int r = e / (ph * pw), pi = e % (ph * pw) / pw, pj = e % pw, i = i0 + pi, j = j0 + pj;
        float g = 0.f;
        if (i < v.H && j >= 0 && j < v.W) g = (r == 0 ? v.y + v.plane * hw : v.x + ((long long)(r - 1) * v.planes + v.plane) * hw)[i * v.W + j];
        patch[e] = g;
    }
}

template <int ORDER2>
static C2W_HD inline float v_power(float d) {
    ESC_NO_CONTRACT
    const float a = __builtin_fabsf(d);
    if constexpr (ORDER2 == 1) return __builtin_sqrtf(a);
    if constexpr (ORDER2 == 2) return a;
    return a * a;
}

// offsets o0 .. o0 + 3 of the thread's cell: its 12 terms go straight to the fold area, in the layout of ordered_sum::stash<V_SUMS>
template <int ORDER2>
static C2W_HD inline void v_terms(const VView& v, int tid, int o0) {
    ESC_NO_CONTRACT
    const float* patch = (const float*)v.lds;
    double* fold = v_fold_area(v);
    const int ph = v_patch_h(v.R), pw = v_patch_w(v.R), ti = tid / V_TW, tj = tid % V_TW;
    const int i = (v.tile / v_tiles_w(v.W)) * V_TH + ti, j = (v.tile % v_tiles_w(v.W)) * V_TW + tj;
    const int own = ti * pw + tj + v.R;
    const float rM = (float)(1.0 / (double)v.M);
    int at[V_BATCH];
    bool in[V_BATCH];
#pragma unroll
    for (int b = 0; b < V_BATCH; ++b) {
        int di, dj;
        v_offset_of(v.R, o0 + b, di, dj);
        in[b] = j < v.W && i + di < v.H && j + dj >= 0 && j + dj < v.W;
        at[b] = in[b] ? own + di * pw + dj : own;
    }
    float gy[V_BATCH], gx[V_BATCH];
    const float yc = patch[own];
#pragma unroll
    for (int b = 0; b < V_BATCH; ++b) gy[b] = v_power<ORDER2>(yc - patch[at[b]]), gx[b] = 0.f;
    const float* row = patch;
    for (int m = 0; m < v.M; ++m) {
        row += ph * pw;
        const float xc = row[own];
#pragma unroll
        for (int b = 0; b < V_BATCH; ++b) gx[b] += v_power<ORDER2>(xc - row[at[b]]);
    }
#pragma unroll
    for (int b = 0; b < V_BATCH; ++b) {
        double e = 0.0, y = 0.0, x = 0.0;
        if (in[b]) {
            ESC_VISIT(v.plane, i * v.W + j, o0 + b);
            const float mean = gx[b] * rM;
            const double d = (double)gy[b] - (double)mean;
            y = (double)gy[b], x = (double)mean;
            e = d * d;
            if (!(__builtin_fabsf(gy[b] + mean) < __builtin_inff())) e = y = x = (double)__builtin_nanf("");
        }
        fold[(b * 3 + 0) * THREADS + tid] = e, fold[(b * 3 + 1) * THREADS + tid] = y, fold[(b * 3 + 2) * THREADS + tid] = x;
    }
}

// the fold of ordered_sum.h over the fold area at N = V_SUMS: thread q writes sum q, the entry of offset o0 + q / 3; v_fold then
// writes V[entry], entry = (plane O + o) 3 + s, from the tiles in index order
static C2W_HD inline void v_fold_groups(const VView& v, int tid) { ordered_sum::fold_groups<V_SUMS>(v_fold_area(v), tid); }
static C2W_HD inline void v_fold_store(const VView& v, int tid, int o0) {
    if (tid >= V_SUMS) return;
    const double t = ordered_sum::fold_total<V_SUMS>(v_fold_area(v), tid);
    const long long O = v_offsets(v.R);
    v.out[((v.plane * v_tiles(v.H, v.W) + v.tile) * O + o0) * 3 + tid] = nan_if_not_finite(t);
}
static C2W_HD inline void v_fold(const double* partial, double* V, long long entry, int nt, int O3) {
    V[entry] = nan_if_not_finite(ordered_sum::fold_parts(partial, entry, nt, O3));
}

}  // namespace escore
#endif
