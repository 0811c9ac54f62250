// Event verification of an ensemble: the index maps and the integer arithmetic of events.hip, written as barrier-separated phases over
// "thread tid of a workgroup", as crps_core.h and temporal_core.h are.  Compiled for the host (core_side.h) the same phases run one
// thread after the other: tests/host_events_main.cpp walks every map below without a GPU.
//
// The event (c2w_hip.h: c2w_event_counts).  thr[F][K] fp32 and dir[F][K] (1: above, x >= thr; 0: below, x <= thr), IEEE comparisons on
// exact fp32 values: infinities compare as numbers, a NaN is no event.  Everything below is integers, so no order of any sum matters.
//
// event_counts: counts[t][f][k][o][j] = the cells of plane (t, f) whose truth indicator is o and in which exactly j of the M members
// have the event; invalid[t][f] = the cells with a NaN among their M + 1 values, which are in no bin.  A workgroup of 256 owns one plane
// or one chunk of CHUNK cells of it.  In a round a thread loads 4 adjacent cells of the truth, keeps them, and streams the M members
// over them; per threshold its four member counts ride in the four bytes of one register (M <= 64 < 256).  The bins live in LDS.
// THE COMMON BIN (o, j) = (0, 0) -- no event, no member -- IS NEVER SENT TO LDS: a thread counts its valid cells in a register, the
// workgroup adds those once, and bin (0, 0) = valid cells - the sum of the other bins.  Every other bin takes one LDS add per cell.
// The workgroup then issues one 64-bit add per non-zero bin to the zeroed output.
//
// fss_sums: rows d = 0 the truth, 1 .. M the members, M + 1 the ensemble (cell value = the member count).  n_d(c) = the sum of row d
// over the (2r + 1)^2 window centred on c, cells outside the domain 0.  out[t][f][k][s][d][0..1] = (sum_c n_d(c)^2, sum_c n_d(c) n_0(c)).
// A workgroup owns (plane, threshold k, tile): the loop over k runs over the GRID, the planes are re-read from the caches.  The tile is
// at most TILE x TILE cells; the region it stages is the tile plus a halo of the call's largest radius R (in x rounded up to a multiple
// of 4, so every load is 16 bytes), clipped to the domain: at most REGION x REGION.  A row's indicators go to LDS and become a summed-
// area table there (a scan along the rows, then along the columns), padded with a zero row and column so that a window sum is four
// reads at clipped corners; all S radii read the same table.  The truth's table stays while the members go by; the member count of
// every region cell accumulates as a byte (four to a word, each word owned by one thread) and gets a 32-bit table at the end, built
// over the bytes themselves: every thread takes its words into registers, a barrier, then it writes their 32-bit entries.  That keeps
// the workgroup under 80 KiB of LDS, so two of them share a CU and one scans while the other sums.
// Products and sums are 64-bit; a wave adds its threads' sums, the workgroup adds the waves' in LDS and issues one 64-bit add per
// entry to the zeroed output.
#ifndef C2W_EVENTS_CORE_H
#define C2W_EVENTS_CORE_H

#include "core_side.h"

#ifndef EV_VISIT_CELL  // the host driver counts here: a cell binned by the counts kernel; a region cell staged, a tile cell summed and
#define EV_VISIT_CELL(plane, k, cell)                // a table corner read by the FSS kernel (domain coordinates, corners 0 .. H / 0 .. W)
#define EV_VISIT_LOAD(d, gy, gx)
#define EV_VISIT_SUM(d, s, gy, gx)
#define EV_VISIT_CORNER(d, s, gy, gx)
#endif

namespace events {

constexpr int THREADS = 256;
constexpr int MAX_M = 64, MAX_K = 8, MAX_S = 8, MAX_R = 16;
constexpr int CHUNK = 4096;  // cells a workgroup of the counts kernel owns: 4 rounds of 256 threads, 4 cells each
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of rounds");
static_assert(MAX_M < 256, "four member counts ride in the bytes of one register");

typedef float F4 __attribute__((vector_size(16)));  // 16 bytes a load

// the indicator: the same bit on every route
static C2W_BOTH inline int event_of(float v, float thr, int above) { return above ? (v >= thr ? 1 : 0) : (v <= thr ? 1 : 0); }

#ifdef C2W_CORE_HOST
static inline void lds_inc(int* p) { ++*p; }
static inline void lds_add(int* p, int a) { *p += a; }
static inline void lds_add64(long long* p, long long a, int) { *p += a; }
static inline void global_add(long long* p, long long a) { *p += a; }
#else
static C2W_HD inline void lds_inc(int* p) { atomicAdd(p, 1); }
static C2W_HD inline void lds_add(int* p, int a) { atomicAdd(p, a); }
// every thread of the wave comes here: the wave adds first, one lane adds to LDS
static C2W_HD inline void lds_add64(long long* p, long long a, int tid) {
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((tid & 63) == 0 && a) atomicAdd((unsigned long long*)p, (unsigned long long)a);
}
static C2W_HD inline void global_add(long long* p, long long a) { atomicAdd((unsigned long long*)p, (unsigned long long)a); }
#endif

// ================================================================================================================ the joint table

constexpr int MAX_BINS = 2 * (MAX_M + 1);                  // (o, j) of one threshold
constexpr int COUNT_LDS_INTS = MAX_K * MAX_BINS + 2;       // the bins, the valid cells, the invalid cells: 4168 bytes

static C2W_BOTH inline bool counts_supported(int hw, int M, int K) { return hw >= 4 && hw % 4 == 0 && M >= 1 && M <= MAX_M && K >= 1 && K <= MAX_K; }
static C2W_BOTH inline int chunks(int hw) { return (hw + CHUNK - 1) / CHUNK; }
static C2W_BOTH inline int chunk_begin(int c) { return c * CHUNK; }
static C2W_BOTH inline int chunk_end(int hw, int c) { return (c + 1) * CHUNK < hw ? (c + 1) * CHUNK : hw; }
static C2W_BOTH inline int rounds(int hw, int c) { return (chunk_end(hw, c) - chunk_begin(c) + 4 * THREADS - 1) / (4 * THREADS); }
static C2W_BOTH inline int cell_of(int c, int it, int tid) { return chunk_begin(c) + (it * THREADS + tid) * 4; }
static C2W_BOTH inline int bins(int M) { return 2 * (M + 1); }
static C2W_BOTH inline int bin_of(int o, int j, int M) { return o * (M + 1) + j; }

struct CView {
    const float* x;      // [M][T][F][hw]
    const float* y;      // [T][F][hw]
    const float* thr;    // [F][K]
    const int* dir;      // [F][K]
    long long* counts;   // [T F][K][2][M + 1]
    long long* invalid;  // [T F]
    long long plane;     // t F + f
    int chunk;
    int M, T, F, hw, K;
    int* lds;  // COUNT_LDS_INTS
};

static C2W_HD inline void c_zero(const CView& v, int tid) {
    for (int i = tid; i < COUNT_LDS_INTS; i += THREADS) v.lds[i] = 0;
}

static C2W_HD inline void c_count(const CView& v, int tid) {
    const int f = (int)(v.plane % v.F), nb = bins(v.M);
    float thr[MAX_K];
    int above = 0;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
        thr[k] = k < v.K ? v.thr[f * v.K + k] : 0.f;
        above |= (k < v.K && v.dir[f * v.K + k] != 0) ? 1 << k : 0;
    }
    const long long member = (long long)v.T * v.F * v.hw;
    int n_valid = 0, n_invalid = 0;
    const int n = rounds(v.hw, v.chunk);
    for (int it = 0; it < n; ++it) {
        const int cell = cell_of(v.chunk, it, tid);
        if (cell >= chunk_end(v.hw, v.chunk)) break;
        const long long at = v.plane * v.hw + cell;
        const F4 g = *(const F4*)(v.y + at);
        unsigned nan = 0, cnt[MAX_K];
#pragma unroll
        for (int c = 0; c < 4; ++c) nan |= (g[c] != g[c]) ? 1u << c : 0u;
#pragma unroll
        for (int k = 0; k < MAX_K; ++k) cnt[k] = 0;
#pragma unroll 4
        for (int m = 0; m < v.M; ++m) {
            const F4 s = *(const F4*)(v.x + m * member + at);
#pragma unroll
            for (int c = 0; c < 4; ++c) nan |= (s[c] != s[c]) ? 1u << c : 0u;
#pragma unroll
            for (int k = 0; k < MAX_K; ++k) {
                if (k >= v.K) break;
                const int a = (above >> k) & 1;
#pragma unroll
                for (int c = 0; c < 4; ++c) cnt[k] += (unsigned)event_of(s[c], thr[k], a) << (8 * c);
            }
        }
#pragma unroll
        for (int k = 0; k < MAX_K; ++k) {
            if (k >= v.K) break;
            const int a = (above >> k) & 1;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if ((nan >> c) & 1) continue;
                EV_VISIT_CELL(v.plane, k, cell + c);
                const int b = bin_of(event_of(g[c], thr[k], a), (int)((cnt[k] >> (8 * c)) & 255u), v.M);
                if (b) lds_inc(v.lds + k * nb + b);  // bin (0, 0) is derived, never added
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) n_invalid += (int)((nan >> c) & 1), n_valid += 1 - (int)((nan >> c) & 1);
    }
    if (n_valid) lds_add(v.lds + MAX_K * MAX_BINS, n_valid);
    if (n_invalid) lds_add(v.lds + MAX_K * MAX_BINS + 1, n_invalid);
}

// bin (0, 0) of threshold tid = the valid cells - the other bins
static C2W_HD inline void c_derive(const CView& v, int tid) {
    if (tid >= v.K) return;
    const int nb = bins(v.M);
    int rest = 0;
    for (int b = 1; b < nb; ++b) rest += v.lds[tid * nb + b];
    v.lds[tid * nb] = v.lds[MAX_K * MAX_BINS] - rest;
}

static C2W_HD inline void c_flush(const CView& v, int tid) {
    const int n = v.K * bins(v.M);
    for (int i = tid; i < n; i += THREADS)
        if (v.lds[i]) global_add(v.counts + v.plane * n + i, (long long)v.lds[i]);
    if (tid == 0 && v.lds[MAX_K * MAX_BINS + 1]) global_add(v.invalid + v.plane, (long long)v.lds[MAX_K * MAX_BINS + 1]);
}

// ================================================================================================================ the FSS sums

constexpr int TILE = 64;                     // cells a workgroup owns along each axis
constexpr int REGION = TILE + 2 * MAX_R;     // 96: the tile and its halo
constexpr int RS = REGION + 1;               // row stride of a table: a zero row and column in front
constexpr int CNT_WORDS = REGION / 4;        // row stride of the member-count bytes, in words
static_assert(REGION * REGION < 65536, "an indicator row's table fits 16-bit entries");
static_assert(MAX_R % 4 == 0 && TILE % 4 == 0, "the region begins and ends on a 16-byte boundary");

constexpr int align16(int b) { return (b + 15) / 16 * 16; }
// the LDS budget of fss_sums_kernel, in bytes
constexpr int SAT16_BYTES = align16(RS * RS * 2);                 // 18832: the truth's table, and the current member's
constexpr int CNT_BYTES = REGION * REGION;                        //  9216: the member count of every region cell, a byte each ...
constexpr int SAT32_BYTES = align16(RS * RS * 4);                 // 37648: ... and, over the same bytes, the ensemble row's table
constexpr int RED_BYTES = 2 * MAX_S * 8;                          //   128: the workgroup's sums of one row
constexpr int OFF_SAT0 = 0, OFF_SATM = SAT16_BYTES, OFF_CNT = 2 * SAT16_BYTES, OFF_SATE = OFF_CNT, OFF_RED = OFF_SATE + SAT32_BYTES;
constexpr int FSS_LDS_BYTES = OFF_RED + RED_BYTES;                // 75440
constexpr int ENS_WORDS = (REGION * CNT_WORDS + THREADS - 1) / THREADS;  // 9: the count words a thread owns
static_assert(FSS_LDS_BYTES <= 160 * 1024, "the LDS of one CU");
static_assert(FSS_LDS_BYTES <= 80 * 1024, "two workgroups share a CU");
static_assert(CNT_BYTES <= SAT32_BYTES, "the ensemble row's table is built over the member counts");
static_assert(OFF_SATE % 16 == 0 && OFF_RED % 16 == 0, "aligned parts");

static C2W_BOTH inline bool radii_ok(const int* radii, int S) {
    if (S < 1 || S > MAX_S) return false;
    for (int s = 0; s < S; ++s)
        if (radii[s] < 0 || radii[s] > MAX_R) return false;
    return true;
}
static C2W_BOTH inline int max_radius(const int* radii, int S) {
    int R = 0;
    for (int s = 0; s < S; ++s) R = radii[s] > R ? radii[s] : R;
    return R;
}
// (M (2r + 1)^2)^2 H W < 2^62: the largest entry fits an int64 with room for the adds
static C2W_BOTH inline bool fss_no_overflow(int H, int W, int M, int R) {
    const long long n = (long long)M * (2 * R + 1) * (2 * R + 1);
    return n * n <= ((1LL << 62) - 1) / ((long long)H * W);
}
static C2W_BOTH inline bool fss_supported(int H, int W, int M, int K, const int* radii, int S) {
    if (H < 4 || W < 4 || W % 4 != 0 || (long long)H * W > (1LL << 20) || M < 1 || M > MAX_M || K < 1 || K > MAX_K) return false;
    return radii_ok(radii, S) && fss_no_overflow(H, W, M, max_radius(radii, S));
}

static C2W_BOTH inline int tiles_y(int H) { return (H + TILE - 1) / TILE; }
static C2W_BOTH inline int tiles_x(int W) { return (W + TILE - 1) / TILE; }

struct Radii {
    int r[MAX_S];
};

// the tile [ty0, ty0 + th) x [tx0, tx0 + tw) and the region [y0, y1) x [x0, x1) a workgroup stages for it
struct Geo {
    int ty0, tx0, th, tw, y0, x0, rh, rw;
};
static C2W_BOTH inline Geo geo_of(int H, int W, int R, int tile) {
    Geo g;
    const int Rx = (R + 3) / 4 * 4;
    g.ty0 = tile / tiles_x(W) * TILE, g.tx0 = tile % tiles_x(W) * TILE;
    g.th = H - g.ty0 < TILE ? H - g.ty0 : TILE, g.tw = W - g.tx0 < TILE ? W - g.tx0 : TILE;
    g.y0 = g.ty0 - R > 0 ? g.ty0 - R : 0, g.x0 = g.tx0 - Rx > 0 ? g.tx0 - Rx : 0;
    const int y1 = g.ty0 + g.th + R < H ? g.ty0 + g.th + R : H, x1 = g.tx0 + g.tw + Rx < W ? g.tx0 + g.tw + Rx : W;
    g.rh = y1 - g.y0, g.rw = x1 - g.x0;
    return g;
}

struct FView {
    const float* x;   // [M][T][F][H W]
    const float* y;   // [T][F][H W]
    const float* thr; // [F][K]
    const int* dir;   // [F][K]
    long long* out;   // [T F][K][S][M + 2][2]
    long long plane;  // t F + f
    int k, tile;
    int M, T, F, H, W, K, S, R;
    Radii radii;
    unsigned char* lds;  // FSS_LDS_BYTES
};

static C2W_HD inline unsigned short* sat0_of(const FView& v) { return (unsigned short*)(v.lds + OFF_SAT0); }
static C2W_HD inline unsigned short* satm_of(const FView& v) { return (unsigned short*)(v.lds + OFF_SATM); }
static C2W_HD inline unsigned* cnt_of(const FView& v) { return (unsigned*)(v.lds + OFF_CNT); }
static C2W_HD inline unsigned* sate_of(const FView& v) { return (unsigned*)(v.lds + OFF_SATE); }
static C2W_HD inline long long* red_of(const FView& v) { return (long long*)(v.lds + OFF_RED); }

// the zero row and column of the two 16-bit tables, the member counts and the sums
static C2W_HD inline void f_zero(const FView& v, int tid) {
    unsigned short *a = sat0_of(v), *b = satm_of(v);
    unsigned* cnt = cnt_of(v);
    for (int i = tid; i < RS; i += THREADS) {
        a[i] = 0, b[i] = 0;
        a[i * RS] = 0, b[i * RS] = 0;
    }
    for (int i = tid; i < REGION * CNT_WORDS; i += THREADS) cnt[i] = 0;
    if (tid < 2 * MAX_S) red_of(v)[tid] = 0;
}

// row d's indicators over the region: d = 0 the truth into its table; d = 1 .. M a member into the member's table and onto the counts
static C2W_HD inline void f_load(const FView& v, const Geo& g, int tid, int d) {
    const int f = (int)(v.plane % v.F), above = v.dir[f * v.K + v.k] != 0 ? 1 : 0;
    const float thr = v.thr[f * v.K + v.k];
    const long long hw = (long long)v.H * v.W;
    const float* src = d == 0 ? v.y + v.plane * hw : v.x + ((long long)(d - 1) * v.T * v.F + v.plane) * hw;
    unsigned short* sat = d == 0 ? sat0_of(v) : satm_of(v);
    unsigned* cnt = cnt_of(v);
    const int qw = g.rw / 4;
    for (int q = tid; q < g.rh * qw; q += THREADS) {
        const int i = q / qw, j = q % qw * 4;
        const F4 s = *(const F4*)(src + (long long)(g.y0 + i) * v.W + g.x0 + j);
        unsigned packed = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = event_of(s[c], thr, above);
            EV_VISIT_LOAD(d, g.y0 + i, g.x0 + j + c);
            sat[(i + 1) * RS + j + c + 1] = (unsigned short)e;
            packed |= (unsigned)e << (8 * c);
        }
        if (d > 0) cnt[i * CNT_WORDS + j / 4] += packed;  // this word is this thread's in every row
    }
}

// the member counts as the ensemble row, in two phases with a barrier between them: the table lies over the bytes it is made from
struct EnsThread {
    unsigned w[ENS_WORDS];
};
static C2W_HD inline void f_ensemble_take(const FView& v, const Geo& g, int tid, EnsThread& th) {
    const unsigned* cnt = cnt_of(v);
    const int qw = g.rw / 4;
#pragma unroll
    for (int n = 0; n < ENS_WORDS; ++n) {
        const int q = tid + n * THREADS;
        th.w[n] = q < g.rh * qw ? cnt[q / qw * CNT_WORDS + q % qw] : 0u;
    }
}
static C2W_HD inline void f_ensemble_put(const FView& v, const Geo& g, int tid, const EnsThread& th) {
    unsigned* sat = sate_of(v);
    const int qw = g.rw / 4;
    for (int i = tid; i < RS; i += THREADS) sat[i] = 0, sat[i * RS] = 0;  // cells (i + 1, j + 1) below never touch row 0 or column 0
#pragma unroll
    for (int n = 0; n < ENS_WORDS; ++n) {
        const int q = tid + n * THREADS;
        if (q >= g.rh * qw) break;
        const int i = q / qw, j = q % qw * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) sat[(i + 1) * RS + j + c + 1] = (th.w[n] >> (8 * c)) & 255u;
    }
}

// the two scans that turn the staged row into its summed-area table: thread i owns region row i, then thread j region column j
template <typename E>
static C2W_HD inline void f_scan_rows(E* sat, const Geo& g, int tid) {
    for (int i = tid; i < g.rh; i += THREADS) {
        E run = 0, a[4];
        E* row = sat + (i + 1) * RS + 1;
        for (int j = 0; j < g.rw; j += 4) {  // the region is a whole number of quads wide: four reads in flight, then the chain
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = row[j + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) row[j + u] = run = (E)(run + a[u]);
        }
    }
}
template <typename E>
static C2W_HD inline void f_scan_cols(E* sat, const Geo& g, int tid) {
    for (int j = tid; j < g.rw; j += THREADS) {
        E run = 0, a[4];
        E* col = sat + RS + j + 1;
        int i = 0;
        for (; i + 4 <= g.rh; i += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = col[(i + u) * RS];
#pragma unroll
            for (int u = 0; u < 4; ++u) col[(i + u) * RS] = run = (E)(run + a[u]);
        }
        for (; i < g.rh; ++i) col[i * RS] = run = (E)(run + col[i * RS]);
    }
}

// the window sum of radius r centred on region cell (ry, rx): four reads at corners clipped to the region, which is the domain's clip
template <typename E>
static C2W_HD inline long long window_of(const E* sat, const Geo& g, int ry, int rx, int r, int d, int s) {
    const int a0 = ry - r > 0 ? ry - r : 0, a1 = ry + r + 1 < g.rh ? ry + r + 1 : g.rh;
    const int b0 = rx - r > 0 ? rx - r : 0, b1 = rx + r + 1 < g.rw ? rx + r + 1 : g.rw;
    EV_VISIT_CORNER(d, s, g.y0 + a0, g.x0 + b0);
    EV_VISIT_CORNER(d, s, g.y0 + a0, g.x0 + b1);
    EV_VISIT_CORNER(d, s, g.y0 + a1, g.x0 + b0);
    EV_VISIT_CORNER(d, s, g.y0 + a1, g.x0 + b1);
    (void)d, (void)s;
    return (long long)sat[a1 * RS + b1] - (long long)sat[a0 * RS + b1] - (long long)sat[a1 * RS + b0] + (long long)sat[a0 * RS + b0];
}

// (sum n_d^2, sum n_d n_0) of row d over the tile's cells at every radius, into the workgroup's sums
template <typename E>
static C2W_HD inline void f_sums(const FView& v, const Geo& g, int tid, const E* sat, int d) {
    const unsigned short* sat0 = sat0_of(v);
    long long pp[MAX_S], po[MAX_S];
#pragma unroll
    for (int s = 0; s < MAX_S; ++s) pp[s] = 0, po[s] = 0;
    for (int c = tid; c < g.th * g.tw; c += THREADS) {
        const int ry = g.ty0 + c / g.tw - g.y0, rx = g.tx0 + c % g.tw - g.x0;
#pragma unroll
        for (int s = 0; s < MAX_S; ++s) {
            if (s >= v.S) break;
            EV_VISIT_SUM(d, s, g.y0 + ry, g.x0 + rx);
            const long long n = window_of(sat, g, ry, rx, v.radii.r[s], d, s), n0 = window_of(sat0, g, ry, rx, v.radii.r[s], -1, s);
            pp[s] += n * n, po[s] += n * n0;
        }
    }
    long long* red = red_of(v);
#pragma unroll
    for (int s = 0; s < MAX_S; ++s) {
        if (s >= v.S) break;
        lds_add64(red + 2 * s, pp[s], tid);
        lds_add64(red + 2 * s + 1, po[s], tid);
    }
}

// thread e = 2 s + column adds the workgroup's sum of row d to the output and clears it for the next row
static C2W_HD inline void f_flush(const FView& v, int tid, int d) {
    if (tid >= 2 * v.S) return;
    long long* red = red_of(v);
    const int s = tid / 2, col = tid % 2;
    if (red[tid]) global_add(v.out + ((((v.plane * v.K + v.k) * v.S + s) * (v.M + 2) + d) * 2 + col), red[tid]);
    red[tid] = 0;
}

}  // namespace events
#endif
