// Ensemble marginals: the index maps and the arithmetic of kde.hip (Gaussian kernel density estimates and the rank histogram), written
// as barrier-separated phases over "thread tid of a workgroup", as swd_core.h is.  Compiled for the host (core_side.h) the same phases
// run one thread after the other over a record per thread: tests/host_kde_main.cpp checks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_kde_eval, c2w_pit_counts).  A data set is one (member, variable) or (truth, variable) over all T times and
// hw cells, n = T hw values; data set ds < n_rep F is member ds / F, variable ds % F of x[n_rep][T][F][hw], the others are variable
// ds - n_rep F of the truth y[T][F][hw].
//   f(g_j) = (1 / (n h sqrt(2 pi))) sum_i exp(-(g_j - x_i)^2 / (2 h^2)),   j < N, h = h[ds]
//
// kde_partial: a workgroup of 256 owns one data set and one chunk of its values (chunk_len: a function of n alone); thread tid owns the
// grid points j = tid + 256 r, r < 4 (N <= 1024), each an fp32 accumulator in a register.  exp(-u^2 / 2) = exp2(-t^2) with
// t = (g - x) k, k = sqrt(log2(e) / 2) / h rounded to fp32 once per data set.  The host hands the grid over as fp32 offsets
// o_j = g_j - c[f] from an fp32 pivot c[f] near the middle of the grid; the thread forms gk_j = o_j k in double and rounds it once.  A
// tile of 1024 values is loaded 16 bytes a thread, x - c is formed in fp32 ON THE LOADED VALUE, before anything else touches it (exact
// whenever x and c lie within a factor of two of each other, as on a pressure field at 101325 +- 1200: a value near 1e5 never meets k
// or a grid point), and goes to LDS; then every thread walks the tile, four values per 16-byte broadcast read, and per pair does
//   t = fma(-(x - c), k, gk_j);  s = t t;  e = v_exp_f32(-s);  acc_j += e            (one fma, one multiply, one exp, one add)
// An fp32 chain holds at most FOLD = 256 terms, then joins a double in value order; the chunk's N doubles go to
// partial[ds][chunk][j].  A value that is not finite makes the whole workgroup write NaN instead.  No atomics: a data set's partials
// are the same bits whatever else rides in the launch.
// kde_fold: thread j of data set ds adds the chunks in index order in double and multiplies by 1 / (n h sqrt(2 pi)) in double; a NaN
// sum is written as NaN explicitly.
//
// pit_count: counts[f][r] += 1 for every (t, cell) with r = #{m : x[m][t][f][cell] <= y[t][f][cell]}, r = 0 .. M (IEEE <=: ties count,
// a NaN on either side does not).  Workgroup b of G (a multiple of F) owns variable b % F and the times b / F, b / F + G / F, ...: its
// variable never changes.  Thread tid owns the 16-byte cell quads tid, tid + 256, ... of a plane; it reads the truth once and the M
// members at stride T F hw, counts per cell in registers and adds one to hist[tid % 16][r] in LDS (16 copies: at most four lanes of a
// wave meet on one address); at the end thread r < M + 1 adds its bin's 16 copies and issues ONE global integer add.
#ifndef C2W_KDE_CORE_H
#define C2W_KDE_CORE_H

#include "core_side.h"
#include "ordered_sum.h"

namespace kde {

constexpr int THREADS = 256;
static_assert(THREADS == ordered_sum::THREADS, "the workgroup the fixed-order sum is written for");
constexpr int MAX_N = 1024;           // grid points: four a thread at most
constexpr int TILE = 4 * THREADS;     // values staged per barrier pair: one 16-byte load a thread
constexpr int FOLD = 256;             // terms an fp32 chain holds before it joins its double
static_assert(TILE % FOLD == 0 && FOLD % 4 == 0, "a tile is a whole number of chains, a chain a whole number of 16-byte reads");
// Chunks per data set once n is large.  The reference's report has D = 8 x 4 + 4 = 36 data sets: 36 x 64 = 2304 workgroups of four
// waves, nine for each of the 256 CUs of an MI355X, six of them resident at a time (78 registers at four points a thread, 4 KiB of
// LDS), so no CU idles before the last few percent; the scratch is 36 x 64 x 1000 doubles = 18 MiB.  A constant, not a function of D
// or of the CU count: the bits of a data set are fixed by (n, N).
constexpr int MAX_CHUNKS = 64;
constexpr int PIT_MAX_M = 64;
constexpr int PIT_COPIES = 16;
constexpr int PIT_HIST = PIT_COPIES * (PIT_MAX_M + 1);

constexpr double SQRT_HALF_LOG2E = 0.84932180028801904272;  // sqrt(log2(e) / 2)
constexpr double SQRT_2PI = 2.50662827463100050242;

static C2W_BOTH inline bool supported(int hw, int N) { return hw >= 4 && hw % 4 == 0 && N >= 1 && N <= MAX_N; }
static C2W_BOTH inline bool pit_supported(int hw, int M) { return hw >= 4 && hw % 4 == 0 && M >= 1 && M <= PIT_MAX_M; }

// ---------------------------------------------------------------------------------------------------------------- maps

// values per chunk: n / 64 rounded up to whole tiles, one tile at least; chunk c owns values c len .. min(n, (c + 1) len) - 1
static C2W_BOTH inline long long chunk_len(long long n) {
    const long long per = (n + MAX_CHUNKS - 1) / MAX_CHUNKS;
    const long long len = (per + TILE - 1) / TILE * TILE;
    return len < TILE ? TILE : len;
}
static C2W_BOTH inline long long chunks(long long n) { return (n + chunk_len(n) - 1) / chunk_len(n); }
static C2W_BOTH inline long long chunk_begin(long long n, long long c) { return c * chunk_len(n); }
static C2W_BOTH inline long long chunk_end(long long n, long long c) {
    const long long e = (c + 1) * chunk_len(n);
    return e < n ? e : n;
}
// the float offset of value i of a data set from the data set's first value: time i / hw, cell i % hw; times lie F hw apart
static C2W_BOTH inline long long value_offset(long long i, int F, int hw) { return (i / hw) * ((long long)F * hw) + i % hw; }
// the grid point register r of thread tid holds; points past N are computed from point N - 1 and dropped
static C2W_BOTH inline int point_of(int tid, int r) { return r * THREADS + tid; }
static C2W_BOTH inline int points_per_thread(int N) { return (N + THREADS - 1) / THREADS; }
// rank histogram: workgroup b of G owns variable b % F and times b / F + k (G / F); a cell's bin is its rank, in copy tid % 16
static C2W_BOTH inline int pit_var(long long b, int F) { return (int)(b % F); }
static C2W_BOTH inline long long pit_first_t(long long b, int F) { return b / F; }
static C2W_BOTH inline int pit_slot(int tid, int r, int M) { return (tid % PIT_COPIES) * (M + 1) + r; }

// ---------------------------------------------------------------------------------------------------------------- density: phases

struct KView {
    const float* x;       // samples [n_rep][T][F][hw]
    const float* y;       // truth [T][F][hw] or null
    const float* off;     // [F][N] fp32 offsets g - c
    const float* pivot;   // [F]
    const double* h;      // [D]
    double* partial;      // [D][chunks][N]
    long long n_x;        // n_rep F
    long long ds, chunk;  // this workgroup's
    int T, F, hw, N;
    float4* lds;          // THREADS float4
};

template <int P>
struct KThread {
    const float* base;  // the data set's first value
    long long n, begin, end;
    float c, k;
    float gk[P], acc[P];
    double tot[P];
    float4 raw;
    int has, bad;
};

static C2W_BOTH inline int var_of(const KView& v) { return (int)(v.ds < v.n_x ? v.ds % v.F : v.ds - v.n_x); }

template <int P>
static C2W_HD inline void k_init(const KView& v, KThread<P>& th, int tid) {
    const int f = var_of(v);
    th.base = v.ds < v.n_x ? v.x + ((v.ds / v.F) * v.T * v.F + f) * (long long)v.hw : v.y + (long long)f * v.hw;
    th.n = (long long)v.T * v.hw;
    th.begin = chunk_begin(th.n, v.chunk), th.end = chunk_end(th.n, v.chunk);
    th.c = v.pivot[f];
    th.k = (float)(SQRT_HALF_LOG2E / v.h[v.ds]);
    th.bad = 0;
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int j = point_of(tid, r) < v.N ? point_of(tid, r) : v.N - 1;
        th.gk[r] = (float)((double)v.off[(long long)f * v.N + j] * (double)th.k);
        th.acc[r] = 0.f, th.tot[r] = 0.0;
    }
}

// the thread's 16 bytes of tile `tile` of the chunk (hw % 4 == 0: four neighbouring values share their time)
template <int P>
static C2W_HD inline void k_fetch(const KView& v, KThread<P>& th, int tid, long long tile) {
    const long long i = th.begin + tile * TILE + 4 * tid;
    th.has = i < th.end;
    if (th.has) th.raw = *(const float4*)(th.base + value_offset(i, v.F, v.hw));
}

// x - c: one rounding, on the loaded value, before anything else
template <int P>
static C2W_HD inline void k_stash(const KView& v, KThread<P>& th, int tid) {
    if (!th.has) return;
    const float4 q = th.raw;
    const float4 o = float4{q.x - th.c, q.y - th.c, q.z - th.c, q.w - th.c};
    th.bad |= (o.x - o.x != 0.f) | (o.y - o.y != 0.f) | (o.z - o.z != 0.f) | (o.w - o.w != 0.f);  // inf - inf and NaN - NaN are NaN
    v.lds[tid] = o;
}

#ifdef C2W_CORE_HOST
static inline float exp2_neg(float s) { return exp2f(-s); }
#else
static C2W_HD inline float exp2_neg(float s) { return __builtin_amdgcn_exp2f(-s); }  // v_exp_f32 with the sign as a source modifier
#endif

template <int P>
static C2W_HD inline void k_pair(KThread<P>& th, float xo) {
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const float t = __builtin_fmaf(-xo, th.k, th.gk[r]);
        th.acc[r] += exp2_neg(t * t);
    }
}

template <int P>
static C2W_HD inline void k_fold(KThread<P>& th) {
#pragma unroll
    for (int r = 0; r < P; ++r) th.tot[r] += (double)th.acc[r], th.acc[r] = 0.f;
}

// the `count` values of the staged tile (a multiple of 4), in value order; every thread reads the same 16 bytes at a time
template <int P>
static C2W_HD inline void k_compute(const KView& v, KThread<P>& th, int count) {
    for (int first = 0; first < count; first += FOLD) {
        const int stop = first + FOLD < count ? first + FOLD : count;
#pragma unroll 2
        for (int q = first / 4; q < stop / 4; ++q) {
            const float4 b = v.lds[q];
            k_pair(th, b.x), k_pair(th, b.y), k_pair(th, b.z), k_pair(th, b.w);
        }
        k_fold(th);
    }
}

template <int P>
static C2W_HD inline long long k_tiles(const KThread<P>& th) { return (th.end - th.begin + TILE - 1) / TILE; }
template <int P>
static C2W_HD inline int k_count(const KThread<P>& th, long long tile) {
    const long long left = th.end - th.begin - tile * TILE;
    return (int)(left < TILE ? left : TILE);
}

template <int P>
static C2W_HD inline void k_store(const KView& v, const KThread<P>& th, int tid, int bad) {
    double* row = v.partial + (v.ds * chunks(th.n) + v.chunk) * v.N;
#pragma unroll
    for (int r = 0; r < P; ++r)
        if (point_of(tid, r) < v.N) row[point_of(tid, r)] = bad ? (double)__builtin_nanf("") : th.tot[r];
}

// dens[ds][j]: the chunks in index order, then the normalisation, all in double
static C2W_HD inline void f_fold(const double* partial, const double* h, double* dens, long long ds, int j, long long n, int N) {
    const long long nc = chunks(n);
    const double s = ordered_sum::fold_strided(partial + ds * nc * N + j, nc, N);  // fold_parts at entry ds N + j, undivided
    dens[ds * N + j] = s != s ? (double)__builtin_nanf("") : s * (1.0 / ((double)n * h[ds] * SQRT_2PI));
}

// ---------------------------------------------------------------------------------------------------------------- rank histogram: phases

struct PView {
    const float* x;     // [M][T][F][hw]
    const float* y;     // [T][F][hw]
    long long* counts;  // [F][M + 1]
    long long block, grid;
    int M, T, F, hw;
    int* hist;  // PIT_HIST
};

#ifdef C2W_CORE_HOST
static inline void lds_inc(int* p) { ++*p; }
static inline void global_add(long long* p, long long a) { *p += a; }
#else
static C2W_HD inline void lds_inc(int* p) { atomicAdd(p, 1); }
static C2W_HD inline void global_add(long long* p, long long a) { atomicAdd((unsigned long long*)p, (unsigned long long)a); }
#endif

static C2W_HD inline void pit_zero(const PView& v, int tid) {
    for (int i = tid; i < PIT_COPIES * (v.M + 1); i += THREADS) v.hist[i] = 0;
}

static C2W_HD inline void pit_count(const PView& v, int tid) {
    const int f = pit_var(v.block, v.F), quads = v.hw / 4;
    const long long plane = (long long)v.F * v.hw, member = (long long)v.T * plane;
    for (long long t = pit_first_t(v.block, v.F); t < v.T; t += v.grid / v.F)
        for (int q = tid; q < quads; q += THREADS) {
            const long long at = t * plane + (long long)f * v.hw + 4 * q;
            const float4 g = *(const float4*)(v.y + at);
            int r0 = 0, r1 = 0, r2 = 0, r3 = 0;
#pragma unroll 4
            for (int m = 0; m < v.M; ++m) {
                const float4 s = *(const float4*)(v.x + m * member + at);
                r0 += s.x <= g.x, r1 += s.y <= g.y, r2 += s.z <= g.z, r3 += s.w <= g.w;
            }
            lds_inc(v.hist + pit_slot(tid, r0, v.M)), lds_inc(v.hist + pit_slot(tid, r1, v.M));
            lds_inc(v.hist + pit_slot(tid, r2, v.M)), lds_inc(v.hist + pit_slot(tid, r3, v.M));
        }
}

static C2W_HD inline void pit_flush(const PView& v, int tid) {
    if (tid > v.M) return;
    long long s = 0;
    for (int c = 0; c < PIT_COPIES; ++c) s += v.hist[c * (v.M + 1) + tid];
    if (s) global_add(v.counts + (long long)pit_var(v.block, v.F) * (v.M + 1) + tid, s);
}

}  // namespace kde
#endif
