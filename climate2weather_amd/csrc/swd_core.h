// Sliced Wasserstein distance of an ensemble to the truth: the index maps and the arithmetic of swd.hip, written as barrier-separated
// phases over "thread tid of a workgroup", as ssim_core.h is.  Compiled for the host (core_side.h) the same phases run one thread after
// the other over a record per thread, and the matrix-core step is replaced by mfma_32x32x2_host, which restates the lane maps and the
// k order of v_mfma_f32_32x32x2_f32 in plain C++: tests/host_swd_main.cpp checks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_swd_project, c2w_swd_distance).  For one variable, samples X (T, d), truth Y (T, d), unit columns theta_p:
//   a = X^ theta_p, b = Y^ theta_p with x^ = (x - shift[f]) * scale[f];  D_p = mean_i (sort(a)_i - sort(b)_i)^2;  SWD = sqrt(mean_p D_p).
//
// Projection: a GEMM, rows = all n_rep T F fields (row i is variable i % F), columns = P projections, K = d.  A workgroup of 512 owns
// BM = 64 fields x all P (padded to BN = 128) projections, so a field is read once and theta once per 64 fields (from L2 / the
// Infinity Cache: 16384 fields of 128 x 128 are 256 workgroups, one a CU, where tiles of 128 fields left half the chip idle).  K runs
// in steps of BK = 32: the next step's 16 bytes of x and 2 x 16 of theta per thread are in flight while this one is multiplied; x^ is
// formed in fp32 on the loaded value BEFORE any product (a pressure near 101325 never meets theta) and both tiles go to one of two LDS
// buffers, rows of LDK = 36 floats so that the 16-byte fragment reads of 16 neighbouring rows fall into 64 different banks.  Wave
// w = (wm, wn) of the 8 owns fields 32 wm .. + 31 and projections 32 wn .. + 31: one 32 x 32 tile, one v_mfma_f32_32x32x2_f32 per k
// pair, two waves a SIMD.  A lane's 16 bytes hold k = 8 g + 4 h .. + 3 (h = lane / 32), and step s of group g multiplies k = 8 g + s
// (h = 0) then k = 8 g + 4 + s (h = 1): the k order of a step is 0 4 1 5 2 6 3 7 | 8 12 ..., the same for every row, fixed by nothing.
// The accumulator is folded into a second one every FOLD = 8 steps (256 k) and at the end, in ascending order: a sum is a chain of
// d / 256 chunk sums of 256-long fmaf chains, fixed by d alone.  No atomics, no scratch; rows past n_fields and columns past P are
// computed from clamped addresses and dropped.  Epilogue: the 64 x 128 sums go through LDS ([projection][field], EPI_LD = 65) and leave
// as proj[rep][f][p][t], threads running along t for one (p, i % F) so that a column to sort is written in contiguous pieces.
//
// Distance: one workgroup per column pair (rep, f, p).  Both columns are loaded into LDS padded with +inf to N = the next power of two,
// a NaN seen at load makes the result NaN explicitly; a bitonic network sorts the two columns side by side (the padding sorts to the
// end and never enters the sum); differences and squares in double, thread partials over i = tid, tid + nthr, ..., 16 second-level
// sums of neighbouring partials, one sum of those: an order fixed by T.
#ifndef C2W_SWD_CORE_H
#define C2W_SWD_CORE_H

#include "core_side.h"

namespace swd {

constexpr int THREADS = 512;
constexpr int BM = 64, BN = 128, BK = 32;
constexpr int LDK = BK + 4;                      // floats per LDS row of a staged tile
constexpr int XT_FLOATS = BM * LDK;              // the x^ tile
constexpr int BUF_FLOATS = (BM + BN) * LDK;      // x^ tile | theta tile
constexpr int LDS_FLOATS = 2 * BUF_FLOATS;       // two buffers: 54 KiB, static
constexpr int FOLD = 8;                      // steps between two folds of the accumulators: 256 k
constexpr int EPI_LD = BM + 1;               // floats per projection row of the epilogue's tile
static_assert(BN * EPI_LD <= LDS_FLOATS, "the epilogue's tile reuses the staging buffers");
constexpr int LOADS = BN * BK / 4 / THREADS;  // 16-byte loads of theta per thread and step: 2 (and BM * BK / 4 / THREADS = 1 of x)
static_assert(BM * BK / 4 == THREADS, "one 16-byte load of x per thread and step");
constexpr int MAX_D = 65536, MAX_P = BN, MAX_T = 16384;
constexpr int SORT_DOUBLES = 1024 + 16;  // one partial per thread | 16 second-level sums

static C2W_BOTH inline bool project_supported(int d, int P) { return d >= 64 && d <= MAX_D && d % 64 == 0 && P >= 1 && P <= MAX_P; }
static C2W_BOTH inline bool distance_supported(int T) { return T >= 1 && T <= MAX_T; }
static C2W_BOTH inline int padded(int T) {
    int n = 1;
    while (n < T) n <<= 1;
    return n;
}
static C2W_BOTH inline int sort_threads(int N) { return N <= 2048 ? 256 : 1024; }

#ifdef C2W_CORE_HOST
struct V16 {
    float v[16];
    float& operator[](int i) { return v[i]; }
    float operator[](int i) const { return v[i]; }
};
#else
typedef __attribute__((ext_vector_type(16))) float V16;
#endif

static C2W_HD inline float comp(const float4& q, int s) { return s == 0 ? q.x : s == 1 ? q.y : s == 2 ? q.z : q.w; }

// ---------------------------------------------------------------------------------------------------------------- projection: maps

// load j of thread tid brings 16 bytes of row stage_row, floats 4 stage_c4 .. + 3 of the step's 32 (x: j = 0 only)
static C2W_HD inline int stage_row(int tid, int j) { return (tid + THREADS * j) >> 3; }
static C2W_HD inline int stage_c4(int tid, int j) { return (tid + THREADS * j) & 7; }
// the 16 bytes lane `lane` of wave `wave` reads of its fields / its projections for k group g of a step: offsets into a buffer
static C2W_HD inline int frag_a(int wave, int lane, int g) { return ((wave >> 2) * 32 + (lane & 31)) * LDK + 8 * g + 4 * (lane >> 5); }
static C2W_HD inline int frag_b(int wave, int lane, int g) { return XT_FLOATS + ((wave & 3) * 32 + (lane & 31)) * LDK + 8 * g + 4 * (lane >> 5); }
// where register r of lane `lane` of a 32 x 32 result tile lies (the matrix core's C/D map)
static C2W_HD inline int acc_row(int lane, int r) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
static C2W_HD inline int acc_col(int lane) { return lane & 31; }
// whether wave `wave` has to multiply at all (else its 32 columns lie past P)
static C2W_HD inline bool active(int wave, int P) { return (wave & 3) * 32 < P; }
// proj[rep][f][p][t] of field i = (rep T + t) F + f
static C2W_HD inline long long out_index(long long i, int p, int T, int F, int P) {
    const long long rep = i / ((long long)T * F);
    const int t = (int)((i / F) % T), f = (int)(i % F);
    return ((rep * F + f) * P + p) * (long long)T + t;
}

struct PView {
    const float* x;
    const float* theta;
    const float* shift;
    const float* scale;
    float* proj;
    long long n_fields, first;  // all rows of the GEMM; the first row of this workgroup
    int T, F, d, P;
    float* lds;
};

struct PThread {
    long long xo, to[LOADS];  // element offsets of the thread's loads at k = 0
    float sh, sc;
    float4 rx, rt[LOADS];
    V16 acc, tot;
};

static C2W_HD inline void p_init(const PView& v, PThread& th, int tid) {
    long long i = v.first + stage_row(tid, 0);
    if (i > v.n_fields - 1) i = v.n_fields - 1;  // a row past the end reads the last field again and is dropped in the epilogue
    th.xo = i * v.d + 4 * stage_c4(tid, 0);
    th.sh = v.shift[i % v.F], th.sc = v.scale[i % v.F];
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
        const int row = stage_row(tid, j), p = row < v.P ? row : v.P - 1;
        th.to[j] = (long long)p * v.d + 4 * stage_c4(tid, j);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) th.acc[r] = 0.f, th.tot[r] = 0.f;
}

static C2W_HD inline void p_fetch(const PView& v, PThread& th, int kt) {
    th.rx = *(const float4*)(v.x + th.xo + (long long)kt * BK);
#pragma unroll
    for (int j = 0; j < LOADS; ++j) th.rt[j] = *(const float4*)(v.theta + th.to[j] + (long long)kt * BK);
}

// x^ = (x - shift) * scale: two roundings, on the loaded value
static C2W_HD inline void p_stash(const PView& v, const PThread& th, int tid, int buf) {
    float* base = v.lds + buf * BUF_FLOATS;
    const float4 q = th.rx;
    const float s = th.sh, c = th.sc;
    *(float4*)(base + stage_row(tid, 0) * LDK + 4 * stage_c4(tid, 0)) = float4{(q.x - s) * c, (q.y - s) * c, (q.z - s) * c, (q.w - s) * c};
#pragma unroll
    for (int j = 0; j < LOADS; ++j) *(float4*)(base + XT_FLOATS + stage_row(tid, j) * LDK + 4 * stage_c4(tid, j)) = th.rt[j];
}

#ifdef C2W_CORE_HOST
// v_mfma_f32_32x32x2_f32 restated: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; D[i][j] is register
// (i & 3) + 4 (i >> 3) of lane j + 32 ((i >> 2) & 1); D = fma(A[i][1], B[1][j], fma(A[i][0], B[0][j], C)).
static inline void mfma_32x32x2_host(const float (&a)[64], const float (&b)[64], V16* (&c)[64]) {
    for (int i = 0; i < 32; ++i)
        for (int j = 0; j < 32; ++j) {
            float& d = (*c[j + 32 * ((i >> 2) & 1)])[(i & 3) + 4 * (i >> 3)];
            d = __builtin_fmaf(a[i + 32], b[j + 32], __builtin_fmaf(a[i], b[j], d));
        }
}
// one step of one wave: th points at the wave's 64 thread records
static inline void p_compute_wave(const PView& v, PThread* th, int wave, int buf) {
    const float* base = v.lds + buf * BUF_FLOATS;
    if (!active(wave, v.P)) return;
    for (int g = 0; g < BK / 8; ++g)
        for (int s = 0; s < 4; ++s) {
            float a[64], b[64];
            V16* c[64];
            for (int l = 0; l < 64; ++l) {
                a[l] = base[frag_a(wave, l, g) + s], b[l] = base[frag_b(wave, l, g) + s];
                c[l] = &th[l].acc;
            }
            mfma_32x32x2_host(a, b, c);
        }
}
#else
static C2W_HD inline void p_compute(const PView& v, PThread& th, int tid, int buf) {
    const float* base = v.lds + buf * BUF_FLOATS;
    const int wave = tid >> 6, lane = tid & 63;
    if (!active(wave, v.P)) return;
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) {
        const float4 a = *(const float4*)(base + frag_a(wave, lane, g)), b = *(const float4*)(base + frag_b(wave, lane, g));
#pragma unroll
        for (int s = 0; s < 4; ++s) th.acc = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(a, s), comp(b, s), th.acc, 0, 0, 0);
    }
}
#endif

// the chunk's sums join the running sums, in ascending chunk order
static C2W_HD inline void p_fold(PThread& th) {
#pragma unroll
    for (int r = 0; r < 16; ++r) th.tot[r] += th.acc[r], th.acc[r] = 0.f;
}

// epilogue 1: the sums into LDS as [projection][field]
static C2W_HD inline void p_epi_stash(const PView& v, const PThread& th, int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    if (!active(wave, v.P)) return;
    const int n = (wave & 3) * 32 + acc_col(lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) v.lds[n * EPI_LD + (wave >> 2) * 32 + acc_row(lane, r)] = th.tot[r];
}

// epilogue 2: element e = (p, a, b) is field first + b F + a: for one p and a, neighbouring threads write neighbouring t
static C2W_HD inline void p_epi_write(const PView& v, int tid) {
    const int q = v.F >= BM ? 1 : (BM + v.F - 1) / v.F, per_p = q * v.F;  // F > BM: b = 0 and a = the row, rows past BM skipped
    const long long total = (long long)v.P * per_p;
    for (long long e = tid; e < total; e += THREADS) {
        const int p = (int)(e / per_p), r = (int)(e % per_p), mm = (r % q) * v.F + r / q;
        const long long i = v.first + mm;
        if (mm >= BM || i >= v.n_fields) continue;
        v.proj[out_index(i, p, v.T, v.F, v.P)] = v.lds[p * EPI_LD + mm];
    }
}

// ---------------------------------------------------------------------------------------------------------------- distance

struct DView {
    const float* px;
    const float* py;
    double* out;
    long long block;  // (rep F + f) P + p
    int F, P, T, N, nthr;
    float* keys;    // column of x: N floats | column of y: N floats
    double* dpart;  // SORT_DOUBLES
};

// phase 0: both columns into LDS, +inf past T; -> whether this thread saw a NaN
static C2W_HD inline int d_load(const DView& v, int tid) {
    const float* cx = v.px + v.block * v.T;
    const float* cy = v.py + (v.block % ((long long)v.F * v.P)) * v.T;
    int nan = 0;
    for (int i = tid; i < v.N; i += v.nthr) {
        const float a = i < v.T ? cx[i] : __builtin_inff(), b = i < v.T ? cy[i] : __builtin_inff();
        nan |= (a != a) | (b != b);
        v.keys[i] = a, v.keys[v.N + i] = b;
    }
    return nan;
}

// the pair compare-exchange `idx` of a stage touches: elements i and i + j of a column, ascending where (i & k) == 0
static C2W_HD inline int pair_low(int idx, int j) { return ((idx & ~(j - 1)) << 1) | (idx & (j - 1)); }

// phase (k, j): N / 2 compare-exchanges in each of the two columns
static C2W_HD inline void d_stage(const DView& v, int tid, int k, int j) {
    const int half = v.N >> 1;
    for (int e = tid; e < v.N; e += v.nthr) {
        const int col = e >= half, i = pair_low(e - col * half, j), l = i + j;
        float* c = v.keys + col * v.N;
        const float a = c[i], b = c[l];
        if ((a > b) == ((i & k) == 0)) c[i] = b, c[l] = a;
    }
}

static C2W_HD inline void d_partial(const DView& v, int tid) {
    double s = 0.0;
    for (int i = tid; i < v.T; i += v.nthr) {
        const double dd = (double)v.keys[i] - (double)v.keys[v.N + i];
        s += dd * dd;
    }
    v.dpart[tid] = s;
}

static C2W_HD inline void d_fold(const DView& v, int tid) {
    if (tid >= 16) return;
    const int n = v.nthr / 16;
    double s = 0.0;
    for (int q = tid * n; q < (tid + 1) * n; ++q) s += v.dpart[q];
    v.dpart[1024 + tid] = s;
}

static C2W_HD inline void d_store(const DView& v, int tid, int nan) {
    if (tid != 0) return;
    double s = 0.0;
    for (int q = 0; q < 16; ++q) s += v.dpart[1024 + q];
    v.out[v.block] = nan ? (double)__builtin_nanf("") : s / (double)v.T;
}

}  // namespace swd
#endif
