// Wind power of an ensemble: the table, the interval lookup, the cell arithmetic, the chunk plan and the fold of wind.hip, written as
// barrier-separated phases over "thread tid of a workgroup", as crps_core.h is.  Compiled for the host (core_side.h) the same phases
// run one thread after the other: tests/host_wind_main.cpp checks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_wind_power).  One cell of one (d, t) plane has the fp32 wind components u, v in m/s; with the hub factor
// c = (hub_height / reference_height)^alpha, formed in float64 by the caller and rounded once,
//   speed = sqrt(u u + v v) c                                   (not hypot: u u may overflow, as the reference's does)
//   power = numpy.interp(speed, xs, ps, left = 0, right = 0)    K >= 2 knots, xs strictly increasing:
//           ps[j] + (speed - xs[j]) slope_j for xs[j] <= speed < xs[j + 1]; ps[K - 1] at speed == xs[K - 1]; 0 above it (cut-out)
//           and below xs[0]; NaN for a NaN speed; 0 for +inf
// and sums[d][t] = {sum of speed, sum of power} over the hw cells of the plane, in double.  A NaN u or v makes the two values of its
// cell, and with them the two sums of its plane, NaN; nothing else.
//
// The table (build_table, host side of c2w_wind_table): a Header, the K - 1 intervals packed as {x_j, p_j, slope_j, x_{j + 1}} -- one
// 16-byte LDS read serves the interpolation and the test that ends the scan -- and BUCKETS starting knots.  The knots are rounded to
// fp32 first and must still increase strictly; slope_j = (p_{j + 1} - p_j) / (x^_{j + 1} - x^_j) is formed in float64 FROM THE ROUNDED
// KNOTS and rounded once, so the table is the piecewise-linear curve through (x^_j, p_j): its value at s is the float64 curve's value
// at a point no further from s than the rounding of a knot (tests/fp64_wind_ref.py leans on this).
//
// The lookup.  bucket_of(s) = min(int((s - x^_0) inv), BUCKETS - 1) with inv = fp32(BUCKETS / (x^_{K - 1} - x^_0)) is monotone in s
// whatever its roundings, so start[b] = the last knot whose bucket is below b (0 if none) is never beyond the interval of an s in
// bucket b, and that interval is at most (knots in bucket b) further: where no bucket holds more than SCAN = 2 knots the lookup is one
// 2-byte read, one 16-byte read and SCAN more, none behind a branch (MODE_BUCKETS).  A curve whose knots crowd a bucket, or whose span
// is too small for inv, takes a binary search over the intervals instead (MODE_BISECT): ceil(log2(K - 1)) dependent reads.
//
// wind_power: a workgroup of 256 owns one plane, or one chunk of CHUNK cells of it (a function of hw alone).  A thread owns 4 adjacent
// cells in each of its ROUNDS rounds and asks for all its 16-byte loads of u and of v before it uses one.  No multiply is fused with an
// add (the host run and the NumPy restatement give the same bits); the square root is the correctly rounded one.  The fp32 values of a
// cell join the thread's two double accumulators in cell order; the workgroup folds them by the fixed-order sum of ordered_sum.h
// (N = 2, nan_if_nan) and writes two doubles: to sums if the plane is one chunk, to partial[plane][chunk][2] otherwise, which the
// shared fold kernel adds in chunk order.  No atomics: a plane's bits are fixed by hw and the table.
#ifndef C2W_WIND_CORE_H
#define C2W_WIND_CORE_H

#include "core_side.h"

#if defined(__clang__)
#define WIND_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define WIND_NO_CONTRACT
#endif
#include "ordered_sum.h"

namespace wind {

constexpr int THREADS = 256;
constexpr int MAX_K = 256;
constexpr int BUCKETS = 256;
constexpr int SCAN = 2;                 // knots a bucket may hold while the bounded scan serves the curve
constexpr int ROUNDS = 4;               // rounds of 256 threads x 4 cells a workgroup makes over its chunk
constexpr int CHUNK = ROUNDS * THREADS * 4;  // 4096 cells
constexpr int LDS_DOUBLES = ordered_sum::lds_doubles<2>();
constexpr int MODE_BUCKETS = 0, MODE_BISECT = 1;
static_assert(THREADS == ordered_sum::THREADS, "the workgroup the fixed-order sum is written for");

struct alignas(16) Pack {
    float v[4];
};

struct alignas(16) Header {  // 32 bytes
    float x0, xl, pl, inv;   // first knot, last knot, power at the last knot, buckets per m/s
    int K, mode, pad0, pad1;
};
struct alignas(16) Entry {   // interval j
    float x, p, m, xn;       // x^_j, p_j, slope_j, x^_{j + 1}
};
static_assert(sizeof(Header) == 32 && sizeof(Entry) == 16, "the packed table");

constexpr int MAX_TABLE_BYTES = 32 + 16 * (MAX_K - 1) + 2 * BUCKETS;  // 4624

static C2W_BOTH inline bool supported(int hw, int K) { return hw >= 4 && hw % 4 == 0 && K >= 2 && K <= MAX_K; }
static C2W_BOTH inline int table_bytes(int K) { return 32 + 16 * (K - 1) + 2 * BUCKETS; }

struct Table {  // pointers into one packed table
    const Header* h;
    const Entry* e;
    const unsigned short* start;
    int K;
};
static C2W_BOTH inline Table view_table(const void* bytes, int K) {
    Table t;
    t.h = (const Header*)bytes, t.e = (const Entry*)((const char*)bytes + 32), t.start = (const unsigned short*)((const char*)bytes + 32 + 16 * (K - 1));
    t.K = K;
    return t;
}

// ---------------------------------------------------------------------------------------------------------------- lookup, arithmetic

// s in [x0, xl): monotone in s; (s - x0) inv < BUCKETS (1 + 2^-22), so the conversion is in range
static C2W_BOTH inline int bucket_of(float s, float x0, float inv) {
    WIND_NO_CONTRACT
    const float d = s - x0;
    const int b = (int)(d * inv);
    return b > BUCKETS - 1 ? BUCKETS - 1 : b;
}

struct Curve {  // the header's values in registers
    float x0, xl, pl, inv;
    int mode;
};
static C2W_BOTH inline Curve curve_of(const Table& t) {
    Curve c;
    c.x0 = t.h->x0, c.xl = t.h->xl, c.pl = t.h->pl, c.inv = t.h->inv, c.mode = t.h->mode;
    return c;
}

// The powers of four speeds.  Written without a branch that depends on a speed, the four cells side by side: their LDS reads are in
// flight together, and a lane outside the curve (below the first knot, at or above the last, NaN) looks up the first knot instead and
// has its value replaced at the end.  The interval of s, x^_0 <= s < x^_{K - 1}, is the largest j <= K - 2 with x^_j <= s.
static C2W_BOTH inline void powers_of(const Table& t, const Curve& c, const float (&s)[4], float (&p)[4]) {
    WIND_NO_CONTRACT
    const int last = t.K - 2;
    float in[4];
    int j[4];
    Entry e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = s[k] >= c.x0 && s[k] < c.xl ? s[k] : c.x0;
    if (c.mode == MODE_BUCKETS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            j[k] = t.start[bucket_of(in[k], c.x0, c.inv)];
            j[k] = j[k] > last ? last : j[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = t.e[j[k]];
#pragma unroll
        for (int i = 0; i < SCAN; ++i) {
#pragma unroll
            for (int k = 0; k < 4; ++k) j[k] += j[k] < last && in[k] >= e[k].xn ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = t.e[j[k]];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int lo = 0, hi = last;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (t.e[mid].x <= in[k]) lo = mid;
                else hi = mid - 1;
            }
            e[k] = t.e[lo];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = in[k] - e[k].x;
        const float r = d * e[k].m;
        const float val = e[k].p + r;
        const float out = s[k] == c.xl ? c.pl : 0.f;  // at the last knot; below the first, above the last (+inf too): nothing
        p[k] = s[k] != s[k] ? s[k] : (s[k] >= c.x0 && s[k] < c.xl ? val : out);
    }
}

static C2W_BOTH inline float speed_of(float u, float v, float hub) {
    WIND_NO_CONTRACT
    const float uu = u * u, vv = v * v;
    const float q = uu + vv;
    const float r = __builtin_sqrtf(q);
    return r * hub;
}

// ---------------------------------------------------------------------------------------------------------------- the table builder

// 0, or -1 for K out of range, a knot or a power that is not finite as fp32, or fp32 knots that do not increase strictly
static inline int build_table(const double* xs, const double* ps, int K, void* bytes) {
    if (K < 2 || K > MAX_K || !xs || !ps || !bytes) return -1;
    float xf[MAX_K], pf[MAX_K];
    for (int j = 0; j < K; ++j) {
        if (!(__builtin_fabs(xs[j]) <= (double)__FLT_MAX__) || !(__builtin_fabs(ps[j]) <= (double)__FLT_MAX__)) return -1;  // NaN too
        xf[j] = (float)xs[j], pf[j] = (float)ps[j];
        if (j > 0 && !(xs[j] > xs[j - 1] && xf[j] > xf[j - 1])) return -1;
    }
    Header* h = (Header*)bytes;
    Entry* e = (Entry*)((char*)bytes + 32);
    unsigned short* start = (unsigned short*)((char*)bytes + 32 + 16 * (K - 1));
    for (int j = 0; j + 1 < K; ++j) {
        const double slope = ((double)pf[j + 1] - (double)pf[j]) / ((double)xf[j + 1] - (double)xf[j]);
        if (!(__builtin_fabs(slope) <= (double)__FLT_MAX__)) return -1;
        e[j].x = xf[j], e[j].p = pf[j], e[j].m = (float)slope, e[j].xn = xf[j + 1];
    }
    const double wide = (double)BUCKETS / ((double)xf[K - 1] - (double)xf[0]);
    const float inv = wide <= (double)__FLT_MAX__ ? (float)wide : 0.f;  // a span too small for it: no buckets
    h->x0 = xf[0], h->xl = xf[K - 1], h->pl = pf[K - 1], h->inv = inv, h->K = K, h->pad0 = h->pad1 = 0;
    int mode = wide <= (double)__FLT_MAX__ ? MODE_BUCKETS : MODE_BISECT;
    for (int b = 0; b < BUCKETS; ++b) start[b] = 0;
    if (mode == MODE_BUCKETS) {
        int count[BUCKETS];
        for (int b = 0; b < BUCKETS; ++b) count[b] = 0;
        for (int j = 0; j + 1 < K; ++j) {  // the last knot is no interval's start
            const int b = bucket_of(xf[j], xf[0], inv);
            if (++count[b] > SCAN) mode = MODE_BISECT;
            for (int a = b + 1; a < BUCKETS; ++a) start[a] = (unsigned short)j;  // the last knot whose bucket is below a
        }
    }
    h->mode = mode;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- maps

static C2W_BOTH inline int chunks(int hw) { return (hw + CHUNK - 1) / CHUNK; }
static C2W_BOTH inline int chunk_end(int hw, int c) { return (c + 1) * CHUNK < hw ? (c + 1) * CHUNK : hw; }
// the first of the 4 cells thread tid owns in round `it` of chunk c
static C2W_BOTH inline int cell_of(int c, int it, int tid) { return c * CHUNK + (it * THREADS + tid) * 4; }
// bytes of partial sums: none while a plane is one chunk
static C2W_BOTH inline long long scratch_bytes(long long planes, int hw) {
    return chunks(hw) > 1 ? planes * chunks(hw) * 2 * (long long)sizeof(double) : 0;
}

// ---------------------------------------------------------------------------------------------------------------- phases

struct View {
    const float* fields;  // [planes][F][hw]
    double* out;          // sums [planes][2] (one chunk a plane) or partial [planes][chunks][2]
    float* derived;       // [planes][2][hw] or null
    long long plane;      // d T + t
    int chunk;
    int F, u_index, v_index, hw;
    float hub;
    Table table;          // in LDS on the device
    double* lds;          // LDS_DOUBLES
};

struct Thread {
    Pack u[ROUNDS], v[ROUNDS];
    double acc[2];
    int has[ROUNDS];
};

// all the thread's loads of the chunk, 16 bytes each, none used before all are asked for
static C2W_HD inline void t_fetch(const View& w, Thread& th, int tid) {
    const float* pu = w.fields + (w.plane * w.F + w.u_index) * w.hw;
    const float* pv = w.fields + (w.plane * w.F + w.v_index) * w.hw;
    const int end = chunk_end(w.hw, w.chunk);
#pragma unroll
    for (int it = 0; it < ROUNDS; ++it) {
        const int cell = cell_of(w.chunk, it, tid);
        th.has[it] = cell < end;
        if (th.has[it]) th.u[it] = *(const Pack*)(pu + cell), th.v[it] = *(const Pack*)(pv + cell);
    }
    th.acc[0] = th.acc[1] = 0.0;
}

static C2W_HD inline void t_cells(const View& w, Thread& th, int tid) {
    const Curve c = curve_of(w.table);
#pragma unroll
    for (int it = 0; it < ROUNDS; ++it) {
        if (!th.has[it]) continue;
        Pack s, p;
#pragma unroll
        for (int k = 0; k < 4; ++k) s.v[k] = speed_of(th.u[it].v[k], th.v[it].v[k], w.hub);
        powers_of(w.table, c, s.v, p.v);
#pragma unroll
        for (int k = 0; k < 4; ++k) th.acc[0] += (double)s.v[k], th.acc[1] += (double)p.v[k];
        if (w.derived) {
            float* d = w.derived + w.plane * 2 * w.hw + cell_of(w.chunk, it, tid);
            *(Pack*)d = s, *(Pack*)(d + w.hw) = p;
        }
    }
}

// the three phases of ordered_sum.h at N = 2: thread s writes the workgroup's entry of sum s, an infinite sum stays; f_fold then
// writes sums[entry], entry = plane 2 + s, from the chunks in index order
static C2W_HD inline void t_stash(const View& w, const Thread& th, int tid) { ordered_sum::stash<2>(w.lds, th.acc, tid); }
static C2W_HD inline void t_fold_groups(const View& w, int tid) { ordered_sum::fold_groups<2>(w.lds, tid); }
static C2W_HD inline void t_fold_store(const View& w, int tid) {
    if (tid >= 2) return;
    const double t = ordered_sum::fold_total<2>(w.lds, tid);
    w.out[(w.plane * chunks(w.hw) + w.chunk) * 2 + tid] = ordered_sum::nan_if_nan(t);
}
static C2W_HD inline void f_fold(const double* partial, double* sums, long long entry, int nc) {
    sums[entry] = ordered_sum::nan_if_nan(ordered_sum::fold_parts(partial, entry, nc, 2));
}

}  // namespace wind
#endif
