// Mean structural similarity of pairs of fp32 fields under a uniform WIN x WIN window: the arithmetic of ssim.hip, written as
// barrier-separated phases over "thread tid of the 256 of a workgroup".  A phase touches LDS only in ways that need no ordering inside
// the phase, so the kernel is phase, __syncthreads(), phase, ...; compiled for the host (core_side.h) the same phases run one thread
// after the other over a Thread record each, which is how the index maps below are checked without a GPU.
//
// Definition (c2w_hip.h: c2w_ssim).  For a pair x, y of H x W, NP = WIN^2, cn = NP / (NP - 1), data range R:
//   u_a = mean of a over the window, a in x, y, xx, yy, xy;  vx = cn (u_xx - u_x^2), vy likewise, vxy = cn (u_xy - u_x u_y)
//   S = (2 u_x u_y + C1)(2 vxy + C2) / ((u_x^2 + u_y^2 + C1)(vx + vy + C2)),  C1 = (0.01 R)^2, C2 = (0.03 R)^2
//   score = mean of S over the (H - WIN + 1)(W - WIN + 1) windows that lie inside the field.
// Route.  p = the mean of y (double sum, fixed order), a = x - p, b = y - p BEFORE any product: variances and the covariance are shift
// invariant, and the luminance factor is 1 - (u_a - u_b)^2 / ((p + u_a)^2 + (p + u_b)^2 + C1), so no fp32 difference of two numbers of
// the size of offset^2 is ever formed.  Window sums are direct and separable: down the columns first (WIN rows of a, b and their three
// products), then along the rows; a thread forms four neighbouring sums at once, which share the WIN - 3 terms in the middle.
//
// A workgroup owns one pair, or four when W <= 32 (slot s of 64 threads, columns 32 s .. 32 s + W - 1 of the LDS rows).  Rows stream
// through a ring of SR + WIN - 1 LDS rows of a and b; per strip of SR = 8 output rows:
//   stash    the 8 new rows, fetched from global memory one strip ahead, go into the ring slots of the 8 rows no longer needed
//   vertical thread (column c, row block rb) reads WIN + 3 rows of its column and writes 4 rows of the 5 column sums: V[row][moment][c]
//   horizontal thread (row rr, columns 4 g .. 4 g + 3) reads WIN + 3 column sums of each moment as 16-byte words, forms S for its four
//            windows and adds them to its own double
// and at the end a slot's partials are added in an order fixed by the shape alone.  A value that no window inside the field uses (a
// column past W of a narrow slot, a row past H in the last strip) may be read but only into sums that are discarded by a select, never
// scaled by zero: a NaN stays in its own pair.
#ifndef C2W_SSIM_CORE_H
#define C2W_SSIM_CORE_H

#include "core_side.h"

namespace ssim {

constexpr int THREADS = 256;
constexpr int SR = 8;         // output rows per strip
constexpr int RB = 4;         // output rows (vertical phase) and columns (horizontal phase) per thread
constexpr int LDW = 128;      // floats per ring row: the widest field, or four slots of 32
constexpr int VLD = LDW + 4;  // floats per row of column sums: the last thread of a row reads up to 3 floats past it (discarded sums)

template <int WIN>
struct Plan {
    static_assert(WIN == 7 || WIN == 11 || WIN == 15, "supported windows");
    static constexpr int RING = SR + WIN - 1;          // rows of a (and of b) in LDS
    static constexpr int NV4 = (WIN + RB - 1 + 3) / 4;  // 16-byte words of column sums behind four neighbouring windows
    static constexpr int RING_FLOATS = RING * LDW;
    static constexpr int V_FLOATS = SR * 5 * VLD;
    static constexpr int FLOATS = 2 * RING_FLOATS + V_FLOATS;  // ring of a | ring of b | V
};
constexpr int DOUBLES = THREADS + 64;  // one partial per thread | 16 second-level partials per slot

struct Shape {
    int H, W;
    int FPW;     // pairs per workgroup: 4 (W <= 32) or 1
    int SW;      // columns between two slots: 32 or W
    int TPF;     // threads per slot in the load phases: 64 or 256
    int G;       // groups of four columns in an LDS row (all slots)
    int OH, OW;  // windows inside the field
    int NS;      // strips
};

static C2W_BOTH inline Shape make_shape(int H, int W, int win) {
    Shape s;
    s.H = H, s.W = W;
    s.FPW = W <= 32 ? 4 : 1;
    s.SW = s.FPW == 4 ? 32 : W;
    s.TPF = THREADS / s.FPW;
    s.G = s.FPW * s.SW / 4;
    s.OH = H - win + 1, s.OW = W - win + 1;
    s.NS = (s.OH + SR - 1) / SR;
    return s;
}

static C2W_BOTH inline bool supported(int H, int W, int win) {
    return H % 8 == 0 && W % 8 == 0 && H >= 16 && H <= 128 && W >= 16 && W <= 128 && (win == 7 || win == 11 || win == 15);
}

// What a phase sees.  x, y, range, out: global memory (c2w_ssim); first: the pair of slot 0; the rest is the workgroup's LDS.
struct View {
    const float* x;
    const float* y;
    const float* range;
    double* out;
    long long n_pairs, n_truth, first;
    float* ringA;
    float* ringB;
    float* V;
    double* dpart;
    double* dlev;
};

// What a thread carries from phase to phase (registers in the kernel)
struct Thread {
    float lp;          // pivot of the slot this thread loads for
    float hp, c1, c2;  // pivot and constants of the slot whose windows it scores
    float4 fx, fy;     // the 16 bytes of x and y fetched for the next strip
    int has;
    double acc;        // sum of S over its windows so far
};

static C2W_HD inline double sum16(const double* d) {  // in order: every thread gets the same bits
    double s = 0.0;
    for (int j = 0; j < 16; ++j) s += d[j];
    return s;
}

// four neighbouring window sums from the shared middle `core` (terms 3 .. WIN-1), terms 0, 1, 2 and terms WIN, WIN+1, WIN+2
static C2W_HD inline void edge(float (&out)[4], float core, float l0, float l1, float l2, float r0, float r1, float r2) {
    const float t2 = core + l2, t21 = t2 + l1;
    out[0] = t21 + l0;
    out[1] = t21 + r0;
    out[2] = (t2 + r0) + r1;
    out[3] = ((core + r0) + r1) + r2;
}

// phase 0: the truth field's sum, thread partials in double in the order of the thread's own loads
static C2W_HD inline void phase_pivot_partial(const View& v, const Shape& sh, int tid) {
    const int slot = tid / sh.TPF, tl = tid % sh.TPF;
    const long long pair = v.first + slot;
    double s = 0.0;
    if (pair < v.n_pairs) {
        const float4* y = (const float4*)(v.y + (pair % v.n_truth) * (long long)(sh.H * sh.W));
        for (int i = tl; i < sh.H * sh.W / 4; i += sh.TPF) {
            const float4 q = y[i];
            s += ((double)q.x + (double)q.y) + ((double)q.z + (double)q.w);
        }
    }
    v.dpart[tid] = s;
}

// phase 1: 16 threads of a slot fold TPF / 16 partials each
static C2W_HD inline void phase_pivot_fold(const View& v, const Shape& sh, int tid) {
    const int slot = tid / sh.TPF, tl = tid % sh.TPF;
    if (tl < 16) {
        const int n = sh.TPF / 16;
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += v.dpart[slot * sh.TPF + tl * n + j];
        v.dlev[slot * 16 + tl] = s;
    }
}

// phase 2: the thread's pivots and constants, and rows 0 .. WIN-2 of a and b into the ring
template <int WIN>
static C2W_HD inline void phase_prologue(const View& v, const Shape& sh, Thread& th, int tid) {
    const int slot = tid / sh.TPF, tl = tid % sh.TPF, W4 = sh.W / 4;
    const long long pair = v.first + slot, HW = (long long)(sh.H * sh.W);
    th.acc = 0.0, th.has = 0;
    th.lp = (float)(sum16(v.dlev + slot * 16) / (double)HW);
    const int hslot = ((tid % sh.G) * 4) / sh.SW;
    const long long hpair = v.first + hslot;
    th.hp = (float)(sum16(v.dlev + hslot * 16) / (double)HW);
    const double R = hpair < v.n_pairs ? (double)v.range[hpair % v.n_truth] : 1.0;
    th.c1 = (float)((0.01 * R) * (0.01 * R)), th.c2 = (float)((0.03 * R) * (0.03 * R));
    if (pair >= v.n_pairs) return;
    const float4* x = (const float4*)(v.x + pair * HW);
    const float4* y = (const float4*)(v.y + (pair % v.n_truth) * HW);
    for (int it = tl; it < (WIN - 1) * W4; it += sh.TPF) {
        const int row = it / W4, q = it % W4, o = row * LDW + slot * sh.SW + 4 * q;
        const float4 a = x[it], b = y[it];
        *(float4*)(v.ringA + o) = float4{a.x - th.lp, a.y - th.lp, a.z - th.lp, a.w - th.lp};
        *(float4*)(v.ringB + o) = float4{b.x - th.lp, b.y - th.lp, b.z - th.lp, b.w - th.lp};
    }
}

// the 16 bytes of x and of y this thread brings in for strip s: rows s SR + WIN - 1 .. + SR - 1, as far as the field goes
template <int WIN>
static C2W_HD inline void fetch(const View& v, const Shape& sh, Thread& th, int tid, int s) {
    const int slot = tid / sh.TPF, tl = tid % sh.TPF, W4 = sh.W / 4;
    const long long pair = v.first + slot, HW = (long long)(sh.H * sh.W);
    const int ri = tl / W4, q = tl % W4, row = s * SR + WIN - 1 + ri;
    th.has = pair < v.n_pairs && ri < SR && row < sh.H;
    if (th.has) {
        th.fx = ((const float4*)(v.x + pair * HW))[row * W4 + q];
        th.fy = ((const float4*)(v.y + (pair % v.n_truth) * HW))[row * W4 + q];
    }
}

// phase 3 (per strip): what fetch brought, pivoted, into the ring slots of the rows the last strip was the last to use
template <int WIN>
static C2W_HD inline void phase_stash(const View& v, const Shape& sh, const Thread& th, int tid, int s) {
    if (!th.has) return;
    const int slot = tid / sh.TPF, tl = tid % sh.TPF, W4 = sh.W / 4;
    const int ri = tl / W4, q = tl % W4, row = s * SR + WIN - 1 + ri;
    const int o = (row % Plan<WIN>::RING) * LDW + slot * sh.SW + 4 * q;
    *(float4*)(v.ringA + o) = float4{th.fx.x - th.lp, th.fx.y - th.lp, th.fx.z - th.lp, th.fx.w - th.lp};
    *(float4*)(v.ringB + o) = float4{th.fy.x - th.lp, th.fy.y - th.lp, th.fy.z - th.lp, th.fy.w - th.lp};
}

// phase 4 (per strip): column sums of a, b, aa, bb, ab over WIN rows, for 4 output rows of one column
template <int WIN>
static C2W_HD inline void phase_vertical(const View& v, const Shape& sh, int tid, int s) {
    constexpr int RING = Plan<WIN>::RING, N = WIN + RB - 1;
    const int WT = sh.FPW * sh.SW, c = tid % WT, rb = tid / WT;
    if (rb >= SR / RB || c % sh.SW >= sh.W) return;
    float a[N], b[N];
    int rr = (s * SR + rb * RB) % RING;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        a[k] = v.ringA[rr * LDW + c], b[k] = v.ringB[rr * LDW + c];
        rr = rr + 1 == RING ? 0 : rr + 1;
    }
    float ca = a[3], cb = b[3], caa = a[3] * a[3], cbb = b[3] * b[3], cab = a[3] * b[3];
#pragma unroll
    for (int k = 4; k < WIN; ++k) {
        ca += a[k], cb += b[k];
        caa = fmaf(a[k], a[k], caa), cbb = fmaf(b[k], b[k], cbb), cab = fmaf(a[k], b[k], cab);
    }
    float m[5][4];
    edge(m[0], ca, a[0], a[1], a[2], a[WIN], a[WIN + 1], a[WIN + 2]);
    edge(m[1], cb, b[0], b[1], b[2], b[WIN], b[WIN + 1], b[WIN + 2]);
    edge(m[2], caa, a[0] * a[0], a[1] * a[1], a[2] * a[2], a[WIN] * a[WIN], a[WIN + 1] * a[WIN + 1], a[WIN + 2] * a[WIN + 2]);
    edge(m[3], cbb, b[0] * b[0], b[1] * b[1], b[2] * b[2], b[WIN] * b[WIN], b[WIN + 1] * b[WIN + 1], b[WIN + 2] * b[WIN + 2]);
    edge(m[4], cab, a[0] * b[0], a[1] * b[1], a[2] * b[2], a[WIN] * b[WIN], a[WIN + 1] * b[WIN + 1], a[WIN + 2] * b[WIN + 2]);
#pragma unroll
    for (int j = 0; j < RB; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) v.V[((rb * RB + j) * 5 + q) * VLD + c] = m[q][j];
}

// S of one window from its five sums over NP = WIN^2 pivoted values
template <int WIN>
static C2W_HD inline float window_score(float sa, float sb, float saa, float sbb, float sab, float p, float c1, float c2) {
    constexpr float inv = 1.0f / (float)(WIN * WIN), cn = (float)(WIN * WIN) / (float)(WIN * WIN - 1);
    const float ua = sa * inv, ub = sb * inv;
    const float va = cn * fmaf(-ua, ua, saa * inv), vb = cn * fmaf(-ub, ub, sbb * inv), vab = cn * fmaf(-ua, ub, sab * inv);
    const float ux = p + ua, uy = p + ub, d = ua - ub;
    const float lum = 1.0f - d * d / fmaf(ux, ux, fmaf(uy, uy, c1));
    return lum * ((2.0f * vab + c2) / (va + vb + c2));
}

// phase 5 (per strip): the row sums of the column sums, S, and the thread's running double
template <int WIN>
static C2W_HD inline void phase_horizontal(const View& v, const Shape& sh, Thread& th, int tid, int s) {
    constexpr int NV4 = Plan<WIN>::NV4;
    if (tid >= SR * sh.G) return;
    const int rr = tid / sh.G, col = (tid % sh.G) * 4, lc = col % sh.SW;
    if (s * SR + rr >= sh.OH || lc >= sh.OW) return;
    float sums[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const float4* p = (const float4*)(v.V + (rr * 5 + q) * VLD + col);
        float w[4 * NV4];
#pragma unroll
        for (int k = 0; k < NV4; ++k) {
            const float4 t = p[k];
            w[4 * k] = t.x, w[4 * k + 1] = t.y, w[4 * k + 2] = t.z, w[4 * k + 3] = t.w;
        }
        float core = w[3];
#pragma unroll
        for (int k = 4; k < WIN; ++k) core += w[k];
        edge(sums[q], core, w[0], w[1], w[2], w[WIN], w[WIN + 1], w[WIN + 2]);
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const float S = window_score<WIN>(sums[0][j], sums[1][j], sums[2][j], sums[3][j], sums[4][j], th.hp, th.c1, th.c2);
        if (lc + j < sh.OW) th.acc += (double)S;
    }
}

// phase 6: every thread's sum
static C2W_HD inline void phase_partial(const View& v, const Thread& th, int tid) {
    v.dpart[tid] = th.acc;
}

// phase 7: 16 threads per slot fold the slot's partials, in the order (row of the strip, group of four columns)
static C2W_HD inline void phase_fold(const View& v, const Shape& sh, int tid) {
    if (tid >= sh.FPW * 16) return;
    const int slot = tid / 16, j = tid % 16, n = sh.TPF / 16;
    double s = 0.0;
    for (int k = j * n; k < (j + 1) * n; ++k) s += v.dpart[sh.FPW == 1 ? k : (k / 8) * 32 + slot * 8 + k % 8];
    v.dlev[tid] = s;
}

// phase 8: the mean over the windows, one double per live pair
static C2W_HD inline void phase_store(const View& v, const Shape& sh, int tid) {
    if (tid >= sh.FPW || v.first + tid >= v.n_pairs) return;
    v.out[v.first + tid] = sum16(v.dlev + tid * 16) / ((double)sh.OH * (double)sh.OW);
}

}  // namespace ssim
#endif
