// Radially averaged power spectrum of one square real field, N in {8, 16, 32, 64, 128}: the arithmetic of spectrum.hip, written as
// nine barrier-separated phases over "thread tl of the TPF that share a field".  A phase touches the field's LDS image only in ways
// that need no ordering inside the phase, so the kernel is phase, __syncthreads(), phase, ...; compiled for the host (core_side.h)
// the same phases run one thread after the other, which is how the index maps below are checked without a GPU.
//
// Definition (a restatement of the radial spectrum the reference takes from its radar library, from memory -- see c2w_hip.h):
//   P[u][v] = |sum_ij x[i][j] exp(-2 pi i (u i + v j) / N)|^2 / N^2,  ku, kv the centred integer wavenumbers of u, v (-N/2 .. N/2-1),
//   r = round(sqrt(ku^2 + kv^2)) (k^2 - k < ku^2 + kv^2 <= k^2 + k  <=>  r = k: no ties),  S[k] = mean of P over the cells with r = k,
//   k = 0 .. N/2 - 1.  x real => P[u][v] = P[-u][-v]: the half plane kv = 0 .. N/2-1 with kv >= 1 weighted twice; every cell with
//   kv = N/2 or ku = -N/2 has r >= N/2 and is dropped, so the Nyquist column and row are never formed.
//
// The image: N rows of LD = N + 4 floats (the pad makes rows 2p, 2p+2, ... start 8 banks apart).
//   rows:    rows 2p and 2p+1 are packed into ONE complex transform z = a + i b, real parts kept in row 2p, imaginary parts in row 2p+1.
//            N = N1 * N2: pass A does N2 transforms of N1 points (stride N2) in registers and applies W_N^(n2 k1); pass B does N1
//            transforms of N2 contiguous points.  Both write where they read, so Z[k1 + N1 k2] ends up in slot pos(k) = k1 N2 + k2.
//   untangle: A[k] = Z[k] + conj Z[N-k], B[k] = (Z[k] - conj Z[N-k]) / i  (twice the transforms of rows 2p, 2p+1; the 1/4 goes into
//            the power's scale) for k < N/2, written over the four floats they were read from:
//            H[2p][k] = (img[2p][pos k], img[2p+1][pos k]),  H[2p+1][k] = (img[2p][pos(N-k)], img[2p+1][pos(N-k)])  (k = 0: pos(N/2)).
//   columns: the same two passes over the row index of H[.][c], in place; the power lands in the real slot of row-slot pos(u).
//   bins:    thread (k, q) walks rows u = q, q + NQ, ...; in a row the cells of bin k are one run of kv, found with the integer rule.
// Every sum has one order fixed by N; nothing here depends on where the field lies in the batch.
#ifndef C2W_SPECTRUM_CORE_H
#define C2W_SPECTRUM_CORE_H

#include "core_side.h"
#ifdef C2W_CORE_HOST
#define SPEC_TABLE static const
#else
#define SPEC_TABLE static __device__ const
#endif

namespace spectrum {

struct Cplx { float re, im; };

// exp(-2 pi i j / 128), j = 0 .. 31, rounded from double; the other three quarters are these times (-i)^q
SPEC_TABLE float QUARTER_TWIDDLE[32][2] = {
        {1.0f, 0.0f}, {0.99879545f, -0.0490676761f}, {0.99518472f, -0.0980171412f}, {0.989176512f, -0.146730468f},
        {0.980785251f, -0.195090324f}, {0.970031261f, -0.242980182f}, {0.956940353f, -0.290284663f}, {0.941544056f, -0.336889863f},
        {0.923879504f, -0.382683426f}, {0.903989315f, -0.427555084f}, {0.881921291f, -0.471396744f}, {0.857728601f, -0.514102757f},
        {0.831469595f, -0.555570245f}, {0.803207517f, -0.59569931f}, {0.773010433f, -0.634393275f}, {0.740951121f, -0.671558976f},
        {0.707106769f, -0.707106769f}, {0.671558976f, -0.740951121f}, {0.634393275f, -0.773010433f}, {0.59569931f, -0.803207517f},
        {0.555570245f, -0.831469595f}, {0.514102757f, -0.857728601f}, {0.471396744f, -0.881921291f}, {0.427555084f, -0.903989315f},
        {0.382683426f, -0.923879504f}, {0.336889863f, -0.941544056f}, {0.290284663f, -0.956940353f}, {0.242980182f, -0.970031261f},
        {0.195090324f, -0.980785251f}, {0.146730468f, -0.989176512f}, {0.0980171412f, -0.99518472f}, {0.0490676761f, -0.99879545f}};

static C2W_HD inline Cplx twiddle128(int j) {  // exp(-2 pi i j / 128), j = 0 .. 127
    const Cplx w{QUARTER_TWIDDLE[j & 31][0], QUARTER_TWIDDLE[j & 31][1]};
    switch (j >> 5) {
        case 0: return w;
        case 1: return Cplx{w.im, -w.re};
        case 2: return Cplx{-w.re, -w.im};
        default: return Cplx{-w.im, w.re};
    }
}

template <int N>
struct Plan {
    static_assert(N == 8 || N == 16 || N == 32 || N == 64 || N == 128, "supported sizes");
    static constexpr int N1 = N == 128 ? 16 : N >= 32 ? 8 : 4;  // register transform of pass A
    static constexpr int N2 = N / N1;                           // register transform of pass B (8, 8, 4, 4, 2)
    static constexpr int LD = N + 4;
    static constexpr int TPF = N >= 64 ? 256 : 2 * N;           // threads per field (16, 32, 64, 256, 256)
    static constexpr int FPW = 256 / TPF;                       // fields per workgroup (16, 8, 4, 1, 1)
    static constexpr int R = N / 2;                             // bins, kept columns, packed row pairs
    static constexpr int NQ = TPF / R;                          // row classes of the bin walk (4, 4, 4, 8, 4)
    static constexpr int IMG = N * LD;                          // floats of one field's image
    // a workgroup's LDS: FPW images | N twiddles | per field: TPF doubles (load partials, later bin partials), 16 doubles, TPF ints
    static constexpr int AUX_D = TPF + 16;                      // doubles per field
    static constexpr size_t lds_bytes() { return sizeof(float) * ((size_t)FPW * IMG + 2 * N) + (size_t)FPW * (sizeof(double) * AUX_D + sizeof(int) * TPF); }
    static C2W_HD constexpr int pos(int k) { return (k % N1) * N2 + k / N1; }
    static C2W_HD constexpr int mirror(int c) { return c ? N - c : N / 2; }
};

// exp(-2 pi i j / 16), j = 0 .. 7: the register transforms' own factors (j = 0 and j = 4 are handled without a multiply)
#define SPEC_C1 0.923879504f
#define SPEC_C2 0.707106769f
#define SPEC_C3 0.382683426f

// Radix-2 decimation-in-time transform of R = 2, 4, 8 or 16 points held in registers (every index below is a compile-time constant
// once the loops are unrolled).
template <int R>
static C2W_HD inline void fft_reg(float (&re)[R], float (&im)[R]) {
    constexpr float WR[8] = {1.0f, SPEC_C1, SPEC_C2, SPEC_C3, 0.0f, -SPEC_C3, -SPEC_C2, -SPEC_C1};
    constexpr float WI[8] = {0.0f, -SPEC_C3, -SPEC_C2, -SPEC_C1, -1.0f, -SPEC_C1, -SPEC_C2, -SPEC_C3};
    constexpr int LOG = R == 16 ? 4 : R == 8 ? 3 : R == 4 ? 2 : 1;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        int j = 0;
#pragma unroll
        for (int b = 0; b < LOG; ++b) j |= ((i >> b) & 1) << (LOG - 1 - b);
        if (i < j) {
            const float tr = re[i], ti = im[i];
            re[i] = re[j], im[i] = im[j];
            re[j] = tr, im[j] = ti;
        }
    }
#pragma unroll
    for (int len = 2; len <= R; len <<= 1) {
        const int half = len >> 1, step = 16 / len;
#pragma unroll
        for (int i = 0; i < R; i += len) {
#pragma unroll
            for (int k = 0; k < half; ++k) {
                const int a = i + k, b = i + k + half, t = k * step;
                float vr, vi;
                if (t == 0) vr = re[b], vi = im[b];
                else if (t == 4) vr = im[b], vi = -re[b];
                else vr = re[b] * WR[t] - im[b] * WI[t], vi = re[b] * WI[t] + im[b] * WR[t];
                const float ur = re[a], ui = im[a];
                re[a] = ur + vr, im[a] = ui + vi;
                re[b] = ur - vr, im[b] = ui - vi;
            }
        }
    }
}

static C2W_HD inline int isqrt_small(int v) {  // floor(sqrt(v)), 0 <= v < 2^15
    int s = (int)sqrtf((float)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

// What a phase sees of one field.  x: the field in global memory; img, dpart, dlev, cnt: its LDS; tw: the workgroup's N twiddles
// exp(-2 pi i j / N); spec: the field's N/2 outputs.
struct FieldView {
    const float* x;
    float* spec;
    float* img;
    const Cplx* tw;
    double* dpart;
    double* dlev;
    int* cnt;
};

template <int N>
static C2W_HD inline double field_sum(const FieldView& v) {  // the 16 second-level partials, in order: every thread gets the same bits
    double s = 0.0;
    for (int j = 0; j < 16; ++j) s += v.dlev[j];
    return s;
}

// phase 0: one coalesced read of the field, 16 bytes a lane; thread partial sums in double, in the order of the thread's own loads
template <int N>
static C2W_HD inline void phase_load(const FieldView& v, int tl) {
    using P = Plan<N>;
    double s = 0.0;
    for (int i = tl; i < N * N / 4; i += P::TPF) {
        const float4 q = ((const float4*)v.x)[i];
        const int row = (4 * i) / N, col = (4 * i) % N;
        *(float4*)(v.img + row * P::LD + col) = q;
        s += ((double)q.x + (double)q.y) + ((double)q.z + (double)q.w);
    }
    v.dpart[tl] = s;
}

// phase 1: 16 threads fold TPF / 16 partials each
template <int N>
static C2W_HD inline void phase_fold(const FieldView& v, int tl) {
    using P = Plan<N>;
    if (tl < 16) {
        double s = 0.0;
        for (int j = 0; j < P::TPF / 16; ++j) s += v.dpart[tl * (P::TPF / 16) + j];
        v.dlev[tl] = s;
    }
}

// The two passes of an N-point transform over a strided line of the image.  `re0`/`im0`: the floats of element 0; element e of the
// line is at re0[off(e)] -- rows: off(e) = e, columns: see col_off.
// phase 2: rows, pass A (with the mean taken off as the values are read)
template <int N>
static C2W_HD inline void phase_rows_a(const FieldView& v, int tl) {
    using P = Plan<N>;
    const float mean = (float)(field_sum<N>(v) / (double)(N * N));
    for (int it = tl; it < P::R * P::N2; it += P::TPF) {
        const int n2 = it % P::N2, p = it / P::N2;
        float* const a = v.img + 2 * p * P::LD + n2;
        float re[P::N1], im[P::N1];
#pragma unroll
        for (int n1 = 0; n1 < P::N1; ++n1) re[n1] = a[P::N2 * n1] - mean, im[n1] = a[P::LD + P::N2 * n1] - mean;
        fft_reg<P::N1>(re, im);
#pragma unroll
        for (int k1 = 0; k1 < P::N1; ++k1) {
            const Cplx w = v.tw[n2 * k1];
            a[P::N2 * k1] = re[k1] * w.re - im[k1] * w.im;
            a[P::LD + P::N2 * k1] = re[k1] * w.im + im[k1] * w.re;
        }
    }
}

// phase 3: rows, pass B
template <int N>
static C2W_HD inline void phase_rows_b(const FieldView& v, int tl) {
    using P = Plan<N>;
    for (int it = tl; it < P::R * P::N1; it += P::TPF) {
        const int k1 = it % P::N1, p = it / P::N1;
        float* const a = v.img + 2 * p * P::LD + k1 * P::N2;
        float re[P::N2], im[P::N2];
#pragma unroll
        for (int n2 = 0; n2 < P::N2; ++n2) re[n2] = a[n2], im[n2] = a[P::LD + n2];
        fft_reg<P::N2>(re, im);
#pragma unroll
        for (int k2 = 0; k2 < P::N2; ++k2) a[k2] = re[k2], a[P::LD + k2] = im[k2];
    }
}

// phase 4: untangle the packed pair, in place on the four floats of slots pos(k) and pos(N - k)
template <int N>
static C2W_HD inline void phase_untangle(const FieldView& v, int tl) {
    using P = Plan<N>;
    for (int it = tl; it < P::R * P::R; it += P::TPF) {
        const int k = it % P::R, p = it / P::R;
        float* const a = v.img + 2 * p * P::LD;
        const int sk = P::pos(k), sm = P::pos(P::mirror(k));
        const float zr = a[sk], zi = a[P::LD + sk];
        if (k == 0) {
            a[sk] = 2.f * zr, a[P::LD + sk] = 0.f;
            a[sm] = 2.f * zi, a[P::LD + sm] = 0.f;
        } else {
            const float mr = a[sm], mi = a[P::LD + sm];
            a[sk] = zr + mr, a[P::LD + sk] = zi - mi;
            a[sm] = zi + mi, a[P::LD + sm] = mr - zr;
        }
    }
}

// H[r][c]'s real float (the imaginary one is LD further): even rows keep column c in slot pos(c), odd rows in slot pos(N - c)
template <int N>
static C2W_HD inline int cell(int r, int se, int so) {
    return (r & ~1) * Plan<N>::LD + ((r & 1) ? so : se);
}

// lane j of a column pass -> column c, ordered so that the even-row slots pos(c) of consecutive lanes are consecutive floats
template <int N>
static C2W_HD inline int lane_column(int j) {
    using P = Plan<N>;
    return (j % (P::N2 / 2)) * P::N1 + j / (P::N2 / 2);
}

// phase 5: columns, pass A
template <int N>
static C2W_HD inline void phase_cols_a(const FieldView& v, int tl) {
    using P = Plan<N>;
    for (int it = tl; it < P::R * P::N2; it += P::TPF) {
        const int c = lane_column<N>(it % P::R), n2 = it / P::R;
        const int se = P::pos(c), so = P::pos(P::mirror(c));
        float re[P::N1], im[P::N1];
#pragma unroll
        for (int n1 = 0; n1 < P::N1; ++n1) {
            const float* a = v.img + cell<N>(P::N2 * n1 + n2, se, so);
            re[n1] = a[0], im[n1] = a[P::LD];
        }
        fft_reg<P::N1>(re, im);
#pragma unroll
        for (int k1 = 0; k1 < P::N1; ++k1) {
            const Cplx w = v.tw[n2 * k1];
            float* a = v.img + cell<N>(P::N2 * k1 + n2, se, so);
            a[0] = re[k1] * w.re - im[k1] * w.im;
            a[P::LD] = re[k1] * w.im + im[k1] * w.re;
        }
    }
}

// phase 6: columns, pass B, and the power |.|^2 (unscaled) into the real float of row-slot k1 N2 + k2 = pos(u), u = k1 + N1 k2
template <int N>
static C2W_HD inline void phase_cols_b(const FieldView& v, int tl) {
    using P = Plan<N>;
    for (int it = tl; it < P::R * P::N1; it += P::TPF) {
        const int c = lane_column<N>(it % P::R), k1 = it / P::R;
        const int se = P::pos(c), so = P::pos(P::mirror(c));
        float re[P::N2], im[P::N2];
#pragma unroll
        for (int n2 = 0; n2 < P::N2; ++n2) {
            const float* a = v.img + cell<N>(k1 * P::N2 + n2, se, so);
            re[n2] = a[0], im[n2] = a[P::LD];
        }
        fft_reg<P::N2>(re, im);
#pragma unroll
        for (int k2 = 0; k2 < P::N2; ++k2) v.img[cell<N>(k1 * P::N2 + k2, se, so)] = re[k2] * re[k2] + im[k2] * im[k2];
    }
}

// phase 7: thread (k, q) sums bin k's cells of rows u = q, q + NQ, ... in double (kv = 0 once, kv >= 1 twice) and counts them
template <int N>
static C2W_HD inline void phase_bins(const FieldView& v, int tl) {
    using P = Plan<N>;
    const int k = tl % P::R, q = tl / P::R;
    double acc = 0.0;
    int n = 0;
    for (int u = q; u < N; u += P::NQ) {
        if (u == N / 2) continue;  // ku = -N/2: every cell has r >= N/2
        const int ku = u < N / 2 ? u : u - N;
        const int lo2 = k * k - k - ku * ku, hi2 = k * k + k - ku * ku;  // lo2 < kv^2 <= hi2
        if (hi2 < 0) continue;
        const int lo = lo2 < 0 ? 0 : isqrt_small(lo2) + 1;
        int hi = isqrt_small(hi2);
        if (hi > N / 2 - 1) hi = N / 2 - 1;
        const int rr = P::pos(u);
        for (int kv = lo; kv <= hi; ++kv) {
            const float p = v.img[cell<N>(rr, P::pos(kv), P::pos(P::mirror(kv)))];
            acc += kv ? 2.0 * (double)p : (double)p;
            n += kv ? 2 : 1;
        }
    }
    v.dpart[k * P::NQ + q] = acc;
    v.cnt[k * P::NQ + q] = n;
}

// phase 8: the NQ partials in order, the scale 1 / (4 N^2) (the untangle kept its factor 2), bin 0 from the field's own sum
template <int N>
static C2W_HD inline void phase_store(const FieldView& v, int tl) {
    using P = Plan<N>;
    if (tl >= P::R) return;
    if (tl == 0) {
        const double s = field_sum<N>(v);
        v.spec[0] = (float)(s * s / (double)(N * N));
        return;
    }
    double acc = 0.0;
    int n = 0;
    for (int q = 0; q < P::NQ; ++q) acc += v.dpart[tl * P::NQ + q], n += v.cnt[tl * P::NQ + q];
    v.spec[tl] = (float)(acc / (4.0 * (double)(N * N) * (double)n));
}

}  // namespace spectrum
#endif
