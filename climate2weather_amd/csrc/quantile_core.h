// Exact order statistics by radix select: the index maps, the key map, the slot logic and the final arithmetic of quantile.hip, written
// as barrier-separated phases over "thread tid of a workgroup", as kde_core.h is.  Compiled for the host (core_side.h) the same phases
// run one thread after the other: tests/host_quantile_main.cpp checks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_quantiles).  Data set d < n_rep F is x[d / F][t][d % F][:] for all t < T, the others are variable
// d - n_rep F of the truth y[T][F][hw]; n = T hw values each.  For level q: nv = #non-NaN, v = (nv - 1) q in double, lo = floor(v),
// hi = min(lo + 1, nv - 1), t = v - lo, a / b the lo-th / hi-th smallest non-NaN value, result a + (b - a) t (t < 0.5) or
// b - (b - a)(1 - t), in double without contraction: numpy's method="linear".
//
// Key: k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) on the loaded bit pattern -- unsigned order of k is the order of the values,
// -0.0 just below +0.0, denormals kept.  A NaN (by its bits) goes to the data set's NaN counter and never to a bin.
//
// Three counting passes over the key's digits, 12 / 10 / 10 bits, most significant first.  Pass 0 counts all 4096 bins of every data
// set.  quantile_locate then turns each of the R = 2 Q target ranks (lo and hi of every level) into (bin, rank within the bin); the
// distinct bins become SLOTS, sorted by their key prefix, and the next pass counts the next digit of every value whose prefix is a
// slot's, 1024 bins per slot.  A value finds its slot through tab[4096]: top 12 key bits -> the first slot with these bits (255: none),
// then a walk over the (few) slots that share them.  After pass 2 a slot's prefix and the rank's bin are the whole key.
// Every number is an integer count: no result depends on the grid, the slab arithmetic or the order of the adds.
#ifndef C2W_QUANTILE_CORE_H
#define C2W_QUANTILE_CORE_H

#include "core_side.h"

namespace qnt {

constexpr int THREADS = 1024;        // counting workgroup: sixteen waves, one 16-byte load a thread and step
constexpr int LOCATE_THREADS = 128;  // locating workgroup: one per data set
constexpr int MAX_Q = 16;            // levels per call
constexpr int MAX_RANKS = 2 * MAX_Q;
constexpr int BITS0 = 12, BITS1 = 10, BITS2 = 10;  // key digits, most significant first
static_assert(BITS0 + BITS1 + BITS2 == 32 && BITS1 == BITS2, "the digits are the key; passes 1 and 2 share one kernel shape");
constexpr int BINS0 = 1 << BITS0;  // 4096: 16 KiB of LDS counters in pass 0
constexpr int BINS = 1 << BITS1;   // 1024 per slot in passes 1 and 2: 4 KiB a slot, 128 KiB at 32 slots
constexpr int NONE = 255;          // tab entry: no slot has these top bits
constexpr int LOADS = 4;          // 16-byte loads a counting thread has in flight
constexpr int WG_PER_CU = 8;       // counting workgroups per compute unit the slab count aims at

static C2W_BOTH inline bool supported(int hw, int Q) { return hw >= 4 && hw % 4 == 0 && Q >= 1 && Q <= MAX_Q; }

// ---------------------------------------------------------------------------------------------------------------- key

static C2W_BOTH inline unsigned key_of(unsigned bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
static C2W_BOTH inline unsigned bits_of(unsigned key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
static C2W_BOTH inline bool is_nan_bits(unsigned bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }  // v != v, on the bits
static C2W_BOTH inline float float_of(unsigned bits) { return __builtin_bit_cast(float, bits); }

// ---------------------------------------------------------------------------------------------------------------- scratch

// byte offsets into the scratch for D data sets and R = 2 Q ranks; [0, zeroed) is what the call zeroes on the stream
struct Layout {
    long long table0;  // long long [D][BINS0]
    long long table1;  // long long [D][R][BINS]
    long long table2;  // long long [D][R][BINS]
    long long nan;     // long long [D]
    long long zeroed;
    long long res;     // long long [D][R]   rank within the rank's slot
    long long pre;     // unsigned [D][R]    key prefix of every slot, ascending
    long long rslot;   // int [D][R]         slot of every rank
    long long ns;      // int [D]            slots in use; 0: the row is NaN, nothing more is counted
    long long tab;     // unsigned char [D][BINS0]
    long long total;
};

static C2W_BOTH inline Layout layout(long long D, int Q) {
    const long long R = 2 * Q;
    Layout l;
    l.table0 = 0;
    l.table1 = l.table0 + D * BINS0 * 8;
    l.table2 = l.table1 + D * R * BINS * 8;
    l.nan = l.table2 + D * R * BINS * 8;
    l.zeroed = l.nan + D * 8;
    l.res = l.zeroed;
    l.pre = l.res + D * R * 8;
    l.rslot = l.pre + D * R * 4;
    l.ns = l.rslot + D * R * 4;
    l.tab = l.ns + (D * 4 + 7) / 8 * 8;
    l.total = (l.tab + D * BINS0 + 15) / 16 * 16;
    return l;
}

// LDS bytes of a counting workgroup: the counters, then (passes 1, 2) the slot prefixes and the table, then the NaN counter
static C2W_BOTH inline int count_lds_bytes(int pass, int Q) { return pass == 0 ? BINS0 * 4 + 16 : 2 * Q * BINS * 4 + 2 * Q * 4 + BINS0 + 16; }

// ---------------------------------------------------------------------------------------------------------------- slabs

// slabs per data set: WG_PER_CU workgroups a compute unit over all D data sets, one plane a slab at least
static C2W_BOTH inline int slab_count(long long D, int T, int cus) {
    long long s = (long long)cus * WG_PER_CU / (D < 1 ? 1 : D);
    return (int)(s < 1 ? 1 : s > T ? T : s);
}
static C2W_BOTH inline int slab_planes(int T, int slabs) { return (T + slabs - 1) / slabs; }
static C2W_BOTH inline int slab_begin(int T, int slabs, int s) {
    const long long b = (long long)s * slab_planes(T, slabs);
    return (int)(b < T ? b : T);
}
static C2W_BOTH inline int slab_end(int T, int slabs, int s) {
    const long long e = (long long)(s + 1) * slab_planes(T, slabs);
    return (int)(e < T ? e : T);
}

// ---------------------------------------------------------------------------------------------------------------- counting: phases

struct CView {
    const float* x;  // samples [n_rep][T][F][hw]
    const float* y;  // truth [T][F][hw] or null
    long long n_x;   // n_rep F
    long long ds;    // this workgroup's data set
    int slab, slabs;
    int T, F, hw;
    int pass, R;
    long long* table;  // this data set's table of this pass: [BINS0] or [R][BINS]
    long long* nan;    // this data set's NaN counter
    const unsigned* pre;       // this data set's slot prefixes [R]
    const unsigned char* tab;  // this data set's [BINS0]
    int ns;                    // this data set's slots (passes 1, 2)
    int* hist;                 // LDS: BINS0 or R BINS counters
    unsigned* lpre;            // LDS: R
    unsigned char* ltab;       // LDS: BINS0
    int* lnan;                 // LDS: 1
#ifdef C2W_CORE_HOST
    int* owner;  // visit mode: the fields hold their own indices; owner[k] is the data set that loaded value k (-1 nobody, -2 twice)
#endif
};

#ifdef C2W_CORE_HOST
static inline void lds_add(int* p, int a) { *p += a; }
static inline void global_add(long long* p, long long a) { *p += a; }
struct alignas(16) Quad { unsigned x, y, z, w; };
#else
static C2W_HD inline void lds_add(int* p, int a) { atomicAdd(p, a); }
#ifndef QNT_COMBINE
#define QNT_COMBINE 1  // on by measurement (profiles/quantiles_measurements.md); -DQNT_COMBINE=0 is the build without it
#endif
static C2W_HD inline void global_add(long long* p, long long a) { atomicAdd((unsigned long long*)p, (unsigned long long)a); }
using Quad = uint4;
#endif

// one more value in counter p.  QNT_COMBINE: when every active lane of the wave holds the same counter (a constant field in every pass,
// a pressure field in pass 0) one lane adds the wave's count instead of 64 lanes queueing on one LDS address; the count is the same
#if defined(C2W_CORE_HOST) || !QNT_COMBINE
static C2W_HD inline void lds_count(int* p) { lds_add(p, 1); }
#else
static C2W_HD inline void lds_count(int* p) {
    const int mine = (int)(size_t)p, first = __builtin_amdgcn_readfirstlane(mine);
    if (__all(mine == first)) {
        const unsigned long long active = __ballot(1);
        if ((int)__lane_id() == __ffsll((long long)active) - 1) lds_add(p, __popcll(active));
    } else {
        lds_add(p, 1);
    }
}
#endif

static C2W_BOTH inline const float* set_base(const CView& v) {
    return v.ds < v.n_x ? v.x + ((v.ds / v.F) * v.T * v.F + v.ds % v.F) * (long long)v.hw : v.y + (v.ds - v.n_x) * (long long)v.hw;
}
static C2W_BOTH inline int count_bins(const CView& v) { return v.pass == 0 ? BINS0 : v.ns * BINS; }

static C2W_HD inline void c_zero(const CView& v, int tid) {
    for (int i = tid; i < count_bins(v); i += THREADS) v.hist[i] = 0;
    if (tid == 0) *v.lnan = 0;
    if (v.pass == 0) return;
    for (int i = tid; i < BINS0; i += THREADS) v.ltab[i] = v.tab[i];
    if (tid < v.ns) v.lpre[tid] = v.pre[tid];
}

// one value: its bin of this pass, if it has one
template <bool FIRST>
static C2W_HD inline void c_one(const CView& v, unsigned bits, int& nans) {
    if (is_nan_bits(bits)) {
        if (FIRST) ++nans;
        return;
    }
    const unsigned k = key_of(bits), top = k >> (32 - BITS0);
    if (FIRST) {
        lds_count(v.hist + top);
        return;
    }
    const int shift = v.pass == 1 ? BITS2 + BITS1 : BITS2;  // the key bits below the prefix
    const int up = 32 - BITS0 - shift;                      // the prefix bits below its top 12
    for (int j = v.ltab[top]; j < v.ns && (v.lpre[j] >> up) == top; ++j)  // NONE = 255 >= ns
        if (v.lpre[j] == (k >> shift)) {
            lds_count(v.hist + j * BINS + (int)((k >> (shift - BITS1)) & (BINS - 1)));
            break;
        }
}

// the slab's planes as one list of 16-byte quads (hw % 4 == 0: a quad never leaves its plane), a quad a thread and step
template <bool FIRST>
static C2W_HD inline void c_count(const CView& v, int tid) {
    const int t0 = slab_begin(v.T, v.slabs, v.slab), t1 = slab_end(v.T, v.slabs, v.slab);
    const unsigned quads = (unsigned)v.hw / 4;
    const long long items = (long long)(t1 - t0) * quads, plane = (long long)v.F * v.hw;  // items < 2^29: the launcher bounds the slab
    const float* base = set_base(v) + t0 * plane;
    int nans = 0;
    for (long long i0 = tid; i0 < items; i0 += LOADS * THREADS) {  // LOADS loads in flight before the first is counted
        Quad b[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const long long i = i0 + u * THREADS;
            if (i >= items) continue;
            const unsigned t = (unsigned)i / quads, q = (unsigned)i - t * quads;
            const float* p = base + t * plane + 4 * q;
            b[u] = *(const Quad*)p;
#ifdef C2W_CORE_HOST
            if (v.owner)
                for (int e = 0; e < 4; ++e) v.owner[(long long)p[e]] = v.owner[(long long)p[e]] == -1 ? (int)v.ds : -2;
#endif
        }
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            if (i0 + u * THREADS >= items) continue;
            c_one<FIRST>(v, b[u].x, nans), c_one<FIRST>(v, b[u].y, nans), c_one<FIRST>(v, b[u].z, nans), c_one<FIRST>(v, b[u].w, nans);
        }
    }
    if (FIRST && nans) lds_add(v.lnan, nans);
}

// one 64-bit integer add per non-zero bin
static C2W_HD inline void c_flush(const CView& v, int tid) {
    for (int i = tid; i < count_bins(v); i += THREADS)
        if (v.hist[i]) global_add(v.table + i, v.hist[i]);
    if (v.pass == 0 && tid == 0 && *v.lnan) global_add(v.nan, *v.lnan);
}

// ---------------------------------------------------------------------------------------------------------------- locating: phases

struct Levels {
    double q[MAX_Q];
};

struct LView {
    long long ds, n;  // the data set, its values NaNs included
    int Q, R, pass, skipna;
    int ns_in, is_dead;  // l_open: the slots the tables of this pass hold; the row is NaN and nothing more is counted
    const double* q;  // [Q] levels (LDS on the device)
    // this data set's part of the scratch
    const long long* table;  // [BINS0] or [R][BINS]
    const long long* nan;
    long long* res;
    unsigned* pre;
    int* rslot;
    int* ns;
    unsigned char* tab;
    // outputs, whole arrays
    double* out;        // [D][Q]
    float* stats;       // [D][Q][2]
    long long* nvalid;  // [D]
    // LDS
    long long* part;   // [MAX_RANKS][LOCATE_THREADS]
    unsigned* newpre;  // [MAX_RANKS]
    int* isfirst;      // [MAX_RANKS]
};

static C2W_BOTH inline long long valid_count(const LView& v) { return v.n - *v.nan; }
// the row is NaN and nothing more is counted: no value, or a NaN where NaNs are not skipped
static C2W_BOTH inline bool dead_at_first(const LView& v) { return valid_count(v) <= 0 || (!v.skipna && *v.nan > 0); }
// before any phase writes: what the previous pass left (dead: no value, a NaN where NaNs are not skipped, or marked so by pass 0)
static C2W_BOTH inline void l_open(LView& v) {
    const int ns = v.pass == 0 ? 1 : *v.ns;
    v.ns_in = ns < 0 ? 0 : ns > v.R ? v.R : ns;
    v.is_dead = v.pass == 0 ? dead_at_first(v) : v.ns_in == 0;
}
static C2W_BOTH inline int slots_in(const LView& v) { return v.ns_in; }
static C2W_BOTH inline int bins_in(const LView& v) { return v.pass == 0 ? BINS0 : BINS; }

// v = (nv - 1) q; rank r is lo = floor(v) (r even) or min(lo + 1, nv - 1) (r odd) of level r / 2
static C2W_BOTH inline long long rank_of(long long nv, double q, int odd) {
    const double pos = (double)(nv - 1) * q;
    long long lo = (long long)floor(pos);
    lo = lo < 0 ? 0 : lo > nv - 1 ? nv - 1 : lo;
    return odd ? (lo + 1 < nv - 1 ? lo + 1 : nv - 1) : lo;
}

// numpy's _lerp in double, every operation rounded on its own
static C2W_BOTH inline double lerp_of(long long nv, double q, float fa, float fb) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double pos = (double)(nv - 1) * q;
    const double t = pos - floor(pos), a = (double)fa, b = (double)fb, diff = b - a;
    const double up = diff * t, down = diff * (1.0 - t);
    return t >= 0.5 ? b - down : a + up;
}

// pass 0: the ranks; every pass: the sums of every slot's table over LOCATE_THREADS equal chunks, and an empty tab
static C2W_HD inline void l_sums(const LView& v, int tid) {
    if (v.pass == 0) {
        if (tid == 0) v.nvalid[v.ds] = valid_count(v);
        if (tid < v.R) v.res[tid] = v.is_dead ? 0 : rank_of(valid_count(v), v.q[tid / 2], tid & 1), v.rslot[tid] = 0;
    }
    const int chunk = bins_in(v) / LOCATE_THREADS;
    for (int s = 0; s < slots_in(v); ++s) {
        const long long* t = v.table + (long long)s * BINS + tid * chunk;  // pass 0 has one slot
        long long sum = 0;
        for (int b = 0; b < chunk; ++b) sum += t[b];
        v.part[s * LOCATE_THREADS + tid] = sum;
    }
    if (v.pass < 2)
        for (int i = tid; i < BINS0; i += LOCATE_THREADS) v.tab[i] = (unsigned char)NONE;
}

static C2W_BOTH inline bool dead(const LView& v) { return v.is_dead != 0; }

// rank tid: the bin of its slot's table that holds it, and its rank within that bin
static C2W_HD inline void l_find(const LView& v, int tid) {
    if (tid >= v.R || dead(v)) return;
    int s = v.rslot[tid];
    s = s < 0 ? 0 : s >= slots_in(v) ? slots_in(v) - 1 : s;
    const long long want = v.res[tid];
    const int chunk = bins_in(v) / LOCATE_THREADS;
    long long cum = 0;
    int c = 0;
    for (; c < LOCATE_THREADS - 1; ++c) {
        const long long p = v.part[s * LOCATE_THREADS + c];
        if (cum + p > want) break;
        cum += p;
    }
    const long long* t = v.table + (long long)s * BINS;
    int b = c * chunk;
    for (const int e = b + chunk; b < e - 1; ++b) {
        if (cum + t[b] > want) break;
        cum += t[b];
    }
    v.newpre[tid] = v.pass == 0 ? (unsigned)b : (v.pre[s] << BITS1) | (unsigned)b;
    v.res[tid] = want - cum;
}

// rank tid is the first of the ranks with its new prefix
static C2W_HD inline void l_mark(const LView& v, int tid) {
    if (tid >= v.R || dead(v)) return;
    int first = 1;
    for (int p = 0; p < tid; ++p) first &= v.newpre[p] != v.newpre[tid];
    v.isfirst[tid] = first;
}

// the distinct new prefixes, ascending, are the next pass's slots; tab points at the first slot of every top-12 value in use
static C2W_HD inline void l_slots(const LView& v, int tid) {
    if (dead(v)) {
        if (tid == 0) *v.ns = 0;
        return;
    }
    if (tid >= v.R) return;
    const unsigned mine = v.newpre[tid];
    const int up = v.pass == 0 ? 0 : BITS1;  // the new prefix's bits below its top 12
    bool first_of_top = true;
    int slot = 0, total = 0;
    for (int r = 0; r < v.R; ++r) {
        const unsigned other = v.newpre[r];
        total += v.isfirst[r];
        slot += v.isfirst[r] && other < mine;
        first_of_top &= !((other >> up) == (mine >> up) && other < mine);
    }
    v.rslot[tid] = slot;
    if (v.isfirst[tid]) v.pre[slot] = mine;
    if (v.isfirst[tid] && first_of_top) v.tab[mine >> up] = (unsigned char)slot;
    if (tid == 0) *v.ns = total;
}

// after pass 2 a rank's new prefix is its key: level tid's two order statistics and the interpolation
static C2W_HD inline void l_final(const LView& v, int tid) {
    if (tid >= v.Q) return;
    const long long at = v.ds * v.Q + tid;
    if (dead(v)) {
        v.stats[2 * at] = v.stats[2 * at + 1] = __builtin_nanf("");
        v.out[at] = (double)__builtin_nanf("");
        return;
    }
    const float a = float_of(bits_of(v.newpre[2 * tid])), b = float_of(bits_of(v.newpre[2 * tid + 1]));
    v.stats[2 * at] = a, v.stats[2 * at + 1] = b;
    v.out[at] = lerp_of(valid_count(v), v.q[tid], a, b);
}

}  // namespace qnt
#endif
