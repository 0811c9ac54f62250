// Event objects of an ensemble: the index maps and the integer arithmetic of objects.hip, written as barrier-separated phases over
// "thread tid of a workgroup", as events_core.h and spells_core.h are.  Compiled for the host (core_side.h) the same phases run one
// thread after the other: tests/host_objects_main.cpp walks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_object_tables).  The rows are d = 0 the truth when one is given, then the M members; D rows in all.  The
// event is events_core.h::event_of on exact fp32 values, thr[F][K] and dir[F][K]; a NaN is no event and is counted per (d, t, f) in
// invalid.  An OBJECT is a maximal connected set of event cells of one (d, t, f, k) plane of H x W cells, connectivity 4 (edge
// neighbours) or 8 (edge and corner neighbours), no wrap-around; its LABEL is the smallest linear index i W + j of its cells.
//
// object_tables: a workgroup of 512 owns one (d, t, f, k) plane -- the thresholds run over the grid, the plane is re-read from the
// caches -- of at most MAX_CELLS = 16384 cells (the project's 128 x 128 window; larger planes take the general route of objects.py, a
// 256 x 256 plane in LDS is not built).  A thread owns QUADS of 4 adjacent cells of a row (W is a multiple of 4).  The phases:
//   o_zero     the bit masks, the areas, the list slots, the counters
//   o_stage    one 16-byte load a quad; the indicators go to a BIT MASK (bit n = cell n = i W + j), the NaNs are counted
//   o_label    lab[n] = the first cell of n's run along its row (found in the bit mask, a word at a time), BACKGROUND for no event
//   o_link     the runs of adjacent rows (and diagonals at connectivity 8) are united: a label-equivalence union-find over lab.  find
//              follows strictly decreasing labels; unite links the LARGER root to the smaller with a compare-and-swap that succeeds
//              only while it still is a root, and starts over otherwise.  Only the cell of a run that first sees a run above links.
//   o_flatten  lab[n] = find(n): the label of the object, its smallest index, whatever the order of the links was; the roots to a mask
//   o_rank1-3  the rank of a root among the roots in index order -- the label order of the list -- from the mask's word counts
//   o_runs     a run's first cell adds the run's length ONCE to the area of its root (a 16-bit half of an LDS word, bit 15 the flag
//              "touches the border"), and its sums and box to the list slot of the root where the rank is under max_objects
//   o_roots    a root: the area histogram, the largest area, the censored count, its slot's label and area
//   o_store    plain stores of the plane's row, its list and (k = 0) its NaN count; one 64-bit add per non-zero area bin
// Every data-dependent loop has a trip bound derived from H W: a defect ends in wrong integers, never in a hang.
//
// The LDS budget, in bytes (OFF_* below): labels 32768 + areas 32768 + two bit masks 2 x 2048 + rank tables 2048 + 128 + counters 64
// + area bins 64 + list slots 8 x 4 x 256 = 8192: 80128 <= 80 KiB, so two workgroups share a CU.
#ifndef C2W_OBJECTS_MAPS_H
#define C2W_OBJECTS_MAPS_H

#include "core_side.h"

#ifndef OB_VISIT_LOAD  // the host driver counts here: a cell staged by the workgroup that owns plane b
#define OB_VISIT_LOAD(b, cell)
#endif
#include "events_core.h"  // event_of: the same indicator on every route; the LDS and global adds

namespace objects {

using events::event_of;
using events::F4;
using events::global_add;
using events::lds_add;
using events::lds_inc;

constexpr int THREADS = 512;                 // 8 waves: the passes are chains of dependent LDS reads, and more waves hide more of them
constexpr int MAX_CELLS = 16384, MAX_K = 8, MAX_OBJECTS = 256, MAX_BINS = 15;  // floor(log2(16384)) + 1 bins
constexpr int WORDS = MAX_CELLS / 32;        // 512 words a bit mask
constexpr int BACKGROUND = 0xffff;           // no event: never followed, never a root
constexpr int FIELDS = 8;                    // label, area, sum_i, sum_j, i_min, i_max, j_min, j_max
constexpr int PLANE_SLOTS = 6;               // objects, cells, largest, censored, sum_i, sum_j
constexpr int BORDER_BIT = 0x8000, AREA_MASK = 0x7fff;
constexpr int STAGE = 8;                     // 16-byte loads a thread has in flight while it stages the plane
constexpr int GROUPS = 16, SCANNERS = THREADS / GROUPS;  // the second level of the rank scan: 32 threads x 16 entries
static_assert(MAX_CELLS <= 0x4000, "an area fits 15 bits: bit 15 of its half-word is the border flag");
static_assert(MAX_CELLS < BACKGROUND, "a label fits 16 bits next to the background");
static_assert(THREADS == WORDS && GROUPS * SCANNERS == THREADS, "a thread ranks one word of the root mask");
static_assert((long long)MAX_CELLS * MAX_CELLS < (1LL << 31), "the sums of a plane fit 32 bits");

// the LDS budget, in bytes
constexpr int OFF_LAB = 0;                                  // 32768: u16 labels
constexpr int OFF_AREA = OFF_LAB + 2 * MAX_CELLS;           // 32768: u16 areas, two to a word
constexpr int OFF_BITS = OFF_AREA + 2 * MAX_CELLS;          //  2048: the indicator mask
constexpr int OFF_ROOTS = OFF_BITS + 4 * WORDS;             //  2048: the root mask
constexpr int OFF_S = OFF_ROOTS + 4 * WORDS;                //  2048: roots in each word, then before it within its group, then before it
constexpr int OFF_G = OFF_S + 4 * THREADS;                  //   128: roots of each group of 16 words
constexpr int OFF_MISC = OFF_G + 4 * SCANNERS;              //    64: the counters below
constexpr int OFF_HIST = OFF_MISC + 64;                     //    64: the area bins
constexpr int OFF_SLOTS = OFF_HIST + 64;                    //  8192: the list
constexpr int LDS_BYTES = OFF_SLOTS + 4 * FIELDS * MAX_OBJECTS;  // 80128
// the counters: the first six in the order of the plane's row
constexpr int MISC_OBJECTS = 0, MISC_CELLS = 1, MISC_LARGEST = 2, MISC_BORDER = 3, MISC_SUM_I = 4, MISC_SUM_J = 5, MISC_INVALID = 6, MISC_INTS = 16;
static_assert(LDS_BYTES <= 80 * 1024, "two workgroups share a CU");
static_assert(MAX_BINS <= 16 && OFF_SLOTS % 16 == 0, "the bins fit their part; aligned parts");

static C2W_BOTH inline bool supported(int H, int W, int K, int connectivity, int max_objects) {
    return H >= 1 && W >= 4 && W % 4 == 0 && (long long)H * W <= MAX_CELLS && K >= 1 && K <= MAX_K && (connectivity == 4 || connectivity == 8) &&
           max_objects >= 0 && max_objects <= MAX_OBJECTS;
}
// the bin of an area a >= 1: floor(log2(a)); bins(hw) = floor(log2(hw)) + 1 of them
static C2W_BOTH inline int area_bin(int a) { return 31 - __builtin_clz((unsigned)a); }
static C2W_BOTH inline int bins(int hw) { return area_bin(hw) + 1; }
static C2W_BOTH inline int quads(int hw) { return hw / 4; }
static C2W_BOTH inline int words(int hw) { return (hw + 31) / 32; }
static C2W_BOTH inline int cell_of(int it, int tid) { return (it * THREADS + tid) * 4; }
// a thread's quads one after the other with their row and column, two divisions a pass instead of two a quad
struct Quad {
    int n, i, j;     // the quad's first cell, its row and its column
    int di, dj;      // 4 THREADS cells further on: that many rows and columns
};
static C2W_BOTH inline Quad quad_first(int tid, int W) {
    Quad q;
    q.n = tid * 4, q.i = q.n / W, q.j = q.n % W, q.di = 4 * THREADS / W, q.dj = 4 * THREADS % W;
    return q;
}
static C2W_BOTH inline void quad_next(Quad& q, int W) {
    q.n += 4 * THREADS, q.i += q.di, q.j += q.dj;
    if (q.j >= W) q.j -= W, ++q.i;
}

#ifdef C2W_CORE_HOST
static inline int ld16(const unsigned short* lab, int i) { return lab[i]; }
static inline bool cas16(unsigned short* lab, int i, int expect, int value, int) {
    if (lab[i] != expect) return false;
    lab[i] = (unsigned short)value;
    return true;
}
static inline void lds_or(unsigned* p, unsigned a) { *p |= a; }
static inline void lds_min(int* p, int a) { *p = a < *p ? a : *p; }
static inline void lds_max(int* p, int a) { *p = a > *p ? a : *p; }
#else
// a relaxed atomic load: read anew every time (other threads link meanwhile), and still an LDS instruction, which a volatile access is not
static C2W_HD inline int ld16(const unsigned short* lab, int i) { return __atomic_load_n(lab + i, __ATOMIC_RELAXED); }
// lab[i] = value if it still is expect: a compare-and-swap of the word that holds the half; another thread may change the other half
// meanwhile, at most once per link or shortcut of that cell, hence the bound
static C2W_HD inline bool cas16(unsigned short* lab, int i, int expect, int value, int bound) {
    unsigned* w = (unsigned*)lab + (i >> 1);
    const int sh = (i & 1) * 16;
    unsigned old = __atomic_load_n(w, __ATOMIC_RELAXED);
    for (int trip = 0; trip < bound; ++trip) {
        if ((int)((old >> sh) & 0xffffu) != expect) return false;
        const unsigned seen = atomicCAS(w, old, (old & ~(0xffffu << sh)) | ((unsigned)value << sh));
        if (seen == old) return true;
        old = seen;
    }
    return false;
}
static C2W_HD inline void lds_or(unsigned* p, unsigned a) { atomicOr(p, a); }
static C2W_HD inline void lds_min(int* p, int a) { atomicMin(p, a); }
static C2W_HD inline void lds_max(int* p, int a) { atomicMax(p, a); }
#endif

struct View {
    const float* x;        // [M][T][F][hw]
    const float* y;        // [T][F][hw] or null
    const float* thr;      // [F][K]
    const int* dir;        // [F][K]
    long long* plane;      // [D][T][F][K][6]
    long long* area_hist;  // [D][F][K][bins(hw)]
    int* objects;          // [D][T][F][K][max_objects][8] or null
    long long* invalid;    // [D][T][F]
    long long b;           // the plane this workgroup owns: ((d T + t) F + f) K + k
    int D, T, F, H, W, K, connectivity, max_objects;
    unsigned char* lds;    // LDS_BYTES
};

static C2W_HD inline unsigned short* lab_of(const View& v) { return (unsigned short*)(v.lds + OFF_LAB); }
static C2W_HD inline int* area_of(const View& v) { return (int*)(v.lds + OFF_AREA); }
static C2W_HD inline unsigned* bits_of(const View& v) { return (unsigned*)(v.lds + OFF_BITS); }
static C2W_HD inline unsigned* roots_of(const View& v) { return (unsigned*)(v.lds + OFF_ROOTS); }
static C2W_HD inline int* s_of(const View& v) { return (int*)(v.lds + OFF_S); }
static C2W_HD inline int* g_of(const View& v) { return (int*)(v.lds + OFF_G); }
static C2W_HD inline int* misc_of(const View& v) { return (int*)(v.lds + OFF_MISC); }
static C2W_HD inline int* hist_of(const View& v) { return (int*)(v.lds + OFF_HIST); }
static C2W_HD inline int* slots_of(const View& v) { return (int*)(v.lds + OFF_SLOTS); }

static C2W_HD inline int k_of(const View& v) { return (int)(v.b % v.K); }
static C2W_HD inline int f_of(const View& v) { return (int)(v.b / v.K % v.F); }
static C2W_HD inline int t_of(const View& v) { return (int)(v.b / v.K / v.F % v.T); }
static C2W_HD inline int d_of(const View& v) { return (int)(v.b / v.K / v.F / v.T); }
// the plane's values: row 0 is the truth when there is one
static C2W_HD inline const float* source_of(const View& v) {
    const long long hw = (long long)v.H * v.W, at = ((long long)t_of(v) * v.F + f_of(v)) * hw, member = (long long)v.T * v.F * hw;
    const int d = d_of(v);
    return v.y ? (d == 0 ? v.y + at : v.x + (d - 1) * member + at) : v.x + d * member + at;
}
static C2W_HD inline long long hist_row(const View& v) { return ((long long)d_of(v) * v.F + f_of(v)) * v.K + k_of(v); }

static C2W_HD inline int bit_of(const unsigned* bits, int n) { return (int)((bits[n >> 5] >> (n & 31)) & 1u); }

// A quad and its two neighbours in its row as six bits: bit c + 1 is cell n0 + c, bit 0 the cell before the quad and bit 5 the cell
// behind it, each 0 where the row ends there.  Two reads of the mask instead of one per cell; n0 is a multiple of 4, so a quad never
// straddles two words and only the neighbours may lie in the next or the previous one.
static C2W_HD inline unsigned quad_window(const unsigned* bits, int n0, int j0, int W) {
    const int w = n0 >> 5, s = n0 & 31;
    unsigned six = ((bits[w] >> s) & 15u) << 1;
    if (j0 > 0) six |= s ? (bits[w] >> (s - 1)) & 1u : bits[w - 1] >> 31;
    if (j0 + 4 < W) six |= (s < 28 ? (bits[w] >> (s + 4)) & 1u : bits[w + 1] & 1u) << 5;
    return six;
}
// the four labels of a quad in one 8-byte access
static C2W_HD inline unsigned long long ld_quad(const unsigned short* lab, int n0) {
    unsigned long long q;
    __builtin_memcpy(&q, __builtin_assume_aligned(lab + n0, 8), 8);
    return q;
}
static C2W_HD inline void st_quad(unsigned short* lab, int n0, unsigned long long q) {
    __builtin_memcpy(__builtin_assume_aligned(lab + n0, 8), &q, 8);
}

// the first cell of the run that holds event cell n, not before lo, the first cell of n's row: the mask is read a word at a time
static C2W_HD inline int run_start(const unsigned* bits, int lo, int n) {
    int w = n >> 5;
    unsigned z = ~bits[w] & (0xffffffffu >> (31 - (n & 31)));  // the cells without the event at or before n in n's word
    for (int trip = 0; trip <= WORDS; ++trip) {
        if (z) {
            const int s = (w << 5) + 32 - __builtin_clz(z);
            return s > lo ? s : lo;
        }
        if ((w << 5) <= lo) return lo;
        z = ~bits[--w];
    }
    return lo;
}
// one past the last cell of the run that holds event cell n, at most hi, one past the last cell of n's row
static C2W_HD inline int run_end(const unsigned* bits, int n, int hi) {
    int w = n >> 5;
    unsigned z = ~bits[w] & (0xffffffffu << (n & 31));
    for (int trip = 0; trip <= WORDS; ++trip) {
        if (z) {
            const int e = (w << 5) + __builtin_ctz(z);
            return e < hi ? e : hi;
        }
        if (((++w) << 5) >= hi) return hi;
        z = ~bits[w];
    }
    return hi;
}

// the root of cell a: labels strictly decrease along the way, so hw steps bound it
static C2W_HD inline int find(const unsigned short* lab, int a, int hw) {
    for (int trip = 0; trip < hw; ++trip) {
        const int p = ld16(lab, a);
        if (p >= a) break;
        a = p;
    }
    return a;
}
// The compare-and-link step: the larger of the two roots is linked to the smaller, if it still is a root; if not, somebody linked it
// meanwhile and the step starts over from the new roots.  Each failure is a success of another thread, of which there are under hw.
// A cell that was more than one step from its root is pointed at the root on the way (its label only ever decreases within its set).
static C2W_HD inline void unite(unsigned short* lab, int a, int b, int hw) {
    for (int trip = 0; trip < hw + 16; ++trip) {
        const int pa = ld16(lab, a), pb = ld16(lab, b);
        const int ra = find(lab, a, hw), rb = find(lab, b, hw);
        if (pa != ra && pa != a) cas16(lab, a, pa, ra, hw);
        if (pb != rb && pb != b) cas16(lab, b, pb, rb, hw);
        if (ra == rb) return;
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        if (cas16(lab, hi, hi, lo, hw)) return;
        a = hi, b = lo;
    }
}

static C2W_HD inline void o_zero(const View& v, int tid) {
    const int hw = v.H * v.W;
    unsigned *bits = bits_of(v), *roots = roots_of(v);
    int *area = area_of(v), *slots = slots_of(v);
    for (int i = tid; i < words(hw); i += THREADS) bits[i] = 0, roots[i] = 0;
    for (int i = tid; i < hw / 4; i += THREADS) ((unsigned long long*)area)[i] = 0;  // hw is a multiple of 4: two words, four areas a store
    for (int i = tid; i < v.max_objects * FIELDS; i += THREADS) {
        const int field = i % FIELDS;
        slots[i] = field == 0 ? -1 : field == 4 || field == 6 ? 0x7fffffff : field == 5 || field == 7 ? -1 : 0;
    }
    if (tid < MISC_INTS) misc_of(v)[tid] = 0, hist_of(v)[tid] = 0;
}

static C2W_HD inline void o_stage(const View& v, int tid) {
    const int hw = v.H * v.W, at = f_of(v) * v.K + k_of(v);
    const float thr = v.thr[at];
    const int above = v.dir[at] != 0 ? 1 : 0;
    const float* src = source_of(v);
    unsigned* bits = bits_of(v);
    int n_invalid = 0;
    for (int it = 0; cell_of(it, tid) < hw; it += STAGE) {
        F4 s[STAGE];  // STAGE loads in flight, then the LDS traffic; a quad past the plane reads quad 0 again and forms no term
#pragma unroll
        for (int u = 0; u < STAGE; ++u) s[u] = *(const F4*)(src + (cell_of(it + u, tid) < hw ? cell_of(it + u, tid) : 0));
#pragma unroll
        for (int u = 0; u < STAGE; ++u) {
            const int n = cell_of(it + u, tid);
            if (n >= hw) break;
            unsigned e = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                OB_VISIT_LOAD(v.b, n + c);
                e |= (unsigned)event_of(s[u][c], thr, above) << c;
                n_invalid += s[u][c] != s[u][c] ? 1 : 0;
            }
            if (e) lds_or(bits + (n >> 5), e << (n & 31));  // n is a multiple of 4: the four bits lie in one word
        }
    }
    if (n_invalid) lds_add(misc_of(v) + MISC_INVALID, n_invalid);
}

static C2W_HD inline void o_label(const View& v, int tid) {
    const int hw = v.H * v.W;
    const unsigned* bits = bits_of(v);
    unsigned short* lab = lab_of(v);
    for (Quad at = quad_first(tid, v.W); at.n < hw; quad_next(at, v.W)) {
        const int n = at.n;
        const unsigned e = (bits[n >> 5] >> (n & 31)) & 15u;
        unsigned long long q = 0;
        int start = -1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool on = (e >> c) & 1u;
            if (on && start < 0) start = c == 0 ? run_start(bits, n - at.j, n) : n + c;
            if (!on) start = -1;
            q |= (unsigned long long)(on ? start : BACKGROUND) << (16 * c);
        }
        st_quad(lab, n, q);
    }
}

static C2W_HD inline void o_link(const View& v, int tid) {
    const int hw = v.H * v.W, W = v.W;
    const unsigned* bits = bits_of(v);
    unsigned short* lab = lab_of(v);
    for (Quad at = quad_first(tid, W); at.n < hw; quad_next(at, W)) {
        const int n0 = at.n, j0 = at.j;
        if (n0 < W || !((bits[n0 >> 5] >> (n0 & 31)) & 15u)) continue;  // the first row links to nothing; nor does a quad without events
        const unsigned cur = quad_window(bits, n0, j0, W), above = quad_window(bits, n0 - W, j0, W);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + c, up = n - W;
            if (!((cur >> (c + 1)) & 1u)) continue;
            const bool left = (cur >> c) & 1u, right = (cur >> (c + 2)) & 1u;               // the neighbours in the row, 0 past its ends
            const bool up_left = (above >> c) & 1u, up_right = (above >> (c + 2)) & 1u;
            if ((above >> (c + 1)) & 1u) {
                if (!(left && up_left)) unite(lab, n, up, hw);  // else the cell to the left, of the same run, has linked the two runs
            } else if (v.connectivity == 8) {
                // a run above that holds up would hold both corners; without it each corner is a run of its own to link, unless the
                // neighbour of the same run on that side lies right under it and links it
                if (up_left && !left) unite(lab, n, up - 1, hw);
                if (up_right && !right) unite(lab, n, up + 1, hw);
            }
        }
    }
}

static C2W_HD inline void o_flatten(const View& v, int tid) {
    const int hw = v.H * v.W;
    const unsigned* bits = bits_of(v);
    unsigned* roots = roots_of(v);
    unsigned short* lab = lab_of(v);
    for (int it = 0; cell_of(it, tid) < hw; ++it) {
        const int n0 = cell_of(it, tid);
        const unsigned e = (bits[n0 >> 5] >> (n0 & 31)) & 15u;
        if (!e) continue;
        const unsigned long long was = ld_quad(lab, n0);
        unsigned long long q = 0;
        unsigned mine = 0;
        int r = -1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool on = (e >> c) & 1u;
            if (on && r < 0) r = find(lab, (int)((was >> (16 * c)) & 0xffffu), hw);  // adjacent cells are one run: one walk serves them
            if (!on) r = -1;
            q |= (unsigned long long)(on ? r : BACKGROUND) << (16 * c);
            mine |= on && r == n0 + c ? 1u << c : 0u;
        }
        st_quad(lab, n0, q);  // a cell another thread walks through points at the same root before and after
        if (mine) lds_or(roots + (n0 >> 5), mine << (n0 & 31));
    }
}

// the roots before each word of the root mask: a thread's word, 32 threads scan 16 of those each, and the sums of the groups before
static C2W_HD inline void o_rank1(const View& v, int tid) {
    s_of(v)[tid] = tid < words(v.H * v.W) ? __builtin_popcount(roots_of(v)[tid]) : 0;
}
static C2W_HD inline void o_rank2(const View& v, int tid) {
    if (tid >= SCANNERS) return;
    int* s = s_of(v) + tid * GROUPS;
    int run = 0;
    for (int u = 0; u < GROUPS; ++u) {
        const int c = s[u];
        s[u] = run, run += c;
    }
    g_of(v)[tid] = run;
    if (run) lds_add(misc_of(v) + MISC_OBJECTS, run);
}
static C2W_HD inline void o_rank3(const View& v, int tid) {
    int base = s_of(v)[tid];  // a thread reads its own entry and the groups' sums, and writes its own entry
    for (int q = 0; q < tid / GROUPS; ++q) base += g_of(v)[q];
    s_of(v)[tid] = base;
}
static C2W_HD inline int rank_of(const View& v, int root) {
    return s_of(v)[root >> 5] + __builtin_popcount(roots_of(v)[root >> 5] & ((1u << (root & 31)) - 1u));
}

static C2W_HD inline void o_runs(const View& v, int tid) {
    const int hw = v.H * v.W, W = v.W;
    const unsigned* bits = bits_of(v);
    const unsigned short* lab = lab_of(v);
    int *area = area_of(v), *slots = slots_of(v);
    int cells = 0, sum_i = 0, sum_j = 0;
    for (Quad at = quad_first(tid, W); at.n < hw; quad_next(at, W)) {
        const int n0 = at.n, i = at.i, j0 = at.j;
        if (!((bits[n0 >> 5] >> (n0 & 31)) & 15u)) continue;
        const unsigned cur = quad_window(bits, n0, j0, W);
        const unsigned long long labels = ld_quad(lab, n0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + c, j = j0 + c;
            if (!((cur >> (c + 1)) & 1u) || ((cur >> c) & 1u)) continue;  // a run's first cell speaks for the run
            const unsigned rest = ~(cur >> (c + 1)) & (31u >> c);         // the cells of the window from n on without the event
            const int len = rest ? __builtin_ctz(rest) : run_end(bits, n0 + 4, (i + 1) * W) - n;  // it ends in the window, or is walked
            const int root = (int)((labels >> (16 * c)) & 0xffffu), sh = (root & 1) * 16;
            const int run_j = len * (2 * j + len - 1) / 2;
            const bool border = i == 0 || i == v.H - 1 || j == 0 || j + len == W;
            lds_add(area + (root >> 1), len << sh);
            if (border) lds_or((unsigned*)area + (root >> 1), (unsigned)BORDER_BIT << sh);
            cells += len, sum_i += i * len, sum_j += run_j;
            if (v.max_objects == 0) continue;
            const int r = rank_of(v, root);
            if (r >= v.max_objects) continue;
            int* slot = slots + r * FIELDS;
            lds_add(slot + 2, i * len), lds_add(slot + 3, run_j);
            lds_min(slot + 4, i), lds_max(slot + 5, i), lds_min(slot + 6, j), lds_max(slot + 7, j + len - 1);
        }
    }
    int* misc = misc_of(v);
    if (cells) lds_add(misc + MISC_CELLS, cells), lds_add(misc + MISC_SUM_I, sum_i), lds_add(misc + MISC_SUM_J, sum_j);
}

static C2W_HD inline void o_roots(const View& v, int tid) {
    const int nw = words(v.H * v.W);
    const unsigned short* area = (const unsigned short*)(v.lds + OFF_AREA);
    int *misc = misc_of(v), *hist = hist_of(v), *slots = slots_of(v);
    if (tid < nw) {
        const int w = tid;
        unsigned m = roots_of(v)[w];
        int r = s_of(v)[w];
        for (int trip = 0; trip < 32 && m; ++trip, ++r) {
            const int n = (w << 5) + __builtin_ctz(m), a16 = area[n], a = a16 & AREA_MASK;
            m &= m - 1;
            if (a < 1) continue;  // cannot be: a root is an event cell
            lds_inc(hist + area_bin(a));
            lds_max(misc + MISC_LARGEST, a);
            if (a16 & BORDER_BIT) lds_inc(misc + MISC_BORDER);
            if (r < v.max_objects) slots[r * FIELDS] = n, slots[r * FIELDS + 1] = a;
        }
    }
}

static C2W_HD inline void o_store(const View& v, int tid) {
    const int* misc = misc_of(v);
    const int nb = bins(v.H * v.W), listed = misc[MISC_OBJECTS] < v.max_objects ? misc[MISC_OBJECTS] : v.max_objects;
    if (tid < PLANE_SLOTS) v.plane[v.b * PLANE_SLOTS + tid] = (long long)misc[tid];
    if (tid == 0 && k_of(v) == 0) v.invalid[v.b / v.K] = (long long)misc[MISC_INVALID];
    if (tid < nb && hist_of(v)[tid]) global_add(v.area_hist + hist_row(v) * nb + tid, (long long)hist_of(v)[tid]);
    const int* slots = slots_of(v);
    for (int i = tid; i < v.max_objects * FIELDS; i += THREADS)
        v.objects[v.b * v.max_objects * FIELDS + i] = i / FIELDS < listed ? slots[i] : (i % FIELDS == 0 ? -1 : 0);
}

}  // namespace objects
#endif
