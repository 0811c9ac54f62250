// Event spells of an ensemble: the index maps and the integer arithmetic of spells.hip, written as barrier-separated phases over
// "thread tid of a workgroup", as events_core.h and temporal_core.h are.  Compiled for the host (core_side.h) the same phases run one
// thread after the other: tests/host_spells_main.cpp walks every map below without a GPU.
//
// Definition (c2w_hip.h: c2w_spell_update).  The rows are d = 0 the truth when one is given, then the M members; D rows in all.  The
// event is events_core.h::event_of on exact fp32 values, thr[F][K] and dir[F][K]; a NaN is no event and is counted per (d, f) in
// invalid.  A SERIES is the indicator of one (d, f, k, cell) over all times seen so far, a SPELL a maximal run of 1s in it.
// state[4][D][F][K][hw] int32 carries a series from one block of times to the next: OPEN (the length of the run open at the last time
// seen, 0 if none), LONGEST, COUNT and HOURS of the spells that have ENDED (hours: of all event hours).  The kernel never closes a run
// at a block's end -- the host does that on a copy when the tables are asked for.
//
// spell_update: a workgroup of 256 owns (row d, variable f, chunk of CHUNK = 1024 cells) and GROUP = 4 thresholds at most (the launcher
// walks the thresholds in groups; the tables' rows are per k, so the groups touch disjoint entries).  A thread owns 4 adjacent cells: it
// loads their state (16 bytes per counter and threshold), walks the block's T planes in order with one 16-byte load a plane, UNROLL = 8
// loads in flight in a straight line -- a step past the end reads plane T - 1 again (the address is clamped) and forms no term -- and
// stores the state where it loaded it.  Per step and (k, cell): an event is ++open, ++hours and, where open was 0, one LDS add to
// onsets[k][phase]; no event with open > 0 is one LDS add to hist[k][min(open, Lmax) - 1], ++count, longest = max(longest, open),
// open = 0.  A field without events costs no LDS traffic.  At the end the workgroup issues one 64-bit add per non-zero LDS entry to the
// global accumulators, which the CALLER zeroed when it created them.  Integer adds commute: no bit depends on any order.
#ifndef C2W_SPELLS_CORE_H
#define C2W_SPELLS_CORE_H

#include "core_side.h"

#ifndef SP_VISIT_READ  // the host driver counts here: a cell-hour read by a threshold group; a state entry loaded; a state entry stored
#define SP_VISIT_READ(d, f, k0, t, cell)
#define SP_VISIT_STATE_LOAD(at)
#define SP_VISIT_STATE_STORE(at)
#endif
#include "events_core.h"  // event_of: the same indicator on every route; the LDS and global adds

namespace spells {

using events::event_of;
using events::global_add;
using events::lds_add;
using events::lds_inc;

constexpr int THREADS = 256;
constexpr int CELLS = 4;                  // adjacent cells a thread owns: 16 bytes a load
constexpr int CHUNK = THREADS * CELLS;    // 1024 cells a workgroup owns
constexpr int GROUP = 4;                  // thresholds a launch serves: 4 cells x 4 thresholds x 4 counters = 64 state registers
constexpr int UNROLL = 8;                 // planes loaded in a straight line
constexpr int MAX_K = 8, MAX_LMAX = 256, MAX_PERIOD = 24;
constexpr int MAX_T = 1 << 20;            // times a call takes: an LDS bin is 32-bit and takes at most CHUNK (T + 1) / 2 adds
constexpr int OPEN = 0, LONGEST = 1, COUNT = 2, HOURS = 3, COUNTERS = 4;  // the planes of state
constexpr int LDS_HIST = 0, LDS_ONSETS = GROUP * MAX_LMAX, LDS_INVALID = LDS_ONSETS + GROUP * MAX_PERIOD;
constexpr int LDS_INTS = LDS_INVALID + 1;  // 1121 ints, 4484 bytes
static_assert((long long)CHUNK * MAX_T < (1LL << 31), "an LDS bin cannot overflow");
static_assert(GROUP * CELLS * COUNTERS == 64, "the state registers of a thread");

typedef float F4 __attribute__((vector_size(16)));  // 16 bytes a load
typedef int I4 __attribute__((vector_size(16)));

static C2W_BOTH inline bool supported(int hw, int K, int lmax, int period) {
    return hw >= 4 && hw % 4 == 0 && K >= 1 && K <= MAX_K && lmax >= 1 && lmax <= MAX_LMAX && period >= 0 && period <= MAX_PERIOD;
}
static C2W_BOTH inline int chunks(int hw) { return (hw + CHUNK - 1) / CHUNK; }
static C2W_BOTH inline int cell_of(int chunk, int tid) { return chunk * CHUNK + tid * CELLS; }
static C2W_BOTH inline int groups(int K) { return (K + GROUP - 1) / GROUP; }
static C2W_BOTH inline int group_size(int K, int g) { return K - g * GROUP < GROUP ? K - g * GROUP : GROUP; }

struct View {
    const float* x;      // [M][T][F][hw]
    const float* y;      // [T][F][hw] or null
    const float* thr;    // [F][K]
    const int* dir;      // [F][K]
    int* state;          // [4][D][F][K][hw]
    long long* hist;     // [D][F][K][lmax]
    long long* onsets;   // [D][F][K][period] or null
    long long* invalid;  // [D][F]
    int d, f, chunk;     // what this workgroup owns
    int k0, kn;          // the thresholds k0 .. k0 + kn - 1 of this launch; the launch with k0 == 0 counts the NaNs
    int D, T, F, hw, K, lmax, period, phase0;  // phase0 = t0 mod period
    int* lds;            // LDS_INTS
};

// event_of with the direction folded into a sign: x <= thr is -x >= -thr for every pair of IEEE numbers, the infinities and both
// zeros included, and a NaN stays no event under either sign -- so one compare serves both directions.  flip is 0 (above) or the sign
// bit (below), sthr the threshold with the same bit flipped.  tests/host_spells_main.cpp holds it against event_of on the special values.
static C2W_BOTH inline unsigned flip_of(int above) { return above ? 0u : 0x80000000u; }
static C2W_BOTH inline float flipped(float v, unsigned flip) {
    unsigned u;
    __builtin_memcpy(&u, &v, 4);
    u ^= flip;
    __builtin_memcpy(&v, &u, 4);
    return v;
}
static C2W_BOTH inline int event_flipped(float v, float sthr, unsigned flip) { return flipped(v, flip) >= sthr ? 1 : 0; }

// entry (counter s, threshold k0 + k, cell) of state
static C2W_HD inline long long state_at(const View& v, int s, int k, int cell) {
    return ((((long long)s * v.D + v.d) * v.F + v.f) * v.K + v.k0 + k) * v.hw + cell;
}
// plane (t = 0, f) of the row this workgroup owns
static C2W_HD inline const float* row_of(const View& v) {
    const long long member = (long long)v.T * v.F * v.hw;
    const float* row = v.y ? (v.d == 0 ? v.y : v.x + (v.d - 1) * member) : v.x + v.d * member;
    return row + (long long)v.f * v.hw;
}
static C2W_HD inline long long table_row(const View& v, int k) { return ((long long)v.d * v.F + v.f) * v.K + v.k0 + k; }

static C2W_HD inline void s_zero(const View& v, int tid) {
    for (int i = tid; i < LDS_INTS; i += THREADS) v.lds[i] = 0;
}

// one cell-hour of one threshold: the counters are references into the thread's registers
static C2W_HD inline void s_step(const View& v, int k, int e, int phase, int& open, int& longest, int& count, int& hours) {
    const int was = open;
    const bool ending = !e && was > 0, starting = e && was == 0;
    open = e ? was + 1 : 0;  // the counters move without a branch; only the two LDS adds, which are rare, are under one
    hours += e;
    count += ending ? 1 : 0;
    longest = ending && was > longest ? was : longest;
    if (ending) lds_inc(v.lds + LDS_HIST + k * MAX_LMAX + (was < v.lmax ? was : v.lmax) - 1);
    if (starting && v.period) lds_inc(v.lds + LDS_ONSETS + k * MAX_PERIOD + phase);
}

static C2W_HD inline void s_walk(const View& v, int tid) {
    const int cell = cell_of(v.chunk, tid);
    if (cell >= v.hw) return;  // hw is a multiple of 4: a thread has its four cells or none
    float sthr[GROUP];
    unsigned flip[GROUP];
#pragma unroll
    for (int k = 0; k < GROUP; ++k) {
        flip[k] = k < v.kn ? flip_of(v.dir[v.f * v.K + v.k0 + k]) : 0u;
        sthr[k] = k < v.kn ? flipped(v.thr[v.f * v.K + v.k0 + k], flip[k]) : 0.f;
    }
    int st[COUNTERS][GROUP][CELLS];
#pragma unroll
    for (int s = 0; s < COUNTERS; ++s) {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            I4 q = {0, 0, 0, 0};
            if (k < v.kn) {
                SP_VISIT_STATE_LOAD(state_at(v, s, k, cell));
                q = *(const I4*)(v.state + state_at(v, s, k, cell));
            }
#pragma unroll
            for (int c = 0; c < CELLS; ++c) st[s][k][c] = q[c];
        }
    }
    const float* row = row_of(v) + cell;
    const long long stride = (long long)v.F * v.hw;
    const int last = v.T - 1;
    int n_invalid = 0, phase = v.phase0;
    for (int tb = 0; tb < v.T; tb += UNROLL) {
        F4 a[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) a[u] = *(const F4*)(row + (long long)(tb + u < last ? tb + u : last) * stride);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (tb + u > last) break;  // the same for the whole workgroup: its load was clamped, it forms no term
            SP_VISIT_READ(v.d, v.f, v.k0, tb + u, cell);
#pragma unroll
            for (int c = 0; c < CELLS; ++c) {
                const float val = a[u][c];
                n_invalid += val != val ? 1 : 0;
#pragma unroll
                for (int k = 0; k < GROUP; ++k) {
                    if (k >= v.kn) break;
                    s_step(v, k, event_flipped(val, sthr[k], flip[k]), phase, st[OPEN][k][c], st[LONGEST][k][c], st[COUNT][k][c], st[HOURS][k][c]);
                }
            }
            phase = phase + 1 < v.period ? phase + 1 : 0;
        }
    }
#pragma unroll
    for (int s = 0; s < COUNTERS; ++s) {
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            if (k >= v.kn) break;
            SP_VISIT_STATE_STORE(state_at(v, s, k, cell));
            *(I4*)(v.state + state_at(v, s, k, cell)) = I4{st[s][k][0], st[s][k][1], st[s][k][2], st[s][k][3]};
        }
    }
    if (v.k0 == 0 && n_invalid) lds_add(v.lds + LDS_INVALID, n_invalid);
}

// one 64-bit add per non-zero entry of the workgroup's bins
static C2W_HD inline void s_flush(const View& v, int tid) {
    for (int i = tid; i < v.kn * v.lmax; i += THREADS) {
        const int k = i / v.lmax, b = i % v.lmax, n = v.lds[LDS_HIST + k * MAX_LMAX + b];
        if (n) global_add(v.hist + table_row(v, k) * v.lmax + b, (long long)n);
    }
    for (int i = tid; i < v.kn * v.period; i += THREADS) {
        const int k = i / v.period, p = i % v.period, n = v.lds[LDS_ONSETS + k * MAX_PERIOD + p];
        if (n) global_add(v.onsets + table_row(v, k) * v.period + p, (long long)n);
    }
    if (tid == 0 && v.lds[LDS_INVALID]) global_add(v.invalid + (long long)v.d * v.F + v.f, (long long)v.lds[LDS_INVALID]);
}

}  // namespace spells
#endif
