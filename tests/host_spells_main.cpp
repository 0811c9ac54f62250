// Host driver for csrc/spells_core.h: runs the phases of spell_update_kernel one thread after the other, workgroup by workgroup and
// threshold group by threshold group (tests/test_spells_cpu.py: the index maps and the integer arithmetic of csrc/spells.hip without a
// GPU).
//   host_spells update M T F hw K Lmax period t0 has_truth split x.f32 y.f32 thr.f32 dir.i32 state.i32 hist.i64 onsets.i64 invalid.i64
//   host_spells visit M T F hw K Lmax period has_truth
// update reads x [M][T][F][hw] and y [T][F][hw], starts from a zeroed state and zeroed accumulators, and takes the T times as one block
// (split = 0) or as the two blocks [0, split) and [split, T), each repacked densely as a caller would hand it over; it writes the state
// and the accumulators as they are, no run closed.  visit counts, through the SP_VISIT_* hooks, that every (row, variable, cell, time)
// is read exactly once per threshold group and every state entry loaded and stored exactly once, nothing out of range.  LDS is filled
// with a pattern before every workgroup, so a slot nobody zeroed shows.  It has its own main, so it is built with
// -fsanitize=address,undefined and run directly.
#include "host_main.h"

static bool g_visit = false;
static int g_bad = 0, g_D = 0, g_T = 0, g_F = 0, g_hw = 0, g_groups = 0;
static std::vector<int> g_reads, g_loads, g_stores;  // [group][d][f][t][cell]; [state entry] twice
static void visit_read(int d, int f, int k0, int t, int cell) {
    if (!g_visit) return;
    const int g = k0 / 4;
    if (d < 0 || d >= g_D || f < 0 || f >= g_F || t < 0 || t >= g_T || cell < 0 || cell + 4 > g_hw || g >= g_groups || k0 % 4) { g_bad = 1; return; }
    for (int c = 0; c < 4; ++c) ++g_reads[((((size_t)g * g_D + d) * g_F + f) * g_T + t) * g_hw + cell + c];
}
static void visit_state(std::vector<int>& seen, long long at) {
    if (!g_visit) return;
    if (at < 0 || at + 4 > (long long)seen.size()) { g_bad = 1; return; }
    for (int c = 0; c < 4; ++c) ++seen[(size_t)at + c];
}
#define SP_VISIT_READ(d, f, k0, t, cell) visit_read(d, f, k0, t, cell)
#define SP_VISIT_STATE_LOAD(at) visit_state(g_loads, at)
#define SP_VISIT_STATE_STORE(at) visit_state(g_stores, at)
#include "spells_core.h"
using namespace spells;

struct Tables {
    int* state;
    long long *hist, *onsets, *invalid;
};

// what c2w_spell_update does with one dense block: a launch per threshold group, a workgroup per (row, variable, chunk)
static void update(const float* x, const float* y, const float* thr, const int* dir, Tables tb, int M, int T, int F, int hw, int K, int lmax, int period,
                   long long t0) {
    if (T == 0) return;
    std::vector<int> lds(LDS_INTS);
    View v{};
    v.x = x, v.y = y, v.thr = thr, v.dir = dir, v.state = tb.state, v.hist = tb.hist, v.onsets = period ? tb.onsets : nullptr, v.invalid = tb.invalid;
    v.D = M + (y ? 1 : 0), v.T = T, v.F = F, v.hw = hw, v.K = K, v.lmax = lmax, v.period = period, v.phase0 = period ? (int)(t0 % period) : 0;
    v.lds = lds.data();
    for (int g = 0; g < groups(K); ++g) {
        v.k0 = g * GROUP, v.kn = group_size(K, g);
        for (v.d = 0; v.d < v.D; ++v.d)
            for (v.f = 0; v.f < F; ++v.f)
                for (v.chunk = 0; v.chunk < chunks(hw); ++v.chunk) {
                    poison(v.lds, LDS_INTS, 0x55555555);
                    PHASE(s_zero(v, t))
                    PHASE(s_walk(v, t))
                    PHASE(s_flush(v, t))
                }
    }
}

// times [a, b) of rows [n][T][F hw] as a dense block [n][b - a][F hw]
static float* block_of(const float* src, int n, int T, size_t plane, int a, int b) {
    float* p = alloc16<float>((size_t)n * (b - a) * plane + 4);
    for (int m = 0; m < n; ++m) memcpy(p + (size_t)m * (b - a) * plane, src + ((size_t)m * T + a) * plane, (size_t)(b - a) * plane * sizeof(float));
    return p;
}

static int run(char** a, bool visit) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), K = atoi(a[4]), lmax = atoi(a[5]), period = atoi(a[6]);
    const long long t0 = visit ? 3 : atoll(a[7]);
    const int has_truth = atoi(a[visit ? 7 : 8]), split = visit ? 0 : atoi(a[9]);
    if (!supported(hw, K, lmax, period) || M < 1 || T < 1 || T > MAX_T || F < 1 || split < 0 || split > T) return 3;
    const int D = M + (has_truth ? 1 : 0);
    const size_t plane = (size_t)F * hw, ny = (size_t)T * plane, nx = (size_t)M * ny, ns = (size_t)4 * D * F * K * hw;
    float *x, *y, *thr;
    int* dir;
    if (visit) {
        x = alloc16<float>(nx), y = alloc16<float>(ny), thr = alloc16<float>((size_t)F * K), dir = alloc16<int>((size_t)F * K);
        for (size_t i = 0; i < nx; ++i) x[i] = (float)((i / plane * 7u + i % plane) % 23u);
        for (size_t i = 0; i < ny; ++i) y[i] = (float)((i / plane * 5u + i % plane) % 19u);
        for (int i = 0; i < F * K; ++i) thr[i] = 4.f + (float)(i % 9), dir[i] = i % 2;
    } else {
        x = read_file<float>(a[10], nx), y = read_file<float>(a[11], ny), thr = read_file<float>(a[12], (size_t)F * K), dir = read_file<int>(a[13], (size_t)F * K);
    }
    int* state = alloc16<int>(ns);
    memset(state, 0, ns * sizeof(int));
    std::vector<long long> hist((size_t)D * F * K * lmax, 0), onsets((size_t)D * F * K * period + 1, 0), invalid((size_t)D * F, 0);
    Tables tb{state, hist.data(), onsets.data(), invalid.data()};
    g_visit = visit, g_D = D, g_T = T, g_F = F, g_hw = hw, g_groups = groups(K);
    if (visit) g_reads.assign((size_t)g_groups * D * F * T * hw, 0), g_loads.assign(ns, 0), g_stores.assign(ns, 0);
    if (split == 0 || split == T) {
        update(x, has_truth ? y : nullptr, thr, dir, tb, M, T, F, hw, K, lmax, period, t0);
    } else {
        const int cut[3] = {0, split, T};
        for (int b = 0; b < 2; ++b) {
            float *xb = block_of(x, M, T, plane, cut[b], cut[b + 1]), *yb = block_of(y, 1, T, plane, cut[b], cut[b + 1]);
            update(xb, has_truth ? yb : nullptr, thr, dir, tb, M, cut[b + 1] - cut[b], F, hw, K, lmax, period, t0 + cut[b]);
            free(xb), free(yb);
        }
    }
    int rc = g_bad ? 8 : 0;
    if (visit && !rc) {
        for (int c : g_reads)
            if (c != 1) rc = 5;  // every cell-hour of every row once per threshold group
        for (size_t i = 0; i < ns && !rc; ++i)
            if (g_loads[i] != 1 || g_stores[i] != 1) rc = 6;  // every state entry loaded once and stored once
        long long spells = 0, begun = 0, hours = 0, open = 0;
        for (long long h : hist) spells += h;
        for (long long o : onsets) begun += o;  // the entry behind the table stays 0
        const size_t each = ns / 4;
        long long ended = 0;
        for (size_t i = 0; i < each; ++i) open += state[i] > 0 ? 1 : 0, ended += state[2 * each + i], hours += state[3 * each + i];
        if (!rc && (spells != ended || (period && begun != ended + open) || hours <= 0)) rc = 7;  // the bins, the counters and the onsets agree
    } else if (!rc) {
        rc = write_file(a[14], state, ns);
        if (!rc) rc = write_file(a[15], hist.data(), hist.size());
        if (!rc) rc = write_file(a[16], onsets.data(), onsets.size() - 1);
        if (!rc) rc = write_file(a[17], invalid.data(), invalid.size());
    }
    free(x), free(y), free(thr), free(dir), free(state);
    return rc;
}

// event_flipped is event_of: every pair of the special values, both directions
static int check_indicator() {
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    const float vals[] = {0.f, -0.f, 1.f, -1.f, 1.5f, -1.5f, 1e-45f, -1e-45f, 3.4028235e38f, -3.4028235e38f, inf, -inf, nan, -nan, 100000.f, 100000.01f};
    for (float a : vals)
        for (float t : vals)
            for (int above = 0; above < 2; ++above)
                if (event_flipped(a, flipped(t, flip_of(above)), flip_of(above)) != event_of(a, t, above)) return 9;
    return 0;
}

int main(int argc, char** argv) {
    if (int rc = check_indicator()) return rc;
    if (argc == 20 && !strcmp(argv[1], "update")) return run(argv + 2, false);
    if (argc == 10 && !strcmp(argv[1], "visit")) return run(argv + 2, true);
    return 1;
}
