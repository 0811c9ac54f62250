// Host driver for csrc/extremes_maps.h: runs the phases of block_extremes_kernel and of lmoments_kernel one thread after the other,
// workgroup by workgroup (tests/test_extremes_cpu.py: the index maps and the arithmetic of csrc/extremes.hip without a GPU).
//   host_extremes update M T F hw block B has_truth cuts x.f32 y.f32 dir.i32 table.f32 open.u32 invalid.i64
//   host_extremes visit M T F hw block B has_truth t0
//   host_extremes lmoments R n hw table.f32 lmom.f64 nvalid.i32
//   host_extremes lvisit R n hw
// update reads x [M][T][F][hw] and y [T][F][hw], starts from "no value yet" keys, a table full of a sentinel and zeroed counters, and
// takes the T hours in the calls that `cuts` says: bit i set is a cut behind hour i (T <= 31), each call repacked densely as a caller
// would hand it over; cuts = -1 runs EVERY cut, holds each against the single call bit for bit (exit code 10) and writes the single
// call's tables.  visit counts, through the EX_VISIT_* hooks, that every (row, variable, cell, hour) is read exactly once, every table
// entry of a block that ends in the call written exactly once and no other, every open key loaded and stored once.  lvisit counts
// that every block extreme is read exactly once as one of the n rows, that the clamped loads behind them stay inside the row, and that
// every output is written.  Before anything else main holds "no value yet" against every special value.  It has its own main, so it is
// built with -fsanitize=address,undefined and run directly.
#include "host_main.h"

static bool g_visit = false;
static int g_bad = 0, g_D = 0, g_T = 0, g_F = 0, g_hw = 0;
static std::vector<int> g_reads, g_table, g_loads, g_stores, g_used, g_clamped;
static void visit_read(int d, int f, int t, int cell) {
    if (!g_visit) return;
    if (d < 0 || d >= g_D || f < 0 || f >= g_F || t < 0 || t >= g_T || cell < 0 || cell + 4 > g_hw) { g_bad = 1; return; }
    for (int c = 0; c < 4; ++c) ++g_reads[(((size_t)d * g_F + f) * g_T + t) * g_hw + cell + c];
}
static void visit_span(std::vector<int>& seen, long long at, int cells) {
    if (!g_visit) return;
    if (at < 0 || at + cells > (long long)seen.size()) { g_bad = 1; return; }
    for (int c = 0; c < cells; ++c) ++seen[(size_t)at + c];
}
#define EX_VISIT_READ(d, f, t, cell) visit_read(d, f, t, cell)
#define EX_VISIT_TABLE(at) visit_span(g_table, at, 4)
#define EX_VISIT_OPEN_LOAD(at) visit_span(g_loads, at, 4)
#define EX_VISIT_OPEN_STORE(at) visit_span(g_stores, at, 4)
#define EX_VISIT_TABLE_READ(at, cells, used) visit_span((used) ? g_used : g_clamped, at, cells)
#include "extremes_maps.h"
using namespace extremes;

static const unsigned SENTINEL = 0x12345678u;  // no extreme is this pattern in any test: an entry nobody wrote

struct Tables {
    unsigned* open;
    float* table;
    long long* invalid;
};

// what c2w_block_extremes_update does with one dense call: a workgroup per (row, variable, chunk)
static void update(const float* x, const float* y, const int* dir, Tables tb, int M, int T, int F, int hw, int block, int B, long long t0) {
    if (T == 0) return;
    int lds[1];
    BView v{};
    v.x = x, v.y = y, v.dir = dir, v.open = tb.open, v.table = tb.table, v.invalid = tb.invalid;
    v.D = M + (y ? 1 : 0), v.T = T, v.F = F, v.hw = hw, v.B = B, v.block = block, v.t0 = t0, v.lds = lds;
    for (v.d = 0; v.d < v.D; ++v.d)
        for (v.f = 0; v.f < F; ++v.f)
            for (v.chunk = 0; v.chunk < chunks(hw); ++v.chunk) {
                poison(v.lds, 1, 0x55555555);
                PHASE(b_zero(v, t))
                PHASE(b_walk(v, t))
                PHASE(b_flush(v, t))
            }
}

// hours [a, b) of rows [n][T][F hw] as a dense call [n][b - a][F hw]
static float* call_of(const float* src, int n, int T, size_t plane, int a, int b) {
    float* p = alloc16<float>((size_t)n * (b - a) * plane + 4);
    for (int m = 0; m < n; ++m) memcpy(p + (size_t)m * (b - a) * plane, src + ((size_t)m * T + a) * plane, (size_t)(b - a) * plane * sizeof(float));
    return p;
}

struct Result {
    std::vector<unsigned> open, table;
    std::vector<long long> invalid;
};

static Result run_cuts(const float* x, const float* y, const int* dir, int M, int T, int F, int hw, int block, int B, int has_truth, unsigned cuts,
                       long long t0) {
    const int D = M + (has_truth ? 1 : 0);
    const size_t plane = (size_t)F * hw, no = (size_t)D * F * hw, nt = no * B;
    unsigned* open = alloc16<unsigned>(no);
    float* table = alloc16<float>(nt);
    for (size_t i = 0; i < no; ++i) open[i] = NONE;
    for (size_t i = 0; i < nt; ++i) memcpy(table + i, &SENTINEL, 4);
    Result r;
    r.invalid.assign((size_t)D * F, 0);
    Tables tb{open, table, r.invalid.data()};
    int a = 0;
    for (int t = 1; t <= T; ++t) {
        if (t < T && !((cuts >> (t - 1)) & 1u)) continue;
        float *xb = call_of(x, M, T, plane, a, t), *yb = call_of(y, 1, T, plane, a, t);
        update(xb, has_truth ? yb : nullptr, dir, tb, M, t - a, F, hw, block, B, t0 + a);
        free(xb), free(yb);
        a = t;
    }
    r.open.assign(open, open + no);
    r.table.resize(nt);
    memcpy(r.table.data(), table, nt * 4);
    free(open), free(table);
    return r;
}

static int run_update(char** a, bool visit) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), block = atoi(a[4]), B = atoi(a[5]), has_truth = atoi(a[6]);
    const long long last = visit ? atoll(a[7]) : atoll(a[7]);  // visit: t0; update: cuts
    const long long t0 = visit ? last : 0;
    if (!update_supported(hw, block, B) || M < 1 || T < 1 || T > MAX_T || F < 1 || end_closed(t0, T, block) > B) return 3;
    const int D = M + (has_truth ? 1 : 0);
    const size_t plane = (size_t)F * hw, ny = (size_t)T * plane, nx = (size_t)M * ny;
    float *x, *y;
    int* dir;
    if (visit) {
        x = alloc16<float>(nx), y = alloc16<float>(ny), dir = alloc16<int>((size_t)F);
        for (size_t i = 0; i < nx; ++i) x[i] = (float)((i / plane * 7u + i % plane) % 23u);
        for (size_t i = 0; i < ny; ++i) y[i] = (float)((i / plane * 5u + i % plane) % 19u);
        for (int i = 0; i < F; ++i) dir[i] = i % 2;
    } else {
        if (T > 31) return 3;
        x = read_file<float>(a[8], nx), y = read_file<float>(a[9], ny), dir = read_file<int>(a[10], (size_t)F);
    }
    int rc = 0;
    if (visit) {
        const size_t no = (size_t)D * F * hw;
        g_visit = true, g_D = D, g_T = T, g_F = F, g_hw = hw;
        g_reads.assign((size_t)D * F * T * hw, 0), g_table.assign(no * B, 0), g_loads.assign(no, 0), g_stores.assign(no, 0);
        Result r = run_cuts(x, y, dir, M, T, F, hw, block, B, has_truth, 0u, t0);
        g_visit = false;
        rc = g_bad ? 8 : 0;
        for (int c : g_reads)
            if (c != 1 && !rc) rc = 5;  // every cell-hour of every row once
        for (size_t i = 0; i < no && !rc; ++i)
            if (g_loads[i] != 1 || g_stores[i] != 1) rc = 6;  // every open key loaded once and stored once
        const long long b0 = first_closed(t0, block), b1 = end_closed(t0, T, block);
        for (size_t i = 0; i < no * B && !rc; ++i) {
            const long long b = (long long)(i / hw % B);
            const int want = b >= b0 && b < b1 ? 1 : 0;  // a block that ends in the call exactly once, any other never
            if (g_table[i] != want || (r.table[i] == SENTINEL) != (want == 0)) rc = 7;
        }
    } else if ((int)last == -1) {
        Result one = run_cuts(x, y, dir, M, T, F, hw, block, B, has_truth, 0u, 0);
        for (unsigned cuts = 1; cuts < (1u << (T - 1)) && !rc; ++cuts) {
            Result r = run_cuts(x, y, dir, M, T, F, hw, block, B, has_truth, cuts, 0);
            if (r.open != one.open || r.table != one.table || r.invalid != one.invalid) rc = 10;
        }
        if (!rc) rc = write_file(a[11], one.table);
        if (!rc) rc = write_file(a[12], one.open);
        if (!rc) rc = write_file(a[13], one.invalid);
    } else {
        Result r = run_cuts(x, y, dir, M, T, F, hw, block, B, has_truth, (unsigned)last, 0);
        rc = write_file(a[11], r.table);
        if (!rc) rc = write_file(a[12], r.open);
        if (!rc) rc = write_file(a[13], r.invalid);
    }
    free(x), free(y), free(dir);
    return rc;
}

// what c2w_lmoments does: a workgroup per (row, chunk of 256 V cells)
static void moments(const float* table, double* lmom, int* n_valid, int R, int n, int hw) {
    by_rows(n, [&](auto rows) {
        constexpr int K = rows.i, V = V_OF<K>;
        LView v{};
        v.table = table, v.lmom = lmom, v.n_valid = n_valid, v.n = n, v.hw = hw;
        for (v.row = 0; v.row < R; ++v.row)
            for (v.chunk = 0; v.chunk < lchunks(hw, V); ++v.chunk) PHASE((l_cells<K, V>(v, t)))
    });
}

static int run_lmoments(char** a, bool visit) {
    const int R = atoi(a[0]), n = atoi(a[1]), hw = atoi(a[2]);
    if (!lmoments_supported(hw, n) || R < 1) return 3;
    const size_t nt = (size_t)R * n * hw, no = (size_t)R * hw;
    float* table;
    if (visit) {
        table = alloc16<float>(nt);
        for (size_t i = 0; i < nt; ++i) table[i] = (float)((i * 2654435761u) % 1009u) - 300.f;
    } else {
        table = read_file<float>(a[3], nt);
    }
    std::vector<double> lmom(no * 4, 12345.0);
    std::vector<int> n_valid(no, -7);
    g_visit = visit;
    if (visit) g_used.assign(nt, 0), g_clamped.assign(nt, 0);
    moments(table, lmom.data(), n_valid.data(), R, n, hw);
    g_visit = false;
    int rc = g_bad ? 8 : 0;
    if (visit) {
        for (int c : g_used)
            if (c != 1 && !rc) rc = 5;  // every block extreme once as one of the n rows
        for (size_t i = 0; i < nt && !rc; ++i)
            if (g_clamped[i] && i / hw % n != (size_t)n - 1) rc = 6;  // a load behind them asks for the last block again, nothing else
        for (size_t i = 0; i < no && !rc; ++i)
            if (n_valid[i] != n) rc = 7;  // every output written
        for (double l : lmom)
            if (l == 12345.0 && !rc) rc = 7;
    } else if (!rc) {
        rc = write_file(a[4], lmom);
        if (!rc) rc = write_file(a[5], n_valid);
    }
    free(table);
    return rc;
}

// "no value yet" is below the key of every value in both directions, a NaN has it, the keys keep the order and give the bits back
static int check_keys() {
    const unsigned vals[] = {0xFF800000u, 0xFF7FFFFFu, 0xC7C35000u, 0xBF800000u, 0x80800000u, 0x807FFFFFu, 0x80000001u, 0x80000000u, 0x00000000u,
                             0x00000001u, 0x007FFFFFu, 0x00800000u, 0x3F800000u, 0x47C35000u, 0x7F7FFFFFu, 0x7F800000u};  // ascending, -inf .. +inf
    const unsigned nans[] = {0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFF800001u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
    for (int maxima = 0; maxima < 2; ++maxima) {
        const unsigned flip = flip_of(maxima);
        for (int i = 0; i < nv; ++i) {
            if (dkey_of(vals[i], flip) <= NONE || extreme_bits(dkey_of(vals[i], flip), flip) != vals[i]) return 9;
            if (i && (maxima ? dkey_of(vals[i - 1], flip) >= dkey_of(vals[i], flip) : dkey_of(vals[i - 1], flip) <= dkey_of(vals[i], flip))) return 9;
        }
        for (unsigned b : nans)
            if (dkey_of(b, flip) != NONE) return 9;
        if (extreme_bits(NONE, flip) != NAN_BITS) return 9;
    }
    if (V_OF<8> != cells_per_thread(8) || V_OF<16> != cells_per_thread(16) || V_OF<32> != cells_per_thread(32) || V_OF<64> != cells_per_thread(64)) return 9;
    return 0;
}

int main(int argc, char** argv) {
    if (int rc = check_keys()) return rc;
    if (argc == 16 && !strcmp(argv[1], "update")) return run_update(argv + 2, false);
    if (argc == 10 && !strcmp(argv[1], "visit")) return run_update(argv + 2, true);
    if (argc == 8 && !strcmp(argv[1], "lmoments")) return run_lmoments(argv + 2, false);
    if (argc == 5 && !strcmp(argv[1], "lvisit")) return run_lmoments(argv + 2, true);
    return 1;
}
