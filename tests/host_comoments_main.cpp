// Host driver for csrc/comoments_maps.h: runs the phases of comoments_update_kernel one thread after the other, workgroup by
// workgroup (tests/test_dependence_cpu.py: the index maps and the arithmetic of csrc/comoments.hip without a GPU).
//   host_comoments update M T F hw has_truth cuts x.f32 y.f32 n.i32 pivot.f32 tpivot.f32 sums.f64 invalid.i64
//   host_comoments visit M T F hw has_truth
// update reads x [M][T][F][hw] and y [T][F][hw], starts from a zeroed state and takes the T hours in the calls that `cuts` says: bit i
// set is a cut behind hour i (T <= 31), each call repacked densely as a caller would hand it over; cuts = -1 runs EVERY cut and holds
// each against the single call bit for bit (exit code 10).  Every run is held, bit for bit, against a straight-line restatement of the
// definition below -- one series after the other, an invalid hour SKIPPED, not walked with the pivot (exit code 11) -- and the single
// call's tables are written.  visit counts, through the CM_VISIT_* hooks, that every (row, cell, hour) is read exactly once and every
// entry of the state (n, pivots, sums) loaded once and stored once.  Before anything else main holds the support function against
// its refusal rows and the layout against its closed forms.  It has its own main, so it is built with -fsanitize=address,undefined
// and run directly.
#include "host_main.h"

static bool g_visit = false;
static int g_bad = 0, g_D = 0, g_T = 0, g_hw = 0;
static std::vector<int> g_reads, g_loads[4], g_stores[4];
static void visit_read(int d, int t, int cell, int cells) {
    if (!g_visit) return;
    if (d < 0 || d >= g_D || t < 0 || t >= g_T || cell < 0 || cell + cells > g_hw) { g_bad = 1; return; }
    for (int c = 0; c < cells; ++c) ++g_reads[((size_t)d * g_T + t) * g_hw + cell + c];
}
static void visit_span(std::vector<int>& seen, long long at, int cells) {
    if (!g_visit) return;
    if (at < 0 || at + cells > (long long)seen.size()) { g_bad = 1; return; }
    for (int c = 0; c < cells; ++c) ++seen[(size_t)at + c];
}
#define CM_VISIT_READ(d, t, cell, cells) visit_read(d, t, cell, cells)
#define CM_VISIT_LOAD(what, at, cells) visit_span(g_loads[what], at, cells)
#define CM_VISIT_STORE(what, at, cells) visit_span(g_stores[what], at, cells)
#include "comoments_maps.h"
using namespace comoments;

struct State {
    std::vector<int> n;
    std::vector<float> pivot, truth_pivot;
    std::vector<double> sums;
    std::vector<long long> invalid;
    bool operator==(const State& o) const {
        return n == o.n && invalid == o.invalid && same(pivot, o.pivot) && same(truth_pivot, o.truth_pivot) && same(sums, o.sums);
    }
    template <typename E>
    static bool same(const std::vector<E>& a, const std::vector<E>& b) {  // as bits: a NaN equals itself, -0.0 is not +0.0
        return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(E)));
    }
};

// the state lives in 16-byte aligned buffers while the phases run, as the launcher demands of its caller
struct Buffers {
    int* n;
    float *pivot, *truth_pivot;
    double* sums;
    size_t nn, np, ns;
    Buffers(int D, int F, int hw, bool truth) : nn((size_t)D * hw), np((size_t)D * F * hw), ns((size_t)D * entries(F, truth) * hw) {
        n = alloc16<int>(nn), pivot = alloc16<float>(np), truth_pivot = alloc16<float>(np), sums = alloc16<double>(ns);
        memset(n, 0, nn * 4), memset(pivot, 0, np * 4), memset(truth_pivot, 0, np * 4), memset(sums, 0, ns * 8);
    }
    ~Buffers() { free(n), free(pivot), free(truth_pivot), free(sums); }
};

// what c2w_comoments_update does with one dense call: a workgroup per (row, chunk)
static void update(const float* x, const float* y, Buffers& b, long long* invalid, int M, int T, int F, int hw) {
    if (T == 0) return;
    int lds[1];
    View v{};
    v.x = x, v.y = y, v.n = b.n, v.pivot = b.pivot, v.truth_pivot = y ? b.truth_pivot : nullptr, v.sums = b.sums, v.invalid = invalid;
    v.D = M + (y ? 1 : 0), v.T = T, v.hw = hw, v.lds = lds;
    by_variables(F, [&](auto vars) {
        constexpr int NF = vars.i;
        for (v.d = 0; v.d < v.D; ++v.d)
            for (v.chunk = 0; v.chunk < chunks(hw, NF); ++v.chunk) {
                poison(v.lds, 1, 0x55555555);
                PHASE(u_zero(v, t))
                if (y) { PHASE((u_walk<NF, true>(v, t))) } else { PHASE((u_walk<NF, false>(v, t))) }
                PHASE(u_flush(v, t))
            }
    });
}

// hours [a, b) of rows [n][T][F hw] as a dense call [n][b - a][F hw]
static float* call_of(const float* src, int n, int T, size_t plane, int a, int b) {
    float* p = alloc16<float>((size_t)n * (b - a) * plane + 4);
    for (int m = 0; m < n; ++m) memcpy(p + (size_t)m * (b - a) * plane, src + ((size_t)m * T + a) * plane, (size_t)(b - a) * plane * sizeof(float));
    return p;
}

static State run_cuts(const float* x, const float* y, int M, int T, int F, int hw, int has_truth, unsigned cuts) {
    const int D = M + (has_truth ? 1 : 0);
    const size_t plane = (size_t)F * hw;
    Buffers b(D, F, hw, has_truth != 0);
    State r;
    r.invalid.assign((size_t)D, 0);
    int a = 0;
    for (int t = 1; t <= T; ++t) {
        if (t < T && !((cuts >> (t - 1)) & 1u)) continue;
        float *xb = call_of(x, M, T, plane, a, t), *yb = call_of(y, 1, T, plane, a, t);
        update(xb, has_truth ? yb : nullptr, b, r.invalid.data(), M, t - a, F, hw);
        free(xb), free(yb);
        a = t;
    }
    r.n.assign(b.n, b.n + b.nn), r.pivot.assign(b.pivot, b.pivot + b.np), r.sums.assign(b.sums, b.sums + b.ns);
    if (has_truth) r.truth_pivot.assign(b.truth_pivot, b.truth_pivot + b.np);
    return r;
}

static bool finite32(float v) {
    unsigned u;
    memcpy(&u, &v, 4);
    return (u >> 23 & 0xFFu) != 0xFFu;
}

// the definition, one series after the other; F is a run-time number here and an invalid hour is skipped
static State straight(const float* x, const float* y, int M, int T, int F, int hw, int has_truth) {
    const int D = M + (has_truth ? 1 : 0), NP = F * (F + 1) / 2, NS = F + NP + (has_truth ? 3 * F : 0);
    State r;
    r.n.assign((size_t)D * hw, 0), r.pivot.assign((size_t)D * F * hw, 0.f), r.sums.assign((size_t)D * NS * hw, 0.0), r.invalid.assign((size_t)D, 0);
    if (has_truth) r.truth_pivot.assign((size_t)D * F * hw, 0.f);
    for (int d = 0; d < D; ++d)
        for (int c = 0; c < hw; ++c) {
            const float* row = has_truth ? (d == 0 ? y : x + (size_t)(d - 1) * T * F * hw) : x + (size_t)d * T * F * hw;
            int n = 0;
            std::vector<double> s((size_t)NS, 0.0), e((size_t)F), eT((size_t)F);
            std::vector<float> P((size_t)F, 0.f), PT((size_t)F, 0.f);
            for (int t = 0; t < T; ++t) {
                bool valid = true;
                for (int f = 0; f < F; ++f) {
                    valid = valid && finite32(row[((size_t)t * F + f) * hw + c]);
                    if (has_truth) valid = valid && finite32(y[((size_t)t * F + f) * hw + c]);
                }
                if (!valid) {
                    ++r.invalid[(size_t)d];
                    continue;
                }
                for (int f = 0; f < F; ++f) {
                    const float xv = row[((size_t)t * F + f) * hw + c], yv = has_truth ? y[((size_t)t * F + f) * hw + c] : 0.f;
                    if (n == 0) P[(size_t)f] = xv, PT[(size_t)f] = yv;
                    e[(size_t)f] = (double)xv - (double)P[(size_t)f], eT[(size_t)f] = (double)yv - (double)PT[(size_t)f];
                }
                ++n;
                int k = 0;
                for (int f = 0; f < F; ++f, ++k) s[(size_t)k] = s[(size_t)k] + e[(size_t)f];
                for (int f = 0; f < F; ++f)
                    for (int g = f; g < F; ++g, ++k) {
                        const double term = e[(size_t)f] * e[(size_t)g];
                        s[(size_t)k] = s[(size_t)k] + term;
                    }
                if (has_truth) {
                    for (int f = 0; f < F; ++f, ++k) s[(size_t)k] = s[(size_t)k] + eT[(size_t)f];
                    for (int f = 0; f < F; ++f, ++k) {
                        const double term = eT[(size_t)f] * eT[(size_t)f];
                        s[(size_t)k] = s[(size_t)k] + term;
                    }
                    for (int f = 0; f < F; ++f, ++k) {
                        const double term = e[(size_t)f] * eT[(size_t)f];
                        s[(size_t)k] = s[(size_t)k] + term;
                    }
                }
            }
            r.n[(size_t)d * hw + c] = n;
            for (int f = 0; f < F; ++f) {
                r.pivot[((size_t)d * F + f) * hw + c] = P[(size_t)f];
                if (has_truth) r.truth_pivot[((size_t)d * F + f) * hw + c] = PT[(size_t)f];
            }
            for (int k = 0; k < NS; ++k) r.sums[((size_t)d * NS + k) * hw + c] = s[(size_t)k];
        }
    return r;
}

static int run_update(char** a) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), has_truth = atoi(a[4]);
    const long long cuts = atoll(a[5]);
    if (!supported(hw, F) || M < 1 || T < 1 || T > 31) return 3;
    const size_t plane = (size_t)F * hw, ny = (size_t)T * plane, nx = (size_t)M * ny;
    float *x = read_file<float>(a[6], nx), *y = read_file<float>(a[7], ny);
    int rc = 0;
    const State want = straight(x, y, M, T, F, hw, has_truth);
    State one = run_cuts(x, y, M, T, F, hw, has_truth, cuts == -1 ? 0u : (unsigned)cuts);
    if (!(one == want)) rc = 11;
    if (cuts == -1)
        for (unsigned c = 1; c < (1u << (T - 1)) && !rc; ++c)
            if (!(run_cuts(x, y, M, T, F, hw, has_truth, c) == one)) rc = 10;
    if (!rc) rc = write_file(a[8], one.n);
    if (!rc) rc = write_file(a[9], one.pivot);
    if (!rc) rc = write_file(a[10], one.truth_pivot);
    if (!rc) rc = write_file(a[11], one.sums);
    if (!rc) rc = write_file(a[12], one.invalid);
    free(x), free(y);
    return rc;
}

static int run_visit(char** a) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), has_truth = atoi(a[4]);
    if (!supported(hw, F) || M < 1 || T < 1 || T > MAX_T) return 3;
    const int D = M + (has_truth ? 1 : 0), NS = entries(F, has_truth != 0);
    const size_t plane = (size_t)F * hw, ny = (size_t)T * plane, nx = (size_t)M * ny;
    float *x = alloc16<float>(nx), *y = alloc16<float>(ny);
    for (size_t i = 0; i < nx; ++i) x[i] = i % 29u == 7u ? NAN : (float)((i / plane * 7u + i % plane) % 23u);
    for (size_t i = 0; i < ny; ++i) y[i] = i % 31u == 3u ? INFINITY : (float)((i / plane * 5u + i % plane) % 19u);
    g_visit = true, g_D = D, g_T = T, g_hw = hw;
    g_reads.assign((size_t)D * T * hw, 0);
    const size_t sizes[4] = {(size_t)D * hw, (size_t)D * F * hw, (size_t)D * F * hw, (size_t)D * NS * hw};
    for (int w = 0; w < 4; ++w) g_loads[w].assign(sizes[w], 0), g_stores[w].assign(sizes[w], 0);
    const State r = run_cuts(x, y, M, T, F, hw, has_truth, 0u);
    g_visit = false;
    int rc = g_bad ? 8 : 0;
    for (int c : g_reads)
        if (c != 1 && !rc) rc = 5;  // every cell-hour of every row once
    for (int w = 0; w < 4 && !rc; ++w) {
        const int want = w == 2 && !has_truth ? 0 : 1;  // the truth's pivots are not touched without a truth
        for (size_t i = 0; i < sizes[w] && !rc; ++i)
            if (g_loads[w][i] != want || g_stores[w][i] != want) rc = 6;  // every entry of the state loaded once and stored once
    }
    if (!rc && !(r == straight(x, y, M, T, F, hw, has_truth))) rc = 11;
    free(x), free(y);
    return rc;
}

// the refusal rows of the launcher's shape checks, and the layout against its closed forms
static int check_maps() {
    const int bad_hw[] = {-4, 0, 1, 2, 3, 5, 6, 7, 9, 1026};
    for (int hw : bad_hw)
        if (supported(hw, 1)) return 9;
    const int good_hw[] = {4, 8, 1024, 1028, 16384};
    for (int hw : good_hw)
        for (int F = -1; F <= 10; ++F)
            if (supported(hw, F) != (F >= 1 && F <= 8)) return 9;
    for (int F = 1; F <= MAX_F; ++F) {
        const int V = cells_per_thread(F);
        if ((V != 1 && V != 2 && V != 4) || chunk_cells(F) != THREADS * V) return 9;
        if (entries(F, true) != 4 * F + F * (F + 1) / 2 || entries(F, false) != F + F * (F + 1) / 2) return 9;
        if (at_S(F) != 0 || at_C(F) != F || at_ST(F) != at_C(F) + pairs(F) || at_QT(F) != at_ST(F) + F || at_X(F) != at_QT(F) + F) return 9;
        if (at_X(F) + F != entries(F, true) || at_ST(F) != entries(F, false)) return 9;
        if (chunks(4, F) != 1 || chunks(chunk_cells(F), F) != 1 || chunks(chunk_cells(F) + 4, F) != 2) return 9;
        if (cell_of(1, 0, F) != chunk_cells(F) || cell_of(0, 1, F) != V) return 9;
    }
    const float inf = INFINITY;
    if (finite_bits(inf) || finite_bits(-inf) || finite_bits(NAN) || finite_bits(-NAN) || !finite_bits(0.f) || !finite_bits(-0.f)) return 9;
    if (!finite_bits(3.4e38f) || !finite_bits(1e-45f)) return 9;
    return 0;
}

int main(int argc, char** argv) {
    if (int rc = check_maps()) return rc;
    if (argc == 15 && !strcmp(argv[1], "update")) return run_update(argv + 2);
    if (argc == 7 && !strcmp(argv[1], "visit")) return run_visit(argv + 2);
    return 1;
}
