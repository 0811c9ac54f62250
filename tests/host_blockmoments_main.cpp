// Host driver for csrc/blockmoments_maps.h: runs the phases of block_moments_kernel one thread after the other, workgroup by workgroup
// (tests/test_scalesplit_cpu.py: the index maps and the arithmetic of csrc/blockmoments.hip without a GPU).
//   host_blockmoments run M T F H W s has_truth x.f32 y.f32 n.i32 pivot.f32 sums.f64
//   host_blockmoments visit M T F H W s has_truth
// run reads x [M][T][F][H][W] and y [T][F][H][W], runs what c2w_block_moments launches into tables poisoned beforehand, holds them,
// bit for bit, against a straight-line restatement of the definition below -- one block after the other, S a run-time number (exit
// code 11) -- and writes them.  visit counts, through the BM_VISIT_* hooks, that every cell of every row's planes is read exactly once
// as the row's own and every block's outputs are stored exactly once.  Before anything else main holds the support function against
// its refusal rows and the maps against their closed forms.  It has its own main, so it is built with -fsanitize=address,undefined and
// run directly.
#include "host_main.h"

static bool g_visit = false;
static int g_bad = 0, g_D = 0, g_planes = 0;
static long long g_hw = 0, g_blocks = 0;
static std::vector<int> g_reads, g_stores;
static void visit_read(int d, int plane, long long at) {
    if (!g_visit) return;
    if (d < 0 || d >= g_D || plane < 0 || plane >= g_planes || at < 0 || at + 4 > g_hw) { g_bad = 1; return; }
    for (int c = 0; c < 4; ++c) ++g_reads[((size_t)d * g_planes + plane) * g_hw + at + c];
}
static void visit_store(int d, int plane, long long block) {
    if (!g_visit) return;
    if (d < 0 || d >= g_D || plane < 0 || plane >= g_planes || block < 0 || block >= g_blocks) { g_bad = 1; return; }
    ++g_stores[((size_t)d * g_planes + plane) * g_blocks + block];
}
#define BM_VISIT_READ(d, plane, at) visit_read(d, plane, at)
#define BM_VISIT_STORE(d, plane, block) visit_store(d, plane, block)
#include "blockmoments_maps.h"
using namespace blockmoments;

struct Tables {
    std::vector<int> n;
    std::vector<float> pivot;
    std::vector<double> sums;
    bool operator==(const Tables& o) const { return n == o.n && same(pivot, o.pivot) && same(sums, o.sums); }
    template <typename E>
    static bool same(const std::vector<E>& a, const std::vector<E>& b) {  // as bits: a NaN equals itself, -0.0 is not +0.0
        return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(E)));
    }
};

// what c2w_block_moments does with one call: a workgroup per (row, 256 consecutive items)
static Tables launch(const float* x, const float* y, int M, int T, int F, int H, int W, int s) {
    const int D = M + (y ? 1 : 0), NS = entries(y != nullptr), planes = T * F;
    const size_t cells = (size_t)D * planes * (H / s) * (W / s);
    Tables r;
    r.n.assign(cells, 0x55555555), r.pivot.assign(cells, -7.f), r.sums.assign(cells * NS, -7.0);  // every element is written
    std::vector<double> lds_sums((size_t)3 * 4 * THREADS);
    std::vector<int> lds_count((size_t)2 * THREADS);
    View v{};
    v.x = x, v.y = y, v.n = r.n.data(), v.pivot = r.pivot.data(), v.sums = r.sums.data();
    v.planes = planes, v.items = (int)row_items(planes, H, W, s), v.H = H, v.W = W;
    v.lds_sums = lds_sums.data(), v.lds_count = lds_count.data();
    by_size(s, [&](auto size) {
        constexpr int S = size.i;
        for (v.d = 0; v.d < D; ++v.d)
            for (v.chunk = 0; v.chunk < (int)chunks(v.items); ++v.chunk) {
                poison(v.lds_sums, lds_sums.size(), (double)NAN);
                poison(v.lds_count, lds_count.size(), 0x55555555);
                if (y) { PHASE((b_walk<S, true>(v, t))) PHASE((b_fold<S, true>(v, t))) }
                else { PHASE((b_walk<S, false>(v, t))) PHASE((b_fold<S, false>(v, t))) }
            }
    });
    return r;
}

static bool finite32(float v) {
    unsigned u;
    memcpy(&u, &v, 4);
    return (u >> 23 & 0xFFu) != 0xFFu;
}

// the definition, one block after the other
static Tables straight(const float* x, const float* y, int M, int T, int F, int H, int W, int s) {
    const int D = M + (y ? 1 : 0), NS = y ? 3 : 2, planes = T * F, h = H / s, w = W / s;
    const size_t hw = (size_t)H * W, cells = (size_t)h * w;
    const unsigned long long nan_bits = 0x7ff8000000000000ull;
    double nan;
    memcpy(&nan, &nan_bits, 8);
    Tables r;
    r.n.assign((size_t)D * planes * cells, 0), r.pivot.assign((size_t)D * planes * cells, 0.f), r.sums.assign((size_t)D * planes * NS * cells, 0.0);
    for (int d = 0; d < D; ++d)
        for (int p = 0; p < planes; ++p)
            for (int i = 0; i < h; ++i)
                for (int j = 0; j < w; ++j) {
                    const float* row = (y ? (d == 0 ? y : x + (size_t)(d - 1) * planes * hw) : x + (size_t)d * planes * hw) + p * hw + (size_t)i * s * W + (size_t)j * s;
                    const float* tru = y ? y + p * hw + (size_t)i * s * W + (size_t)j * s : row;
                    const float P = row[0], PT = tru[0];
                    int n = 0, nt = 0;
                    double S1 = 0.0, S2 = 0.0, X = 0.0;
                    for (int c = 0; c < s; ++c) {
                        double A = 0.0, Q = 0.0, XC = 0.0;
                        for (int q = 0; q < s; ++q) {
                            const float xv = row[(size_t)q * W + c], yv = tru[(size_t)q * W + c];
                            n += finite32(xv), nt += finite32(yv);
                            const double e = (double)xv - (double)P, eT = (double)yv - (double)PT;
                            const double ee = e * e, et = e * eT;
                            A = A + e, Q = Q + ee, XC = XC + et;
                        }
                        S1 = S1 + A, S2 = S2 + Q, X = X + XC;
                    }
                    const size_t at = ((size_t)d * planes + p) * cells + (size_t)i * w + j, at_s = ((size_t)d * planes + p) * NS * cells + (size_t)i * w + j;
                    r.n[at] = n, r.pivot[at] = P;
                    r.sums[at_s] = n == s * s ? S1 : nan, r.sums[at_s + cells] = n == s * s ? S2 : nan;
                    if (y) r.sums[at_s + 2 * cells] = n == s * s && nt == s * s ? X : nan;
                }
    return r;
}

static bool shape_ok(int M, int T, int F, int H, int W, int s) {
    return supported(H, W, s) && M >= 1 && T >= 1 && F >= 1 && row_items((long long)T * F, H, W, s) < (1 << 24);
}

static int run_tables(char** a) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), H = atoi(a[3]), W = atoi(a[4]), s = atoi(a[5]), has_truth = atoi(a[6]);
    if (!shape_ok(M, T, F, H, W, s)) return 3;
    const size_t ny = (size_t)T * F * H * W, nx = (size_t)M * ny;
    float *x = read_file<float>(a[7], nx), *y = read_file<float>(a[8], ny);
    const Tables got = launch(x, has_truth ? y : nullptr, M, T, F, H, W, s);
    int rc = got == straight(x, has_truth ? y : nullptr, M, T, F, H, W, s) ? 0 : 11;
    if (!rc) rc = write_file(a[9], got.n);
    if (!rc) rc = write_file(a[10], got.pivot);
    if (!rc) rc = write_file(a[11], got.sums);
    free(x), free(y);
    return rc;
}

static int run_visit(char** a) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), H = atoi(a[3]), W = atoi(a[4]), s = atoi(a[5]), has_truth = atoi(a[6]);
    if (!shape_ok(M, T, F, H, W, s)) return 3;
    const size_t ny = (size_t)T * F * H * W, nx = (size_t)M * ny;
    float *x = alloc16<float>(nx), *y = alloc16<float>(ny);
    for (size_t i = 0; i < nx; ++i) x[i] = i % 291u == 7u ? NAN : (float)((i / 13u * 7u + i) % 23u);
    for (size_t i = 0; i < ny; ++i) y[i] = i % 311u == 3u ? INFINITY : (float)((i / 11u * 5u + i) % 19u);
    g_visit = true, g_D = M + (has_truth ? 1 : 0), g_planes = T * F, g_hw = (long long)H * W, g_blocks = (long long)(H / s) * (W / s);
    g_reads.assign((size_t)g_D * g_planes * g_hw, 0), g_stores.assign((size_t)g_D * g_planes * g_blocks, 0);
    const Tables got = launch(x, has_truth ? y : nullptr, M, T, F, H, W, s);
    g_visit = false;
    int rc = g_bad ? 8 : 0;
    for (int c : g_reads)
        if (c != 1 && !rc) rc = 5;  // every cell of every row once
    for (int c : g_stores)
        if (c != 1 && !rc) rc = 6;  // every block's outputs once
    if (!rc && !(got == straight(x, has_truth ? y : nullptr, M, T, F, H, W, s))) rc = 11;
    free(x), free(y);
    return rc;
}

// the refusal rows of the launcher's shape checks, and the maps against their closed forms
static int check_maps() {
    for (int s = -1; s <= 70; ++s)
        if (supported(64, 64, s) != (s == 4 || s == 8 || s == 16 || s == 32)) return 9;
    if (supported(20, 16, 8) || supported(16, 20, 8) || supported(0, 16, 4) || supported(16, 0, 4) || supported(4, 4, 8) || supported(-8, 8, 8)) return 9;
    if (!supported(4, 4, 4) || !supported(8, 516, 4) || !supported(16, 24, 8) || !supported(64, 96, 32)) return 9;
    if (entries(true) != 3 || entries(false) != 2 || group_rows(4) != 4 || group_rows(8) != 8 || group_rows(32) != 8) return 9;
    if (items_per_plane(8, 516, 4) != 2 * 129 || row_items(3, 8, 516, 4) != 3 * 258 || chunks(256) != 1 || chunks(257) != 2 || chunks(1) != 1) return 9;
    if (bound_rounds(16, false) != 32 || bound_rounds(16, true) != 34) return 9;
    for (int s = 4; s <= 32; s *= 2)
        if (THREADS % (s / 4) || s % group_rows(s)) return 9;  // no block straddles a workgroup; the groups tile the rows
    const float inf = INFINITY;
    if (finite_bits(inf) || finite_bits(-inf) || finite_bits(NAN) || finite_bits(-NAN) || !finite_bits(0.f) || !finite_bits(-0.f)) return 9;
    if (!finite_bits(3.4e38f) || !finite_bits(1e-45f)) return 9;
    return 0;
}

int main(int argc, char** argv) {
    if (int rc = check_maps()) return rc;
    if (argc == 14 && !strcmp(argv[1], "run")) return run_tables(argv + 2);
    if (argc == 9 && !strcmp(argv[1], "visit")) return run_visit(argv + 2);
    return 1;
}
