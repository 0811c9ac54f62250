// Host driver for csrc/temporal_core.h: runs the phases of tincr_terms_kernel one thread after the other, workgroup by workgroup
// (tests/test_temporal_cpu.py: the index maps, the arithmetic and the fold order of csrc/temporal.hip without a GPU).
//   host_temporal terms n_rep with_truth T F hw L x.f32 y.f32 S.f64
//   host_temporal visit n_rep with_truth T F hw L
// `visit` counts, through TINCR_VISIT, how often every (cell, lag) of every anchor plane is taken up: exactly once where the lag has a
// pair, never where it has none; it also checks that every entry of the output and of the partial sums was written.  It has its own
// main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"

static std::vector<int>* g_visits = nullptr;  // [plane][lag - 1][cell]
static int g_hw = 0, g_L = 0;
static void visit4(long long plane, int cell, int tau) {
    if (!g_visits) return;
    for (int c = 0; c < 4; ++c) ++(*g_visits)[((size_t)plane * g_L + (tau - 1)) * g_hw + cell + c];
}
#define TINCR_VISIT(plane, cell, tau) visit4(plane, cell, tau)
#include "temporal_core.h"
using namespace tincr;

// one workgroup of tincr_terms_kernel<HAS_Y>
template <bool HAS_Y>
static void group(View& v) {
    poison(v.lds, LDS_DOUBLES, NAN);  // a slot nobody stashed that reaches a sum shows
    const int n = rounds(v.hw, v.chunk), np = passes(v.L);
    for (int pass = 0; pass < np; ++pass) {
        if (!pass_has_pairs(v, pass)) {
            PHASE(t_store(v, t, pass, false))
            continue;
        }
        std::vector<Thread> th(THREADS);
        PHASE(t_init(th[t]))
        for (int it = 0; it < n; ++it) PHASE(t_round<HAS_Y>(v, th[t], t, pass, it))
        PHASE(t_stash(v, th[t], t))
        PHASE(t_fold_groups(v, t))
        PHASE(t_store(v, t, pass, true))
    }
}

static int run(char** a, bool visit) {
    const int n_rep = atoi(a[0]), with_y = atoi(a[1]), T = atoi(a[2]), F = atoi(a[3]), hw = atoi(a[4]), L = atoi(a[5]);
    if (!supported(hw, L) || n_rep < 1 || T < 1 || F < 1) return 3;
    const size_t ny = (size_t)T * F * hw, nx = (size_t)n_rep * ny;
    float *x, *y = nullptr;
    if (visit) {
        x = alloc16<float>(nx), y = alloc16<float>(ny);
        for (size_t k = 0; k < nx; ++k) x[k] = (float)(k % 1021) * 0.25f;
        for (size_t k = 0; k < ny; ++k) y[k] = (float)(k % 1019) * 0.5f;
    } else {
        x = read_file<float>(a[6], nx);
        if (with_y) y = read_file<float>(a[7], ny);
    }
    const int nc = chunks(hw);
    const long long rows = n_rep + (with_y ? 1 : 0), planes = rows * T * F;
    std::vector<double> S((size_t)planes * L * 3, NAN), partial((size_t)(scratch_bytes(rows, T, F, hw, L) / 8), NAN), lds(LDS_DOUBLES);
    std::vector<int> visits(visit ? (size_t)planes * L * hw : 0, 0);
    g_visits = visit ? &visits : nullptr, g_hw = hw, g_L = L;
    View v{};
    v.x = x, v.y = with_y ? y : nullptr, v.out = nc > 1 ? partial.data() : S.data();
    v.T = T, v.F = F, v.hw = hw, v.L = L, v.lds = lds.data();
    for (v.plane = 0; v.plane < planes; ++v.plane)
        for (v.chunk = 0; v.chunk < nc; ++v.chunk) with_y ? group<true>(v) : group<false>(v);
    int rc = 0;
    if (visit)
        for (double p : partial)
            if (p != p) rc = 6;  // a partial nobody wrote (the inputs are finite, so no workgroup wrote NaN on purpose)
    if (nc > 1)
        for (long long e = 0; e < planes * L * 3; ++e) f_fold(partial.data(), S.data(), e, nc, L);
    if (visit) {
        for (double s : S)
            if (s != s) rc = rc ? rc : 7;  // an entry nobody wrote
        for (long long pl = 0; pl < planes && !rc; ++pl) {
            const int t = (int)((pl / F) % T);
            for (int tau = 1; tau <= L && !rc; ++tau)
                for (int c = 0; c < hw; ++c)
                    if (visits[((size_t)pl * L + (tau - 1)) * hw + c] != (t + tau < T ? 1 : 0)) {
                        rc = 5;
                        break;
                    }
        }
    } else if (!rc) {
        rc = write_file(a[8], S);
    }
    free(x), free(y);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 11 && !strcmp(argv[1], "terms")) return run(argv + 2, false);
    if (argc == 8 && !strcmp(argv[1], "visit")) return run(argv + 2, true);
    return 1;
}
