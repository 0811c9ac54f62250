// Host driver for csrc/kde_core.h: runs the phases of the three kernels one thread after the other, workgroup by workgroup
// (tests/test_kde_cpu.py: the index maps, the fold order and the bin rule of csrc/kde.hip without a GPU).
//   host_kde density n_rep T F hw N with_truth x.f32 y.f32 offsets.f32 pivot.f32 h.f64 dens.f64
//   host_kde visit   n_rep T F hw N owner_x.i32 owner_y.i32
//   host_kde pit     M T F hw grid x.f32 y.f32 counts.i64
// `visit` fills x and y with their own indices, so what a workgroup fetched says where it read: owner[k] is the one data set that
// fetched value k (-1: nobody, -2: fetched more than once); it also checks that every grid point belongs to exactly one (thread,
// register).  It has its own main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"
#include "kde_core.h"
using namespace kde;

// one workgroup of kde_partial_kernel<P>; seen (if given) collects the floats every thread fetched
template <int P>
static void partial_group(KView& v, std::vector<float>* seen) {
    std::vector<KThread<P>> th(THREADS);
    poison(v.lds, THREADS, float4{NAN, NAN, NAN, NAN});  // a value nothing staged that reaches a sum shows
    PHASE(k_init(v, th[t], t))
    const long long tiles = k_tiles(th[0]);
    auto fetch = [&](long long tile) {
        for (int t = 0; t < THREADS; ++t) {
            k_fetch(v, th[t], t, tile);
            if (!seen || !th[t].has) continue;
            const float4 q = th[t].raw;
            seen->push_back(q.x), seen->push_back(q.y), seen->push_back(q.z), seen->push_back(q.w);
        }
    };
    fetch(0);
    for (long long tile = 0; tile < tiles; ++tile) {
        PHASE(k_stash(v, th[t], t))
        if (tile + 1 < tiles) fetch(tile + 1);
        PHASE(k_compute(v, th[t], k_count(th[t], tile)))
    }
    int bad = 0;
    PHASE(bad |= th[t].bad)
    PHASE(k_store(v, th[t], t, bad))
}

static void partial_dispatch(KView& v, std::vector<float>* seen) {
    switch (points_per_thread(v.N)) {
        case 1: partial_group<1>(v, seen); break;
        case 2: partial_group<2>(v, seen); break;
        case 3: partial_group<3>(v, seen); break;
        default: partial_group<4>(v, seen); break;
    }
}

static int density(char** a, bool visit) {
    const long long n_rep = atoll(a[0]);
    const int T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), N = atoi(a[4]);
    const bool with_y = visit || atoi(a[5]);
    if (!supported(hw, N) || n_rep < 1 || T < 1 || F < 1) return 3;
    const long long n_x = n_rep * F, D = n_x + (with_y ? F : 0), n = (long long)T * hw, nc = chunks(n);
    const size_t nx = (size_t)n_rep * T * F * hw, ny = (size_t)T * F * hw;
    if (visit && nx + ny >= (1u << 24)) return 3;  // an index must be an fp32
    float *x, *y = nullptr, *off, *pivot;
    double* h;
    if (visit) {
        x = alloc16<float>(nx), y = alloc16<float>(ny);
        for (size_t k = 0; k < nx; ++k) x[k] = (float)k;
        for (size_t k = 0; k < ny; ++k) y[k] = (float)(nx + k);
        off = (float*)calloc((size_t)F * N, 4), pivot = (float*)calloc(F, 4), h = alloc16<double>((size_t)D);
        for (long long i = 0; i < D; ++i) h[i] = 1.0;
    } else {
        x = read_file<float>(a[6], nx);
        if (with_y) y = read_file<float>(a[7], ny);
        off = read_file<float>(a[8], (size_t)F * N), pivot = read_file<float>(a[9], F), h = read_file<double>(a[10], D);
    }
    std::vector<double> partial((size_t)(D * nc * N), NAN), dens((size_t)D * N, -7.25);
    std::vector<int> owner(nx + ny, -1);
    float4* lds = (float4*)aligned_alloc(16, sizeof(float4) * THREADS);
    KView v{};
    v.x = x, v.y = y, v.off = off, v.pivot = pivot, v.h = h, v.partial = partial.data(), v.n_x = n_x, v.T = T, v.F = F, v.hw = hw, v.N = N, v.lds = lds;
    for (v.ds = 0; v.ds < D; ++v.ds)
        for (v.chunk = 0; v.chunk < nc; ++v.chunk) {
            std::vector<float> seen;
            partial_dispatch(v, visit ? &seen : nullptr);
            for (float q : seen) owner[(size_t)q] = owner[(size_t)q] == -1 ? (int)v.ds : -2;
        }
    for (long long ds = 0; ds < D; ++ds)
        for (int blk = 0; blk < (N + THREADS - 1) / THREADS; ++blk)
            for (int t = 0; t < THREADS; ++t)
                if (blk * THREADS + t < N) f_fold(partial.data(), h, dens.data(), ds, blk * THREADS + t, n, N);
    int rc = 0;
    if (visit) {
        std::vector<int> hits(N, 0);
        for (int t = 0; t < THREADS; ++t)
            for (int r = 0; r < points_per_thread(N); ++r)
                if (point_of(t, r) < N) ++hits[point_of(t, r)];
        for (int j = 0; j < N; ++j)
            if (hits[j] != 1) rc = 5;
        for (double p : partial)
            if (p != p) rc = 6;  // a partial nobody wrote (the indices are finite, so no workgroup wrote NaN on purpose)
        std::vector<int> ox(owner.begin(), owner.begin() + nx), oy(owner.begin() + nx, owner.end());
        if (!rc) rc = write_file(a[5], ox) | write_file(a[6], oy);
    } else {
        rc = write_file(a[11], dens);
    }
    free(lds), free(x), free(y), free(off), free(pivot), free(h);
    return rc;
}

static int pit(char** a) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]);
    const long long grid = atoll(a[4]);
    if (!pit_supported(hw, M) || T < 1 || F < 1 || grid < F || grid % F) return 3;
    float *x = read_file<float>(a[5], (size_t)M * T * F * hw), *y = read_file<float>(a[6], (size_t)T * F * hw);
    std::vector<long long> counts((size_t)F * (M + 1), 0);
    std::vector<int> hist(PIT_HIST);
    PView v{};
    v.x = x, v.y = y, v.counts = counts.data(), v.grid = grid, v.M = M, v.T = T, v.F = F, v.hw = hw, v.hist = hist.data();
    for (v.block = 0; v.block < grid; ++v.block) {
        poison(hist.data(), hist.size(), -1000000);  // a bin nobody zeroed shows
        PHASE(pit_zero(v, t))
        PHASE(pit_count(v, t))
        PHASE(pit_flush(v, t))
    }
    free(x), free(y);
    return write_file(a[7], counts);
}

int main(int argc, char** argv) {
    if (argc == 14 && !strcmp(argv[1], "density")) return density(argv + 2, false);
    if (argc == 9 && !strcmp(argv[1], "visit")) return density(argv + 2, true);
    if (argc == 10 && !strcmp(argv[1], "pit")) return pit(argv + 2);
    return 1;
}
