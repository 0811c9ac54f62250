// Host driver for csrc/crps_core.h: runs the phases of the two kernels one thread after the other, workgroup by workgroup
// (tests/test_crps_cpu.py: the index maps, the arithmetic and the fold order of csrc/crps.hip without a GPU).
//   host_crps terms M T F hw with_cells x.f32 y.f32 sums.f64 cells.f32
//   host_crps visit M T F hw owner_x.i32 owner_y.i32
// `visit` fills x and y with their own indices, so what a thread fetched says where it read: owner[k] is the one plane whose workgroups
// fetched value k (-1: nobody, -2: fetched more than once); it also checks that row i of a thread's registers holds member i of the
// thread's own cells and that the rows from M on hold +inf.  It has its own main, so it is built with -fsanitize=address,undefined
// and run directly.
#include "host_main.h"
#include "crps_core.h"
using namespace crps;

// one workgroup of crps_terms_kernel<K, V>; owner (if given) collects who fetched what; returns 0 or the number of a failed check
template <int K, int V>
static int group(View& v, std::vector<int>* owner, size_t nx) {
    std::vector<Thread<K, V>> th(THREADS);
    poison(v.lds, LDS_DOUBLES, NAN);  // a slot nobody stashed that reaches a sum shows
    PHASE(t_init(v, th[t]))
    const long long member = (long long)v.T * v.F * v.hw;
    const int n = rounds(v.hw, v.chunk, V);
    for (int it = 0; it < n; ++it) {
        PHASE(t_fetch(v, th[t], t, it))
        if (owner)
            for (int t = 0; t < THREADS; ++t) {
                if (!th[t].has) continue;
                for (int c = 0; c < V; ++c) {
                    const long long at = v.plane * v.hw + th[t].cell + c;
                    for (int i = 0; i < K; ++i) {
                        if (i >= v.M) {
                            if (!(th[t].s[i][c] == INFINITY)) return 7;
                            continue;
                        }
                        if (th[t].s[i][c] != (float)(i * member + at)) return 5;
                        int& o = (*owner)[(size_t)th[t].s[i][c]];
                        o = o == -1 ? (int)v.plane : -2;
                    }
                    if (th[t].y[c] != (float)(nx + at)) return 5;
                    int& o = (*owner)[(size_t)th[t].y[c]];
                    o = o == -1 ? (int)v.plane : -2;
                }
            }
        PHASE(t_cells(v, th[t]))
    }
    PHASE(t_stash(v, th[t], t))
    PHASE(t_fold_groups(v, t))
    PHASE(t_fold_store(v, t))
    return 0;
}

static int dispatch(View& v, std::vector<int>* owner, size_t nx) {
    switch (rows_of(v.M)) {
        case 8: return group<8, 4>(v, owner, nx);
        case 16: return group<16, 4>(v, owner, nx);
        case 32: return group<32, 2>(v, owner, nx);
        default: return group<64, 1>(v, owner, nx);
    }
}

static int run(char** a, bool visit) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]);
    if (!supported(hw, M) || T < 1 || F < 1) return 3;
    const bool with_cells = !visit && atoi(a[4]);
    const size_t ny = (size_t)T * F * hw, nx = (size_t)M * ny;
    if (visit && nx + ny >= (1u << 24)) return 3;  // an index must be an fp32
    float *x, *y;
    if (visit) {
        x = alloc16<float>(nx), y = alloc16<float>(ny);
        for (size_t k = 0; k < nx; ++k) x[k] = (float)k;
        for (size_t k = 0; k < ny; ++k) y[k] = (float)(nx + k);
    } else {
        x = read_file<float>(a[5], nx), y = read_file<float>(a[6], ny);
    }
    const int nc = chunks(hw);
    const long long planes = (long long)T * F;
    std::vector<double> sums((size_t)planes * 4, -7.25), partial((size_t)(scratch_bytes(T, F, hw) / 8), NAN), lds(LDS_DOUBLES);
    std::vector<float> cells(with_cells ? 4 * ny : 0, -7.25f);
    std::vector<int> owner(nx + ny, -1);
    View v{};
    v.x = x, v.y = y, v.out = nc > 1 ? partial.data() : sums.data(), v.cells = with_cells ? cells.data() : nullptr;
    v.M = M, v.T = T, v.F = F, v.hw = hw, v.lds = lds.data();
    int rc = 0;
    for (v.plane = 0; v.plane < planes && !rc; ++v.plane)
        for (v.chunk = 0; v.chunk < nc && !rc; ++v.chunk) rc = dispatch(v, visit ? &owner : nullptr, nx);
    if (nc > 1)
        for (long long e = 0; e < planes * 4; ++e) f_fold(partial.data(), sums.data(), e, nc);
    if (!rc && visit) {
        for (double p : partial)
            if (p != p) rc = 6;  // a partial nobody wrote (the indices are finite, so no workgroup wrote NaN on purpose)
        std::vector<int> ox(owner.begin(), owner.begin() + nx), oy(owner.begin() + nx, owner.end());
        if (!rc) rc = write_file(a[4], ox) | write_file(a[5], oy);
    } else if (!rc) {
        rc = write_file(a[7], sums) | write_file(a[8], cells);
    }
    free(x), free(y);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 11 && !strcmp(argv[1], "terms")) return run(argv + 2, false);
    if (argc == 8 && !strcmp(argv[1], "visit")) return run(argv + 2, true);
    return 1;
}
