// Host driver for csrc/wind_core.h: builds the packed table and runs the phases of the two kernels one thread after the other,
// workgroup by workgroup (tests/test_wind_cpu.py: the table, the lookup, the index maps, the arithmetic and the fold order of
// csrc/wind.hip without a GPU).
//   host_wind table K xs.f64 ps.f64 table.u8                                    (exit 5: the curve is refused)
//   host_wind power planes F u v hw with_derived hub K xs.f64 ps.f64 fields.f32 sums.f64 derived.f32
//   host_wind visit planes F u v hw owner.i32
// `visit` fills the fields with their own indices, so what a thread fetched says where it read: owner[k] is the one plane whose
// workgroups fetched value k (-1: nobody, -2: fetched more than once); it also checks that the thread holds the u value and the v value
// of the same cell.  It has its own main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"
#include "wind_core.h"
using namespace wind;

// one workgroup of wind_power_kernel; owner (if given) collects who fetched what; returns 0 or the number of a failed check
static int group(View& w, std::vector<int>* owner) {
    std::vector<Thread> th(THREADS);
    poison(w.lds, LDS_DOUBLES, NAN);  // a slot nobody stashed that reaches a sum shows
    PHASE(t_fetch(w, th[t], t))
    if (owner) {
        for (int t = 0; t < THREADS; ++t)
            for (int it = 0; it < ROUNDS; ++it) {
                if (!th[t].has[it]) continue;
                for (int k = 0; k < 4; ++k) {
                    const long long cell = cell_of(w.chunk, it, t) + k;
                    if (cell >= w.hw) return 8;
                    const long long at_u = (w.plane * w.F + w.u_index) * w.hw + cell, at_v = (w.plane * w.F + w.v_index) * w.hw + cell;
                    if (th[t].u[it].v[k] != (float)at_u || th[t].v[it].v[k] != (float)at_v) return 5;
                    for (long long at : {at_u, at_v}) {
                        int& o = (*owner)[(size_t)at];
                        o = o == -1 ? (int)w.plane : -2;
                    }
                }
            }
        return 0;
    }
    PHASE(t_cells(w, th[t], t))
    PHASE(t_stash(w, th[t], t))
    PHASE(t_fold_groups(w, t))
    PHASE(t_fold_store(w, t))
    return 0;
}

static int table(char** a) {
    const int K = atoi(a[0]);
    if (K < 1 || K > 4096) return 3;
    double *xs = read_file<double>(a[1], K), *ps = read_file<double>(a[2], K);
    const size_t n = K >= 2 && K <= MAX_K ? (size_t)table_bytes(K) : 16;
    unsigned char* bytes = (unsigned char*)aligned_alloc(16, n);
    memset(bytes, 0, n);
    int rc = build_table(xs, ps, K, bytes) ? 5 : write_file(a[3], bytes, n);
    free(xs), free(ps), free(bytes);
    return rc;
}

static int run(char** a, bool visit) {
    const long long planes = atoll(a[0]);
    const int F = atoi(a[1]), u = atoi(a[2]), v = atoi(a[3]), hw = atoi(a[4]);
    if (planes < 1 || F < 1 || u < 0 || u >= F || v < 0 || v >= F || hw < 4 || hw % 4) return 3;
    const size_t n = (size_t)planes * F * hw;
    const bool with_derived = !visit && atoi(a[5]);
    int K = 2;
    float* x;
    double xs2[2] = {1.0, 2.0}, ps2[2] = {0.0, 1.0}, *xs = xs2, *ps = ps2;
    if (visit) {
        if (n >= (1u << 24)) return 3;  // an index must be an fp32
        x = alloc16<float>(n);
        for (size_t k = 0; k < n; ++k) x[k] = (float)k;
    } else {
        K = atoi(a[7]);
        if (!supported(hw, K)) return 3;
        xs = read_file<double>(a[8], K), ps = read_file<double>(a[9], K);
        x = read_file<float>(a[10], n);
    }
    unsigned char* bytes = (unsigned char*)aligned_alloc(16, (size_t)table_bytes(K));
    if (build_table(xs, ps, K, bytes)) return 5;
    const int nc = chunks(hw);
    std::vector<double> sums((size_t)planes * 2, -7.25), partial((size_t)(scratch_bytes(planes, hw) / 8), NAN), lds(LDS_DOUBLES);
    std::vector<float> derived(with_derived ? (size_t)planes * 2 * hw : 0, -7.25f);
    std::vector<int> owner(visit ? n : 0, -1);
    View w{};
    w.fields = x, w.out = nc > 1 ? partial.data() : sums.data(), w.derived = with_derived ? derived.data() : nullptr;
    w.F = F, w.u_index = u, w.v_index = v, w.hw = hw, w.hub = visit ? 1.f : strtof(a[6], nullptr), w.table = view_table(bytes, K), w.lds = lds.data();
    int rc = 0;
    for (w.plane = 0; w.plane < planes && !rc; ++w.plane)
        for (w.chunk = 0; w.chunk < nc && !rc; ++w.chunk) rc = group(w, visit ? &owner : nullptr);
    if (!rc && visit) {
        rc = write_file(a[5], owner.data(), owner.size());
    } else if (!rc) {
        if (nc > 1)
            for (long long e = 0; e < planes * 2; ++e) f_fold(partial.data(), sums.data(), e, nc);
        rc = write_file(a[11], sums.data(), sums.size()) | write_file(a[12], derived.data(), derived.size());
    }
    free(x), free(bytes);
    if (!visit) free(xs), free(ps);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "table")) return table(argv + 2);
    if (argc == 15 && !strcmp(argv[1], "power")) return run(argv + 2, false);
    if (argc == 8 && !strcmp(argv[1], "visit")) return run(argv + 2, true);
    return 1;
}
