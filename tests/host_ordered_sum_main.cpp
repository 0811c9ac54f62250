// Host driver for csrc/ordered_sum.h: runs the fixed-order sum one thread after the other (tests/test_ordered_sum_cpu.py: the LDS layout,
// the order of the additions and the two write policies, without a GPU).
//   host_ordered_sum workgroup N policy acc.f64 out.f64               acc [N][256] -> out [N]: stash, fold_groups, fold_total, policy
//   host_ordered_sum parts outer parts inner policy partial.f64 out.f64   partial [outer][parts][inner] -> out [outer][inner]
// policy: 0 nan_if_nan, 1 nan_if_not_finite; N: 1, 2, 4 or 12.  The LDS starts as NaNs, so a slot nobody wrote that reaches a sum shows.
// It has its own main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"
#include "ordered_sum.h"
using namespace ordered_sum;

static double written(int policy, double t) { return policy ? nan_if_not_finite(t) : nan_if_nan(t); }

template <int N>
static int workgroup(int policy, const char* in, const char* out_path) {
    double* acc = read_file<double>(in, (size_t)N * THREADS, 0);
    std::vector<double> lds(lds_doubles<N>(), NAN), out(N, -7.25);
    double mine[THREADS][N];
    for (int t = 0; t < THREADS; ++t)
        for (int s = 0; s < N; ++s) mine[t][s] = acc[(size_t)s * THREADS + t];
    free(acc);
    PHASE(stash<N>(lds.data(), mine[t], t))
    PHASE(fold_groups<N>(lds.data(), t))
    PHASE(if (t < N) out[t] = written(policy, fold_total<N>(lds.data(), t)))
    return write_file(out_path, out);
}

static int parts(char** a) {
    const long long outer = atoll(a[0]), np = atoll(a[1]), inner = atoll(a[2]);
    const int policy = atoi(a[3]);
    if (outer < 1 || np < 1 || inner < 1) return 3;
    double* partial = read_file<double>(a[4], (size_t)(outer * np * inner), 0);
    std::vector<double> out((size_t)(outer * inner), -7.25);
    for (long long e = 0; e < outer * inner; ++e) out[(size_t)e] = written(policy, fold_parts(partial, e, np, inner));
    free(partial);
    return write_file(a[5], out);
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "workgroup")) {
        const int policy = atoi(argv[3]);
        switch (atoi(argv[2])) {
            case 1: return workgroup<1>(policy, argv[4], argv[5]);
            case 2: return workgroup<2>(policy, argv[4], argv[5]);
            case 4: return workgroup<4>(policy, argv[4], argv[5]);
            case 12: return workgroup<12>(policy, argv[4], argv[5]);
            default: return 3;
        }
    }
    if (argc == 8 && !strcmp(argv[1], "parts")) return parts(argv + 2);
    return 1;
}
