// Host driver for csrc/swd_core.h: runs the phases of both kernels one thread after the other, workgroup by workgroup, with the matrix
// core restated in C++ (tests/test_swd_cpu.py: the index maps, the k order and the sort network of csrc/swd.hip without a GPU).
//   host_swd project  n_rep T F d P x.f32 theta.f32 shift.f32 scale.f32 proj.f32
//   host_swd distance n_rep F P T proj_x.f32 proj_y.f32 out.f64
// It has its own main, so it may be built with -fsanitize=address,undefined and run directly.
#include "host_main.h"
#include "swd_core.h"
using namespace swd;

static int project(char** a) {
    const long long n_rep = atoll(a[0]);
    const int T = atoi(a[1]), F = atoi(a[2]), d = atoi(a[3]), P = atoi(a[4]);
    if (!project_supported(d, P) || n_rep < 1 || T < 1 || F < 1) return 3;
    const long long n_fields = n_rep * T * F;
    float *x = read_file<float>(a[5], (size_t)n_fields * d), *theta = read_file<float>(a[6], (size_t)P * d), *shift = read_file<float>(a[7], F), *scale = read_file<float>(a[8], F);
    std::vector<float> out((size_t)n_fields * P, -7.25f);
    float* lds = (float*)aligned_alloc(16, sizeof(float) * LDS_FLOATS);
    std::vector<PThread> th(THREADS);
    PView v{};
    v.x = x, v.theta = theta, v.shift = shift, v.scale = scale, v.proj = out.data();
    v.n_fields = n_fields, v.T = T, v.F = F, v.d = d, v.P = P, v.lds = lds;
    const int steps = d / BK;
    for (v.first = 0; v.first < n_fields; v.first += BM) {
        poison(lds, LDS_FLOATS, NAN);  // a value nothing wrote that reaches a kept sum shows in the output
        PHASE(p_init(v, th[t], t))
        PHASE(p_fetch(v, th[t], 0))
        PHASE(p_stash(v, th[t], t, 0))
        for (int kt = 0; kt < steps; ++kt) {
            if (kt + 1 < steps) PHASE(p_fetch(v, th[t], kt + 1))
            for (int w = 0; w < THREADS / 64; ++w) p_compute_wave(v, th.data() + 64 * w, w, kt & 1);
            if ((kt + 1) % FOLD == 0 || kt + 1 == steps) PHASE(p_fold(th[t]))
            if (kt + 1 < steps) PHASE(p_stash(v, th[t], t, (kt + 1) & 1))
        }
        poison(lds, LDS_FLOATS, NAN);
        PHASE(p_epi_stash(v, th[t], t))
        PHASE(p_epi_write(v, t))
    }
    free(lds), free(x), free(theta), free(shift), free(scale);
    return write_file(a[9], out);
}

static int distance(char** a) {
    const long long n_rep = atoll(a[0]);
    const int F = atoi(a[1]), P = atoi(a[2]), T = atoi(a[3]);
    if (!distance_supported(T) || n_rep < 1 || F < 1 || P < 1) return 3;
    const long long n = n_rep * F * P;
    float *px = read_file<float>(a[4], (size_t)n * T), *py = read_file<float>(a[5], (size_t)F * P * T);
    std::vector<double> out((size_t)n, -7.25), dpart(SORT_DOUBLES);
    DView v{};
    v.px = px, v.py = py, v.out = out.data(), v.F = F, v.P = P, v.T = T, v.N = padded(T), v.nthr = sort_threads(v.N);
    std::vector<float> keys(2 * (size_t)v.N);
    v.keys = keys.data(), v.dpart = dpart.data();
    for (v.block = 0; v.block < n; ++v.block) {
        poison(keys.data(), keys.size(), NAN), poison(dpart.data(), dpart.size(), NAN);
        int nan = 0;
        for (int t = 0; t < v.nthr; ++t) nan |= d_load(v, t);
        if (!nan) {
            for (int k = 2; k <= v.N; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1)
                    for (int t = 0; t < v.nthr; ++t) d_stage(v, t, k, j);
            for (int t = 0; t < v.nthr; ++t) d_partial(v, t);
            for (int t = 0; t < v.nthr; ++t) d_fold(v, t);
        }
        for (int t = 0; t < v.nthr; ++t) d_store(v, t, nan);
    }
    free(px), free(py);
    return write_file(a[6], out);
}

int main(int argc, char** argv) {
    if (argc == 12 && !strcmp(argv[1], "project")) return project(argv + 2);
    if (argc == 9 && !strcmp(argv[1], "distance")) return distance(argv + 2);
    return 1;
}
