// Host driver for csrc/ssim_core.h: runs the kernel's phases one thread after the other, workgroup by workgroup, over the pairs of two
// files (tests/test_ssim_cpu.py: the index maps and the arithmetic of csrc/ssim.hip without a GPU).
//   host_ssim H W win n_pairs n_truth x.f32 y.f32 range.f32 out.f64
#include "host_main.h"
#include "ssim_core.h"
using namespace ssim;

template <int WIN>
void run(View v, int H, int W) {
    using P = Plan<WIN>;
    const Shape sh = make_shape(H, W, WIN);
    float* f = (float*)aligned_alloc(16, sizeof(float) * P::FLOATS);
    std::vector<double> d(DOUBLES);
    std::vector<Thread> th(THREADS);
    v.ringA = f, v.ringB = f + P::RING_FLOATS, v.V = f + 2 * P::RING_FLOATS;
    v.dpart = d.data(), v.dlev = d.data() + THREADS;
    for (v.first = 0; v.first < v.n_pairs; v.first += sh.FPW) {
        poison(f, P::FLOATS, NAN);  // a value nothing wrote that reaches a kept sum shows in the output
        PHASE(phase_pivot_partial(v, sh, t))
        PHASE(phase_pivot_fold(v, sh, t))
        PHASE(phase_prologue<WIN>(v, sh, th[t], t))
        PHASE(fetch<WIN>(v, sh, th[t], t, 0))
        for (int s = 0; s < sh.NS; ++s) {
            PHASE(phase_stash<WIN>(v, sh, th[t], t, s))
            if (s + 1 < sh.NS) PHASE(fetch<WIN>(v, sh, th[t], t, s + 1))
            PHASE(phase_vertical<WIN>(v, sh, t, s))
            PHASE(phase_horizontal<WIN>(v, sh, th[t], t, s))
        }
        PHASE(phase_partial(v, th[t], t))
        PHASE(phase_fold(v, sh, t))
        PHASE(phase_store(v, sh, t))
    }
    free(f);
}

int main(int argc, char** argv) {
    if (argc != 10) return 1;
    const int H = atoi(argv[1]), W = atoi(argv[2]), win = atoi(argv[3]);
    const long long np = atoll(argv[4]), nt = atoll(argv[5]);
    if (!supported(H, W, win) || np < 0 || nt < 1) return 3;
    View v{};
    float* x = read_file<float>(argv[6], (size_t)np * H * W, 0);  // no slack: a read past an input shows
    float* y = read_file<float>(argv[7], (size_t)nt * H * W, 0);
    float* r = read_file<float>(argv[8], (size_t)nt, 0);
    std::vector<double> out((size_t)np, -7.25);
    v.x = x, v.y = y, v.range = r, v.out = out.data(), v.n_pairs = np, v.n_truth = nt;
    switch (win) {
        case 7: run<7>(v, H, W); break;
        case 11: run<11>(v, H, W); break;
        default: run<15>(v, H, W); break;
    }
    free(x), free(y), free(r);
    return write_file(argv[9], out);
}
