// Host driver for csrc/spectrum_core.h: runs the kernel's nine phases one thread after the other over the fields of a file
// (tests/test_spectra_cpu.py: the index maps and the arithmetic of csrc/spectrum.hip without a GPU).
//   host_spectrum N n_fields in.f32 out.f32
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>
struct alignas(16) float4 { float x, y, z, w; };
#include "spectrum_core.h"
using namespace spectrum;

template <int N>
void run(const float* x, float* spec, long long nf) {
    using P = Plan<N>;
    std::vector<float> img(P::IMG);
    std::vector<Cplx> tw(N);
    std::vector<double> d(P::AUX_D);
    std::vector<int> c(P::TPF);
    for (int j = 0; j < N; ++j) tw[j] = twiddle128(j * (128 / N));
    for (long long f = 0; f < nf; ++f) {
        FieldView v{x + f * N * N, spec + f * P::R, img.data(), tw.data(), d.data(), d.data() + P::TPF, c.data()};
        for (auto& e : img) e = NAN;  // a read of the row padding, or of a slot nothing wrote, shows in the output
#define PHASE(fn) for (int t = 0; t < P::TPF; ++t) fn<N>(v, t);
        PHASE(phase_load) PHASE(phase_fold) PHASE(phase_rows_a) PHASE(phase_rows_b) PHASE(phase_untangle)
        PHASE(phase_cols_a) PHASE(phase_cols_b) PHASE(phase_bins) PHASE(phase_store)
#undef PHASE
    }
}

int main(int argc, char** argv) {
    if (argc != 5) return 1;
    const int N = atoi(argv[1]);
    const long long nf = atoll(argv[2]);
    float* x = (float*)aligned_alloc(16, (size_t)nf * N * N * 4);
    std::vector<float> s((size_t)nf * N / 2);
    FILE* fi = fopen(argv[3], "rb");
    if (!fi || fread(x, 4, (size_t)nf * N * N, fi) != (size_t)(nf * N * N)) return 2;
    fclose(fi);
    switch (N) {
        case 8: run<8>(x, s.data(), nf); break;
        case 16: run<16>(x, s.data(), nf); break;
        case 32: run<32>(x, s.data(), nf); break;
        case 64: run<64>(x, s.data(), nf); break;
        case 128: run<128>(x, s.data(), nf); break;
        default: return 3;
    }
    FILE* fo = fopen(argv[4], "wb");
    if (!fo || fwrite(s.data(), 4, s.size(), fo) != s.size()) return 4;
    fclose(fo);
    free(x);
    return 0;
}
