// Host driver for csrc/spectrum_core.h: runs the kernel's nine phases one thread after the other over the fields of a file
// (tests/test_spectra_cpu.py: the index maps and the arithmetic of csrc/spectrum.hip without a GPU).
//   host_spectrum N n_fields in.f32 out.f32
#include "host_main.h"
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
        poison(img.data(), img.size(), NAN);  // a read of the row padding, or of a slot nothing wrote, shows in the output
#define FIELD_PHASE(fn) PHASE_N(P::TPF, fn<N>(v, t))
        FIELD_PHASE(phase_load) FIELD_PHASE(phase_fold) FIELD_PHASE(phase_rows_a) FIELD_PHASE(phase_rows_b) FIELD_PHASE(phase_untangle)
        FIELD_PHASE(phase_cols_a) FIELD_PHASE(phase_cols_b) FIELD_PHASE(phase_bins) FIELD_PHASE(phase_store)
#undef FIELD_PHASE
    }
}

int main(int argc, char** argv) {
    if (argc != 5) return 1;
    const int N = atoi(argv[1]);
    const long long nf = atoll(argv[2]);
    float* x = read_file<float>(argv[3], (size_t)nf * N * N, 0);  // no slack: a read past the last field shows
    std::vector<float> s((size_t)nf * N / 2);
    switch (N) {
        case 8: run<8>(x, s.data(), nf); break;
        case 16: run<16>(x, s.data(), nf); break;
        case 32: run<32>(x, s.data(), nf); break;
        case 64: run<64>(x, s.data(), nf); break;
        case 128: run<128>(x, s.data(), nf); break;
        default: return 3;
    }
    free(x);
    return write_file(argv[4], s);
}
