// Host driver for csrc/qmap_core.h: runs the phases of the three kernels of csrc/qmap.hip one thread after the other, workgroup by
// workgroup (tests/test_qmap_cpu.py: the index maps, the sort, the bisection and the arithmetic without a GPU).
//   host_qmap nodes n_rep T F hw G K skipna block x.f32 tidx.i32 goff.i32 levels.f64 q.f64 nvalid.i64
//   host_qmap apply n_rep T F hw G K slabs x.f32 xq.f64 yq.f64 tidx.i32 goff.i32 out.f32
// `nodes` walks the cells in blocks of `block`, as the host layer does; it fails if the network leaves a series unsorted or an output
// is left unwritten.  `apply` works in place and counts, through QMAP_VISIT, how often every element is taken up: exactly once.  It
// has its own main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"

static std::vector<int>* g_visits = nullptr;
static void visit4(long long at) {
    for (int e = 0; e < 4; ++e) ++(*g_visits)[(size_t)at + e];
}
#define QMAP_VISIT(index) visit4(index)
#include "qmap_core.h"
using namespace qmap;

static int run_nodes(char** a) {
    const int n_rep = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), G = atoi(a[4]), K = atoi(a[5]), skipna = atoi(a[6]), block = atoi(a[7]);
    if (n_rep < 1 || T < 1 || F < 1 || G < 1 || block < 1) return 3;
    float* x = read_file<float>(a[8], (size_t)n_rep * T * F * hw);
    int *tidx = read_file<int>(a[9], T), *goff = read_file<int>(a[10], G + 1);
    double* levels = read_file<double>(a[11], K);
    int max_len = 0;
    for (int g = 0; g < G; ++g) max_len = goff[g + 1] - goff[g] > max_len ? goff[g + 1] - goff[g] : max_len;
    if (!supported(hw, K, max_len)) return 3;
    const int Tu = goff[G];
    const long long rows = (long long)n_rep * F, cells = (long long)rows * G * hw;
    const unsigned long long unwritten_bits = 0x7FF8DEADBEEF0000ull;  // a NaN no arithmetic here produces
    double unwritten;
    memcpy(&unwritten, &unwritten_bits, 8);
    std::vector<double> q((size_t)cells * K, unwritten);
    std::vector<long long> nvalid((size_t)cells, -1);
    std::vector<float> tile(TILE * TILE_LD);
    std::vector<unsigned> keys(padded(max_len));
    for (int c0 = 0; c0 < hw; c0 += block) {
        const int c1 = c0 + block < hw ? c0 + block : hw;
        std::vector<float> scratch((size_t)(scratch_bytes(rows, c1 - c0, Tu) / 4), -12345.0f);
        GView gv{};
        gv.x = x, gv.tidx = tidx, gv.scratch = scratch.data(), gv.T = T, gv.F = F, gv.hw = hw, gv.Tu = Tu, gv.c0 = c0, gv.c1 = c1, gv.tile = tile.data();
        for (gv.row = 0; gv.row < rows; ++gv.row)
            for (gv.ctile = 0; gv.ctile < tiles(c1 - c0); ++gv.ctile)
                for (gv.ptile = 0; gv.ptile < tiles(Tu); ++gv.ptile) {
                    poison(tile.data(), tile.size(), -12345.0f);
                    PHASE(g_load(gv, t))
                    PHASE(g_store(gv, t))
                }
        SView sv{};
        sv.scratch = scratch.data(), sv.goff = goff, sv.levels = levels, sv.q = q.data(), sv.nvalid = nvalid.data();
        sv.F = F, sv.hw = hw, sv.Tu = Tu, sv.c0 = c0, sv.c1 = c1, sv.G = G, sv.K = K, sv.skipna = skipna, sv.max_len = max_len;
        sv.nthr = sort_threads(padded(max_len)), sv.keys = keys.data();
        const long long series = rows * (c1 - c0) * G;
        for (sv.series = 0; sv.series < series; ++sv.series) {
            poison(keys.data(), keys.size(), 12345u);
            PHASE_N(sv.nthr, s_load(sv, t))
            const int N = padded(length_of(sv));
            for (int k = 2; k <= N; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) PHASE_N(sv.nthr, s_stage(sv, t, k, j))
            for (int i = 1; i < N; ++i)
                if (keys[i - 1] > keys[i]) return 6;  // the network sorts
            PHASE_N(sv.nthr, s_nodes(sv, t))
        }
    }
    for (long long n : nvalid)
        if (n < 0) return 7;  // an entry nobody wrote
    for (double v : q)
        if (!memcmp(&v, &unwritten, 8)) return 7;
    int rc = write_file(a[12], q);
    if (!rc) rc = write_file(a[13], nvalid);
    free(x), free(tidx), free(goff), free(levels);
    return rc;
}

static int run_apply(char** a) {
    const int n_rep = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), G = atoi(a[4]), K = atoi(a[5]), slabs = atoi(a[6]);
    if (n_rep < 1 || T < 1 || F < 1 || G < 1 || slabs < 1) return 3;
    const size_t n = (size_t)n_rep * T * F * hw, nt = (size_t)G * F * hw * K;
    float* x = read_file<float>(a[7], n);
    double *xq = read_file<double>(a[8], nt), *yq = read_file<double>(a[9], nt);
    int *tidx = read_file<int>(a[10], T), *goff = read_file<int>(a[11], G + 1);
    int max_len = 0;
    for (int g = 0; g < G; ++g) max_len = goff[g + 1] - goff[g] > max_len ? goff[g + 1] - goff[g] : max_len;
    if (!supported(hw, K, max_len)) return 3;
    std::vector<int> visits(n, 0);
    g_visits = &visits;
    std::vector<double> lds((size_t)apply_lds_bytes(K) / 8);
    AView v{};
    v.x = x, v.out = x, v.xq = xq, v.yq = yq, v.tidx = tidx, v.goff = goff, v.n_rep = n_rep, v.slabs = slabs;  // in place
    v.T = T, v.F = F, v.hw = hw, v.Tu = goff[G], v.K = K, v.lds = lds.data();
    for (v.g = 0; v.g < G; ++v.g)
        for (v.f = 0; v.f < F; ++v.f)
            for (v.cblock = 0; v.cblock < cell_blocks(hw, K); ++v.cblock)
                for (v.slab = 0; v.slab < slabs; ++v.slab) {
                    poison(lds.data(), lds.size(), NAN);
                    PHASE_N(APPLY_THREADS, a_stage(v, t))
                    PHASE_N(APPLY_THREADS, a_walk(v, t))
                }
    int rc = 0;
    std::vector<char> listed(T, 0);
    for (int p = 0; p < goff[G]; ++p) listed[tidx[p]] = 1;
    for (size_t i = 0; i < n && !rc; ++i)
        if (visits[i] != listed[(i / ((size_t)F * hw)) % T]) rc = 5;
    if (!rc) rc = write_file(a[12], x, n);
    free(x), free(xq), free(yq), free(tidx), free(goff);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 16 && !strcmp(argv[1], "nodes")) return run_nodes(argv + 2);
    if (argc == 15 && !strcmp(argv[1], "apply")) return run_apply(argv + 2);
    return 1;
}
