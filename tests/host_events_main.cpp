// Host driver for csrc/events_core.h: runs the phases of event_counts_kernel and fss_sums_kernel one thread after the other, workgroup
// by workgroup (tests/test_events_cpu.py: the index maps and the integer arithmetic of csrc/events.hip without a GPU).
//   host_events counts M T F hw K x.f32 y.f32 thr.f32 dir.i32 counts.i64 invalid.i64
//   host_events fss M T F H W K S r_0 .. r_{S-1} x.f32 y.f32 thr.f32 dir.i32 sums.i64
//   host_events visit_counts M T F hw K
//   host_events visit_fss M T F H W K S r_0 .. r_{S-1}
// The visit modes count, through the EV_VISIT_* hooks, how often every cell is binned (once per threshold), every region cell staged
// (once per tile whose halo reaches it, inside the domain), every tile cell summed (once per row and radius) and every corner of the
// cumulative table read (as often as the windows clipped to the DOMAIN say), and compare the tables with a direct count.  LDS is
// filled with a pattern before every workgroup, so a slot nobody zeroed shows.  It has its own main, so it is built with
// -fsanitize=address,undefined and run directly.
#include "host_main.h"

static int g_H = 0, g_W = 0, g_hw = 0, g_K = 0, g_S = 0, g_M = 0, g_bad = 0;
static std::vector<long long> g_cells, g_loads, g_sums, g_corners;  // [plane][k][cell]; [d][cell]; [d][s][cell]; [s][(H + 1) (W + 1)]
static bool g_visit = false;
static void visit_cell(long long plane, int k, int cell) {
    if (g_visit) ++g_cells[((size_t)plane * g_K + k) * g_hw + cell];
}
static void visit_load(int d, int gy, int gx) {
    if (!g_visit) return;
    if (gy < 0 || gy >= g_H || gx < 0 || gx >= g_W) g_bad = 1;
    else ++g_loads[(size_t)d * g_hw + gy * g_W + gx];
}
static void visit_sum(int d, int s, int gy, int gx) {
    if (!g_visit) return;
    if (gy < 0 || gy >= g_H || gx < 0 || gx >= g_W) g_bad = 1;
    else ++g_sums[((size_t)d * g_S + s) * g_hw + gy * g_W + gx];
}
static void visit_corner(int d, int s, int gy, int gx) {
    if (!g_visit || d != 0) return;  // the truth's own row: every row reads the same corners
    if (gy < 0 || gy > g_H || gx < 0 || gx > g_W) g_bad = 1;
    else ++g_corners[(size_t)s * (g_H + 1) * (g_W + 1) + gy * (g_W + 1) + gx];
}
#define EV_VISIT_CELL(plane, k, cell) visit_cell(plane, k, cell)
#define EV_VISIT_LOAD(d, gy, gx) visit_load(d, gy, gx)
#define EV_VISIT_SUM(d, s, gy, gx) visit_sum(d, s, gy, gx)
#define EV_VISIT_CORNER(d, s, gy, gx) visit_corner(d, s, gy, gx)
#include "events_core.h"
using namespace events;

struct Inputs {
    float *x, *y, *thr;
    int* dir;
};
// finite fields with events in every row, thresholds inside their range, alternating directions
static Inputs synthetic(int M, int T, int F, int hw, int K) {
    const size_t ny = (size_t)T * F * hw, nx = (size_t)M * ny;
    Inputs in;
    in.x = alloc16<float>(nx), in.y = alloc16<float>(ny), in.thr = alloc16<float>((size_t)F * K), in.dir = alloc16<int>((size_t)F * K);
    for (size_t i = 0; i < nx; ++i) in.x[i] = (float)((i * 7919u) % 1021u) * 0.25f;
    for (size_t i = 0; i < ny; ++i) in.y[i] = (float)((i * 104729u) % 1019u) * 0.25f;
    for (int i = 0; i < F * K; ++i) in.thr[i] = 60.f + 20.f * (float)(i % 9), in.dir[i] = i % 2;
    return in;
}
static void release(Inputs& in) { free(in.x), free(in.y), free(in.thr), free(in.dir); }

static void counts_group(CView& v) {
    poison(v.lds, COUNT_LDS_INTS, 0x55555555);
    PHASE(c_zero(v, t))
    PHASE(c_count(v, t))
    PHASE(c_derive(v, t))
    PHASE(c_flush(v, t))
}

static int run_counts(char** a, bool visit) {
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), hw = atoi(a[3]), K = atoi(a[4]);
    if (!counts_supported(hw, M, K) || T < 1 || F < 1) return 3;
    const size_t ny = (size_t)T * F * hw;
    Inputs in;
    if (visit) in = synthetic(M, T, F, hw, K);
    else in.x = read_file<float>(a[5], M * ny), in.y = read_file<float>(a[6], ny), in.thr = read_file<float>(a[7], (size_t)F * K), in.dir = read_file<int>(a[8], (size_t)F * K);
    const long long planes = (long long)T * F;
    std::vector<long long> counts((size_t)planes * K * bins(M), 0), invalid((size_t)planes, 0);  // the launcher zeroes both
    std::vector<int> lds(COUNT_LDS_INTS);
    g_visit = visit, g_hw = hw, g_K = K;
    if (visit) g_cells.assign((size_t)planes * K * hw, 0);
    CView v{};
    v.x = in.x, v.y = in.y, v.thr = in.thr, v.dir = in.dir, v.counts = counts.data(), v.invalid = invalid.data();
    v.M = M, v.T = T, v.F = F, v.hw = hw, v.K = K, v.lds = lds.data();
    for (v.plane = 0; v.plane < planes; ++v.plane)
        for (v.chunk = 0; v.chunk < chunks(hw); ++v.chunk) counts_group(v);
    int rc = 0;
    if (visit) {
        for (long long c : g_cells)
            if (c != 1) rc = 5;  // every cell of every plane once per threshold (the synthetic fields hold no NaN)
        for (long long p = 0; p < planes && !rc; ++p)
            for (int k = 0; k < K; ++k) {
                long long n = 0;
                for (int b = 0; b < bins(M); ++b) {
                    const long long c = counts[((size_t)p * K + k) * bins(M) + b];
                    if (c < 0) rc = 6;
                    n += c;
                }
                if (n != hw || invalid[p] != 0) rc = rc ? rc : 7;  // the derived bin (0, 0) makes the bins add up to the plane
            }
    } else {
        rc = write_file(a[9], counts);
        if (!rc) rc = write_file(a[10], invalid);
    }
    release(in);
    return rc;
}

static void fss_group(FView& v) {
    poison(v.lds, FSS_LDS_BYTES, 0xA5);
    const Geo g = geo_of(v.H, v.W, v.R, v.tile);
    PHASE(f_zero(v, t))
    for (int d = 0; d <= v.M; ++d) {
        unsigned short* sat = d == 0 ? sat0_of(v) : satm_of(v);
        PHASE(f_load(v, g, t, d))
        PHASE(f_scan_rows(sat, g, t))
        PHASE(f_scan_cols(sat, g, t))
        PHASE(f_sums(v, g, t, sat, d))
        PHASE(f_flush(v, t, d))
    }
    std::vector<EnsThread> ens(THREADS);
    PHASE(f_ensemble_take(v, g, t, ens[t]))
    PHASE(f_ensemble_put(v, g, t, ens[t]))
    PHASE(f_scan_rows(sate_of(v), g, t))
    PHASE(f_scan_cols(sate_of(v), g, t))
    PHASE(f_sums(v, g, t, sate_of(v), v.M + 1))
    PHASE(f_flush(v, t, v.M + 1))
}

static int run_fss(char** a, int argc, bool visit) {
    if (argc < 7) return 1;
    const int M = atoi(a[0]), T = atoi(a[1]), F = atoi(a[2]), H = atoi(a[3]), W = atoi(a[4]), K = atoi(a[5]), S = atoi(a[6]);
    if (S < 1 || S > MAX_S || argc != 7 + S + (visit ? 0 : 5)) return 1;
    int radii[MAX_S] = {0};
    for (int s = 0; s < S; ++s) radii[s] = atoi(a[7 + s]);
    if (!fss_supported(H, W, M, K, radii, S) || T < 1 || F < 1) return 3;
    char** files = a + 7 + S;
    const int hw = H * W, R = max_radius(radii, S);
    const size_t ny = (size_t)T * F * hw;
    Inputs in;
    if (visit) in = synthetic(M, T, F, hw, K);
    else in.x = read_file<float>(files[0], M * ny), in.y = read_file<float>(files[1], ny), in.thr = read_file<float>(files[2], (size_t)F * K), in.dir = read_file<int>(files[3], (size_t)F * K);
    const long long planes = (long long)T * F;
    std::vector<long long> sums((size_t)planes * K * S * (M + 2) * 2, 0);  // the launcher zeroes it
    std::vector<unsigned char> lds(FSS_LDS_BYTES + 16);
    g_visit = visit, g_H = H, g_W = W, g_hw = hw, g_K = K, g_S = S, g_M = M;
    if (visit) {
        g_loads.assign((size_t)(M + 1) * hw, 0), g_sums.assign((size_t)(M + 2) * S * hw, 0);
        g_corners.assign((size_t)S * (H + 1) * (W + 1), 0);
    }
    FView v{};
    v.x = in.x, v.y = in.y, v.thr = in.thr, v.dir = in.dir, v.out = sums.data();
    v.M = M, v.T = T, v.F = F, v.H = H, v.W = W, v.K = K, v.S = S, v.R = R;
    for (int s = 0; s < MAX_S; ++s) v.radii.r[s] = s < S ? radii[s] : 0;
    v.lds = (unsigned char*)(((size_t)lds.data() + 15) / 16 * 16);
    const int nt = tiles_y(H) * tiles_x(W);
    for (v.plane = 0; v.plane < planes; ++v.plane)
        for (v.k = 0; v.k < K; ++v.k)
            for (v.tile = 0; v.tile < nt; ++v.tile) fss_group(v);
    int rc = g_bad ? 8 : 0;
    if (visit && !rc) {
        const long long each = planes * K;
        for (long long c : g_sums)
            if (c != each) rc = 5;  // every cell once per row and radius
        // a cell is staged by every tile whose halo reaches it: said again here, from the tile grid alone
        const int Rx = (R + 3) / 4 * 4;
        for (int y = 0; y < H && !rc; ++y)
            for (int x = 0; x < W; ++x) {
                long long n = 0;
                for (int ty = 0; ty < H; ty += TILE)
                    for (int tx = 0; tx < W; tx += TILE)
                        n += (y >= ty - R && y < (ty + TILE < H ? ty + TILE : H) + R && x >= tx - Rx && x < (tx + TILE < W ? tx + TILE : W) + Rx) ? 1 : 0;
                for (int d = 0; d <= M; ++d)
                    if (g_loads[(size_t)d * hw + y * W + x] != n * each) rc = 6;
            }
        // the corners of the windows clipped to the domain, counted directly
        for (int s = 0; s < S && !rc; ++s) {
            std::vector<long long> want((size_t)(H + 1) * (W + 1), 0);
            const int r = radii[s];
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const int a0 = y - r > 0 ? y - r : 0, a1 = y + r + 1 < H ? y + r + 1 : H, b0 = x - r > 0 ? x - r : 0, b1 = x + r + 1 < W ? x + r + 1 : W;
                    ++want[a0 * (W + 1) + b0], ++want[a0 * (W + 1) + b1], ++want[a1 * (W + 1) + b0], ++want[a1 * (W + 1) + b1];
                }
            for (size_t i = 0; i < want.size(); ++i)
                if (g_corners[(size_t)s * want.size() + i] != want[i] * each) rc = 7;
        }
    } else if (!rc) {
        rc = write_file(files[4], sums);
    }
    release(in);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 13 && !strcmp(argv[1], "counts")) return run_counts(argv + 2, false);
    if (argc == 7 && !strcmp(argv[1], "visit_counts")) return run_counts(argv + 2, true);
    if (argc >= 3 && !strcmp(argv[1], "fss")) return run_fss(argv + 2, argc - 2, false);
    if (argc >= 3 && !strcmp(argv[1], "visit_fss")) return run_fss(argv + 2, argc - 2, true);
    return 1;
}
