// Host driver for csrc/objects_maps.h: runs the phases of object_tables_kernel one thread after the other, workgroup by workgroup
// (tests/test_objects_cpu.py: the index maps and the link / flatten arithmetic of csrc/objects.hip without a GPU).
//   host_objects check H W connectivity max_objects
// builds, inside the program, the adversarial planes of a labeller -- empty, full, checkerboard, two blocks that touch at a corner, a
// comb whose teeth join on the last row, a U, nested rings, a spiral, a serpentine, random fields at three densities, NaNs -- for
// M = 2 members and a truth, T = 2 times, F = 2 variables and K = 3 thresholds of mixed directions, runs every plane's workgroup and
// compares all four tables with a plain flood fill written here.  Through OB_VISIT_LOAD it also counts that every workgroup stages
// every cell of its plane exactly once and nothing else.  The bit-mask helpers run_start / run_end are held against a cell-by-cell
// walk.  Every other plane's links are made in the opposite thread order.  LDS is filled with a pattern before every workgroup, so a slot nobody zeroed shows.  Exit status 0, or a number that says what
// differed.  It has its own main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"
#include <algorithm>

static long long g_plane = -1;
static int g_hw = 0, g_bad = 0;
static std::vector<int> g_seen;
static void visit_load(long long b, int cell) {
    if (b != g_plane || cell < 0 || cell >= g_hw) { g_bad = 1; return; }
    ++g_seen[(size_t)cell];
}
#define OB_VISIT_LOAD(b, cell) visit_load(b, cell)
#include "objects_maps.h"
using namespace objects;

enum Kind { EMPTY, FULL, CHECKER, DIAGONAL, COMB, U_SHAPE, RINGS, SPIRAL, SERPENTINE, RANDOM30, RANDOM59, RANDOM80, NANS, KINDS };

static unsigned g_rng = 12345u;
static float uniform() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (float)(g_rng >> 8) / 16777216.f;
}

static void spiral(std::vector<char>& g, int H, int W) {
    int i = 0, j = 0, di = 0, dj = 1;
    auto in = [&](int a, int b) { return a >= 0 && a < H && b >= 0 && b < W; };
    g[0] = 1;
    for (int guard = 0; guard < 4 * H * W + 8; ++guard) {
        bool moved = false;
        for (int turn = 0; turn < 2 && !moved; ++turn) {
            const int ni = i + di, nj = j + dj, mi = i + 2 * di, mj = j + 2 * dj;
            if (in(ni, nj) && !g[ni * W + nj] && !(in(mi, mj) && g[mi * W + mj])) {
                i = ni, j = nj, g[i * W + j] = 1, moved = true;
            } else {
                const int t = di;
                di = dj, dj = -t;
            }
        }
        if (!moved) return;
    }
}

// the values of one plane: +1 is the event of the two-valued kinds, mirrored where flip; variable f is moved by 10 f and scaled by 1 + f
static void make(int kind, int H, int W, bool flip, int f, float* out) {
    std::vector<char> g((size_t)H * W, 0);
    if (kind == SPIRAL) spiral(g, H, W);
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            char e = 0;
            const int r = std::min(std::min(i, H - 1 - i), std::min(j, W - 1 - j));
            switch (kind) {
                case EMPTY: e = 0; break;
                case FULL: e = 1; break;
                case CHECKER: e = (i + j) % 2 == 0; break;
                case DIAGONAL: e = (i < H / 2 && j < W / 2) || (i >= H / 2 && j >= W / 2); break;
                case COMB: e = j % 2 == 0 || i == H - 1; break;
                case U_SHAPE: e = j == 0 || j == W - 1 || i == H - 1; break;
                case RINGS: e = r % 2 == 0; break;
                case SPIRAL: e = g[i * W + j]; break;
                case SERPENTINE: e = i % 2 == 0 || (i % 4 == 1 && j == W - 1) || (i % 4 == 3 && j == 0); break;
                case RANDOM30: e = uniform() < 0.30f; break;
                case RANDOM59: case NANS: e = uniform() < 0.59f; break;
                case RANDOM80: e = uniform() < 0.80f; break;
            }
            float v = 10.f * f + (1.f + f) * (e ? 1.f : -1.f);
            if (kind == NANS && uniform() < 0.06f) v = __builtin_nanf("");
            out[i * W + (flip ? W - 1 - j : j)] = v;
        }
}

struct Tables {
    std::vector<long long> plane, hist, invalid;
    std::vector<int> objs;
};

// the definition, as a flood fill in row-major order: the first cell of a fill is the label, the fills come in label order
static void fill_plane(const float* src, float thr, int above, int H, int W, int conn, int max_objects, long long* plane, long long* hist, int* objs) {
    const int hw = H * W;
    std::vector<char> todo((size_t)hw);
    for (int n = 0; n < hw; ++n) todo[n] = (char)event_of(src[n], thr, above);
    for (int s = 0; s < max_objects; ++s) objs[s * 8] = -1;
    std::vector<int> stack;
    long long count = 0;
    for (int n0 = 0; n0 < hw; ++n0) {
        if (!todo[n0]) continue;
        todo[n0] = 0, stack.assign(1, n0);
        int area = 0, si = 0, sj = 0, i0 = H, i1 = -1, j0 = W, j1 = -1;
        while (!stack.empty()) {
            const int c = stack.back(), i = c / W, j = c % W;
            stack.pop_back();
            ++area, si += i, sj += j;
            i0 = std::min(i0, i), i1 = std::max(i1, i), j0 = std::min(j0, j), j1 = std::max(j1, j);
            for (int di = -1; di <= 1; ++di)
                for (int dj = -1; dj <= 1; ++dj) {
                    if ((di == 0 && dj == 0) || (conn == 4 && di != 0 && dj != 0)) continue;
                    const int a = i + di, b = j + dj;
                    if (a < 0 || a >= H || b < 0 || b >= W || !todo[a * W + b]) continue;
                    todo[a * W + b] = 0, stack.push_back(a * W + b);
                }
        }
        plane[1] += area, plane[2] = std::max(plane[2], (long long)area), plane[4] += si, plane[5] += sj;
        plane[3] += i0 == 0 || j0 == 0 || i1 == H - 1 || j1 == W - 1 ? 1 : 0;
        int bin = 0;
        while ((2 << bin) <= area) ++bin;
        ++hist[bin];
        if (count < max_objects) {
            int* o = objs + count * 8;
            o[0] = n0, o[1] = area, o[2] = si, o[3] = sj, o[4] = i0, o[5] = i1, o[6] = j0, o[7] = j1;
        }
        ++count;
    }
    plane[0] = count;
}

// run_start and run_end against a walk over single cells, on a random mask, every event cell of every row
static int check_runs(int H, int W) {
    const int hw = H * W;
    std::vector<unsigned> bits((size_t)words(hw), 0u);
    for (int n = 0; n < hw; ++n)
        if (uniform() < 0.7f) bits[n >> 5] |= 1u << (n & 31);
    for (int n = 0; n < hw; ++n) {
        if (!bit_of(bits.data(), n)) continue;
        const int lo = n / W * W, hi = lo + W;
        int s = n, e = n + 1;
        while (s > lo && bit_of(bits.data(), s - 1)) --s;
        while (e < hi && bit_of(bits.data(), e)) ++e;
        if (run_start(bits.data(), lo, n) != s || run_end(bits.data(), n, hi) != e) return 10;
    }
    return 0;
}

static int check(int H, int W, int conn, int max_objects) {
    const int M = 2, T = 2, F = 2, K = 3, D = M + 1, hw = H * W, B = bins(hw);
    if (!supported(H, W, K, conn, max_objects)) return 3;
    if (int rc = check_runs(H, W)) return rc;
    if (area_bin(1) != 0 || area_bin(3) != 1 || area_bin(4) != 2 || area_bin(16384) != 14 || bins(16384) != MAX_BINS || bins(4) != 3) return 11;
    const size_t ny = (size_t)T * F * hw, nx = (size_t)M * ny, planes = (size_t)D * T * F * K;
    float *x = alloc16<float>(nx), *y = alloc16<float>(ny), *thr = alloc16<float>((size_t)F * K);
    int* dir = alloc16<int>((size_t)F * K);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < K; ++k) thr[f * K + k] = 10.f * f + (1.f + f) * (-0.5f + 0.5f * k), dir[f * K + k] = (f * K + k) % 2 == 0;
    unsigned char* lds = alloc16<unsigned char>(LDS_BYTES);
    int rc = 0;
    for (int kind = 0; kind < KINDS && !rc; ++kind) {
        for (int d = 0; d < D; ++d)
            for (int t = 0; t < T; ++t)
                for (int f = 0; f < F; ++f) make(kind, H, W, (d + t) % 2 == 1, f, (d == 0 ? y : x + (size_t)(d - 1) * ny) + ((size_t)t * F + f) * hw);
        Tables got, want;
        for (Tables* tb : {&got, &want}) {
            tb->plane.assign(planes * 6, tb == &got ? -77 : 0), tb->hist.assign((size_t)D * F * K * B, 0);
            tb->invalid.assign((size_t)D * T * F, tb == &got ? -77 : 0), tb->objs.assign(planes * max_objects * 8 + 1, tb == &got ? -77 : 0);
        }
        want.objs.back() = -77;  // the entry behind the list stays what it was
        View v{};
        v.x = x, v.y = y, v.thr = thr, v.dir = dir, v.plane = got.plane.data(), v.area_hist = got.hist.data();
        v.objects = max_objects ? got.objs.data() : nullptr, v.invalid = got.invalid.data();
        v.D = D, v.T = T, v.F = F, v.H = H, v.W = W, v.K = K, v.connectivity = conn, v.max_objects = max_objects, v.lds = lds;
        for (v.b = 0; v.b < (long long)planes && !rc; ++v.b) {
            poison(lds, LDS_BYTES, (unsigned char)0x55);
            g_plane = v.b, g_hw = hw, g_seen.assign((size_t)hw, 0);
            PHASE(o_zero(v, t))
            PHASE(o_stage(v, t))
            PHASE(o_label(v, t))
            if (v.b % 2 == 0) {
                PHASE(o_link(v, t))
            } else {  // the links in the opposite order: the minimum labels make the result independent of it
                for (int t = THREADS - 1; t >= 0; --t) o_link(v, t);
            }
            PHASE(o_flatten(v, t))
            PHASE(o_rank1(v, t))
            PHASE(o_rank2(v, t))
            PHASE(o_rank3(v, t))
            PHASE(o_runs(v, t))
            PHASE(o_roots(v, t))
            PHASE(o_store(v, t))
            for (int c : g_seen)
                if (c != 1) rc = 5;  // every cell of the plane staged once
            const int k = (int)(v.b % K), f = (int)(v.b / K % F), t = (int)(v.b / K / F % T), d = (int)(v.b / K / F / T);
            if (k_of(v) != k || f_of(v) != f || t_of(v) != t || d_of(v) != d) rc = 6;
            const float* src = (d == 0 ? y : x + (size_t)(d - 1) * ny) + ((size_t)t * F + f) * hw;
            if (source_of(v) != src) rc = 6;
            fill_plane(src, thr[f * K + k], dir[f * K + k], H, W, conn, max_objects, want.plane.data() + v.b * 6,
                       want.hist.data() + (((size_t)d * F + f) * K + k) * B, want.objs.data() + v.b * max_objects * 8);
            long long nan = 0;
            for (int n = 0; n < hw; ++n) nan += src[n] != src[n] ? 1 : 0;
            want.invalid[((size_t)d * T + t) * F + f] = nan;
        }
        if (g_bad) rc = 8;
        if (!rc && got.plane != want.plane) rc = 20 + kind;
        if (!rc && got.hist != want.hist) rc = 40 + kind;
        if (!rc && got.objs != want.objs) rc = 60 + kind;
        if (!rc && got.invalid != want.invalid) rc = 80 + kind;
    }
    free(x), free(y), free(thr), free(dir), free(lds);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "check")) return check(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    return 1;
}
