// Host driver for csrc/escore_core.h: runs the phases of the kernels one thread after the other, workgroup by workgroup
// (tests/test_escore_cpu.py: the index maps, the arithmetic and the fold order of csrc/escore.hip without a GPU).
//   host_escore pairs M planes hw x.f32 y.f32 d2.f64
//   host_escore vario M planes H W R order2 x.f32 y.f32 V.f64
//   host_escore visit_pairs M planes hw
//   host_escore visit_vario M planes H W R
// `visit_pairs` fills x and y with their own indices, so what a workgroup staged in LDS says where it read: it asserts that every cell
// of every row of every plane is fetched exactly once, by a workgroup of its own plane, and that every pair of every plane is written
// exactly once.  `visit_vario` counts the (cell, offset) pairs the threads take up and asserts that every pair with both cells inside
// the field is visited exactly once and no other, and that the halo holds the field's values where it lies inside.  Both exit with the
// number of the failed check.  The program has its own main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"

static std::vector<int>* g_visits = nullptr;  // [plane][offset][cell]
static long long g_cells = 0, g_offsets = 0;
#define ESC_VISIT(plane, cell, offset) \
    if (g_visits) ++(*g_visits)[(size_t)(((plane) * g_offsets + (offset)) * g_cells + (cell))]
#include "escore_core.h"
using namespace escore;

// -------------------------------------------------------------------------------------------------------------------- pairs

// one workgroup of escore_pairs_kernel; fetched (if given) counts who staged what
static int pairs_group(PView& v, std::vector<int>* fetched, size_t nx) {
    std::vector<PThread> th(THREADS);
    poison(v.lds, p_lds_bytes(v.M), 0xff);  // NaNs: a slot nobody wrote that reaches a sum shows
    PHASE(p_stage(v, t))
    if (fetched) {
        const float* rows = (const float*)v.lds;
        for (int r = 0; r <= v.M; ++r)
            for (int c = 0; c < P_CHUNK; ++c) {
                const long long cell = (long long)v.chunk * P_CHUNK + c;
                const float got = rows[r * P_PITCH + c];
                if (cell >= v.hw) {
                    if (got != 0.f) return 7;
                    continue;
                }
                const long long at = r == 0 ? (long long)nx + v.plane * v.hw + cell : ((long long)(r - 1) * v.planes + v.plane) * v.hw + cell;
                if (got != (float)at) return 5;
                ++(*fetched)[(size_t)at];
            }
    }
    PHASE(p_pairs_of_tile(v, th[t], t))
    PHASE(p_stash(v, th[t], t))
    PHASE(p_fold_store(v, t))
    return 0;
}

static int run_pairs(char** a, bool visit) {
    const int M = atoi(a[0]), hw = atoi(a[2]);
    const long long planes = atoll(a[1]);
    if (!p_supported(hw, M) || planes < 1) return 3;
    const size_t ny = (size_t)planes * hw, nx = (size_t)M * ny;
    if (visit && nx + ny >= (1u << 24)) return 3;  // an index must be an fp32
    float *x, *y;
    if (visit) {
        x = alloc16<float>(nx), y = alloc16<float>(ny);
        for (size_t k = 0; k < nx; ++k) x[k] = (float)k;
        for (size_t k = 0; k < ny; ++k) y[k] = (float)(nx + k);
    } else {
        x = read_file<float>(a[3], nx), y = read_file<float>(a[4], ny);
    }
    const int nc = p_chunks(hw), P = p_pairs(M);
    std::vector<double> d2((size_t)planes * P, -7.25), partial((size_t)(p_scratch_bytes(planes, hw, M) / 8), -7.25);
    std::vector<unsigned char> lds(p_lds_bytes(M) + 16);
    std::vector<int> fetched(nx + ny, 0);
    PView v{};
    v.x = x, v.y = y, v.out = nc > 1 ? partial.data() : d2.data(), v.planes = planes, v.M = M, v.hw = hw;
    v.lds = lds.data() + (16 - (size_t)lds.data() % 16) % 16;
    int rc = 0;
    for (v.plane = 0; v.plane < planes && !rc; ++v.plane)
        for (v.chunk = 0; v.chunk < nc && !rc; ++v.chunk) rc = pairs_group(v, visit ? &fetched : nullptr, nx);
    if (!rc && visit) {
        for (int f : fetched)
            if (f != 1) rc = 6;  // a value nobody fetched, or fetched twice
        for (double p : partial)
            if (p == -7.25 || p != p) rc = 8;  // a partial nobody wrote (indices differ, so no distance is -7.25)
        if (nc == 1)
            for (double p : d2)
                if (p == -7.25 || p != p) rc = 8;
    }
    if (nc > 1)
        for (long long e = 0; e < planes * P; ++e) p_fold(partial.data(), d2.data(), e, nc, P);
    if (!rc && !visit) rc = write_file(a[5], d2);
    free(x), free(y);
    return rc;
}

// -------------------------------------------------------------------------------------------------------------------- variogram

template <int ORDER2>
static int vario_group(VView& v, bool visit, size_t nx) {
    poison(v.lds, v_lds_bytes(v.R, v.M), 0xff);
    PHASE(v_stage(v, t))
    if (visit) {  // the patch holds the field's own indices inside the field and zeros outside
        const float* patch = (const float*)v.lds;
        const int ph = v_patch_h(v.R), pw = v_patch_w(v.R);
        const int i0 = (v.tile / v_tiles_w(v.W)) * V_TH, j0 = (v.tile % v_tiles_w(v.W)) * V_TW - v.R;
        const long long hw = (long long)v.H * v.W;
        for (int r = 0; r <= v.M; ++r)
            for (int pi = 0; pi < ph; ++pi)
                for (int pj = 0; pj < pw; ++pj) {
                    const int i = i0 + pi, j = j0 + pj;
                    const float got = patch[(r * ph + pi) * pw + pj];
                    const bool inside = i < v.H && j >= 0 && j < v.W;
                    const long long at = (r == 0 ? (long long)nx + v.plane * hw : ((long long)(r - 1) * v.planes + v.plane) * hw) + (long long)i * v.W + j;
                    if (inside ? got != (float)at : got != 0.f) return 5;
                }
    }
    const int O = v_offsets(v.R);
    for (int o0 = 0; o0 < O; o0 += V_BATCH) {
        PHASE(v_terms<ORDER2>(v, t, o0))
        PHASE(v_fold_groups(v, t))
        PHASE(v_fold_store(v, t, o0))
    }
    return 0;
}

static int run_vario(char** a, bool visit) {
    const int M = atoi(a[0]), H = atoi(a[2]), W = atoi(a[3]), R = atoi(a[4]), order2 = visit ? 2 : atoi(a[5]);
    const long long planes = atoll(a[1]);
    if (!v_supported(H, W, R, M, order2) || planes < 1) return 3;
    const size_t hw = (size_t)H * W, ny = (size_t)planes * hw, nx = (size_t)M * ny;
    if (visit && nx + ny >= (1u << 24)) return 3;
    float *x, *y;
    if (visit) {
        x = alloc16<float>(nx), y = alloc16<float>(ny);
        for (size_t k = 0; k < nx; ++k) x[k] = (float)k;
        for (size_t k = 0; k < ny; ++k) y[k] = (float)(nx + k);
    } else {
        x = read_file<float>(a[6], nx), y = read_file<float>(a[7], ny);
    }
    const int nt = v_tiles(H, W), O = v_offsets(R);
    if (O % V_BATCH != 0) return 9;
    std::vector<double> V((size_t)planes * O * 3, -7.25), partial((size_t)(v_scratch_bytes(planes, H, W, R) / 8), -7.25);
    std::vector<unsigned char> lds(v_lds_bytes(R, M) + 16);
    std::vector<int> visits(visit ? (size_t)planes * O * hw : 0, 0);
    g_visits = visit ? &visits : nullptr, g_cells = (long long)hw, g_offsets = O;
    VView v{};
    v.x = x, v.y = y, v.out = nt > 1 ? partial.data() : V.data(), v.planes = planes, v.M = M, v.H = H, v.W = W, v.R = R;
    v.lds = lds.data() + (16 - (size_t)lds.data() % 16) % 16;
    int rc = 0;
    for (v.plane = 0; v.plane < planes && !rc; ++v.plane)
        for (v.tile = 0; v.tile < nt && !rc; ++v.tile)
            rc = order2 == 1 ? vario_group<1>(v, visit, nx) : order2 == 2 ? vario_group<2>(v, visit, nx) : vario_group<4>(v, visit, nx);
    if (!rc && visit) {
        for (long long pl = 0; pl < planes && !rc; ++pl)
            for (int o = 0; o < O && !rc; ++o) {
                int di, dj;
                v_offset_of(R, o, di, dj);
                if (!(di > 0 || (di == 0 && dj > 0)) || abs(di) > R || abs(dj) > R) rc = 10;
                for (int i = 0; i < H && !rc; ++i)
                    for (int j = 0; j < W; ++j) {
                        const int want = i + di < H && j + dj >= 0 && j + dj < W ? 1 : 0;
                        if (visits[(size_t)((pl * O + o) * (long long)hw + i * W + j)] != want) rc = 6;
                    }
            }
        for (double p : partial)
            if (p == -7.25 || p != p) rc = rc ? rc : 8;
    }
    if (nt > 1)
        for (long long e = 0; e < planes * O * 3; ++e) v_fold(partial.data(), V.data(), e, nt, O * 3);
    if (!rc && !visit) rc = write_file(a[8], V);
    free(x), free(y);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 8 && !strcmp(argv[1], "pairs")) return run_pairs(argv + 2, false);
    if (argc == 5 && !strcmp(argv[1], "visit_pairs")) return run_pairs(argv + 2, true);
    if (argc == 11 && !strcmp(argv[1], "vario")) return run_vario(argv + 2, false);
    if (argc == 7 && !strcmp(argv[1], "visit_vario")) return run_vario(argv + 2, true);
    return 1;
}
