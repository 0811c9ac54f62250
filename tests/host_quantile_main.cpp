// Host driver for csrc/quantile_core.h: runs the phases of the two kernels of csrc/quantile.hip one thread after the other, workgroup
// by workgroup, pass by pass (tests/test_quantiles_cpu.py: the slab map, the key, the slot logic and the interpolation without a GPU).
//   host_quantile visit  n_rep T F hw slabs owner_x.i32 owner_y.i32
//   host_quantile select n_rep T F hw with_truth Q skipna slabs x.f32 y.f32 q.f64 out.f64 stats.f32 nvalid.i64
// `visit` fills x and y with their own indices, so what a workgroup loaded says where it read: owner[k] is the one data set that
// loaded value k (-1: nobody, -2: loaded more than once), in every one of the three passes; it also checks that the pass-0 table of
// every data set sums to n.  It has its own main, so it is built with -fsanitize=address,undefined and run directly.
#include "host_main.h"
#include "quantile_core.h"
using namespace qnt;

struct Run {
    const float *x, *y;
    long long n_rep;
    int T, F, hw, Q, skipna, slabs;
    const double* q;
    std::vector<int>* owner;  // visit mode: refilled by every pass
    std::vector<int> owner0;  // visit mode: what pass 0 left
    int rc = 0;
};

// the whole call: memset, then three times (count over D x slabs workgroups, locate over D workgroups)
static void select(Run& r, std::vector<double>& out, std::vector<float>& stats, std::vector<long long>& nvalid) {
    const long long n_x = r.n_rep * r.F, D = n_x + (r.y ? r.F : 0), n = (long long)r.T * r.hw;
    const int R = 2 * r.Q;
    const Layout lay = layout(D, r.Q);
    unsigned char* scratch = (unsigned char*)aligned_alloc(16, (size_t)lay.total);  // exactly the bytes the launcher asks for
    memset(scratch, 0xA5, (size_t)lay.total);
    memset(scratch, 0, (size_t)lay.zeroed);
    unsigned char* lds = (unsigned char*)aligned_alloc(16, ((size_t)(count_lds_bytes(0, r.Q) > count_lds_bytes(1, r.Q) ? count_lds_bytes(0, r.Q) : count_lds_bytes(1, r.Q)) + 15) / 16 * 16);
    std::vector<long long> part((size_t)MAX_RANKS * LOCATE_THREADS);
    unsigned newpre[MAX_RANKS];
    int isfirst[MAX_RANKS];
    for (int pass = 0; pass < 3; ++pass) {
        if (r.owner) std::fill(r.owner->begin(), r.owner->end(), -1);
        for (long long b = 0; b < D * r.slabs; ++b) {
            poison(lds, (size_t)count_lds_bytes(pass, r.Q), 0x5A);  // a counter nobody zeroed shows
            CView v{};
            v.x = r.x, v.y = r.y, v.n_x = n_x, v.ds = b / r.slabs, v.slab = (int)(b % r.slabs), v.slabs = r.slabs, v.T = r.T, v.F = r.F, v.hw = r.hw;
            v.pass = pass, v.R = R, v.owner = r.owner ? r.owner->data() : nullptr;
            v.nan = (long long*)(scratch + lay.nan) + v.ds;
            v.pre = (const unsigned*)(scratch + lay.pre) + v.ds * R;
            v.tab = scratch + lay.tab + v.ds * BINS0;
            v.hist = (int*)lds;
            if (pass == 0) {
                v.table = (long long*)(scratch + lay.table0) + v.ds * BINS0;
                v.lnan = v.hist + BINS0;
            } else {
                v.table = (long long*)(scratch + (pass == 1 ? lay.table1 : lay.table2)) + v.ds * R * BINS;
                const int ns = ((const int*)(scratch + lay.ns))[v.ds];
                v.ns = ns < 0 ? 0 : ns > R ? R : ns;
                v.lpre = (unsigned*)(v.hist + R * BINS), v.ltab = (unsigned char*)(v.lpre + R), v.lnan = (int*)(v.ltab + BINS0);
                if (v.ns == 0) continue;
            }
            for (int t = 0; t < THREADS; ++t) c_zero(v, t);
            for (int t = 0; t < THREADS; ++t) pass == 0 ? c_count<true>(v, t) : c_count<false>(v, t);
            for (int t = 0; t < THREADS; ++t) c_flush(v, t);
        }
        if (r.owner) {
            for (int o : *r.owner)
                if (o < 0 && !(pass > 0 && o == -1)) r.rc = 5;  // pass 0 loads every value once; later passes never twice
            if (pass == 0) r.owner0 = *r.owner;
            if (pass == 0)
                for (long long d = 0; d < D; ++d) {
                    long long sum = 0;
                    for (int i = 0; i < BINS0; ++i) sum += ((long long*)(scratch + lay.table0))[d * BINS0 + i];
                    if (sum != n) r.rc = 6;
                }
        }
        for (long long d = 0; d < D; ++d) {
            LView v{};
            v.ds = d, v.n = n, v.Q = r.Q, v.R = R, v.pass = pass, v.skipna = r.skipna, v.q = r.q;
            v.table = pass == 0 ? (const long long*)(scratch + lay.table0) + d * BINS0
                                : (const long long*)(scratch + (pass == 1 ? lay.table1 : lay.table2)) + d * R * BINS;
            v.nan = (const long long*)(scratch + lay.nan) + d;
            v.res = (long long*)(scratch + lay.res) + d * R;
            v.pre = (unsigned*)(scratch + lay.pre) + d * R;
            v.rslot = (int*)(scratch + lay.rslot) + d * R;
            v.ns = (int*)(scratch + lay.ns) + d;
            v.tab = scratch + lay.tab + d * BINS0;
            v.out = out.data(), v.stats = stats.data(), v.nvalid = nvalid.data();
            v.part = part.data(), v.newpre = newpre, v.isfirst = isfirst;
            for (auto& p : part) p = -(1LL << 60);  // a sum nobody wrote shows
            l_open(v);
            for (int t = 0; t < LOCATE_THREADS; ++t) l_sums(v, t);
            for (int t = 0; t < LOCATE_THREADS; ++t) l_find(v, t);
            if (pass == 2) {
                for (int t = 0; t < LOCATE_THREADS; ++t) l_final(v, t);
                continue;
            }
            for (int t = 0; t < LOCATE_THREADS; ++t) l_mark(v, t);
            for (int t = 0; t < LOCATE_THREADS; ++t) l_slots(v, t);
        }
    }
    free(lds), free(scratch);
}

static int visit(char** a) {
    Run r{};
    r.n_rep = atoll(a[0]), r.T = atoi(a[1]), r.F = atoi(a[2]), r.hw = atoi(a[3]), r.slabs = atoi(a[4]);
    r.Q = 2, r.skipna = 1;
    if (!supported(r.hw, r.Q) || r.n_rep < 1 || r.T < 1 || r.F < 1 || r.slabs < 1) return 3;
    const size_t nx = (size_t)r.n_rep * r.T * r.F * r.hw, ny = (size_t)r.T * r.F * r.hw;
    if (nx + ny >= (1u << 24)) return 3;  // an index must be an fp32
    float *x = alloc16<float>(nx), *y = alloc16<float>(ny);
    for (size_t k = 0; k < nx; ++k) x[k] = (float)k;
    for (size_t k = 0; k < ny; ++k) y[k] = (float)(nx + k);
    const long long D = (r.n_rep + 1) * r.F;
    const double q[2] = {0.0, 1.0};
    std::vector<int> owner(nx + ny, -1);
    std::vector<double> out((size_t)D * r.Q);
    std::vector<float> stats((size_t)D * r.Q * 2);
    std::vector<long long> nvalid((size_t)D);
    r.x = x, r.y = y, r.q = q, r.owner = &owner;
    select(r, out, stats, nvalid);
    if (r.rc) return r.rc;
    // the select ran on the indices themselves: the minimum and the maximum of every data set are its first and last index
    for (long long d = 0; d < D; ++d) {
        const long long rep = d / r.F, f = d % r.F;
        const long long lo = d < r.n_rep * r.F ? (rep * r.T * r.F + f) * r.hw : (long long)nx + f * r.hw;
        const long long hi = lo + (long long)(r.T - 1) * r.F * r.hw + r.hw - 1;
        if (stats[(size_t)d * 4] != (float)lo || stats[(size_t)d * 4 + 3] != (float)hi || nvalid[(size_t)d] != (long long)r.T * r.hw) return 7;
    }
    owner = r.owner0;
    std::vector<int> ox(owner.begin(), owner.begin() + nx), oy(owner.begin() + nx, owner.end());
    const int rc = write_file(a[5], ox) | write_file(a[6], oy);
    free(x), free(y);
    return rc;
}

static int select_mode(char** a) {
    Run r{};
    r.n_rep = atoll(a[0]), r.T = atoi(a[1]), r.F = atoi(a[2]), r.hw = atoi(a[3]);
    const bool with_y = atoi(a[4]);
    r.Q = atoi(a[5]), r.skipna = atoi(a[6]), r.slabs = atoi(a[7]);
    if (!supported(r.hw, r.Q) || r.n_rep < 1 || r.T < 1 || r.F < 1 || r.slabs < 1) return 3;
    const size_t nx = (size_t)r.n_rep * r.T * r.F * r.hw, ny = (size_t)r.T * r.F * r.hw;
    float *x = read_file<float>(a[8], nx), *y = with_y ? read_file<float>(a[9], ny) : nullptr;
    double* q = read_file<double>(a[10], r.Q);
    const long long D = (r.n_rep + (with_y ? 1 : 0)) * r.F;
    std::vector<double> out((size_t)D * r.Q, -7.25);
    std::vector<float> stats((size_t)D * r.Q * 2, -7.25f);
    std::vector<long long> nvalid((size_t)D, -7);
    r.x = x, r.y = y, r.q = q;
    select(r, out, stats, nvalid);
    const int rc = r.rc | write_file(a[11], out) | write_file(a[12], stats) | write_file(a[13], nvalid);
    free(x), free(y), free(q);
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 9 && !strcmp(argv[1], "visit")) return visit(argv + 2);
    if (argc == 16 && !strcmp(argv[1], "select")) return select_mode(argv + 2);
    return 1;
}
