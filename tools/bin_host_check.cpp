// Host check of the kernel body of tobac_flow_amd/csrc/bin_kernels.h (tf_bin_points): the same text compiled for the CPU,
// run lane after lane on exactly-sized heap buffers against plain loops, meant for AddressSanitizer + UBSan:
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/bin_host_check.cpp -o bin_host_check
//   ./bin_host_check
//
// Lanes run one after the other, so the atomics are plain read-modify-writes.  Checked: every load and store inside its
// buffer at every alignment and tail form; the bin of every point against a linear scan of the edges (uniform edges,
// float32-derived midpoints, a zero-width bin, points on and next to every edge, beyond both ends, +-inf, NaN) under both
// last-edge rules; masks, time windows, mirrored axes, both product types; counts exactly, sums within the summation-order
// bound 2 (n - 1) 2^-53 sum|term| per bin, one-term bins bit for bit.  The last part runs three frames of a 40000 x 40000
// grid -- flat indices beyond 2^32 -- in a sparse mapping of which only the touched pages ever exist.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <vector>
#include <sys/mman.h>

#define __host__
#define __device__
#define __forceinline__ inline
#define __restrict__
struct int4 { int32_t x, y, z, w; };
struct float4 { float x, y, z, w; };
struct double2 { double x, y; };
struct uchar4 { uint8_t x, y, z, w; };
template <typename T> static T atomicAdd(T *p, T v) { T o = *p; *p = o + v; return o; }
static unsigned long long atomicMin(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::min(o, v); return o; }
static unsigned long long atomicMax(unsigned long long *p, unsigned long long v) { unsigned long long o = *p; *p = std::max(o, v); return o; }
static uint32_t atomicOr(uint32_t *p, uint32_t v) { uint32_t o = *p; *p = o | v; return o; }

#include "../tobac_flow_amd/csrc/bin_kernels.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) printf("FAILED %s (line %d)\n", #c, __LINE__); failures++; } } while (0)

template <typename E> struct Buf {                                 // exactly-sized copy, `shift` elements past a 16-byte boundary
    std::vector<E> store; E *p;
    Buf(const std::vector<E> &v, int shift) : store(v.size() + shift), p(nullptr) { if (!v.empty()) std::memcpy(store.data() + shift, v.data(), v.size() * sizeof(E)); p = store.data() + shift; }
};

static void run_all_lanes(const TfBinPoints &P)
{
    const int64_t blocks = (P.n_points + LR_BLOCK - 1) / LR_BLOCK;
    for (int64_t b = 0; b < blocks; b++)
        for (int t = 0; t < 256; t++) {
            if (P.coord_dtype == TF_F32) bn_points_body<float>(b, t, P); else bn_points_body<double>(b, t, P);
        }
}

// ---- the plain statement: linear scans, points in their order --------------------------------------------------------------
static double plain_around(double v, int d, double scale) { return d > 0 ? std::nearbyint(v * scale) / scale : d < 0 ? std::nearbyint(v / scale) * scale : std::nearbyint(v); }
static float plain_around(float v, int d, double scale) { const float s = (float)scale; return d > 0 ? std::nearbyintf(v * s) / s : d < 0 ? std::nearbyintf(v / s) * s : std::nearbyintf(v); }

template <typename C>
static int64_t plain_bin(C vc, const std::vector<double> &e, int rule, int dec, double scale)
{
    const double v = (double)vc;
    int64_t n_le = 0;                                             // searchsorted(e, v, "right"): NaN sorts behind everything
    for (double x : e) n_le += (x <= v) || std::isnan(v);
    int64_t k = n_le - 1;
    const int64_t nb = (int64_t)e.size() - 1;
    if (rule == TF_BIN_RULE_NUMPY) { if (v == e.back()) k--; }
    else if (v >= e.back() && plain_around(vc, dec, scale) == plain_around((C)e.back(), dec, scale)) k--;
    return k >= 0 && k < nb ? k : -1;
}

static std::vector<double> make_edges(int kind, int64_t n_edges, std::mt19937 &rng)
{
    std::vector<double> e((size_t)n_edges);
    if (kind == 0) for (int64_t i = 0; i < n_edges; i++) e[(size_t)i] = -3.0 + 0.25 * (double)i;                  // uniform
    else if (kind == 1) {                                         // midpoints of float32 coordinates: not equidistant in double
        std::vector<float> c((size_t)n_edges - 1);
        for (size_t i = 0; i < c.size(); i++) c[i] = 0.151872f - 5.6e-05f * (float)i;
        std::reverse(c.begin(), c.end());
        e[0] = c[0]; e.back() = c.back();
        for (size_t i = 1; i + 1 < e.size(); i++) e[i] = ((double)c[i - 1] + (double)c[i]) / 2;
    } else if (kind == 2) {                                       // irregular, with a zero-width bin (NumPy rule only)
        double x = -1;
        for (int64_t i = 0; i < n_edges; i++) { e[(size_t)i] = x; x += (i % 5 == 2) ? 0.0 : 0.001 * (double)(1 + rng() % 900); }
    } else {                                                      // wide bins: a negative `decimals`
        double x = -1000;
        for (int64_t i = 0; i < n_edges; i++) { e[(size_t)i] = x; x += 250.0 * (double)(1 + rng() % 3); }
    }
    return e;
}

template <typename C>
static std::vector<C> make_coords(const std::vector<double> &e, int64_t n, int runs, std::mt19937 &rng)
{
    std::vector<C> v((size_t)n);
    const double lo = e.front(), hi = e.back(), inf = std::numeric_limits<double>::infinity();
    C held = (C)lo;
    for (int64_t i = 0; i < n; i++) {
        const unsigned r = rng() % 16;
        const double edge = e[rng() % e.size()];
        C c;
        if (runs && i % runs) c = held;                           // runs of equal bins of every length and phase
        else if (r < 6) c = (C)(lo + (hi - lo) * (double)(rng() % 100000) / 100000.0);
        else if (r == 6) c = (C)edge;
        else if (r == 7) c = std::nextafter((C)edge, (C)inf);
        else if (r == 8) c = std::nextafter((C)edge, (C)-inf);
        else if (r == 9) c = (C)hi;
        else if (r == 10) c = std::nextafter((C)hi, (C)inf);
        else if (r == 11) c = (C)(hi + 1e-9 * std::fabs(hi) + 1e-12);
        else if (r == 12) c = (C)(lo - 0.5);
        else if (r == 13) c = (C)(hi + 0.5);
        else if (r == 14) c = (rng() & 1) ? (C)inf : (C)-inf;
        else c = std::numeric_limits<C>::quiet_NaN();
        v[(size_t)i] = held = c;
    }
    return v;
}

struct Case { int nd, rule, edge_kind, value_dtype, weight_dtype, shift, runs; bool keep, keep_value, finite_value, windows; int flip; int64_t n; };

template <typename C>
static void one_case(const Case &cs, unsigned seed)
{
    std::mt19937 rng(seed);
    const int64_t n = cs.n;
    const int64_t ne[3] = {cs.n == 1003 ? 68 : 2 + (int64_t)(rng() % 9), 2 + (int64_t)(rng() % 6), 2 + (int64_t)(rng() % 4)};
    std::vector<std::vector<double>> edges;
    std::vector<std::vector<C>> coords;
    int64_t n_bins = 1;
    int dec[3] = {0, 0, 0};
    double scale[3] = {1, 1, 1};
    for (int d = 0; d < cs.nd; d++) {
        edges.push_back(make_edges(cs.edge_kind, ne[d], rng));
        coords.push_back(make_coords<C>(edges[d], n, cs.runs, rng));
        n_bins *= ne[d] - 1;
        if (cs.rule == TF_BIN_RULE_SCIPY) {
            double w = std::numeric_limits<double>::infinity();
            for (size_t i = 1; i < edges[d].size(); i++) w = std::min(w, edges[d][i] - edges[d][i - 1]);
            dec[d] = (int)(-std::log10(w)) + 6;
            scale[d] = std::pow(10.0, std::abs(dec[d]));
        }
    }
    const int64_t T = cs.windows ? 5 : 1;
    std::vector<int64_t> time((size_t)n), ws = {0, 10, 10, 30, 50}, we = {12, 20, 20, 30, 60};   // overlap, twice the same, empty, gap
    std::vector<uint8_t> keep((size_t)n), kv((size_t)n);
    std::vector<float> v32((size_t)n), w32((size_t)n);
    std::vector<double> v64((size_t)n), w64((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        time[(size_t)i] = (int64_t)(rng() % 64) - 2;
        keep[(size_t)i] = rng() % 5 != 0; kv[(size_t)i] = rng() % 3 != 0;
        float v = (float)((int)(rng() % 2000) - 1000) / 7.f, w = (float)(1 + rng() % 1000) / 3.f;
        { const unsigned r = rng() % 40; if (r == 0) v = NAN; else if (r == 1) v = INFINITY; }   // SciPy rule without finite_value: the status bit
        v32[(size_t)i] = v; v64[(size_t)i] = (double)v * 1.0000001; w32[(size_t)i] = w; w64[(size_t)i] = (double)w * 0.9999999;
    }
    Buf<uint8_t> K(keep, cs.shift), KV(kv, cs.shift);
    Buf<int64_t> TM(time, cs.shift), WS(ws, 0), WE(we, 0);
    Buf<float> V32(v32, cs.shift), W32(w32, cs.shift);
    Buf<double> V64(v64, cs.shift), W64(w64, cs.shift);
    std::vector<Buf<C>> CB;
    std::vector<Buf<double>> EB;
    for (int d = 0; d < cs.nd; d++) { CB.emplace_back(coords[d], cs.shift); EB.emplace_back(edges[d], 0); }
    const size_t cells = (size_t)(T * n_bins);
    std::vector<int32_t> count(cells, 0), count_v(cells, 0);
    std::vector<double> sum_w(cells, 0.0), sum_wv(cells, 0.0);
    uint32_t status = 0;

    TfBinPoints P;
    std::memset(&P, 0, sizeof(P));
    P.n_dims = cs.nd; P.coord_dtype = sizeof(C) == 4 ? TF_F32 : TF_F64; P.rule = cs.rule;
    P.value_dtype = cs.value_dtype < 0 ? 0 : cs.value_dtype; P.weight_dtype = cs.weight_dtype < 0 ? 0 : cs.weight_dtype;
    P.flags = cs.finite_value ? TF_BIN_FINITE_VALUE : 0; P.flip_mask = cs.flip & ((1 << cs.nd) - 1);
    P.n_points = n; P.n_frames = T;
    for (int d = 0; d < cs.nd; d++) { P.decimals[d] = dec[d]; P.round_scale[d] = scale[d]; P.n_edges[d] = ne[d]; P.coord[d] = CB[(size_t)d].p; P.edges[d] = EB[(size_t)d].p; }
    if (cs.keep) P.keep = K.p;
    if (cs.keep_value) P.keep_value = KV.p;
    if (cs.value_dtype == TF_F32) P.value = V32.p; else if (cs.value_dtype == TF_F64) P.value = V64.p;
    if (cs.weight_dtype == TF_F32) P.weight = W32.p; else if (cs.weight_dtype == TF_F64) P.weight = W64.p;
    if (cs.windows) { P.time = TM.p; P.win_start = WS.p; P.win_end = WE.p; }
    P.count = count.data(); P.count_v = count_v.data(); P.sum_w = sum_w.data();
    if (P.value) P.sum_wv = sum_wv.data();
    P.status = &status;
    run_all_lanes(P);

    // plain loops
    std::vector<int64_t> pc(cells, 0), pcv(cells, 0);
    std::vector<double> psw(cells, 0.0), pswv(cells, 0.0), abs_w(cells, 0.0), abs_wv(cells, 0.0);
    uint32_t want_status = 0;
    for (int64_t i = 0; i < n; i++) {
        if (cs.keep && !keep[(size_t)i]) continue;
        bool finite = true, inside = true, differ = false;
        int64_t bin = 0;
        for (int d = 0; d < cs.nd; d++) {
            const C c = coords[(size_t)d][(size_t)i];
            finite = finite && std::isfinite((double)c);
            const int64_t k = plain_bin<C>(c, edges[(size_t)d], cs.rule, dec[d], scale[d]);
            if (cs.rule == TF_BIN_RULE_SCIPY) differ = differ || (k >= 0) != (plain_bin<C>(c, edges[(size_t)d], TF_BIN_RULE_NUMPY, 0, 1) >= 0);
            inside = inside && k >= 0;
            const int64_t nb = ne[d] - 1;
            bin = bin * nb + (k < 0 ? 0 : ((P.flip_mask >> d) & 1) ? nb - 1 - k : k);
        }
        const double vd = cs.value_dtype == TF_F32 ? (double)v32[(size_t)i] : cs.value_dtype == TF_F64 ? v64[(size_t)i] : 0.0;
        const double wd = cs.weight_dtype == TF_F32 ? (double)w32[(size_t)i] : cs.weight_dtype == TF_F64 ? w64[(size_t)i] : 1.0;
        double prod = vd * wd;
        if (cs.value_dtype == TF_F32 && cs.weight_dtype != TF_F64) prod = (double)(v32[(size_t)i] * (cs.weight_dtype == TF_F32 ? w32[(size_t)i] : 1.f));
        for (int64_t f = 0; f < T; f++) {
            if (cs.windows && !(ws[(size_t)f] <= time[(size_t)i] && time[(size_t)i] < we[(size_t)f])) continue;
            bool with_value = !cs.keep_value || kv[(size_t)i];
            if (with_value && P.value && !std::isfinite(vd)) {
                if (cs.finite_value) with_value = false;
                else if (cs.rule == TF_BIN_RULE_SCIPY) { want_status |= TF_BIN_STATUS_VALUE; continue; }
            }
            if (cs.rule == TF_BIN_RULE_SCIPY && !finite) { want_status |= TF_BIN_STATUS_COORD; continue; }
            if (differ) want_status |= TF_BIN_STATUS_RULES_DIFFER;
            if (!inside) continue;
            const size_t at = (size_t)(f * n_bins + bin);
            pc[at]++;
            if (!with_value) continue;
            pcv[at]++; psw[at] += wd; pswv[at] += prod; abs_w[at] += std::fabs(wd); abs_wv[at] += std::fabs(prod);
        }
    }
    CHECK(status == want_status);
    const double u = std::ldexp(1.0, -53);
    auto close = [&](double got, double want, int64_t terms, double mag) {
        if (std::isnan(want) || std::isinf(want) || std::isinf(mag)) return std::isnan(got) == std::isnan(want) && (std::isnan(want) || got == want || std::isinf(mag));
        if (terms <= 1) return got == want;
        return std::fabs(got - want) <= 2.0 * (double)(terms - 1) * u * mag;
    };
    for (size_t at = 0; at < cells; at++) {
        CHECK(count[at] == pc[at]);
        CHECK(count_v[at] == pcv[at]);
        CHECK(close(sum_w[at], psw[at], pcv[at], abs_w[at]));
        if (P.value) CHECK(close(sum_wv[at], pswv[at], pcv[at], abs_wv[at]));
    }
}

// three frames of a 40000 x 40000 grid: 4.8e9 cells, flat indices beyond 2^32, in a sparse mapping
static void beyond_2_32()
{
    const int64_t side = 40000, T = 3, n_bins = side * side, n = 1003;
    const size_t bytes = (size_t)(T * n_bins) * sizeof(int32_t);
    void *map = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (map == MAP_FAILED) { printf("FAILED to map %zu sparse bytes\n", bytes); failures++; return; }
    std::vector<double> e((size_t)side + 1);
    for (int64_t i = 0; i <= side; i++) e[(size_t)i] = (double)i;
    std::mt19937 rng(99);
    std::vector<double> y((size_t)n), x((size_t)n);
    std::vector<int64_t> time((size_t)n), ws = {0, 10, 20}, we = {10, 20, 30};
    for (int64_t i = 0; i < n; i++) {
        y[(size_t)i] = (double)(side - 1 - (int64_t)(rng() % 7)) + 0.5; x[(size_t)i] = (double)(rng() % side) + 0.25;
        time[(size_t)i] = (int64_t)(rng() % 30);
    }
    Buf<double> Y(y, 0), X(x, 1), E(e, 0);
    Buf<int64_t> TM(time, 0), WS(ws, 0), WE(we, 0);
    TfBinPoints P;
    std::memset(&P, 0, sizeof(P));
    P.n_dims = 2; P.coord_dtype = TF_F64; P.rule = TF_BIN_RULE_NUMPY; P.n_points = n; P.n_frames = T;
    for (int d = 0; d < 2; d++) { P.round_scale[d] = 1; P.n_edges[d] = side + 1; P.edges[d] = E.p; }
    P.coord[0] = Y.p; P.coord[1] = X.p;
    P.time = TM.p; P.win_start = WS.p; P.win_end = WE.p;
    P.count = (int32_t *)map;
    run_all_lanes(P);
    std::map<uint64_t, int32_t> want;
    for (int64_t i = 0; i < n; i++)
        want[(uint64_t)(time[(size_t)i] / 10) * (uint64_t)n_bins + (uint64_t)y[(size_t)i] * (uint64_t)side + (uint64_t)x[(size_t)i]]++;
    int64_t found = 0, beyond = 0;
    for (const auto &cell : want) {
        beyond += cell.first > 0xffffffffull;
        CHECK(((const int32_t *)map)[cell.first] == cell.second);
        found += cell.second;
    }
    CHECK(found == n && beyond > 100);
    munmap(map, bytes);
}

int main()
{
    unsigned seed = 1;
    const int64_t sizes[] = {0, 1, 63, 64, 65, 1003, 4096, 4099, 2 * 4096 + 5};
    for (int64_t n : sizes)
        for (int nd = 1; nd <= 3; nd++)
            for (int rule = 0; rule < 2; rule++)
                for (int shift = 0; shift < 2; shift++) {
                    const int r = (int)(seed % 7);
                    Case cs;
                    cs.nd = nd; cs.rule = rule; cs.n = n; cs.shift = shift;
                    static const int scipy_kinds[] = {0, 1, 3}, value_types[] = {TF_F32, TF_F64, TF_F32, -1};
                    static const int weight_types[] = {TF_F32, TF_F64, -1, TF_F64, TF_F32}, run_lengths[] = {0, 3, 17, 70, 0, 300, 1};
                    cs.edge_kind = rule == TF_BIN_RULE_NUMPY ? (int)(seed % 4) : scipy_kinds[seed % 3];
                    cs.value_dtype = value_types[seed % 4];
                    cs.weight_dtype = weight_types[seed % 5];
                    cs.runs = run_lengths[r];
                    cs.keep = seed % 3 != 0; cs.keep_value = seed % 2 != 0; cs.finite_value = seed % 4 < 2;
                    cs.windows = seed % 3 != 1; cs.flip = (int)(seed % 8);
                    one_case<float>(cs, seed);
                    one_case<double>(cs, seed + 1000);
                    seed++;
                }
    beyond_2_32();
    printf(failures ? "%d FAILURES\n" : "bin host check: all equal (%d failures)\n", failures);
    return failures != 0;
}
