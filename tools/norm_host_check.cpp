// Host check of the kernel bodies of tobac_flow_amd/csrc/norm_kernels.h: the same text compiled for the CPU and run lane
// after lane, workgroup after workgroup, on exactly-sized heap buffers, in the launch geometry of norm_methods.hip.
// Meant for AddressSanitizer + UBSan as well as for the plain build of tests/test_norm_cases_cpu.py:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/norm_host_check.cpp -o norm_host_check
//   ./norm_host_check <manifest>
//
// The manifest has one case per line:
//   name method H W flags vmin vmax max_std quantiles size exact input expected
// `input` is a raw file of 2 H W float32 (frame 0, frame 1), `expected` one of 2 H W bytes.  An exact case must match
// byte for byte; any other within the rounding class's cap (no byte off by more than 1, at most 0.1 % of the bytes off).
// Lanes run one after the other, so the atomics are plain read-modify-writes and a barrier is the end of a loop over
// the lanes; what is checked is indexing and arithmetic.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define __host__
#define __device__
#define __restrict__
static unsigned atomicAdd(unsigned *p, unsigned v) { unsigned o = *p; *p = o + v; return o; }

#include "../tobac_flow_amd/csrc/norm_kernels.h"

template <typename T> static std::vector<T> read_raw(const std::string &path, size_t count)
{
    std::vector<T> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read((char *)v.data(), (std::streamsize)(count * sizeof(T)));
    if (!f || f.gcount() != (std::streamsize)(count * sizeof(T))) { printf("cannot read %zu elements from %s\n", count, path.c_str()); exit(2); }
    return v;
}

static NmPartial tree(std::vector<NmPartial> &s)
{
    for (int o = NM_LANES / 2; o > 0; o >>= 1)
        for (int t = 0; t < o; t++) s[t] = nm_combine(s[t], s[t + o]);
    return s[0];
}

static void reduce(const float *f0, const float *f1, int64_t n, int method, const TfNormParams &p, int stage, NmState &st)
{
    int64_t g = (2 * n + NM_LANES * 16 - 1) / (NM_LANES * 16);
    g = g < 1 ? 1 : g > NM_MAX_PARTIALS ? NM_MAX_PARTIALS : g;
    std::vector<NmPartial> part((size_t)g), s(NM_LANES);
    const double mean = stage ? st.sum / (double)st.n : 0.0;
    for (int64_t b = 0; b < g; b++) {
        for (int t = 0; t < NM_LANES; t++) s[t] = nm_reduce_lane(f0, f1, n, b * NM_LANES + t, g * NM_LANES, stage != 0, mean);
        part[(size_t)b] = tree(s);
    }
    for (int t = 0; t < NM_LANES; t++) {
        s[t] = nm_empty();
        for (int64_t i = t; i < g; i += NM_LANES) s[t] = nm_combine(s[t], part[(size_t)i]);
    }
    nm_finish(method, p, stage, tree(s), st);
}

static void local_linear(const float *f0, const float *f1, int H, int W, const TfNormParams &p, const NmState &st, uint8_t *o0, uint8_t *o1)
{
    const int64_t n = (int64_t)H * W;
    const NmWindow kx = nm_window(p.size, W), ky = nm_window(p.size, H);
    const int sets = p.size >= 3 ? 1 : 2;
    std::vector<std::vector<float>> planes(4 * sets, std::vector<float>((size_t)n));
    std::vector<float> A((size_t)W), B((size_t)W);
    NmPlanes pl[2];
    for (int f = 0; f < sets; f++) {
        const float *src0 = f0, *src1 = f1;
        if (sets == 2 && (p.size == 1 || f == 0)) { src0 = f ? f1 : f0; src1 = nullptr; }
        float *rmin = planes[4 * f].data(), *rmax = planes[4 * f + 1].data(), *hmin = planes[4 * f + 2].data(), *hmax = planes[4 * f + 3].data();
        for (int y = 0; y < H; y++) {
            const int64_t row = (int64_t)y * W;
            for (int t = 0; t < NM_LANES; t++) nm_row_load<false>(t, src0 + row, src1 ? src1 + row : nullptr, W, st.mean, A.data());
            for (int t = 0; t < NM_LANES; t++) nm_row_scan<false>(t, W, kx, A.data(), B.data());
            for (int t = 0; t < NM_LANES; t++) nm_row_emit<false>(t, W, kx, A.data(), B.data(), rmin + row);
            for (int t = 0; t < NM_LANES; t++) nm_row_load<true>(t, src0 + row, src1 ? src1 + row : nullptr, W, st.mean, A.data());
            for (int t = 0; t < NM_LANES; t++) nm_row_scan<true>(t, W, kx, A.data(), B.data());
            for (int t = 0; t < NM_LANES; t++) nm_row_emit<true>(t, W, kx, A.data(), B.data(), rmax + row);
        }
        const int64_t lanes = ((int64_t)W * ((H + ky.w - 1) / ky.w) + NM_LANES - 1) / NM_LANES * NM_LANES;
        for (int64_t l = 0; l < lanes; l++) nm_col_suffix_lane(l, H, W, ky, rmin, rmax, hmin, hmax);
        pl[f] = NmPlanes{rmin, rmax, hmin, hmax};
    }
    if (sets == 1) pl[1] = pl[0];
    const int64_t lanes = ((int64_t)W * nm_col_chunks(H, ky) + NM_LANES - 1) / NM_LANES * NM_LANES;
    for (int64_t l = 0; l < lanes; l++) nm_col_finish_lane(l, H, W, ky, pl[0], pl[1], sets == 1, f0, f1, st.mean, o0, o1);
}

static void uniform(const float *f0, const float *f1, int64_t n, const TfNormParams &p, const NmState &st, uint8_t *o0, uint8_t *o1)
{
    const int Q = (int)p.quantiles, R = 2 * (Q + 1);
    std::vector<unsigned> resid(R), prefix(R), active(R), hist((size_t)R * NM_BINS), newp(R), cnt(NM_LANES), part(NM_LANES);
    std::vector<unsigned> lds_active(NM_MAX_RANKS), lds_hist(NM_LDS_SLOTS * NM_BINS);
    std::vector<int> slot(R);
    std::vector<double> gamma(Q + 1), edges(Q + 1);
    int nactive = 0;
    NmSelect sel{resid.data(), prefix.data(), active.data(), slot.data(), &nactive, gamma.data(), edges.data(), hist.data()};
    for (int k = 0; k < (Q + NM_LANES) / NM_LANES * NM_LANES; k++) nm_plan_lane(k, Q, st.n, sel);
    int64_t groups = (2 * n + NM_LANES * 32 - 1) / (NM_LANES * 32); if (groups > 1024) groups = 1024;
    for (int pass = 0; pass < 3; pass++) {
        std::fill(hist.begin(), hist.end(), 0u);
        for (int64_t b = 0; b < groups; b++) {
            std::copy(active.begin(), active.begin() + nactive, lds_active.begin());
            std::fill(lds_hist.begin(), lds_hist.end(), 0u);
            for (int t = 0; t < NM_LANES; t++)
                nm_hist_lane(f0, f1, n, b * NM_LANES + t, groups * NM_LANES, pass, lds_active.data(), nactive, lds_hist.data(), hist.data());
            for (int t = 0; t < NM_LANES; t++) nm_hist_flush(t, nactive, lds_hist.data(), hist.data());
        }
        for (int sl = 0; sl < nactive; sl++) {
            unsigned *h = hist.data() + (size_t)sl * NM_BINS;
            for (int t = 0; t < NM_LANES; t++) rs_scan_sum(t, h, part.data());
            for (int t = 0; t < NM_LANES; t++) rs_scan_write(t, h, part.data());
        }
        for (int t = 0; t < NM_LANES; t++) nm_resolve_digit(t, R, pass, sel, newp.data());
        for (int t = 0; t < NM_LANES; t++) nm_resolve_count(t, R, newp.data(), cnt.data());
        for (int t = 0; t < NM_LANES; t++) nm_resolve_slots(t, R, sel, newp.data(), cnt.data());
    }
    for (int k = 0; k < (Q + NM_LANES) / NM_LANES * NM_LANES; k++) nm_edge_lane(k, Q, sel, newp.data());
    int64_t blocks = (n + NM_LANES - 1) / NM_LANES; if (blocks > 4096) blocks = 4096;
    for (int64_t l = 0; l < blocks * NM_LANES; l++) nm_uniform_map_lane(f0, f1, n, l, blocks * NM_LANES, edges.data(), Q + 1, st.lo, st.hi, o0, o1);
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: norm_host_check <manifest>\n"); return 2; }
    std::ifstream manifest(argv[1]);
    std::string line;
    int failures = 0, cases = 0;
    // keys: order-preserving, and back
    const float vals[] = {-INFINITY, -3.5f, -1e-40f, -0.0f, 0.0f, 1e-40f, 2.25f, INFINITY};
    for (size_t a = 0; a + 1 < sizeof vals / sizeof *vals; a++)
        if (!(rs_key(vals[a]) < rs_key(vals[a + 1])) || rs_unkey(rs_key(vals[a])) != vals[a]) { printf("FAILED key order at %zu\n", a); failures++; }
    while (std::getline(manifest, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string name, input, expected;
        int method, H, W, exact;
        TfNormParams p;
        in >> name >> method >> H >> W >> p.flags >> p.vmin >> p.vmax >> p.max_std >> p.quantiles >> p.size >> exact >> input >> expected;
        if (!in) { printf("bad manifest line: %s\n", line.c_str()); return 2; }
        const int64_t n = (int64_t)H * W;
        const std::vector<float> x = read_raw<float>(input, (size_t)(2 * n));
        const std::vector<uint8_t> want = read_raw<uint8_t>(expected, (size_t)(2 * n));
        std::vector<uint8_t> got((size_t)(2 * n), 0xAA);
        const float *f0 = x.data(), *f1 = x.data() + n;
        NmState st;
        std::memset(&st, 0, sizeof st);
        reduce(f0, f1, n, method, p, 0, st);
        if (method == TF_NORM_Z_SCORE) reduce(f0, f1, n, method, p, 1, st);
        if (method == TF_NORM_LOCAL_LINEAR) local_linear(f0, f1, H, W, p, st, got.data(), got.data() + n);
        else if (method == TF_NORM_UNIFORM) uniform(f0, f1, n, p, st, got.data(), got.data() + n);
        else {
            int64_t blocks = (n + NM_LANES - 1) / NM_LANES; if (blocks > 4096) blocks = 4096;
            for (int64_t l = 0; l < blocks * NM_LANES; l++) nm_map_lane(method, f0, f1, n, l, blocks * NM_LANES, st, got.data(), got.data() + n);
        }
        int64_t differ = 0; int largest = 0;
        for (int64_t i = 0; i < 2 * n; i++) {
            const int d = std::abs((int)got[(size_t)i] - (int)want[(size_t)i]);
            differ += d != 0; largest = std::max(largest, d);
        }
        const bool ok = exact ? differ == 0 : (largest <= 1 && (double)differ <= 1e-3 * (double)(2 * n));
        printf("%s %s: %lld of %lld bytes differ, largest step %d (%s)\n", ok ? "ok" : "FAILED", name.c_str(), (long long)differ, (long long)(2 * n),
               largest, exact ? "exact" : "capped");
        failures += !ok; cases++;
    }
    printf(failures ? "%d FAILURES\n" : "norm host check: %d failures", failures);
    printf(" in %d cases\n", cases);
    return failures != 0 || cases == 0;
}
