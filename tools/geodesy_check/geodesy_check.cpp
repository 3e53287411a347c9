// Host check of the arithmetic of tobac_flow_amd/csrc/geodesy_kernels.h: the same text that the gfx950 kernels run,
// compiled for the CPU with plain g++, so that the device arithmetic itself is checked against the oracles of
// tests/geodesy_cases.py without a device (tests/test_geodesy_cases_cpu.py builds and feeds it).
//
//   g++ -O2 -std=c++17 -ffp-contract=off -o geodesy_check tools/geodesy_check/geodesy_check.cpp
//   ./geodesy_check < cases.txt
//
// One case per input line, numbers in any form strtod reads (hex floats included); one output line per case, hex floats:
//   geod a rf lon1 lat1 lon2 lat2                  ->  az12 az21 dist failed
//   inv h lon_0 a rf sweep_y x y                   ->  lat lon
//   fwd h lon_0 a rf sweep_y lat lon               ->  x y
//   fwdalt h lon_0 a rf sweep_y lat lon alt        ->  x y
//   view mode s0 s1 s2 lat lon sx sy               ->  out0 out1
//   rule i n raw_prev raw_here                     ->  spacing
//   toecef a rf lon lat alt                        ->  X Y Z
//   fromecef a rf X Y Z                            ->  lon lat alt
//   geos2ecef h lon_0 a rf sweep_y x y             ->  X Y Z hit
//   parallax h lon_0 a rf sweep_y h_ltg a_ltg rf_ltg lla_a lla_rf lat lon   ->  dlon dlat x y alt hit
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define __host__
#define __device__

#include "../../tobac_flow_amd/csrc/geodesy_kernels.h"

static TfGeos geos_of(const std::vector<double> &v)
{
    TfGeos g;
    g.h = v[0]; g.lon_0 = v[1]; g.lat_0 = 0.0; g.a = v[2]; g.rf = v[3];
    g.sweep_y = (int32_t)v[4]; g.flags = 0;
    return g;
}

int main()
{
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        char *p = line, kind[16] = "";
        int used = 0;
        if (sscanf(p, "%15s%n", kind, &used) != 1) continue;
        p += used;
        std::vector<double> v;
        for (;;) {
            char *end;
            const double d = strtod(p, &end);
            if (end == p) break;
            v.push_back(d);
            p = end;
        }
        const std::string k(kind);
        const size_t need = k == "geod" ? 6 : k == "inv" || k == "fwd" ? 7 : k == "fwdalt" ? 8 : k == "view" ? 8 : k == "rule" ? 4 :
                            k == "toecef" || k == "fromecef" ? 5 : k == "geos2ecef" ? 7 : k == "parallax" ? 12 : 0;
        if (need == 0 || v.size() != need) { fprintf(stderr, "bad case: %s", line); return 2; }
        if (k == "geod") {
            const GdInverse r = gd_geod_inverse_one(v[0], v[1] != 0.0 ? 1.0 / v[1] : 0.0, v[2], v[3], v[4], v[5]);
            printf("%a %a %a %d\n", r.az12, r.az21, r.s, r.failed);
        } else if (k == "inv") {
            const GdGeos s = gd_geos_setup(geos_of(v));
            double ty, hy, lat, lon;
            gd_geos_row_terms(s, v[6], ty, hy);
            gd_geos_inverse_one(s, v[5], ty, hy, lat, lon);
            printf("%a %a\n", lat, lon);
        } else if (k == "fwd" || k == "fwdalt") {
            const GdGeos s = gd_geos_setup(geos_of(v));
            double x, y;
            if (k == "fwd") gd_geos_forward_one(s, v[5], v[6], x, y);
            else gd_geos_forward_alt_one(s, v[5], v[6], v[7], x, y);
            printf("%a %a\n", x, y);
        } else if (k == "view") {
            double a0, a1;
            gd_view_angles_one((int)v[0], &v[1], v[4], v[5], v[6], v[7], a0, a1);
            printf("%a %a\n", a0, a1);
        } else if (k == "toecef" || k == "fromecef") {
            const double f = v[1] != 0.0 ? 1.0 / v[1] : 0.0;
            double o0, o1, o2;
            if (k == "toecef") gd_geodetic_to_ecef_one(v[0], f, v[2], v[3], v[4], o0, o1, o2);
            else gd_ecef_to_geodetic_one(v[0], f, v[2], v[3], v[4], o0, o1, o2);
            printf("%a %a %a\n", o0, o1, o2);
        } else if (k == "geos2ecef") {
            double X, Y, Z;
            const bool hit = gd_geos_to_ecef_one(gd_geos_setup(geos_of(v)), v[5], v[6], X, Y, Z);
            printf("%a %a %a %d\n", X, Y, Z, (int)hit);
        } else if (k == "parallax") {
            TfGeos ltg = geos_of(v);
            ltg.h = v[5]; ltg.a = v[6]; ltg.rf = v[7];
            double dlon, dlat, x, y, alt;
            const bool hit = gd_glm_parallax_one(gd_parallax_setup(geos_of(v), ltg, v[8], v[9]), v[10], v[11], dlon, dlat, x, y, alt);
            printf("%a %a %a %a %a %d\n", dlon, dlat, x, y, alt, (int)hit);
        } else {
            printf("%a\n", gd_spacing_rule((int64_t)v[0], (int64_t)v[1], v[2], v[3]));
        }
    }
    return 0;
}
