"""Generate tests/golden/binning_ref.npz: the inputs of tests/binning_cases.py and what NumPy and SciPy make of them.

    python tests/golden/make_binning_golden.py

The yardsticks of the point binning are the libraries themselves -- np.histogramdd, np.histogram2d,
scipy.stats.binned_statistic_dd and binned_statistic_2d -- called here in the argument patterns of the reference's
tobac_flow/glm.py:77-145 (per frame np.histogram2d(y, x, bins=(y_bins[::-1], x_bins))[0][::-1] over the flashes of the
files inside the frame's open window, -1 where no file is), tobac_flow/nexrad.py:80-231 (per site and frame two such
histograms and binned_statistic_dd(..., statistic="mean", expand_binnumbers=True), then the accumulation over sites with
NaN and -33) and scripts/grid_flux.py:65-73 (two binned_statistic_2d sums and their quotient).  The reference's own
modules cannot be imported for this: they need xarray, pyproj and pyart at import, none of which is installed, and
their functions take file names and datasets rather than arrays.  The loops in tests/binning_cases.py (glm_loop,
nexrad_site_loop, nexrad_regrid, flux_loop) are restatements of those lines over arrays, written for this repository.

Stored: every input, and the libraries' results.  Written with NumPy 2.2 and SciPy 1.15."""
import os
import sys

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import binning_cases as bc  # noqa: E402

out = {}

glm = bc.glm_case()
out.update({f"glm/{k}": v for k, v in glm.items()})
out["glm/grid"] = bc.glm_loop(glm)
assert (out["glm/grid"][1] == -1).all() and (out["glm/grid"][3] == 0).all() and out["glm/grid"][[0, 2, 4]].max() > 0

nex = bc.nexrad_case()
out.update({f"nexrad/{k}": nex[k] for k in ("goes_dates", "x_bins", "y_bins")})
stacks = []
for s, site in enumerate(nex["sites"]):
    out.update({f"nexrad/site{s}/{k}": v for k, v in site.items()})
    stacks.append(bc.nexrad_site_loop(site, nex))
    for name, stack in zip(("raw", "masked", "mean"), stacks[-1]):
        out[f"nexrad/site{s}/{name}"] = stack
out["nexrad/ref_grid"], out["nexrad/ref_mask"] = bc.nexrad_regrid(stacks)
assert out["nexrad/ref_grid"][0, 5, 7] == -33 and np.isnan(out["nexrad/ref_grid"]).any() and (stacks[1][2][3] == 0).all()
assert (stacks[1][0][3] > 0).any() and np.nanmax(out["nexrad/ref_grid"]) > 0

flux = bc.flux_case()
out.update({f"flux/{k}": v for k, v in flux.items() if k != "area64"})      # area64 is area widened
out["flux/mean_f32_weights"] = bc.flux_loop(flux, "area")
out["flux/mean_f64_weights"] = bc.flux_loop(flux, "area64")
assert np.isnan(out["flux/mean_f32_weights"]).any() and np.isfinite(out["flux/mean_f32_weights"]).any()

# the libraries called directly on scattered points: 1, 2 and 3 axes, with and without weights / values
for nd in (1, 2, 3):
    c = bc.scattered(500, nd, seed=40 + nd)
    for d in range(nd):
        out[f"scattered{nd}/coord{d}"], out[f"scattered{nd}/edges{d}"] = c["coords"][d], c["edges"][d]
    out[f"scattered{nd}/v64"], out[f"scattered{nd}/w64"] = c["v64"], c["w64"]
    out[f"scattered{nd}/histogramdd"] = np.histogramdd(c["coords"], bins=c["edges"])[0]
    out[f"scattered{nd}/histogramdd_weights"] = np.histogramdd(c["coords"], bins=c["edges"], weights=c["w64"])[0]
    for statistic in ("count", "sum", "mean"):
        out[f"scattered{nd}/binned_{statistic}"] = stats.binned_statistic_dd(c["coords"], c["v64"], statistic, bins=c["edges"])[0]
c = bc.scattered(500, 2, seed=42)
out["scattered2/histogram2d"] = np.histogram2d(c["coords"][0], c["coords"][1], bins=c["edges"])[0]
out["scattered2/binned_2d_mean"] = stats.binned_statistic_2d(c["coords"][0], c["coords"][1], c["v64"], "mean", bins=c["edges"])[0]

# the edge rules
edges = bc.coord_bin_edges(bc.abi_x())
for name, dtype in (("f32", np.float32), ("f64", np.float64)):
    pts = bc.edge_points(edges, dtype)
    out[f"edges/{name}_points"] = pts
    out[f"edges/{name}_numpy"] = np.histogramdd([pts], bins=[edges])[0]
    finite = bc.edge_points(edges, dtype, specials=False)
    out[f"edges/{name}_scipy"] = stats.binned_statistic_dd([finite], None, "count", bins=[edges])[0]
out["edges/edges"] = edges
out["zero_width/numpy"] = np.histogramdd([bc.ZERO_WIDTH_POINTS], bins=[bc.ZERO_WIDTH_EDGES])[0]
assert out["zero_width/numpy"].tolist() == [1, 0, 2]
for width in bc.SCIPY_WIDTHS:
    e, pts = bc.scipy_rounding_case(width)
    out[f"rounding/{width}_scipy"] = stats.binned_statistic_dd([pts], None, "count", bins=[e])[0]
    out[f"rounding/{width}_numpy"] = np.histogramdd([pts], bins=[e])[0]
    assert out[f"rounding/{width}_scipy"][-1] == 3 and out[f"rounding/{width}_numpy"][-1] == 1

path = os.path.join(HERE, "binning_ref.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
