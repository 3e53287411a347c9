"""Keeps the staging sweep complete (tests/staging_sweep_cases.py, tests/test_gpu_staging_truth.py): every place in the
package that shares a cached device twin (`share=True`), remembers a result as one (`remember=True`), or calls the staging
layer directly (`_staging.upload(`, `_staging.download(`, `Prefetch(`) must be listed in the sweep's table with the case that
runs through it.  A new call site fails here until it has a case; a site that is gone fails until its line is removed."""
import os

import staging_sweep_cases as sweep

PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tobac_flow_amd")


def test_every_staging_site_of_the_package_has_a_sweep_case():
    found = sweep.scan_sites(PACKAGE)
    assert len(found) >= 20, sorted(found)                             # (the search itself works)
    missing, gone = found - set(sweep.SITES), set(sweep.SITES) - found
    assert not missing, f"staging sites without a sweep case in tests/staging_sweep_cases.SITES: {sorted(missing)}"
    assert not gone, f"tests/staging_sweep_cases.SITES lists sites the package no longer has: {sorted(gone)}"


def test_every_listed_case_exists_and_the_search_sees_a_planted_site(tmp_path):
    assert set(sweep.SITES.values()) <= set(sweep.CASES)
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "m.py").write_text(
        "import x\n\n\ndef f(a):\n    def inner():\n        return x.to_dev(a, share=True)\n    return inner()\n\n\n"
        "class C:\n    def g(self, a):\n        return x.to_host(a, remember=True)\n\n\nP = x.Prefetch([])\n")
    assert sweep.scan_sites(str(tmp_path)) == {("sub/m.py", "f"), ("sub/m.py", "C.g"), ("sub/m.py", "<module>")}
