"""Registers of the composed three-step sweep (no GPU: hipcc cross-compiles; tools/kernel_resources.py as in
test_kernel_resources.py, whose compiled table this shares within one session).

Every instance of cheb_sweep3_composed must build without scratch, within 256 VGPRs and at two waves per SIMD.  The
composed body drops the t_{n-1} prefetch of the halo lanes and one store level, so no dictionary form may need more
registers than its classic sibling cheb_sweep3<..., 0, 4>."""

import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    import kernel_resources

    return kernel_resources.collect()


def _row(resources, name):
    matches = [row for key, row in resources.items() if key.startswith(f"void bdg::{name}(")]
    assert len(matches) == 1, (name, [k for k in resources if name.split("<")[0] in k][:5])
    return matches[0]


@pytest.mark.timeout(600)
def test_composed_sweep_instances_fit_two_waves_per_simd_without_scratch(resources):
    count = 0
    for mode in ("RealPHMode", "ComplexPHMode"):
        for lanes in (2, 4):
            for reverse, gen in (("false", "false"), ("true", "false"), ("false", "true")):
                row = _row(resources, f"cheb_sweep3_composed<bdg::{mode}, {lanes}, {reverse}, {gen}>")
                classic = _row(resources, f"cheb_sweep3<bdg::{mode}, {lanes}, {reverse}, {gen}, 0, 4>")
                print(f"cheb_sweep3_composed<{mode}, {lanes}, {reverse}, {gen}>: {row['vgpr']} VGPRs, {row['scratch']} B scratch, "
                      f"{row['occupancy']} waves/SIMD (classic: {classic['vgpr']} VGPRs)")
                assert row["scratch"] == 0 and row["vgpr"] <= 256 and row["occupancy"] >= 2, (mode, lanes, reverse, gen, row)
                assert row["vgpr"] <= classic["vgpr"], (mode, lanes, reverse, gen, row, classic)
                count += 1
    assert count == 12
    # no other instance exists: the streamed forms and the full-block modes keep the classic body
    assert len([key for key in resources if "cheb_sweep3_composed<" in key]) == 12
