"""The switches a large system flips, forced on small matrices: non-temporal vector loads and stores (on by themselves
only above 256 MB of vectors), launches that do not alternate their direction, one or three streams instead of two
(one by itself only above 1.6e6 site-vectors) and strip-ordered tiles (only when the L2 budget asks for them), for the
five drivers of the Clenshaw family: bdg_fermi_blocks, bdg_apply_series, bdg_green_moments, bdg_green_local_moments and
bdg_moment_matrix.  None of them changes an arithmetic operation, so the result must not change by one bit: no
reference is needed, only the default run of the same handle."""

import numpy as np
import pytest

from bodge_amd import correlation as corr

import fermi_cases as cases

pytestmark = pytest.mark.gpu

M = 40  # coefficients / moments of every case


# ------------------------------------------------------------------ one small case per entry point
def _fermi_blocks(system, solver):
    """33 random colours in 4 components: three batches, the last one ragged."""
    colours, n_colours = cases.random_colours(system.lattice.size, 33), 33
    coef = cases.fermi_coefficients(system, cases.TEMPERATURE, M)
    return solver.fermi_blocks(cases.scale_of(system), coef, colours, n_colours, 4, *cases.pattern_of(system))


def _apply_series(system, solver):
    """150 vectors and two functions: 300 columns, several batches at every lane width."""
    rng = np.random.default_rng(6)
    coef = (rng.standard_normal((M, 2)) + 1j * rng.standard_normal((M, 2))) / (1 + np.arange(M))[:, None]
    x = rng.standard_normal((150, solver.dim)) + 1j * rng.standard_normal((150, solver.dim))
    return solver.apply_series(cases.scale_of(system), coef, x / np.linalg.norm(x, axis=1, keepdims=True))


def _green_moments(system, solver):
    n = system.lattice.size
    rows = np.concatenate([4 * j + np.arange(4) for j in (n // 2, 1)])
    return solver.green_moments(cases.scale_of(system), M, rows, np.array([n // 2, n - 1, 0], dtype=np.int32))


def _green_local_moments(system, solver):
    sites = np.random.default_rng(7).permutation(system.lattice.size).astype(np.int32)
    return solver.green_local_moments(cases.scale_of(system), M, sites, 4)


def _moment_matrix(system, solver):
    jx = corr.as_operator(system, corr.current_operator(system, 0))
    rng = np.random.default_rng(8)
    x = rng.standard_normal((5, solver.dim)) + 1j * rng.standard_normal((5, solver.dim))
    return solver.moment_matrix(cases.scale_of(system), M, jx, jx, x=x / np.linalg.norm(x, axis=1, keepdims=True))


ENTRY_POINTS = {
    "fermi_blocks": _fermi_blocks,
    "apply_series": _apply_series,
    "green_moments": _green_moments,
    "green_local_moments": _green_local_moments,
    "moment_matrix": _moment_matrix,
}
PERF_FLAG = {"fermi_blocks": "clenshaw", "apply_series": "apply", "green_moments": "green",
             "green_local_moments": "green_local", "moment_matrix": "correlation"}
STREAMED = ("fermi_blocks", "apply_series")  # the drivers that run their batches side by side (BODGE_AMD_STREAMS)

SETTINGS = [(entry, switch, value) for entry in ENTRY_POINTS
            for switch, value in [("BODGE_AMD_STREAM_VECTORS", "1"), ("BODGE_AMD_STREAM_VECTORS", "2"),
                                  ("BODGE_AMD_STREAM_VECTORS", "3"), ("BODGE_AMD_ALTERNATE", "0")]
            + ([("BODGE_AMD_STREAMS", "1"), ("BODGE_AMD_STREAMS", "3")] if entry in STREAMED else [])]


# ------------------------------------------------------------------ memory hints, direction, streams
@pytest.mark.parametrize("name", ["dictionary", "disordered_complex"])
@pytest.mark.parametrize("entry,switch,value", SETTINGS)
def test_switch_does_not_change_one_bit(name, entry, switch, value, knobs):
    system = cases.SYSTEMS[name]()
    solver = system._solver()
    default = ENTRY_POINTS[entry](system, solver)
    before = solver.perf()
    assert before[PERF_FLAG[entry]] > 0 and before["launches"] >= M - 1 and np.abs(default).max() > 1e-3
    if entry in STREAMED:
        assert before["streams"] == 2 and before["launches"] >= 3 * (M - 1)  # at least three batches on two streams
    knobs.set(switch, value)
    switched = ENTRY_POINTS[entry](system, solver)
    after = solver.perf()
    print(name, entry, switch, value, np.abs(switched - default).max())
    assert np.array_equal(switched, default)
    assert after["launches"] == before["launches"] and after["lanes_per_row"] == before["lanes_per_row"]
    if switch == "BODGE_AMD_STREAMS":
        assert after["streams"] == int(value)
    knobs.unset(switch)
    assert np.array_equal(ENTRY_POINTS[entry](system, solver), default)  # ... and two identical calls agree


# ------------------------------------------------------------------ strip-ordered tiles
@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_strip_ordered_tiles_do_not_change_one_bit(entry, knobs):
    """900 block rows in planes of 150 (test_gpu_parity.test_strip_ordered_tiles_do_not_change_results forces the strips
    the same way): the geometry hint only permutes the order in which the row tiles are processed."""
    system = cases.SYSTEMS["strips_6x150"]()
    solver = system._solver()
    solver.set_lattice_shape((0, 0, 0))
    natural = ENTRY_POINTS[entry](system, solver)
    before = solver.perf()
    assert before["strip_rows"] == 0 and before[PERF_FLAG[entry]] > 0
    assert before["grid"] >= cases.tiles_of(900, before["lanes_per_row"])  # one tile per workgroup
    solver.set_lattice_shape((6, 150, 1))
    knobs.set("BODGE_AMD_L2_BUDGET", "4096")  # absurdly small: forces the narrowest strips
    strips = ENTRY_POINTS[entry](system, solver)
    after = solver.perf()
    print(entry, after["strip_rows"], after["lanes_per_row"], np.abs(strips - natural).max())
    assert 0 < after["strip_rows"] < 150
    assert after["launches"] == before["launches"] and after["lanes_per_row"] == before["lanes_per_row"]
    assert np.array_equal(strips, natural)
    if entry == "fermi_blocks":
        # No dense reference at this size; the restatement is sparse and cheap.  Bound of the distance: each of the M
        # steps of the recurrence adds at most 32 roundings of 2^-53 to an entry (a row of at most 7 blocks of 4 products
        # and sums, the three terms of the recurrence), relative to the largest entry of the vectors, which Clenshaw's
        # recurrence of a Chebyshev series does not amplify.
        coef = cases.fermi_coefficients(system, cases.TEMPERATURE, M)
        restated = cases.restated_blocks(system, cases.scale_of(system), coef, cases.random_colours(900, 33), 33, 4,
                                         *cases.pattern_of(system))
        bound = M * 32 * 2.0 ** -53 * max(1.0, np.abs(restated).max())
        print(entry, "device - restated", np.abs(strips - restated).max(), "bound", bound)
        assert np.abs(restated).max() > 0.1 and np.abs(strips - restated).max() <= bound
