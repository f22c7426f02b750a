"""The tile loops of the Clenshaw family with several tiles per workgroup: cheb_family and cheb_family_dict
(csrc/family.hpp) under every tail, and the dictionary loop fermi.hpp kept (cheb_clenshaw_dict).

On a production-size system a workgroup walks several tiles; on the small systems of the other tests it walks one
(their perf["grid"] >= tiles asserts say so).  Here BODGE_AMD_BLOCKS_PER_CU=1 caps the grid at one workgroup per CU on a
67 x 63 lattice (tests/family_tile_cases.py: 528 tiles at 32 lanes, the last one ragged), so the step to the next tile,
the prefetched row words and their hand-over, the sentinel past the last tile, the reuse of the per-wave LDS, the
reversed walk of the odd launches and the strip order at several positions all run more than once per launch.

The arithmetic of a block row does not depend on the workgroup that owns it, so for every driver but
bdg_green_state_moments (whose partial sums follow the grid) the reference is the run of the same handle with one tile
per workgroup (BODGE_AMD_BLOCKS_PER_CU=8), bit for bit: the rest of the suite ties that path to dense eigh.  The numpy
restatements on sparse H hold the multi-tile results independently of any device code."""

import numpy as np
import pytest

from bodge_amd import correlation as corr

import family_tile_cases as cases
import response_map_cases
from test_gpu_apply import ARITHMETIC
from test_gpu_green_states import rounding_bound as state_rounding_bound

pytestmark = pytest.mark.gpu

M = cases.M
N = int(np.prod(cases.SHAPE))
# form of the matrix -> (system of family_tile_cases, BODGE_AMD_DICT before upload, the arithmetic modes that differ)
FORMS = {
    "dictionary": ("uniform", None, sorted(ARITHMETIC)),
    "streamed": ("uniform", "0", sorted(ARITHMETIC)),               # the same real matrix without its dictionary
    "disordered": ("disordered", None, ["packed", "real_full"]),   # complex, streamed by itself: REAL=0 changes nothing
}


def _fresh(form, arithmetic, knobs):
    """A new system and handle under the switches of (form, arithmetic): the dictionary switch is read at upload."""
    name, dictionary, _ = FORMS[form]
    knobs.update(ARITHMETIC[arithmetic])
    if dictionary is not None:
        knobs.set("BODGE_AMD_DICT", dictionary)
    system = cases.SYSTEMS[name]()
    return name, system, system._solver()


def _assert_form(perf, flag, form, arithmetic, lanes):
    """The perf record says which kernel ran: the family, the form of the matrix, the arithmetic, the lanes."""
    name = FORMS[form][0]
    real = name == "uniform" and "complex" not in arithmetic
    # (no dictionary kernel in real arithmetic at 64 lanes: the streamed form runs, as test_gpu_fermi.py notes)
    dictionary = form == "dictionary" and not (real and lanes == 64)
    assert perf[flag] == (2 if dictionary else 1), (flag, perf[flag])
    assert (perf["dict_blocks"] > 0) == dictionary
    assert perf["real_arithmetic"] == (1 if real else 0)
    assert perf["ph_packed"] == (0 if arithmetic.endswith("full") else 1)
    assert perf["lanes_per_row"] == lanes, (perf["lanes_per_row"], lanes)


def _entry(entry, system, solver):
    return lambda: cases.ENTRY_POINTS[entry](system, solver)


def _one_tile(knobs, solver, call, lanes, n_sites=N):
    """The reference run: `call()` under BODGE_AMD_BLOCKS_PER_CU=8, (result, perf), one tile per workgroup asserted."""
    knobs.set("BODGE_AMD_BLOCKS_PER_CU", "8")
    result = call()
    perf = solver.perf()
    assert perf["lanes_per_row"] == lanes and perf["grid"] >= cases.tiles_of(n_sites, lanes), (perf["grid"], lanes)
    return result, perf


def _capped(knobs, solver, call, blocks_per_cu, lanes, n_sites=N, factor=2):
    """`call()` under BODGE_AMD_BLOCKS_PER_CU=n: (result, perf), with tiles > factor * grid asserted from perf."""
    knobs.set("BODGE_AMD_BLOCKS_PER_CU", str(blocks_per_cu))
    result = call()
    perf = solver.perf()
    tiles = cases.tiles_of(n_sites, lanes)
    assert perf["lanes_per_row"] == lanes and tiles > factor * perf["grid"], (tiles, perf["grid"], perf["lanes_per_row"])
    return result, perf


# ------------------------------------------------------------------ 1. bit equality across grids
GRID_CASES = [(entry, form, arithmetic, 32) for entry in cases.ENTRY_POINTS for form in FORMS for arithmetic in FORMS[form][2]]
GRID_CASES += [(entry, "dictionary", arithmetic, 64) for entry in cases.ENTRY_POINTS
               for arithmetic in ("complex_packed", "complex_full")]


@pytest.mark.parametrize("entry,form,arithmetic,lanes", GRID_CASES)
def test_several_tiles_per_workgroup_do_not_change_one_bit(entry, form, arithmetic, lanes, knobs):
    """One workgroup per CU (every workgroup walks 2 - 3 tiles at 32 lanes, 4 - 5 at 64), two per CU (a few workgroups
    take a second tile), the default grid, and one per CU without the alternating direction, against one tile per
    workgroup."""
    _, system, solver = _fresh(form, arithmetic, knobs)
    call = _entry(entry, system, solver)
    flag = cases.PERF_FLAG[entry]
    solver.set_lanes_per_row(lanes)
    try:
        reference, before = _one_tile(knobs, solver, call, lanes)
        _assert_form(before, flag, form, arithmetic, lanes)
        assert np.abs(reference).max() > 1e-3 and before["launches"] >= M - 1
        runs = {}
        runs["one workgroup per CU"] = _capped(knobs, solver, call, 1, lanes)
        runs["two workgroups per CU"] = _capped(knobs, solver, call, 2, lanes, factor=1)
        knobs.unset("BODGE_AMD_BLOCKS_PER_CU")
        runs["default grid"] = (call(), solver.perf())
        knobs.set("BODGE_AMD_ALTERNATE", "0")
        runs["one workgroup per CU, no alternation"] = _capped(knobs, solver, call, 1, lanes)
    finally:
        solver.set_lanes_per_row(0)
    for label, (result, perf) in runs.items():
        print(entry, form, arithmetic, lanes, label, "grid", perf["grid"], "tiles", cases.tiles_of(N, lanes),
              np.abs(result - reference).max())
        _assert_form(perf, flag, form, arithmetic, lanes)
        assert perf["launches"] == before["launches"] and perf["vector_steps"] == before["vector_steps"], label
        assert np.array_equal(result, reference), (label, np.abs(result - reference).max())


# ------------------------------------------------------------------ 2. lane widths
@pytest.mark.parametrize("form", ["dictionary", "streamed", "disordered"])
@pytest.mark.parametrize("arithmetic", ["packed", "complex_full"])
@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_apply_series_at_every_lane_width(form, arithmetic, lanes, knobs):
    """bdg_apply_series takes any width: 264, 528 and 1056 tiles for 256 workgroups.  No case is refused: the one
    form without an instance, the dictionary form in real arithmetic at 64 lanes, is no BDG_EINVAL in this family
    (make_family_plan asks dict_kernel, which has no such kernel, and plans the streamed form of that width, as
    bdg_fermi_blocks does in test_gpu_fermi.test_lane_widths_match_restatement_and_dense); _assert_form pins that the
    streamed kernel ran, and it is held to the same bit equality."""
    _, system, solver = _fresh(form, arithmetic, knobs)
    if FORMS[form][0] == "disordered" and arithmetic == "complex_full":
        arithmetic = "real_full"  # (a complex matrix: REAL=0 changes nothing, the record is that of PH=0)
    call = _entry("apply_series", system, solver)
    solver.set_lanes_per_row(lanes)
    try:
        reference, before = _one_tile(knobs, solver, call, lanes)
        capped, perf = _capped(knobs, solver, call, 1, lanes, factor=1 if lanes == 16 else 2)
    finally:
        solver.set_lanes_per_row(0)
    print(form, arithmetic, lanes, "grid", perf["grid"], "tiles", cases.tiles_of(N, lanes), np.abs(capped - reference).max())
    for record in (before, perf):
        _assert_form(record, "apply", form, arithmetic, lanes)
        assert record["launches"] == -(-70 // lanes) * M and record["vector_steps"] == 70 * M
    assert np.abs(reference).max() > 1e-3
    assert np.array_equal(capped, reference)


# ------------------------------------------------------------------ 3. against numpy, independent of the device code
LARGEST = {}  # entry -> the largest distance printed so far (the figure of DESIGN.md §10)


def _hold_to_restatement(label, entry, name, got):
    """Bound: 32·M·2⁻⁵³·max(1, max|restated|), derived in test_gpu_clenshaw_switches.py."""
    restated = cases.restated(entry, name)
    if entry == "green_local_moments":
        got = got[:, cases.local_positions()]
    bound = cases.rounding_bound(M, restated)
    distance = np.abs(got - restated).max()
    LARGEST[entry] = max(LARGEST.get(entry, 0.0), distance)
    print(*label, "device - restated", distance, "bound", bound, "largest so far", LARGEST[entry])
    assert got.shape == restated.shape and np.abs(restated).max() > 1e-3
    assert distance <= bound, (label, distance, bound)


@pytest.mark.parametrize("entry", sorted(cases.ENTRY_POINTS))
@pytest.mark.parametrize("form", ["dictionary", "disordered"])
def test_several_tiles_per_workgroup_match_the_numpy_restatement(entry, form, knobs):
    name, system, solver = _fresh(form, "packed", knobs)
    call = _entry(entry, system, solver)
    solver.set_lanes_per_row(32)
    try:
        got, perf = _capped(knobs, solver, call, 1, 32)
    finally:
        solver.set_lanes_per_row(0)
    _assert_form(perf, cases.PERF_FLAG[entry], form, "packed", 32)
    _hold_to_restatement((entry, form, "grid", perf["grid"]), entry, name, got)


# ------------------------------------------------------------------ 4. strip order x several tiles
@pytest.mark.parametrize("entry", sorted(cases.ENTRY_POINTS))
@pytest.mark.parametrize("form", ["dictionary", "disordered"])
def test_strip_ordered_tiles_over_several_positions_do_not_change_one_bit(entry, form, knobs):
    """tile_order read at every position of a workgroup's walk, forwards and backwards: strips of 8 rows in planes of 63
    (the narrowest: an L2 budget of 4 KB) against the natural order with one tile per workgroup."""
    _, system, solver = _fresh(form, "packed", knobs)
    call = _entry(entry, system, solver)
    solver.set_lanes_per_row(32)
    try:
        solver.set_lattice_shape((0, 0, 0))
        natural, before = _one_tile(knobs, solver, call, 32)
        assert before["strip_rows"] == 0
        solver.set_lattice_shape(cases.SHAPE)
        knobs.set("BODGE_AMD_L2_BUDGET", "4096")
        strips, perf = _capped(knobs, solver, call, 1, 32)
    finally:
        solver.set_lanes_per_row(0)
    print(entry, form, "strip rows", perf["strip_rows"], "grid", perf["grid"], np.abs(strips - natural).max())
    assert 0 < perf["strip_rows"] < cases.SHAPE[1]
    _assert_form(perf, cases.PERF_FLAG[entry], form, "packed", 32)
    assert perf["launches"] == before["launches"] and np.abs(natural).max() > 1e-3
    assert np.array_equal(strips, natural)


# ------------------------------------------------------------------ 5. green_state_moments
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("arithmetic", ["packed", "complex_full"])
def test_state_moments_are_carried_across_two_and_three_tiles(form, arithmetic, knobs):
    """What test_gpu_green_states.test_accumulators_are_carried_across_the_tiles_of_a_workgroup leaves out: 32 lanes (a
    tail's Column state over 2 - 3 tiles of every workgroup), the streamed form and complex arithmetic.  The partial sums
    follow the grid, so every run is held to the numpy restatement under that file's rounding bound instead."""
    _, system, solver = _fresh(form, arithmetic, knobs)
    states = cases.states_of(system)
    assert np.allclose(np.linalg.norm(states, axis=1), 1.0, rtol=1e-12)
    scale = cases.scale_of(system)
    expected = cases.restated_state_moments("uniform")
    bound = state_rounding_bound(M, N, expected)

    def call():
        return solver.green_state_moments(scale, M, states, 4)

    solver.set_lanes_per_row(32)
    try:
        runs = {}
        runs["one tile per workgroup"] = _one_tile(knobs, solver, call, 32)
        runs["one workgroup per CU"] = _capped(knobs, solver, call, 1, 32)
        knobs.set("BODGE_AMD_ALTERNATE", "0")
        runs["one workgroup per CU, no alternation"] = _capped(knobs, solver, call, 1, 32)
    finally:
        solver.set_lanes_per_row(0)
    real = "complex" not in arithmetic
    for label, (result, perf) in runs.items():
        distance = np.abs(result - expected).max()
        print(form, arithmetic, label, "grid", perf["grid"], "device - restated", distance, "bound", bound)
        assert perf["green_states"] == (2 if form == "dictionary" else 1) and perf["real_arithmetic"] == int(real)
        assert perf["ph_packed"] == (0 if arithmetic.endswith("full") else 1)
        assert perf["launches"] == M - 1 and perf["vector_steps"] == (M - 1) * 24  # six states: one batch
        assert np.abs(expected).max() > 0.1 and distance <= bound, (label, distance, bound)


# ------------------------------------------------------------------ 6. drivers that reuse apply's kernels
def _moment_matrix(system, solver):
    """5 random vectors, 16 moments: two panels of 16 rows of 8.6 MB."""
    jx = corr.as_operator(system, corr.current_operator(system, 0))
    x = cases.apply_vectors(system, 5)
    return solver.moment_matrix(cases.scale_of(system), 16, jx, jx, x=x)


def _response_map(system, solver):
    """A random operator on the four rows of an interior site, 64 target sites."""
    rows, a = response_map_cases.random_source(system)
    coef = response_map_cases.random_coefficients(M)
    return solver.response_map(cases.scale_of(system), rows, a, coef, cases.green_targets(system.lattice.size))


def _subspace_filter(system, solver):
    """40 start columns through a series of M real coefficients, read back."""
    coef = np.random.default_rng(12).standard_normal(M) / (1 + np.arange(M))
    solver.subspace_begin(40, seed=5)
    try:
        solver.subspace_filter(cases.scale_of(system), coef)
        return solver.subspace_read(0, 40)
    finally:
        solver.subspace_end()


REUSERS = {"moment_matrix": (_moment_matrix, "correlation"), "response_map": (_response_map, "response_map"),
           "subspace_filter": (_subspace_filter, "apply")}


@pytest.mark.parametrize("driver", sorted(REUSERS))
def test_drivers_on_the_stored_source_kernels_do_not_change_one_bit(driver, knobs):
    """bdg_moment_matrix, bdg_response_map and bdg_subspace_filter launch bdg_apply_series' kernels with plans of their
    own; the products after the recurrence have grids of their own and do not follow the switch."""
    run, flag = REUSERS[driver]
    _, system, solver = _fresh("dictionary", "packed", knobs)

    def call():
        return run(system, solver)

    solver.set_lanes_per_row(32)
    try:
        reference, before = _one_tile(knobs, solver, call, 32)
        capped, perf = _capped(knobs, solver, call, 1, 32)
    finally:
        solver.set_lanes_per_row(0)
    print(driver, "grid", perf["grid"], "launches", perf["launches"], np.abs(capped - reference).max())
    assert before[flag] > 0 and perf[flag] == before[flag] and perf["dict_blocks"] > 0
    assert perf["launches"] == before["launches"] > 0
    assert np.abs(reference).max() > 1e-3
    assert np.array_equal(capped, reference)


# ------------------------------------------------------------------ 7. one 3-D lattice
def test_rows_of_seven_blocks_over_several_tiles(knobs):
    """17 x 16 x 16 sites: 7 blocks per row, the z-neighbours read from the wave's rows in LDS, the others gathered;
    544 tiles at 32 lanes.  Bit for bit against one tile per workgroup, and within the bound of the restatement."""
    system = cases.SYSTEMS["cube"]()
    solver = system._solver()
    n = system.lattice.size
    call = _entry("apply_series", system, solver)
    solver.set_lanes_per_row(32)
    try:
        reference, before = _one_tile(knobs, solver, call, 32, n)
        capped, perf = _capped(knobs, solver, call, 1, 32, n)
    finally:
        solver.set_lanes_per_row(0)
    for record in (before, perf):
        assert record["apply"] == 2 and record["dict_blocks"] > 0 and record["real_arithmetic"] == record["ph_packed"] == 1
        assert record["launches"] == 3 * M
    print("cube", "grid", perf["grid"], "tiles", cases.tiles_of(n, 32), np.abs(capped - reference).max())
    assert np.array_equal(capped, reference)
    _hold_to_restatement(("apply_series", "cube", "grid", perf["grid"]), "apply_series", "cube", capped)
