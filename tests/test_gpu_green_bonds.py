"""green_bonds() on the GPU: every model in both forms of the matrix, every arithmetic mode and lane width against the
numpy restatement and the dense resolvent; the raw moments through identity weights against bdg_green_local_moments (bit
for bit) and bdg_green_moments; batches, ranges of the device table and several tiles per workgroup (bit for bit); the
derived hole columns; the public function against green_map() and green()."""

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import green as gr

import family_tile_cases
import green_bonds_cases as cases

pytestmark = pytest.mark.gpu

ARITHMETIC = {
    "packed": {},
    "real_full": {"BODGE_AMD_PH": "0"},
    "complex_packed": {"BODGE_AMD_REAL": "0"},
    "complex_full": {"BODGE_AMD_REAL": "0", "BODGE_AMD_PH": "0"},
}


def effective(name, arithmetic):
    """(real, packed) as the library will decide them for this model under the switches of `arithmetic`."""
    return (cases.IS_REAL[name] and "complex" not in arithmetic, cases.IS_PH[name] and not arithmetic.endswith("full"))


def modes_of(name):
    """The arithmetic settings that run different kernels on this model (a complex matrix ignores REAL, one without
    the Nambu form of the blocks would ignore PH)."""
    seen, out = set(), []
    for arithmetic in ARITHMETIC:
        if effective(name, arithmetic) not in seen:
            seen.add(effective(name, arithmetic))
            out.append(arithmetic)
    return out


def fresh(name, form, arithmetic, knobs, build=None):
    """A new system and handle under the switches of (form, arithmetic): the dictionary switch is read at upload."""
    for switch in ("BODGE_AMD_REAL", "BODGE_AMD_PH"):  # (both, every time: a switch of the mode before does not linger)
        if switch in ARITHMETIC[arithmetic]:
            knobs.set(switch, ARITHMETIC[arithmetic][switch])
        else:
            knobs.unset(switch)
    knobs.set("BODGE_AMD_DICT", "1" if form == "dictionary" else "0")
    system = (build or cases.SYSTEMS[name])()
    return system, system._solver()


def assert_form(perf, name, form, arithmetic, lanes):
    real, packed = effective(name, arithmetic)
    dictionary = form == "dictionary" and not (real and lanes == 64)
    assert perf["green_bonds"] == (2 if dictionary else 1), (perf["green_bonds"], perf["dict_skipped"])
    assert (perf["dict_blocks"] > 0) == dictionary
    assert perf["real_arithmetic"] == int(real) and perf["ph_packed"] == int(packed)
    assert perf["lanes_per_row"] == lanes and perf["green"] == 0 and perf["green_local"] == 0


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", sorted(cases.SYSTEMS))
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
def test_device_matches_restatement_and_dense(name, form, knobs):
    """The default moments for Γ = 0.1.  Device - restated <= 32·M·2⁻⁵³·max(1, max|restated|), device -
    dense <= 20 x the restatement's own distance (cases.RESTATEMENT_ERROR).  Columns as the public function picks them
    (2 where the hole columns can be derived) at every lane width, all four at 16 lanes."""
    reference = cases.system_of(name)
    indptr, indices = cases.pattern_of(reference)
    scale, moments = cases.scale_of(reference), cases.moments_of(reference)
    weights = gr.moment_weights(moments, scale, cases.Z)
    columns = 2 if cases.DERIVES[name] else 4
    dense = cases.dense(name)
    for arithmetic in modes_of(name):
        system, solver = fresh(name, form, arithmetic, knobs)
        widths = [(lanes, columns) for lanes in (4, 8, 16, 32)] + [(16, 4)] * (columns == 2)
        if form == "dictionary" and "complex" in arithmetic or not cases.IS_REAL[name]:
            widths.append((64, columns))
        try:
            for lanes, c in widths:
                solver.set_lanes_per_row(lanes)
                got = solver.green_bond_blocks(scale, weights, indptr, indices, c).transpose(1, 0, 2, 3)
                perf = solver.perf()
                assert_form(perf, name, form, arithmetic, lanes)
                restated = cases.restated(name, c)
                to_restated, bound = np.abs(got - restated).max(), cases.rounding_bound(moments, restated)
                to_dense = cases.distance(got, dense)
                print(name, form, arithmetic, "lanes", lanes, "columns", c, "M", moments, "device - restated", to_restated,
                      "bound", bound, "device - dense", to_dense, "limit", 20 * cases.RESTATEMENT_ERROR[name])
                assert to_restated <= bound
                assert to_dense <= 20 * cases.RESTATEMENT_ERROR[name]
                per_lane = 2 if perf["real_arithmetic"] else 1
                sites = np.unique(indices).size
                batch = max(1, min(lanes * per_lane, 64, sites * c) // c)
                assert perf["launches"] == -(-sites // batch) * (moments - 1), (perf["launches"], sites, batch)
                assert perf["vector_steps"] == (moments - 1) * sites * c
                assert perf["window_ms"] >= perf["kernel_ms"] > 0 and perf["bytes_moved"] > 0
        finally:
            solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ 2. raw moments through identity weights
@pytest.mark.parametrize("name,form", [("swave", "dictionary"), ("peierls", "streamed"), ("cube", "dictionary"),
                                       ("dwave_open", "streamed")])
@pytest.mark.parametrize("columns", [2, 4])
def test_identity_weights_return_the_moment_table(name, form, columns, knobs):
    """w = δ: 1·μ plus exact zeros.  The diagonal blocks are bdg_green_local_moments of the same handle and lanes bit
    for bit (the same tile loop, the same batches); the bonds are bdg_green_moments from the source rows of a site to
    its neighbours under the rounding bound (its batches are narrower)."""
    system, solver = fresh(name, form, "packed", knobs)
    indptr, indices = cases.pattern_of(system)
    rows = cases.block_rows(indptr)
    scale, moments, lanes = cases.scale_of(system), 48, 16
    solver.set_lanes_per_row(lanes)
    try:
        table = solver.green_bond_blocks(scale, np.eye(moments, dtype=np.complex128), indptr, indices, columns)
        assert_form(solver.perf(), name, form, "packed", lanes)
        assert table.shape == (moments, indices.size, 4, 4)
        diagonal = np.flatnonzero(rows == indices)
        local = solver.green_local_moments(scale, moments, indices[diagonal], columns)
        assert solver.perf()["lanes_per_row"] == lanes and solver.perf()["green_bonds"] == 0
        print(name, form, columns, "diagonal", np.abs(table[:, diagonal, :, :columns] - local).max())
        assert np.array_equal(table[:, diagonal, :, :columns], local)
        if columns == 2:  # the hole columns are the rule applied to the same numbers: exact
            assert np.array_equal(table[:, diagonal], gr.hole_columns(local))
        assert np.array_equal(table[0, diagonal], np.broadcast_to(np.eye(4), (diagonal.size, 4, 4)))
        assert np.abs(table[0, rows != indices]).max(initial=0.0) == 0
        bound = cases.rounding_bound(moments, table)
        n = system.lattice.size
        for i in sorted({0, n // 2, n - 1}):
            blocks = np.flatnonzero(indices == i)
            source = 4 * i + np.arange(columns, dtype=np.int64)
            picked = solver.green_moments(scale, moments, source, rows[blocks].astype(np.int32))  # (M, T, 4, columns)
            print(name, form, columns, "site", i, np.abs(table[:, blocks, :, :columns] - picked).max(), bound)
            assert np.abs(table[:, blocks, :, :columns] - picked).max() <= bound
    finally:
        solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ 3. batches
def test_cuts_and_shuffled_site_lists_equal_the_run_over_all_sites_bit_for_bit(knobs):
    """9 x 8 sites: 72 > 32 sites of a batch at two columns, so slot bases above zero and bonds into the sites of the
    neighbouring batch everywhere.  A vector's recurrence does not depend on the batch it rides in, and the contraction
    of an entry not on the rest of the table."""
    system = family_tile_cases.apply_cases.uniform_swave((9, 8, 1))
    energies = np.array([-0.4, 0.0, 0.7])
    every = system.green_bonds(energies, broadening=0.1, moments=160)
    perf = every.info["perf"]
    assert perf["vectors_per_launch"] == 64 and perf["launches"] == 3 * 159 and every.info["columns"] == 2
    assert every.blocks.shape == (72 * 5, 3, 4, 4)
    cut = [(x, 3, 0) for x in range(9)]                                # (its y neighbours are no column sites)
    rng = np.random.default_rng(5)
    coords = list(system.lattice.sites())
    shuffled_all = [coords[i] for i in rng.permutation(72)]
    shuffled_some = [coords[i] for i in rng.permutation(72)[:41]]      # two batches, other slots than in `every`
    for label, sites, count in (("cut", cut, 9), ("all, shuffled", shuffled_all, 72), ("41, shuffled", shuffled_some, 41)):
        part = system.green_bonds(energies, sites, broadening=0.1, moments=160)
        assert part.blocks.shape[0] == 5 * count and set(part.indices.tolist()) == {system.lattice[s] for s in sites}
        in_every, in_part = cases.shared_blocks(every.indptr, every.indices, part.indptr, part.indices)
        assert in_part.size == 5 * count
        print(label, np.abs(every.blocks[in_every] - part.blocks[in_part]).max())
        assert np.array_equal(every.blocks[in_every], part.blocks[in_part]), label
    with pytest.raises(IndexError):
        system.green_bonds(energies, cut, broadening=0.1, moments=16).spectral()


# ------------------------------------------------------------------ 4. ranges of the device table
@pytest.mark.parametrize("columns", [2, 4])
def test_ranges_of_the_device_table_do_not_change_one_bit(columns, knobs):
    system = cases.SYSTEMS["dwave_open"]()
    solver = system._solver()
    indptr, indices = cases.pattern_of(system)
    scale, moments = cases.scale_of(system), 40
    weights = gr.moment_weights(moments, scale, cases.Z)
    whole = solver.green_bond_blocks(scale, weights, indptr, indices, columns)
    perf = solver.perf()
    assert perf["green_ranges"] == 1 and whole.shape == (4, 150, 4, 4)
    batch = perf["vectors_per_launch"] // columns                       # sites of a batch; 5 blocks per column site
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", str(15 * min(batch, 30) * 5 * 4 * columns * 16))  # 15 moments per range
    chunked = solver.green_bond_blocks(scale, weights, indptr, indices, columns)
    assert solver.perf()["green_ranges"] == 3
    assert np.array_equal(whole, chunked)
    knobs.set("BODGE_AMD_GREEN_TABLE_BYTES", "1")                       # (less than one moment: one moment per range)
    single = solver.green_bond_blocks(scale, weights, indptr, indices, columns)
    assert solver.perf()["green_ranges"] == 40
    assert np.array_equal(whole, single)


# ------------------------------------------------------------------ 5. several tiles per workgroup
N = int(np.prod(family_tile_cases.SHAPE))


@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("arithmetic", ["packed", "complex_full"])
def test_several_tiles_per_workgroup_do_not_change_one_bit(form, arithmetic, knobs):
    """67 x 63 sites at 32 lanes: 528 tiles; BODGE_AMD_BLOCKS_PER_CU=1 lets every workgroup walk two or three of them,
    =8 gives every tile a workgroup of its own (the method of test_gpu_family_tiles.py)."""
    knobs.update(ARITHMETIC[arithmetic])
    knobs.set("BODGE_AMD_DICT", "1" if form == "dictionary" else "0")
    system = family_tile_cases.SYSTEMS["uniform"]()
    solver = system._solver()
    scale, moments, lanes = cases.scale_of(system), family_tile_cases.M, 32
    weights = gr.moment_weights(moments, scale, np.array([-0.3, 0.2, 0.9]) + 0.1j)
    columns = 4 if arithmetic == "complex_full" else 2
    cut = [system.lattice[(x, 31, 0)] for x in range(64)]
    patterns = [("cut", cases.pattern_of(system, cut))]
    if form == "dictionary" and arithmetic == "packed":
        patterns.append(("all", cases.pattern_of(system)))
    tiles = family_tile_cases.tiles_of(N, lanes)
    solver.set_lanes_per_row(lanes)
    try:
        for label, (indptr, indices) in patterns:
            knobs.set("BODGE_AMD_BLOCKS_PER_CU", "8")
            reference = solver.green_bond_blocks(scale, weights, indptr, indices, columns)
            before = solver.perf()
            assert before["lanes_per_row"] == lanes and before["grid"] >= tiles
            assert before["green_bonds"] == (2 if form == "dictionary" else 1)
            assert before["real_arithmetic"] == (0 if arithmetic == "complex_full" else 1)
            knobs.set("BODGE_AMD_BLOCKS_PER_CU", "1")
            capped = solver.green_bond_blocks(scale, weights, indptr, indices, columns)
            perf = solver.perf()
            assert perf["lanes_per_row"] == lanes and tiles > 2 * perf["grid"], (tiles, perf["grid"])
            assert perf["launches"] == before["launches"] and np.abs(reference).max() > 1e-3
            print(form, arithmetic, label, "grid", perf["grid"], "tiles", tiles, np.abs(capped - reference).max())
            assert np.array_equal(capped, reference), label
    finally:
        solver.set_lanes_per_row(0)


# ------------------------------------------------------------------ 6. derived hole columns
@pytest.mark.parametrize("name", [name for name in sorted(cases.SYSTEMS) if cases.DERIVES[name]])
def test_derived_hole_columns_equal_the_four_column_run(name):
    system = cases.SYSTEMS[name]()
    two = system.green_bonds(cases.ENERGIES, broadening=cases.GAMMA)
    four = system.green_bonds(cases.ENERGIES, broadening=cases.GAMMA, _all_columns=True)
    assert two.info["columns"] == 2 and two.info["hole_columns_derived"] and four.info["columns"] == 4
    difference = np.abs(two.blocks - four.blocks).max()
    print(name, difference)
    assert difference <= 1e-13 * max(1.0, np.abs(four.blocks).max())


# ------------------------------------------------------------------ 7. the public function
def test_public_function_against_green_map_and_green():
    system = cases.SYSTEMS["dwave_open"]()
    energies = cases.ENERGIES
    g = system.green_bonds(energies, broadening=cases.GAMMA)
    moments = g.info["moments"]
    assert moments == cases.moments_of(system) and g.info["perf"]["green_bonds"] in (1, 2)
    assert g.blocks.shape == (150, 4, 4, 4) and g.indptr.dtype == np.int32 and g.lattice is system.lattice
    assert cases.distance(g.blocks, cases.dense("dwave_open")) <= 20 * cases.RESTATEMENT_ERROR["dwave_open"]
    local, mapped = g.local(), system.green_map(energies, broadening=cases.GAMMA)
    assert local.sites == mapped.sites and mapped.info["moments"] == moments
    print("local - green_map", np.abs(local.blocks - mapped.blocks).max(), cases.rounding_bound(moments, mapped.blocks))
    assert np.abs(local.blocks - mapped.blocks).max() <= cases.rounding_bound(moments, mapped.blocks)
    assert np.allclose(local.ldos(), mapped.ldos(), rtol=0, atol=cases.rounding_bound(moments, mapped.blocks))
    for j, i in (((3, 2, 0), (2, 2, 0)), ((2, 3, 0), (2, 2, 0)), ((0, 0, 0), (5, 0, 0)), ((4, 4, 0), (4, 4, 0))):
        one = system.green(i, energies, targets=[j], broadening=cases.GAMMA)
        assert one.info["moments"] == moments
        bound = cases.rounding_bound(moments, one.blocks)
        print(j, i, np.abs(g.block(j, i) - one.blocks[0]).max(), bound)
        assert np.abs(g.block(j, i) - one.blocks[0]).max() <= bound
    fx, fy = g.anomalous((3, 2, 0), (2, 2, 0)), g.anomalous((2, 3, 0), (2, 2, 0))
    assert fx.shape == (4, 2, 2) and np.abs(fx).max() > 1e-3
    assert np.all(np.real(fx[:, 0, 1] * np.conj(fy[:, 0, 1])) < 0)  # d-wave: opposite sign on x and y bonds
    value = g.expectation(ba.correlation.current_operator(system, 0))
    assert value.shape == energies.shape and np.abs(value.imag).max() <= 1e-13


def test_argument_errors_of_the_entry_point():
    system = cases.SYSTEMS["swave"]()
    solver = system._solver()
    scale = cases.scale_of(system)
    indptr, indices = cases.pattern_of(system)
    weights = np.ones((2, 8), dtype=np.complex128)
    bad = indptr.copy()
    bad[3] = bad[2] - 1
    with pytest.raises(ValueError, match="monotone"):
        solver.green_bond_blocks(scale, weights, bad, indices, 2)
    bad = indices.copy()
    bad[7] = system.lattice.size
    with pytest.raises(ValueError, match="out of range"):
        solver.green_bond_blocks(scale, weights, indptr, bad, 2)
    bad = indices.copy()
    bad[[0, 1]] = bad[[1, 0]]
    with pytest.raises(ValueError, match="canonical"):
        solver.green_bond_blocks(scale, weights, indptr, bad, 2)
    with pytest.raises(ValueError, match="components"):
        solver.green_bond_blocks(scale, weights, indptr, indices, 3)
    with pytest.raises(ValueError, match="scale"):
        solver.green_bond_blocks(0.0, weights, indptr, indices, 2)
    # the call ends a Lanczos run on the handle, as its siblings do
    solver.lanczos_begin(2)
    solver.green_bond_blocks(scale, weights, indptr, indices, 2)
    with pytest.raises(ValueError, match="lanczos_begin"):
        solver.lanczos_advance(1)
