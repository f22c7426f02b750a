"""response_map() on the GPU: bdg_response_map against the numpy restatement and the dense sum over eigenpairs in every
kernel form and arithmetic mode, the shapes at which the product kernel can go wrong, chunks of sites bit for bit, the
route through correlation(), and the susceptibility maps end to end."""

import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import bodge_amd as ba
from bodge_amd import correlation as corr

import correlation_cases as ccases
import response_map_cases as cases

pytestmark = pytest.mark.gpu

ARITHMETIC = {
    "packed": {},
    "real_full": {"BODGE_AMD_PH": "0"},
    "complex_packed": {"BODGE_AMD_REAL": "0"},
    "complex_full": {"BODGE_AMD_REAL": "0", "BODGE_AMD_PH": "0"},
}


# ------------------------------------------------------------------ against the restatement and dense
@pytest.mark.parametrize("name", cases.SYSTEMS)
@pytest.mark.parametrize("form", ["dictionary", "streamed"])
@pytest.mark.parametrize("arithmetic", sorted(ARITHMETIC))
def test_device_matches_restatement_and_dense(name, form, arithmetic, knobs):
    """M = 48, a random complex c, a random non-Hermitian 4×4 A at the interior site, all sites.  The tolerance is 20
    times the distance of the numpy restatement from the dense sum over the eigenpairs on the same case
    (tests/test_response_map_host.py prints it)."""
    knobs.update(ARITHMETIC[arithmetic])
    if form == "streamed":
        knobs.set("BODGE_AMD_DICT", "0")
    system = ccases.SYSTEMS[name]()  # (a fresh handle: the dictionary switch is read at upload)
    rows, a, coef, restated, dense, own = cases.references(name)
    tolerance = cases.parity_tolerance(name)
    n, M = system.lattice.size, cases.M_SMALL
    solver = system._solver()
    got = solver.response_map(cases.scale_of(system), rows, a, coef, np.arange(n))
    perf = solver.perf()
    print(name, form, arithmetic, "max|K|", np.abs(dense).max(), "device - restated", np.abs(got - restated).max(),
          "device - dense", np.abs(got - dense).max(), "restated - dense", own, "tolerance", tolerance)
    assert got.shape == (1, n, 4, 4)
    assert np.abs(got - restated).max() <= tolerance and np.abs(got - dense).max() <= tolerance

    assert perf["response_map"] == 1
    assert perf["correlation"] == perf["apply"] == perf["clenshaw"] == perf["green"] == perf["green_local"] == 0
    assert perf["lanes_per_row"] == 4 and perf["launches"] == M - 1 and perf["vector_steps"] == 4 * (M - 1)
    assert perf["gemm_flops"] == 8.0 * M * M * (4 * 4 * n)
    assert perf["gemm_ms"] > 0 and perf["window_ms"] >= perf["gemm_ms"]
    is_real = np.abs(np.asarray(system.matrix("dense")).imag).max() == 0
    assert perf["real_arithmetic"] == (1 if is_real and "complex" not in arithmetic else 0)
    if form == "streamed":
        assert perf["dict_blocks"] == 0
    elif name in ("dictionary", "cube"):
        assert perf["dict_blocks"] > 0
    if arithmetic.endswith("full"):
        assert perf["ph_packed"] == 0


# ------------------------------------------------------------------ shapes of the product kernel
M_SHAPES = [1, 2, 17, 65, 130]


@functools.lru_cache(maxsize=None)
def _shape_yardstick(name, support_sites):
    """The restated-to-dense distance at the largest M of the shape cases, three kernels: 20 times it is the tolerance
    of every M.  Measured per M instead it degenerates: at M = 1 the blocks are c_00 A on the source site and zero
    elsewhere, and the two references agree to the last place by luck and not by accuracy."""
    return cases.references(name, max(M_SHAPES), support_sites, 3)[5]


@pytest.mark.parametrize("name", ["cube", "dictionary"])
@pytest.mark.parametrize("M", M_SHAPES)
@pytest.mark.parametrize("lanes", [4, 32])
@pytest.mark.parametrize("support_sites", [1, 2, 3])
def test_product_kernel_shapes(name, M, lanes, support_sites):
    """Moments that fill no tile, one tile and a bit, two tiles and a bit; supports of 4, 8 and 12 rows in batches of 4
    lanes (one to three batches, no padding) and of 32 lanes (28, 24, 20 zero columns); three kernels and one.  All 48 or
    56 sites make K = 4·Sp·sites a multiple of 64 (768 to 7168: whole tiles of k); one site (K = 16 to 128) and 17
    shuffled sites (K = 272 to 2176, no multiple of 64 at 4 lanes) end in a ragged tile.  The one-kernel call and the
    shorter target lists must reproduce the bits of the three-kernel call on all sites: an entry's sums run over n and
    m only."""
    system = cases.system_of(name)
    rows, a, coef, restated, dense, _ = cases.references(name, M, support_sites, 3)
    tolerance = 20 * _shape_yardstick(name, support_sites)
    n, scale = system.lattice.size, cases.scale_of(system)
    everything = np.arange(n)
    rng = np.random.default_rng(5)
    source = int(rows[0] // 4)
    shuffled = rng.permutation(np.concatenate([[source], rng.choice(np.delete(everything, source), 16, replace=False)]))
    solver = system._solver()
    solver.set_lanes_per_row(lanes)
    try:
        got = solver.response_map(scale, rows, a, coef, everything)
        perf = solver.perf()
        single = solver.response_map(scale, rows, a, coef[0], everything)
        perf_single = solver.perf()
        one = solver.response_map(scale, rows, a, coef, [source])
        some = solver.response_map(scale, rows, a, coef, shuffled)
        perf_some = solver.perf()
    finally:
        solver.set_lanes_per_row(0)
    print(name, M, lanes, support_sites, "device - restated", np.abs(got - restated).max(), "device - dense",
          np.abs(got - dense).max(), "tolerance", tolerance)
    assert got.shape == (3, n, 4, 4) and perf["lanes_per_row"] == lanes
    assert np.abs(got - restated).max() <= tolerance and np.abs(got - dense).max() <= tolerance
    assert single.shape == (1, n, 4, 4) and np.array_equal(single[0], got[0])
    assert one.shape == (3, 1, 4, 4) and np.array_equal(one[:, 0], got[:, source])
    assert some.shape == (3, 17, 4, 4) and np.array_equal(some, got[:, shuffled])
    S = 4 * support_sites
    batches = -(-S // lanes)
    columns = batches * lanes
    assert perf["launches"] == batches * (M - 1) and perf["vector_steps"] == S * (M - 1)
    assert perf["gemm_flops"] == 3 * 8.0 * M * M * (4 * columns * n)
    assert perf_single["gemm_flops"] == 8.0 * M * M * (4 * columns * n)
    assert perf_some["gemm_flops"] == 3 * 8.0 * M * M * (4 * columns * 17)


# ------------------------------------------------------------------ chunks of sites
def test_chunks_of_sites_give_the_bits_of_the_unchunked_call(knobs):
    """disordered_300, M = 130, one source site (4 columns): a site takes 2·130·4·4·16 = 33 280 bytes of the two panels.
    A budget of exactly 16 sites makes 19 chunks (18 of 16 sites and one of 12), each with its own recurrence: the same
    bits.  One byte less and the call gives up and names the bytes.  A repeated call is bit-identical."""
    system = cases.system_of("disordered_300")
    scale = cases.scale_of(system)
    M = 130
    rows, a = cases.random_source(system)
    coef = cases.random_coefficients(M, 2)
    sites = np.arange(300)
    solver = system._solver()
    whole = solver.response_map(scale, rows, a, coef, sites)
    perf = solver.perf()
    assert perf["launches"] == M - 1 and perf["gemm_flops"] == 2 * 8.0 * M * M * (16 * 300)
    assert np.array_equal(whole, solver.response_map(scale, rows, a, coef, sites))
    site_bytes = 2 * M * 4 * 4 * 16
    knobs.set("BODGE_AMD_CORRELATION_BYTES", str(16 * site_bytes))
    chunked = solver.response_map(scale, rows, a, coef, sites)
    perf = solver.perf()
    print("chunked - whole", np.abs(chunked - whole).max(), "bit-identical:", np.array_equal(chunked, whole))
    assert perf["launches"] == 19 * (M - 1)
    assert perf["gemm_flops"] == 2 * 8.0 * M * M * (16 * 300)  # (the chunks tile the same sites)
    assert np.array_equal(chunked, whole)
    knobs.set("BODGE_AMD_CORRELATION_BYTES", str(16 * site_bytes - 1))
    with pytest.raises(ValueError, match=str(16 * site_bytes)):
        solver.response_map(scale, rows, a, coef, sites)
    # fewer than 16 sites asked for: they are what has to fit
    knobs.set("BODGE_AMD_CORRELATION_BYTES", str(5 * site_bytes))
    assert np.array_equal(solver.response_map(scale, rows, a, coef, sites[:5]), whole[:, :5])
    knobs.set("BODGE_AMD_CORRELATION_BYTES", str(5 * site_bytes - 1))
    with pytest.raises(ValueError, match=str(5 * site_bytes)):
        solver.response_map(scale, rows, a, coef, sites[:5])


# ------------------------------------------------------------------ against the existing route
def test_blocks_agree_with_correlation_on_the_source_unit_vectors():
    """Tr[T_n A T_m B_j] = Tr[T_m B_j T_n A], and A annihilates every unit vector off its support: correlation(B_j, A,
    vectors=<unit vectors of the source rows>).mu.T contracted with c is Σ_γδ B_j[γ,δ] K_j[γ,δ].  B_j random, scaled to
    Σ|B| = 1 so that the contraction moves an entry's error by no more than itself; the tolerance is the 20× rule of
    the parity test."""
    name = "disordered_complex"
    system = cases.system_of(name)
    rows, a, coef, restated, _, _ = cases.references(name)
    n, M = system.lattice.size, cases.M_SMALL
    tolerance = cases.parity_tolerance(name)
    A = sp.lil_matrix((4 * n, 4 * n), dtype=np.complex128)
    A[np.ix_(rows, rows)] = a
    A = A.tocsr()
    vectors = np.zeros((4 * n, rows.size), dtype=np.complex128)
    vectors[rows, np.arange(rows.size)] = 1.0
    blocks = system._solver().response_map(cases.scale_of(system), rows, a, coef, np.arange(n))[0]
    rng = np.random.default_rng(12)
    for j in (int(rows[0] // 4), 0, n - 1):
        b = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
        b /= np.abs(b).sum()
        B = sp.lil_matrix((4 * n, 4 * n), dtype=np.complex128)
        B[4 * j : 4 * j + 4, 4 * j : 4 * j + 4] = b
        mu = system.correlation(B.tocsr(), A, moments=M, vectors=vectors, scale=cases.scale_of(system)).mu
        expected = np.sum(coef[0] * mu.T)
        got = np.sum(b * blocks[j])
        print("site", j, got, expected, abs(got - expected), "restated", abs(np.sum(b * restated[0, j]) - expected), "tolerance", tolerance)
        assert abs(got - expected) <= tolerance


# ------------------------------------------------------------------ end to end
def _end_to_end_tolerance(figures, pin):
    """20 × the restatement's own distance from the dense map at the same M (relative to max|χ|), and never looser than
    the pin of the corresponding correlation test."""
    return np.minimum(20 * figures, pin)


def test_static_spin_map_matches_the_dense_divided_differences():
    system = cases.system_of("disordered_complex")
    M, _, exact, figures = cases.end_to_end("static")
    site = ccases.interior_site(system)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (the rule's M has converged)
        result = system.response_map(corr.spin_operator(system, [site], "z"), temperature=cases.END_TO_END["static_temperature"])
    assert isinstance(result, ba.ResponseMap) and result.moments == M and result.omega is None
    assert result.blocks.shape == (system.lattice.size, 4, 4) and result.sites == list(system.lattice.sites())
    assert result.info["support"] == 1 and result.info["chunks"] == 1 and result.info["perf"]["response_map"] == 1
    chi = result.spin("z")
    largest = np.abs(exact[0]).max()
    tolerance = _end_to_end_tolerance(figures, cases.END_TO_END["static_pin"])[0]
    print("static: moments", M, "max|chi|", largest, "device - dense, relative", np.abs(chi - exact[0]).max() / largest,
          "restated - dense", figures[0], "tolerance", tolerance)
    assert np.abs(chi - exact[0]).max() <= tolerance * largest


def test_dynamic_spin_map_matches_the_dense_double_sum():
    system = cases.system_of("disordered_complex")
    M, _, exact, figures = cases.end_to_end("response")
    site = ccases.interior_site(system)
    T, eta = cases.END_TO_END["temperature"], cases.END_TO_END["broadening"]
    cut = [(x, 4, 0) for x in range(9)][::-1]
    sz = corr.spin_operator(system, [site], "z")
    result = system.response_map(sz, temperature=T, broadening=eta, omega=list(cases.END_TO_END["omega"]))
    assert result.moments == M and result.blocks.shape == (2, system.lattice.size, 4, 4)
    assert np.array_equal(result.omega, cases.END_TO_END["omega"])
    chi = result.spin("z")
    tolerance = _end_to_end_tolerance(figures, cases.END_TO_END["response_pin"])
    for k in range(2):
        largest = np.abs(exact[k]).max()
        print("omega", cases.END_TO_END["omega"][k], "max|chi|", largest, "device - dense, relative",
              np.abs(chi[k] - exact[k]).max() / largest, "restated - dense", figures[k], "tolerance", tolerance[k])
        assert np.abs(chi[k] - exact[k]).max() <= tolerance[k] * largest
    # a line cut in the order given, a scalar ω squeezed
    line = system.response_map(sz, temperature=T, broadening=eta, omega=0.7, sites=cut)
    assert line.blocks.shape == (9, 4, 4) and line.sites == cut and line.omega == 0.7
    index = [system.lattice[c] for c in cut]
    assert np.array_equal(line.blocks, result.blocks[1][index])
    assert np.array_equal(line.density(), result.density()[1][index])
    # the caller's function: F = 1 gives Tr[A B_j] = the block of A on its own site, nothing elsewhere
    plain = system.response_map(sz, function=lambda x, y: np.ones(np.broadcast(x, y).shape), moments=8)
    j = system.lattice[site]
    assert np.abs(plain.blocks[j] - np.diag([1, -1, -1, 1])).max() <= 1e-13
    assert np.abs(np.delete(plain.blocks, j, axis=0)).max() <= 1e-13


# ------------------------------------------------------------------ refusals that need a handle
def test_rows_and_sites_are_checked_against_the_matrix_size():
    system = cases.system_of("cube")
    solver = system._solver()
    n = system.lattice.size
    a, c = np.eye(4), np.ones((2, 2))
    for rows, sites, message in (([0, 1, 2, 4 * n], [0], "source row"), ([0, 1, -1, 2], [0], "source row"),
                                 ([0, 1, 2, 1], [0], "source row 1 listed twice"), ([0, 1, 2, 3], [n], "block row"),
                                 ([0, 1, 2, 3], [-1], "block row"), ([0, 1, 2, 3], [3, 5, 3], "block row 3 listed twice")):
        with pytest.raises(ValueError, match=message):
            solver.response_map(6.0, rows, a, c, sites)
    # the public call takes a site twice and answers twice
    sz = corr.spin_operator(system, [(1, 1, 1)], "z")
    twice = system.response_map(sz, function=lambda x, y: x * y, moments=6, sites=[(0, 0, 0), (1, 1, 1), (0, 0, 0)])
    assert twice.blocks.shape == (3, 4, 4) and np.array_equal(twice.blocks[0], twice.blocks[2])


def test_slab_handles_are_refused():
    from bodge_amd.solver import SlabGroup

    system = ccases.uniform_swave((8, 4, 1))
    with SlabGroup.from_hamiltonian(system, 2) as group:
        with pytest.raises(ValueError, match="slab"):
            group.members[0].response_map(1.0, [0, 1, 2, 3], np.eye(4), np.ones((2, 2)), [0])


def test_a_lanczos_run_on_the_handle_is_ended():
    system = ccases.SYSTEMS["dictionary"]()
    solver = system._solver()
    solver.lanczos_begin(2, max_iter=64)
    solver.lanczos_advance(2)
    system.response_map(corr.spin_operator(system, [(1, 1, 0)], "z"), function=lambda x, y: x + y, moments=4)
    with pytest.raises(ValueError, match="lanczos_begin"):
        solver.lanczos_advance(1)
