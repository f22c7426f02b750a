"""response_map() without a GPU: the recurrence, the product and the contraction restated in numpy against the dense
sum over eigenpairs, the orientation of every index, the contractions of ResponseMap, the support rule, the argument
errors of bdg_response_map and the register budget of the new product kernel."""

import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

import bodge_amd as ba
from bodge_amd import correlation as corr
from bodge_amd import response_map as rmap

import response_map_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ algorithm
@pytest.mark.parametrize("name", cases.SYSTEMS)
def test_restatement_matches_dense_blocks(name):
    """M = 48, a random complex c, a random non-Hermitian 4×4 A at the interior site, all sites.  The distance printed
    here is the yardstick of the device tolerances (20 × it).  Measured: largest |K| 5.5 - 9.1, distance 3.7e-14 -
    1.0e-13 (5.1e-15 - 1.1e-14 of the largest entry)."""
    rows, a, coef, restated, dense, distance = cases.references(name)
    largest = float(np.abs(dense).max())
    print(name, "max|K| =", largest, "restated - dense =", distance, "relative", distance / largest)
    n = cases.system_of(name).lattice.size
    assert restated.shape == dense.shape == (1, n, 4, 4)
    assert largest > 1e-3
    assert distance <= 1e-13 * largest
    assert cases.parity_tolerance(name) >= 20 * distance > 0


def test_orientation_against_the_double_sum_over_eigenpairs():
    """A random complex Hermitian H (6 sites), a random non-Hermitian A on two sites, a random non-Hermitian B on one
    site, a random complex c: Σ_γδ B[γ,δ] K[γ,δ] equals Σ_ab A_ab (B_j)_ba F(E_a, E_b) summed as it stands.  A swap of
    n and m, of α and β, of γ and δ, or a missing conjugate each move the result by order one."""
    rng = np.random.default_rng(3)
    n_sites, M = 6, 12
    dim = 4 * n_sites
    h = rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))
    h = h + h.conj().T
    scale = 1.05 * np.abs(np.linalg.eigvalsh(h)).max()
    rows = np.array([4, 5, 6, 7, 16, 17, 18, 19])
    a = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    c = rng.standard_normal((1, M, M)) + 1j * rng.standard_normal((1, M, M))
    sites = np.array([3, 1, 4])
    w, v = np.linalg.eigh(h)
    values = cases.series_on_spectrum(w, scale, c)
    restated = cases.restated_blocks(h, scale, rows, a, c, sites)
    dense = cases.dense_blocks(w, v, rows, a, values, sites)
    A = np.zeros((dim, dim), dtype=np.complex128)
    A[np.ix_(rows, rows)] = a
    a_eig = v.conj().T @ A @ v
    for s, j in enumerate(sites):
        b = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
        B = np.zeros((dim, dim), dtype=np.complex128)
        B[4 * j : 4 * j + 4, 4 * j : 4 * j + 4] = b
        b_eig = v.conj().T @ B @ v
        expected = np.sum(a_eig * b_eig.T * values[0])
        for label, blocks in (("restated", restated), ("dense", dense)):
            got = np.sum(b * blocks[0, s])
            print(label, j, got, expected, abs(got - expected) / abs(expected))
            assert abs(got - expected) <= 1e-12 * abs(expected), label
        # the transposed orientations are different numbers: the check can tell them apart
        assert abs(np.sum(b.T * restated[0, s]) - expected) > 1e-3 * abs(expected)
    swapped = cases.restated_blocks(h, scale, rows, a, c.transpose(0, 2, 1), sites)
    assert np.abs(swapped - restated).max() > 1e-3 * np.abs(restated).max()
    assert np.abs(cases.restated_blocks(h, scale, rows, a.T, c, sites) - restated).max() > 1e-3 * np.abs(restated).max()


# ------------------------------------------------------------------ the result class
def test_contractions_carry_the_half_and_the_blocks_of_the_operators():
    rng = np.random.default_rng(1)
    blocks = rng.standard_normal((2, 5, 4, 4)) + 1j * rng.standard_normal((2, 5, 4, 4))
    result = ba.ResponseMap(blocks=blocks, sites=[(i, 0, 0) for i in range(5)], omega=np.array([0.0, 0.7]),
                            temperature=0.5, scale=6.0, moments=8)
    b = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    expected = 0.5 * (b[None, None] * blocks).sum(axis=(2, 3))
    assert result.contract(b).shape == (2, 5) and np.abs(result.contract(b) - expected).max() <= 1e-14
    system = cases.system_of("cube")
    site = (1, 2, 1)
    j = system.lattice[site]
    for direction in (1, 2, 3, "x", "y", "z"):
        block = corr.spin_operator(system, [site], direction)[4 * j : 4 * j + 4, 4 * j : 4 * j + 4].toarray()
        assert np.array_equal(rmap.spin_block(direction), block)
        assert np.array_equal(result.spin(direction), result.contract(block))
    assert np.array_equal(rmap.density_block(), np.diag([1, 1, -1, -1]))
    assert np.array_equal(result.density(), result.contract(np.diag([1, 1, -1, -1])))
    single = ba.ResponseMap(blocks=blocks[0], sites=result.sites, omega=None, temperature=0.5, scale=6.0, moments=8)
    assert single.spin("z").shape == (5,) and np.array_equal(single.spin("z"), result.spin("z")[0])
    with pytest.raises(ValueError, match="4×4"):
        result.contract(np.eye(3))
    with pytest.raises(ValueError, match="direction"):
        result.spin(4)


def test_support_of_the_operator_is_found_and_limited():
    system = cases.system_of("cube")
    lattice = system.lattice
    sz = corr.spin_operator(system, [(1, 1, 1)], "z")
    support, a = rmap.operator_support(system, sz)
    assert support.tolist() == [lattice[(1, 1, 1)]] and np.array_equal(a, np.diag([1, -1, -1, 1]))
    # rows and columns both count: a hop from one site to another has a support of two, non-Hermitian as it is
    hop = np.zeros((4 * lattice.size, 4 * lattice.size), dtype=np.complex128)
    i, j = lattice[(0, 0, 0)], lattice[(3, 2, 1)]
    hop[4 * j + 1, 4 * i + 2] = 2.0 - 1.0j
    support, a = rmap.operator_support(system, hop)
    assert support.tolist() == sorted([i, j]) and a.shape == (8, 8)
    assert a[4 * (1 if j > i else 0) + 1, 4 * (0 if j > i else 1) + 2] == 2.0 - 1.0j and np.count_nonzero(a) == 1
    eight = corr.spin_operator(system, [(x, y, 0) for x in range(4) for y in range(2)], "x")
    assert rmap.operator_support(system, eight)[0].size == 8
    nine = corr.spin_operator(system, [(x, y, 0) for x in range(3) for y in range(3)], "x")
    with pytest.raises(ValueError, match="support of A is 9 sites"):
        rmap.operator_support(system, nine)
    with pytest.raises(ValueError, match="support of A is 9 sites"):
        system.response_map(nine, temperature=0.1, moments=4)
    with pytest.raises(ValueError, match="zero"):
        rmap.operator_support(system, np.zeros((4 * lattice.size, 4 * lattice.size)))
    for options, message in (({}, "temperature"), ({"temperature": 0.1, "omega": [0.0]}, "broadening"),
                             ({"function": lambda x, y: x * y}, "moments"),
                             ({"function": lambda x, y: x * y, "omega": [0.0], "moments": 4}, "not both"),
                             ({"temperature": 0.1, "moments": 0}, "moments"), ({"temperature": 0.1, "sites": []}, "empty")):
        with pytest.raises(ValueError, match=message):
            system.response_map(sz, **options)


# ------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_without_a_gpu(hip_library):
    """bdg_response_map checks counts, the size of the support, scale and pointers before it looks at the handle, so
    each refusal is reachable here without one, in the order of the header; ranges, repeats and the slab refusal
    need a handle and are in tests/test_gpu_response_map.py."""
    from bodge_amd import backend

    buf = np.zeros(64)
    ptr = backend.as_f64p(buf)
    rows = backend.as_i64p(np.zeros(40, dtype=np.int64))
    sites = backend.as_i32p(np.zeros(1, dtype=np.int32))
    call = hip_library.bdg_response_map
    for args, message in (
        ((None, 1.0, 0, 1, rows, ptr, 1, ptr, 1, sites, ptr), b"n_moments"),
        ((None, -1.0, 0, 0, None, None, 0, None, 0, None, None), b"n_moments"),
        ((None, 1.0, 1, 0, rows, ptr, 0, ptr, 0, sites, ptr), b"n_source_rows"),
        ((None, 1.0, 1, 1, rows, ptr, 0, ptr, 0, sites, ptr), b"n_kernels"),
        ((None, 0.0, 1, 33, rows, ptr, 1, ptr, 0, sites, ptr), b"n_sites"),
        ((None, 0.0, 1, 33, rows, ptr, 1, ptr, 1, sites, ptr), b"limited to 32"),
        ((None, 0.0, 1, 32, None, ptr, 1, ptr, 1, sites, ptr), b"scale"),
        ((None, float("nan"), 1, 1, rows, ptr, 1, ptr, 1, sites, ptr), b"scale"),
        ((None, 1.0, 1, 1, None, ptr, 1, ptr, 1, sites, ptr), b"null argument"),
        ((None, 1.0, 1, 1, rows, None, 1, ptr, 1, sites, ptr), b"null argument"),
        ((None, 1.0, 1, 1, rows, ptr, 1, None, 1, sites, ptr), b"null argument"),
        ((None, 1.0, 1, 1, rows, ptr, 1, ptr, 1, None, ptr), b"null argument"),
        ((None, 1.0, 1, 1, rows, ptr, 1, ptr, 1, sites, None), b"null argument"),
        ((None, 1.0, 1, 1, rows, ptr, 1, ptr, 1, sites, ptr), b"null system handle"),
    ):
        assert call(*args) == -1 and message in hip_library.bdg_last_error(), (args[1:4], message)
    assert "bdg_response_map" in backend.SIGNATURES
    names = [name for name, _ in backend.Perf._fields_]
    for name, kind in (("response_map", ctypes.c_int32), ("gemm_ms", ctypes.c_double), ("gemm_flops", ctypes.c_double)):
        assert (name, kind) in backend.Perf._fields_
    assert names.index("gemm_flops") == names.index("gemm_ms") + 1 == names.index("response_map") + 2


def test_solver_binding_checks_shapes_before_the_library():
    from bodge_amd.solver import DeviceSolver

    solver = object.__new__(DeviceSolver)
    solver.dim, solver.n_sites = 48, 12
    a, c = np.zeros((4, 4)), np.zeros((3, 3))
    for args in (([0, 1, 2, 3], a, np.zeros((3, 2)), [0]), ([0, 1, 2, 3], a, np.zeros((0, 3, 3)), [0]),
                 ([0, 1, 2], a, c, [0]), ([], np.zeros((0, 0)), c, [0]), ([0, 1, 2, 3], a, c, [])):
        with pytest.raises(ValueError, match="response_map"):
            solver.response_map(1.0, *args)


def test_product_path_fails_loudly_without_gpu(hip_library):
    """No CPU fallback: without a device response_map() raises, it does not compute."""
    from bodge_amd import backend

    if backend.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device behaviour cannot be exercised here")
    system = cases.system_of("cube")
    with pytest.raises(RuntimeError, match="GPU|HIP"):
        system.response_map(corr.spin_operator(system, [(1, 1, 1)], "z"), temperature=0.5, moments=8)


# ------------------------------------------------------------------ end-to-end figures
def test_static_map_at_the_rules_moments_stays_inside_the_pin():
    """χ_zz(r) from S_z at the interior site of disordered_complex, T = 0.1, static, M from the moment rule: the
    restatement against dense_static at every site, relative to max|χ|.  The pin is that of the static test of
    correlation (1e-7).  Measured: M = 507, max|χ| 0.303, distance 4.9e-14 of it."""
    M, restated, exact, figures = cases.end_to_end("static")
    print("static: moments", M, "max|chi|", np.abs(exact).max(), "restated - dense, relative", figures)
    assert restated.shape == exact.shape == (1, cases.system_of("disordered_complex").lattice.size)
    assert np.abs(exact).max() > 1e-3
    assert figures.max() <= cases.END_TO_END["static_pin"]


def test_dynamic_map_at_the_rules_moments_stays_inside_the_pin():
    """The same map with ω = 0 and 0.7, T = η = 0.5 against dense_response, pin 1e-11 as the response test of
    correlation.  Measured: M = 325, max|χ| 0.279 / 0.273, distance 4.1e-15 / 7.2e-15 of it."""
    M, restated, exact, figures = cases.end_to_end("response")
    print("response: moments", M, "max|chi|", np.abs(exact).max(axis=1), "restated - dense, relative", figures)
    assert restated.shape == exact.shape == (2, cases.system_of("disordered_complex").lattice.size)
    assert np.abs(exact).max() > 1e-3
    assert figures.max() <= cases.END_TO_END["response_pin"]


# ------------------------------------------------------------------ kernels
@pytest.mark.timeout(900)
def test_product_kernel_keeps_its_registers_and_nothing_spills():
    """resp_gemm uses no scratch and keeps two workgroups' worth of waves per SIMD, as corr_gram is pinned; the pick and
    the contraction do not spill."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    resources = kernel_resources.collect()
    gemm = {key: row for key, row in resources.items() if "resp_gemm" in key}
    assert gemm, sorted(key for key in resources if "resp" in key)
    for key, row in gemm.items():
        print(key, row)
        assert row["scratch"] == 0 and row["occupancy"] >= 2, (key, row)
    for name in ("resp_pick", "resp_contract"):
        rows = [row for key, row in resources.items() if f"bdg::{name}(" in key]
        assert len(rows) == 1 and rows[0]["scratch"] == 0, (name, rows)
