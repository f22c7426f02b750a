"""correlation() without a GPU: the two recurrences and the Gram product restated in numpy against the dense double
sum, the Kubo contractions of MomentMatrix, the operators, the argument errors of bdg_moment_matrix and the register
budget of the new kernels."""

import ctypes
import os
import shutil
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import correlation as corr

import correlation_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SYSTEMS = ["disordered_real", "disordered_complex", "dictionary", "cube"]


# ------------------------------------------------------------------ algorithm
@pytest.mark.parametrize("name", HOST_SYSTEMS)
@pytest.mark.parametrize("pair", ["jj", "js"])
def test_restatement_matches_dense_double_sum(name, pair):
    """M = 48.  "jj": A = B = J_x, exact trace; "js": A = J_x, B = S_z on one interior site, three unit vectors.  The
    largest |μ| must exceed 1e-3 (a pair that vanishes cannot pass) and the restatement must be within 1e-13 of it.
    Measured: largest entry 288 - 512 (jj) and 0.02 - 0.03 (js), error at most 2.3e-15 of it."""
    restated, dense, largest, distance = cases.references(name, pair, cases.M_SMALL)
    print(name, pair, "max|mu| =", largest, "restated - dense =", distance, "relative", distance / largest)
    assert restated.shape == dense.shape == (cases.M_SMALL, cases.M_SMALL)
    assert largest > 1e-3
    assert distance <= 1e-13 * largest


def _restated_moments(system, A, B, M):
    scale = cases.scale_of(system)
    mu = cases.restated_moment_matrix(system.matrix("csr"), scale, A, B, M, np.eye(4 * system.lattice.size))
    return ba.MomentMatrix(mu=mu, scale=scale, moments=M, info={"route": "restated"})


@pytest.fixture(scope="module")
def current_case():
    system = cases.system_of("disordered_complex")
    return system, corr.current_operator(system, 0)


def test_response_matches_the_dense_double_sum(current_case):
    """T = η = 0.5, ω = 0 and 0.7, the number of moments from moments_for_response: 325 at a = 5.5738 (printed).
    Relative error at most 1e-11.  Measured with the dense μ: 1.4e-6 / 5.0e-6 at M = 128, 2.0e-9 / 5.8e-9 at 192,
    2.4e-12 / 2.5e-11 at 256, 2.8e-14 / 5.6e-14 at 320: the pin fails a rule that returns fewer than about 260 moments.
    expand() does not warn at the rule's M, at either ω, and warns at M = 64."""
    system, jx = current_case
    scale = cases.scale_of(system)
    M = cheb.moments_for_response(scale, 0.5, 0.5)
    print("scale", scale, "moments", M)
    assert 300 <= M <= 350
    moments = _restated_moments(system, jx, jx, M)
    omegas = np.array([0.0, 0.7])
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (the rule's M has converged: expand does not warn)
        got = moments.response(omegas, 0.5, 0.5)
    for w, value in zip(omegas, got):
        exact = cases.dense_response(system, jx, jx, w, 0.5, 0.5)
        print("omega", w, value, exact, abs(value - exact) / abs(exact))
        assert abs(value - exact) <= 1e-11 * abs(exact)
    short = _restated_moments(system, jx, jx, 64)
    for w in omegas:
        with pytest.warns(RuntimeWarning, match="converged"):
            short.response([w], 0.5, 0.5)


def test_static_limit_matches_the_dense_divided_differences(current_case):
    """static(0.1) at M = 384: absolute error at most 1e-7.  The plain double sum is -57.47; static() is the ω = 0, η = 0
    limit of response() and carries its factor ½: -28.735 (measured error 5.0e-10, 1.0e-9 on the plain sum)."""
    system, jx = current_case
    moments = _restated_moments(system, jx, jx, 384)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = moments.static(0.1)
    exact = cases.dense_static(system, jx, jx, 0.1)
    print("static", got, exact, abs(got - exact))
    assert abs(2 * exact.real + 57.47) < 0.01
    assert abs(got - exact) <= 1e-7


def test_expand_is_a_plain_trace_and_moment_rule_has_its_form():
    system = cases.system_of("cube")
    jx = corr.current_operator(system, 0)
    moments = _restated_moments(system, jx, jx, 32)
    # F = 1: Tr[A B]; F = x y: Tr[H A H B]
    h = system.matrix("csr")
    assert abs(moments.expand(lambda x, y: np.ones(np.broadcast(x, y).shape)) - (jx @ jx).diagonal().sum()) < 1e-10
    assert abs(moments.expand(lambda x, y: x * y) - (h @ jx @ h @ jx).diagonal().sum()) < 1e-9
    # M = ceil(digits ln10 / asinh(γ / a)) + 16 with γ = min(η, πT), πT when η = 0
    for scale, t, eta, gamma in ((5.574, 0.5, 0.5, 0.5), (5.574, 0.05, 0.5, 0.05 * np.pi), (3.0, 0.2, 0.0, 0.2 * np.pi)):
        expected = int(np.ceil(12 * np.log(10.0) / np.arcsinh(gamma / scale))) + 16
        assert cheb.moments_for_response(scale, t, eta) == expected
    assert cheb.moments_for_response(5.574, 0.5, 0.5, digits=6) < cheb.moments_for_response(5.574, 0.5, 0.5)
    with pytest.raises(ValueError, match="temperature"):
        system.correlation(jx, jx)
    with pytest.raises(ValueError, match="temperature"):
        system.correlation(jx, jx, temperature=0.5)


# ------------------------------------------------------------------ operators
def test_current_operator_is_the_phase_derivative_of_the_matrix():
    system = cases.system_of("disordered_complex")
    jx = corr.current_operator(system, 0)
    step = 1e-6
    plus = cases.peierls_swave(step).matrix("csr")
    minus = cases.peierls_swave(-step).matrix("csr")
    assert abs(cases.peierls_swave(0.0).matrix("csr") - system.matrix("csr")).max() == 0
    difference = (plus - minus) / (2 * step)
    assert abs(jx).max() > 0.5
    assert abs(difference - jx).max() <= 1e-8
    assert abs(jx - jx.getH()).max() == 0
    # a periodic edge counts as one lattice constant, with the sign of the step across the face (no other block wraps)
    ring = cases.uniform_swave((5, 3, 1))
    with ring as (H, _):
        H.set_edges(-1.0 * ba.σ0, axis=0)
    edge = corr.current_operator(ring, 0)
    first, last = ring.lattice[(0, 1, 0)], ring.lattice[(4, 1, 0)]
    assert edge[4 * last, 4 * first] == -1j * (+1) * 1.0 and edge[4 * first, 4 * last] == -1j * (-1) * 1.0
    # along the axis without extent nothing flows; pairing blocks carry no phase
    assert corr.current_operator(system, 2).nnz == 0
    dense = jx.toarray().reshape(system.lattice.size, 4, system.lattice.size, 4)
    assert np.abs(dense[:, :2, :, 2:]).max() == 0 and np.abs(dense[:, 2:, :, :2]).max() == 0


def test_spin_operator_is_hermitian_and_particle_hole_symmetric():
    system = cases.system_of("cube")
    n = system.lattice.size
    tau_x = sp.kron(sp.identity(n), np.kron(np.array([[0, 1], [1, 0]]), np.eye(2))).tocsr()
    sites = [(1, 1, 1), (2, 0, 1)]
    for direction in (1, 2, 3, "x", "y", "z"):
        s = corr.spin_operator(system, sites, direction)
        assert s.shape == (4 * n, 4 * n) and abs(s - s.getH()).max() == 0
        assert abs(tau_x @ s.conj() @ tau_x + s).max() == 0  # S = -τx S* τx
        i = system.lattice[sites[0]]
        assert np.array_equal(s[4 * i : 4 * i + 2, 4 * i : 4 * i + 2].toarray(), ba.σ[_number(direction) - 1])
        assert s.nnz == 4 * len(sites)
    assert abs(corr.spin_operator(system, (1, 1, 1), 3) - corr.spin_operator(system, [(1, 1, 1)], "z")).max() == 0
    jx = corr.current_operator(system, 0)
    assert abs(tau_x @ jx.conj() @ tau_x + jx).max() == 0
    with pytest.raises(ValueError, match="direction"):
        corr.spin_operator(system, sites, 4)


def _number(direction):
    return {"x": 1, "y": 2, "z": 3}.get(direction, direction)


def test_as_operator_round_trips_its_input_kinds():
    system = cases.system_of("disordered_complex")
    indptr, indices, data = corr.as_operator(system, system)
    assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.complex128
    reference = system.bsr_arrays()
    for got, expected in zip((indptr, indices, data), reference):
        assert np.array_equal(got, expected)
    kinds = {"hamiltonian": system, "sparse": system.matrix("csr"), "dense": np.asarray(system.matrix("dense")),
             "blocks": system._data.copy(), "bsr": system.matrix("bsr"), "coo": system.matrix("csr").tocoo()}
    for label, given in kinds.items():
        triple = corr.as_operator(system, given)
        for got, expected in zip(triple, (indptr, indices, data)):
            assert got.dtype == expected.dtype and np.array_equal(got, expected), label
    # an operator with its own, smaller pattern
    sz = corr.spin_operator(system, [(4, 4, 0)], 3)
    ptr, idx, blocks = corr.as_operator(system, sz)
    assert blocks.shape == (1, 4, 4) and idx[0] == system.lattice[(4, 4, 0)] and ptr[-1] == 1
    assert np.array_equal(blocks[0], np.diag([1, -1, -1, 1]))
    for bad in (np.zeros((3, 3)), sp.identity(8).tocsr(), np.zeros((5, 4, 4)), "J"):
        with pytest.raises(ValueError, match="operator"):
            corr.as_operator(system, bad)


# ------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_without_a_gpu(hip_library):
    """bdg_moment_matrix checks counts, scale, pointers, the rows / x choice and the operators' own arrays before it looks
    at the handle, so each refusal is reachable here without one, in this order; what needs the matrix size (indptr[nb],
    the column indices) and the slab refusal need a handle and are in tests/test_gpu_correlation.py."""
    from bodge_amd import backend

    one = np.zeros(2)
    ptr = backend.as_f64p(one)
    rows = backend.as_i64p(np.zeros(1, dtype=np.int64))
    indptr = np.zeros(2, dtype=np.int32)
    indices = np.zeros(1, dtype=np.int32)
    good = backend.Operator(0, backend.as_i32p(indptr), backend.as_i32p(indices), ptr)
    negative = backend.Operator(-1, backend.as_i32p(indptr), backend.as_i32p(indices), ptr)
    hollow = backend.Operator(1, backend.as_i32p(indptr), None, ptr)
    a = ctypes.byref(good)
    call = hip_library.bdg_moment_matrix
    for args, message in (
        ((None, 1.0, 0, a, a, 1, rows, None, ptr), b"n_moments"),
        ((None, -1.0, 0, None, None, 0, None, None, None), b"n_moments"),
        ((None, 1.0, 1, a, a, 0, rows, None, ptr), b"n_vectors"),
        ((None, 0.0, 1, a, a, 0, rows, None, ptr), b"n_vectors"),
        ((None, 0.0, 1, a, a, 1, rows, None, ptr), b"scale"),
        ((None, float("nan"), 1, None, a, 1, rows, None, ptr), b"scale"),
        ((None, 1.0, 1, None, a, 1, rows, None, ptr), b"null argument"),
        ((None, 1.0, 1, a, None, 1, rows, ptr, ptr), b"null argument"),
        ((None, 1.0, 1, a, a, 1, rows, None, None), b"null argument"),
        ((None, 1.0, 1, a, a, 1, rows, ptr, ptr), b"exactly one"),
        ((None, 1.0, 1, a, a, 1, None, None, ptr), b"exactly one"),
        ((None, 1.0, 1, ctypes.byref(negative), a, 1, rows, None, ptr), b"operator A"),
        ((None, 1.0, 1, a, ctypes.byref(hollow), 1, None, ptr, ptr), b"operator B"),
        ((None, 1.0, 1, a, a, 1, rows, None, ptr), b"null system handle"),
        ((None, 1.0, 1, a, a, 1, None, ptr, ptr), b"null system handle"),
    ):
        assert call(*args) == -1 and message in hip_library.bdg_last_error(), (args[1:3], args[5], message)
    assert "bdg_moment_matrix" in backend.SIGNATURES
    for field in (("correlation", ctypes.c_int32), ("gram_ms", ctypes.c_double), ("gram_flops", ctypes.c_double)):
        assert field in backend.Perf._fields_[-3:]


def test_solver_binding_checks_shapes_before_the_library():
    from bodge_amd.solver import DeviceSolver

    solver = object.__new__(DeviceSolver)
    solver.dim, solver.n_sites = 48, 12
    op = (np.zeros(13, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 4, 4)))
    x = np.zeros((2, 48), dtype=np.complex128)
    for kwargs in ({}, {"rows": [0], "x": x}, {"x": x[:, :47]}, {"x": x[0]}, {"rows": []}, {"x": x[:0]}):
        with pytest.raises(ValueError, match="moment_matrix"):
            solver.moment_matrix(1.0, 4, op, op, **kwargs)
    with pytest.raises(ValueError, match="moment_matrix"):
        solver.moment_matrix(1.0, 0, op, op, rows=[0])
    with pytest.raises(ValueError, match="operator A"):
        solver.moment_matrix(1.0, 4, (op[0][:-1], op[1], op[2]), op, rows=[0])


def test_product_path_fails_loudly_without_gpu(hip_library):
    """No CPU fallback: without a device correlation() raises, it does not compute."""
    from bodge_amd import backend

    if backend.device_count() > 0:
        pytest.skip("a GPU is visible; the no-device behaviour cannot be exercised here")
    system = cases.system_of("cube")
    jx = corr.current_operator(system, 0)
    with pytest.raises(RuntimeError, match="GPU|HIP"):
        system.correlation(jx, jx, moments=8)


# ------------------------------------------------------------------ kernels
@pytest.mark.timeout(900)
def test_gram_kernel_keeps_its_registers_and_nothing_spills():
    """Every emitted instance of corr_gram uses no scratch and keeps two workgroups' worth of waves per SIMD; the
    operator and the reduction kernel do not spill."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    resources = kernel_resources.collect()
    gram = {key: row for key, row in resources.items() if "corr_gram" in key}
    assert gram, sorted(key for key in resources if "corr" in key)
    for key, row in gram.items():
        print(key, row)
        assert row["scratch"] == 0 and row["occupancy"] >= 2, (key, row)
    for name in ("corr_operator", "corr_reduce"):
        rows = [row for key, row in resources.items() if f"bdg::{name}(" in key]
        assert len(rows) == 1 and rows[0]["scratch"] == 0, (name, rows)
