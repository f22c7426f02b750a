"""Two-operator response functions of H without a diagonalisation (`Hamiltonian.correlation`).

Everything of the form Σ_ab A_ab B_ba F(E_a, E_b) - a current-current response, a spin susceptibility between two
sites, any Kubo formula - is one contraction away from the matrix of double Chebyshev moments

    μ[n, m] = Tr[T_n(H~) A T_m(H~) B] = Σ_ab T_n(E~_a) A_ab T_m(E~_b) B_ba,     H~ = H / scale,  n, m < M

which the GPU computes (`bdg_moment_matrix`): two Chebyshev recurrences per batch of start vectors
and a tall-skinny complex Gram product on the fp64 matrix cores.  The host makes the operators, the start vectors
and the coefficients c_nm of F, and contracts.

`mu` and `expand` are plain traces over the 4N Nambu states.  `response` and `static` carry the factor ½ that undoes
the Nambu double counting for particle-hole symmetric A and B, as `FermiMatrix.expectation` does.
"""

from __future__ import annotations

import warnings
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from .common import typecheck


# ---------------------------------------------------------------- operators
def _canonical_triple(matrix: sp.bsr_matrix) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    matrix = sp.bsr_matrix(matrix, blocksize=(4, 4), copy=True)
    matrix.sum_duplicates()
    matrix.eliminate_zeros()  # (whole zero blocks leave the pattern)
    matrix.sort_indices()
    return (np.ascontiguousarray(matrix.indptr, dtype=np.int32), np.ascontiguousarray(matrix.indices, dtype=np.int32),
            np.ascontiguousarray(matrix.data, dtype=np.complex128).reshape(-1, 4, 4))


def as_operator(system, op) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """BSR triple (indptr int32, indices int32, data (nnzb, 4, 4) complex128) of an operator on the lattice of `system`,
    canonical (sorted, no duplicates, no all-zero blocks).  `op`: a Hamiltonian on the same lattice (its blocks), a
    scipy sparse or dense (4N, 4N) matrix, or a (nnzb, 4, 4) block array on the block pattern of `system`."""
    n = system.lattice.size
    pattern = system._matrix
    if hasattr(op, "_matrix") and hasattr(op, "lattice"):
        if op.lattice.size != n or op._matrix.shape != pattern.shape:
            raise ValueError("operator: the Hamiltonian lives on another lattice")
        return _canonical_triple(op._matrix)
    if sp.issparse(op):
        if op.shape != (4 * n, 4 * n):
            raise ValueError(f"operator: expected a ({4 * n}, {4 * n}) matrix, got {op.shape}")
        return _canonical_triple(sp.csr_matrix(op, dtype=np.complex128))
    array = np.asarray(op)
    if array.dtype == object or not np.issubdtype(array.dtype, np.number):
        raise ValueError("operator: expected a Hamiltonian, a matrix or an array of blocks")
    if array.ndim == 3 and array.shape == pattern.data.shape:
        return _canonical_triple(sp.bsr_matrix((array.astype(np.complex128), pattern.indices, pattern.indptr),
                                               shape=pattern.shape, blocksize=(4, 4)))
    if array.ndim == 2 and array.shape == (4 * n, 4 * n):
        return _canonical_triple(sp.csr_matrix(array.astype(np.complex128)))
    raise ValueError(f"operator: expected a ({4 * n}, {4 * n}) matrix or blocks of shape {pattern.data.shape}, got {array.shape}")


EXPAND_TAIL = 16  # rows and columns of the coefficients `expand` looks at: the margin of `moments_for_response`

_DIRECTIONS = {1: 1, 2: 2, 3: 3, "x": 1, "y": 2, "z": 3}


def spin_operator(system, sites, direction) -> sp.csr_matrix:
    """Σ_{i in sites} of the spin component `direction` (1, 2, 3 or "x", "y", "z") in Nambu form: the on-site block
    diag(σ_k, -σ_k*) on every given site (a coordinate or a list of them).  Hermitian and particle-hole symmetric, so
    ½ Tr[f(H) S] is the spin expectation in units of ħ/2.  Returns scipy CSR (4N, 4N)."""
    from .common import σ1, σ2, σ3

    if direction not in _DIRECTIONS:
        raise ValueError("spin_operator: direction must be 1, 2, 3 or 'x', 'y', 'z'")
    pauli = np.asarray((σ1, σ2, σ3)[_DIRECTIONS[direction] - 1], dtype=np.complex128)
    block = np.zeros((4, 4), dtype=np.complex128)
    block[:2, :2] = pauli
    block[2:, 2:] = -pauli.conj()
    if len(sites) == 3 and all(isinstance(v, (int, np.integer)) for v in sites):
        sites = [sites]
    index = np.unique(np.array([system.lattice[tuple(int(v) for v in site)] for site in sites], dtype=np.int64))
    n = system.lattice.size
    rows = (4 * index[:, None, None] + np.arange(4)[None, :, None]) + np.zeros((1, 1, 4), dtype=np.int64)
    cols = (4 * index[:, None, None] + np.arange(4)[None, None, :]) + np.zeros((1, 4, 1), dtype=np.int64)
    values = np.broadcast_to(block, (len(index), 4, 4))
    out = sp.csr_matrix((values.reshape(-1), (rows.reshape(-1), cols.reshape(-1))), shape=(4 * n, 4 * n))
    out.eliminate_zeros()
    return out


def current_operator(system, axis: int) -> sp.csr_matrix:
    """J = ∂H/∂φ at φ = 0 for the Peierls phase φ per lattice constant along `axis` (0, 1, 2): every normal block
    between the sites i (row) and j (column) is multiplied by exp(iφ(x_j - x_i)) in the electron sector, the hole
    sector follows as -conj(·), so the block of J is diag(i (x_j - x_i) h_ij, -conj(i (x_j - x_i) h_ij)) with h_ij
    the electron 2x2 block of H.  Pairing blocks carry no phase (a uniform vector potential leaves the on-site and
    the bond pairing of this model untouched), so they do not enter.  Only across a periodic edge of the lattice
    (`edge_array(axis)`: opposite faces) x_j - x_i is the nearest-image distance; every other block keeps its own.
    Hermitian and particle-hole symmetric.  Returns scipy CSR (4N, 4N)."""
    if axis not in (0, 1, 2):
        raise ValueError("current_operator: axis must be 0, 1 or 2")
    lattice = system.lattice
    if not hasattr(lattice, "site_array"):
        raise ValueError("current_operator: the lattice has no site coordinates")
    position = np.asarray(lattice.site_array(), dtype=np.float64)[:, axis]
    n = lattice.size
    matrix = system._matrix
    block_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(matrix.indptr))
    distance = position[matrix.indices.astype(np.int64)] - position[block_rows]
    extent = int(lattice.shape[axis])
    if extent > 2 and hasattr(lattice, "edge_array"):
        # only the blocks of the periodic edges wrap: site pairs on opposite faces, one lattice constant apart
        edges = np.asarray(lattice.edge_array(axis), dtype=np.int64).reshape(-1, 2)
        wrapped = np.isin(block_rows * n + matrix.indices.astype(np.int64), edges[:, 0] * n + edges[:, 1])
        distance = np.where(wrapped, distance - extent * np.sign(distance), distance)
    data = np.zeros_like(system._data)
    data[:, :2, :2] = 1j * distance[:, None, None] * system._data[:, :2, :2]
    data[:, 2:, 2:] = -data[:, :2, :2].conj()
    out = sp.bsr_matrix((data, matrix.indices, matrix.indptr), shape=matrix.shape, blocksize=(4, 4)).tocsr()
    out.eliminate_zeros()
    return out


# ---------------------------------------------------------------- the Kubo kernels
def _fermi_difference_quotient(x, y, temperature: float):
    """(f(x) - f(y)) / (x - y) with f′ on the diagonal.  f(x) - f(y) = -sinh(u - v) / (2 cosh u cosh v) with u = x/2T,
    v = y/2T: close to the diagonal the quotient is -sinh(d)/d · sech u · sech v / 4T (no cancellation), elsewhere the
    difference of the two tanh is taken as it stands."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    u, v = x / (2.0 * temperature), y / (2.0 * temperature)
    d = u - v
    near = np.abs(d) < 1.0
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        safe = np.where(d == 0.0, 1.0, d)
        sinhc = np.where(d == 0.0, 1.0, np.sinh(np.where(near, safe, 1.0)) / np.where(near, safe, 1.0))
        close = -sinhc / (np.cosh(u) * np.cosh(v)) / (4.0 * temperature)
        far = -0.5 * (np.tanh(u) - np.tanh(v)) / np.where(near, 1.0, x - y)
    return np.where(near, close, far)


def random_phase_vectors(system, count: int, seed: int = 0) -> np.ndarray:
    """(count, 4N) vectors with entries exp(iθ), θ uniform in [0, 2π) from numpy.random.default_rng(seed): E[v v†] = 1,
    so the mean of <v|O|v> over them is an unbiased estimate of Tr O."""
    rng = np.random.default_rng(seed)
    return np.exp(2j * np.pi * rng.random((int(count), 4 * system.lattice.size)))


@dataclass
class MomentMatrix:
    """Double Chebyshev moments of two operators A and B on the spectrum of H.

    mu       (M, M) complex128, μ[n, m] = Tr[T_n(H/scale) A T_m(H/scale) B]: a plain trace over the 4N Nambu states
             (for `vectors=R` its stochastic estimate, for caller vectors Σ_v <v|…|v>)
    scale    half-width of the band the polynomials live on
    moments  M
    info     route, number of start vectors, the device's performance record
    """

    mu: np.ndarray
    scale: float
    moments: int
    info: dict = field(default_factory=dict)

    def expand(self, F, digits: float = 12) -> complex:
        """Σ_ab A_ab B_ba F(E_a, E_b) = Σ_nm c_nm μ_nm for a function F(x, y) of two energies (not scaled; it must
        broadcast) that is smooth on the band: a plain trace, no factor ½.  c = `chebyshev_coefficients_2d(F, scale,
        M)`.  Warns when the last min(M/8, 16) rows or columns of c exceed 10^-digits of its largest entry: the series
        has not converged at this number of moments.  (16 is the margin `moments_for_response` adds beyond the order
        at which its estimate of the coefficients reaches 10^-digits: the rule's own M does not warn.)"""
        from .chebyshev import chebyshev_coefficients_2d

        c = chebyshev_coefficients_2d(F, self.scale, self.moments)
        size = np.abs(c)
        tail = max(1, min(self.moments // 8, EXPAND_TAIL))
        largest = float(size.max(initial=0.0))
        edge = max(float(size[-tail:, :].max(initial=0.0)), float(size[:, -tail:].max(initial=0.0)))
        if largest > 0 and edge > 10.0 ** (-float(digits)) * largest:
            warnings.warn(f"expand: the last {tail} rows or columns of the coefficients reach {edge / largest:.1e} of the "
                          f"largest one: {self.moments} moments have not converged to 1e-{float(digits):g}", RuntimeWarning,
                          stacklevel=2)
        return complex(np.sum(c * self.mu))

    def response(self, omega, temperature: float, broadening: float, digits: float = 12) -> np.ndarray:
        """χ_AB(ω) = ½ Σ_ab A_ab B_ba (f(E_a) - f(E_b)) / (ω + iη + E_a - E_b) for an array of ω (η = `broadening` > 0,
        f the Fermi function at `temperature`).  The ½ undoes the Nambu double counting for particle-hole symmetric
        A and B."""
        from .chebyshev import fermi_function

        if not temperature > 0:
            raise ValueError("response: the temperature must be positive")
        if not broadening > 0:
            raise ValueError("response: the broadening must be positive (static() is the ω = 0, η = 0 limit)")
        omegas = np.asarray(omega, dtype=np.float64)
        out = np.empty(omegas.size, dtype=np.complex128)
        for k, w in enumerate(omegas.reshape(-1)):
            out[k] = 0.5 * self.expand(
                lambda x, y: (fermi_function(x, temperature) - fermi_function(y, temperature)) / (w + 1j * broadening + x - y),
                digits)
        return out.reshape(omegas.shape)

    def static(self, temperature: float, digits: float = 12) -> complex:
        """The ω = 0, η = 0 limit of `response`: ½ Σ_ab A_ab B_ba (f(E_a) - f(E_b)) / (E_a - E_b), the divided
        difference evaluated stably with f′(E_a) on the diagonal (degenerate levels included)."""
        if not temperature > 0:
            raise ValueError("static: the temperature must be positive")
        return 0.5 * self.expand(lambda x, y: _fermi_difference_quotient(x, y, temperature), digits)


# ---------------------------------------------------------------- the call
@typecheck
def correlation(system, A, B, *, moments: int | None = None, vectors=None, seed: int = 0,
                scale: float | int | None = None, temperature: float | int | None = None,
                broadening: float | int | None = None, digits: float | int = 12) -> MomentMatrix:
    """μ[n, m] = Tr[T_n(H~) A T_m(H~) B] on the GPU (see `Hamiltonian.correlation`).

    `A`, `B`: anything `as_operator` takes.  `vectors=None`: the exact trace over all 4N unit vectors; an integer R:
    the mean over R random-phase vectors from numpy.random.default_rng(seed), an unbiased estimate of the trace; an
    array in the layouts of `apply`: Σ_v <v|…|v> over the vectors as given.  `moments=None` takes
    `moments_for_response(scale, temperature, broadening, digits)` and needs both.  `scale` defaults to 1.01 x the
    Gershgorin bound."""
    from .apply import _to_rows
    from .chebyshev import moments_for_response
    from .observables import _scale_of

    scale = _scale_of(system) if scale is None else float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("correlation: scale must be positive")
    if moments is None:
        if temperature is None or broadening is None:
            raise ValueError("correlation: give moments=, or temperature= and broadening= for the automatic number")
        moments = moments_for_response(scale, float(temperature), float(broadening), float(digits))
    if moments < 1:
        raise ValueError("correlation: moments must be >= 1")
    a, b = as_operator(system, A), as_operator(system, B)
    solver = system._solver()
    if vectors is None:
        mu = solver.moment_matrix(scale, moments, a, b, rows=np.arange(4 * system.lattice.size, dtype=np.int64))
        route, count = "exact", 4 * system.lattice.size
    elif isinstance(vectors, (int, np.integer)) and not isinstance(vectors, bool):
        if vectors < 1:
            raise ValueError("correlation: vectors must be >= 1")
        mu = solver.moment_matrix(scale, moments, a, b, x=random_phase_vectors(system, int(vectors), seed)) / int(vectors)
        route, count = "stochastic", int(vectors)
    else:
        rows, _ = _to_rows(system, vectors)
        mu = solver.moment_matrix(scale, moments, a, b, x=rows)
        route, count = "vectors", rows.shape[0]
    return MomentMatrix(mu=mu, scale=scale, moments=int(moments), info={"route": route, "vectors": count, "perf": solver.perf()})
