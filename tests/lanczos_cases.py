"""Shared by tests/test_lanczos_host.py and tests/test_gpu_lanczos.py: the systems, the numpy restatements of the
Lanczos process on H^2 (csrc/lanczos.hpp), of the Ritz accumulation and of the device Rayleigh-Ritz step, and a
solver object with the Lanczos signatures of `DeviceSolver` that runs on them."""

import functools

import numpy as np
import scipy.sparse as sp

import bodge_amd as ba
import systems
from oracle import cheb_ref

LD = np.longdouble
CLD = np.clongdouble


# ------------------------------------------------------------------ systems
def swave(shape, mu=3.0, gap=0.3, zeeman=0.05, flux=0.0, disorder=0.0, seed=7):
    """s-wave lattice H_ii = (μ + w_i) σ0 - m σ3, Δ_ii = -Δ0 jσ2, bonds -σ0 (open edges).  `flux` puts the Peierls
    phase exp(±i·flux·y) on the x bonds (a complex matrix); `disorder` draws w_i uniformly from ±disorder (every
    diagonal block different)."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    system.hermiticity_check = "host"
    potential = np.zeros(lattice.size)
    if disorder:
        potential = disorder * (2.0 * np.random.default_rng(seed).random(lattice.size) - 1.0)
    with system as (H, Δ):
        H.set_sites((mu + potential)[:, None, None] * ba.σ0 - zeeman * ba.σ3)
        Δ.set_sites(-gap * ba.jσ2)
        if flux:
            pairs = lattice.bond_array(axis=0, coords=True)        # (B, 2, 3): i -> j
            phase = np.exp(1j * flux * pairs[:, 0, 1] * (pairs[:, 1, 0] - pairs[:, 0, 0]))
            H.set_bonds(-phase[:, None, None] * ba.σ0, axis=0)
            for axis in (1, 2):
                H.set_bonds(-1.0 * ba.σ0, axis=axis)
        else:
            H.set_bonds(-1.0 * ba.σ0)
    return system


def _random357():
    spec = systems.CATALOG["random357"]
    return spec["build"](ba, **spec["kwargs"])


SYSTEMS = {
    "chain101": lambda: swave((101, 1, 1)),                              # rows of <= 3 blocks
    "plane9x13": lambda: swave((9, 13, 1)),                              # <= 5 blocks; 117 sites: two ragged 64-row tiles
    "plane9x13_flux": lambda: swave((9, 13, 1), zeeman=0.0, flux=0.3),   # complex, every level two-fold
    "cube5x6x7": lambda: swave((5, 6, 7)),                               # <= 7 blocks
    "square12": lambda: swave((12, 12, 1), zeeman=0.0),                  # levels 0.30005914 x2, 0.3099775 x4
    "plane10x12_flux": lambda: swave((10, 12, 1), zeeman=0.0, flux=0.3),  # 0.01621189, 0.06723201, 0.07192748, x2 each
    "disorder17x16": lambda: swave((17, 16, 1), disorder=0.5),           # 272 distinct diagonal blocks: streamed
    "random357": _random357,                                             # no stencil: rows of 13 complex blocks
    "plane33x32": lambda: swave((33, 32, 1)),                            # grid-stride sizes only
    "plane130x127": lambda: swave((130, 127, 1)),                        # grid-stride sizes only (float64 reference)
    "swave20": lambda: systems.swave_square(ba),
}
SMALL = ("chain101", "plane9x13", "plane9x13_flux", "cube5x6x7", "square12", "plane10x12_flux", "disorder17x16",
         "random357")
HORIZON = 16        # iterations over which trajectories are compared (never beyond 24: round-off amplification)
LOCAL_HORIZON = 64  # iterations over which the local relations are checked


@functools.lru_cache(maxsize=None)
def build(name):
    return SYSTEMS[name]()


@functools.lru_cache(maxsize=None)
def sparse_matrix(name):
    """float64 form: scipy CSR, complex128."""
    return sp.csr_matrix(build(name).matrix("csr"), dtype=np.complex128)


@functools.lru_cache(maxsize=None)
def dense_long_double(name):
    """Dense np.clongdouble form (small systems)."""
    return np.asarray(build(name).matrix("dense")).astype(CLD)


class SparseLongDouble:
    """The CSR matrix with np.clongdouble products (scipy has none): what the local checks on many vectors use."""

    def __init__(self, csr):
        csr = sp.csr_matrix(csr)
        csr.sort_indices()
        assert np.all(np.diff(csr.indptr) > 0), "a row without entries (np.add.reduceat needs one per row)"
        self.shape = csr.shape
        self._data = csr.data.astype(CLD)
        self._indices, self._starts = csr.indices, csr.indptr[:-1]

    def __matmul__(self, x):
        x = np.asarray(x, dtype=CLD)
        flat = x.reshape(x.shape[0], -1)
        out = np.add.reduceat(self._data[:, None] * flat[self._indices], self._starts, axis=0)
        return out.reshape(x.shape)


@functools.lru_cache(maxsize=None)
def sparse_long_double(name):
    return SparseLongDouble(sparse_matrix(name))


@functools.lru_cache(maxsize=None)
def norm_bound(name):
    """‖H‖ as every distance here measures it: the Gershgorin bound (the same number for a lattice of any size)."""
    return float(build(name).gershgorin_bound())


@functools.lru_cache(maxsize=None)
def dense_eigh(name):
    return np.linalg.eigh(np.asarray(build(name).matrix("dense")))


def start_block(name, n_vectors, seed, kind, first_id=0):
    return cheb_ref.random_block(4 * build(name).lattice.size, seed, range(first_id, first_id + n_vectors), kind)


# ------------------------------------------------------------------ references
def _complex_of(dtype):
    return CLD if np.dtype(dtype) in (np.dtype(LD), np.dtype(CLD)) else np.complex128


def _squares(w):
    """Σ_rows |w|² per column, summed pairwise: numpy adds the rows of a 2-D array one after the other (a running sum
    loses ~sqrt(rows)·2^-53, which at 66 040 rows is well above what the device's tree of partial sums loses), and
    pairwise only along a contiguous last axis (oracle/cheb_ref._column_dots does the same)."""
    return np.sum(np.ascontiguousarray((w.real * w.real + w.imag * w.imag).T), axis=1)


def _norms(w):
    return np.sqrt(_squares(w))


def lanczos_step(matrix, v, previous, b_prev):
    """One iteration on every column: (α_j, β_{j+1}, v_{j+1}) from v_j, v_{j-1} and β_j."""
    u = matrix @ v
    alpha = _squares(u)
    w = (matrix @ u) - b_prev * previous - alpha * v
    beta = _norms(w)
    return alpha, beta, w / beta


def lanczos_reference(matrix, v0, m, dtype=np.float64):
    """The three-term process on H^2 as csrc/lanczos.hpp states it, on every column of v0 (n, C) independently:
        v_0 = v0/|v0|;  u = H v_j;  α_j = |u|^2;  w = H u - β_j v_{j-1} - α_j v_j;  β_{j+1} = |w|;  v_{j+1} = w/β_{j+1}
    `matrix` is anything with a product in the arithmetic of `dtype` (float64: scipy sparse; long double: a dense
    np.clongdouble array or `SparseLongDouble`).  Returns α (m, C), β (m, C) with β[j] = β_{j+1} (the rows
    `lanczos_advance` returns) and V (m + 1, n, C)."""
    ctype = _complex_of(dtype)
    v0 = np.asarray(v0, dtype=ctype)
    v0 = v0.reshape(v0.shape[0], -1)
    real = np.zeros(0, dtype=ctype).real.dtype
    alpha = np.zeros((m, v0.shape[1]), dtype=real)
    beta = np.zeros((m, v0.shape[1]), dtype=real)
    vectors = np.zeros((m + 1,) + v0.shape, dtype=ctype)
    vectors[0] = v0 / _norms(v0)
    previous, b_prev = np.zeros_like(v0), np.zeros(v0.shape[1], dtype=real)
    for j in range(m):
        alpha[j], beta[j], vectors[j + 1] = lanczos_step(matrix, vectors[j], previous, b_prev)
        previous, b_prev = vectors[j], beta[j]
    return alpha, beta, vectors


def ritz_accumulate_reference(vectors, coef):
    """y[l, c, :] = Σ_j coef[j, l, c] v_j^(c), in long double.  vectors (>= n_iter, n, C), coef (n_iter, L, C)."""
    coef = np.asarray(coef, dtype=LD)
    out = np.zeros((coef.shape[1], coef.shape[2], vectors.shape[1]), dtype=CLD)
    for j in range(coef.shape[0]):
        out += coef[j][:, :, None] * np.asarray(vectors[j], dtype=CLD).T[None, :, :]
    return out


def _orthonormal_combinations(gram, cut, symmetric):
    """`combinations` of lanczos_ritz_pairs: M with B = Z M orthonormal, from the Gram matrix G = Z^H Z through the
    eigen-decomposition of its unit-diagonal form; weights above cut·largest, largest first."""
    norm = np.sqrt(np.maximum(np.diag(gram).real, 0.0))
    weight, u = np.linalg.eigh(gram / np.outer(norm, norm))
    keep = [e for e in range(len(weight) - 1, -1, -1) if weight[e] > cut * weight[-1]]
    scaled = u[:, keep] / np.sqrt(weight[keep]) / norm[:, None]
    return scaled @ u[:, keep].conj().T if symmetric else scaled


def ritz_pairs_reference(matrix, ritz, eps, rank_tol=1e-4):
    """The steps of lanczos_ritz_pairs on a block of Ritz vectors of H^2, ritz (L, C, n), with its rules:
    Z = (H + ε) Y; columns whose squared norm is <= 1e-12 of the longest dropped; eigen-decomposition of the
    unit-diagonal Gram matrix, weights above rank_tol·largest kept; Loewdin; S = B^H H B, Hermitian part, eigh.
    Returns (values ascending (K,), vectors (K, n), states found per level (L,))."""
    values, states, found = [], [], []
    for block, e in zip(ritz, eps):
        y = np.asarray(block, dtype=np.complex128).T                     # (n, C)
        z = matrix @ y + e * y
        length2 = np.sum(np.abs(z) ** 2, axis=0)
        use = np.flatnonzero(length2 > 1e-12 * length2.max()) if length2.max() > 0 else []
        if len(use) == 0:
            found.append(0)
            continue
        z = z[:, use]
        basis = z @ _orthonormal_combinations(z.conj().T @ z, rank_tol, False)
        basis = basis @ _orthonormal_combinations(basis.conj().T @ basis, 0.0, True)
        small = basis.conj().T @ (matrix @ basis)
        energy, rotation = np.linalg.eigh(0.5 * (small + small.conj().T))
        final = basis @ rotation
        values.extend(energy)
        states.extend(final.T)
        found.append(len(energy))
    order = np.argsort(np.asarray(values), kind="stable")
    dim = matrix.shape[0]
    vectors = np.array([states[i] for i in order], dtype=np.complex128).reshape(len(order), dim)
    return np.asarray(values)[order], vectors, np.asarray(found)


# ------------------------------------------------------------------ a solver on the references
class NumpyLanczosSolver:
    """`DeviceSolver`'s Lanczos calls (and spmv) on the float64 restatements, for the front-end logic of
    `observables.lowest_eigenvalues` / `lowest_eigenpairs` without a device."""

    def __init__(self, matrix):
        self.matrix = sp.csr_matrix(matrix, dtype=np.complex128)
        self.dim = self.matrix.shape[0]
        self.n_sites = self.dim // 4
        self._run = None

    @classmethod
    def from_hamiltonian(cls, system, device=None):
        return cls(system.matrix("csr"))

    def spmv(self, x):
        self._run = None
        return self.matrix @ np.asarray(x, dtype=np.complex128).reshape(-1)

    def lanczos_begin(self, n_vectors, seed=0, first_id=0, kind=cheb_ref.VEC_RADEMACHER, max_iter=10000):
        if not 1 <= n_vectors <= 64:
            raise ValueError("bodge_hip: Lanczos runs 1..64 start vectors")
        if not 1 <= max_iter <= 1 << 20:
            raise ValueError("bodge_hip: bad iteration limit")
        if kind not in (cheb_ref.VEC_RADEMACHER, cheb_ref.VEC_Z4):
            raise ValueError("bodge_hip: unknown vector kind")
        start = cheb_ref.random_block(self.dim, seed, range(first_id, first_id + n_vectors), kind)
        self._run = dict(v=start / _norms(start), previous=np.zeros_like(start), beta=np.zeros(n_vectors), iter=0,
                         max_iter=max_iter, n=n_vectors)

    def _iterate(self):
        run = self._run
        alpha, beta, following = lanczos_step(self.matrix, run["v"], run["previous"], run["beta"])
        run["previous"], run["v"], run["beta"] = run["v"], following, beta
        run["iter"] += 1
        return alpha, beta

    def lanczos_advance(self, n_iter):
        run = self._run
        if run is None:
            raise ValueError("bodge_hip: lanczos_begin has not been called on this handle")
        if n_iter < 1 or run["iter"] + n_iter > run["max_iter"]:
            raise ValueError("bodge_hip: iteration count exceeds the limit given to bdg_lanczos_begin")
        rows = [self._iterate() for _ in range(n_iter)]
        return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])

    def _ritz_block(self, coef):
        run = self._run
        coef = np.asarray(coef, dtype=np.float64)
        if run is None or coef.ndim != 3 or coef.shape[2] != run["n"]:
            raise ValueError("bodge_hip: coefficients must be (iterations, levels, start vectors of lanczos_begin)")
        if run["iter"] != 0:
            raise ValueError("bodge_hip: the Ritz-vector pass starts from a freshly begun process")
        if not (1 <= coef.shape[0] <= run["max_iter"] and 1 <= coef.shape[1] <= 64):
            raise ValueError("bodge_hip: bad iteration or level count")
        out = np.zeros((coef.shape[1], run["n"], self.dim), dtype=np.complex128)
        for j in range(coef.shape[0]):
            out += coef[j][:, :, None] * run["v"].T[None, :, :]
            self._iterate()
        return out

    def lanczos_ritz_vectors(self, coef):
        return self._ritz_block(coef)

    def lanczos_ritz_pairs(self, coef, eps, k, rank_tol=1e-4):
        eps = np.asarray(eps, dtype=np.float64)
        if self._run is not None and self._run["n"] > 16:
            raise ValueError("bodge_hip: Rayleigh-Ritz on the device handles at most 16 columns")
        if not 0.0 <= rank_tol < 1.0:
            raise ValueError("bodge_hip: bad rank tolerance")
        block = self._ritz_block(coef)
        if eps.shape != (block.shape[0],):
            raise ValueError("bodge_hip: eps must be (levels,)")
        values, vectors, found = ritz_pairs_reference(self.matrix, block, eps, rank_tol)
        self._run = None
        return values[:k], vectors[:k], int(found.sum())


# ------------------------------------------------------------------ figures shared by the host and the GPU tests
def trajectory_distance(name, got_alpha, got_beta, ref_alpha, ref_beta):
    """max |Δα|, |Δβ| over the rows given, relative to ‖H‖²."""
    scale2 = norm_bound(name) ** 2
    return float(max(np.abs(got_alpha - ref_alpha).max(), np.abs(got_beta - ref_beta).max()) / scale2)


@functools.lru_cache(maxsize=None)
def long_double_run(name, n_vectors, seed, kind, first_id=0, m=HORIZON):
    """α, β of the long-double process (the CSR product: the host test pins it to the dense one)."""
    return lanczos_reference(sparse_long_double(name), start_block(name, n_vectors, seed, kind, first_id), m, LD)[:2]


@functools.lru_cache(maxsize=None)
def reference_distance(name, dense=False):
    """What separates the float64 restatement from the long-double one over the first HORIZON iterations: four seeds,
    Rademacher and Z4 start vectors, relative to ‖H‖².  The GPU tests allow the device 20 times this.  `dense`: the
    long-double side on the dense np.clongdouble matrix (what the host test pins) instead of the CSR product."""
    start = np.concatenate([start_block(name, 1, seed, kind) for seed in range(4)
                            for kind in (cheb_ref.VEC_RADEMACHER, cheb_ref.VEC_Z4)], axis=1)
    a64, b64, _ = lanczos_reference(sparse_matrix(name), start, HORIZON)
    ald, bld, _ = lanczos_reference(dense_long_double(name) if dense else sparse_long_double(name), start, HORIZON, LD)
    return trajectory_distance(name, a64, b64, ald, bld)


def local_figures(name, alpha, beta, vectors):
    """The relations every single iteration obeys, evaluated in long double on float64 vectors (n_iter + 1 of them,
    (j, n, C)) with float64 α, β (n_iter, C):
        residual  max_j ‖H² v_j − β_j v_{j−1} − α_j v_j − β_{j+1} v_{j+1}‖ / ‖H‖²   (j < n_iter)
        norm      max_j |‖v_j‖ − 1|
        overlap   max_j |v_j · v_{j+1}|
        alpha     max_j |α_j − ‖H v_j‖²| / ‖H‖²
    They hold over any horizon: no trajectory is compared."""
    matrix = sparse_long_double(name)
    scale2 = LD(norm_bound(name)) ** 2
    v = np.asarray(vectors, dtype=CLD)
    a, b = np.asarray(alpha, dtype=LD), np.asarray(beta, dtype=LD)
    m = a.shape[0]
    hv = np.moveaxis(matrix @ np.moveaxis(v[:m], 1, 0), 0, 1)  # (the product acts on the leading axis)
    h2v = np.moveaxis(matrix @ np.moveaxis(hv, 1, 0), 0, 1)
    w = h2v - a[:, None, :] * v[:m] - b[:, None, :] * v[1:m + 1]
    w[1:] -= b[:-1, None, :] * v[:m - 1]
    return dict(
        residual=float(np.sqrt(np.sum(np.abs(w) ** 2, axis=1)).max() / scale2),
        norm=float(np.abs(np.sqrt(np.sum(np.abs(v) ** 2, axis=1)) - 1).max()),
        overlap=float(np.abs(np.sum(v[:-1].conj() * v[1:], axis=1)).max()),
        alpha=float(np.abs(np.sum(np.abs(hv) ** 2, axis=1) - a).max() / scale2),
    )


@functools.lru_cache(maxsize=None)
def reference_local_figures(name, n_vectors, seed, kind, m=LOCAL_HORIZON):
    """`local_figures` of the float64 restatement's own vectors."""
    alpha, beta, vectors = lanczos_reference(sparse_matrix(name), start_block(name, n_vectors, seed, kind), m)
    return local_figures(name, alpha, beta, vectors)


# ------------------------------------------------------------------ the two-pass front end on the references
TWO_PASS_MAX_ITER = 3000  # (the CPU runs below converge k = 3 levels within 1000 iterations for every vector count used)


class RecordingSolver(NumpyLanczosSolver):
    """Keeps what `lowest_eigenpairs` hands to the second pass."""

    recorded = None

    def lanczos_begin(self, n_vectors, seed=0, first_id=0, kind=cheb_ref.VEC_RADEMACHER, max_iter=10000):
        self.begin_arguments = dict(n_vectors=n_vectors, seed=seed, first_id=first_id, kind=kind, max_iter=max_iter)
        super().lanczos_begin(n_vectors, seed, first_id, kind, max_iter)

    def lanczos_ritz_pairs(self, coef, eps, k, rank_tol=1e-4):
        self.recorded = (np.array(coef, dtype=np.float64), np.array(eps, dtype=np.float64))
        return super().lanczos_ritz_pairs(coef, eps, k, rank_tol)


def two_pass(system, solver, vectors, k=3, seed=0):
    """The public two-pass logic, `lowest_eigenpairs(k, vectors=vectors, method="lanczos")` at its default tol, on a
    system whose solver the calling test has replaced (with monkeypatch) by `solver`, a `RecordingSolver`: returns
    (coef (n_iter, levels, vectors), eps (levels,), begin arguments).  A warning of the front end (levels not
    converged) is an error here: the case would be checking something else."""
    import warnings

    from bodge_amd import observables

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        observables.lowest_eigenpairs(system, k, vectors=vectors, seed=seed, max_iter=TWO_PASS_MAX_ITER,
                                      method="lanczos", format="raw")
    coef, eps = solver.recorded
    return coef, eps, dict(solver.begin_arguments)


def levels_of(name, k, same=1e-7):
    """The k lowest distinct positive eigenvalues from the dense spectrum with their multiplicities and the
    projectors onto their eigenspaces: [(value, multiplicity, P (4N, 4N))]."""
    values, states = dense_eigh(name)
    positive = np.flatnonzero(values > 0)
    out, i = [], 0
    while len(out) < k:
        members = [p for p in positive[i:] if values[p] - values[positive[i]] <= same]
        block = states[:, members]
        out.append((float(values[members].mean()), len(members), block @ block.conj().T))
        i += len(members)
    return out


def states_per_level(values, levels, same=1e-7):
    return [int(np.sum(np.abs(np.asarray(values) - value) <= same)) for value, _, _ in levels]
