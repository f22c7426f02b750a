"""Shared by tests/test_correlation_host.py and tests/test_gpu_correlation.py: the systems of apply_cases, the numpy
restatement of bdg_moment_matrix (two forward recurrences and one Gram product) and the dense eigh oracle."""

import functools

import numpy as np

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import correlation as corr

from apply_cases import SYSTEMS, scale_of, uniform_swave, unit_vectors  # noqa: F401  (re-exported for the tests)

M_SMALL = 48


# ------------------------------------------------------------------ restatement and oracle
def restated_moment_matrix(h, scale, A, B, M, X):
    """μ[n, m] = Σ_v <x_v|T_n(h/scale) A T_m(h/scale) B|x_v> as bdg_moment_matrix sums it: L_n = T_n x, R_m = A T_m (B x)
    by the forward recurrence t_{n+1} = 2 h t_n / scale - t_{n-1}, then conj(L) @ R.T.  h, A, B sparse (4N, 4N); X (V, 4N)."""
    X = np.asarray(X, dtype=np.complex128).T                  # (4N, V)

    def chain(start, after=None):
        rows, t0, t1 = [], start, None
        for n in range(M):
            if n == 1:
                t1 = (h @ t0) / scale
            elif n > 1:
                t0, t1 = t1, 2 * (h @ t1) / scale - t0
            t = t0 if n == 0 else t1
            rows.append(np.asarray(t if after is None else after @ t).reshape(-1))
        return np.array(rows)                                  # (M, 4N·V)

    left = chain(X)
    right = chain(np.asarray(B @ X), after=A)
    return left.conj() @ right.T


def dense_moment_matrix(system, scale, A, B, M, X=None):
    """The same from numpy.linalg.eigh: Σ_ab T_n(E~_a) A_ab T_m(E~_b) (B P)_ba with P = X†-weighted projector Σ_v |x_v><x_v|
    (X (V, 4N)), or 1 for the trace."""
    w, v = _eigh(system)
    a_eig = v.conj().T @ (A @ v)                               # A_ab
    bp = B.toarray() if hasattr(B, "toarray") else np.asarray(B)
    if X is not None:
        X = np.asarray(X, dtype=np.complex128)
        bp = bp @ (X.T @ X.conj())
    b_eig = v.conj().T @ bp @ v                                # (B P)_ba as [b, a]
    cheb_t = np.cos(np.arange(M)[:, None] * np.arccos(np.clip(w / scale, -1.0, 1.0))[None, :])  # T_n(E~_a): (M, 4N)
    return cheb_t @ (np.asarray(a_eig) * np.asarray(b_eig).T) @ cheb_t.T


_EIGH = {}


def _eigh(system):
    key = id(system)
    if key not in _EIGH:
        _EIGH[key] = (system, *np.linalg.eigh(np.asarray(system.matrix("dense"))))
    return _EIGH[key][1:]


def dense_response(system, A, B, omega, temperature, broadening):
    """½ Σ_ab A_ab B_ba (f(E_a) - f(E_b)) / (ω + iη + E_a - E_b): the double sum over the eigenpairs of eigh."""
    w, v = _eigh(system)
    a_eig = np.asarray(v.conj().T @ (A @ v))
    b_eig = np.asarray(v.conj().T @ (B @ v))
    f = cheb.fermi_function(w, temperature)
    kernel = (f[:, None] - f[None, :]) / (omega + 1j * broadening + w[:, None] - w[None, :])
    return 0.5 * np.sum(a_eig * b_eig.T * kernel)


def dense_static(system, A, B, temperature):
    """The ω = 0, η = 0 limit: divided differences of f off the diagonal, f′ = -f(1 - f)/T on it and on degenerate pairs."""
    w, v = _eigh(system)
    a_eig = np.asarray(v.conj().T @ (A @ v))
    b_eig = np.asarray(v.conj().T @ (B @ v))
    f = cheb.fermi_function(w, temperature)
    gap = w[:, None] - w[None, :]
    same = np.abs(gap) < 1e-9
    derivative = -(f * (1 - f) / temperature)
    kernel = np.where(same, 0.5 * (derivative[:, None] + derivative[None, :]),
                      (f[:, None] - f[None, :]) / np.where(same, 1.0, gap))
    return 0.5 * np.sum(a_eig * b_eig.T * kernel)


# ------------------------------------------------------------------ the cases: systems, operator pairs, references
@functools.lru_cache(maxsize=None)
def system_of(name):
    return SYSTEMS[name]()


def interior_site(system):
    return tuple(int(s) // 2 for s in system.lattice.shape)


def operator_pair(system, pair):
    """"jj": A = B = J_x with the exact trace (X = None); "js": A = J_x, B = S_z on one interior site, on three unit vectors."""
    jx = corr.current_operator(system, 0)
    if pair == "jj":
        return jx, jx, None
    return jx, corr.spin_operator(system, [interior_site(system)], 3), unit_vectors(system)


@functools.lru_cache(maxsize=None)
def references(name, pair, M):
    """(restated, dense, largest |dense entry|, distance of the two) for one case: computed once, shared, not modified."""
    system = system_of(name)
    scale = scale_of(system)
    A, B, X = operator_pair(system, pair)
    start = np.eye(4 * system.lattice.size) if X is None else X
    restated = restated_moment_matrix(system.matrix("csr"), scale, A, B, M, start)
    dense = dense_moment_matrix(system, scale, A, B, M, X)
    restated.setflags(write=False)
    dense.setflags(write=False)
    return restated, dense, float(np.abs(dense).max()), float(np.abs(restated - dense).max())


def peierls_swave(phase, shape=(9, 8, 1), seed=5, axis=0):
    """apply_cases.disordered_swave(onsite=σ2) with the Peierls phase exp(iφ(x_j - x_i)) on its hopping blocks."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    rng = np.random.default_rng(seed)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -(0.5 + 0.4 * rng.random()) * ba.σ0 + 0.3 * rng.random() * ba.σ2
            Δ[i, i] = (0.2 + 0.2 * rng.random()) * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * np.exp(1j * phase * (j[axis] - i[axis])) * ba.σ0
    return system
