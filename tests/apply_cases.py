"""Shared by tests/test_apply_host.py and tests/test_gpu_apply.py: the systems, the numpy restatement of the
stored-source Clenshaw recurrence of bdg_apply_series, and the dense eigh oracle."""

import numpy as np

import bodge_amd as ba
from bodge_amd import chebyshev as cheb


# ------------------------------------------------------------------ systems
def disordered_swave(shape=(9, 8, 1), onsite=None, seed=5):
    """s-wave lattice with a different on-site matrix on every site: `onsite` = σ3 keeps the matrix real, σ2 makes it
    complex.  More distinct blocks than sites of a dictionary: the streamed-block kernels."""
    onsite = ba.σ3 if onsite is None else onsite
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    rng = np.random.default_rng(seed)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -(0.5 + 0.4 * rng.random()) * ba.σ0 + 0.3 * rng.random() * onsite
            Δ[i, i] = (0.2 + 0.2 * rng.random()) * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
    return system


def uniform_swave(shape=(8, 7, 1), mu=0.5, gap=0.3, zeeman=0.2, hop=-1.0):
    """Real, particle-hole packed, a handful of distinct blocks: the dictionary kernels."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        H.set_sites(-mu * ba.σ0 - zeeman * ba.σ3)
        Δ.set_sites(gap * ba.jσ2)
        H.set_bonds(hop * ba.σ0)
    return system


SYSTEMS = {
    "disordered_real": lambda: disordered_swave(),
    "disordered_complex": lambda: disordered_swave(onsite=ba.σ2),
    "disordered_300": lambda: disordered_swave((20, 15, 1), seed=11),
    "dictionary": lambda: uniform_swave(),
    "cube": lambda: uniform_swave((4, 4, 3)),
}


def scale_of(system):
    return 1.01 * system.gershgorin_bound()


def unit_vectors(system, count=3, seed=1):
    """(count, 4N) random complex vectors of norm 1."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((count, 4 * system.lattice.size)) + 1j * rng.standard_normal((count, 4 * system.lattice.size))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ------------------------------------------------------------------ restatement and oracle
def stored_source_clenshaw(h, scale, coef, x):
    """y[v, f] = Σ_k coef[k, f] T_k(h / scale) x[v] as bdg_apply_series sums it: b_M = b_{M+1} = 0,
    b_k = 2 H~ b_{k+1} - b_{k+2} + c_k x (k = M-1 .. 1), y = H~ b_1 - b_2 + c_0 x.  h dense or sparse (4N, 4N),
    coef (M, F), x (V, 4N); returns (V, F, 4N)."""
    coef = np.asarray(coef, dtype=np.complex128)
    x = np.asarray(x, dtype=np.complex128)
    source = np.repeat(x, coef.shape[1], axis=0).T            # (4N, V·F), column v·F + f = x_v
    weights = np.tile(coef, (1, x.shape[0]))                  # (M, V·F), column v·F + f = c[:, f]
    b1 = np.zeros_like(source)
    b2 = np.zeros_like(source)
    for k in range(coef.shape[0] - 1, 0, -1):
        b1, b2 = 2 * (h @ b1) / scale - b2 + weights[k] * source, b1
    y = (h @ b1) / scale - b2 + weights[0] * source
    return np.ascontiguousarray(y.T).reshape(x.shape[0], coef.shape[1], -1)


def dense_function(system, values_of, x):
    """V g(E) V† x by numpy.linalg.eigh: `values_of(E)` returns (4N,) or (F, 4N) values on the spectrum; result
    (V, 4N) or (V, F, 4N)."""
    w, v = np.linalg.eigh(np.asarray(system.matrix("dense")))
    g = np.asarray(values_of(w))
    projected = x @ v.conj()                                   # (V, 4N): <n|x_v>
    if g.ndim == 1:
        return (projected * g) @ v.T
    return np.einsum("vn,fn,mn->vfm", projected, g, v)


def fermi_coefficients(scale, temperature, digits=13.0):
    from bodge_amd.apply import series_coefficients

    return series_coefficients(lambda e: cheb.fermi_function(e, temperature), scale, digits)
