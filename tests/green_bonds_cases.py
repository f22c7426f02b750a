"""Shared by tests/test_green_bonds_host.py and tests/test_gpu_green_bonds.py: the models, the pattern of a call, a numpy
restatement of bdg_green_bond_blocks on sparse H (unit columns in batches, one recurrence, the rows of the pattern
blocks picked, the hole-column rule, the weights in ascending n) and the dense reference V (z - E)^-1 V† cut to the
pattern.  The restatements are computed once per (model, columns) and handed out read-only."""

import functools

import numpy as np
import scipy.sparse as sp

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import green as gr
from bodge_amd.observables import _scale_of

import systems

GAMMA = 0.1
ENERGIES = np.array([-0.45, 0.0, 0.3, 1.1])  # both signs, the gap centre, one energy in the band of every model


# ------------------------------------------------------------------ models
def dwave_open(shape=(6, 5, 1), mu=1.0, gap=0.3):
    """The d-wave pattern of systems.dwave_cube in the plane, open edges: H has rows of 3, 4 and 5 blocks (bonds are
    missing at the rim), the skeleton keeps the zero wrap-around blocks - the pattern asks for G between opposite
    faces, where H has no block.  The pairing sits on the bonds alone."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    d = ba.dwave()
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = mu * ba.σ0
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
            Δ[i, j] = -gap * d(i, j)
    return system


def peierls_disordered(shape=(5, 5, 1), phase=0.3, seed=21):
    """systems.peierls_square with a different on-site matrix on every site: complex (no real form), every diagonal
    block distinct."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    rng = np.random.default_rng(seed)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = (1.0 + 0.4 * rng.random()) * ba.σ0 - 0.3 * rng.random() * ba.σ3
            Δ[i, i] = -(0.2 + 0.2 * rng.random()) * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -np.exp(1j * phase * (j[0] - i[0])) * ba.σ0
    return system


def cube(shape=(3, 3, 3), mu=1.0, gap=0.3, zeeman=0.2):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = mu * ba.σ0 - zeeman * ba.σ3
            Δ[i, i] = -gap * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
    return system


SYSTEMS = {
    "swave": lambda: systems.swave_square(ba, L=6, gap=0.3, mu=1.0),  # 36 sites: two batches at two columns
    "dwave_open": dwave_open,                                        # bond pairing, open edges
    "periodic": lambda: systems.random_periodic(ba, shape=(5, 4, 1)),  # wrap-around pairs carry blocks of H
    "peierls": peierls_disordered,                                   # complex, disordered
    "cube": lambda: cube(),                                          # 3 x 3 x 3: rows of 7 blocks
    "single": lambda: cube((1, 1, 1)),                               # one site: the pattern is its diagonal block
}
IS_REAL = {"swave": True, "dwave_open": True, "periodic": False, "peierls": False, "cube": True, "single": True}
IS_PH = {name: True for name in SYSTEMS}  # every block of a Hamiltonian has the Nambu form: packed storage applies
# H = -τx H* τx as a whole (has_symmetric_spectrum): the hole columns follow from the electron columns.  Not so for
# random_periodic, whose pairing blocks are set on one side of a bond only.
DERIVES = {name: name != "periodic" for name in SYSTEMS}


@functools.lru_cache(maxsize=None)
def system_of(name):
    """The system for host-side use (matrices, references): built once, never modified."""
    return SYSTEMS[name]()


def scale_of(system):
    return _scale_of(system)


def moments_of(system, gamma=GAMMA):
    """The default number of moments of the public API at this broadening."""
    return cheb.moments_for_resolvent(scale_of(system), gamma, 12.0)


# ------------------------------------------------------------------ patterns
def pattern_of(system, columns=None):
    """(indptr, indices) int32 of the skeleton blocks of H whose column site is in `columns` (default: all)."""
    n = system.lattice.size
    indptr = np.asarray(system._matrix.indptr, dtype=np.int64)
    indices = np.asarray(system._matrix.indices, dtype=np.int64)
    if columns is None:
        return indptr.astype(np.int32), indices.astype(np.int32)
    wanted = np.zeros(n, dtype=bool)
    wanted[np.asarray(columns, dtype=np.int64)] = True
    rows = np.repeat(np.arange(n), np.diff(indptr))
    keep = wanted[indices]
    out = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=out[1:])
    return out, indices[keep].astype(np.int32)


def block_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def shared_blocks(indptr_a, indices_a, indptr_b, indices_b):
    """Positions (in a, in b) of the blocks the two patterns share."""
    n = len(indptr_a) - 1
    keys_a = block_rows(indptr_a) * n + indices_a
    keys_b = block_rows(indptr_b) * n + indices_b
    common, in_a, in_b = np.intersect1d(keys_a, keys_b, return_indices=True)
    return in_a, in_b


# ------------------------------------------------------------------ the restatement
def bond_moments(h, indptr, indices, moments, scale, columns=4, batch=None):
    """bdg_green_bond_blocks up to the contraction, in numpy on the sparse matrix h: the column sites are the distinct
    entries of `indices`, ascending, in batches of `batch` (default 64 / columns); in a batch vector v = columns * s + b
    starts at e_{4 i_s + b}, all vectors run one recurrence, and of every t_n the four rows of block row j are picked
    from the vectors of site i for every pattern block (j, i) of the batch: (M, nnz, 4, columns)."""
    h = sp.csr_matrix(h)
    indices = np.asarray(indices, dtype=np.int64)
    rows = block_rows(indptr)
    sites = np.unique(indices)
    position = np.full(h.shape[0] // 4, -1, dtype=np.int64)
    position[sites] = np.arange(sites.size)
    batch = batch or max(1, 64 // columns)
    mu = np.empty((moments, indices.size, 4, columns), dtype=np.complex128)
    for s0 in range(0, sites.size, batch):
        own = sites[s0 : s0 + batch]
        width = own.size * columns
        start = (4 * own[:, None] + np.arange(columns)[None, :]).reshape(-1)
        mine = np.flatnonzero((position[indices] >= s0) & (position[indices] < s0 + own.size))
        slot = position[indices[mine]] - s0
        pick_rows = 4 * rows[mine][:, None, None] + np.arange(4)[None, :, None]          # [k, a, .]
        pick_cols = columns * slot[:, None, None] + np.arange(columns)[None, None, :]   # [k, ., b]
        prev = np.zeros((h.shape[0], width), dtype=np.complex128)
        cur = prev.copy()
        cur[start, np.arange(width)] = 1.0
        for n in range(moments):
            mu[n, mine] = cur[pick_rows, pick_cols]
            cur, prev = (1.0 if n == 0 else 2.0) * (h @ cur) / scale - prev, cur
    return mu


def contract(mu, weights):
    """(nnz, K, 4, 4) Σ_n w[e, n] μ_n in ascending n from the moments (M, nnz, 4, 4) and the weights (K, M)."""
    out = np.zeros((mu.shape[1], weights.shape[0], 4, 4), dtype=np.complex128)
    for n in range(mu.shape[0]):
        out += weights[None, :, n, None, None] * mu[n][:, None]
    return out


def restate(system, indptr, indices, z, moments, columns=4, batch=None):
    """The blocks G(z_e) on the pattern as the device computes them: (nnz, K, 4, 4).  columns = 2 derives the hole
    columns block by block (green.hole_columns)."""
    scale = scale_of(system)
    h = sp.csr_matrix(system.matrix("csr"))
    mu = bond_moments(h, indptr, indices, moments, scale, columns, batch)
    if columns == 2:
        mu = gr.hole_columns(mu)
    return contract(mu, gr.moment_weights(moments, scale, z))


def dense_blocks(system, indptr, indices, z):
    """V (z - E)^-1 V† from numpy.linalg.eigh, cut to the pattern: (nnz, K, 4, 4)."""
    n = system.lattice.size
    w, v = np.linalg.eigh(np.asarray(system.matrix("dense")))
    rows = block_rows(indptr)
    out = np.empty((len(indices), len(z), 4, 4), dtype=np.complex128)
    for e, ze in enumerate(z):
        g = (v / (ze - w)[None, :]) @ v.conj().T
        out[:, e] = g.reshape(n, 4, n, 4)[rows, :, np.asarray(indices, dtype=np.int64), :]
    return out


def distance(got, exact):
    """max |got - exact| relative to the largest entry of `exact`."""
    return float(np.abs(got - exact).max() / np.abs(exact).max())


Z = ENERGIES + 1j * GAMMA


@functools.lru_cache(maxsize=None)
def restated(name, columns=4):
    """restate() of the whole skeleton at Z with the default moments: read-only."""
    system = system_of(name)
    out = restate(system, *pattern_of(system), Z, moments_of(system), columns)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dense(name):
    system = system_of(name)
    out = dense_blocks(system, *pattern_of(system), Z)
    out.setflags(write=False)
    return out


# Distance of restated(name, 4) from dense(name), as measured on the CPU (test_green_bonds_host.py prints them): the
# truncation of the series at the default moments (digits = 12) and the rounding of the recurrence.  The yardstick of
# the device tolerance: 20 times the model's figure.
RESTATEMENT_ERROR = {"swave": 5.49e-13, "dwave_open": 7.00e-13, "periodic": 7.18e-13, "peierls": 5.68e-13, "cube": 9.73e-13,
                     "single": 2.32e-13}


def rounding_bound(moments, reference):
    """32·M·2⁻⁵³·max(1, max|reference|): the bound of DESIGN.md §10 (32 roundings per entry and step)."""
    return 32 * moments * 2.0**-53 * max(1.0, float(np.abs(reference).max()))
