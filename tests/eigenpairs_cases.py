"""Shared by tests/test_eigenpairs_host.py and tests/test_gpu_eigenpairs.py: the systems and their windows, the
library's start vectors in numpy, the numpy restatement of the filtered subspace iteration of
bodge_amd/eigenpairs.py on a sparse H, and numpy.linalg.eigh of the dense matrix as reference."""

import functools

import numpy as np

import bodge_amd as ba
from bodge_amd import chebyshev as cheb

import apply_cases

TOL = 1e-9
MOMENTS = 256


# ------------------------------------------------------------------ systems
def swave_with_moments(shape, n_magnetic, onsite, seed, periodic=False, coupling=2.0):
    """t = 1, μ = 0.5, Δ = 0.5 jσ2 on every site; `n_magnetic` random sites carry -J u `onsite`, u uniform in
    [0.6, 1.4] (σ3 keeps the matrix real, σ2 makes it complex); `periodic` sets the wrap-around edges."""
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    rng = np.random.default_rng(seed)
    sites = list(lattice.sites())
    chosen = rng.choice(len(sites), size=n_magnetic, replace=False) if n_magnetic else []
    strength = {sites[int(c)]: coupling * (0.6 + 0.8 * rng.random()) for c in chosen}
    with system as (H, Δ):
        for i in sites:
            H[i, i] = -0.5 * ba.σ0 - strength.get(i, 0.0) * onsite
            Δ[i, i] = 0.5 * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
        if periodic:
            for i, j in lattice.edges():
                if i != j:
                    H[i, j] = -1.0 * ba.σ0
    return system


# name -> (builder, target of the lower edge (None: exactly 0), target of the upper edge)
SYSTEMS = {
    "ysr_real": (lambda: swave_with_moments((12, 10, 1), 6, ba.σ3, seed=7), None, 0.55),
    "ysr_complex": (lambda: swave_with_moments((12, 10, 1), 6, ba.σ2, seed=2), None, 0.53),
    "cube": (lambda: swave_with_moments((5, 4, 3), 4, ba.σ3, seed=4), None, 0.41),
    "periodic_degenerate": (lambda: swave_with_moments((8, 8, 1), 0, ba.σ3, seed=0, periodic=True), 0.88, 1.78),
}


def scale_of(system):
    return 1.01 * system.gershgorin_bound()


def gap_edge(levels, target, reach=0.06):
    """Midpoint of the widest spacing between neighbouring levels whose midpoint lies within `reach` of `target`:
    a window edge that sits in a real gap."""
    mid = 0.5 * (levels[1:] + levels[:-1])
    near = np.flatnonzero(np.abs(mid - target) <= reach)
    best = near[np.argmax(np.diff(levels)[near])]
    return float(mid[best])


class Case:
    """One system with its dense spectrum, its window and what lies inside."""

    def __init__(self, name):
        build, lo_target, hi_target = SYSTEMS[name]
        self.name = name
        self.system = build()
        self.dense = np.asarray(self.system.matrix("dense"))
        self.h = self.system.matrix("csr")
        self.scale = scale_of(self.system)
        self.levels, self.states = np.linalg.eigh(self.dense)
        self.lo = 0.0 if lo_target is None else gap_edge(self.levels, lo_target)
        self.hi = gap_edge(self.levels, hi_target)
        self.inside = np.flatnonzero((self.levels >= self.lo) & (self.levels <= self.hi))
        self.energies = self.levels[self.inside]
        self.count = len(self.inside)
        edges = [self.hi] if lo_target is None else [self.lo, self.hi]
        self.edge_gap = min(float(np.abs(self.levels - edge).min()) for edge in edges)

    def clusters(self, resolution=1e-8):
        """Index ranges of the levels in the window that agree to `resolution`: the degenerate clusters."""
        cuts = np.flatnonzero(np.diff(self.energies) > resolution) + 1
        return [np.arange(a, b) for a, b in zip(np.r_[0, cuts], np.r_[cuts, self.count])]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ------------------------------------------------------------------ the library's start vectors
def _splitmix64(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def start_vector(dim, seed, vec_id):
    """Rademacher start vector (seed, vec_id) of the library (kernels.hpp start_entry): one hash per site, bit
    63 - component of it decides the sign of entry 4 site + component."""
    mask = (1 << 64) - 1
    inner = _splitmix64(np.array([vec_id & mask], dtype=np.uint64))[0]
    key = _splitmix64(np.array([(seed & mask) ^ int(inner)], dtype=np.uint64))[0]
    rows = np.arange(dim, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _splitmix64(key + (rows >> np.uint64(2)))
    return np.where((h >> (np.uint64(63) - (rows & np.uint64(3)))) & np.uint64(1) == 0, 1.0, -1.0).astype(np.complex128)


def start_block(dim, seed, first_id, count):
    return np.stack([start_vector(dim, seed, first_id + c) for c in range(count)])


# ------------------------------------------------------------------ restatement
def window_series(scale, lo, hi, moments):
    """c_0 = (θ_lo − θ_hi)/π, c_k = 2 (sin kθ_lo − sin kθ_hi)/(kπ), θ = arccos(E/scale), times the Jackson kernel."""
    t_lo, t_hi = np.arccos(np.clip(lo / scale, -1, 1)), np.arccos(np.clip(hi / scale, -1, 1))
    k = np.arange(1, moments)
    coef = np.r_[(t_lo - t_hi) / np.pi, 2 * (np.sin(k * t_lo) - np.sin(k * t_hi)) / (k * np.pi)]
    return coef * cheb.jackson_kernel(moments)


def whiten_and_diagonalise(s, g, cut=1e-12):
    w, u = np.linalg.eigh(0.5 * (s + s.conj().T))
    keep = w > cut * w[-1]
    white = u[:, keep] / np.sqrt(w[keep])
    small = white.conj().T @ g @ white
    theta, z = np.linalg.eigh(0.5 * (small + small.conj().T))
    return theta, white @ z


def filtered_subspace(h, scale, lo, hi, *, moments=MOMENTS, columns, tol=TOL, max_iter=40, seed=0, limit=512):
    """The driver of bodge_amd/eigenpairs.py in numpy.  X holds the block's columns as rows (B, 4N).  Returns
    (E, V (k, 4N), iterations, residuals, columns at the end); unconverged pairs are left out."""
    dim = h.shape[0]
    coef = window_series(scale, lo, hi, moments)[:, None]
    grid = np.clip(np.linspace(lo, hi, 65) / scale, -1, 1)
    kept_from = 0.5 * np.polynomial.chebyshev.chebval(grid, coef[:, 0]).max()  # half the filter's plateau
    x = start_block(dim, seed, 0, columns)
    norm2 = np.full(columns, float(dim))  # |column|² before the filter: 4N for a start vector, 1 for a Ritz vector
    next_id = columns
    settling = True
    for iteration in range(1, max_iter + 1):
        x = apply_cases.stored_source_clenshaw(h, scale, coef, x)[:, 0]
        hx = (h @ x.T).T
        theta, q = whiten_and_diagonalise(x.conj() @ x.T, x.conj() @ hx.T)
        x, hx = q.T @ x, q.T @ hx
        residual = np.linalg.norm(hx - theta[:, None] * x, axis=1)
        gain = 1.0 / np.sqrt((np.abs(q) ** 2 * norm2[:, None]).sum(axis=0))  # what the filter left of each Ritz vector
        rank = len(theta)
        norm2 = np.r_[np.ones(rank), np.full(columns - rank, float(dim))]
        if rank < columns:
            x = np.vstack([x, start_block(dim, seed, next_id, columns - rank)])
            next_id += columns - rank
        inside = (theta >= lo) & (theta <= hi)
        done = inside & (residual <= tol * scale)
        genuine = done | (inside & (gain >= kept_from))
        if settling:  # (the first iteration and the one after the block grew: start vectors, no gains to speak of)
            settling = False
            continue
        guarded = (~genuine).any() or (rank < columns <= dim)  # (a direction the filter annihilated was a guard too)
        if not guarded:
            if 2 * columns > limit:
                raise ValueError(f"more states than {limit} columns hold")
            columns *= 2
            grown = start_block(dim, seed, next_id, columns)
            next_id += columns
            grown[:rank] = x[:rank]
            x = grown
            norm2 = np.r_[np.ones(rank), np.full(columns - rank, float(dim))]
            settling = True
            continue
        if (done | ~genuine).all():
            break
    return theta[done], x[: len(theta)][done], iteration, residual[done], columns


# Iterations of the restatement at M = 256, tol = 1e-9, B = ⌈1.25 count⌉ + 8, seed 0, as measured
ITERATIONS = {"ysr_real": 19, "ysr_complex": 24, "cube": 7, "periodic_degenerate": 4}


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement on a case with B = ⌈1.25 count⌉ + 8 columns and twice the measured iterations as cap,
    computed once per session."""
    c = case(name)
    return filtered_subspace(c.h, c.scale, c.lo, c.hi, columns=int(np.ceil(1.25 * c.count)) + 8,
                             max_iter=2 * ITERATIONS[name])


# ------------------------------------------------------------------ figures of merit
def orthonormality(v):
    """max |V V† − 1| for states as rows."""
    return float(np.abs(v.conj() @ v.T - np.eye(len(v))).max()) if len(v) else 0.0


def subspace_deviation(c, v):
    """max over the degenerate clusters of the window of ‖P_ref − P‖₂, P the projector on the cluster's states."""
    worst = 0.0
    for members in c.clusters():
        ref = c.states[:, c.inside[members]]
        got = v[members].T
        worst = max(worst, float(np.linalg.norm(ref @ ref.conj().T - got @ got.conj().T, 2)))
    return worst
