"""Local one-body density matrix F = f(H) on the Hamiltonian's block pattern (`Hamiltonian.fermi_matrix`).

f(ε) = 1/(1 + e^{ε/T}) applied to the whole 4N x 4N BdG matrix, Nambu basis (e↑, e↓, h↑, h↓) per site.
`FermiMatrix.blocks[k]` = f(H)[4j:4j+4, 4i:4i+4] for block k = (block row j, block column i) of the
Hamiltonian's block skeleton - the diagonal, every bond and every periodic-edge pair, zero blocks of H
included (`system.matrix("bsr")` drops those; where H has no all-zero block the two patterns agree).
The helpers are slices of these blocks, so no sign convention is hidden in them.

Two routes:

* "dense": the device eigensolver (`DeviceSolver.eigh`), F = V f(E) V^†, cut to the pattern.  Small
  matrices, and T = 0 (f(0) = ½ on zero modes).
* "chebyshev": probe vectors and Clenshaw's recurrence on the GPU (`bdg_fermi_blocks`).
  The sites are coloured so that two sites of one colour are at least `distance` apart in the graph of
  H; one probe per (colour, Nambu component) gives a column of every pattern block of that colour.
  distance=None is one site per colour: exact up to the truncation of the series (`digits`).  With a
  finite distance the blocks pick up the contribution of same-colour sites at least distance-1 away,
  which decays like exp(-r·πT/a) in a metal and faster in a gapped phase (error model: DESIGN.md §10).
"""

from __future__ import annotations

import numpy as np

from .common import Coord
from .lattice import CubicLattice

DENSE_AUTO_LIMIT = 2048  # method="auto": 4N up to which the dense route is taken (that of free_energy)


# ---------------------------------------------------------------- colouring
def _smallest_divisor_at_least(length: int, d: int) -> int:
    for p in range(d, length + 1):
        if length % p == 0:
            return p
    return length


def colour_periods(shape, distance: int | None) -> tuple[int, int, int]:
    """Per-axis colour period of a cubic lattice: the extent itself (one colour per coordinate) when
    `distance` is None or reaches the extent, else the smallest divisor of the extent that is >= distance.

    The block skeleton holds the wrap-around pair of every axis of extent >= 3, zero or not, and those
    blocks are part of the result.  With a period that divides the extent, two sites of one colour are
    at least `distance` apart in the periodic graph as well, which contains H's graph; a period that
    did not divide it would put sites of one colour next to each other across the wrap (open axes
    included, through the zero wrap-around blocks of the pattern)."""
    periods = []
    for length in shape:
        length = int(length)
        if distance is None or distance >= length:
            periods.append(length)
        else:
            periods.append(_smallest_divisor_at_least(length, int(distance)))
    return tuple(periods)


def cubic_colours(shape, periods) -> tuple[np.ndarray, int]:
    """colour = (x mod dx) + dx·((y mod dy) + dy·(z mod dz)) for every site in index order."""
    Lx, Ly, Lz = (int(v) for v in shape)
    dx, dy, dz = (int(v) for v in periods)
    x, y, z = np.meshgrid(np.arange(Lx), np.arange(Ly), np.arange(Lz), indexing="ij")
    colour = (x % dx) + dx * ((y % dy) + dy * (z % dz))
    return colour.reshape(-1).astype(np.int32), dx * dy * dz


def graph_colours(indptr: np.ndarray, indices: np.ndarray, distance: int) -> tuple[np.ndarray, int]:
    """Greedy colouring of any block graph: two sites of one colour are at least `distance` hops apart."""
    import scipy.sparse as sp

    n = len(indptr) - 1
    step = sp.csr_matrix((np.ones(len(indices), dtype=np.int8), indices, indptr), shape=(n, n))
    step = ((step + step.T + sp.identity(n, dtype=np.int8, format="csr")) > 0).astype(np.int8)
    reach = sp.identity(n, dtype=np.int8, format="csr")
    for _ in range(distance - 1):
        reach = ((reach @ step) > 0).astype(np.int8)
    reach = reach.tocsr()
    colour = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        used = set(colour[reach.indices[reach.indptr[i]:reach.indptr[i + 1]]].tolist())
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    return colour, int(colour.max(initial=-1)) + 1


def site_colours(system, distance: int | None) -> tuple[np.ndarray, int]:
    """(colour per site, number of colours) for probing at `distance` (None: one site per colour)."""
    n = system.lattice.size
    if distance is not None:
        distance = int(distance)
        if distance < 3:
            raise ValueError("fermi_matrix: distance must be >= 3 (or None for the exact result)")
    if isinstance(system.lattice, CubicLattice):
        periods = colour_periods(system.lattice.shape, distance)
        return cubic_colours(system.lattice.shape, periods)
    if distance is None or distance > n:
        return np.arange(n, dtype=np.int32), n
    indptr, indices, _ = system.bsr_arrays()
    return graph_colours(indptr, indices, distance)


# ---------------------------------------------------------------- the result
class FermiMatrix:
    """Blocks of f(H) on the Hamiltonian's block skeleton, with the usual contractions.

    `blocks` (nnzb, 4, 4) complex128, `indptr` / `indices` the pattern (int32), `lattice` the system's.
    """

    def __init__(self, lattice, indptr: np.ndarray, indices: np.ndarray, blocks: np.ndarray, temperature: float,
                 method: str, info: dict | None = None):
        self.lattice = lattice
        self.indptr = indptr
        self.indices = indices
        self.blocks = blocks
        self.temperature = float(temperature)
        self.method = method
        self.info = dict(info or {})  # route details: moments, distance, colours, perf record of the call
        n = lattice.size
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        self._keys = rows * n + indices
        self._diag = self._find(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))
        self._mirror = None

    def _find(self, rows: np.ndarray, cols: np.ndarray) -> np.ndarray:
        wanted = rows * self.lattice.size + cols
        found = np.minimum(np.searchsorted(self._keys, wanted), len(self._keys) - 1)
        if np.any(self._keys[found] != wanted):
            raise IndexError("The pattern has no block for this pair of sites")
        return found

    def block(self, i: Coord, j: Coord) -> np.ndarray:
        """f(H)[4i:4i+4, 4j:4j+4] for lattice coordinates i, j (a copy)."""
        k = self._find(np.array([self.lattice[i]], dtype=np.int64), np.array([self.lattice[j]], dtype=np.int64))[0]
        return self.blocks[k].copy()

    def density(self) -> np.ndarray:
        """(N,) n_i = Re(F_ii[0,0] + F_ii[1,1])."""
        d = self.blocks[self._diag]
        return (d[:, 0, 0] + d[:, 1, 1]).real.copy()

    def magnetization(self) -> np.ndarray:
        """(N, 3) m_i^k = Re tr(σ_k F_ii[0:2, 0:2])."""
        from .common import σ1, σ2, σ3

        d = self.blocks[self._diag][:, 0:2, 0:2]
        return np.stack([np.einsum("ab,nba->n", s, d).real for s in (σ1, σ2, σ3)], axis=1)

    def pair_amplitude(self) -> np.ndarray:
        """(N,) complex F_ii[0, 3]."""
        return self.blocks[self._diag][:, 0, 3].copy()

    def pairing(self, i: Coord, j: Coord) -> np.ndarray:
        """The 2x2 electron-hole block F_ij[0:2, 2:4]."""
        return self.block(i, j)[0:2, 2:4]

    def expectation(self, dH) -> complex:
        """½ Σ_{(i,j) in pattern} tr(F_ji dH_ij) for a block array dH (nnzb, 4, 4) on this pattern, or a
        Hamiltonian on the same lattice (its blocks).  Equals dF/dλ for H(λ) linear in λ with ∂H/∂λ = dH
        particle-hole symmetric; real up to round-off for Hermitian dH."""
        data = getattr(dH, "_data", dH)
        data = np.asarray(data)
        if data.shape != self.blocks.shape:
            raise ValueError(f"expected blocks of shape {self.blocks.shape} on the same pattern, got {data.shape}")
        if self._mirror is None:
            n = self.lattice.size
            rows = self._keys // n
            self._mirror = self._find(self._keys - rows * n, rows)
        return complex(0.5 * np.einsum("kab,kba->", self.blocks[self._mirror], data))


# ---------------------------------------------------------------- the routes
def _dense_blocks(system, temperature: float, indptr, indices) -> np.ndarray:
    n = system.lattice.size
    w, v = system._solver().eigh(vectors=True)
    if temperature > 0:
        from .chebyshev import fermi_function

        occupation = fermi_function(w, temperature)
    else:
        # T = 0: f = 1 below zero, 0 above, ½ on zero modes (|E| within round-off of the solver)
        zero = np.abs(w) <= 1e-12 * max(1.0, float(np.abs(w).max(initial=0.0)))
        occupation = np.where(zero, 0.5, np.where(w < 0, 1.0, 0.0))
    full = (v * occupation[None, :]) @ v.conj().T
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    return np.ascontiguousarray(full.reshape(n, 4, n, 4)[rows, :, indices.astype(np.int64), :])


def _particle_hole_columns(blocks: np.ndarray, diag: np.ndarray) -> None:
    """Columns b = 2, 3 from b = 0, 1 in place: F = 1 - C F* C with C = τx, i.e.
    F[a, b] = δ_ij δ_ab - conj(F[a ^ 2, b ^ 2]) on the same block (j, i)."""
    for b in (2, 3):
        for a in range(4):
            blocks[:, a, b] = -blocks[:, a ^ 2, b ^ 2].conj()
    blocks[diag, 2, 2] += 1.0
    blocks[diag, 3, 3] += 1.0


def fermi_matrix(system, temperature: float, *, method: str = "auto", moments: int | None = None,
                 digits: float = 12, distance: int | None = None, devices=None, scale: float | None = None,
                 _all_columns: bool = False) -> FermiMatrix:
    """f(H) on the block pattern of `system` at temperature T (see `Hamiltonian.fermi_matrix`)."""
    if temperature < 0:
        raise ValueError("Expected non-negative temperature!")
    if method not in ("auto", "chebyshev", "dense"):
        raise ValueError(f"fermi_matrix: unknown method '{method}' (auto, chebyshev or dense)")
    if distance is not None and int(distance) < 3:
        raise ValueError("fermi_matrix: distance must be >= 3 (or None for the exact result)")
    if method == "auto":
        method = "dense" if temperature == 0 or system.shape[0] <= DENSE_AUTO_LIMIT else "chebyshev"
    if method == "chebyshev" and temperature <= 0:
        raise ValueError("fermi_matrix: the Chebyshev route needs T > 0 (method='dense' takes T = 0)")
    indptr = system._matrix.indptr.astype(np.int32, copy=True)
    indices = system._matrix.indices.astype(np.int32, copy=True)
    lattice = system.lattice

    if method == "dense":
        blocks = _dense_blocks(system, temperature, indptr, indices)
        return FermiMatrix(lattice, indptr, indices, blocks, temperature, "dense")

    from . import chebyshev as cheb
    from .observables import _scale_of

    scale = _scale_of(system) if scale is None else float(scale)
    if moments is None:
        moments = cheb.moments_for_fermi(scale, temperature, digits)
    coef = cheb.chebyshev_coefficients(lambda x: cheb.fermi_function(scale * x, temperature), int(moments))
    colours, n_colours = site_colours(system, distance)
    # particle-hole symmetry (H = -τx H* τx block by block) gives the hole columns from the electron columns
    halve = not _all_columns and system.has_symmetric_spectrum(1e-12)
    components = 2 if halve else 4
    if devices is None:
        solver = system._solver()
        blocks = solver.fermi_blocks(scale, coef, colours, n_colours, components, indptr, indices)
        perf = solver.perf()
    else:
        blocks, perf = _fermi_blocks_devices(system, scale, coef, colours, n_colours, components, indptr, indices,
                                             [int(d) for d in devices])
    if halve:
        rows = np.repeat(np.arange(lattice.size, dtype=np.int64), np.diff(indptr))
        _particle_hole_columns(blocks, np.flatnonzero(rows == indices))
    info = {"moments": int(moments), "scale": scale, "distance": distance, "colours": n_colours,
            "components": components, "perf": perf}
    return FermiMatrix(lattice, indptr, indices, blocks, temperature, "chebyshev", info)


def _fermi_blocks_devices(system, scale, coef, colours, n_colours, components, indptr, indices, devices):
    """The colours shared out over GPUs of this process (contiguous ranges, one host thread per device): every
    device probes its own colours only (the others are marked -1) and fills its blocks; the results add up."""
    from concurrent.futures import ThreadPoolExecutor

    if not devices:
        raise ValueError("fermi_matrix: devices=[] names no GPU")
    parts = min(len(devices), n_colours)
    bounds = [n_colours * p // parts for p in range(parts + 1)]
    mirrors = [system._solver(lane=p, device=devices[p]) for p in range(parts)]

    def run(p):
        lo, hi = bounds[p], bounds[p + 1]
        mine = np.where((colours >= lo) & (colours < hi), colours - lo, -1).astype(np.int32)
        blocks = mirrors[p].fermi_blocks(scale, coef, mine, hi - lo, components, indptr, indices)
        return blocks, mirrors[p].perf()

    with ThreadPoolExecutor(max_workers=parts) as pool:
        results = list(pool.map(run, range(parts)))
    total = results[0][0]
    for blocks, _ in results[1:]:
        total += blocks
    return total, [perf for _, perf in results]
