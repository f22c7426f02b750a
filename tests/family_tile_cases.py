"""Shared by tests/test_family_tiles_host.py and tests/test_gpu_family_tiles.py: the lattices on which a workgroup of the
Clenshaw-family tile loops (csrc/family.hpp, and fermi.hpp's own dictionary loop) walks several tiles, one caller per
entry point, the tile arithmetic of a launch, and the numpy restatements the device results are held to.

A tile is (64 / lanes) * 4 block rows (fermi_cases.tiles_of) and BODGE_AMD_BLOCKS_PER_CU=n sets the grid to
min(tiles, n * CUs) rounded up to a multiple of 8 (make_family_plan), so on the 256 CUs of an MI355X the 67 x 63 lattice
is 528 tiles for 256 workgroups at 32 lanes: every workgroup walks two or three of them.  Both sides are odd: the last
tile is ragged, and a tile straddles two lattice rows almost everywhere."""

import functools

import numpy as np
import scipy.sparse as sp

import bodge_amd as ba
from bodge_amd import apply as ap

import apply_cases
import fermi_cases
import green_states_cases
from fermi_cases import scale_of, tiles_of  # noqa: F401  (re-exported for the tests)

SHAPE = (67, 63, 1)       # 4221 sites
CUBE_SHAPE = (17, 16, 16)  # 4352 sites, rows of 7 blocks: z-neighbours inside a wave's rows, y and x neighbours gathered
M = 24                    # coefficients / moments of every case
CUS = 256                 # compute units of an MI355X: the grids quoted below (the GPU tests read theirs from perf)
TIMES = np.array([2.0, -0.7])  # apply_series: exp(-iHt) at two times of opposite sign

SYSTEMS = {
    "uniform": lambda: apply_cases.uniform_swave(SHAPE),                       # real, packed, 5 blocks per row: dictionary
    "disordered": lambda: apply_cases.disordered_swave(SHAPE, onsite=ba.σ2),   # complex, 4221 distinct blocks: streamed
    "cube": lambda: apply_cases.uniform_swave(CUBE_SHAPE),                     # 7 blocks per row
}


@functools.lru_cache(maxsize=None)
def system_of(name):
    """The system for host-side use (matrices, references): built once, never modified.  A GPU test builds its own with
    SYSTEMS[name]() after it has set the switches that are read at upload."""
    return SYSTEMS[name]()


@functools.lru_cache(maxsize=None)
def sparse_of(name):
    return sp.csr_matrix(system_of(name).matrix("csr"))


# ------------------------------------------------------------------ the tile arithmetic of a launch
def grid_of(tiles, blocks_per_cu, cus=CUS):
    """make_family_plan's grid under BODGE_AMD_BLOCKS_PER_CU: min(tiles, n * CUs) rounded up to a multiple of 8."""
    return max(8, -(-min(tiles, blocks_per_cu * cus) // 8) * 8)


def tile_shares(tiles, grid):
    """Tiles per workgroup, (grid,) ints, by tile_split: workgroup b serves XCD b & 7, whose tiles are
    [tiles * x // 8, tiles * (x + 1) // 8), and takes every (grid / 8)-th of them from b >> 3 on."""
    shares = np.zeros(grid, dtype=np.int64)
    step = grid // 8
    for b in range(grid):
        xcd = b & 7
        lo, hi = tiles * xcd // 8, tiles * (xcd + 1) // 8
        shares[b] = len(range(lo + (b >> 3), hi, step))
    return shares


def last_tile_rows(n_sites, lanes):
    """Block rows of the last tile (a full one: rows per tile)."""
    rows = (64 // lanes) * 4
    return n_sites - (tiles_of(n_sites, lanes) - 1) * rows


# ------------------------------------------------------------------ one caller per entry point
def fermi_colours(n_sites):
    """33 random colours in 4 components: three batches at 32 lanes in real arithmetic, five in complex."""
    return fermi_cases.random_colours(n_sites, 33), 33


def _fermi_blocks(system, solver):
    colours, n_colours = fermi_colours(system.lattice.size)
    coef = fermi_cases.fermi_coefficients(system, fermi_cases.TEMPERATURE, M)
    return solver.fermi_blocks(scale_of(system), coef, colours, n_colours, 4, *fermi_cases.pattern_of(system))


def apply_coefficients(system):
    """The first M coefficients of exp(-iHt) at TIMES: (M, 2) complex (cut short: a polynomial like any other)."""
    coef = ap.evolution_coefficients(scale_of(system), TIMES, 12.0)
    assert coef.shape[0] >= M
    return np.ascontiguousarray(coef[:M])


def apply_vectors(system, count=35):
    """35 random unit vectors: with two functions 70 columns, several batches at every lane width."""
    return apply_cases.unit_vectors(system, count, seed=6)


def _apply_series(system, solver):
    return solver.apply_series(scale_of(system), apply_coefficients(system), apply_vectors(system))


def green_sources(n_sites):
    """8 source rows: the four of a site in the middle and of site 1."""
    return np.concatenate([4 * j + np.arange(4) for j in (n_sites // 2, 1)]).astype(np.int64)


def green_targets(n_sites):
    """64 target sites in no order: the first, the last eight (the ragged last tile), the sources' own and random ones."""
    fixed = np.concatenate([[0, 1, n_sites // 2], np.arange(n_sites - 8, n_sites)])
    rest = np.setdiff1d(np.arange(n_sites), fixed)
    picked = np.random.default_rng(9).choice(rest, 64 - fixed.size, replace=False)
    return np.random.default_rng(10).permutation(np.concatenate([fixed, picked])).astype(np.int32)


def _green_moments(system, solver):
    n = system.lattice.size
    return solver.green_moments(scale_of(system), M, green_sources(n), green_targets(n))


def local_sites(n_sites):
    """Every site, permuted: 528 batches of 8 sites at 32 lanes in complex arithmetic."""
    return np.random.default_rng(7).permutation(n_sites).astype(np.int32)


def _green_local_moments(system, solver):
    return solver.green_local_moments(scale_of(system), M, local_sites(system.lattice.size), 4)


ENTRY_POINTS = {
    "fermi_blocks": _fermi_blocks,
    "apply_series": _apply_series,
    "green_moments": _green_moments,
    "green_local_moments": _green_local_moments,
}
PERF_FLAG = {"fermi_blocks": "clenshaw", "apply_series": "apply", "green_moments": "green",
             "green_local_moments": "green_local"}


def states_of(system):
    """Six normalised states for bdg_green_state_moments: plane waves at k = 0, (π/2, 0, 0), an allowed k and its -k, a
    Gaussian packet carrying a momentum and a real standing wave: (6, N)."""
    lattice = system.lattice
    k = green_states_cases.allowed_momentum(lattice)
    waves = lattice.plane_waves(np.array([[0.0, 0.0, 0.0], [np.pi / 2, 0.0, 0.0], k, -k]))
    return np.concatenate([waves, [green_states_cases.gaussian_packet(lattice, (0.9, -0.4, 0.0), width=9.0),
                                   green_states_cases.standing_wave(lattice)]])


# ------------------------------------------------------------------ the two Green recurrences in numpy
def _forward(h, scale, moments, start):
    """t_0 = start, t_1 = H~ t_0, t_{n+1} = 2 H~ t_n - t_{n-1} (H~ = h / scale), one after the other.  The vectors have
    h's type: a real h (float64) runs the recurrence of the unit vectors in real numbers, as the device does."""
    cur, prev = start, np.zeros_like(start)
    for n in range(moments):
        yield cur
        cur, prev = (1.0 if n == 0 else 2.0) * (h @ cur) / scale - prev, cur


def picked_moments(h, scale, moments, source_rows, target_sites):
    """bdg_green_moments in numpy: the unit vectors of the scalar rows `source_rows` through the forward recurrence, the
    four rows of every target site picked at every n: (M, T, 4, S) with [n, t, a, v] = <e_{4 j_t + a}|T_n(H~)|e_row_v>.
    h dense or sparse (4N, 4N)."""
    source_rows = np.asarray(source_rows, dtype=np.int64)
    target_sites = np.asarray(target_sites, dtype=np.int64)
    start = np.zeros((h.shape[0], source_rows.size), dtype=h.dtype)
    start[source_rows, np.arange(source_rows.size)] = 1.0
    pick = (4 * target_sites[:, None] + np.arange(4)[None, :]).reshape(-1)
    mu = np.empty((moments, target_sites.size, 4, source_rows.size), dtype=np.complex128)
    for n, t in enumerate(_forward(h, scale, moments, start)):
        mu[n] = np.asarray(t)[pick].reshape(target_sites.size, 4, source_rows.size)
    return mu


def local_moments(h, scale, moments, sites, columns=4, chunk=32):
    """bdg_green_local_moments in numpy: column `columns` * s + b starts at e_{4 j_s + b}, every column runs the forward
    recurrence on its own, and of every t_n the four rows of the column's own site are picked: (M, S, 4, columns) with
    [n, s, a, b] = <e_{4 j_s + a}|T_n(H~)|e_{4 j_s + b}>.  The sites go `chunk` at a time (memory only: a column does
    not see its neighbours).  h dense or sparse (4N, 4N)."""
    sites = np.asarray(sites, dtype=np.int64)
    mu = np.empty((moments, sites.size, 4, columns), dtype=np.complex128)
    for s0 in range(0, sites.size, chunk):
        own = sites[s0 : s0 + chunk]
        width = own.size * columns
        start = np.zeros((h.shape[0], width), dtype=h.dtype)
        start[(4 * own[:, None] + np.arange(columns)[None, :]).reshape(-1), np.arange(width)] = 1.0
        rows = 4 * np.repeat(own, columns)[None, :] + np.arange(4)[:, None]    # [a, v]: row a of the site of column v
        for n, t in enumerate(_forward(h, scale, moments, start)):
            picked = np.asarray(t)[rows, np.arange(width)[None, :]]            # [a, v]
            mu[n, s0 : s0 + chunk] = picked.reshape(4, own.size, columns).transpose(1, 0, 2)
    return mu


def dense_chebyshev_moments(w, v, scale, moments, rows, columns):
    """[n, i, k] = (V cos(n arccos(E / scale)) V†)[rows_i, columns_k] from the eigenpairs (w, v) of eigh."""
    theta = np.arccos(np.clip(w / scale, -1.0, 1.0))
    table = np.cos(np.arange(moments)[:, None] * theta[None, :])               # (M, 4N)
    return np.einsum("ia,na,ka->nik", v[np.asarray(rows)], table, v[np.asarray(columns)].conj(), optimize=True)


def local_sample(shape=SHAPE):
    """The sites of a 2-D lattice whose local moments the restatement covers: a grid of 8 x 7 sites nine apart,
    (3 + 9a, 4 + 9b), and the last eight sites, 63 of 4221 (all sites would take a minute of numpy).  Their offsets
    within a tile of 8 rows are (1 + b - a) mod 8: all of them.  Each of these columns is a recurrence over all block
    rows, and within M steps a picked row hears of every row up to M - 1 bonds away: a wrong row anywhere on the lattice
    is at most 8 bonds from a sampled site (tests/test_family_tiles_host.py), where it arrives damped by some 1 / scale
    per bond, 1e-6 against a bound of 1e-13.  The other sites are tied to these by the bit equality with the one-tile
    run."""
    lx, ly, lz = shape
    assert lz == 1
    x, y = np.meshgrid(np.arange(3, lx, 9), np.arange(4, ly, 9), indexing="ij")
    return np.union1d((y + ly * x).reshape(-1), np.arange(lx * ly - 8, lx * ly))


# ------------------------------------------------------------------ cached references
@functools.lru_cache(maxsize=None)
def restated(entry, name):
    """The numpy restatement of ENTRY_POINTS[entry] on SYSTEMS[name] (sparse H): computed once, shared, read-only.
    green_local_moments: on the sites local_sample() only, in ascending order (the device result has every site: take
    its rows with local_positions())."""
    system = system_of(name)
    h, scale, n = sparse_of(name), scale_of(system_of(name)), system.lattice.size
    if entry == "fermi_blocks":
        colours, n_colours = fermi_colours(n)
        coef = fermi_cases.fermi_coefficients(system, fermi_cases.TEMPERATURE, M)
        out = fermi_cases.restated_blocks(system, scale, coef, colours, n_colours, 4, *fermi_cases.pattern_of(system))
    elif entry == "apply_series":
        out = apply_cases.stored_source_clenshaw(h, scale, apply_coefficients(system), apply_vectors(system))
    elif entry == "green_moments":
        out = picked_moments(h, scale, M, green_sources(n), green_targets(n))
    elif entry == "green_local_moments":
        real = abs(h.imag).max() == 0  # (float64 is four times cheaper, and what the device does with a real matrix)
        out = local_moments(h.real if real else h, scale, M, local_sample(system.lattice.shape))
    else:
        raise KeyError(entry)
    out.setflags(write=False)
    return out


def local_positions(shape=SHAPE):
    """Where the sites of local_sample() stand in local_sites(): result[:, local_positions()] is the sample's."""
    n_sites = int(np.prod(shape))
    where = np.empty(n_sites, dtype=np.int64)
    where[local_sites(n_sites)] = np.arange(n_sites)
    return where[local_sample(shape)]


def rounding_bound(moments, reference):
    """32·M·2⁻⁵³·max(1, max|reference|): at most 32 roundings per entry and step of the recurrence, relative to the
    largest entry (derived in test_gpu_clenshaw_switches.test_strip_ordered_tiles_do_not_change_one_bit)."""
    return 32 * moments * 2.0**-53 * max(1.0, float(np.abs(reference).max()))


@functools.lru_cache(maxsize=None)
def restated_state_moments(name):
    """green_states_cases.state_moments of states_of() on SYSTEMS[name], M moments, 4 columns: read-only."""
    system = system_of(name)
    out = green_states_cases.state_moments(system, states_of(system), M, scale_of(system), columns=4)
    out.setflags(write=False)
    return out
