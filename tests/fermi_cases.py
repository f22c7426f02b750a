"""Shared by tests/test_fermi_host.py, tests/test_gpu_fermi.py and tests/test_gpu_clenshaw_switches.py: the systems, the
colourings, the numpy restatement of the probed Clenshaw recurrence of bdg_fermi_blocks, and the dense eigh oracle of
a probed result for any colouring.

For any colouring - whether it respects a distance or not - the probed result of block (j, i), column b, is the sum over
the sites i' of i's colour of the dense g(H)[4j:4j+4, 4i'+b]: the kernels do not care how far apart the sites of one
colour are, so a random colouring is a sharp reference for them."""

import functools

import numpy as np
import scipy.sparse as sp

import bodge_amd as ba
from bodge_amd import chebyshev as cheb
from bodge_amd import fermi

import apply_cases

TEMPERATURE = 0.1
COLOUR_COUNTS = (1, 5, 33)  # in 4 components: one batch with padding lanes, 20 vectors, 132 vectors in three batches


# ------------------------------------------------------------------ systems
def swave(shape=(6, 5, 1), mu=0.5, gap=0.3, zeeman=0.2, hop=-1.0, periodic=False):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        H.set_sites(-mu * ba.σ0 - zeeman * ba.σ3)
        Δ.set_sites(gap * ba.jσ2)
        H.set_bonds(hop * ba.σ0)
        if periodic:
            H.set_edges(hop * ba.σ0)
    return system


def pwave_chiral(shape=(5, 5, 1)):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    spin = ba.pwave("e_z * (p_x + jp_y)")
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -0.7 * ba.σ0
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
            Δ[i, j] = 0.4 * spin(i, j)
    return system


def dwave_bonds(shape=(6, 6, 1), mu=0.4, amplitude=0.3, hop=-1.0):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    spin = ba.dwave()
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -mu * ba.σ0
        for i, j in lattice.bonds():
            H[i, j] = hop * ba.σ0
            Δ[i, j] = amplitude * spin(i, j)
    return system


def ssd_envelope(shape=(6, 6, 1)):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    envelope = ba.ssd(system)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -0.5 * envelope(i, i) * ba.σ0
            Δ[i, i] = 0.4 * envelope(i, i) * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * envelope(i, j) * ba.σ0
    return system


def phases(shape=(5, 6, 1)):
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    with system as (H, Δ):
        for i in lattice.sites():
            H[i, i] = -0.3 * ba.σ0 + 0.1 * ba.σ1
            Δ[i, i] = 0.3 * ba.jσ2
        for i, j in lattice.bonds():
            step = np.subtract(j, i)
            H[i, j] = -np.exp(1j * (0.7 * step[0] + 0.3 * step[1])) * ba.σ0
    return system


# the seven systems of the exact-mode tests of tests/test_gpu_fermi.py
EXACT_MODE_SYSTEMS = {
    "swave_zeeman": lambda: swave(),
    "pwave_chiral": pwave_chiral,
    "dwave": dwave_bonds,
    "ssd": ssd_envelope,
    "phases": phases,
    "periodic_7x4": lambda: swave((7, 4, 1), periodic=True),
    "cubic_3d": lambda: swave((3, 3, 3), mu=0.2),
}

SYSTEMS = {
    **EXACT_MODE_SYSTEMS,
    **apply_cases.SYSTEMS,                      # disordered_300: more distinct on-site blocks than a dictionary holds
    "chain_3": lambda: swave((3, 1, 1)),        # fewer block rows than one wave holds at any lane width
    "single_site": lambda: swave((1, 1, 1)),
    "gapped_12x12": lambda: swave((12, 12, 1), mu=0.5, gap=1.0, zeeman=0.0),  # the finite-distance path (periods 3, 6)
    "strips_6x150": lambda: swave((6, 150, 1)),  # 900 sites: strip-ordered tiles (no dense reference at this size)
}
# ... of which these go through every kernel form against both references
REFERENCE_SYSTEMS = sorted(set(SYSTEMS) - {"gapped_12x12", "strips_6x150"})
# ... and these certainly have a block dictionary (a handful of distinct blocks, at most 7 per row)
DICTIONARY_SYSTEMS = ("swave_zeeman", "dwave", "periodic_7x4", "cubic_3d", "dictionary", "cube")


@functools.lru_cache(maxsize=None)
def system_of(name):
    """The system for host-side use (matrices, patterns, references): built once, never modified.  A test that flips a
    switch read at upload builds its own with SYSTEMS[name]()."""
    return SYSTEMS[name]()


def scale_of(system):
    return 1.01 * system.gershgorin_bound()


def pattern_of(system):
    """H's block skeleton (zero blocks included), the pattern fermi_matrix fills."""
    return system._matrix.indptr.astype(np.int32), system._matrix.indices.astype(np.int32)


def fermi_coefficients(system, temperature, moments=None):
    scale = scale_of(system)
    m = cheb.moments_for_fermi(scale, temperature) if moments is None else moments
    return cheb.chebyshev_coefficients(lambda x: cheb.fermi_function(scale * x, temperature), m)


def is_real(system):
    return bool(np.abs(system.bsr_arrays()[2].imag).max(initial=0.0) == 0)


def is_particle_hole_packed(system):
    """The library's rule at upload: the lower-right 2x2 of every block is minus the conjugate of the upper-left."""
    data = system.bsr_arrays()[2]
    return bool(np.array_equal(data[:, 2:4, 2:4], -data[:, 0:2, 0:2].conj()))


# ------------------------------------------------------------------ colourings (all seeded)
def random_colours(n_sites, n_colours, seed=0):
    """Colours drawn from -1 .. n_colours - 1 with no regard to the lattice: adjacent sites share colours, some sites are
    not probed (-1) and, with more colours than sites, some colours are empty."""
    rng = np.random.default_rng([seed, n_sites, n_colours])
    return rng.integers(-1, n_colours, n_sites).astype(np.int32)


def shared_out_colours(colours, n_colours, lo, hi):
    """What one device of a `devices=[...]` run is given: the colours lo .. hi - 1 renumbered from 0, the rest -1."""
    return np.where((colours >= lo) & (colours < hi), colours - lo, -1).astype(np.int32), hi - lo


def colouring(name, key):
    """(colours, n_colours) of system `name` for a hashable key:
    ("random", n_colours, seed), ("distance", d) = fermi.site_colours, ("shared", n_colours, seed, lo, hi)."""
    system = system_of(name)
    n = system.lattice.size
    if key[0] == "random":
        return random_colours(n, key[1], key[2]), key[1]
    if key[0] == "distance":
        colours, n_colours = fermi.site_colours(system, key[1])
        return colours.astype(np.int32), n_colours
    if key[0] == "shared":
        return shared_out_colours(random_colours(n, key[1], key[2]), key[1], key[3], key[4])
    raise KeyError(key)


# the colourings whose reference distances set a system's tolerance
TOLERANCE_COLOURINGS = tuple(("random", c, 0) for c in COLOUR_COUNTS) + (("shared", 33, 0, 9, 21),)


# ------------------------------------------------------------------ restatement and oracle
def restated_blocks(system, scale, coef, colours, n_colours, components, indptr, indices):
    """The algorithm of bdg_fermi_blocks in numpy: one probe per (colour, component), Clenshaw's recurrence
    b_k = 2 H~ b_{k+1} - b_{k+2} + c_k r (k = M-1 .. 1), y = H~ b_1 - b_2 + c_0 r, and the extraction of the pattern
    columns.  (nnzb, 4, 4); the columns from `components` on, and the blocks whose column site has colour -1, stay 0."""
    h = sp.csr_matrix(system.matrix("csr"))
    n = system.lattice.size
    coef = np.asarray(coef, dtype=np.float64)
    colours = np.asarray(colours)
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    out = np.zeros((len(indices), 4, 4), dtype=np.complex128)
    for c in range(n_colours):
        members = np.flatnonzero(colours == c)
        mine = np.flatnonzero(colours[indices] == c)
        if len(members) == 0 or len(mine) == 0:
            continue
        probes = np.zeros((4 * n, components))
        for b in range(components):
            probes[4 * members + b, b] = 1.0
        b1 = np.zeros_like(probes, dtype=np.complex128)
        b2 = np.zeros_like(b1)
        for k in range(len(coef) - 1, 0, -1):
            b1, b2 = 2 * (h @ b1) / scale - b2 + coef[k] * probes, b1
        y = (h @ b1) / scale - b2 + coef[0] * probes
        for b in range(components):
            out[mine, :, b] = y.reshape(n, 4, components)[rows[mine], :, b]
    return out


@functools.lru_cache(maxsize=None)
def _eigh(name):
    return np.linalg.eigh(np.asarray(system_of(name).matrix("dense")))


def dense_function(system, values_of, name=None):
    """V g(E) V† by numpy.linalg.eigh, (4N, 4N); `name` shares the eigenpairs of a system of SYSTEMS."""
    w, v = _eigh(name) if name is not None else np.linalg.eigh(np.asarray(system.matrix("dense")))
    return (v * np.asarray(values_of(w))) @ v.conj().T


def dense_probed_blocks(system, values_of, colours, n_colours, components, indptr, indices, name=None):
    """V g(E) V† from numpy.linalg.eigh times the 0/1 probe matrix, cut to the pattern: block k = (j, i), column b, is
    Σ_{i' of i's colour} g(H)[4j:4j+4, 4i'+b].  Blocks whose column site is not probed (colour -1) are zero, and so are
    the columns from `components` on."""
    n = system.lattice.size
    full = dense_function(system, values_of, name).reshape(n, 4, n, 4)
    colours = np.asarray(colours)
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    out = np.zeros((len(indices), 4, 4), dtype=np.complex128)
    for c in range(n_colours):
        mine = np.flatnonzero(colours[indices] == c)
        if len(mine) == 0:
            continue
        summed = full[:, :, np.flatnonzero(colours == c), :components].sum(axis=2)  # (n, 4, components)
        out[mine, :, :components] = summed[rows[mine]]
    return out


# ------------------------------------------------------------------ cached references
@functools.lru_cache(maxsize=None)
def references(name, temperature, key):
    """(restated, dense, largest |dense entry|, distance of the two) of the Fermi function on H's skeleton for one
    (system, temperature, colouring), in 4 components: computed once, shared, read-only.  The columns of a probe do not
    depend on the other probes (in the references as on the device), so the 2-component result is `two_components` of
    this one."""
    system = system_of(name)
    colours, n_colours = colouring(name, key)
    indptr, indices = pattern_of(system)
    coef = fermi_coefficients(system, temperature)
    restated = restated_blocks(system, scale_of(system), coef, colours, n_colours, 4, indptr, indices)
    dense = dense_probed_blocks(system, lambda e: cheb.fermi_function(e, temperature), colours, n_colours, 4, indptr,
                                indices, name)
    restated.setflags(write=False)
    dense.setflags(write=False)
    return restated, dense, float(np.abs(dense).max()), float(np.abs(restated - dense).max())


def two_components(blocks):
    """The result of a 2-component call: columns 0 and 1, the others zero."""
    out = np.zeros_like(blocks)
    out[:, :, :2] = blocks[:, :, :2]
    return out


@functools.lru_cache(maxsize=None)
def reference_distance(name, temperature, keys=TOLERANCE_COLOURINGS):
    """One number per (system, temperature): the largest distance of the two references over the system's colourings."""
    return max(references(name, temperature, key)[3] for key in keys)


# ------------------------------------------------------------------ what run_fermi_blocks derives
def batch_plan(real, n_colours, components, lanes_override=0):
    """(lanes per row, colours per batch, batches) as run_fermi_blocks derives them for a small matrix (the 96 MB rule
    of the vector buffer does not bind): whole colours per batch, at most 64 vectors, `lanes_override` lanes when
    set_lanes_per_row fixes them (a lane holds two vectors in real arithmetic)."""
    per_lane = 2 if real else 1
    width = 64
    if lanes_override >= 4:
        width = min(64, lanes_override * per_lane)
    per_batch = max(1, min(n_colours, width // components))
    active = per_batch * components
    lanes = max(4, 1 << (-(-active // per_lane) - 1).bit_length())
    if lanes_override >= 4 and lanes_override * per_lane >= active:
        lanes = lanes_override
    return lanes, per_batch, -(-n_colours // per_batch)


def tiles_of(n_sites, lanes):
    """Row tiles of a launch: 64 / lanes block rows per wave, four waves per workgroup."""
    rows_per_tile = (64 // lanes) * 4
    return -(-n_sites // rows_per_tile)
