"""Shared by tests/test_roll_units_host.py and tests/test_gpu_roll_units.py: the 3-D rolling kernel (cheb_roll3, K8) with
its units cut for equal length (RollArgs.chunk > 0).

* Plain Python restatements of how the host picks the launch shape (plans.hpp: choose_segments, RollPlan::segments_for,
  RollPlan::chunk_for) and of how the kernel turns a unit into its pieces (sweep.hpp, the `while (g0 < g1)` loop).
* `palette_system`: a lattice matrix that is not translation invariant and has few distinct blocks, built with the
  array setters alone.
* The case table and the oracle's dot products per (system, start, steps), computed once and handed
  out read-only.

The cases are sized for 256 CUs with one workgroup per CU (BODGE_AMD_BLOCKS_PER_CU=1): 1024 wave slots."""

import functools
from collections import namedtuple

import numpy as np

import bodge_amd as ba
from oracle import cheb_ref

WAVES = 1024           # 256 CUs x 1 workgroup x 4 waves
GRID = 256
COMMON_KNOBS = {"BODGE_AMD_SWEEP": "1", "BODGE_AMD_BLOCKS_PER_CU": "1"}


# ------------------------------------------------------------------ restatements
def choose_segments(n_cols, lx, waves, extra_planes, min_planes, keep=0.97):
    """plans.hpp choose_segments: x-segments per column that cost the fewest (rounds of waves) x (planes per wave)."""
    best, best_cost = 1, 0.0
    for segs in range(1, max(1, lx // min_planes) + 1):
        units = n_cols * segs
        rounds = float((units + waves - 1) // waves)
        cost = rounds * (float((lx + segs - 1) // segs) + extra_planes)
        if segs == 1 or cost < keep * best_cost:
            best, best_cost = segs, cost
    return best


def roll_owned(lanes):
    return 64 // lanes - 2


def windows(shape, lanes):
    """RollArgs.n_cols: windows of `roll_owned(lanes)` in-plane positions per plane."""
    plane = shape[1] * shape[2]
    return (plane + roll_owned(lanes) - 1) // roll_owned(lanes)


class RollPlan:
    """The part of plans.hpp's RollPlan that decides the shape of a launch."""

    def __init__(self, n_cols, lx, waves=WAVES, share=1):
        self.n_cols, self.lx, self.waves, self.share = n_cols, lx, waves, share
        self.whole_segs = max(1, min(choose_segments(n_cols, lx, waves, 2, 4), lx // 4))  # make_roll_plan

    def segments_for(self, planes):
        if planes >= self.lx:
            return self.whole_segs
        return max(1, min(choose_segments(self.n_cols, planes, self.waves, 2, 4), planes // 4))

    def chunk_for(self, planes):
        slots = max(1, self.waves // max(1, self.share))
        total = self.n_cols * planes
        units = self.n_cols * self.segments_for(planes) * max(1, self.share)
        if int(0.92 * self.waves) <= units <= self.waves:  # ((int64_t)(0.92 * waves): truncated)
            return 0
        chunk = (total + slots - 1) // slots
        return chunk if 8 <= chunk <= planes else 0


def units(n_cols, x_lo, x_hi, chunk):
    """cheb_roll3 with chunk > 0: the pieces [(col, x0, x1), ...] of every unit, as its loop makes them."""
    span = x_hi - x_lo
    plane_steps = n_cols * span
    out = []
    for u in range((plane_steps + chunk - 1) // chunk):
        g0 = u * chunk
        g1 = min(g0 + chunk, plane_steps)
        pieces = []
        while g0 < g1:
            col = g0 // span
            xa = g0 - col * span
            xb = min(xa + (g1 - g0), span)
            pieces.append((col, x_lo + xa, x_lo + xb))
            g0 += xb - xa
        out.append(pieces)
    return out


def act_planes(x0, x1, reverse):
    """The planes a piece advances, in marching order: act(k) = x0 + x1 - 1 - k on the piece's bounds when reversed."""
    return [x0 + x1 - 1 - k if reverse else k for k in range(x0, x1)]


# ------------------------------------------------------------------ systems
_MU = np.array([2.6, 2.75, 2.9, 3.05, 3.2, 3.35, 3.5, 3.65])
_ZEEMAN = np.array([0.0, 0.05, -0.04, 0.08, 0.02, -0.07, 0.03, 0.06])
_GAP = np.array([0.10, 0.13, 0.07, 0.16, 0.11, 0.09, 0.14, 0.12])
_HOP = np.array([1.0, 0.9, 1.1, 0.95])
_HOP_Z = np.array([0.0, 0.05, -0.04, 0.02])
_DWAVE = 0.1
_PHASE = 0.3


def _hash(a):
    """SplitMix64 finaliser: which palette entry a site / bond gets."""
    return cheb_ref._splitmix64(np.asarray(a, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def palette_system(shape, kind="real"):
    """Open lattice whose blocks come from small palettes chosen by a hash: on-site μ_k σ0 - m_k σ3 with -Δ_k jσ2 (8
    entries, by site index), hopping -t_k σ0 + δ_k σ3 (4 entries, by the bond's (lo, hi) sites), d-wave pairing on the
    bonds.  Not translation invariant: a wrong stencil word, or a plane read from the wrong place, changes the numbers.
    kind "real": 20 distinct blocks; "peierls": the x bonds carry e^{±0.3i} as well (complex, 24 distinct blocks)."""
    if kind not in ("real", "peierls"):
        raise ValueError(kind)
    lattice = ba.CubicLattice(shape)
    system = ba.Hamiltonian(lattice)
    system.hermiticity_check = "host"  # (the same builder with and without a GPU; the system keeps no device mirror)
    site = (_hash(np.arange(lattice.size)) >> np.uint64(33)).astype(np.int64) % 8
    pairs = lattice.bond_array()
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    bond = (_hash(lo * lattice.size + hi) >> np.uint64(33)).astype(np.int64) % 4
    hop = -_HOP[bond, None, None] * ba.σ0 + _HOP_Z[bond, None, None] * ba.σ3
    if kind == "peierls":
        along_x = hi - lo == shape[1] * shape[2]
        forward = pairs[:, 1] > pairs[:, 0]
        hop = hop * np.where(along_x, np.exp(1j * _PHASE * np.where(forward, 1.0, -1.0)), 1.0)[:, None, None]
    coords = lattice.bond_array(coords=True)
    with system as (H, Δ):
        H.set_sites(_MU[site, None, None] * ba.σ0 - _ZEEMAN[site, None, None] * ba.σ3)
        Δ.set_sites(-_GAP[site, None, None] * ba.jσ2)
        H.set_bonds(hop)
        Δ.set_bonds(-_DWAVE * ba.dwave()(coords[:, 0], coords[:, 1]))
    return system


@functools.lru_cache(maxsize=None)
def matrix_of(shape, kind):
    bsr = palette_system(shape, kind).matrix("bsr")
    return bsr, cheb_ref.spectral_bound(bsr)


# ------------------------------------------------------------------ cases
# start: ("rademacher" | "z4", n_vectors, seed) or ("unit", plane): 8 unit rows on that plane
# chunk / n_units / two_piece / shortest / last_unit: what the LAST launch of the run must look like
Case = namedtuple("Case", "shape kind start steps lanes share knobs chunk n_units two_piece shortest last_unit")

CASES = {
    "A": Case((24, 72, 75), "real", ("rademacher", 8, 11), 7, 4, 1, {}, 10, 927, 308, 2, 4),
    "B": Case((24, 72, 75), "real", ("rademacher", 16, 12), 6, 4, 2, {}, 19, 488, 365, 1, 11),
    "C": Case((42, 72, 75), "real", ("rademacher", 4, 13), 6, 2, 1, {}, 8, 945, 135, 2, 8),
    "D": Case((24, 72, 75), "peierls", ("z4", 4, 14), 7, 4, 1, {}, 10, 927, 308, 2, 4),
    # A in the other arithmetic modes.  Complex arithmetic carries 4 vectors per lane group: the 8 vectors are two lane
    # groups side by side on two streams (share 2), cut like B
    "E-full": Case((24, 72, 75), "real", ("rademacher", 8, 11), 7, 4, 1, {"BODGE_AMD_PH": "0"}, 10, 927, 308, 2, 4),
    "E-complex": Case((24, 72, 75), "real", ("rademacher", 8, 11), 7, 4, 2, {"BODGE_AMD_REAL": "0"}, 19, 488, 365, 1, 11),
    "E-complex-full": Case((24, 72, 75), "real", ("rademacher", 8, 11), 7, 4, 2,
                           {"BODGE_AMD_PH": "0", "BODGE_AMD_REAL": "0"}, 19, 488, 365, 1, 11),
    "F9": Case((24, 72, 75), "real", ("unit", 12), 9, 4, 1, {}, 8, 917, 337, 1, 6),
    "F14": Case((24, 72, 75), "real", ("unit", 12), 14, 4, 1, {}, 10, 927, 308, 2, 4),
    # unit rows on plane 5: the band stays against x = 0 and never reaches x = 23 - launches 12-15 are cut (8, 8, 8, 9) with
    # x_lo + x_hi != lx, two of them reversed: a reversal about anything but the band's own bounds lands on other planes
    "F16-low": Case((24, 72, 75), "real", ("unit", 5), 16, 4, 1, {}, 9, 944, 343, 1, 5),
    # two slabs of 24 planes: every member plans for its own planes, with share 1 (run_group)
    "G": Case((48, 72, 75), "real", ("rademacher", 8, 15), 7, 4, 1, {}, 10, 927, 308, 2, 4),
}
# (real_arithmetic, ph_packed) the perf record must show
MODES = {"A": (1, 1), "B": (1, 1), "C": (1, 1), "D": (0, 1), "E-full": (1, 0), "E-complex": (0, 1),
         "E-complex-full": (0, 0), "F9": (1, 1), "F14": (1, 1), "F16-low": (1, 1), "G": (1, 1)}
SLABS = {"G": 2}


def planes_of(name):
    """Planes one handle of the case owns (slab members: their share of the lattice)."""
    return CASES[name].shape[0] // SLABS.get(name, 1)


def plan_of(name):
    case = CASES[name]
    return RollPlan(windows(case.shape, case.lanes), planes_of(name), WAVES, case.share)


def launches(name):
    """(x_lo, x_hi, n_segs, chunk) of every launch of the case's run, as Batch::step sets them."""
    case, plan = CASES[name], plan_of(name)
    out = []
    for n in range(case.steps):
        x_lo, x_hi = 0, plan.lx
        if case.start[0] == "unit":
            x_lo, x_hi = max(0, case.start[1] - (n + 1)), min(plan.lx, case.start[1] + n + 2)
        out.append((x_lo, x_hi, plan.segments_for(x_hi - x_lo), plan.chunk_for(x_hi - x_lo)))
    return out


def unit_rows(name):
    """Case F: 8 unit rows on one plane, distinct y, z and Nambu components."""
    case = CASES[name]
    _, ly, lz = case.shape
    x = case.start[1]
    sites = [(3, 5), (70, 74), (0, 0), (35, 40), (71, 1), (17, 62), (44, 13), (9, 33)]
    return np.array([4 * ((x * ly + y) * lz + z) + (i % 4) for i, (y, z) in enumerate(sites)], dtype=np.int64)


def start_block(name):
    case = CASES[name]
    n = 4 * int(np.prod(case.shape))
    if case.start[0] == "unit":
        return cheb_ref.unit_block(n, unit_rows(name))
    kind = cheb_ref.VEC_Z4 if case.start[0] == "z4" else cheb_ref.VEC_RADEMACHER
    return cheb_ref.random_block(n, case.start[2], range(case.start[1]), kind)


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = CASES[name]
    bsr, scale = matrix_of(case.shape, case.kind)
    d, e = cheb_ref.recurrence_dots(bsr, scale, 2 * case.steps, start_block(name))
    d.setflags(write=False)
    e.setflags(write=False)
    return d, e


def reference(name):
    """The oracle's (d, e), all columns and all steps of the case (read-only): one run per (system, start), as long as
    the longest case that shares them."""
    case = CASES[name]
    same = [(c.steps, other) for other, c in CASES.items() if (c.shape, c.kind, c.start) == (case.shape, case.kind, case.start)]
    d, e = _reference(max(same)[1])
    return d[:case.steps], e[:case.steps]
