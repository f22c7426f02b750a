#!/usr/bin/env python3
"""eigenpairs() on a 64x64 s-wave lattice with magnetic impurities: every state below 0.8 Δ, and lowest_eigenpairs(k)
for the same k on the same commit (profiles/eigenpairs.json).  Needs a GPU.

    python3 tools/eigenpairs_benchmark.py [--out profiles/eigenpairs.json] [--size 64] [--impurities 24] [--moments M]

The lattice: t = 1, μ = 0.5, Δ = 0.5 jσ2, `impurities` random sites with an on-site -J u σ3, J = 2, u uniform in
[0.6, 1.4]; window (0, 0.8 Δ).  Reported: states found, iterations, columns, degree, wall time of the call and its split
into filter, project and rotate (wall time of the library calls, each of which ends with a stream synchronisation; the
rest is the host's Rayleigh-Ritz step and the transfers), the largest residual, and wall time and result of
lowest_eigenpairs(k) for the k found, capped at --lanczos-max-iter iterations (what did not converge by then is in
its warnings).  One warm-up call, then the median of three (of two for lowest_eigenpairs).  No rate or ratio is
claimed before the file this writes exists.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bodge_amd as ba
from bodge_amd.observables import _scale_of

GAP = 0.5


def impurity_lattice(size, impurities, seed=0):
    lattice = ba.CubicLattice((size, size, 1))
    system = ba.Hamiltonian(lattice)
    rng = np.random.default_rng(seed)
    sites = list(lattice.sites())
    strength = {sites[int(c)]: 2.0 * (0.6 + 0.8 * rng.random()) for c in rng.choice(len(sites), size=impurities, replace=False)}
    with system as (H, D):
        for i in sites:
            H[i, i] = -0.5 * ba.σ0 - strength.get(i, 0.0) * ba.σ3
            D[i, i] = GAP * ba.jσ2
        for i, j in lattice.bonds():
            H[i, j] = -1.0 * ba.σ0
    return system


class Stopwatch:
    """Wall time spent inside the named methods of a solver."""

    def __init__(self, solver, names):
        self.seconds = {name: 0.0 for name in names}
        self._solver, self._originals = solver, {}
        for name in names:
            original = getattr(solver, name)
            self._originals[name] = original
            setattr(solver, name, self._timed(name, original))

    def _timed(self, name, original):
        def call(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return original(*args, **kwargs)
            finally:
                self.seconds[name] += time.perf_counter() - t0
        return call

    def stop(self):
        for name in self._originals:
            delattr(self._solver, name)
        return dict(self.seconds)


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eigenpairs.json"))
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--impurities", type=int, default=24)
ap.add_argument("--moments", type=int, default=None)
ap.add_argument("--lanczos-max-iter", type=int, default=4000,
                help="iteration cap of the lowest_eigenpairs comparison (its default of 20000 with k in the tens takes "
                     "more than seven minutes, most of it the host's tridiagonal solves at every checkpoint)")
args = ap.parse_args()

system = impurity_lattice(args.size, args.impurities)
solver = system._solver()
scale = _scale_of(system)
window = (0.0, 0.8 * GAP)
options = {"method": "subspace", "moments": args.moments, "format": "raw"}
system.eigenpairs(window, **options)  # warm-up (tables, buffers, kernel load)
runs = []
for _ in range(3):
    watch = Stopwatch(solver, ("subspace_filter", "subspace_project", "subspace_rotate"))
    t0 = time.perf_counter()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        energies, states = system.eigenpairs(window, **options)
    wall = time.perf_counter() - t0
    split = watch.stop()
    runs.append({"wall_s": wall, "filter_s": split["subspace_filter"], "project_s": split["subspace_project"],
                 "rotate_s": split["subspace_rotate"], "warnings": [str(w.message) for w in caught]})
report = dict(solver.last_eigenpairs)
h = system.matrix("csr")
residual = float(np.linalg.norm(h @ states - states * energies, axis=0).max()) if len(energies) else 0.0
record = {"lattice": f"{args.size}x{args.size}", "impurities": args.impurities, "window": list(window), "scale": scale,
          "states": int(len(energies)), **report, "runs": runs,
          "wall_s_median": statistics.median(r["wall_s"] for r in runs),
          "filter_s_median": statistics.median(r["filter_s"] for r in runs),
          "project_s_median": statistics.median(r["project_s"] for r in runs),
          "rotate_s_median": statistics.median(r["rotate_s"] for r in runs),
          "largest_residual_over_scale": residual / scale,
          "orthonormality": float(np.abs(states.conj().T @ states - np.eye(len(energies))).max()) if len(energies) else 0.0}
print(json.dumps({"eigenpairs": record}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:  # (written again below with the comparison: that part can take long)
    json.dump(record, fh, indent=1)

k = max(1, len(energies))
walls = []
for attempt in range(3):  # (the first is the warm-up)
    t0 = time.perf_counter()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            low_e, low_v = system.lowest_eigenpairs(k, method="lanczos", format="raw", vectors=16,
                                                    max_iter=args.lanczos_max_iter)
            failure = None
        except (RuntimeError, ValueError) as exc:
            low_e, failure = np.zeros(0), str(exc)
    walls.append(time.perf_counter() - t0)
found = min(len(low_e), len(energies))
record["lowest_eigenpairs"] = {
    "k": k, "vectors": 16, "max_iter": args.lanczos_max_iter, "found": int(len(low_e)), "wall_s": walls[1:], "wall_s_median": statistics.median(walls[1:]),
    "warnings": [str(w.message) for w in caught], "failure": failure,
    "largest_difference": float(np.abs(low_e[:found] - energies[:found]).max()) if found else None}
print(json.dumps({"lowest_eigenpairs": record["lowest_eigenpairs"]}), flush=True)
with open(args.out, "w") as fh:
    json.dump(record, fh, indent=1)
