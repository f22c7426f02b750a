#!/usr/bin/env python3
"""What probing costs in accuracy, from the dense resolvent on the CPU (no GPU needed): a disordered
32 x 32 s-wave model (gap 0.3), `distance=16` (256 colours of 4 sites).  For Γ = 0.1 and 0.3 and energies inside the gap
and in the band, the worst-site error of the probed LDOS relative to the largest exact LDOS at that energy set: with
signs +1 (the bias) and for the mean of 4 and 16 samples of ±1 signs (noise), from the probed dense sum
D_jj = Σ_{j' in colour(j)} ξ_j ξ_j' G_jj'.

    python3 tools/green_probe_accuracy.py [--size 32] [--distance 16]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bodge_amd as ba
from bodge_amd import fermi, green

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=32)
ap.add_argument("--distance", type=int, default=16)
args = ap.parse_args()

L, GAP = args.size, 0.3
lattice = ba.CubicLattice((L, L, 1))
system = ba.Hamiltonian(lattice)
with system as (H, D):
    H.set_sites((-0.5 + np.random.default_rng(5).uniform(-0.2, 0.2, L * L))[:, None, None] * ba.σ0)
    D.set_sites(GAP * ba.jσ2)
    H.set_bonds(-1.0 * ba.σ0)
n = L * L
colour, n_colours = fermi.site_colours(system, args.distance)
w, v = np.linalg.eigh(np.asarray(system.matrix("dense")))
member = np.zeros((n_colours, n))
member[colour, np.arange(n)] = 1.0


def ldos_error(z, signs):
    """max over sites of |probed LDOS - exact LDOS| for the mean over the rows of `signs`, and the largest exact LDOS."""
    g = ((v / (z - w)[None, :]) @ v.conj().T).reshape(n, 4, n, 4)
    exact = -(g[np.arange(n), 0, np.arange(n), 0] + g[np.arange(n), 1, np.arange(n), 1]).imag / np.pi
    probed = np.zeros(n)
    for xi in signs:
        for a in (0, 1):
            summed = (g[:, a, :, a] * xi[None, :]) @ member.T          # [j, c] = Σ_{j' in c} ξ_j' G_jj'[a][a]
            probed += -(xi * summed[np.arange(n), colour]).imag / np.pi / len(signs)
    return float(np.abs(probed - exact).max()), float(exact.max())


rec = {"lattice": f"{L}x{L}", "gap": GAP, "distance": args.distance, "colours": int(n_colours)}
for gamma in (0.1, 0.3):
    for label, energies in (("in_gap", (0.0, 0.1, 0.2)), ("in_band", (0.5, 1.0, 2.0))):
        row = {}
        for name, signs in (("signs_plus", np.ones((1, n))), ("z2_4_samples", green.z2_signs(0, 4, n).astype(float)),
                            ("z2_16_samples", green.z2_signs(0, 16, n).astype(float))):
            pairs = [ldos_error(e + 1j * gamma, signs) for e in energies]
            row[name] = max(p[0] for p in pairs) / max(p[1] for p in pairs)
        rec[f"gamma_{gamma}_{label}"] = row
print(json.dumps(rec, indent=1))
