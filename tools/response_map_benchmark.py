#!/usr/bin/env python3
"""Time of response_map() on the 64x64 README model against the two routes that were there before it
(profiles/response_map.json).  Needs a GPU.

    python3 tools/response_map_benchmark.py [--out profiles/response_map.json] [--moments 512] [--size 64] [--sample 16]

S_z at the centre site, the static kernel at T = 0.05, M moments; the map on all sites and on a line cut of `size`
sites.  Per case: median of five calls after a warm-up of the wall time of the public call, of the HIP-event window of
the device call, of gemm_ms (the resp_gemm launches) and of gemm_flops / gemm_ms, and the share of the window spent
outside the product (the recurrence, the picks, the contraction).  Two yardsticks, neither of them the code under test:

  pairs      what the map took before: correlation(B_j, A, vectors=<unit vectors of the source rows>) once per target
             site, timed on a sample of `sample` sites spread over the lattice and SCALED to the number of sites of the
             case (the record says so).  Three figures per call: the wall time with .static(T) as the README example
             asks (the coefficients made in every call), the wall time with the coefficients made once outside the
             loop and contracted by hand, and the HIP-event window; each value is compared with the map's entry.
  matmul     torch.matmul of complex128 tensors of the product's shape, (M x M) (M x K), on the same GPU under
             HIP-event timing (torch.cuda.Event), counted with the same 8 flops per complex multiply-add: the kernel
             guide gives no fp64-matrix peak to compare with.

Every step runs in a child process of its own under its own time limit (`--step NAME`), one after the other; the
first one that fails ends the run.  torch brings its own HIP runtime, which finds no device in a process where the
library's has already opened it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

STEP_LIMITS = {"map": 300, "cut": 120, "pairs": 300, "matmul": 300}  # seconds

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--moments", type=int, default=512)
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--sample", type=int, default=16)
ap.add_argument("--temperature", type=float, default=0.05)
ap.add_argument("--step", choices=sorted(STEP_LIMITS), help="run one step in this process and print its record")
ap.add_argument("--entries", type=int, help="step matmul: K, the complex entries of a panel row")
args = ap.parse_args()


def matmul_yardstick(rows, entries, repeats=5):
    """TFLOP/s of torch.matmul on (rows, rows) x (rows, entries) complex128 tensors: median of `repeats` after a warm-up."""
    import torch

    device = torch.device("cuda")
    generator = torch.Generator(device=device).manual_seed(0)
    c = torch.view_as_complex(torch.randn(rows, rows, 2, dtype=torch.float64, device=device, generator=generator))
    x = torch.view_as_complex(torch.randn(rows, entries, 2, dtype=torch.float64, device=device, generator=generator))
    times = []
    for _ in range(repeats + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = torch.matmul(c.T, x)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    del c, x, out
    ms = statistics.median(times[1:])
    return {"rows": rows, "entries": entries, "ms": times[1:], "ms_median": ms, "TFLOPs": 8.0 * rows * rows * entries / ms / 1e9}


def model():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bodge_amd as ba
    from bodge_amd import correlation as corr

    system = ba.Hamiltonian(ba.CubicLattice((args.size, args.size, 1)))
    with system as (H, D):
        H.set_sites(3.0 * ba.σ0 - 0.05 * ba.σ3)
        D.set_sites(-0.1 * ba.jσ2)
        H.set_bonds(-1.0 * ba.σ0)
    source = (args.size // 2, args.size // 2, 0)
    return system, corr, source, corr.spin_operator(system, [source], "z")


def map_step(sites):
    system, corr, source, sz = model()
    options = {"temperature": args.temperature, "moments": args.moments, "sites": sites(system)}
    runs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (M is fixed here, not the rule's: the tail warning is expected)
        system.response_map(sz, temperature=args.temperature, moments=8, sites=options["sites"])  # warm-up
        for _ in range(6):
            t0 = time.time()
            result = system.response_map(sz, **options)
            p = result.info["perf"]
            runs.append({"wall_s": time.time() - t0, "window_ms": p["window_ms"], "gemm_ms": p["gemm_ms"],
                         "TFLOPs": p["gemm_flops"] / p["gemm_ms"] / 1e9})
    runs = runs[1:]
    n_sites = len(result.sites)
    rec = {"sites": n_sites, "moments": args.moments, "lanes_per_row": p["lanes_per_row"], "real": p["real_arithmetic"],
           "ph": p["ph_packed"], "dict_blocks": p["dict_blocks"], "launches": p["launches"], "chunks": result.info["chunks"],
           "entries_per_row": 4 * result.info["columns"] * n_sites, "gemm_flops": p["gemm_flops"],
           "wall_s": [r["wall_s"] for r in runs], "window_ms": [r["window_ms"] for r in runs],
           "gemm_ms": [r["gemm_ms"] for r in runs],
           "wall_s_median": statistics.median(r["wall_s"] for r in runs),
           "window_ms_median": statistics.median(r["window_ms"] for r in runs),
           "gemm_ms_median": statistics.median(r["gemm_ms"] for r in runs),
           "gemm_TFLOPs": statistics.median(r["TFLOPs"] for r in runs)}
    rec["share_outside_gemm"] = 1.0 - rec["gemm_ms_median"] / rec["window_ms_median"]
    chi = result.spin("z")
    rec["chi_zz_source"] = [float(chi[result.sites.index(source)].real), float(chi[result.sites.index(source)].imag)]
    return rec


def pairs_step():
    """The route of the parent commit on a sample of sites; per-call wall times, to be scaled by the caller."""
    import numpy as np

    system, corr, source, sz = model()
    from bodge_amd.chebyshev import chebyshev_coefficients_2d
    from bodge_amd.observables import _scale_of

    n = system.lattice.size
    rows = 4 * system.lattice[source] + np.arange(4)
    vectors = np.zeros((4 * n, 4), dtype=np.complex128)
    vectors[rows, np.arange(4)] = 1.0
    coordinates = list(system.lattice.sites())
    sample = [coordinates[k] for k in np.linspace(0, n - 1, args.sample).astype(int)]
    scale = _scale_of(system)
    c = chebyshev_coefficients_2d(lambda x, y: corr._fermi_difference_quotient(x, y, args.temperature), scale, args.moments)
    system.correlation(corr.spin_operator(system, [sample[0]], "z"), sz, moments=8, vectors=vectors)  # warm-up
    walls, walls_by_hand, windows, values, by_hand = [], [], [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for site in sample:
            t0 = time.time()
            moments = system.correlation(corr.spin_operator(system, [site], "z"), sz, moments=args.moments, vectors=vectors)
            t1 = time.time()
            by_hand.append(0.5 * np.sum(c * moments.mu.T))  # (the coefficients made once, outside the loop)
            t2 = time.time()
            values.append(moments.static(args.temperature))  # (as the README example asks: the coefficients per call)
            t3 = time.time()
            walls.append((t1 - t0) + (t3 - t2))
            walls_by_hand.append(t2 - t0)
            windows.append(moments.info["perf"]["window_ms"])
        chi = system.response_map(sz, temperature=args.temperature, moments=args.moments, sites=sample).spin("z")
    # static() contracts c with mu as Tr[T_n B T_m A]: c is symmetric for the static kernel, so it is the map's entry
    return {"sample": args.sample, "moments": args.moments, "wall_s_per_call": walls, "wall_s_per_call_by_hand": walls_by_hand,
            "window_ms_per_call": windows, "wall_s_per_call_median": statistics.median(walls),
            "wall_s_per_call_by_hand_median": statistics.median(walls_by_hand),
            "window_ms_per_call_median": statistics.median(windows),
            "largest_difference_from_the_map": float(np.abs(np.array(values) - chi).max()),
            "largest_difference_from_the_map_by_hand": float(np.abs(np.array(by_hand) - chi).max()),
            "largest_chi": float(np.abs(chi).max())}


if args.step:
    if args.step == "matmul":
        record = matmul_yardstick(args.moments, args.entries)
    elif args.step == "map":
        record = map_step(lambda system: None)
    elif args.step == "cut":
        record = map_step(lambda system: [(x, args.size // 2, 0) for x in range(args.size)])
    else:
        record = pairs_step()
    print(json.dumps(record), flush=True)
    sys.exit(0)


def run_step(name, *extra):
    """One step in a child process under its own time limit; None (and the reason on stderr) when it fails."""
    command = [sys.executable, os.path.abspath(__file__), "--step", name, "--moments", str(args.moments), "--size", str(args.size),
               "--sample", str(args.sample), "--temperature", str(args.temperature), *extra]
    try:
        child = subprocess.run(command, capture_output=True, text=True, timeout=STEP_LIMITS[name])
    except subprocess.TimeoutExpired:
        print(f"step {name}: no result after {STEP_LIMITS[name]} s", file=sys.stderr)
        return None
    if child.returncode != 0:
        print(f"step {name}: exit status {child.returncode}\n{child.stderr[-2000:]}", file=sys.stderr)
        return None
    return json.loads(child.stdout.strip().splitlines()[-1])


out = {"lattice": f"{args.size}x{args.size}", "moments": args.moments, "temperature": args.temperature}
for name in ("map", "cut", "pairs"):
    out[name] = run_step(name)
    if out[name] is None:
        sys.exit(1)  # (nothing more is started on a GPU that has just failed a step)
    print(json.dumps({name: out[name]}), flush=True)
out["matmul"] = run_step("matmul", "--entries", str(out["map"]["entries_per_row"]))
if out["matmul"] is None:
    sys.exit(1)
print(json.dumps({"matmul": out["matmul"]}), flush=True)
out["gemm_over_matmul"] = out["map"]["gemm_TFLOPs"] / out["matmul"]["TFLOPs"]
for name in ("map", "cut"):
    rec = {"scaled_from_calls": args.sample, "map_wall_s": out[name]["wall_s_median"], "map_window_ms": out[name]["window_ms_median"]}
    for label, key, unit in (("static", "wall_s_per_call_median", "map_wall_s"), ("by_hand", "wall_s_per_call_by_hand_median", "map_wall_s"),
                             ("window", "window_ms_per_call_median", "map_window_ms")):
        per_call = out["pairs"][key]
        rec[label] = {"pairs_scaled": per_call * out[name]["sites"], "ratio": per_call * out[name]["sites"] / rec[unit],
                      "pair_calls_that_cost_one_map": rec[unit] / per_call}
    out[f"{name}_against_pairs"] = rec
print(json.dumps({k: out[k] for k in ("gemm_over_matmul", "map_against_pairs", "cut_against_pairs")}), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
