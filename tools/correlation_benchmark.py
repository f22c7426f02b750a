#!/usr/bin/env python3
"""Rate of the Gram product of correlation() on the 64x64 README model against torch.matmul of two complex128 panels
of the same shape (profiles/correlation.json).  Needs a GPU.

    python3 tools/correlation_benchmark.py [--out profiles/correlation.json] [--moments 256,512] [--vectors 64] [--size 64]

A = B = current_operator(axis 0), 64 random-phase vectors.  Per M: median of five calls after a warm-up of the wall
time, of the HIP-event window of the call, of gram_ms (the corr_gram + corr_reduce launches) and of gram_flops /
gram_ms, and the share of the window spent outside the Gram launches (the two recurrences, the operator kernel, the
copies into the panels).  The yardstick is torch.matmul(conj(X), Y^T) for two complex128 tensors of the panel shape
(rows of a panel x K) on the same GPU under HIP-event timing (torch.cuda.Event), counted with the same 8 flops per
complex multiply-add: the kernel guide gives no fp64-matrix peak to compare with.  The yardstick runs in a child
process of its own (`--yardstick ROWS,ENTRIES`): torch brings its own HIP runtime, which finds no device in a process
where the library's has already opened it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time


def readme_swave(L):
    system = ba.Hamiltonian(ba.CubicLattice((L, L, 1)))
    with system as (H, D):
        H.set_sites(3.0 * ba.σ0 - 0.05 * ba.σ3)
        D.set_sites(-0.1 * ba.jσ2)
        H.set_bonds(-1.0 * ba.σ0)
    return system


def matmul_yardstick(rows, entries, repeats=5):
    """TFLOP/s of torch.matmul on (rows, entries) complex128 panels: median of `repeats` after a warm-up."""
    import torch

    device = torch.device("cuda")
    generator = torch.Generator(device=device).manual_seed(0)
    x = torch.randn(rows, entries, 2, dtype=torch.float64, device=device, generator=generator)
    y = torch.randn(rows, entries, 2, dtype=torch.float64, device=device, generator=generator)
    x, y = torch.view_as_complex(x), torch.view_as_complex(y)
    times = []
    for _ in range(repeats + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = torch.matmul(x.conj(), y.T)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    del x, y, out
    torch.cuda.empty_cache()
    ms = statistics.median(times[1:])
    return {"rows": rows, "entries": entries, "ms": times[1:], "ms_median": ms, "TFLOPs": 8.0 * rows * rows * entries / ms / 1e9}


ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--moments", default="256,512")
ap.add_argument("--vectors", type=int, default=64)
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--no-yardstick", action="store_true")
ap.add_argument("--yardstick", metavar="ROWS,ENTRIES", help="only time torch.matmul on panels of this shape and print the record")
args = ap.parse_args()
if args.yardstick:
    rows, entries = (int(v) for v in args.yardstick.split(","))
    print(json.dumps(matmul_yardstick(rows, entries)), flush=True)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bodge_amd as ba
from bodge_amd import backend
from bodge_amd import correlation as corr
from bodge_amd.observables import _scale_of


def yardstick_in_child(rows, entries):
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardstick", f"{rows},{entries}"],
                           capture_output=True, text=True, timeout=300)
    if child.returncode != 0:
        return {"rows": rows, "entries": entries, "error": child.stderr.strip().splitlines()[-1:] or ["failed"]}
    return json.loads(child.stdout.strip().splitlines()[-1])


system = readme_swave(args.size)
solver = system._solver()
scale = _scale_of(system)
jx = corr.as_operator(system, corr.current_operator(system, 0))
x = corr.random_phase_vectors(system, args.vectors, seed=0)
solver.moment_matrix(scale, 8, jx, jx, x=x)  # warm-up (tables, kernel load)
out = {"lattice": f"{args.size}x{args.size}", "vectors": args.vectors, "scale": scale}
for M in (int(v) for v in args.moments.split(",")):
    runs = []
    for _ in range(6):
        t0 = time.time()
        solver.moment_matrix(scale, M, jx, jx, x=x)
        p = solver.perf()
        runs.append({"wall_s": time.time() - t0, "window_ms": p["window_ms"], "gram_ms": p["gram_ms"],
                     "TFLOPs": p["gram_flops"] / p["gram_ms"] / 1e9})
    runs = runs[1:]
    entries = 4 * system.lattice.size * p["lanes_per_row"]
    # rows of a panel by the rule of the library: M, or the largest multiple of 64 for which two panels stay within 4 GiB
    budget = int(backend.get_option("BODGE_AMD_CORRELATION_BYTES") or os.environ.get("BODGE_AMD_CORRELATION_BYTES") or 4 << 30)
    panel_rows = M if 2 * M * entries * 16 <= budget else budget // (2 * entries * 16) // 64 * 64
    rec = {"moments": M, "lanes_per_row": p["lanes_per_row"], "real": p["real_arithmetic"], "ph": p["ph_packed"],
           "dict_blocks": p["dict_blocks"], "launches": p["launches"], "vector_steps": p["vector_steps"],
           "entries_per_row": entries, "panel_rows": panel_rows, "gram_flops": p["gram_flops"],
           "wall_s": [r["wall_s"] for r in runs], "window_ms": [r["window_ms"] for r in runs],
           "gram_ms": [r["gram_ms"] for r in runs],
           "wall_s_median": statistics.median(r["wall_s"] for r in runs),
           "window_ms_median": statistics.median(r["window_ms"] for r in runs),
           "gram_ms_median": statistics.median(r["gram_ms"] for r in runs),
           "gram_TFLOPs": statistics.median(r["TFLOPs"] for r in runs)}
    rec["share_outside_gram"] = 1.0 - rec["gram_ms_median"] / rec["window_ms_median"]
    if not args.no_yardstick:
        rec["torch_matmul"] = yardstick_in_child(panel_rows, entries)
        if "TFLOPs" in rec["torch_matmul"]:
            rec["gram_over_matmul"] = rec["gram_TFLOPs"] / rec["torch_matmul"]["TFLOPs"]
    out[f"M={M}"] = rec
    print(json.dumps({f"M={M}": rec}), flush=True)
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
