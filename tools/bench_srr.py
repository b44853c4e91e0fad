"""Times the classical reconstruction's descent update and whole reconstructions on the GPU, fused against composed.

    python tools/bench_srr.py [--sizes 128 256] [--phantoms 48 128] [--repeats 21]

* one update  out = x - alpha (grad + beta dR(x))  at N^3: ``torch.ops.nesvor.srr_step`` (csrc/srr.hip) against the torch
  expression ``NESVOR_SRR=composed`` runs (``edge_prior_gradient``), alternating, HIP events, warm, medians; the fused update's
  achieved bytes/s against the 12 B/voxel it must move (x and grad in, out back);
* ``reconstruct_volume`` (30 iterations) of three simulated stacks of an N^3 phantom (1.5 mm pixels, 3 mm slices, 1 mm
  voxels), fused against composed: what share the update has next to A and A^T.
One JSON object per line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, repeats):
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return ms


def _alternate(fns, warmup, repeats):
    """Medians (and ranges) of several callables timed in turn, so that drift hits all of them alike."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            ms[k] += _time(f, 1)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def bench_update(n, repeats, device):
    from nesvor_amd.srr import edge_prior_gradient

    g = torch.Generator().manual_seed(n)
    x = torch.rand((1, 1, n, n, n), generator=g).to(device)
    grad = torch.randn((1, 1, n, n, n), generator=g).to(device)
    alpha, delta = 0.5, 0.1
    beta = 0.02 * delta * delta

    def composed():  # the body of SRR.forward's loop after the adjoint
        gr = grad.clone()
        gr.add_(edge_prior_gradient(x, delta), alpha=beta)
        return x.sub(gr, alpha=alpha).clamp_(min=0)

    fns = {"fused": lambda: torch.ops.nesvor.srr_step(x, grad, alpha, beta, delta, True), "composed": composed,
           "clone_only": lambda: grad.clone()}  # (the composed path's copy of grad is the caller's adjoint output in the solver)
    torch.cuda.reset_peak_memory_stats(device)
    base = torch.cuda.memory_allocated(device)
    composed()
    peak_composed = torch.cuda.max_memory_allocated(device) - base
    diff = float((fns["fused"]() - composed()).abs().max())
    r = _alternate(fns, 3, repeats)
    voxels = n ** 3
    out = {"what": "update", "n": n, "repeats": repeats, **{k: v for k, v in r.items()},
           "composed_minus_clone_ms": r["composed"]["median_ms"] - r["clone_only"]["median_ms"],
           "speedup_fused_over_composed": r["composed"]["median_ms"] / r["fused"]["median_ms"],
           "fused_bytes": 12 * voxels, "fused_TBps": 12 * voxels / (r["fused"]["median_ms"] * 1e-3) / 1e12,
           "composed_peak_temporaries_bytes": peak_composed, "volume_bytes": 4 * voxels, "max_abs_diff": diff}
    print(json.dumps(out), flush=True)


def bench_reconstruction(n, repeats, device):
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.svr import reconstruct_volume
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=n), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=1.5, s_thick=3.0, normalize=False)
    k = len(slices) // 3
    stacks = [torch.stack([s.image for s in slices[j * k:(j + 1) * k]]).contiguous() for j in range(3)]
    poses = [RigidTransform.cat([s.transformation for s in slices[j * k:(j + 1) * k]]) for j in range(3)]
    shape = {}

    def run(mode):
        def f():
            if mode == "composed":
                os.environ["NESVOR_SRR"] = "composed"
            else:
                os.environ.pop("NESVOR_SRR", None)
            try:
                shape["volume"] = tuple(reconstruct_volume(stacks, None, poses, 1.5, 3.0, 1.0, n_iter=30).image.shape)
            finally:
                os.environ.pop("NESVOR_SRR", None)
        return f

    r = _alternate({"fused": run("fused"), "composed": run("composed")}, 2, repeats)
    print(json.dumps({"what": "reconstruct_volume, 30 iterations", "phantom": n, "slices": len(slices), "slice_size": int(stacks[0].shape[-1]),
                      "volume": shape["volume"], "repeats": repeats, **r,
                      "speedup_fused_over_composed": r["composed"]["median_ms"] / r["fused"]["median_ms"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--phantoms", type=int, nargs="*", default=[48, 128])
    ap.add_argument("--repeats", type=int, default=21)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_srr.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401

    device = torch.device("cuda:0")
    for n in a.sizes:
        bench_update(n, a.repeats, device)
    for n in a.phantoms:
        bench_reconstruction(n, max(a.repeats // 4, 3), device)


if __name__ == "__main__":
    main()
