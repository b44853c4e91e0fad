"""Times the stack denoising (nesvor_amd/denoise.py) on the GPU, fused against composed.

    python tools/bench_denoise.py [--shapes 40x128x128 120x128x128] [--radii 1,3 2,5] [--repeats 21] [--stacks 3]

For each shape (slices x height x width) and each (patch radius, search radius): synthetic slices (a ramp, steps and noise of
0.05 in [0, 1]) with a 70 % mask and sigma = 0.05 on every slice.  The non-local means alone, alternating between the fused
kernel (``torch.ops.nesvor.nlm_denoise``, csrc/denoise.hip) and the torch expression in fp32 (``denoise.nlm_composed``), with
the peak device memory either takes beyond its inputs; then a whole ``denoise_stacks`` (the noise estimate included) of
``--stacks`` such stacks on both paths.  HIP events, warm, medians with ranges.  One JSON object per line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_structural import _alternate  # noqa: E402


def _composed(f):
    def g():
        os.environ["NESVOR_DENOISE"] = "composed"
        try:
            return f()
        finally:
            os.environ.pop("NESVOR_DENOISE", None)
    return g


def _synthetic(n, h, w, device):
    g = torch.Generator().manual_seed(n + h + w)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    y = 0.15 + 0.3 * xx * yy + 0.2 * (xx > 0.4) + 0.25 * (yy > 0.6) + 0.05 * torch.randn(n, 1, h, w, generator=g)
    mask = torch.rand(n, 1, h, w, generator=g) < 0.7
    return y.clamp(0, 1).contiguous().to(device), mask.to(device), torch.full((n,), 0.05, device=device)


def _peak_bytes(f):
    """Peak device memory of one call beyond what is allocated when it starts."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["40x128x128", "120x128x128"])
    ap.add_argument("--radii", type=str, nargs="+", default=["1,3", "2,5"], help="patch radius,search radius")
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--stacks", type=int, default=3, help="stacks of the denoise_stacks timing (0: skip it)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_denoise.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import denoise
    from nesvor_amd.image import Stack

    device = torch.device("cuda:0")
    os.environ.pop("NESVOR_DENOISE", None)
    for shape in a.shapes:
        n, h, w = (int(v) for v in shape.split("x"))
        y, mask, sigma = _synthetic(n, h, w, device)
        for radii in a.radii:
            P, S = (int(v) for v in radii.split(","))
            fns = {"nlm_fused": lambda: torch.ops.nesvor.nlm_denoise(y, mask, sigma, P, S, a.strength),
                   "nlm_composed": lambda: denoise.nlm_composed(y, mask, sigma, P, S, a.strength)}
            r = _alternate(fns, 2, a.repeats)
            fused, composed = fns["nlm_fused"](), fns["nlm_composed"]()
            row = {"what": "non-local means of one stack", "slices": n, "slice_shape": [h, w], "patch_radius": P, "search_radius": S,
                   "repeats": a.repeats, **r, "speedup": r["nlm_composed"]["median_ms"] / r["nlm_fused"]["median_ms"],
                   "largest_difference": float((fused[0] - composed[0]).abs().max()), "equal_bits": torch.equal(fused[0], composed[0]),
                   "peak_bytes_fused": _peak_bytes(fns["nlm_fused"]), "peak_bytes_composed": _peak_bytes(fns["nlm_composed"]),
                   "stack_bytes": 4 * n * h * w}
            del fused, composed
            if a.stacks > 0:
                def run():
                    stacks = [Stack(y, mask) for _ in range(a.stacks)]  # (denoise_stacks replaces st.slices: y itself is never written)
                    return denoise.denoise_stacks(stacks, P, S, a.strength)

                r2 = _alternate({"stacks_fused": run, "stacks_composed": _composed(run)}, 1, max(3, a.repeats // 3))
                row.update(stacks=a.stacks, **r2, speedup_stacks=r2["stacks_composed"]["median_ms"] / r2["stacks_fused"]["median_ms"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
