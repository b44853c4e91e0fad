"""Times the volume comparison (nesvor_amd/evaluate.py) on the GPU, fused against composed.

    python tools/bench_evaluate.py [--sizes 128 256] [--repeats 11]

For each size n: the n^3 phantom on a 1 mm lattice as the reference, and a copy of it on a 0.8 mm lattice tilted by 10 degrees
about (1,2,3) (``Volume.resample``) as the volume under test.  The resampling with its first sums alone, the 3-D SSIM with its
second sums alone, and a whole ``compare_volumes`` (both passes, the fit between them and the report's host read), alternating
between the fused kernels (``torch.ops.nesvor.volume_resample`` / ``volume_ssim``, csrc/evaluate.hip) and the torch expressions
(``NESVOR_EVALUATE=composed``).  HIP events, warm, medians with ranges.  One JSON object per line.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _alternate(fns, warmup, repeats):
    """Medians (and ranges) of several callables timed in turn, so that drift hits all of them alike."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def _composed(f):
    def g():
        os.environ["NESVOR_EVALUATE"] = "composed"
        try:
            return f()
        finally:
            os.environ.pop("NESVOR_EVALUATE", None)
    return g


def _rotation(degrees, axis):
    k = torch.tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    a = math.radians(degrees)
    return torch.eye(3, dtype=torch.float64) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def _pair(size, device):
    from nesvor_amd.image import Volume
    from nesvor_amd.phantom import phantom3d
    from nesvor_amd.transform import RigidTransform

    image = torch.tensor(phantom3d(n=size), dtype=torch.float32, device=device).clamp(min=0)
    identity = torch.eye(3, 4, dtype=torch.float32, device=device)[None]
    reference = Volume(image, image > 0, RigidTransform(identity, trans_first=True), 1.0, 1.0, 1.0)
    tilt = torch.cat([_rotation(10.0, (1.0, 2.0, 3.0)).float(), torch.zeros(3, 1)], 1)[None].to(device)
    volume = reference.resample(0.8, RigidTransform(tilt, trans_first=True))
    # (the command keeps the poses on the host: so does this)
    for v in (reference, volume):
        v.transformation = RigidTransform(v.transformation.matrix(True).cpu(), trans_first=True)
    return reference, volume


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--repeats", type=int, default=11)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import evaluate

    device = torch.device("cuda:0")
    os.environ.pop("NESVOR_EVALUATE", None)
    for size in a.sizes:
        reference, volume = _pair(size, device)
        M = evaluate.index_map(reference, volume)
        flat = M.reshape(12).tolist()
        i0, mr, x0, mx = reference.image.contiguous(), reference.mask.contiguous(), volume.image.contiguous(), volume.mask.contiguous()
        j0, valid, first = torch.ops.nesvor.volume_resample(i0, mr, x0, mx, flat)
        _, a_fit, b_fit, L = evaluate.fit_from_sums(first, "scale", None)
        params = torch.stack([a_fit, b_fit, (0.01 * L) ** 2, (0.03 * L) ** 2]).float()
        fns = {"resample_fused": lambda: torch.ops.nesvor.volume_resample(i0, mr, x0, mx, flat),
               "resample_composed": lambda: evaluate.resample_composed(i0, mr, x0, mx, M),
               "ssim_fused": lambda: torch.ops.nesvor.volume_ssim(i0, j0, valid, params),
               "ssim_composed": lambda: evaluate.ssim3d_composed(i0, j0, valid, params),
               "compare_fused": lambda: evaluate.compare_volumes(reference, volume),
               "compare_composed": _composed(lambda: evaluate.compare_volumes(reference, volume))}
        r = _alternate(fns, 2, a.repeats)
        report = evaluate.compare_volumes(reference, volume)
        voxels = i0.numel()
        print(json.dumps({"what": "volume comparison", "reference_shape": list(i0.shape), "volume_shape": list(x0.shape), "repeats": a.repeats,
                          **r, **{f"speedup_{k}": r[f"{k}_composed"]["median_ms"] / r[f"{k}_fused"]["median_ms"]
                                  for k in ("resample", "ssim", "compare")},
                          # reads I0, J0 (4 bytes) and v (1 byte) once, writes the map (4 bytes): the least the pass can move
                          "ssim_fused_min_bytes": 13 * voxels,
                          "ssim_fused_TBps_of_min_bytes": 13 * voxels / (r["ssim_fused"]["median_ms"] * 1e-3) / 1e12,
                          "report": {k: report[k] for k in evaluate.METRICS}}), flush=True)


if __name__ == "__main__":
    main()
