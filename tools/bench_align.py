"""Times the multi-pose moments of the rigid alignment (nesvor_amd/align.py) on the GPU.

    python tools/bench_align.py [--sizes 128 256] [--repeats 11] [--align-size 128] [--align-repeats 3]

For each size n: the pair of tools/bench_evaluate.py (the n^3 phantom on a 1 mm lattice, and its copy on a 0.8 mm lattice tilted
by 10 degrees about (1,2,3)).  One step's 12 poses - theta = 0 moved by +-1 (degree, mm) along each of the six parameters - three
ways, in turn: the fused call (``torch.ops.nesvor.volume_pose_moments``, one pass over the reference), 12 launches of
``torch.ops.nesvor.volume_resample`` (what the sums cost before the kernel existed: two volume-sized outputs per pose), and the
composed torch expression (``align.pose_moments_composed``).  Then, at ``--align-size``, a whole ``align_volumes`` of the copy
moved by 5 degrees and (2, -1, 1.5) mm, fused against ``NESVOR_EVALUATE=composed``.  HIP events, warm, medians with ranges.  One
JSON object per line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_evaluate import _alternate, _composed, _pair, _rotation  # noqa: E402


def _moved(volume, degrees, axis, shift):
    """``volume`` with the pose G o T_X, G: p -> Q p + q (host matrices, world = R (p + t))."""
    from nesvor_amd.image import Volume
    from nesvor_amd.transform import RigidTransform

    mat = volume.transformation.matrix(True)[0].double().cpu()
    R = _rotation(degrees, axis) @ mat[:, :3]
    t = mat[:, 3] + R.t() @ torch.tensor(shift, dtype=torch.float64)
    return Volume(volume.image, volume.mask, RigidTransform(torch.cat([R, t[:, None]], 1)[None], trans_first=True),
                  volume.resolution_x, volume.resolution_y, volume.resolution_z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--align-size", type=int, default=128)
    ap.add_argument("--align-repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import align

    device = torch.device("cuda:0")
    os.environ.pop("NESVOR_EVALUATE", None)
    for size in a.sizes:
        reference, volume = _pair(size, device)
        thetas = [[sign * (j == k) for j in range(6)] for k in range(6) for sign in (1.0, -1.0)]
        maps = align.pose_maps(reference, volume, thetas, align.centroid(reference))
        flat, each = maps.reshape(-1).tolist(), [m.reshape(12).tolist() for m in maps]
        i0, mr, x0, mx = reference.image.contiguous(), reference.mask.contiguous(), volume.image.contiguous(), volume.mask.contiguous()
        fns = {"fused": lambda: torch.ops.nesvor.volume_pose_moments(i0, mr, x0, mx, flat),
               "resample_x12": lambda: [torch.ops.nesvor.volume_resample(i0, mr, x0, mx, m)[2] for m in each],
               "composed": lambda: align.pose_moments_composed(i0, mr, x0, mx, maps)}
        r = _alternate(fns, 2, a.repeats)
        sums = fns["fused"]()
        same_n = bool((sums[:, 0] == torch.stack(fns["resample_x12"]())[:, 0]).all())
        voxels = i0.numel()
        print(json.dumps({"what": "moments of 12 poses", "reference_shape": list(i0.shape), "volume_shape": list(x0.shape), "repeats": a.repeats,
                          **r, "speedup_over_resample_x12": r["resample_x12"]["median_ms"] / r["fused"]["median_ms"],
                          "speedup_over_composed": r["composed"]["median_ms"] / r["fused"]["median_ms"],
                          "fused_ns_per_voxel_and_pose": r["fused"]["median_ms"] * 1e6 / (12 * voxels),
                          "valid_fraction_of_pose_0": float(sums[0, 0]) / voxels, "counts_equal_the_resamplers": same_n}), flush=True)
    reference, volume = _pair(a.align_size, device)
    moved = _moved(volume, 5.0, (3.0, 1.0, 2.0), (2.0, -1.0, 1.5))
    fns = {"align_fused": lambda: align.align_volumes(reference, moved), "align_composed": _composed(lambda: align.align_volumes(reference, moved))}
    r = _alternate(fns, 1, a.align_repeats)
    out = align.align_volumes(reference, moved)
    print(json.dumps({"what": "align_volumes, rigid", "reference_shape": list(reference.image.shape), "volume_shape": list(moved.image.shape),
                      "repeats": a.align_repeats, **r, "speedup": r["align_composed"]["median_ms"] / r["align_fused"]["median_ms"],
                      "evaluations": out["evaluations"], "levels": out["levels"], "rotation_deg": out["rotation_deg"],
                      "translation_mm": out["translation_mm"], "ncc_before": out["ncc_before"], "ncc_after": out["ncc_after"],
                      "accepted": out["accepted"]}), flush=True)


if __name__ == "__main__":
    main()
