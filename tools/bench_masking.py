"""Times the stack masking (nesvor_amd/masking.py) on the GPU, fused against composed.

    python tools/bench_masking.py [--stacks 3] [--slices 40] [--size 128] [--repeats 21]

One ``mask_stacks`` call with ``--stacks-intersection`` and one with ``--otsu-thresholding`` on stacks x slices of size^2 pixels
(three oblique stacks around one centre, 1 mm pixels, 3 mm slices), alternating between the fused ops
(``torch.ops.nesvor.stack_mask / otsu_histogram / otsu_threshold``, csrc/masking.hip) and the float64 torch expressions
(``NESVOR_MASKING=composed``).  HIP events, warm, medians with ranges.  Also the device memory either path takes during one call:
the peak above the inputs and the total it allocates.  One JSON object per line.
"""
import argparse
import json
import logging
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


def _memory(f):
    """(peak bytes above what was allocated before the call, bytes allocated during the call) of one call of f."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_stats()
    f()
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats()
    return (after["allocated_bytes.all.peak"] - before["allocated_bytes.all.current"],
            after["allocated_bytes.all.allocated"] - before["allocated_bytes.all.allocated"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=3)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=21)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_masking.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import masking
    from nesvor_amd.image import Stack
    from nesvor_amd.phantom import stack_transforms
    from nesvor_amd.transform import RigidTransform

    # near-orthogonal stacks, rotated a little off the axes so that no voxel sits on a slab face
    angles = [[0.1, 0.1, 0.1], [1.5, 0.05, -0.07], [0.06, 1.6, 0.09]]

    device = torch.device("cuda:0")
    n, s = a.slices, a.size
    g = torch.Generator().manual_seed(n * s)
    images, poses = [], []
    for j in range(a.stacks):
        images.append(((1 + 0.5 * torch.randn(n, 1, s, s, generator=g)).abs() + 0.1).to(device))
        poses.append(stack_transforms([x + 0.01 * (j // 3) for x in angles[j % 3]], n, 3.0, device).matrix(True).contiguous())

    def whole(mode, **kw):
        def f():
            stacks = [Stack(img, img > 0, RigidTransform(T, trans_first=True), resolution_x=1.0, resolution_y=1.0, thickness=3.0, gap=3.0)
                      for img, T in zip(images, poses)]  # (fresh masks every call: mask_stacks narrows them)
            if mode == "composed":
                os.environ["NESVOR_MASKING"] = "composed"
            try:
                return stacks, masking.mask_stacks(stacks, **kw)
            finally:
                os.environ.pop("NESVOR_MASKING", None)
        return f

    os.environ.pop("NESVOR_MASKING", None)
    logging.disable(logging.INFO)  # (the per-stack report lines are not what is timed)
    fns = {"intersection_fused": whole("fused", stacks_intersection=True), "intersection_composed": whole("composed", stacks_intersection=True),
           "otsu_fused": whole("fused", otsu_thresholding=True), "otsu_composed": whole("composed", otsu_thresholding=True)}
    r = _alternate(fns, 3, a.repeats)
    memory = {k: dict(zip(("peak_temporary_bytes", "allocated_bytes"), _memory(f))) for k, f in fns.items()}
    same = {}
    for what in ("intersection", "otsu"):
        (sf, rf), (sc, rc) = fns[f"{what}_fused"](), fns[f"{what}_composed"]()
        same[what] = {"differing_voxels": [int((x.mask != y.mask).sum()) for x, y in zip(sf, sc)],
                      "kept_share": [x["kept_share"] for x in rf], "otsu_threshold": [x["otsu_threshold"] for x in rf],
                      "otsu_threshold_composed": [x["otsu_threshold"] for x in rc]}
    print(json.dumps({"what": "mask_stacks", "stacks": a.stacks, "slices": n, "size": s, "repeats": a.repeats, **r,
                      "speedup_intersection": r["intersection_composed"]["median_ms"] / r["intersection_fused"]["median_ms"],
                      "speedup_otsu": r["otsu_composed"]["median_ms"] / r["otsu_fused"]["median_ms"],
                      "memory": memory, "results": same}), flush=True)


if __name__ == "__main__":
    main()
