"""Times the structural exclusion (nesvor_amd/structural.py) on the GPU, fused against composed.

    python tools/bench_structural.py [--sizes 48 128] [--repeats 21] [--n-iter 30]

For each phantom size: three still stacks (1.5 mm pixels, 3 mm slices, normalised by their 0.99 quantile), sim = A x of the
equalised back-projection.  ``StructuralExclusion.update`` on them, alternating between the fused kernel
(``torch.ops.nesvor.structural_ssim``, csrc/structural.hip) and the torch expression (``NESVOR_STRUCTURAL=composed``); also the
map and the sums alone on both paths (the rest of an update is a few operations on n-vectors and two comparisons); then a
whole ``svr.reconstruct_volume`` plain, with the switch on the fused path and with it on the composed path.  HIP events, warm,
medians with ranges.  One JSON object per line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RES_S, THICK, RES_R = 1.5, 3.0, 1.0


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


def _stacks(size, device):
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=size), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=RES_S, s_thick=THICK, motion_deg=0, motion_mm=0, seed=0, normalize=False)
    allv = torch.cat([s.image[s.mask] for s in slices])
    q = torch.kthvalue(allv, max(int(0.99 * allv.numel()), 1)).values
    n = len(slices) // 3
    stacks = [(torch.stack([s.image for s in slices[j * n:(j + 1) * n]]) / q).contiguous() for j in range(3)]
    poses = [RigidTransform.cat([s.transformation for s in slices[j * n:(j + 1) * n]]) for j in range(3)]
    return stacks, poses


def _composed(f):
    def g():
        os.environ["NESVOR_STRUCTURAL"] = "composed"
        try:
            return f()
        finally:
            os.environ.pop("NESVOR_STRUCTURAL", None)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[48, 128])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--n-iter", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_structural.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import structural, svr
    from nesvor_amd.srr import PSFreconstruction

    device = torch.device("cuda:0")
    os.environ.pop("NESVOR_STRUCTURAL", None)
    for size in a.sizes:
        stacks, poses = _stacks(size, device)
        images, m, frame_poses, _ = svr._frame_keep(stacks, None, poses, RES_S)
        shape = svr._cover_shape(frame_poses, m, RES_S, THICK, RES_R)
        op, params = svr._operator(images, m, frame_poses, RES_S, THICK, RES_R, shape)
        sim = op.forward(PSFreconstruction(op.transforms, images, m, None, params)).contiguous()
        scale = torch.ones(images.shape[0], device=device)
        state = structural.StructuralExclusion()
        fns = {"update_fused": lambda: state.update(sim, images, m), "update_composed": _composed(lambda: state.update(sim, images, m)),
               "ssim_fused": lambda: torch.ops.nesvor.structural_ssim(sim, images, m, scale, 0.4, 1.0),
               "ssim_composed": lambda: structural.ssim_composed(sim, images, m, scale, 0.4, 1.0)}
        r = _alternate(fns, 3, a.repeats)
        pixels = images.numel()
        print(json.dumps({"what": "one structural update", "phantom": size, "slices": int(images.shape[0]),
                          "slice_shape": list(images.shape[-2:]), "repeats": a.repeats, **r,
                          "speedup_update": r["update_composed"]["median_ms"] / r["update_fused"]["median_ms"],
                          "speedup_ssim": r["ssim_composed"]["median_ms"] / r["ssim_fused"]["median_ms"],
                          "ssim_fused_bytes": 13 * pixels,
                          "ssim_fused_TBps": 13 * pixels / (r["ssim_fused"]["median_ms"] * 1e-3) / 1e12}), flush=True)
        run = lambda **k: svr.reconstruct_volume(stacks, None, poses, RES_S, THICK, RES_R, n_iter=a.n_iter, **k)
        fns = {"plain": run, "structural_fused": lambda: run(structural=structural.StructuralExclusion()),
               "structural_composed": _composed(lambda: run(structural=structural.StructuralExclusion()))}
        r = _alternate(fns, 1, max(3, a.repeats // 3))
        print(json.dumps({"what": "reconstruct_volume", "phantom": size, "n_iter": a.n_iter, "repeats": max(3, a.repeats // 3), **r,
                          "structural_fused_over_plain": r["structural_fused"]["median_ms"] / r["plain"]["median_ms"],
                          "structural_composed_over_fused": r["structural_composed"]["median_ms"] / r["structural_fused"]["median_ms"]}),
              flush=True)


if __name__ == "__main__":
    main()
