"""Times the package registration (``GroupSVR``, nesvor_amd/registration.py; ``nesvor_svr_similarity_groups``, csrc/svr.hip).

    python tools/bench_packages.py [--repeats 21] [--pipeline]

* one 13-pose package gradient - 3 stacks x 40 slices of 128^2 pixels of 1.5 mm in P = 4 packages (12 groups) against a 128^3
  volume with the 153 non-zero taps of the (9,5,5) PSF - on the fused path (one ``svr_similarity_groups`` call) and on the
  composed path (``NESVOR_PACKAGES=composed``: composition in torch, gather, ``svr_similarity``, ordered adds);
  ``svr_similarity`` itself at the same shape (120 slices x 13 poses) beside them;
* one whole package stage (3 levels, 4 rounds each) on both paths, on the phantom case of tests/test_gpu_packages.py;
* ``--pipeline``: that case through ``register_slices`` with and without ``packages`` - mean simulated NCC and the error of the
  packages' relative pose per stack.
HIP events around warm calls, medians and ranges (the stage: host clock around a synchronised call - it reads results back
every iteration); one JSON object per line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _path(composed):
    if composed:
        os.environ["NESVOR_PACKAGES"] = "composed"
    else:
        os.environ.pop("NESVOR_PACKAGES", None)
    return "composed" if composed else "fused"


def bench_gradient(repeats, device):
    import torch
    from bench_acq import _poses, _time
    from nesvor_amd.registration import GroupSVR, _SliceLevel, package_groups
    from nesvor_amd.utils import get_PSF

    g = torch.Generator().manual_seed(120)
    stacks, per, hw, N, P, res = 3, 40, 128, 128, 4, 1.5
    n = stacks * per
    psf = get_PSF(res_ratio=(1.5, 1.5, 3.0)).to(device)
    base = torch.cat([_poses(per, 2.0, g) for _ in range(stacks)]).to(device)  # voxels = mm here
    lv = _SliceLevel(torch.rand((N, N, N), generator=g).to(device), torch.rand((n, hw, hw), generator=g).to(device),
                     (torch.rand((n, hw, hw), generator=g) < 0.7).to(device), psf, res, 1.0)
    groups = package_groups([per] * stacks, [P])
    gsvr = GroupSVR(num_levels=1, num_steps=1, step_size=1, max_iter=1, optimizer={"name": "gd", "momentum": 0.1}, loss={"name": "ncc"})
    gsvr._prepare(lv, base, gsvr.group_centroids(base, lv.mask, res, groups), groups)
    G = groups[0].numel() - 1
    x = torch.zeros((G, 13, 6), device=device)
    j = torch.arange(6)
    x[:, 1 + 2 * j, j], x[:, 2 + 2 * j, j] = 0.5, -0.5
    out = {}
    for composed in (False, True):
        what = _path(composed)
        fn = lambda: gsvr._group_sums(x, lv, None)
        out[what] = fn()
        print(json.dumps({"what": f"package gradient, {what}", "groups": G, "slices": n, "slice_size": hw, "volume": N, "poses": 13,
                          "taps": int((psf != 0).sum()), "repeats": repeats, "valid_share": float(out[what][:, 0, 0].sum() / lv.mask.sum()),
                          **_time(fn, 3, repeats)}), flush=True)
    _path(False)
    print(json.dumps({"what": "package gradient, fused == composed", "bit_equal": bool(torch.equal(out["fused"], out["composed"]))}), flush=True)
    tf = base[:, None].repeat(1, 13, 1, 1).contiguous()
    fn = lambda: torch.ops.nesvor.svr_similarity(lv.volume, psf, tf, lv.slices, lv.mask, res)
    print(json.dumps({"what": "svr_similarity at the same shape", "slices": n, "poses": 13, "repeats": repeats, **_time(fn, 3, repeats)}),
          flush=True)


def _stage_inputs(device):
    import torch
    import test_gpu_packages as T
    from nesvor_amd import registration as R
    from nesvor_amd.transform import RigidTransform, mat_update_resolution

    stacks, _, _ = T._package_stacks(device)
    res_s, thick = T._RES_S, T._THICK
    imgs = [R.resample(s.slices * s.mask, (res_s, res_s), (res_s, res_s)) for s in stacks]
    slices, poses, _ = R._common_frame(imgs, [s.transformation for s in stacks], res_s)
    mask = slices > 0
    keep = torch.nonzero(mask.flatten(1).any(1)).flatten()
    slices, mask = slices[keep].contiguous(), mask[keep].contiguous()
    theta = poses.axisangle()[keep].clone()
    current = RigidTransform(theta)
    shape = R._cover_shape(current, mask, res_s, thick, res_s)
    volume = R.reconstruct_from_slices(mat_update_resolution(current.matrix(), 1, res_s), slices, res_s, thick, res_s, shape)
    groups = R.package_groups([s.slices.shape[0] for s in stacks], [T._P], keep.tolist())
    return theta, groups, slices, mask, volume, {"res_s": res_s, "s_thick": thick, "res_r": res_s}


def bench_stage(repeats, device):
    import torch
    from nesvor_amd.registration import GroupSVR

    theta, groups, slices, mask, volume, params = _stage_inputs(device)
    results = {}
    for composed in (False, True):
        what = _path(composed)
        gsvr = GroupSVR(num_levels=3, num_steps=4, step_size=2, max_iter=20, optimizer={"name": "gd", "momentum": 0.1}, loss={"name": "ncc"})
        ms = []
        for r in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[what] = gsvr(theta, groups, slices, mask, volume, params, True)[0]
            torch.cuda.synchronize()
            if r:  # (the first call is the warm-up)
                ms.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"what": f"package stage, {what}", "groups": groups[0].numel() - 1, "slices": int(slices.shape[0]),
                          "slice_size": int(slices.shape[-1]), "volume": list(volume.shape[-3:]), "repeats": repeats,
                          "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}), flush=True)
    _path(False)
    print(json.dumps({"what": "package stage, fused == composed", "bit_equal": bool(torch.equal(results["fused"], results["composed"]))}),
          flush=True)


def pipeline(device):
    import test_gpu_packages as T
    from nesvor_amd import registration as R

    for packages in (None, [T._P] * 3):
        stacks, nominals, moves = T._package_stacks(device)
        t0 = time.perf_counter()
        out = R.register_slices(stacks, res_s=T._RES_S, packages=packages)
        seconds = time.perf_counter() - t0
        errors = T._relative_pose_errors(out, nominals, moves)
        print(json.dumps({"what": "register_slices, full pipeline", "packages": packages, "seconds": seconds,
                          "mean_simulated_ncc": T._simulated_ncc(out), "relative_pose_error_deg_mm": errors}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--pipeline", action="store_true")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_packages.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401

    device = torch.device("cuda:0")
    bench_gradient(a.repeats, device)
    bench_stage(max(a.repeats // 4, 3), device)
    if a.pipeline:
        pipeline(device)


if __name__ == "__main__":
    main()
