"""Times the joint-histogram entry point of the stack registration's mutual-information similarity (csrc/vvr_nmi.hip, nesvor_amd/nmi.py)
against the composed path (``vvr_sample`` + ``nmi.joint_histogram``), the sampling alone and the moment sums of csrc/vvr.hip on the
same pyramid level, and ``register_stacks`` with ``nmi`` against ``ncc``.

    python tools/bench_vvr_nmi.py [--repeats 21] [--skip-pipeline]

Levels (``VVR._level(0, ...)``, the finest): a pair of stacks of 40 slices of 128^2 pixels (1.5 mm in-plane, 3 mm slices: 80 x 128 x
128 voxels) cut from the 128^3 phantom - piecewise constant, so most points hit a handful of cells, the worst case for same-address
LDS atomics - and the same shape filled with a smooth random volume, whose points spread over the histogram; and the 64^3 phantom
pair of the tests (32 slices of 64^2, 1 mm, 2 mm slices).  Arms, alternating inside every repeat, for the 13 poses of a gradient and
for K = 1 (the accept test): ``nesvor_vvr_similarity``; ``vvr_joint_histogram`` at 32 and 64 bins; ``vvr_sample`` alone; the composed
path at 32 bins, whose result must equal the kernel's.  Then the whole ``register_stacks`` on the two-stack 64^3 case, host clock
around a device synchronise.  HIP events, warm, medians and ranges; one JSON object per line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--skip-pipeline", action="store_true")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_vvr_nmi.py measures on the GPU: no HIP device found")
    from bench_psf_bank import _alternate, _stats
    from nesvor_amd import _lib, nmi
    from nesvor_amd import ops  # noqa: F401  (registers torch.ops.nesvor)
    from nesvor_amd.phantom import phantom3d
    from nesvor_amd.registration import VVR
    from nesvor_amd.transform import RigidTransform

    device = torch.device("cuda:0")
    g = torch.Generator().manual_seed(130)
    big = torch.tensor(phantom3d(n=128), dtype=torch.float32)[4:124:3]  # 40 slices of 128^2
    smooth = torch.nn.functional.avg_pool3d(torch.rand(1, 1, 44, 132, 132, generator=g), 5, 1)[0, 0] + 0.1
    small = torch.tensor(phantom3d(n=64), dtype=torch.float32)[::2]
    levels = {"phantom 40 x 128^2": (big, 1.5, 3.0), "smooth random 40 x 128^2": (smooth, 1.5, 3.0), "phantom 32 x 64^2": (small, 1.0, 2.0)}
    theta_t = RigidTransform(torch.tensor([[0.2, -0.1, 0.3, 4.0, -3.0, 2.0]], device=device), trans_first=False)
    cur = theta_t.axisangle(trans_first=False) / VVR._unit(torch.zeros(1, 6, device=device)) + torch.tensor([[1.0, 0.5, -1.0, 0.8, -0.6, 0.4]], device=device)
    e = torch.zeros((13, 6), device=device)
    j = torch.arange(6, device=device)
    e[1 + 2 * j, j], e[2 + 2 * j, j] = 0.25, -0.25
    for what, (vol, res_s, s_thick) in levels.items():
        vol = vol.to(device)[None, None].contiguous()
        vvr = VVR(3, 4, 2, 20, {"name": "gd", "momentum": 0.1}, {"name": "nmi"}, False)
        vvr.theta_t, vvr.trans_first = theta_t, False
        res = [s_thick, res_s, res_s]
        vvr.res = min(res)
        vvr.relative_res = [r / vvr.res for r in res]
        lv = vvr._level(0, vol, vol)
        src, unit = lv.source.contiguous(), list(lv.to_unit_host)
        D, H, W = src.shape[-3:]
        M = lv.values.numel()
        J = lv.values.view(1, -1)
        for K in (13, 1):
            thetas = (cur + e)[:K]
            mats = RigidTransform(thetas * vvr._unit(thetas), trans_first=False).inv().compose(theta_t).matrix().contiguous()
            maps = {b: (tuple(nmi.axis_map(src.min(), src.max(), b).tolist()), tuple(nmi.axis_map(lv.values.min(), lv.values.max(), b).tolist()))
                    for b in (32, 64)}
            sums = torch.empty((K, 3), dtype=torch.float64, device=device)

            def moments():
                _lib.check(_lib.load().nesvor_vvr_similarity(_lib.ptr(src), D, H, W, _lib.ptr(lv.points), _lib.ptr(lv.values), _lib.ptr(mats),
                                                             lv.to_unit_host, M, K, _lib.ptr(sums), None, _lib.stream_ptr()), "vvr similarity")

            def hist(b):
                return torch.ops.nesvor.vvr_joint_histogram(src, lv.points, lv.values, mats, unit, *maps[b][0], *maps[b][1], b)

            def composed(b):
                I = torch.ops.nesvor.vvr_sample(src, lv.points, mats, unit)
                rows = torch.tensor(maps[b][1], dtype=torch.float32, device=device).view(1, 2).expand(K, 2)
                Jk = J.expand(K, -1)
                return nmi.joint_histogram(I, Jk, torch.ones_like(Jk, dtype=torch.bool), maps[b][0], rows, b)

            assert torch.equal(hist(32), composed(32)), "the kernel's histogram differs from the composed definition"
            h = hist(32)[0].double()
            top = float(h.flatten().topk(4).values.sum() / h.sum())  # how concentrated the histogram is: the share of its four fullest cells
            arms = {"vvr_similarity": moments, "joint_histogram_32": lambda: hist(32), "joint_histogram_64": lambda: hist(64),
                    "vvr_sample": lambda: torch.ops.nesvor.vvr_sample(src, lv.points, mats, unit), "composed_32": lambda: composed(32)}
            ms = _alternate(arms, 3, a.repeats)
            print(json.dumps({"what": what, "K": K, "points": M, "source": [D, H, W], "share_of_four_fullest_cells": round(top, 3),
                              "repeats": a.repeats, **{k: _stats(v) for k, v in ms.items()}}), flush=True)

    if a.skip_pipeline:
        return
    from nesvor_amd.image import Stack
    from nesvor_amd.registration import register_stacks

    def stacks():
        sl = small.to(device)[:, None].contiguous()
        n = sl.shape[0]

        def poses(offset):
            t = torch.zeros((n, 6), dtype=torch.float32, device=device)
            t[:, -1] = (torch.arange(n, dtype=torch.float32, device=device) - (n - 1) / 2) * 2.0
            return offset.compose(RigidTransform(t))

        off = RigidTransform(torch.tensor([[math.radians(4.0), 0.0, math.radians(-2.0), 3.0, -2.0, 1.0]], device=device))
        return [Stack(sl.clone(), sl > 0, poses(RigidTransform(torch.zeros((1, 6), device=device))), resolution_x=1.0, resolution_y=1.0,
                      thickness=2.0, gap=2.0),
                Stack((4 * sl * (1 - sl)).contiguous(), sl > 0, poses(off), resolution_x=1.0, resolution_y=1.0, thickness=2.0, gap=2.0)]

    out = {"what": "register_stacks, two 32 x 64^2 stacks, the second remapped by 4 J (1 - J)", "runs": 3}
    for similarity in ("ncc", "nmi"):
        register_stacks(stacks(), similarity=similarity)  # warm
        secs = []
        for _ in range(3):
            st = stacks()
            torch.cuda.synchronize()
            t0 = time.time()
            done = register_stacks(st, similarity=similarity)
            torch.cuda.synchronize()
            secs.append(time.time() - t0)
        m0, m1 = done[0].transformation.matrix(), done[1].transformation.matrix()
        out[similarity] = {"median_s": round(statistics.median(secs), 3), "min_s": round(min(secs), 3), "max_s": round(max(secs), 3),
                           "translation_difference_mm": round(float((m0[:, :, 3] - m1[:, :, 3]).abs().max()), 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
