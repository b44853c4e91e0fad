"""Times the slice bias fields (nesvor_amd/slice_bias.py) on the GPU, fused against composed.

    python tools/bench_slice_bias.py [--shapes 55x59x59 120x128x128] [--sigma-mm 12] [--repeats 21] [--phantom 48] [--n-iter 30]

For each shape (slices x height x width): synthetic slices (sim in [0.02, 0.9), a rough field, a 70 % mask, random weights),
pixel size 1.5 mm.  ``SliceBias.update`` on them, alternating between the fused kernel (``torch.ops.nesvor.slice_bias_update``,
csrc/slice_bias.hip) and the torch expression (``NESVOR_SLICE_BIAS=composed``); also b_new and the sums alone on both paths (the
rest of an update is a few operations on n-vectors and one subtraction).  Then a whole ``svr.reconstruct_volume`` on the
phantom's three still stacks: plain, with the fields on the fused path and with them on the composed path.  HIP events, warm,
medians with ranges.  One JSON object per line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_structural import RES_R, RES_S, THICK, _alternate, _stacks  # noqa: E402


def _composed(f):
    def g():
        os.environ["NESVOR_SLICE_BIAS"] = "composed"
        try:
            return f()
        finally:
            os.environ.pop("NESVOR_SLICE_BIAS", None)
    return g


def _synthetic(n, h, w, device):
    g = torch.Generator().manual_seed(n + h + w)
    sim = 0.02 + 0.88 * torch.rand(n, 1, h, w, generator=g)
    scale = 0.8 + 0.4 * torch.rand(n, generator=g)
    y = sim * torch.exp(0.2 * torch.randn(n, 1, h, w, generator=g)) / scale.view(n, 1, 1, 1)
    mask = torch.rand(n, 1, h, w, generator=g) < 0.7
    weight = torch.rand(n, 1, h, w, generator=g)
    return tuple(t.to(device) for t in (sim, y, mask, scale, weight))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["55x59x59", "120x128x128"])
    ap.add_argument("--sigma-mm", type=float, default=12.0)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--phantom", type=int, default=48, help="phantom size of the reconstruct_volume timing (0: skip it)")
    ap.add_argument("--n-iter", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_slice_bias.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import slice_bias, svr

    device = torch.device("cuda:0")
    os.environ.pop("NESVOR_SLICE_BIAS", None)
    sigma_px = a.sigma_mm / RES_S
    for shape in a.shapes:
        n, h, w = (int(v) for v in shape.split("x"))
        sim, y, mask, scale, weight = _synthetic(n, h, w, device)
        b = torch.zeros_like(sim)
        state = slice_bias.SliceBias(a.sigma_mm)

        def update():
            state.b = None  # (every timed update is a first round)
            state.update(sim, y, mask, scale, weight, RES_S)

        fns = {"update_fused": update, "update_composed": _composed(update),
               "field_fused": lambda: torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, weight, b, sigma_px, 0.05),
               "field_composed": lambda: slice_bias.field_composed(sim, y, mask, scale, weight, b, sigma_px, 0.05)}
        r = _alternate(fns, 3, a.repeats)
        print(json.dumps({"what": "one slice bias update", "slices": n, "slice_shape": [h, w], "sigma_px": sigma_px,
                          "radius": slice_bias.window_radius(sigma_px), "repeats": a.repeats, **r,
                          "speedup_update": r["update_composed"]["median_ms"] / r["update_fused"]["median_ms"],
                          "speedup_field": r["field_composed"]["median_ms"] / r["field_fused"]["median_ms"]}), flush=True)
    if a.phantom > 0:
        stacks, poses = _stacks(a.phantom, device)
        run = lambda **k: svr.reconstruct_volume(stacks, None, poses, RES_S, THICK, RES_R, n_iter=a.n_iter, **k)
        fns = {"plain": run, "slice_bias_fused": lambda: run(slice_bias=slice_bias.SliceBias(a.sigma_mm)),
               "slice_bias_composed": _composed(lambda: run(slice_bias=slice_bias.SliceBias(a.sigma_mm)))}
        repeats = max(3, a.repeats // 3)
        r = _alternate(fns, 1, repeats)
        print(json.dumps({"what": "reconstruct_volume", "phantom": a.phantom, "n_iter": a.n_iter, "repeats": repeats, **r,
                          "slice_bias_fused_over_plain": r["slice_bias_fused"]["median_ms"] / r["plain"]["median_ms"],
                          "slice_bias_composed_over_fused": r["slice_bias_composed"]["median_ms"] / r["slice_bias_fused"]["median_ms"]}),
              flush=True)


if __name__ == "__main__":
    main()
