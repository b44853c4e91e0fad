"""Times the bias field correction (nesvor_amd/bias.py) on the GPU, fused against composed.

    python tools/bench_bias.py [--slices 40] [--size 128] [--repeats 21] [--whole-repeats 3]

On one stack of slices x size^2 voxels (a disc mask of about 70 %, a smooth field on noisy tissue classes): ONE iteration
(histogram + sharpening + fit + update) at S = 1 and S = 8 spans per axis, alternating between the fused ops
(``torch.ops.nesvor.n4_histogram / n4_fit / n4_update_``, csrc/bias.hip) and the float64 torch expressions; the three ops, the
sharpening (float64 torch on n_bins-sized arrays, shared by both paths) and the stop test's host read alone; and a whole
default correction on either path.  HIP events, warm, medians.  One JSON object per line.
"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--whole-repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bias.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import bias

    device = torch.device("cuda:0")
    n, s = a.slices, a.size
    g = torch.Generator().manual_seed(n * s)
    zz, yy, xx = torch.meshgrid(torch.linspace(-1, 1, n), torch.linspace(-1, 1, s), torch.linspace(-1, 1, s), indexing="ij")
    disc = (yy ** 2 + xx ** 2 < 0.94 ** 2)
    tissue = 0.2 + 0.1 * ((yy ** 2 + xx ** 2 < 0.5 ** 2).float() + (xx.abs() < 0.2).float())  # three classes
    img = tissue * (1 + 0.03 * torch.randn(n, s, s, generator=g)).abs() * torch.exp(0.35 * xx - 0.25 * yy ** 2 + 0.2 * zz * xx + 0.15 * zz)
    img = (img * disc).to(device).contiguous()
    valid = (img > 0).contiguous()
    v = torch.where(valid, torch.log(img.clamp(min=1e-30)), torch.zeros_like(img))
    vm = v[valid]
    rng = torch.stack([vm.min(), vm.max()])
    n_bins, fwhm, noise = 200, 0.15, 0.01
    common = {"what": "bias_field_correction", "slices": n, "size": s, "voxels": n * s * s, "valid": int(valid.sum()), "repeats": a.repeats}

    os.environ.pop("NESVOR_BIAS", None)
    for S in (1, 8):
        tables = bias.LevelTables(img.shape, S, device)
        f32, f64, v64 = torch.zeros_like(v), torch.zeros_like(v, dtype=torch.float64), v.double()
        hist = torch.ops.nesvor.n4_histogram(v, f32, valid, rng, n_bins)
        lut = bias.sharpen_lut(hist, rng, fwhm, noise)
        lattice, _ = torch.ops.nesvor.n4_fit(v, f32, valid, rng, lut, *tables.basis32, *tables.span, S)
        stats = torch.ops.nesvor.n4_update_(lattice, *tables.basis32, *tables.span, S, f32.clone(), v, valid)
        tables.dense  # (built once per level, outside the iteration)

        def fused_iteration():
            f32.zero_()
            return bias._iteration(v, f32, valid, rng, tables, n_bins, fwhm, noise, True)

        def fused_iteration_with_read():
            f32.zero_()
            return float(bias._cv(bias._iteration(v, f32, valid, rng, tables, n_bins, fwhm, noise, True)[1]))

        fns = {"iteration_fused": fused_iteration,
               "iteration_fused_with_cv_read": fused_iteration_with_read,
               "iteration_composed": lambda: bias._iteration(v64, f64, valid, rng.double(), tables, n_bins, fwhm, noise, False),
               "histogram_fused": lambda: torch.ops.nesvor.n4_histogram(v, f32, valid, rng, n_bins),
               "fit_fused": lambda: torch.ops.nesvor.n4_fit(v, f32, valid, rng, lut, *tables.basis32, *tables.span, S),
               "update_fused": lambda: torch.ops.nesvor.n4_update_(lattice, *tables.basis32, *tables.span, S, f32, v, valid),
               "histogram_composed": lambda: bias.histogram_composed(v64, f64, valid, rng, n_bins),
               "fit_composed": lambda: bias.fit_composed(v64, f64, valid, rng, lut, tables),
               "update_composed": lambda: bias.update_composed(lattice, tables, f64, v64, valid),
               "sharpen_lut": lambda: bias.sharpen_lut(hist, rng, fwhm, noise),
               "cv_read": lambda: float(bias._cv(stats))}
        r = _alternate(fns, 3, a.repeats)
        print(json.dumps({**common, "S": S, "C": S + 3, **r,
                          "speedup_iteration": r["iteration_composed"]["median_ms"] / r["iteration_fused"]["median_ms"],
                          "sharpen_share_of_fused_iteration": r["sharpen_lut"]["median_ms"] / r["iteration_fused"]["median_ms"]}), flush=True)

    def whole(mode):
        def f():
            if mode == "composed":
                os.environ["NESVOR_BIAS"] = "composed"
            try:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                _, field, info = bias.correct_bias_field(img, None)
                e.record()
                e.synchronize()
                return s.elapsed_time(e), field, info
            finally:
                os.environ.pop("NESVOR_BIAS", None)
        return f

    out = {}
    for mode in ("fused", "composed"):
        whole(mode)()  # warm
        runs = [whole(mode)() for _ in range(a.whole_repeats)]
        out[mode] = {"median_ms": statistics.median(r[0] for r in runs), "iterations": runs[0][2]["iterations"], "cv": runs[0][2]["cv"]}
        out[mode + "_field"] = runs[0][1]
    diff = float((out.pop("fused_field").double() - out.pop("composed_field")).abs().max())
    print(json.dumps({**common, "whole_correction": out, "repeats": a.whole_repeats,
                      "speedup_whole": out["composed"]["median_ms"] / out["fused"]["median_ms"],
                      "ms_per_iteration_fused": out["fused"]["median_ms"] / sum(out["fused"]["iterations"]),
                      "largest_field_difference": diff}), flush=True)


if __name__ == "__main__":
    main()
