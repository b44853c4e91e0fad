"""Timing of the 16-bit-operand dX + dW launch pair (csrc/mlp.hip: mlp_bwd_dx16_kernel / mlp_bwd_dw16_kernel) next to the fp32-MFMA
pair on the same shapes (mlp_wide.hip at width 64: what NESVOR_MLP_FP32=mfma runs for them), and the step time of default-precision
training at --depth 3 (bias-free half-precision networks: autograd over flat_network, the pair in every backward).

    python tools/bench_mlp_half_pair.py [--n-log2 20] [--reps 20] [--steps 20]

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def time_backward(mode, depth, k_b, out_dim, N, reps, dev):
    from nesvor_amd import mlp

    g = torch.Generator().manual_seed(0)
    dims = [k_b] + [64] * depth + [out_dim]
    W = [((torch.rand(o, i, generator=g) * 2 - 1) * (6.0 / (i + o)) ** 0.5).to(dev) for i, o in zip(dims, dims[1:])]
    B = [torch.zeros(o, device=dev) for o in dims[1:]]
    xb = torch.randn(k_b, N, generator=g).to(dev)
    dy = torch.randn(out_dim, N, generator=g).to(dev)
    _, saved = mlp.forward_raw(W, B, None, xb, 0, k_b, 256, True, mode)
    dxb = torch.empty_like(xb)
    old = mlp.FUSED_BACKWARD
    mlp.FUSED_BACKWARD = False  # the launch pair in every mode (these shapes take nothing else)
    try:
        for _ in range(3):
            mlp.backward_raw(W, B, None, xb, dy, saved, 0, k_b, 256, dxb, False, mode)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
        for r in range(reps):
            ev[2 * r].record()
            mlp.backward_raw(W, B, None, xb, dy, saved, 0, k_b, 256, dxb, False, mode)
            ev[2 * r + 1].record()
        torch.cuda.synchronize()
    finally:
        mlp.FUSED_BACKWARD = old
    ts = sorted(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(reps))
    return ts[len(ts) // 2]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-log2", type=int, default=20)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--steps", type=int, default=20)
    a = p.parse_args()
    from nesvor_amd import mlp

    dev = torch.device("cuda:0")
    N = 1 << a.n_log2
    for name, depth, k_b in (("density depth 3, 24 inputs", 3, 24), ("density depth 2, 48 inputs", 2, 48)):
        row = {"shape": name, "N": N}
        for tag, mode in (("bf16_pair_ms", mlp.BF16), ("fp16_pair_ms", mlp.FP16), ("fp32_mfma_pair_ms", mlp.MFMA_FP32)):
            row[tag] = round(time_backward(mode, depth, k_b, 16, N, a.reps, dev), 4)
        print(json.dumps(row), flush=True)
    print(json.dumps(train_step_time(a.steps, dev)), flush=True)


def train_step_time(steps, dev):
    """Mean FusedTrainer.step time, default precision, --depth 3, 4096 pixels x 64 samples on a simulated 64^3 phantom."""
    from argparse import Namespace

    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.train import Dataset

    vol = torch.tensor(phantom3d(n=64), dtype=torch.float32, device=dev)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    args = Namespace(
        n_features_per_level=2, log2_hashmap_size=19, level_scale=1.3819, coarsest_resolution=16.0, finest_resolution=0.5,
        n_levels_bias=0, depth=3, width=64, n_features_z=15, n_features_slice=16, no_transformation_optimization=False,
        no_slice_scale=False, no_pixel_variance=False, no_slice_variance=False, single_precision=False,
        weight_transformation=0.1, weight_bias=100.0, image_regularization="edge", weight_image=2.0, delta=0.2,
        learning_rate=5e-3, gamma=0.33, milestones=[0.5, 0.75, 0.9], n_iter=steps, batch_size=4096, n_samples=64,
        output_resolution=0.8, output_intensity_mean=700.0, mask_threshold=1.0, no_output_psf=False, debug=False,
        device=dev, dtype=torch.float16, inference_batch_size=32768, n_inference_samples=128)
    ds = Dataset(slices, args)
    torch.manual_seed(0)
    model = NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, args)
    tr = FusedTrainer(model, args)
    batches = [ds.get_batch(args.batch_size, dev) for _ in range(4)]
    for i in range(3):
        b = batches[i % 4]
        tr.step(b["xyz"], b["v"], b["slice_idx"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        b = batches[i % 4]
        tr.step(b["xyz"], b["v"], b["slice_idx"])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tr.finish()
    return {"measurement": "default-precision training step, depth 3", "points": args.batch_size * args.n_samples,
            "direct_step": tr.direct is not None, "step_ms": round(dt * 1e3, 3)}


if __name__ == "__main__":
    main()
