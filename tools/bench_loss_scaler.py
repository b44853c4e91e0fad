#!/usr/bin/env python
"""The ``--fp16-loss-scaling`` training step at bench.py's size (4096 slice pixels x 256 PSF samples = 2^20 points, the
half-precision model structure with fp16 matrix operands under the reference's GradScaler): iterations/s with the host
scaler (NESVOR_LOSS_SCALER=host: one device read per step) and with the device scaler (csrc/scaler.hip), two models of the same
seed in one process, timed regions alternating between them.  Prints one JSON line.

    python tools/bench_loss_scaler.py [--steps 100] [--warmup 10] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="timed regions per scaler, alternating host / device")
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--n-samples", type=int, default=256)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss_scaler.py needs a HIP device")

    import __graft_entry__ as ge

    ge.build()
    from bench import make_args
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.train import Dataset

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    vol = torch.tensor(phantom3d(n=128), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    args = make_args(device, opt.batch_size, opt.n_samples, 2, n_iter=6000)
    args.dtype, args.single_precision, args.fp16_loss_scaling = torch.float16, False, True
    ds = Dataset(slices, args)
    trainers = {}
    for mode in ("host", "device"):
        os.environ["NESVOR_LOSS_SCALER"] = mode
        torch.manual_seed(0)
        model = NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, args)
        trainers[mode] = FusedTrainer(model, args)
        assert trainers[mode].scaler.on_device == (mode == "device")
    os.environ.pop("NESVOR_LOSS_SCALER")
    perm_gen = torch.Generator(device=device).manual_seed(0)

    def run(tr, n):
        for _ in range(n):
            b = ds.get_batch(args.batch_size, device, perm_gen)
            tr.step(b["xyz"], b["v"], b["slice_idx"])

    for tr in trainers.values():  # warm-up: code objects, workspaces, the hash-grid record queues
        for _ in range(opt.warmup):
            run(tr, 1)
            torch.cuda.synchronize(device)
    ms = {mode: [] for mode in trainers}
    for _ in range(opt.rounds):
        for mode, tr in trainers.items():
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run(tr, opt.steps)
            torch.cuda.synchronize(device)
            ms[mode].append((time.perf_counter() - t0) / opt.steps * 1e3)
    points = opt.batch_size * opt.n_samples
    out = {"points_per_iter": points, "steps_per_region": opt.steps, "regions": opt.rounds}
    for mode, v in ms.items():
        med = statistics.median(v)
        out[mode] = {"iters_per_s": 1e3 / med, "ms_per_step": med, "regions_ms_per_step": v,
                     "t": trainers[mode].t, "skipped": trainers[mode].scaler.skipped, "scale": trainers[mode].scaler.scale}
    out["device_over_host"] = out["device"]["iters_per_s"] / out["host"]["iters_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
