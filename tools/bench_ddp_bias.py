#!/usr/bin/env python
"""The bias-field model (``n_levels_bias=4``, BASELINE C5's model) at bench.py's size (4096 slice pixels x 256 PSF samples = 2^20
points) on ONE GPU, four trainers of the same seed in one process, timed regions alternating between them:

    single        : single process - one nesvor_step_run per iteration, AdamW inside
    ddp_one_call  : forced data-parallel group of one rank (NESVOR_DDP_FORCE=1), the staged one-call step
                    (NESVOR_STEP_BIAS_SUM_STOP / _RESUME around the all-reduce of the bias field's mean)
    ddp_python    : the same group with NESVOR_STEP_NATIVE=0 - the launches issued from Python, a blocking all-reduce of the
                    mean: what this model ran under data parallelism before the staged step
    ddp_sharded   : ddp_one_call with the sharded optimizer (NESVOR_DDP_SHARDED=1)

Per configuration: ms per step (median over the regions, and every region), and the HOST time per step (the loop's wall time
before the closing synchronisation).  On one GPU every collective is the identity: the figures are the overhead of the
data-parallel machinery, not a scaling result.

The measurement runs in a child process under a time limit of its own; a failure or a timeout ends the tool with that status.
Prints one JSON line.

    python tools/bench_ddp_bias.py [--steps 200] [--warmup 20] [--rounds 3] [--backend nccl] [--timeout 400]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(opt):
    import torch
    import torch.distributed as dist

    from nesvor_amd import ddp

    ddp.cap_hw_queues()  # (before the first HIP call, as ddp.init_distributed does)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddp_bias.py needs a HIP device")
    import __graft_entry__ as ge

    ge.build()
    from bench import make_args
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.train import Dataset

    os.environ.update(NESVOR_DDP_FORCE="1", NESVOR_DIST_BACKEND=opt.backend, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    if "MASTER_PORT" not in os.environ:  # a free port: several users of one machine do not collide
        import socket

        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    vol = torch.tensor(phantom3d(n=128), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    args = make_args(device, opt.batch_size, opt.n_samples, 2, n_iter=6000)
    args.n_levels_bias = 4
    ds = Dataset(slices, args)

    def model():
        torch.manual_seed(0)
        return NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, args)

    trainers = {"single": FusedTrainer(model(), args)}  # (made before the process group exists: a single-process trainer)
    trainers["single"].defer_table_join = True  # as train() sets it without a per-iteration callback
    ddp.init_distributed()
    for name, env in (("ddp_one_call", {}), ("ddp_python", {"NESVOR_STEP_NATIVE": "0"}), ("ddp_sharded", {"NESVOR_DDP_SHARDED": "1"})):
        os.environ.update(env)
        tr = trainers[name] = FusedTrainer(model(), args, world_size=1, distributed=True)
        ddp.broadcast_params_(tr.flat.param)
        tr.reduce_hook = ddp.make_reduce_hook()
        for k in env:
            os.environ.pop(k)
        assert tr.direct is not None and tr.direct.parallel and tr.direct.native_ready() == (name != "ddp_python"), name
        assert tr.sharded == (name == "ddp_sharded")
    assert trainers["single"].direct.native_ready() and not trainers["single"].direct.parallel
    perm_gen = torch.Generator(device=device).manual_seed(0)

    def run(tr, n):
        for _ in range(n):
            b = ds.get_batch(args.batch_size, device, perm_gen)
            tr.step(b["xyz"], b["v"], b["slice_idx"])

    for tr in trainers.values():  # warm-up: code objects, workspaces, the hash-grid record queues, the communicator
        for _ in range(opt.warmup):
            run(tr, 1)
            torch.cuda.synchronize(device)
    ms = {name: [] for name in trainers}
    host = {name: [] for name in trainers}
    for _ in range(opt.rounds):
        for name, tr in trainers.items():
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run(tr, opt.steps)
            t1 = time.perf_counter()
            tr.join()
            torch.cuda.synchronize(device)
            host[name].append((t1 - t0) / opt.steps * 1e3)
            ms[name].append((time.perf_counter() - t0) / opt.steps * 1e3)
    out = {"points_per_iter": opt.batch_size * opt.n_samples, "n_levels_bias": args.n_levels_bias, "backend": opt.backend,
           "steps_per_region": opt.steps, "regions": opt.rounds}
    for name in trainers:
        out[name] = {"ms_per_step": statistics.median(ms[name]), "host_ms_per_step": statistics.median(host[name]),
                     "regions_ms_per_step": [round(x, 4) for x in ms[name]], "regions_host_ms_per_step": [round(x, 4) for x in host[name]],
                     "t": trainers[name].t}
    out["one_call_minus_python_ms"] = out["ddp_one_call"]["ms_per_step"] - out["ddp_python"]["ms_per_step"]
    out["one_call_minus_single_ms"] = out["ddp_one_call"]["ms_per_step"] - out["single"]["ms_per_step"]
    print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed region (steady state: at least 200)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="timed regions per configuration, alternating")
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--n-samples", type=int, default=256)
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    opt = ap.parse_args()
    if opt.worker:
        return worker(opt)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", *sys.argv[1:]]
    try:
        rc = subprocess.run(cmd, timeout=opt.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"no result within {opt.timeout} s - stopping")
    if rc != 0:
        raise SystemExit(f"exit status {rc} - stopping")


if __name__ == "__main__":
    main()
