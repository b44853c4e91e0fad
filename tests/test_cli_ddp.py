"""``reconstruct`` under a launcher (torchrun's environment): every rank joins the process group and trains data-parallel, rank
0 alone samples and writes the outputs.  Two spawned ranks over gloo on device 0, with the bias field - the model whose step
needs a collective of its own."""
import json
import os
import socket

import pytest
import torch


def test_parser_keeps_the_reference_flag_table_and_the_launcher_changes_no_flag():
    """CPU: the launcher support adds no flag and moves no default of the reference's table; ``--device`` stays an integer index
    (unset = 0, or the rank's own device under a launcher)."""
    from nesvor_amd.cli import build_parser

    a = build_parser().parse_args(["reconstruct", "--input-slices", "x", "--output-volume", "v.nii.gz"])
    assert a.n_levels_bias == 0 and a.batch_size == 4096 and a.n_iter == 6000 and a.seed is None and a.device is None
    b = build_parser().parse_args(["reconstruct", "--input-slices", "x", "--device", "3", "--n-levels-bias", "4"])
    assert b.device == 3 and b.n_levels_bias == 4
    names = {o for act in build_parser()._subparsers._group_actions[0].choices["reconstruct"]._actions for o in act.option_strings}
    assert not any("rank" in n or "world" in n or "dist" in n for n in names)


def test_other_commands_return_at_once_on_ranks_above_zero(monkeypatch):
    """CPU: ``register`` / ``sample-volume`` / ``sample-slices`` stay single-process - under a launcher every rank but 0 returns
    before it touches a device or a file."""
    from nesvor_amd import cli

    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "2")
    cli.main(["sample-volume", "--input-model", "/nonexistent/model.pt", "--output-volume", "/nonexistent/v.nii.gz"])
    cli.main(["register", "--input-stacks", "/nonexistent/a.nii.gz", "--output-slices", "/nonexistent/out"])


def test_seedless_launch_broadcasts_a_seed_that_fits_int64(monkeypatch, tmp_path):
    """CPU: ``reconstruct`` under a launcher WITHOUT ``--seed``: rank 0's ``torch.seed()`` - an unsigned 64-bit value, above 2^63
    half of the time - travels as an int64 and becomes the process's seed; and only rank 0 opens ``--output-log``."""
    import logging
    from argparse import Namespace

    import torch.distributed as dist

    from nesvor_amd import cli

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    for k, v in dict(NESVOR_DDP_FORCE="1", NESVOR_DIST_BACKEND="gloo", NESVOR_SINGLE_DEVICE="1", MASTER_ADDR="127.0.0.1",
                     MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0").items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)  # (no HIP device on the CPU box; nothing is launched)
    monkeypatch.setattr(torch, "seed", lambda: 2**63 + 5)
    log = tmp_path / "run.log"
    args = Namespace(command="reconstruct", verbose=0, output_log=str(log), seed=None, device=None)
    try:
        cli._setup(args)
        assert dist.is_initialized() and args.distributed and args.rank == 0
        assert torch.initial_seed() == 5  # the low 63 bits of rank 0's draw
        assert str(args.device) == "cuda:0" and log.exists()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        logging.basicConfig(force=True)
    # a rank above 0 does not open (and truncate) the log file
    log.unlink()
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(cli, "_under_launcher", lambda: True)
    import nesvor_amd.ddp as ddp

    monkeypatch.setattr(ddp, "init_distributed", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("stop here")))
    with pytest.raises(RuntimeError, match="stop here"):
        cli._setup(Namespace(command="reconstruct", verbose=0, output_log=str(log), seed=None, device=None))
    assert not log.exists()
    logging.basicConfig(force=True)


def _cli_worker(rank, world, port, paths, out_dir, seed_flags=("--seed", "0")):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      NESVOR_DIST_BACKEND="gloo", NESVOR_SINGLE_DEVICE="1", NESVOR_DDP_OVERLAP="1", NESVOR_DDP_SHARDED="0",
                      NESVOR_DDP_FORCE="0")
    import torch.distributed as dist

    import nesvor_amd.train as train_mod
    from nesvor_amd import cli

    seen = {"outputs": 0, "world_in_train": None, "seed_in_train": None, "device": None}
    orig_outputs, orig_train = cli._outputs, train_mod.train

    def outputs(data, args):
        seen["outputs"] += 1
        return orig_outputs(data, args)

    def train(slices, args, *a, **k):
        seen["world_in_train"] = dist.get_world_size() if dist.is_initialized() else 0
        seen["seed_in_train"] = torch.initial_seed()
        seen["device"] = str(args.device)
        return orig_train(slices, args, *a, **k)

    cli._outputs, train_mod.train = outputs, train
    cli.main(["reconstruct", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--output-volume", os.path.join(out_dir, "recon.nii.gz"),
              "--output-model", os.path.join(out_dir, "model.pt"), "--n-levels-bias", "2", "--single-precision", "--n-iter", "80",
              "--batch-size", "512", "--n-samples", "32", "--log2-hashmap-size", "12", "--finest-resolution", "2.0",
              "--output-resolution", "2.0", *seed_flags, "--verbose", "0", "--output-log", os.path.join(out_dir, "run.log")])
    seen["group_left"] = dist.is_initialized()
    with open(os.path.join(out_dir, f"seen{rank}.json"), "w") as f:
        json.dump(seen, f)


@pytest.mark.gpu
@pytest.mark.parametrize("seed_flags", [("--seed", "0"), ()], ids=["seed0", "seedless"])
def test_cli_reconstruct_two_ranks_write_once(tmp_path, device, seed_flags):
    import torch.multiprocessing as mp

    from nesvor_amd.image import Volume
    from nesvor_amd.image_io import load_model, load_volume
    from nesvor_amd.phantom import phantom3d, simulate_stacks, stack_geometry
    from nesvor_amd.transform import RigidTransform

    # (the stacks of tests/test_cli.py::test_cli_reconstruct_sample_roundtrip)
    vs, res_s, gap = 32, 1.5, 3.0
    vol = torch.tensor(phantom3d(n=vs), dtype=torch.float32, device=device)
    torch.manual_seed(0)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=res_s, s_thick=gap, normalize=False)
    n_slice, _ = stack_geometry(vs, 1.0, res_s, gap)
    paths = []
    for i in range(3):
        ss = slices[i * n_slice : (i + 1) * n_slice]
        img = torch.cat([s.image for s in ss], 0)
        ax = torch.cat([s.transformation.axisangle() for s in ss], 0).mean(0, keepdim=True)
        p = str(tmp_path / f"stack{i}.nii.gz")
        Volume(img, img > 0, RigidTransform(ax), res_s, res_s, gap).save(p, masked=False)
        paths.append(p)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_cli_worker, args=(2, port, paths, str(tmp_path), seed_flags), nprocs=2, join=True)
    seen = [json.load(open(tmp_path / f"seen{r}.json")) for r in range(2)]
    assert [s["world_in_train"] for s in seen] == [2, 2]  # the process group existed, with both ranks, while training
    assert seen[0]["seed_in_train"] == seen[1]["seed_in_train"]  # identical seeds in front of train(): --seed, or rank 0's draw
    assert (seen[0]["seed_in_train"] == 0) == bool(seed_flags)
    assert os.path.exists(tmp_path / "run.log")  # (--output-log: opened by rank 0 alone)
    assert [s["outputs"] for s in seen] == [1, 0]  # only rank 0 reached _outputs
    assert not seen[0]["group_left"] and not seen[1]["group_left"]  # every rank destroyed the group
    v = load_volume(str(tmp_path / "recon.nii.gz"), device=device)
    assert v.image.ndim == 3 and abs(v.resolution_x - 2.0) < 1e-3 and torch.isfinite(v.image).all()
    assert abs(float(v.image[v.mask].mean()) - 700.0) < 1.0  # --output-intensity-mean
    inr, mask, stored = load_model(str(tmp_path / "model.pt"), device)
    assert stored.n_levels_bias == 2 and all(torch.isfinite(p).all() for p in inr.parameters())
