"""GPU (-m gpu): the loss scaler of the fp16 mode on the device (csrc/scaler.hip, fused.LossScaler with a device).

* the finiteness reduction, the predicated AdamW and the update kernel against their host counterparts;
* the trainer: the device scaler steps exactly as the host scaler (the reference implementation) does, without a host read
  per step;
* data parallelism: two ranks over gloo on the one GPU of the test box stay identical, both skip a step whose gradient
  overflowed on ONE rank, and training keeps the mode's PSNR."""
import math
import os
import warnings

import pytest
import torch

from conftest import small_args

pytestmark = pytest.mark.gpu


def _scaler(device, **kw):
    from nesvor_amd.fused import LossScaler

    return LossScaler(device=device, **kw)


# ------------------------------------------------------------------------------------------------------------ found_inf
@pytest.mark.parametrize("n", [1, 4095, (1 << 24) + 3])
def test_grad_found_inf_flags_nan_and_inf_anywhere(device, n):
    sc = _scaler(device)
    g = torch.randn(n, device=device)
    g[: min(n, 3)] = torch.tensor([3.4028235e38, -1e-45, 0.0], device=device)[: min(n, 3)]  # largest finite, denormal, zero

    def verdict(x):
        sc.found_inf = 0
        sc.grad_found_inf(x)
        return sc.found_inf

    assert verdict(g) == 0
    # first, last, the first element of the ragged tail (n % 4 != 0) and one inside the vector body
    positions = sorted({0, n - 1, n // 4 * 4 if n % 4 else n - 1, n // 2})
    for pos in positions:
        keep = g[pos].clone()
        for bad in (float("nan"), float("inf"), float("-inf")):
            g[pos] = bad
            assert verdict(g) == 1, (n, pos, bad)
        g[pos] = keep
    assert verdict(g) == 0
    # a view that starts off a 16-byte boundary (the kernel's scalar head)
    if n > 8:
        v = g[1:]
        assert verdict(v) == 0
        for pos in (0, 1, 2, v.numel() - 1):
            keep = v[pos].clone()
            v[pos] = float("nan")
            assert verdict(v) == 1, ("offset view", n, pos)
            v[pos] = keep
    # the same answer every time
    g[n - 1] = float("inf")
    assert [verdict(g) for _ in range(20)] == [1] * 20
    g[n - 1] = 1.0
    assert [verdict(g) for _ in range(20)] == [0] * 20


def test_grad_found_inf_accumulates_until_update(device):
    sc = _scaler(device)
    bad = torch.tensor([1.0, float("nan"), 2.0, 3.0], device=device)
    sc.grad_found_inf(bad)
    sc.grad_found_inf(torch.ones(64, device=device))  # a finite range after it does not clear the verdict
    assert sc.found_inf == 1
    sc.update()
    assert sc.found_inf == 0 and sc.skipped == 1 and sc.scale == 0.5


# ------------------------------------------------------------------------------------------------------- predicated AdamW
def _adam_buffers(device, n, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 300.0
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    return [x.to(device) for x in (p, g, m, v)]


@pytest.mark.parametrize("n", [4, 1001, 1 << 20])
def test_adamw_step_scaled_equals_adamw_step_on_a_finite_step(device, n):
    lr, b1, b2, eps, wd = 5e-3, 0.9, 0.99, 1e-15, 1e-2
    for t, scale, world in ((1, 1.0, 1), (2, 2.0 ** 10, 1), (7, 0.5, 2), (1234, 2.0 ** -3, 3), (20000, 2.0 ** 24, 8)):
        ref = _adam_buffers(device, n, t)
        got = [x.clone() for x in ref]
        sc = _scaler(device, init_scale=scale)
        sc.t = t - 1  # the kernel takes step t = state.t + 1
        torch.ops.nesvor.adamw_step_(*ref, lr, b1, b2, eps, wd, t, 1.0 / (world * scale), True)
        torch.ops.nesvor.adamw_step_scaled_(*got, lr, b1, b2, eps, wd, world, True, sc.state)
        for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), ref, got):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (n, t, name)
        assert sc.t == t - 1  # (advanced by the update kernel, not here)


def test_adamw_step_scaled_skips_a_flagged_step(device):
    n = 4099
    p, g, m, v = _adam_buffers(device, n, 5)
    before = [x.clone() for x in (p, g, m, v)]
    sc = _scaler(device, init_scale=4.0)
    sc.found_inf = 1
    torch.ops.nesvor.adamw_step_scaled_(p, g, m, v, 5e-3, 0.9, 0.99, 1e-15, 1e-2, 1, False, sc.state)
    for a, b in zip((p, g, m, v), before):
        assert torch.equal(a, b)  # zero_grad off: nothing at all is written
    torch.ops.nesvor.adamw_step_scaled_(p, g, m, v, 5e-3, 0.9, 0.99, 1e-15, 1e-2, 1, True, sc.state)
    assert torch.equal(p, before[0]) and torch.equal(m, before[2]) and torch.equal(v, before[3])
    assert float(g.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------- update kernel
def test_loss_scaler_update_matches_the_host_scaler_over_5000_verdicts(device):
    import random

    from nesvor_amd.fused import LossScaler

    host, dev = LossScaler(growth_interval=7), _scaler(device, growth_interval=7)
    rng = random.Random(1234)
    t = 0
    for i in range(5000):
        # overflow at random, and whenever the scale has grown large (keeps it inside the float range, as training does)
        found = rng.random() < 0.06 or host.scale >= 2.0 ** 40
        dev.found_inf = int(found)
        dev.update()
        host.update(found)
        t += 0 if found else 1
        d = dev._read()
        assert (d["scale"], d["growth_tracker"], d["skipped"], d["t"], d["found_inf"]) == (
            host.scale, host.growth_tracker, host.skipped, t, 0), i
    assert host.skipped > 100 and t > 1000 and host.scale > 1.0


# ------------------------------------------------------------------------------------- the scale's way into the backward
def test_device_scale_reaches_the_loss_weights_and_the_pose_regulariser(device):
    """nesvor_loss_scale_weights and nesvor_step_epilogue_scaled against the host-scaled launch: same bits."""
    from nesvor_amd import _lib

    lib = _lib.load()
    n, B = 17, 33
    r = lambda *s: torch.randn(*s, device=device)
    dc, c, dmat, ax, dtrans, loss_pix, terms = r(n), r(n), r(n, 12), r(n, 6), r(n, 6), r(B, 3), r(n)
    for scale in (1.0, 2.0 ** 13, 2.0 ** -5):
        sc = _scaler(device, init_scale=scale)
        base = torch.tensor([1.0, 0.5, 2.0, 100.0], device=device)
        gw = torch.empty_like(base)
        _lib.check(lib.nesvor_loss_scale_weights(_lib.ptr(base), _lib.ptr(gw), 4, _lib.ptr(sc.state), _lib.stream_ptr()), "weights")
        assert torch.equal(gw, base * scale)
        out = []
        for w_trans, scale_ptr in ((0.1 * scale, None), (0.1, sc.state)):
            dlogit, dax, losses = torch.empty(n, device=device), torch.empty(n, 6, device=device), torch.empty(5, device=device)
            _lib.check(lib.nesvor_step_epilogue_scaled(
                _lib.ptr(dc), _lib.ptr(c), _lib.ptr(dlogit), _lib.ptr(dmat), _lib.ptr(ax), _lib.ptr(dtrans), w_trans, _lib.ptr(scale_ptr),
                _lib.ptr(dax), _lib.ptr(loss_pix), _lib.ptr(terms), _lib.ptr(losses), n, B, 0.25, -0.2, _lib.stream_ptr()), "epilogue")
            out.append((dlogit, dax, losses))
        for a, b in zip(*out):
            assert torch.equal(a, b), scale


# ---------------------------------------------------------------------------------------------------------------- trainer
def _phantom_setup(device, n=32):
    from nesvor_amd.phantom import phantom3d, simulate_stacks

    vol = torch.tensor(phantom3d(n=n), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    return vol, slices


def _mk(device, **kw):
    # the phantom setup of test_gpu_model.py::test_train_phantom_fp16_loss_scaling_keeps_psnr_and_skips_overflowing_steps
    return small_args(device=device, n_iter=300, batch_size=512, n_samples=16, finest_resolution=1.0, log2_hashmap_size=14,
                      no_transformation_optimization=True, depth=2, **kw)


def _fp16_args(device):
    return _mk(device, dtype=torch.float16, single_precision=False, fp16_loss_scaling=True)


def _trainer(ds, args, monkeypatch=None, host=False):
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR

    torch.manual_seed(0)
    model = NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, args)
    if monkeypatch is not None:
        monkeypatch.setenv("NESVOR_LOSS_SCALER", "host" if host else "device")
    tr = FusedTrainer(model, args)
    if monkeypatch is not None:
        monkeypatch.delenv("NESVOR_LOSS_SCALER")
    return tr


def test_device_scaler_trains_bit_identically_to_the_host_scaler(device, monkeypatch):
    """50 steps on the same batches and PSF noise, a forced overflow and scale growth among them: parameters, both moments, the
    step count and the scaler's state equal the host scaler's bit for bit.  (The backward itself is not bit-reproducible from run
    to run - float atomics in the per-slice sums, arrival order in the hash-grid owner pass - so every step hands the device
    trainer's gradient to the host trainer as well; the two backward passes are compared within that run-to-run tolerance, and
    the loss weights they start from bit for bit.)"""
    from nesvor_amd import mlp
    from nesvor_amd.train import Dataset

    _, slices = _phantom_setup(device)
    args = _fp16_args(device)
    try:
        ds = Dataset(slices, args)
        D = _trainer(ds, args, monkeypatch, host=False)
        H = _trainer(ds, args, monkeypatch, host=True)
        assert D.scaler.on_device and not H.scaler.on_device
        assert torch.equal(D.flat.param, H.flat.param)
        gen = torch.Generator(device="cpu").manual_seed(7)
        for i in range(50):
            if i == 3:
                D.scaler.growth_interval = H.scaler.growth_interval = 7
            if i in (20, 41):
                D.scaler.scale = H.scaler.scale = 2.0 ** 60  # every gradient overflows
            if i in (21, 42):
                D.scaler.scale = H.scaler.scale = 4.0  # (instead of ~50 more backoffs from 2^59)
            b = ds.get_batch(args.batch_size, device)
            noise = torch.randn(b["xyz"].shape[0], args.n_samples, 3, generator=gen).to(device)
            H._scaled_backward(b["xyz"], b["v"], b["slice_idx"], noise)
            gh = H.flat.grad.clone()
            D._scaled_backward(b["xyz"], b["v"], b["slice_idx"], noise)
            assert torch.equal(D.direct.gw, H.direct.gw), i
            if i not in (20, 41):
                gd = D.flat.grad
                assert bool(torch.isfinite(gd).all()) and float((gd - gh).abs().max()) <= 1e-3 * float(gh.abs().max()), i
            H.flat.grad.copy_(D.flat.grad)
            D._scaled_update()
            H._scaled_update()
            for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
                assert torch.equal(getattr(D.flat, name), getattr(H.flat, name)), (i, name)
        assert D.t == H.t == 48
        assert D.scaler.state_dict() == H.scaler.state_dict()
        assert H.scaler.skipped == 2 and H.scaler.scale == 8.0  # 4 at step 42, one growth in the 8 steps after it
        # the public step: the same path in one call
        b = ds.get_batch(args.batch_size, device)
        losses = D.step(b["xyz"], b["v"], b["slice_idx"])
        assert D.t == 49 and all(bool(torch.isfinite(v)) for v in losses.values())
        D.finish()
        H.finish()
    finally:
        mlp.HALF_OPERANDS[0] = True


def _count_sync_warnings(tr, batches):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            for b in batches:
                tr.step(b["xyz"], b["v"], b["slice_idx"])
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def test_device_scaler_adds_no_host_synchronisation(device, monkeypatch):
    """Under torch.cuda.set_sync_debug_mode("warn") a step with the device scaler warns no more often than the same model's step
    without a scaler; the host scaler's per-step read of the verdict is caught by the same check."""
    from nesvor_amd import mlp
    from nesvor_amd.train import Dataset

    _, slices = _phantom_setup(device)
    try:
        args = _fp16_args(device)
        ds = Dataset(slices, args)
        batches = [ds.get_batch(args.batch_size, device) for _ in range(8)]
        counts = {}
        for name in ("baseline", "device", "host"):
            a = _mk(device, dtype=torch.float16, single_precision=False) if name == "baseline" else args
            mlp.HALF_OPERANDS[0] = True
            tr = _trainer(ds, a, monkeypatch, host=name == "host")
            assert (tr.scaler is None) == (name == "baseline")
            for b in batches[:3]:  # warm-up: workspaces, record queues, code objects
                tr.step(b["xyz"], b["v"], b["slice_idx"])
            counts[name] = _count_sync_warnings(tr, batches[3:])
            tr.finish()
        print("synchronising calls in 5 steps:", counts)
        assert counts["device"] <= counts["baseline"]
        assert counts["host"] >= 5 and counts["host"] > counts["device"]  # (the check sees the host scaler's read: one per step)
    finally:
        mlp.HALF_OPERANDS[0] = True


def test_sharded_optimizer_is_refused_under_the_loss_scaler(device, monkeypatch):
    import torch.distributed as dist

    from nesvor_amd.train import Dataset

    _, slices = _phantom_setup(device, n=24)
    args = _fp16_args(device)
    args.ddp_sharded_optimizer = True
    ds = Dataset(slices, args)
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR

    model = NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, args)
    assert not (dist.is_available() and dist.is_initialized())
    with pytest.raises(RuntimeError, match="sharded optimizer"):
        FusedTrainer(model, args, world_size=2, distributed=True)


# ------------------------------------------------------------------------------------------------------- data parallel
def _psnr(a, b, peak):
    return 10 * math.log10(peak**2 / float(((a - b) ** 2).mean()))


def _ddp_scaler_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      NESVOR_DIST_BACKEND="gloo", NESVOR_SINGLE_DEVICE="1", NESVOR_DDP_OVERLAP="1", NESVOR_DDP_SHARDED="0",
                      NESVOR_DDP_FORCE="0")
    import torch.distributed as dist

    from nesvor_amd import ddp, mlp
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.train import Dataset, train

    ddp.init_distributed()
    device = ddp.local_device(rank)
    torch.cuda.set_device(device)
    vol, slices = _phantom_setup(device)
    out = {}

    # ---- (a) 30 steps under the device scaler, an Inf in rank 1's gradient before the exchange of step 20
    args = _fp16_args(device)
    ds = Dataset(slices, args)
    torch.manual_seed(0)
    model = NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, args)
    tr = FusedTrainer(model, args, world_size=world, distributed=True)
    assert tr.scaler is not None and tr.scaler.on_device and tr.direct is not None
    ddp.broadcast_params_(tr.flat.param)
    exchange = ddp.make_reduce_hook()
    inject = [False]

    def hook(flat_grad):
        if inject[0] and rank == 1:
            flat_grad[12345].fill_(float("inf"))
        exchange(flat_grad)

    tr.reduce_hook = hook
    assert tr.direct.split_level == 0 and tr.direct.early_update is None  # one all-reduce of the whole buffer
    tr.scaler.growth_interval = 7
    perm_gen = torch.Generator(device=device).manual_seed(0)
    torch.manual_seed(1 + rank)  # per-rank PSF noise
    for i in range(30):
        b = ddp.shard_batch(ds.get_batch(args.batch_size, device, perm_gen), rank, world)
        if i == 20:
            inject[0] = True
            before = [x.clone() for x in (tr.flat.param, tr.flat.exp_avg, tr.flat.exp_avg_sq)]
            st = tr.scaler.state_dict()
            t0 = tr.t
        tr.step(b["xyz"], b["v"], b["slice_idx"])
        if i == 20:
            inject[0] = False
            st1 = tr.scaler.state_dict()
            out["skip"] = {
                "t_unchanged": tr.t == t0,
                "skipped": st1["skipped"] - st["skipped"],
                "backoff": st1["scale"] == st["scale"] * 0.5,
                "untouched": all(torch.equal(a, x) for a, x in zip(before, (tr.flat.param, tr.flat.exp_avg, tr.flat.exp_avg_sq))),
                "grad_zero": float(tr.flat.grad.abs().max()) == 0.0,
            }
    tr.finish()
    out["flat"] = [x.detach().cpu() for x in (tr.flat.param, tr.flat.exp_avg, tr.flat.exp_avg_sq)]
    out["scaler"] = tr.scaler._read()
    out["t"] = tr.t

    # ---- (b) reconstruction quality: fp32 model and fp16 + device scaler, both trained data-parallel
    g = torch.arange(32, dtype=torch.float32) - 15.5
    zz, yy, xx = torch.meshgrid(g, g, g, indexing="ij")
    pts = torch.stack([xx, yy, zz], -1).reshape(-1, 3).to(device)
    truth = vol.reshape(-1)
    inside = truth > 0
    psnr = {}
    for name, kw in (("fp32", dict(dtype=torch.float32, single_precision=True)),
                     ("fp16+scaler", dict(dtype=torch.float16, single_precision=False, fp16_loss_scaling=True))):
        mlp.HALF_OPERANDS[0] = True
        torch.manual_seed(0)
        inr, _, _ = train(slices, _mk(device, **kw))
        with torch.no_grad():
            r = inr(pts[:, None], False).mean(-1).float()
        s = float((r[inside] * truth[inside]).sum() / (r[inside] ** 2).sum())
        psnr[name] = _psnr(r[inside] * s, truth[inside], float(truth.max()))
    out["psnr"] = psnr
    torch.save(out, os.path.join(out_dir, f"scaler_rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_device_scaler_data_parallel_two_ranks(device, tmp_path):
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_ddp_scaler_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a = torch.load(tmp_path / "scaler_rank0.pt")
    b = torch.load(tmp_path / "scaler_rank1.pt")
    for r in (a, b):  # both ranks skipped the step whose gradient overflowed on rank 1 only
        assert r["skip"] == {"t_unchanged": True, "skipped": 1, "backoff": True, "untouched": True, "grad_zero": True}, r["skip"]
    for x, y in zip(a["flat"], b["flat"]):
        assert torch.equal(x, y)
    assert a["scaler"] == b["scaler"] and a["t"] == b["t"] == 29
    assert a["scaler"]["skipped"] == 1 and all(bool(torch.isfinite(x).all()) for x in a["flat"])
    p = a["psnr"]
    print(f"data parallel PSNR: fp32 model {p['fp32']:.2f} dB, fp16 operands + device loss scaler {p['fp16+scaler']:.2f} dB")
    assert p["fp16+scaler"] > 8.0 and abs(p["fp16+scaler"] - p["fp32"]) <= 0.5
