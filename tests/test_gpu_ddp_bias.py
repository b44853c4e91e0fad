"""GPU (-m gpu): the bias-field model (``n_levels_bias > 0``) data-parallel on the one-call step (csrc/step.hip:
NESVOR_STEP_BIAS_SUM_STOP / NESVOR_STEP_BIAS_SUM_RESUME around the all-reduce of ONE float, ``DirectStep._run_native``).

No multi-GPU box is needed: a forced group of one rank (NESVOR_DDP_FORCE=1; gloo, and RCCL for the production collective), and two
ranks over gloo that share device 0 - the arrangement of the data-parallel tests in tests/test_gpu_model.py."""
import os
import socket

import numpy as np
import pytest
import torch

from conftest import small_args

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_OFF = os.environ.get("NESVOR_STEP_NATIVE", "1") == "0"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture()
def forced_group(monkeypatch):
    """A gloo group of ONE rank with the data-parallel exchange forced on, for the duration of a test."""
    import torch.distributed as dist

    monkeypatch.setenv("NESVOR_DDP_FORCE", "1")
    dist.init_process_group(backend="gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _golden_model(golden, device, args, seed=3):
    """The construction of test_one_call_step_equals_python_issued_step: the golden geometry, parameters moved so that every
    gradient path is live."""
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.transform import RigidTransform

    tf = RigidTransform(torch.tensor(golden["fw_sd::axisangle_init"]).to(device), trans_first=True)
    res = torch.tensor(golden["ds_resolution"]).to(device)
    bbox = torch.tensor(golden["fw_sd::inr.bounding_box"]).to(device)
    torch.manual_seed(seed)
    m = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name in ("logit_coef", "log_var_slice"):
                p.add_(0.3 * torch.randn_like(p))
            if name == "axisangle":
                p.add_(0.02 * torch.randn_like(p))
            if name == "inr.encoding.params":
                p.mul_(1e3)
    return m, (tf, res, bbox)


def _trainer(model, args, hook=True):
    from nesvor_amd import ddp
    from nesvor_amd.fused import FusedTrainer

    t = FusedTrainer(model, args, world_size=1, distributed=True)
    if hook:
        t.reduce_hook = ddp.make_reduce_hook()
    return t


# -------------------------------------------------------------------------------------------------------- 1. the path is taken
@pytest.mark.parametrize("over", [{"n_levels_bias": 2, "n_samples": 16}, {"n_levels_bias": 2, "depth": 2, "n_samples": 16},
                                  {"n_levels_bias": 2, "n_samples": 16, "dtype": torch.float16, "single_precision": False, "mlp_fp16": True}])
def test_bias_field_data_parallel_takes_the_one_call_step(device, golden, forced_group, over):
    """A bias-field model in a (forced) data-parallel group with a reduce hook installed runs ``_run_native`` - the fp32 model at
    both depths and the half-precision structure (bias-free networks) in scaled fp16."""
    if NATIVE_OFF:
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    from nesvor_amd import direct as direct_mod

    args = small_args(device=device, **over)
    m, _ = _golden_model(golden, device, args)
    t = _trainer(m, args)
    assert t.direct is not None and t.direct.parallel and t.direct.has_b
    assert t.direct.native_ready() is True
    calls = []
    orig = direct_mod.DirectStep._run_native

    def spy(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    direct_mod.DirectStep._run_native = spy
    try:
        d = lambda k: torch.tensor(golden[f"fw_{k}"]).to(device)
        losses = t.step(d("xyz"), d("v"), d("idx"))
    finally:
        direct_mod.DirectStep._run_native = orig
    torch.cuda.synchronize()
    assert len(calls) == 1 and t.direct._last_state is not None
    assert all(np.isfinite(float(v)) for v in losses.values()) and torch.isfinite(t.flat.param).all()


def test_timing_spans_survive_the_split(device, golden, forced_group, monkeypatch):
    """``nesvor_step_timing`` across the two calls of a staged step: the spans of the STOP call (sampler, hash-grid forward) and of
    the RESUME call (density forward, loss, backwards) are all read back from one run."""
    if NATIVE_OFF:
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    monkeypatch.setenv("NESVOR_DDP_OVERLAP", "0")
    args = small_args(device=device, n_levels_bias=2, n_samples=16)
    m, _ = _golden_model(golden, device, args)
    t = _trainer(m, args)
    t.direct.set_native_timing(True)
    d = lambda k: torch.tensor(golden[f"fw_{k}"]).to(device)
    t.step(d("xyz"), d("v"), d("idx"))
    spans = t.direct.read_native_timing()
    want = {"psf_transform_fwd", "hashgrid_fwd", "mlp_fwd_density", "mlp_fwd_sigma", "imaging_loss_bwd", "mlp_bwd_density",
            "hashgrid_bwd_aggregate", "hashgrid_bwd_owner", "psf_transform_bwd"}
    assert want <= set(spans), sorted(spans)
    assert all(0.0 < spans[k] < 100.0 for k in want), spans


# -------------------------------------------------------------------------------------------------------------------- 2. C ABI
def test_step_run_accepts_the_bias_field_in_phases_and_stages(device, golden):
    """``nesvor_step_run`` on a ``has_b`` descriptor (built by ``DirectStep._native_state``): a staged phase-0 pair, an un-staged
    phase-1 / phase-2 pair and a staged phase-1 pair + phase 2 all return 0, and every completed step leaves
    losses[5] = lb_mean^2.  Flag combinations that make no sense are refused."""
    if NATIVE_OFF:
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    from nesvor_amd import _lib
    from nesvor_amd.fused import FusedTrainer

    args = small_args(device=device, n_levels_bias=2, n_samples=16)
    m, _ = _golden_model(golden, device, args)
    t = FusedTrainer(m, args)
    ds = t.direct
    d = lambda k: torch.tensor(golden[f"fw_{k}"]).to(device).contiguous()
    xyz, v, idx = d("xyz"), d("v"), d("idx")
    ds.run(xyz, v, idx)  # (single process, phase 0: creates the context and hands it the hash-grid backward's workspace)
    torch.cuda.synchronize()
    st = ds._last_state
    assert st is not None and st["desc"].has_b == 1
    lib = _lib.load()
    vals = torch.zeros(6, dtype=torch.float32, device=device)
    split = ds._split_candidate if ds._split_candidate else 1
    STOP, RESUME = _lib.STEP_BIAS_SUM_STOP, _lib.STEP_BIAS_SUM_RESUME

    def call(phase, split_level, offset):
        with torch.cuda.device(device):
            return lib.nesvor_step_run(st["handle"], _lib.ptr(xyz), _lib.ptr(v), _lib.ptr(idx), 1234, offset, _lib.ptr(vals), phase,
                                       split_level, None, _lib.stream_ptr())

    def completed():
        torch.cuda.current_stream(device).wait_stream(ds.side)
        torch.cuda.synchronize()
        lb = st["buf"]["lb_mean"][0]
        assert torch.isfinite(vals).all() and float(lb) != 0.0
        assert float(vals[5]) == float(lb * lb)
        t.flat.grad.zero_()

    assert call(0 | STOP, 0, 1) == 0 and call(0 | RESUME, 0, 1) == 0  # (NULL event: the stream is ordered already)
    completed()
    assert call(1, split, 2) == 0 and call(2, split, 2) == 0
    completed()
    assert call(1 | STOP, split, 3) == 0 and call(1 | RESUME, split, 3) == 0 and call(2, split, 3) == 0
    completed()
    invalid = 1  # hipErrorInvalidValue
    assert call(0 | STOP | RESUME, 0, 4) == invalid and call(2 | STOP, split, 4) == invalid and call(2 | RESUME, split, 4) == invalid
    assert lib.nesvor_step_set_bias_mean_ranks(st["handle"], 1) == 0
    assert lib.nesvor_step_set_bias_mean_event(st["handle"], None) == 0
    # a model without a bias field has no stages
    args0 = small_args(device=device, n_samples=16)
    m0, _ = _golden_model(golden, device, args0)
    t0 = FusedTrainer(m0, args0)
    t0.direct.run(xyz, v, idx)
    torch.cuda.synchronize()
    st0 = t0.direct._last_state
    with torch.cuda.device(device):
        assert lib.nesvor_step_run(st0["handle"], _lib.ptr(xyz), _lib.ptr(v), _lib.ptr(idx), 1234, 1, _lib.ptr(vals), 0 | STOP, 0, None,
                                   _lib.stream_ptr()) == invalid


# ------------------------------------------------------------------------ 3. one step: staged one-call against Python-issued
@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("over", [
    {"n_levels_bias": 2, "depth": 2, "n_samples": 16}, {"n_levels_bias": 2, "no_pixel_variance": True, "n_samples": 32},
    {"n_levels_bias": 2, "n_samples": 24}, {"n_levels_bias": 2, "mlp_fp16": True, "n_samples": 16},
    # the half-precision STRUCTURE in scaled fp16: bias-free networks, b_net with NULL biases on the staged step
    {"n_levels_bias": 2, "mlp_fp16": True, "n_samples": 16, "dtype": torch.float16, "single_precision": False},
])
def test_staged_one_call_step_equals_python_issued_step(device, golden, forced_group, monkeypatch, over, overlap):
    """The staged one-call step against the same launches issued from Python (``NESVOR_STEP_NATIVE=0``, the only path this model
    had under data parallelism), both in a forced group of one with a reduce hook: with NESVOR_DDP_OVERLAP=1 the fine hash-grid
    levels are exchanged (and updated) early, i.e. the step runs as STOP | phase 1, RESUME | phase 1, phase 2; with 0 as STOP |
    phase 0, RESUME | phase 0.  Tolerances: those of test_one_call_step_equals_python_issued_step - the project's statement for
    "same kernels, the mean's reduction done by a torch op on one side"."""
    if NATIVE_OFF:
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    from nesvor_amd.models import NeSVoR

    monkeypatch.setenv("NESVOR_DDP_OVERLAP", overlap)
    args = small_args(device=device, **over)
    m1, (tf, res, bbox) = _golden_model(golden, device, args)
    m2 = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    m2.load_state_dict(m1.state_dict())
    t1, t2 = _trainer(m1, args, hook=False), _trainer(m2, args, hook=False)
    assert t1.direct is not None and t2.direct is not None
    t2.direct._native_on = False
    assert t1.direct.native_ready() and not t2.direct.native_ready()
    # (1) gradients of one iteration, no optimizer: the split of the hash-grid backward as a reduce hook would set it, but without
    # the hook's early AdamW of the fine levels (the one-call path takes that inside ``run``)
    for t in (t1, t2):
        t.direct.set_overlap(True)
    assert bool(t1.direct.split_level) == (overlap == "1") and t1.direct.split_level == t2.direct.split_level
    d = lambda k: torch.tensor(golden[f"fw_{k}"]).to(device)
    torch.manual_seed(11)
    l1 = t1.direct.run(d("xyz"), d("v"), d("idx"))
    l2 = t2.direct.run(d("xyz"), d("v"), d("idx"))
    assert t1.direct._last_state is not None and t2.direct._last_state is None
    for t in (t1, t2):  # (the early exchange of the fine levels is the identity here: wait for it, nothing to apply)
        early = t.direct.take_early_reduce()
        if early is not None:
            for w in early[0]:
                w.wait()
    assert list(l1.keys()) == list(l2.keys())
    for k in l1:
        a, b = float(l1[k]), float(l2[k])
        print(f"{over} overlap={overlap} one step {k}: one-call {a!r} python-issued {b!r}")
        assert abs(a - b) <= 1e-6 * abs(b) + 1e-9, (k, a, b)
    torch.cuda.synchronize()
    scale = float(t2.flat.grad.abs().max())
    worst = float((t1.flat.grad - t2.flat.grad).abs().max())
    print(f"{over} overlap={overlap} flat gradient: max |diff| {worst:.3e}, largest entry {scale:.3e}")
    assert scale > 0 and worst <= 1e-5 * scale
    t1.flat.grad.zero_(); t2.flat.grad.zero_()
    t1.direct._noise_calls = t2.direct._noise_calls = 0
    # (2) three full steps with the reduce hook: early exchange and early AdamW of the fine levels (overlap), the rest behind the step
    from nesvor_amd import ddp

    for t in (t1, t2):
        t.reduce_hook = ddp.make_reduce_hook()
    for it in range(3):
        l1 = t1.step(d("xyz"), d("v"), d("idx"))
        l2 = t2.step(d("xyz"), d("v"), d("idx"))
        for k in l1:
            a, b = float(l1[k]), float(l2[k])
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (it, k, a, b)
        assert t1.t == t2.t == it + 1
        apart = ((t1.flat.param - t2.flat.param).abs() > 1e-5 * (1 + t2.flat.param.abs())).float().mean()
        print(f"{over} overlap={overlap} step {it}: fraction of parameters apart {float(apart):.3e}")
        assert float(apart) < 2e-3, (it, float(apart))
    assert float(t1.flat.grad.abs().max()) == 0.0


# ----------------------------------------------------------------------------------------- 4. two ranks: the global mean
def _global_mean_worker(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      NESVOR_DIST_BACKEND="gloo", NESVOR_SINGLE_DEVICE="1", NESVOR_DDP_OVERLAP="1", NESVOR_DDP_SHARDED="0",
                      NESVOR_DDP_FORCE="0")
    import torch.distributed as dist

    from nesvor_amd import ddp
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import B_REG

    ddp.init_distributed()
    device = ddp.local_device(rank)
    torch.cuda.set_device(device)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "reference_golden.npz"), allow_pickle=False)
    args = small_args(device=device, n_levels_bias=2, n_samples=16)
    m, _ = _golden_model(golden, device, args)  # (same seed: the same parameters on both ranks)
    t = FusedTrainer(m, args, world_size=world, distributed=True)
    t.reduce_hook = ddp.make_reduce_hook()
    assert t.direct.native_ready() and t.direct.split_level
    d = lambda k: torch.tensor(golden[f"fw_{k}"])
    B = d("xyz").shape[0]
    half = slice(rank * (B // 2), (rank + 1) * (B // 2))
    torch.manual_seed(100 + rank)  # different PSF noise per rank
    losses = t.direct.run(d("xyz")[half].to(device), d("v")[half].to(device), d("idx")[half].to(device))
    torch.cuda.synchronize()
    st = t.direct._last_state
    assert st is not None
    mine = st["buf"]["log_bias"].detach().cpu()
    both = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    assert not torch.equal(both[0], both[1])
    allv = torch.cat(both).double()
    mean, mean_abs = float(allv.mean()), float(allv.abs().mean())
    N = mine.numel()
    # mean_share_kernel (csrc/step.hip), serial fp32 additions on its longest path at N points per rank:
    #   3 per float4 iteration of a thread (pairwise inside the quad, then the accumulate), ceil((N / 4) / (256 G)) iterations with
    #   G = min(256, ceil(N / 1024)) workgroups; at most 1 tail iteration; 8 for the workgroup's tree, 8 for the tree over the
    #   partials; then 2 roundings for the factor 1 / (N W) (forming it, multiplying by it).
    # Each addition adds at most 2^-24 x (sum of |terms| below it): over the whole sum depth x 2^-24 x sum |log_bias|, i.e. depth x
    # 2^-24 x mean |log_bias| after the division - a factor 2 on top - plus ONE rounding, relative to the result, for the
    # two-term all-reduce.
    G = min(256, -(-N // 1024))
    depth = 3 * -(-(N // 4) // (256 * G)) + (1 if N % 4 else 0) + 8 + 8 + 2
    bound = 2 * depth * 2.0 ** -24 * mean_abs + 2.0 ** -24 * abs(mean)
    lb = st["buf"]["lb_mean"].detach().cpu()
    err = abs(float(lb[0].double()) - mean)
    print(f"rank {rank}: lb_mean {float(lb[0])!r} float64 mean {mean!r} |diff| {err:.3e} bound {bound:.3e} (depth {depth}, mean|log_bias| {mean_abs:.3e})")
    assert err <= bound, (err, bound)
    breg = losses[B_REG].detach().cpu().reshape(1)
    sq = float(lb[0]) ** 2
    assert abs(float(breg[0]) - sq) <= 2.0 ** -23 * sq, (float(breg[0]), sq)
    pair = [torch.empty_like(breg) for _ in range(world)]
    dist.all_gather(pair, breg)
    assert pair[0].view(torch.int32).item() == pair[1].view(torch.int32).item()  # bit-identical on both ranks
    lbs = [torch.empty_like(lb) for _ in range(world)]
    dist.all_gather(lbs, lb)
    assert torch.equal(lbs[0], lbs[1])
    early = t.direct.take_early_reduce()
    if early is not None:
        ddp.wait_all(early[0])
    t.direct.join_owner()
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_share_the_global_mean_of_log_bias(device):
    """Two ranks, different halves of the golden batch, one ``direct.run`` each: every rank's ``lb_mean`` equals the float64 mean
    over BOTH ranks' ``log_bias`` within the rounding bound of the reduction (derived in the worker; an absolute bound - the mean
    may be close to zero), and ``losses[B_REG]`` is its square, bit-identical on both ranks."""
    if NATIVE_OFF:
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    import torch.multiprocessing as mp

    mp.spawn(_global_mean_worker, args=(2, _free_port()), nprocs=2, join=True)


# --------------------------------------------------------------------------------------------- 5. / 6. train() in a group
def _ddp_bias_train_worker(rank, world, port, out_dir, tag, overlap="1", backend="gloo", sharded="0", force="0", native="1"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), NESVOR_DIST_BACKEND=backend, NESVOR_SINGLE_DEVICE="1" if backend == "gloo" else "0",
                      NESVOR_DDP_OVERLAP=overlap, NESVOR_DDP_SHARDED=sharded, NESVOR_DDP_FORCE=force, NESVOR_STEP_NATIVE=native)
    import torch.distributed as dist

    from nesvor_amd import ddp, direct as direct_mod
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.train import train

    ddp.init_distributed()
    device = ddp.local_device(rank)
    torch.cuda.set_device(device)
    vol = torch.tensor(phantom3d(n=24), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    args = small_args(device=device, n_iter=12, batch_size=256, n_samples=16, n_levels_bias=2)
    calls = []
    orig = direct_mod.DirectStep._run_native

    def spy(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    direct_mod.DirectStep._run_native = spy
    torch.manual_seed(0)
    inr, out_slices, mask = train(slices, args)
    assert len(calls) == (12 if native == "1" else 0), len(calls)  # every iteration took the one-call step (or none: the reference path)
    sd = {k: v.detach().cpu() for k, v in inr.state_dict().items()}
    torch.save(sd, os.path.join(out_dir, f"rank{rank}_{tag}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _spread(a, b):
    """max over the state dict of |a - b| / (atol + rtol |b|) at the tolerance (2e-3, 2e-5): <= 1 passes assert_close"""
    return max(float(((a[k].double() - b[k].double()).abs() / (2e-5 + 2e-3 * b[k].double().abs())).max()) for k in a)


def test_train_bias_field_two_ranks_stay_in_sync(device, tmp_path):
    """``train()`` with ``n_levels_bias=2`` for 12 iterations on the 24^3 phantom, two ranks over gloo: every worker asserts that
    all 12 iterations took the one-call step; the replicas end bit-identical and finite with the early exchange on, off and with
    the sharded optimizer; and the trained model agrees with the same run on the Python-issued path (NESVOR_STEP_NATIVE=0).

    Tolerance: rtol 2e-3, atol 2e-5 - the figure of the overlap on / off comparison of the bias-free model.  The Python-issued
    path is run TWICE with the same seed (runs that differ through the memory-side float atomics only) and the spread between
    the two, in units of that tolerance, is printed next to the one-call runs' distance.  Measured on an MI355X: the
    Python-issued path against itself 0.002 x the tolerance - twice that is far below it, so the figure stands for this model
    too; the one-call runs (early exchange on / off / sharded) 0.008 x the tolerance from the Python-issued path."""
    if NATIVE_OFF:
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    import torch.multiprocessing as mp

    out = str(tmp_path)
    runs = {"py_a": ("0", "gloo", "0", "0", "0"), "py_b": ("0", "gloo", "0", "0", "0"), "ov1": ("1", "gloo", "0", "0", "1"),
            "ov0": ("0", "gloo", "0", "0", "1"), "sharded": ("1", "gloo", "1", "0", "1")}
    for tag, cfg in runs.items():
        mp.spawn(_ddp_bias_train_worker, args=(2, _free_port(), out, tag, *cfg), nprocs=2, join=True)
    load = lambda tag, r: torch.load(tmp_path / f"rank{r}_{tag}.pt")
    ref, ref_b = load("py_a", 0), load("py_b", 0)
    print(f"Python-issued path against itself (same seed): {_spread(ref_b, ref):.3f} x (rtol 2e-3, atol 2e-5)")
    for tag in ("ov1", "ov0", "sharded"):
        a, b = load(tag, 0), load(tag, 1)
        assert a.keys() == b.keys() == ref.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (tag, k)
        assert all(torch.isfinite(v).all() for v in a.values()), tag
        print(f"one-call {tag} against the Python-issued path: {_spread(a, ref):.3f} x (rtol 2e-3, atol 2e-5)")
    for tag in ("ov1", "ov0", "sharded"):
        a = load(tag, 0)
        for k in ref:
            torch.testing.assert_close(a[k], ref[k], rtol=2e-3, atol=2e-5, msg=f"{tag} {k}")


def test_train_bias_field_rccl_single_rank(device, tmp_path):
    """Backend "nccl" (= RCCL) in a forced group of ONE rank with the bias field: the production collective carries the scalar
    and the step waits for it through the event recorded on the communication stream - the only place that hand-over is
    exercised on a 1-GPU box.  The trained model equals the forced single-rank run over gloo within the tolerance above, with
    and without the sharded optimizer."""
    if NATIVE_OFF:
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    import torch.multiprocessing as mp

    out = str(tmp_path)
    mp.spawn(_ddp_bias_train_worker, args=(1, _free_port(), out, "gloo", "0", "gloo", "0", "1"), nprocs=1, join=True)
    ref = torch.load(tmp_path / "rank0_gloo.pt")
    assert all(torch.isfinite(v).all() for v in ref.values())
    for sharded in ("0", "1"):
        mp.spawn(_ddp_bias_train_worker, args=(1, _free_port(), out, f"nccl{sharded}", "1", "nccl", sharded, "1"), nprocs=1, join=True)
        got = torch.load(tmp_path / f"rank0_nccl{sharded}.pt")
        assert got.keys() == ref.keys()
        print(f"RCCL (sharded={sharded}) against gloo, forced group of one: {_spread(got, ref):.3f} x (rtol 2e-3, atol 2e-5)")
        for k in ref:
            torch.testing.assert_close(got[k], ref[k], rtol=2e-3, atol=2e-5, msg=k)


def test_train_bias_field_rccl_two_gpus(tmp_path):
    """The production exchange with the bias field, one process per GPU; skips with fewer than two HIP devices."""
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    import torch.multiprocessing as mp

    mp.spawn(_ddp_bias_train_worker, args=(2, _free_port(), str(tmp_path), "nccl2", "1", "nccl"), nprocs=2, join=True)
    a, b = torch.load(tmp_path / "rank0_nccl2.pt"), torch.load(tmp_path / "rank1_nccl2.pt")
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert all(torch.isfinite(v).all() for v in a.values())
