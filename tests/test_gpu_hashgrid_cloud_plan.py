"""GPU (-m gpu): the hand-over from the per-cloud hash-grid forward to the aggregation pass of the backward
(``nesvor_hashgrid_forward_plan`` / ``nesvor_hashgrid_backward_plan``, csrc/hashgrid.hip).

The forward of a clustered batch can write, per 256-point cloud, the order the aggregation pass would sort the cloud into and a
plan record (bounding box, lattice boxes, window bits, round schedule).  A backward that takes them must compute what the
backward that finds them itself computes:

* the forward's own outputs do not change (bit-identical ``pe`` and ``pe_absmax``);
* the ``order`` bytes equal the bytes the aggregation pass writes when it sorts;
* ``grad_u`` is bit-identical (a per-lane sum over levels, independent of the schedule), ``grad_table`` agrees within the
  tolerance tests/test_gpu_ops.py uses between the owner-path backward and oracle/hashgrid.py (rtol 1e-4, atol 1e-4: the owner
  pass sums records in arrival order) and agrees with that oracle, no record overflows its queue;
* a backward split by level range that takes the forward's order (no plan: the schedule depends on the range) equals the unsplit one;
* the one-call training step, which hands over, follows the Python-issued step, which does not.

Grids: the headline one (L = 16, T = 2^19, F = 2) and a small one whose levels are all hashed (L = 6, T = 2^12); feature-major.
Point sets at N = 512 (two full clouds) and N = 333 (the second cloud has 77 samples): PSF-like clouds as bench.py builds them,
clouds uniform over the unit cube (no box level), clouds of 256 identical samples (one cell at every level), clouds on the faces
u = 0 and u = 1.  The queues are sized so that nothing can overflow (queue_scale NULL, NESVOR_HASHGRID_CAP_SCALE = 4: every
sub-queue then holds more than 4 x 1024 = 8 N records, all that a level can produce - two uniform clouds that land on one XCC fill
the single chunk of a coarse level with up to 4096), so that a
non-zero overflow counter is a statement about the kernels."""
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SPECS = {"headline": (16, 2, 19, 9, 1.26), "small": (6, 2, 12, 16, 1.3819)}
SPLIT = {"headline": 10, "small": 3}
SETS = ("psf", "uniform", "identical", "faces")
TOL = dict(rtol=1e-4, atol=1e-4)  # tests/test_gpu_ops.py::test_hashgrid_headline_config_vs_oracle, owner method, grad_table


@pytest.fixture(scope="module", autouse=True)
def _worst_case_queues():
    # module scope: the ``case`` fixture below is module-scoped and is set up before any function-scoped fixture, so a
    # function-scoped setenv would come too late for the launches it makes (make_plan reads the variable on every call)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("NESVOR_HASHGRID_CAP_SCALE", "4")
        yield


def _points(kind, N):
    g = torch.Generator().manual_seed({"psf": 11, "uniform": 12, "identical": 13, "faces": 14}[kind])
    n_pix, S = 2, 256
    if kind == "psf":  # bench.py::measure_extras
        c = torch.rand(n_pix, 1, 3, generator=g) * 110 + 10
        x = c + torch.randn(n_pix, S, 3, generator=g) * torch.tensor([0.77, 0.77, 1.27])
        u = (x.reshape(-1, 3) / 130.0).clamp(0, 1)
    elif kind == "uniform":
        u = torch.rand(n_pix * S, 3, generator=g)
    elif kind == "identical":
        u = torch.rand(n_pix, 1, 3, generator=g).expand(n_pix, S, 3).reshape(-1, 3)
    else:
        u = torch.rand(n_pix * S, 3, generator=g)
        axis = torch.randint(0, 3, (n_pix * S,), generator=g)
        side = torch.randint(0, 2, (n_pix * S,), generator=g).float()
        u[torch.arange(n_pix * S), axis] = side
    return u[:N].contiguous()


@functools.lru_cache(maxsize=None)
def _table(spec_name):
    from nesvor_amd.grid import HashGridSpec

    spec = HashGridSpec(*SPECS[spec_name])
    table = (torch.rand(spec.n_params, generator=torch.Generator().manual_seed(1337)) * 2 - 1) * 1e-1
    return spec, table


_WS = {}


def _workspace(lib, spec, N, device):
    key = (spec.n_levels, spec.log2_hashmap_size, N)
    if key not in _WS:
        nbytes = lib.nesvor_hashgrid_backward_workspace_bytes(ctypes.byref(spec.c_struct), N, None)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        ws[: lib.nesvor_hashgrid_backward_workspace_zero_bytes()].zero_()
        _WS[key] = ws
    return _WS[key]


def _overflow(lib, spec, ws):
    off = lib.nesvor_hashgrid_backward_overflow_offset(ctypes.c_void_p(ws.data_ptr()))
    return ws[off : off + 4 * 32].view(torch.int32)[: spec.n_levels].cpu().tolist()


def _compute(spec_name, kind, N):
    """Everything the tests of one (grid, point set, N) look at."""
    from nesvor_amd import _lib
    from oracle import hashgrid as O

    device = torch.device("cuda:0")
    lib = _lib.load()
    spec, table_cpu = _table(spec_name)
    L, E = spec.n_levels, spec.n_output_dims
    g = ctypes.byref(spec.c_struct)
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    u_cpu = _points(kind, N)
    dy_cpu = torch.randn(N, E, generator=torch.Generator().manual_seed(1))
    u, table = u_cpu.to(device), table_cpu.to(device)
    dy = dy_cpu.t().contiguous().to(device)  # feature-major (E, N)
    bound = dy.abs().max().reshape(1).clone()
    layout = _lib.LAYOUT_FEATURE_MAJOR
    ALL, LATER = _lib.HG_STAGE_ALL, _lib.HG_STAGE_KEEP | _lib.HG_STAGE_ACCUMULATE_U
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    out = {"spec": spec, "N": N, "name": f"{spec_name} {kind} N={N}"}
    with torch.cuda.device(device):
        # forward without / with the hand-over
        pe0, mx0 = torch.empty(E, N, device=device), torch.zeros(1, device=device)
        _lib.check(lib.nesvor_hashgrid_forward_bounded(g, P(u), P(table), P(pe0), N, layout | _lib.LAYOUT_CLUSTERED, P(mx0), stream), "forward")
        n_order, n_plan = lib.nesvor_hashgrid_cloud_order_bytes(N), lib.nesvor_hashgrid_cloud_plan_bytes(g, N)
        assert n_order == (N + 255) // 256 * 256 and n_plan > 0 and n_plan % (16 * ((N + 255) // 256)) == 0
        order = torch.full((n_order,), 255, dtype=torch.uint8, device=device)
        plan = torch.zeros(n_plan // 4, dtype=torch.int32, device=device)
        pe1, mx1 = torch.empty(E, N, device=device), torch.zeros(1, device=device)
        _lib.check(lib.nesvor_hashgrid_forward_plan(g, P(u), P(table), P(pe1), N, layout, P(mx1), P(order), P(plan), None, stream), "forward + plan")
        out.update(pe0=pe0, pe1=pe1, mx0=mx0, mx1=mx1, order=order.cpu())
        ws = _workspace(lib, spec, N, device)

        def backward(stages, l0, l1, gt, gu, p_order, p_plan):
            _lib.check(lib.nesvor_hashgrid_backward_plan(g, P(u), P(table), P(dy), P(gt), P(gu), N, layout, P(ws), stages, l0, l1, None, P(bound),
                                                         P(p_order), P(p_plan), stream), "backward")

        # the backward that sorts and plans for itself ...
        gt0, gu0 = torch.zeros_like(table), torch.full_like(u, float("nan"))
        backward(ALL, 0, L, gt0, gu0, None, None)
        off = lib.nesvor_hashgrid_backward_order_offset(g, N, None)
        out.update(gt0=gt0.cpu(), gu0=gu0.cpu(), order_bwd=ws[off : off + n_order].cpu(), overflow0=_overflow(lib, spec, ws))
        # ... the one that takes the forward's order and plan ...
        gt1, gu1 = torch.zeros_like(table), torch.full_like(u, float("nan"))
        backward(ALL, 0, L, gt1, gu1, order, plan)
        out.update(gt1=gt1.cpu(), gu1=gu1.cpu(), overflow1=_overflow(lib, spec, ws))
        # ... and the split one: fine levels, then the coarse ones adding to grad_u, both with the forward's order, no plan
        s = SPLIT[spec_name]
        gt2, gu2 = torch.zeros_like(table), torch.full_like(u, float("nan"))
        backward(ALL, s, L, gt2, gu2, order, None)
        backward(ALL | LATER, 0, s, gt2, gu2, order, None)
        out.update(gt2=gt2.cpu(), gu2=gu2.cpu(), overflow2=_overflow(lib, spec, ws))
        # (the same split where the first launch sorts and the second re-uses its order)
        gt3, gu3 = torch.zeros_like(table), torch.full_like(u, float("nan"))
        backward(ALL, s, L, gt3, gu3, None, None)
        backward(ALL | LATER, 0, s, gt3, gu3, None, None)
        out.update(gt3=gt3.cpu(), gu3=gu3.cpu())
        torch.cuda.synchronize(device)
    lv = O.make_levels(*SPECS[spec_name][:1], *SPECS[spec_name][2:])
    out["gt_ref"], out["gu_ref"] = O.encode_backward(u_cpu, table_cpu, lv, spec.n_features, dy_cpu)
    return out


CASES = [(s, k, n) for s in SPECS for k in SETS for n in (512, 333)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def case(request, device):
    """Computed once per (grid, point set, N) and shared by the tests below (pytest runs them case by case)."""
    assert os.environ.get("NESVOR_HASHGRID_CAP_SCALE") == "4"  # (the queues of _compute's launches are the worst-case ones)
    return _compute(*request.param)


def test_forward_outputs_do_not_change(case):
    c = case
    assert torch.equal(c["pe0"], c["pe1"])
    assert torch.equal(c["mx0"], c["mx1"]) and float(c["mx0"]) > 0


def test_forward_order_equals_the_aggregation_pass_order(case):
    c = case
    assert torch.equal(c["order"], c["order_bwd"])
    # every cloud's bytes are a permutation of 0..255, the lanes past N last
    clouds = c["order"].view(-1, 256).long()
    assert torch.equal(clouds.sort(dim=1).values, torch.arange(256).expand_as(clouds))
    tail = c["N"] % 256
    if tail:
        assert bool((clouds[-1, :tail] < tail).all()) and bool((clouds[-1, tail:] >= tail).all())


def test_backward_with_plan_equals_backward_without(case):
    c = case
    print(f"{c['name']}: overflow self {c['overflow0']} plan {c['overflow1']}; max |grad_table| {float(c['gt_ref'].abs().max()):.3g}, "
          f"plan - self {float((c['gt1'] - c['gt0']).abs().max()):.3g}, plan - oracle {float((c['gt1'] - c['gt_ref']).abs().max()):.3g}, "
          f"self - oracle {float((c['gt0'] - c['gt_ref']).abs().max()):.3g}")
    assert torch.equal(c["gu1"], c["gu0"])
    torch.testing.assert_close(c["gt1"], c["gt0"], **TOL)
    torch.testing.assert_close(c["gt1"], c["gt_ref"], **TOL)
    torch.testing.assert_close(c["gt0"], c["gt_ref"], **TOL)
    assert c["overflow0"] == [0] * c["spec"].n_levels and c["overflow1"] == [0] * c["spec"].n_levels


def test_split_backward_with_forward_order_equals_unsplit(case):
    c = case
    print(f"{c['name']}: overflow split {c['overflow2']}; split - self {float((c['gt2'] - c['gt0']).abs().max()):.3g}, "
          f"grad_u split - self {float((c['gu2'] - c['gu0']).abs().max()):.3g}")
    # against the split backward that sorts for itself: the same launches on the same order, grad_u bit-identical
    assert torch.equal(c["gu2"], c["gu3"])
    torch.testing.assert_close(c["gt2"], c["gt3"], **TOL)
    # against the unsplit backward: grad_u is (fine levels) + (coarse levels), another order of the same per-lane fp32 sum over
    # L <= 16 levels - at most 16 x 2^-24 = 1e-6 of the sum of the terms' magnitudes; ten times that of the largest gradient
    torch.testing.assert_close(c["gu2"], c["gu0"], rtol=1e-5, atol=1e-5 * float(c["gu0"].abs().max()))
    torch.testing.assert_close(c["gt2"], c["gt0"], **TOL)
    torch.testing.assert_close(c["gt2"], c["gt_ref"], **TOL)
    assert c["overflow2"] == [0] * c["spec"].n_levels


def test_plan_is_refused_where_it_does_not_hold(device):
    """A plan covers all levels of a clustered batch: a level range or the unclustered hint with a plan is an error, not a
    silently different schedule."""
    from nesvor_amd import _lib

    lib = _lib.load()
    spec, N = _table("small")[0], 512
    g = ctypes.byref(spec.c_struct)
    one = ctypes.c_void_p(16)  # never dereferenced: the calls are refused on the host
    for layout, l0, l1 in ((_lib.LAYOUT_FEATURE_MAJOR, 0, 3), (_lib.LAYOUT_FEATURE_MAJOR | _lib.LAYOUT_UNCLUSTERED, 0, spec.n_levels)):
        assert lib.nesvor_hashgrid_backward_plan(g, one, one, one, one, None, N, layout, one, _lib.HG_STAGE_AGGREGATE, l0, l1, None, None, one, one, None) != 0


def test_one_call_step_hands_over_and_follows_the_python_issued_step(device, golden):
    """Two steps of ``nesvor_step_run`` at B = 2 pixels x S = 256 samples (two clouds: the forward writes order and plan, the
    aggregation pass reads them) against the same launches issued from Python one by one, where the backward sorts and plans for
    itself: step-1 losses bit for bit (they depend on the forward alone), step-2 losses to the tolerance of
    test_one_call_step_equals_python_issued_step (1e-4 relative + 1e-7)."""
    from conftest import small_args
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.transform import RigidTransform

    if os.environ.get("NESVOR_STEP_NATIVE", "1") == "0":
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    args = small_args(device=device, n_samples=256, batch_size=2)
    tf = RigidTransform(torch.tensor(golden["fw_sd::axisangle_init"]).to(device), trans_first=True)
    res = torch.tensor(golden["ds_resolution"]).to(device)
    bbox = torch.tensor(golden["fw_sd::inr.bounding_box"]).to(device)
    torch.manual_seed(3)
    m1 = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    with torch.no_grad():
        for name, p in m1.named_parameters():
            if name in ("logit_coef", "log_var_slice"):
                p.add_(0.3 * torch.randn_like(p))
            if name == "axisangle":
                p.add_(0.02 * torch.randn_like(p))
            if name == "inr.encoding.params":
                p.mul_(1e3)
    m2 = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    m2.load_state_dict(m1.state_dict())
    t1, t2 = FusedTrainer(m1, args), FusedTrainer(m2, args)
    assert t1.direct is not None and t2.direct is not None
    t2.direct._native_on = False
    assert t1.direct.native_ready() and not t2.direct.native_ready()
    d = lambda k: torch.tensor(golden[f"fw_{k}"]).to(device)[:2].contiguous()
    for it in range(2):
        l1 = t1.step(d("xyz"), d("v"), d("idx"))
        l2 = t2.step(d("xyz"), d("v"), d("idx"))
        assert list(l1.keys()) == list(l2.keys())
        for k in l1:
            a, b = float(l1[k]), float(l2[k])
            print(f"step {it + 1} {k}: one-call {a!r} python-issued {b!r}")
            if it == 0:
                assert a == b, (k, a, b)
            else:
                assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (k, a, b)
