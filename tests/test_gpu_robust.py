"""Robust statistics on the GPU: the E-step kernel (csrc/robust.hip) against the torch expression in fp64, its refusals, the
fused EM rounds against the composed ones, ``reconstruct_volume(robust_rounds=3)`` on the 48^3 phantom and the command line."""
import json
import os

import pytest
import torch

# (n, h, w): a single pixel; one wave; one pixel past a wave; exactly one workgroup; two workgroups, the second ragged
CASES = [((1, 1, 1), "none"), ((3, 8, 8), "random"), ((3, 5, 13), "random"), ((2, 16, 16), "random"),
         ((5, 19, 23), "none"), ((5, 19, 23), "random"), ((5, 19, 23), "slice")]
SIGMA2 = (1e-6, 4e-4, 1e-2)
C = (0.01, 0.9)
_DATA = {}


def _data(shape, kind, device):
    """sim in [0.1, 0.9), y = (sim + 0.02 noise) / gain with gains in [0.7, 1.3] (which are also the scales passed: the
    residuals are then of the size of the middle sigma) and +0.8 on a few pixels; shared by the tests and never written."""
    key = (shape, kind)
    if key not in _DATA:
        n, h, w = shape
        g = torch.Generator().manual_seed(100 * n + 10 * h + w)
        sim = 0.1 + 0.8 * torch.rand(n, 1, h, w, generator=g)
        scale = 0.7 + 0.6 * torch.rand(n, generator=g)
        y = (sim + 0.02 * torch.randn(n, 1, h, w, generator=g)) / scale.view(n, 1, 1, 1)
        y = y + 0.8 * (torch.rand(n, 1, h, w, generator=g) < 0.02)
        mask = None
        if kind != "none":
            mask = torch.rand(n, 1, h, w, generator=g) < 0.7
            if kind == "slice":
                mask[1] = False
        _DATA[key] = tuple(None if t is None else t.to(device) for t in (sim, y, mask, scale))
    return _DATA[key]


def _model(sim, y, mask, sigma2, c):
    yv = y if mask is None else y[mask]
    m = 1.0 / (2.1 * float(yv.max()) - 1.9 * float(yv.min()))
    return torch.tensor([sigma2, c, m], dtype=torch.float32, device=sim.device)


def _ulp(value: torch.Tensor) -> float:
    v = value.float()
    return float(torch.nextafter(v, torch.full_like(v, float("inf"))) - v)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", CASES)
def test_estep_against_the_torch_expression_in_fp64(device, shape, kind):
    """For p and each of the six sums the kernel's largest error against the fp64 expression is at most twice that of the same
    expression evaluated per pixel in fp32 (its sums in fp64) plus one fp32 ulp of the largest magnitude; the count is exact and
    p is exactly 0 off the mask.  Measured on MI355X (largest over the cases): DESIGN.md, "Robust statistics"."""
    from nesvor_amd.robust import estep_composed

    sim, y, mask, scale = _data(shape, kind, device)
    n = shape[0]
    count = torch.full((n,), float(shape[1] * shape[2]), dtype=torch.float64, device=device) if mask is None else mask.flatten(1).sum(1).double()
    names = ("n", "sum p", "sum p e2", "sum (1-p)^2", "sum p y sim", "sum p y2", "sum e2")
    for sigma2 in SIGMA2:
        for c in C:
            model = _model(sim, y, mask, sigma2, c)
            p64, s64 = estep_composed(sim.double(), y.double(), mask, scale.double(), model.double())
            p32, s32 = estep_composed(sim, y, mask, scale, model)
            p, s = torch.ops.nesvor.robust_estep(sim, y, mask, scale, model)
            assert p.shape == sim.shape and p.dtype == torch.float32 and s.shape == (n, 7) and s.dtype == torch.float64
            assert torch.equal(s[:, 0], count)
            if mask is not None:
                assert bool((p[~mask] == 0).all())
                if kind == "slice":
                    assert bool((s[1] == 0).all())
            err_k, err_c = float((p.double() - p64).abs().max()), float((p32.double() - p64).abs().max())
            ulp = _ulp(p64.abs().max())
            print(f"{shape} {kind} sigma2 {sigma2:g} c {c:g}: p kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e}")
            assert err_k <= 2 * err_c + ulp
            for j in range(1, 7):
                err_k, err_c = float((s[:, j] - s64[:, j]).abs().max()), float((s32[:, j] - s64[:, j]).abs().max())
                ulp = _ulp(s64[:, j].abs().max())
                print(f"    {names[j]}: kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e} (largest {float(s64[:, j].abs().max()):.4e})")
                assert err_k <= 2 * err_c + ulp, names[j]
            again_p, again_s = torch.ops.nesvor.robust_estep(sim, y, mask, scale, model)
            assert torch.equal(again_p, p) and torch.equal(again_s, s)


@pytest.mark.gpu
def test_estep_takes_a_byte_mask_and_flat_slices(device):
    sim, y, mask, scale = _data((5, 19, 23), "random", device)
    model = _model(sim, y, mask, 4e-4, 0.9)
    p, s = torch.ops.nesvor.robust_estep(sim, y, mask, scale, model)
    p8, s8 = torch.ops.nesvor.robust_estep(sim[:, 0], y[:, 0], mask[:, 0].to(torch.uint8), scale, model)
    assert p8.shape == (5, 19, 23) and torch.equal(p8, p[:, 0]) and torch.equal(s8, s)
    meta = torch.ops.nesvor.robust_estep(sim.to("meta"), y.to("meta"), None, scale.to("meta"), model.to("meta"))
    assert meta[0].shape == sim.shape and meta[1].shape == (5, 7) and meta[1].dtype == torch.float64


@pytest.mark.gpu
def test_estep_refusals(device):
    """Every refusal returns before a launch (csrc/robust.hip: the checks are the first statements of nesvor_robust_estep), so
    the sentinels in p and stats stay."""
    from nesvor_amd import _lib

    lib = _lib.load()
    n, h, w = 5, 19, 23
    sim, y, mask, scale = _data((n, h, w), "random", device)
    model = _model(sim, y, mask, 4e-4, 0.9)
    p = torch.full((n, h, w), -7.0, device=device)
    stats = torch.full((n, 7), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_robust_estep_workspace_bytes(n, h, w))
    assert nbytes == 8 * 7 * n * 2  # two workgroups per slice
    assert lib.nesvor_robust_estep_workspace_bytes(0, h, w) == 0 and lib.nesvor_robust_estep_workspace_bytes(n, 0, w) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    P = _lib.ptr

    def call(n_=n, h_=h, w_=w, sim_=sim, y_=y, scale_=scale, model_=model, p_=p, stats_=stats, ws_=ws, nb=nbytes):
        return lib.nesvor_robust_estep(P(sim_), P(y_), P(mask), P(scale_), P(model_), n_, h_, w_, P(p_), P(stats_), P(ws_), nb, _lib.stream_ptr())

    assert call(nb=nbytes - 1) != 0 and call(nb=0) != 0 and call(ws_=None) != 0  # a short or missing workspace
    assert call(n_=-1) != 0 and call(h_=0) != 0 and call(w_=0) != 0 and call(w_=-3) != 0
    assert call(h_=65536, w_=65536) != 0 and call(h_=1, w_=2 ** 31 - 256) != 0  # h w > INT_MAX - 256
    for name in ("sim_", "y_", "scale_", "model_", "p_", "stats_"):
        assert call(**{name: None}) != 0
    assert call(n_=0) == 0 and call(n_=0, ws_=None, nb=0) == 0  # no slices: a no-op
    torch.cuda.synchronize()
    assert bool((p == -7.0).all()) and bool((stats == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(p.view_as(sim), torch.ops.nesvor.robust_estep(sim, y, mask, scale, model)[0])
    empty = torch.ops.nesvor.robust_estep(sim[:0], y[:0], None, scale[:0], model)
    assert empty[0].shape == (0, 1, h, w) and empty[1].shape == (0, 7)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::robust_estep'"):
        torch.ops.nesvor.robust_estep(sim.cpu(), y.cpu(), mask.cpu(), scale.cpu(), model.cpu())
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.robust_estep(sim.double(), y.double(), mask, scale.double(), model.double())
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.robust_estep(sim, y, mask, scale, model.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.nesvor.robust_estep(sim.transpose(-1, -2), y.transpose(-1, -2), None, scale, model)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        torch.ops.nesvor.robust_estep(sim, y, mask.float(), scale, model)
    with pytest.raises(RuntimeError, match="one shape"):
        torch.ops.nesvor.robust_estep(sim, y[:4].contiguous(), mask, scale, model)
    with pytest.raises(RuntimeError, match="scale"):
        torch.ops.nesvor.robust_estep(sim, y, mask, scale[:4].contiguous(), model)


# ---------------------------------------------------------------------------------------------------------------------
# the EM rounds on both paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fused_em_follows_the_composed_one(device, monkeypatch):
    """Three rounds on the (5,19,23) case with its random mask: slice weights and scales of the fused path within 1e-4 of the
    composed fp32 path, both within 1e-3 of the same rounds in fp64."""
    from nesvor_amd import robust

    sim, y, mask, _ = _data((5, 19, 23), "random", device)
    calls = []
    inner = robust.estep_composed
    monkeypatch.setattr(robust, "estep_composed", lambda *a: calls.append(1) or inner(*a))

    def rounds(s, t):
        rs = robust.RobustStatistics().init(s, t, mask)
        for _ in range(3):
            rs.update(s, t, mask)
        return rs

    monkeypatch.delenv("NESVOR_ROBUST", raising=False)
    fused = rounds(sim, y)
    assert not calls  # the fused path never evaluates the torch expression
    monkeypatch.setenv("NESVOR_ROBUST", "composed")
    composed = rounds(sim, y)
    assert len(calls) == 4
    monkeypatch.delenv("NESVOR_ROBUST")
    exact = rounds(sim.double(), y.double())
    assert len(calls) == 8 and exact.scale.dtype == torch.float64 and fused.scale.dtype == composed.scale.dtype == torch.float32
    gap = lambda a, b: max(float((a.slice_weight.double() - b.slice_weight.double()).abs().max()),
                           float((a.scale.double() - b.scale.double()).abs().max()))
    print(f"weights {fused.slice_weight.tolist()} scales {fused.scale.tolist()} model {fused.model.tolist()}")
    print(f"fused - composed {gap(fused, composed):.3e}; against fp64: fused {gap(fused, exact):.3e}, composed {gap(composed, exact):.3e}")
    assert gap(fused, composed) <= 1e-4
    assert gap(fused, exact) <= 1e-3 and gap(composed, exact) <= 1e-3
    assert float((fused.model.double() - exact.model).abs().max()) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_a_round_reads_nothing_back_to_the_host(device, monkeypatch, path):
    """``update`` under torch's synchronisation check: any read of a device value (``.item()``, ``nonzero``, a blocking copy)
    raises there."""
    from nesvor_amd import robust

    sim, y, mask, _ = _data((5, 19, 23), "random", device)
    if path == "composed":
        monkeypatch.setenv("NESVOR_ROBUST", "composed")
    else:
        monkeypatch.delenv("NESVOR_ROBUST", raising=False)
    rs = robust.RobustStatistics().init(sim, y, mask)
    rs.update(sim, y, mask)  # (warm: the library is loaded, the allocator has its blocks)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rs.update(sim, y, mask)
        w, s = rs.weights(), rs.scaled(y)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert w.shape == s.shape == sim.shape and bool(torch.isfinite(rs.model).all())
    with pytest.raises(RuntimeError):  # the check is live: a read does raise under it
        torch.cuda.set_sync_debug_mode("error")
        try:
            rs.model[0].item()
        finally:
            torch.cuda.set_sync_debug_mode(before)


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline on the 48^3 phantom (three still stacks, 1.5 mm pixels, 3 mm slices, as tests/test_srr_fused.py builds them)
# ---------------------------------------------------------------------------------------------------------------------
_RES_S, _THICK, _RES_R = 1.5, 3.0, 1.0
MIN_PIXELS = 200
_STILL = {}


def _still(device):
    """The phantom and its three stacks WITHOUT motion (so the world frame is the phantom's), normalised by the 0.99 quantile
    q of their masked intensities as ``simulate_stacks`` does; built once, never written."""
    if _STILL:
        return _STILL
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=48), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=_RES_S, s_thick=_THICK, motion_deg=0, motion_mm=0, seed=0, normalize=False)
    allv = torch.cat([s.image[s.mask] for s in slices])
    q = torch.kthvalue(allv, max(int(0.99 * allv.numel()), 1)).values
    n = len(slices) // 3
    stacks = [(torch.stack([s.image for s in slices[j * n:(j + 1) * n]]) / q).contiguous() for j in range(3)]
    poses = [RigidTransform.cat([s.transformation for s in slices[j * n:(j + 1) * n]]) for j in range(3)]
    _STILL.update(phantom=vol / q, stacks=stacks, poses=poses, n=n)
    return _STILL


def _psnr(rec, phantom):
    from nesvor_amd.image import Volume
    from nesvor_amd.transform import RigidTransform

    identity = RigidTransform(torch.eye(3, 4, device=phantom.device)[None])
    truth = Volume(phantom, None, identity, 1.0, 1.0, 1.0).sample_points(rec.xyz_masked)
    peak = float(phantom.max())
    return float(10 * torch.log10(peak * peak / ((rec.image[rec.mask].double() - truth.double()) ** 2).mean()))


def _reconstruct_both(stacks, poses):
    from nesvor_amd.svr import reconstruct_volume

    plain = reconstruct_volume(stacks, None, poses, _RES_S, _THICK, _RES_R, n_iter=30, beta=0.02, delta=0.1, robust_rounds=0)
    out = {}
    robust = reconstruct_volume(stacks, None, poses, _RES_S, _THICK, _RES_R, n_iter=30, beta=0.02, delta=0.1, robust_rounds=3,
                                robust_out=out)
    return plain, robust, out


def _by_input_slice(out, stacks):
    """slice weight / scale per concatenated input slice (NaN for the empty ones) and the masked pixel counts."""
    pixels = torch.cat([(s > 0).flatten(1).sum(1) for s in stacks])
    weight = torch.full((pixels.numel(),), float("nan"), device=pixels.device)
    scale = weight.clone()
    weight[out["keep"]], scale[out["keep"]] = out["slice_weight"], out["scale"]
    assert torch.equal(torch.nonzero(pixels > 0).flatten(), out["keep"])
    return weight, scale, pixels


@pytest.mark.gpu
def test_pipeline_rejects_permuted_slices_and_finds_the_stack_gains(device, monkeypatch):
    """Stack 1 times 0.7, stack 2 times 1.3, the masked pixels of three slices permuted: robust statistics end closer to the
    phantom than the plain run, reject the three slices, keep the others and order the stacks' scales by their gains.
    Measured on MI355X: DESIGN.md, "Robust statistics"."""
    monkeypatch.delenv("NESVOR_SRR", raising=False)
    monkeypatch.delenv("NESVOR_ROBUST", raising=False)
    c = _still(device)
    n = c["n"]
    stacks = [c["stacks"][0].clone(), c["stacks"][1] * 0.7, c["stacks"][2] * 1.3]
    g = torch.Generator().manual_seed(5)
    bad = []
    for j, k in ((0, n // 2), (1, n // 2 - 2), (2, n // 2 + 2)):
        img = stacks[j][k]
        on = img > 0
        assert int(on.sum()) >= MIN_PIXELS
        values = img[on]
        img[on] = values[torch.randperm(values.numel(), generator=g).to(device)]
        bad.append(j * n + k)
    plain, robust, out = _reconstruct_both(stacks, c["poses"])
    p_plain, p_robust = _psnr(plain, c["phantom"]), _psnr(robust, c["phantom"])
    weight, scale, pixels = _by_input_slice(out, stacks)
    big = pixels >= MIN_PIXELS
    clean = big.clone()
    clean[bad] = False
    medians = [float(scale[j * n:(j + 1) * n][big[j * n:(j + 1) * n]].median()) for j in range(3)]
    print(f"PSNR inside the mask: plain {p_plain:.3f} dB, robust {p_robust:.3f} dB")
    print("weights", [round(v, 3) for v in weight.tolist()])
    print("scales", [round(v, 3) for v in scale.tolist()])
    print("pixels", pixels.tolist(), "permuted", bad, "median scales per stack", medians)
    assert p_robust > p_plain
    assert all(float(weight[k]) < 0.5 for k in bad)
    assert float((weight[clean] > 0.5).double().mean()) >= 0.9
    assert medians[1] > medians[0] > medians[2]


@pytest.mark.gpu
def test_pipeline_keeps_clean_slices(device, monkeypatch):
    """No gain change, no permutation: at least 90 % of the slices with >= 200 pixels keep a weight above 0.5 and the PSNR is
    not below the plain run's minus 0.1 dB (the project's parity margin)."""
    monkeypatch.delenv("NESVOR_SRR", raising=False)
    monkeypatch.delenv("NESVOR_ROBUST", raising=False)
    c = _still(device)
    plain, robust, out = _reconstruct_both(c["stacks"], c["poses"])
    p_plain, p_robust = _psnr(plain, c["phantom"]), _psnr(robust, c["phantom"])
    weight, scale, pixels = _by_input_slice(out, c["stacks"])
    big = pixels >= MIN_PIXELS
    print(f"PSNR inside the mask: plain {p_plain:.3f} dB, robust {p_robust:.3f} dB")
    print("weights", [round(v, 3) for v in weight.tolist()])
    print("scales", [round(v, 3) for v in scale.tolist()])
    assert float((weight[big] > 0.5).double().mean()) >= 0.9
    assert p_robust >= p_plain - 0.1


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def _moving_stacks(device, tmp_path):
    """The three 48^3-phantom stacks with inter-slice motion of tests/test_svr.py as NIfTI files; also the (stack, slice) pairs of
    the non-empty slices."""
    from nesvor_amd.image import Volume
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=48), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=_RES_S, s_thick=_THICK, motion_deg=2, motion_mm=1, seed=0)
    n = len(slices) // 3
    paths, nonempty = [], []
    for j in range(3):
        ss = slices[j * n:(j + 1) * n]
        img = torch.stack([s.image for s in ss])[:, 0].contiguous()
        nonempty += [(j, k) for k in torch.nonzero((img > 0).flatten(1).any(1)).flatten().tolist()]
        ax = RigidTransform.cat([s.transformation for s in ss]).axisangle().mean(0, keepdim=True)  # stack centre pose
        p = str(tmp_path / f"stack{j}.nii.gz")
        Volume(img, img > 0, RigidTransform(ax), _RES_S, _RES_S, _THICK).save(p, masked=False)
        paths.append(p)
    return paths, nonempty


@pytest.mark.gpu
def test_cli_svr_with_outlier_rejection(tmp_path, device, monkeypatch):
    from nesvor_amd import cli, svr
    from nesvor_amd.image_io import load_volume

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    monkeypatch.delenv("NESVOR_ROBUST", raising=False)
    paths, nonempty = _moving_stacks(device, tmp_path)
    n_nonempty = len(nonempty)
    made = []
    inner = svr.reconstruct_volume

    def spy(*a, **k):
        vol = inner(*a, **k)
        made.append((a, k, vol.image.clone()))  # (the command rescales the volume it gets in place)
        return vol

    monkeypatch.setattr(svr, "reconstruct_volume", spy)
    out, weights, sim = str(tmp_path / "v.nii.gz"), str(tmp_path / "w.json"), str(tmp_path / "sim")
    common = ["svr", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--registration", "none", "--n-iter-srr", "6",
              "--verbose", "0"]
    cli.main(common + ["--output-volume", out, "--outlier-rejection", "--slice-weights", weights, "--simulated-slices", sim])
    assert len(made) == 1 and made[0][1]["robust_rounds"] == 3
    vol = load_volume(out, device=device)
    assert tuple(vol.image.shape) == tuple(made[0][2].shape) and float(vol.image.max()) > 700.0
    rows = json.load(open(weights))
    assert len(rows) == n_nonempty > 30
    assert all(set(r) == {"stack", "slice", "weight", "scale"} for r in rows)
    assert all(0.0 <= r["weight"] <= 1.0 and r["scale"] > 0.0 for r in rows)
    assert all(type(r["stack"]) is int and type(r["slice"]) is int for r in rows)
    assert [(r["stack"], r["slice"]) for r in rows] == nonempty  # every non-empty slice of every input stack, once, in order
    print("rejected", sum(r["weight"] < 0.5 for r in rows), "of", len(rows), "scales",
          min(r["scale"] for r in rows), max(r["scale"] for r in rows))
    assert len([f for f in os.listdir(sim) if f.endswith(".nii.gz")]) == n_nonempty
    # without the flag: the plain pipeline, bit for bit
    plain = str(tmp_path / "plain.nii.gz")
    cli.main(common + ["--output-volume", plain])
    assert len(made) == 2 and "robust_rounds" not in made[1][1] and not os.path.exists(str(tmp_path / "never.json"))
    a, k, image = made[1]
    direct = inner(*a, **k, robust_rounds=0)
    assert torch.equal(direct.image, image)


@pytest.mark.gpu
def test_cli_slice_weights_from_input_slices(tmp_path, device, monkeypatch):
    """``--input-slices`` files carry no stack: ``stack`` is null and ``slice`` the file's place in the folder's numeric order."""
    from nesvor_amd import cli

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    monkeypatch.delenv("NESVOR_ROBUST", raising=False)
    paths, nonempty = _moving_stacks(device, tmp_path)
    folder, out, weights = str(tmp_path / "slices"), str(tmp_path / "v.nii.gz"), str(tmp_path / "w.json")
    cli.main(["register", "--input-stacks", *paths, "--output-slices", folder, "--thicknesses", "3", "3", "3", "--registration", "none",
              "--verbose", "0"])
    cli.main(["svr", "--input-slices", folder, "--output-volume", out, "--n-iter-srr", "3", "--outlier-rejection", "--robust-rounds", "2",
              "--slice-weights", weights, "--verbose", "0"])
    rows = json.load(open(weights))
    assert [r["stack"] for r in rows] == [None] * len(nonempty)
    assert [r["slice"] for r in rows] == list(range(len(nonempty)))
    assert all(0.0 <= r["weight"] <= 1.0 and r["scale"] > 0.0 for r in rows)
