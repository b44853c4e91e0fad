"""Structural exclusion on the GPU: the SSIM kernel (csrc/structural.hip) against the torch expression in fp64, its refusals, the
fused update against the composed one, ``reconstruct_volume(structural=...)`` on the 48^3 phantom and the command line."""
import json
import math

import pytest
import torch

from test_gpu_robust import MIN_PIXELS, _RES_R, _RES_S, _THICK, _data, _moving_stacks, _psnr, _still, _ulp

# (n, h, w): a single pixel; smaller than the window's radius both ways; exactly one tile; one pixel past a tile edge both ways
# with three tiles across; 2 x 2 ragged tiles without a mask, with a random one, and with that and an empty slice
CASES = [((1, 1, 1), "none"), ((1, 5, 5), "random"), ((3, 16, 16), "random"), ((2, 17, 33), "random"),
         ((5, 19, 23), "none"), ((5, 19, 23), "random"), ((5, 19, 23), "slice")]
T_LOCAL = 0.4
NAMES = ("n", "sum ssim", "#(ssim < t)", "sum I", "sum J", "sum I^2", "sum J^2", "sum I J")


def _three(sim, y, mask, scale):
    """(map, sums) of the expression in fp64, of the expression in fp32 and of the kernel; and d, the map error the rule
    allows the kernel: twice the fp32 expression's plus one fp32 ulp of the largest magnitude."""
    from nesvor_amd.structural import ssim_composed

    m64, s64 = ssim_composed(sim.double(), y.double(), mask, scale.double(), T_LOCAL, 1.0)
    m32, s32 = ssim_composed(sim, y, mask, scale, T_LOCAL, 1.0)
    m, s = torch.ops.nesvor.structural_ssim(sim, y, mask, scale, T_LOCAL, 1.0)
    d = 2 * float((m32.double() - m64).abs().max()) + _ulp(m64.abs().max())
    return (m64, s64), (m32, s32), (m, s), d


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", CASES)
def test_ssim_against_the_torch_expression_in_fp64(device, shape, kind):
    """For the map and each of the six float sums the kernel's largest error against the fp64 expression is at most twice that
    of the same expression evaluated per pixel in fp32 (its sums in fp64) plus one fp32 ulp of the largest magnitude; n is exact,
    the count below the threshold lies between the fp64 counts at t - d and t + d (d the allowed map error) and the map is
    exactly 0 off the mask.  Measured on MI355X (largest over the cases): DESIGN.md, "Structural exclusion"."""
    sim, y, mask, scale = _data(shape, kind, device)
    n = shape[0]
    (m64, s64), (m32, s32), (m, s), d = _three(sim, y, mask, scale)
    valid = torch.ones_like(sim, dtype=torch.bool) if mask is None else mask
    assert m.shape == sim.shape and m.dtype == torch.float32 and s.shape == (n, 8) and s.dtype == torch.float64
    assert torch.equal(s[:, 0], valid.flatten(1).sum(1).double())
    assert bool((m[~valid] == 0).all())
    if kind == "slice":
        assert bool((s[1] == 0).all())
    err_k, err_c = float((m.double() - m64).abs().max()), float((m32.double() - m64).abs().max())
    print(f"{shape} {kind}: map kernel {err_k:.3e} composed {err_c:.3e} allowed {d:.3e} (bit-equal to composed: {torch.equal(m, m32)})")
    assert err_k <= d
    low = (valid & (m64 < T_LOCAL - d)).flatten(1).sum(1).double()
    high = (valid & (m64 < T_LOCAL + d)).flatten(1).sum(1).double()
    print(f"    {NAMES[2]}: kernel {s[:, 2].tolist()} between {low.tolist()} and {high.tolist()}")
    assert bool((low <= s[:, 2]).all()) and bool((s[:, 2] <= high).all())
    for j in (1, 3, 4, 5, 6, 7):
        err_k, err_c = float((s[:, j] - s64[:, j]).abs().max()), float((s32[:, j] - s64[:, j]).abs().max())
        ulp = _ulp(s64[:, j].abs().max())
        print(f"    {NAMES[j]}: kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e} (largest {float(s64[:, j].abs().max()):.4e})")
        assert err_k <= 2 * err_c + ulp, NAMES[j]
    again_m, again_s = torch.ops.nesvor.structural_ssim(sim, y, mask, scale, T_LOCAL, 1.0)
    assert torch.equal(again_m, m) and torch.equal(again_s, s)


@pytest.mark.gpu
def test_ssim_takes_a_byte_mask_and_flat_slices(device):
    sim, y, mask, scale = _data((5, 19, 23), "random", device)
    m, s = torch.ops.nesvor.structural_ssim(sim, y, mask, scale, T_LOCAL, 1.0)
    m8, s8 = torch.ops.nesvor.structural_ssim(sim[:, 0], y[:, 0], mask[:, 0].to(torch.uint8), scale, T_LOCAL, 1.0)
    assert m8.shape == (5, 19, 23) and torch.equal(m8, m[:, 0]) and torch.equal(s8, s)
    meta = torch.ops.nesvor.structural_ssim(sim.to("meta"), y.to("meta"), None, scale.to("meta"), T_LOCAL, 1.0)
    assert meta[0].shape == sim.shape and meta[0].dtype == torch.float32 and meta[0].device.type == "meta"
    assert meta[1].shape == (5, 8) and meta[1].dtype == torch.float64


@pytest.mark.gpu
def test_ssim_refusals(device):
    """Every refusal returns before a launch (csrc/structural.hip: the checks are the first statements of
    nesvor_structural_ssim), so the sentinels in the map and the sums stay."""
    from nesvor_amd import _lib

    lib = _lib.load()
    n, h, w = 5, 19, 23
    sim, y, mask, scale = _data((n, h, w), "random", device)
    out = torch.full((n, h, w), -7.0, device=device)
    stats = torch.full((n, 8), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_structural_ssim_workspace_bytes(n, h, w))
    assert nbytes == 8 * 8 * n * 4  # 2 x 2 tiles per slice
    assert lib.nesvor_structural_ssim_workspace_bytes(0, h, w) == 0 and lib.nesvor_structural_ssim_workspace_bytes(n, 0, w) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    P = _lib.ptr
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def call(n_=n, h_=h, w_=w, sim_=sim, y_=y, scale_=scale, out_=out, stats_=stats, ws_=ws, nb=nbytes, c1_=c1, c2_=c2, t_=T_LOCAL):
        return lib.nesvor_structural_ssim(P(sim_), P(y_), P(mask), P(scale_), n_, h_, w_, c1_, c2_, t_, P(out_), P(stats_), P(ws_), nb,
                                          _lib.stream_ptr())

    assert call(nb=nbytes - 1) != 0 and call(nb=0) != 0 and call(ws_=None) != 0  # a short or missing workspace
    assert call(n_=-1) != 0 and call(h_=0) != 0 and call(w_=0) != 0 and call(w_=-3) != 0
    assert call(h_=65536, w_=65536) != 0 and call(h_=1, w_=2 ** 31 - 256) != 0  # h w > INT_MAX - 256
    for name in ("sim_", "y_", "scale_", "out_", "stats_"):
        assert call(**{name: None}) != 0
    for name in ("c1_", "c2_", "t_"):
        for bad in (-1e-3, float("inf"), float("-inf"), float("nan")):
            assert call(**{name: bad}) != 0, (name, bad)
    assert call(n_=0) == 0 and call(n_=0, ws_=None, nb=0) == 0  # no slices: a no-op
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((stats == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    direct = torch.ops.nesvor.structural_ssim(sim, y, mask, scale, T_LOCAL, 1.0)
    assert torch.equal(out.view_as(sim), direct[0]) and torch.equal(stats, direct[1])
    empty = torch.ops.nesvor.structural_ssim(sim[:0], y[:0], None, scale[:0], T_LOCAL, 1.0)
    assert empty[0].shape == (0, 1, h, w) and empty[1].shape == (0, 8)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::structural_ssim'"):
        torch.ops.nesvor.structural_ssim(sim.cpu(), y.cpu(), mask.cpu(), scale.cpu(), T_LOCAL, 1.0)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.structural_ssim(sim.double(), y.double(), mask, scale.double(), T_LOCAL, 1.0)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.structural_ssim(sim, y, mask, scale.double(), T_LOCAL, 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.nesvor.structural_ssim(sim.transpose(-1, -2), y.transpose(-1, -2), None, scale, T_LOCAL, 1.0)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        torch.ops.nesvor.structural_ssim(sim, y, mask.float(), scale, T_LOCAL, 1.0)
    with pytest.raises(RuntimeError, match="one shape"):
        torch.ops.nesvor.structural_ssim(sim, y[:4].contiguous(), mask, scale, T_LOCAL, 1.0)
    with pytest.raises(RuntimeError, match="scale"):
        torch.ops.nesvor.structural_ssim(sim, y, mask, scale[:4].contiguous(), T_LOCAL, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the update on both paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fused_update_follows_the_composed_one(device, monkeypatch):
    """On the (5,19,23) case with its random mask: the slice correlations of the fused path within 1e-5 of the composed ones (in
    fp32 and in fp64), the same slices kept, and the pixel decisions differ from fp64's only where ssim64 is within the allowed
    map error of the threshold."""
    from nesvor_amd import structural

    sim, y, mask, scale = _data((5, 19, 23), "random", device)
    calls = []
    inner = structural.ssim_composed
    monkeypatch.setattr(structural, "ssim_composed", lambda *a: calls.append(1) or inner(*a))
    monkeypatch.delenv("NESVOR_STRUCTURAL", raising=False)
    fused = structural.StructuralExclusion().update(sim, y, mask, scale)
    assert not calls  # the fused path never evaluates the torch expression
    monkeypatch.setenv("NESVOR_STRUCTURAL", "composed")
    composed = structural.StructuralExclusion().update(sim, y, mask, scale)
    assert len(calls) == 1
    monkeypatch.delenv("NESVOR_STRUCTURAL")
    exact = structural.StructuralExclusion().update(sim.double(), y.double(), mask, scale.double())
    assert len(calls) == 2 and exact.ssim.dtype == torch.float64 and fused.ssim.dtype == composed.ssim.dtype == torch.float32
    d = 2 * float((composed.ssim.double() - exact.ssim).abs().max()) + _ulp(exact.ssim.abs().max())
    print(f"ncc fused {fused.ncc.tolist()} gaps: composed {float((fused.ncc - composed.ncc).abs().max()):.3e} "
          f"fp64 {float((fused.ncc - exact.ncc).abs().max()):.3e}; shares {fused.pixel_share().tolist()}; d {d:.3e}")
    assert fused.ncc.dtype == torch.float64
    assert float((fused.ncc - composed.ncc).abs().max()) <= 1e-5 and float((fused.ncc - exact.ncc).abs().max()) <= 1e-5
    assert torch.equal(fused.slice_keep, composed.slice_keep) and torch.equal(fused.slice_keep, exact.slice_keep)
    near = (exact.ssim - T_LOCAL).abs() <= d
    for other in (fused, composed):
        assert not bool(((other.pixel_keep != exact.pixel_keep) & ~near).any())
    assert torch.equal(fused.weights(), (fused.pixel_keep & fused.slice_keep.view(-1, 1, 1, 1)).float())


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_an_update_reads_nothing_back_to_the_host(device, monkeypatch, path):
    """``update`` under torch's synchronisation check: any read of a device value (``.item()``, ``nonzero``, a blocking copy)
    raises there."""
    from nesvor_amd import structural

    sim, y, mask, scale = _data((5, 19, 23), "random", device)
    if path == "composed":
        monkeypatch.setenv("NESVOR_STRUCTURAL", "composed")
    else:
        monkeypatch.delenv("NESVOR_STRUCTURAL", raising=False)
    se = structural.StructuralExclusion()
    se.update(sim, y, mask, scale)  # (warm: the library is loaded, the allocator has its blocks)
    se.update(sim, y, mask)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        se.update(sim, y, mask, scale)
        w, share = se.weights(), se.pixel_share()
        se.update(sim, y, None)
        w_none = se.weights()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert w.shape == w_none.shape == sim.shape and share.shape == (5,) and bool(torch.isfinite(se.ncc).all())
    with pytest.raises(RuntimeError):  # the check is live: a read does raise under it
        torch.cuda.set_sync_debug_mode("error")
        try:
            se.ncc[0].item()
        finally:
            torch.cuda.set_sync_debug_mode(before)


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline on the 48^3 phantom (the three still stacks of tests/test_gpu_robust.py)
# ---------------------------------------------------------------------------------------------------------------------
def _reconstruct_both(stacks, poses):
    from nesvor_amd.structural import StructuralExclusion
    from nesvor_amd.svr import reconstruct_volume

    plain = reconstruct_volume(stacks, None, poses, _RES_S, _THICK, _RES_R, n_iter=30, beta=0.02, delta=0.1)
    out = {}
    structural = reconstruct_volume(stacks, None, poses, _RES_S, _THICK, _RES_R, n_iter=30, beta=0.02, delta=0.1, robust_rounds=0,
                                    structural=StructuralExclusion(), structural_out=out)
    return plain, structural, out


def _by_input_slice(out, stacks):
    """slice_keep / ncc / pixel_share per concatenated input slice (False / NaN for the empty ones) and the masked pixel counts."""
    pixels = torch.cat([(s > 0).flatten(1).sum(1) for s in stacks])
    assert torch.equal(torch.nonzero(pixels > 0).flatten(), out["keep"])
    kept = torch.zeros(pixels.numel(), dtype=torch.bool, device=pixels.device)
    ncc = torch.full((pixels.numel(),), float("nan"), dtype=torch.float64, device=pixels.device)
    share = ncc.clone()
    kept[out["keep"]], ncc[out["keep"]], share[out["keep"]] = out["slice_keep"], out["ncc"], out["pixel_share"]
    return kept, ncc, share, pixels


@pytest.mark.gpu
def test_pipeline_excludes_permuted_slices(device, monkeypatch):
    """The masked pixels of three slices permuted: structural exclusion alone ends closer to the phantom than the plain run,
    excludes the three slices and keeps at least 90 % of the others with >= 200 pixels.  Measured on MI355X: DESIGN.md,
    "Structural exclusion"."""
    monkeypatch.delenv("NESVOR_SRR", raising=False)
    monkeypatch.delenv("NESVOR_STRUCTURAL", raising=False)
    c = _still(device)
    n = c["n"]
    stacks = [s.clone() for s in c["stacks"]]
    g = torch.Generator().manual_seed(5)
    bad = []
    for j, k in ((0, n // 2), (1, n // 2 - 2), (2, n // 2 + 2)):
        img = stacks[j][k]
        on = img > 0
        assert int(on.sum()) >= MIN_PIXELS
        values = img[on]
        img[on] = values[torch.randperm(values.numel(), generator=g).to(device)]
        bad.append(j * n + k)
    plain, structural, out = _reconstruct_both(stacks, c["poses"])
    p_plain, p_structural = _psnr(plain, c["phantom"]), _psnr(structural, c["phantom"])
    kept, ncc, share, pixels = _by_input_slice(out, stacks)
    clean = pixels >= MIN_PIXELS
    clean[bad] = False
    print(f"PSNR inside the mask: plain {p_plain:.3f} dB, structural {p_structural:.3f} dB")
    print("ncc", [round(v, 3) for v in ncc.tolist()])
    print("pixel share", [round(v, 3) for v in share.tolist()])
    print("pixels", pixels.tolist(), "permuted", bad, "kept", kept.tolist())
    print(f"kept clean slices {float(kept[clean].double().mean()):.3f}, their pixel share: mean {float(share[clean & kept].mean()):.4f} "
          f"min {float(share[clean & kept].min()):.4f}")
    assert not any(bool(kept[k]) for k in bad)
    assert float(kept[clean].double().mean()) >= 0.9
    assert p_structural > p_plain


@pytest.mark.gpu
def test_pipeline_keeps_clean_slices(device, monkeypatch):
    """No permutation: at least 90 % of the slices with >= 200 pixels are kept and the PSNR is not below the plain run's minus
    0.1 dB (the project's parity margin)."""
    monkeypatch.delenv("NESVOR_SRR", raising=False)
    monkeypatch.delenv("NESVOR_STRUCTURAL", raising=False)
    c = _still(device)
    plain, structural, out = _reconstruct_both(c["stacks"], c["poses"])
    p_plain, p_structural = _psnr(plain, c["phantom"]), _psnr(structural, c["phantom"])
    kept, ncc, share, pixels = _by_input_slice(out, c["stacks"])
    big = pixels >= MIN_PIXELS
    print(f"PSNR inside the mask: plain {p_plain:.3f} dB, structural {p_structural:.3f} dB")
    print("ncc", [round(v, 3) for v in ncc.tolist()])
    print("pixel share", [round(v, 3) for v in share.tolist()])
    print(f"kept slices {float(kept[big].double().mean()):.3f}, their pixel share: mean {float(share[big & kept].mean()):.4f} "
          f"min {float(share[big & kept].min()):.4f}")
    assert float(kept[big].double().mean()) >= 0.9
    assert p_structural >= p_plain - 0.1


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_svr_with_structural_exclusion(tmp_path, device, monkeypatch):
    from nesvor_amd import cli, svr
    from nesvor_amd.structural import StructuralExclusion

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    monkeypatch.delenv("NESVOR_ROBUST", raising=False)
    monkeypatch.delenv("NESVOR_STRUCTURAL", raising=False)
    paths, nonempty = _moving_stacks(device, tmp_path)
    made = []
    inner = svr.reconstruct_volume

    def spy(*a, **k):
        vol = inner(*a, **k)
        made.append((a, k, vol.image.clone()))  # (the command rescales the volume it gets in place)
        return vol

    monkeypatch.setattr(svr, "reconstruct_volume", spy)
    out, weights = str(tmp_path / "v.nii.gz"), str(tmp_path / "w.json")
    common = ["svr", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--registration", "none", "--n-iter-srr", "6",
              "--verbose", "0", "--output-volume", out]
    cli.main(common + ["--structural-exclusion", "--slice-weights", weights])
    assert len(made) == 1 and isinstance(made[0][1]["structural"], StructuralExclusion) and made[0][1]["robust_rounds"] == 0
    assert made[0][1]["structural"].rounds == 3 and made[0][1]["structural"].local_ssim == 0.4 and made[0][1]["structural"].global_ncc == 0.5
    rows = json.load(open(weights))
    assert len(rows) == len(nonempty) > 30
    assert all(set(r) == {"stack", "slice", "ncc", "pixel_share", "excluded"} for r in rows)
    assert all(abs(r["ncc"]) <= 1.0 + 1e-9 and 0.0 <= r["pixel_share"] <= 1.0 and type(r["excluded"]) is bool for r in rows)
    assert all(r["excluded"] == (not r["ncc"] >= 0.5) for r in rows) and not any(math.isnan(r["ncc"]) for r in rows)
    assert [(r["stack"], r["slice"]) for r in rows] == nonempty  # every non-empty slice of every input stack, once, in order
    print("excluded", sum(r["excluded"] for r in rows), "of", len(rows), "smallest ncc", min(r["ncc"] for r in rows))
    # both switches: the rows carry both sets
    cli.main(common + ["--structural-exclusion", "--outlier-rejection", "--robust-rounds", "2", "--slice-weights", weights,
                       "--local-ssim-threshold", "0.3", "--global-ncc-threshold", "0.6"])
    assert len(made) == 2 and made[1][1]["robust_rounds"] == 2
    assert made[1][1]["structural"].local_ssim == 0.3 and made[1][1]["structural"].global_ncc == 0.6
    rows = json.load(open(weights))
    assert all(set(r) == {"stack", "slice", "weight", "scale", "ncc", "pixel_share", "excluded"} for r in rows)
    assert [(r["stack"], r["slice"]) for r in rows] == nonempty
    assert all(0.0 <= r["weight"] <= 1.0 and r["scale"] > 0.0 for r in rows)
    # without the switch: today's call, and the plain pipeline bit for bit
    cli.main(common)
    assert len(made) == 3 and "structural" not in made[2][1] and "structural_out" not in made[2][1] and "robust_rounds" not in made[2][1]
    a, k, image = made[2]
    direct = inner(*a, **k)
    assert torch.equal(direct.image, image)
