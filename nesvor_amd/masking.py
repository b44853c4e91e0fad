"""Stack masking (``--volume-mask``, ``--stacks-intersection``, ``--background-threshold``, ``--otsu-thresholding``): which voxels
of the input stacks count, decided before anything else looks at them.

Upstream NeSVoR has these four network-free switches in releases after the one this project models; the definitions below are
this module's own.  Stack ``j`` has slices (n_j,1,h_j,w_j), a bool mask (its file mask, or ``> 0`` without one), per-slice poses
``T_{j,s}``, ``resolution_x / y``, ``thickness`` and ``gap``.  Pixel (s, r, c) lies at

    p = transform_points(T_{j,s}, ((c - (w_j - 1) / 2) rx, (r - (h_j - 1) / 2) ry, 0))

(the lattice of ``Image.xyz_masked_untransformed``), evaluated in float64.  The mask is narrowed in this order; every step only
removes voxels:

1. background threshold T: keep ``image > T`` (a NaN is dropped);
2. volume mask: a (D,H,W) 0 / 1 array on a posed lattice (``load_volume``; ``> 0`` counts as 1): keep a voxel if the trilinear
   interpolation of the array at p is ``>= 0.5``; off the lattice the array is 0 (as in ``Volume.sample_points``: a point up to
   one voxel outside still interpolates against that 0).  With ``u = local / resolution + (shape - 1) / 2`` the continuous voxel
   index of p, the eight corners ``floor(u) + {0,1}^3`` are weighted by the products of ``1 - frac`` / ``frac``;
3. stacks intersection: keep a voxel of stack j only if for every other stack k some slice t of k contains it: with
   ``q = T_{k,t}^{-1} p``, ``|q_x| <= w_k rx_k / 2``, ``|q_y| <= h_k ry_k / 2`` and ``|q_z| <= max(thickness_k, gap_k) / 2``.  The
   slabs are geometry: a slice that is empty under its mask still counts, and moved stacks are handled by their per-slice poses.
   Ignored with a warning when a volume mask is given (upstream's rule) and with one stack;
4. Otsu, per stack, on the voxels kept so far: ``lo`` / ``hi`` their extremes, ``width = (hi - lo) / n_bins``, bin
   ``min(floor((v - lo) / width), n_bins - 1)`` in double with integer counts, centres ``m_i = lo + (i + 0.5) width``; for the
   splits ``i = 0 .. n_bins - 2`` the between-class variance ``w0 w1 (mu0 - mu1)^2`` from the class weights and the class means of
   the centres, in double, the running sums in ascending bin order; the first maximum wins, ``t = float32(m_i)``, keep
   ``image > t``.  Fewer than two kept voxels or ``hi == lo``: ``t = -inf`` (nothing is removed) and a warning.

On HIP fp32 stacks steps 1 to 3 are ONE launch per stack (``torch.ops.nesvor.stack_mask``, csrc/masking.hip: the other stacks'
world-to-slice matrices go through LDS, the per-slice {count, min, max} of the kept intensities come out reproducibly), Otsu is
``otsu_histogram`` + ``otsu_threshold`` and its result goes back into ``stack_mask`` as a device float.  ``NESVOR_MASKING=composed``,
host tensors and other dtypes take the float64 torch expressions ``stack_mask_composed``, ``otsu_histogram_composed`` and
``otsu_threshold_composed`` (same arguments; the yardstick of tests/test_masking.py and tests/test_gpu_masking.py), which loop over
the other stacks' slices with (N,3) temporaries.  Both paths share the tables built here.  The ONE host read per stack is the
report (and with it the test for an emptied stack).
"""
import logging
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

MAX_BINS = 1024  # histogram bins the fused ops take
SWITCHES = ("--background-threshold", "--volume-mask", "--stacks-intersection", "--otsu-thresholding")


def _fused(x: torch.Tensor, n_bins: int) -> bool:
    return os.environ.get("NESVOR_MASKING", "") != "composed" and x.is_cuda and x.dtype == torch.float32 and 2 <= n_bins <= MAX_BINS


# ---------------------------------------------------------------------------------------------------------------------
# tables (shared by both paths)
# ---------------------------------------------------------------------------------------------------------------------
def world_to_local(mat: torch.Tensor) -> torch.Tensor:
    """(n,3,4) poses [R | t] with x' = R (x + t) -> (n,3,4) float64 [R^T | -t]: x = R^T x' - t (exact: a transposition)."""
    m = mat.double()
    return torch.cat([m[:, :, :3].transpose(1, 2), -m[:, :, 3:]], -1).contiguous()


def slab_tables(stacks: Sequence, skip: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The slabs of every stack but ``skip``: (world-to-slice matrices (S,3,4) float64, half-extents (K,3) float64,
    offsets (K + 1) int32 into the matrices)."""
    mats, extents, offsets = [], [], [0]
    for k, st in enumerate(stacks):
        if k == skip:
            continue
        mats.append(world_to_local(st.transformation.matrix(True)))
        h, w = int(st.slices.shape[-2]), int(st.slices.shape[-1])
        extents.append([w * float(st.resolution_x) / 2, h * float(st.resolution_y) / 2, max(float(st.thickness), float(st.gap)) / 2])
        offsets.append(offsets[-1] + int(mats[-1].shape[0]))
    dev = stacks[skip].slices.device
    return (torch.cat(mats, 0).to(dev).contiguous(), torch.tensor(extents, dtype=torch.float64, device=dev),
            torch.tensor(offsets, dtype=torch.int32, device=dev))


def volume_tables(volume, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """A mask ``Volume`` -> (its 0 / 1 array as uint8 (D,H,W), geometry (15) float64: the world-to-lattice matrix (3,4) and
    the voxel sizes {x, y, z})."""
    if volume.image.ndim != 3 or min(volume.image.shape) < 2:
        raise SystemExit(f"--volume-mask: a 3-D mask with at least 2 voxels on every axis expected, got {tuple(volume.image.shape)}")
    mat = volume.transformation.matrix(True)
    if mat.shape[0] != 1:
        raise ValueError("volume mask: one pose expected")
    geom = torch.cat([world_to_local(mat).reshape(12).cpu(),
                      torch.tensor([float(volume.resolution_x), float(volume.resolution_y), float(volume.resolution_z)], dtype=torch.float64)])
    return (volume.image > 0).to(torch.uint8).to(device).contiguous(), geom.to(device)


def pixel_positions(transforms: torch.Tensor, h: int, w: int, rx: float, ry: float) -> torch.Tensor:
    """(n h w, 3) float64: the world positions of all pixels of a stack, slices first."""
    T = transforms.double()
    dev = T.device
    x = (torch.arange(w, dtype=torch.float64, device=dev) - 0.5 * (w - 1)) * rx
    y = (torch.arange(h, dtype=torch.float64, device=dev) - 0.5 * (h - 1)) * ry
    n = T.shape[0]
    a = torch.stack([(x[None, None, :] + T[:, 0, 3, None, None]).expand(n, h, w), (y[None, :, None] + T[:, 1, 3, None, None]).expand(n, h, w),
                     T[:, 2, 3, None, None].expand(n, h, w)], -1)  # (n,h,w,3): x + t
    R = T[:, None, None, :, :3]
    return torch.stack([(R[..., i, 0] * a[..., 0] + R[..., i, 1] * a[..., 1]) + R[..., i, 2] * a[..., 2] for i in range(3)], -1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the composed float64 path (the arguments of the fused ops)
# ---------------------------------------------------------------------------------------------------------------------
def volume_value_composed(p: torch.Tensor, volume: torch.Tensor, geometry: torch.Tensor) -> torch.Tensor:
    """(N) float64: the trilinear interpolation of the 0 / 1 array ``volume`` (D,H,W) at world points p (N,3), 0 off the lattice."""
    g = geometry.double()
    M = g[:12].reshape(3, 4)
    local = p @ M[:, :3].t() + M[:, 3]
    shape_xyz = torch.tensor([volume.shape[2], volume.shape[1], volume.shape[0]], dtype=torch.float64, device=p.device)
    u = local / g[12:15] + 0.5 * (shape_xyz - 1)
    ok = ((u > -1) & (u < shape_xyz)).all(1)
    u = torch.where(ok[:, None], u, torch.zeros_like(u))
    i0 = torch.floor(u)
    f = u - i0
    i0 = i0.long()
    vol = (volume != 0).double()
    acc = torch.zeros(p.shape[0], dtype=torch.float64, device=p.device)
    lim = shape_xyz.long()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                idx = i0 + torch.tensor([dx, dy, dz], device=p.device)
                on = ((idx >= 0) & (idx < lim)).all(1) & ok
                idx = torch.minimum(idx.clamp(min=0), lim - 1)
                wgt = ((f[:, 2] if dz else 1 - f[:, 2]) * (f[:, 1] if dy else 1 - f[:, 1])) * (f[:, 0] if dx else 1 - f[:, 0])
                acc = acc + torch.where(on, vol[idx[:, 2], idx[:, 1], idx[:, 0]] * wgt, torch.zeros_like(wgt))
    return acc


def slab_distance_composed(p: torch.Tensor, slabs: torch.Tensor, extents: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """(N, K) float64: per other stack the largest ``e`` such that p lies inside some slab shrunk by e on every face (negative:
    outside every slab by that much).  ``>= 0`` is the containment test; the tests use the value as the distance to a face."""
    off = [int(o) for o in offsets.tolist()]
    out = []
    for k in range(len(off) - 1):
        best = torch.full((p.shape[0],), -float("inf"), dtype=torch.float64, device=p.device)
        for t in range(off[k], off[k + 1]):  # one slice at a time: the temporaries stay (N,3)
            q = p @ slabs[t, :, :3].t() + slabs[t, :, 3]
            best = torch.maximum(best, (extents[k] - q.abs()).amin(1))
        out.append(best)
    return torch.stack(out, 1) if out else torch.zeros((p.shape[0], 0), dtype=torch.float64, device=p.device)


def slice_stats_composed(slices: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """(n,3) float64 {count, min, max} of the kept intensities per slice (+inf / -inf without one; a NaN enters neither)."""
    n = slices.shape[0]
    v, k = slices.reshape(n, -1).double(), keep.reshape(n, -1)
    real = k & ~torch.isnan(v)
    inf = torch.full_like(v, float("inf"))
    return torch.stack([k.sum(1).double(), torch.where(real, v, inf).amin(1), torch.where(real, v, -inf).amax(1)], 1)


def stack_mask_composed(slices, mask, transforms, resolution_x, resolution_y, threshold=None, volume=None, volume_geometry=None,
                        slabs=None, slab_extents=None, slab_offsets=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Steps 1 to 3 as float64 torch expressions, with the arguments of ``torch.ops.nesvor.stack_mask``:
    -> (mask uint8 of the shape of ``slices``, stats (n,3) float64)."""
    n, h, w = int(slices.shape[0]), int(slices.shape[-2]), int(slices.shape[-1])
    keep = torch.ones(slices.shape, dtype=torch.bool, device=slices.device) if mask is None else mask.reshape(slices.shape) != 0
    if threshold is not None:
        keep = keep & (slices > threshold.to(slices.dtype).reshape(()))
    has_slabs = slab_offsets is not None and slab_offsets.numel() > 1
    if volume is not None or has_slabs:
        p = pixel_positions(transforms, h, w, float(resolution_x), float(resolution_y))
        if volume is not None:
            keep = keep & (volume_value_composed(p, volume, volume_geometry) >= 0.5).reshape(slices.shape)
        if has_slabs:
            keep = keep & (slab_distance_composed(p, slabs, slab_extents, slab_offsets) >= 0).all(1).reshape(slices.shape)
    return keep.to(torch.uint8), slice_stats_composed(slices, keep)


def otsu_histogram_composed(slices: torch.Tensor, mask: Optional[torch.Tensor], rng: torch.Tensor, n_bins: int) -> torch.Tensor:
    """(n_bins) int64: the counts of the kept intensities between rng = {lo, hi} (float64)."""
    v = slices.reshape(-1).double()
    keep = torch.ones_like(v, dtype=torch.bool) if mask is None else mask.reshape(-1) != 0
    lo, hi = rng.double()[0], rng.double()[1]
    c = (v - lo) / ((hi - lo) / n_bins)
    counted = keep & (c >= 0)
    b = torch.where(counted, torch.floor(c).clamp(max=n_bins - 1), torch.zeros_like(c)).long()
    return torch.zeros(n_bins, dtype=torch.int64, device=v.device).index_add_(0, b, counted.long())


def otsu_threshold_composed(hist: torch.Tensor, rng: torch.Tensor) -> torch.Tensor:
    """(1) float32: Otsu's threshold of an integer histogram over rng = {lo, hi}; -inf where it is not defined."""
    n_bins = int(hist.shape[0])
    lo, hi = rng.double()[0], rng.double()[1]
    width = (hi - lo) / n_bins
    i = torch.arange(n_bins, dtype=torch.float64, device=hist.device)
    centres = lo + (i + 0.5) * width
    cnt = hist.double()
    cum_n, cum_s = torch.cumsum(cnt, 0), torch.cumsum(cnt * centres, 0)
    total_n, total_s = cum_n[-1], cum_s[-1]
    n0, n1 = cum_n[:-1], total_n - cum_n[:-1]
    both = (n0 > 0) & (n1 > 0)
    d = cum_s[:-1] / n0.clamp(min=1) - (total_s - cum_s[:-1]) / n1.clamp(min=1)
    var = torch.where(both, ((n0 / total_n) * (n1 / total_n)) * (d * d), torch.zeros_like(d))
    var = torch.nan_to_num(var, nan=0.0)
    first = torch.where(var == var.max(), i[:-1], torch.full_like(var, float(n_bins))).min()  # the first maximum, no host read
    t = lo + (first + 0.5) * width
    usable = (total_n >= 2) & (hi > lo)
    return torch.where(usable, t, torch.full_like(t, -float("inf"))).float().reshape(1)


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
def _paths(fused: bool):
    if fused:
        ops = torch.ops.nesvor
        return ops.stack_mask, ops.otsu_histogram, ops.otsu_threshold
    return stack_mask_composed, otsu_histogram_composed, otsu_threshold_composed


def stack_range(stats: torch.Tensor) -> torch.Tensor:
    """{lo, hi} float64 of a stack from its per-slice stats; on the device."""
    return torch.stack([stats[:, 1].min(), stats[:, 2].max()])


def _blame(rule, slices, mask, transforms, rx, ry, steps) -> str:
    """The first rule after which no voxel is left (the slow way, one rule at a time: only on the way to the exit)."""
    if not bool(mask.any()):
        return "its own mask (--stack-masks, or no positive voxel)"
    for name, kw in steps:
        mask, _ = rule(slices, mask, transforms, rx, ry, **kw)
        if not bool(mask.any()):
            return name
    return SWITCHES[3]


def mask_stacks(stacks: List, *, volume_mask=None, stacks_intersection: bool = False, background_threshold: Optional[float] = None,
                otsu_thresholding: bool = False, n_bins_otsu: int = 256, names: Optional[Sequence[str]] = None) -> List[Dict]:
    """Narrows ``stack.mask`` of every ``Stack`` in place by the rules of the module docstring; ``volume_mask`` is a ``Volume``
    (``load_volume``).  Returns one report per stack: ``slices_before`` / ``slices_after`` (non-empty slices), ``voxels_before`` /
    ``voxels_after``, ``kept_share``, ``otsu_threshold`` (None without Otsu, -inf where it was not defined) and ``fused``.  A stack
    left without a voxel ends the program (``SystemExit``) naming the stack and the switch that emptied it."""
    if otsu_thresholding and not 2 <= int(n_bins_otsu):
        raise SystemExit("--n-bins-otsu: at least 2 bins expected")
    if stacks_intersection and volume_mask is not None:
        logging.warning("--stacks-intersection is ignored: --volume-mask is given")
        stacks_intersection = False
    if stacks_intersection and len(stacks) < 2:
        logging.warning("--stacks-intersection is ignored: it needs more than one stack")
        stacks_intersection = False
    reports = []
    results = []
    for j, st in enumerate(stacks):
        slices = st.slices if st.slices.is_floating_point() else st.slices.float()
        slices = slices.contiguous()
        dev = slices.device
        fused = _fused(slices, int(n_bins_otsu))
        rule, histogram, otsu = _paths(fused)
        transforms = st.transformation.matrix(True).to(torch.float32).contiguous()
        rx, ry = float(st.resolution_x), float(st.resolution_y)
        before = (st.mask != 0).contiguous()
        steps = []  # (switch, keyword arguments of its rule)
        if background_threshold is not None:
            steps.append((SWITCHES[0], {"threshold": torch.tensor([float(background_threshold)], dtype=torch.float32, device=dev)}))
        if volume_mask is not None:
            vol, geom = volume_tables(volume_mask, dev)
            steps.append((SWITCHES[1], {"volume": vol, "volume_geometry": geom}))
        if stacks_intersection:
            slabs, extents, offsets = slab_tables(stacks, j)
            steps.append((SWITCHES[2], {"slabs": slabs, "slab_extents": extents, "slab_offsets": offsets}))
        kw = {"threshold": None, "volume": None, "volume_geometry": None, "slabs": None, "slab_extents": None, "slab_offsets": None}
        for _, step in steps:
            kw.update(step)
        new, stats = rule(slices, before, transforms, rx, ry, *kw.values())
        t = None
        if otsu_thresholding:
            rng = stack_range(stats)
            t = otsu(histogram(slices, new, rng, int(n_bins_otsu)), rng)
            new, stats = rule(slices, new, transforms, rx, ry, t, None, None, None, None, None)
        count_before = before.reshape(before.shape[0], -1).sum(1)
        packed = torch.stack([(count_before > 0).sum().double(), count_before.sum().double(), (stats[:, 0] > 0).sum().double(),
                              stats[:, 0].sum(), (t.double()[0] if t is not None else torch.zeros((), dtype=torch.float64, device=dev))])
        results.append((new, packed, fused, (rule, slices, before, transforms, rx, ry, steps)))
    for j, (st, (new, packed, fused, blame)) in enumerate(zip(stacks, results)):
        s0, v0, s1, v1, t = packed.tolist()  # the one host read of the stack
        name = names[j] if names is not None else f"stack {j}"
        if v1 == 0:
            raise SystemExit(f"Stack masking left no voxel of {name}: emptied by {_blame(*blame)}")
        if otsu_thresholding and t == -float("inf"):
            logging.warning("--otsu-thresholding: %s has fewer than two voxels or one intensity only; nothing is thresholded", name)
        st.mask = new.reshape(st.mask.shape).to(torch.bool)
        reports.append({"slices_before": int(s0), "slices_after": int(s1), "voxels_before": int(v0), "voxels_after": int(v1),
                        "kept_share": v1 / v0 if v0 else 0.0, "otsu_threshold": t if otsu_thresholding else None, "fused": fused})
        logging.info("Stack masking, %s: %d -> %d voxels (%.1f %%), %d -> %d non-empty slices%s (%s path)", name, int(v0), int(v1),
                     100 * reports[-1]["kept_share"], int(s0), int(s1),
                     f", Otsu threshold {t:.6g}" if otsu_thresholding else "", "fused" if fused else "composed")
    return reports
