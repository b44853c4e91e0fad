"""Rigid alignment for the ``evaluate`` command (``--align``): the rigid correction of the input volume's pose that maximises its
correlation with the reference over the voxels both cover, found before the comparison of nesvor_amd/evaluate.py runs.  Without
it ``evaluate`` measures the misalignment of two volumes that do not share a world frame (a ground truth, another tool's output,
a run with another ``--template-stack``), not the reconstruction.  The reference project has no counterpart: the definition is
this module's.

Definition.  R is the reference ``Volume`` and X the input ``Volume``, as in evaluate.py.

Pose parameters.  theta = (rotation vector in degrees (3), translation in mm (3)).  c is the centroid of R's mask in world
coordinates, computed once in float64 (the one extra host read).  The correction G(theta): p -> c + Rot(theta)(p - c) + t takes
reference world coordinates to the input's world coordinates; Rot is Rodrigues' formula in float64 on the host.

Index map.  M(theta) = ``evaluate.index_map(R', X)`` where R' is R with the pose G o T_R (world = R_R (p + t_R)):
    R' = Rot R_R,      t' = t_R + R'^T (c - Rot c + t),
composed exactly so: at theta = 0 Rot is the identity, every product with it and every sum with 0 is exact, and M(0) equals
``index_map(R, X)`` bit for bit.

Moments.  For one index map the moments are the resampler's own over its own validity rule (v = maskR and inside and
mX >= 0.5; u in double, lerps and products in the images' dtype): {n, sum I, sum J, sum I^2, sum J^2, sum I J} are entries
0, 2, 3, 4, 5, 6 of ``evaluate.resample_composed``'s sums.

Loss.  L = 1 - r with r as ``evaluate.fit_from_sums`` defines it (0 at a degenerate variance product).  A pose whose n is below
half of n0, the count at the pose with which the level starts, has L = +inf: the descent cannot walk the volumes apart.  Inside a
difference quotient +inf counts as 2 (the largest finite loss).

Pyramid.  Level 0 is the two volumes as they are.  Level l > 0 of a volume: ``image * mask`` and the mask as float are blurred
with ``utils.gaussian_blur`` (sigma = 0.5 2^l voxels per axis, truncated 4), both are resampled with ``registration.resample`` to
voxels 2^l times as large, and the mask is ``>= 0.5``.  The pose is unchanged, the voxel sizes are multiplied by 2^l.  A level is
used only if every axis of both volumes keeps at least 12 samples at it; ``levels`` (3) is the most that are used.  This is
torch, once per level: not the hot path.

Descent (host floats, decisions in float64 Python; ``registration.VVR``'s scheme).  Levels run from coarse to fine.  Per level
there are ``rounds`` = 6 rounds; the step length s starts at ``step`` 2^l (``step`` = 1.0, degrees and mm alike) and halves from
round to round.  A round makes up to ``max_iter`` = 30 moves: g_j = L(theta + s e_j) - L(theta - s e_j) over the free parameters
(all six for ``rigid``, the translation for ``translation``), the trial pose theta - s g / (|g| + 1e-12) is accepted only if its
loss is strictly smaller, and the first rejection ends the round.
The first call of a level evaluates its start pose alone (K = 1) and gives n0; each step is then one launch with the 12 (6)
perturbed poses and one with the trial pose, and the current loss is carried over from the accepted trial - which is why a
pose's sums must not depend on what else is in the call (csrc/evaluate.hip keeps that promise bit for bit).  Each launch ends in
ONE host read of its (K, 6) sums.

Acceptance.  After level 0 the result is kept only if r(theta*) > r(0) at level 0; otherwise theta = 0 with a warning, and the
comparison that follows is bit-identical to ``--align none`` because M(0) is the old map.  If R and X share no voxel at
theta = 0 on the coarsest level used, the alignment is skipped (theta = 0; the command gives its "shares no voxel" warning).

Afterwards ``evaluate.compare_tensors`` runs unchanged with M(theta*).

Two paths.  On HIP fp32 tensors ``pose_moments`` is ``torch.ops.nesvor.volume_pose_moments`` (csrc/evaluate.hip: up to 16 poses
in one pass over R); ``NESVOR_EVALUATE=composed``, host tensors and other dtypes take ``pose_moments_composed``, one
``resample_composed`` per pose - the choice is ``evaluate._fused``'s.
"""
import logging
import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import torch

from . import evaluate as _ev
from .structural import MIN_VAR_PRODUCT

DOFS = {"rigid": (0, 1, 2, 3, 4, 5), "translation": (3, 4, 5)}
MAX_POSES = 16  # index maps per launch of the fused path (EVALUATE_MAX_POSES of nesvor_amd/ops.py)
MIN_SAMPLES = 12  # per axis, of both volumes, for a pyramid level to be used
_MOMENTS = (0, 2, 3, 4, 5, 6)  # of resample_composed's eight sums


# ---------------------------------------------------------------------------------------------------------------------
# poses and index maps
# ---------------------------------------------------------------------------------------------------------------------
def rotation(rotvec_deg: Sequence[float]) -> torch.Tensor:
    """Rodrigues: the rotation (3,3) float64 of a rotation vector in degrees; exactly the identity for the zero vector."""
    v = torch.tensor([math.radians(float(a)) for a in rotvec_deg], dtype=torch.float64)
    angle = float(v.norm())
    eye = torch.eye(3, dtype=torch.float64)
    if angle == 0.0:
        return eye
    k = (v / angle).tolist()
    K = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    return eye + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def centroid(reference) -> torch.Tensor:
    """c (3) float64 on the host: the centroid of R's mask in world coordinates (of the whole lattice for an empty mask).  One
    host read."""
    Rr, tr, sr, cr = _ev._geometry(reference)
    mask = reference.mask != 0
    d, h, w = mask.shape
    m = mask.double()
    total = m.sum()
    sums = [(m.sum(dims) * torch.arange(size, dtype=torch.float64, device=m.device)).sum()
            for dims, size in (((0, 1), w), ((0, 2), h), ((1, 2), d))]
    x, y, z, n = torch.stack(sums + [total]).tolist()  # the one host read
    index = torch.tensor([x / n, y / n, z / n], dtype=torch.float64) if n > 0 else cr.clone()
    return Rr @ ((index - cr) * sr + tr)


def correction(theta: Sequence[float], centre: torch.Tensor) -> torch.Tensor:
    """G (4,4) float64: p -> c + Rot (p - c) + t."""
    rot = rotation(theta[:3])
    c = torch.as_tensor(centre, dtype=torch.float64)
    t = torch.tensor([float(v) for v in theta[3:6]], dtype=torch.float64)
    G = torch.eye(4, dtype=torch.float64)
    G[:3, :3] = rot
    G[:3, 3] = (c - rot @ c) + t
    return G


def _posed(volume, R: torch.Tensor, t: torch.Tensor):
    """What ``evaluate._geometry`` reads of a volume, with the pose (R, t) in its place."""
    from .transform import RigidTransform

    return SimpleNamespace(image=SimpleNamespace(shape=tuple(volume.image.shape)),
                           transformation=RigidTransform(torch.cat([R, t[:, None]], 1)[None], trans_first=True),
                           resolution_x=volume.resolution_x, resolution_y=volume.resolution_y, resolution_z=volume.resolution_z)


def pose_maps(reference, volume, thetas, centre) -> torch.Tensor:
    """(K,3,4) float64 on the host: M(theta_k) of the module docstring; ``thetas`` is K rows of six numbers."""
    Rr, tr, _, _ = _ev._geometry(reference)
    maps = []
    for theta in thetas:
        G = correction(theta, centre)
        R1 = G[:3, :3] @ Rr
        t1 = tr + R1.t() @ G[:3, 3]
        maps.append(_ev.index_map(_posed(reference, R1, t1), volume))
    return torch.stack(maps) if maps else torch.zeros((0, 3, 4), dtype=torch.float64)


def aligned_pose(volume, theta: Sequence[float], centre: torch.Tensor):
    """The pose G^-1 o T_X: X's own voxels with it share the reference's world frame (``--output-aligned``)."""
    from .transform import RigidTransform

    Rx, tx, _, _ = _ev._geometry(volume)
    G = correction(theta, centre)
    return RigidTransform(torch.cat([G[:3, :3].t() @ Rx, (tx - Rx.t() @ G[:3, 3])[:, None]], 1)[None], trans_first=True)


# ---------------------------------------------------------------------------------------------------------------------
# the moments of K poses
# ---------------------------------------------------------------------------------------------------------------------
def pose_moments_composed(ref, ref_mask, vol, vol_mask, maps) -> torch.Tensor:
    """(K,6) fp64 on the tensors' device: one ``resample_composed`` per map."""
    rows = [_ev.resample_composed(ref, ref_mask, vol, vol_mask, M)[2][list(_MOMENTS)] for M in torch.as_tensor(maps).reshape(-1, 3, 4)]
    return torch.stack(rows) if rows else torch.zeros((0, 6), dtype=torch.float64, device=ref.device)


def pose_moments(ref, ref_mask, vol, vol_mask, maps) -> torch.Tensor:
    """(K,6) fp64 on the device: {n, sum I, sum J, sum I^2, sum J^2, sum I J} under each of the K index maps (host, (K,3,4))."""
    maps = torch.as_tensor(maps, dtype=torch.float64).reshape(-1, 3, 4)
    if not (_ev._fused(ref) and vol.is_cuda and vol.dtype == torch.float32):
        return pose_moments_composed(ref, ref_mask, vol, vol_mask, maps)
    args = (ref.contiguous(), None if ref_mask is None else ref_mask.contiguous(), vol.contiguous(),
            None if vol_mask is None else vol_mask.contiguous())
    out = [torch.ops.nesvor.volume_pose_moments(*args, maps[k:k + MAX_POSES].reshape(-1).tolist()) for k in range(0, maps.shape[0], MAX_POSES)]
    return out[0] if len(out) == 1 else torch.cat(out) if out else torch.zeros((0, 6), dtype=torch.float64, device=ref.device)


def correlation(sums: Sequence[float]) -> float:
    """r of ``evaluate.fit_from_sums`` from one row {n, sum I, sum J, sum I^2, sum J^2, sum I J} of host floats."""
    n, s_i, s_j, s_ii, s_jj, s_ij = sums
    n_safe = n if n > 0 else 1.0
    mean_i, mean_j = s_i / n_safe, s_j / n_safe
    cov = s_ij / n_safe - mean_i * mean_j
    product = (s_ii / n_safe - mean_i * mean_i) * (s_jj / n_safe - mean_j * mean_j)
    return cov / math.sqrt(product) if product > MIN_VAR_PRODUCT else 0.0


def loss(sums: Sequence[float], n0: float) -> float:
    """1 - r, or +inf for a pose that keeps less than half of the n0 voxels the level started with."""
    return math.inf if sums[0] < 0.5 * n0 else 1.0 - correlation(sums)


# ---------------------------------------------------------------------------------------------------------------------
# the pyramid
# ---------------------------------------------------------------------------------------------------------------------
def usable_levels(reference, volume, levels: int) -> int:
    """How many pyramid levels are used: level l needs size // 2^l >= 12 on every axis of both volumes."""
    smallest = min(min(reference.image.shape), min(volume.image.shape))
    count = 1
    while count < max(int(levels), 1) and smallest // 2 ** count >= MIN_SAMPLES:
        count += 1
    return count


def pyramid_level(volume, level: int, dtype, device):
    """A ``Volume`` at level ``level`` of the module docstring's pyramid (image in ``dtype`` on ``device``, bool mask)."""
    from .image import Volume
    from .registration import resample
    from .utils import gaussian_blur

    image, mask = volume.image.to(device=device, dtype=dtype), (volume.mask != 0).to(device)
    res = [float(volume.resolution_x), float(volume.resolution_y), float(volume.resolution_z)]
    if level > 0:
        f = 2.0 ** level
        both = torch.stack([image * mask.to(dtype), mask.to(dtype)])[:, None]  # (2,1,D,H,W)
        both = resample(gaussian_blur(both, 0.5 * f, truncated=4.0), res, [r * f for r in res])
        image, mask, res = both[0, 0], both[1, 0] >= 0.5, [r * f for r in res]
    return Volume(image.contiguous(), mask.contiguous(), volume.transformation, *res)


# ---------------------------------------------------------------------------------------------------------------------
# the descent
# ---------------------------------------------------------------------------------------------------------------------
class _Problem:
    """One level: the moments of poses on its two volumes, counted."""

    def __init__(self, reference, volume, centre, counter: List[int]):
        self.reference, self.volume, self.centre, self.counter = reference, volume, centre, counter
        self.tensors = (reference.image, reference.mask, volume.image, volume.mask)

    def sums(self, thetas: List[List[float]]) -> List[List[float]]:
        self.counter[0] += len(thetas)
        return pose_moments(*self.tensors, pose_maps(self.reference, self.volume, thetas, self.centre)).tolist()  # the one host read


def _finite(value: float) -> float:
    return 2.0 if math.isinf(value) else value


def descend(problem: _Problem, theta: List[float], free: Sequence[int], step: float, rounds: int, max_iter: int,
            start: Optional[List[float]] = None):
    """One level of the module docstring's descent from ``theta`` (``start``: its sums, if the caller has them) ->
    (theta, its sums, n0)."""
    start = problem.sums([theta])[0] if start is None else start
    n0 = start[0]
    current, current_sums = loss(start, n0), start
    for _ in range(rounds):
        for _ in range(max_iter):
            trials = []
            for j in free:
                for sign in (1.0, -1.0):
                    moved = list(theta)
                    moved[j] = moved[j] + sign * step
                    trials.append(moved)
            losses = [_finite(loss(row, n0)) for row in problem.sums(trials)]
            g = [losses[2 * i] - losses[2 * i + 1] for i in range(len(free))]
            norm = math.sqrt(sum(v * v for v in g))
            trial = list(theta)
            for i, j in enumerate(free):
                trial[j] = trial[j] - step * g[i] / (norm + 1e-12)
            trial_sums = problem.sums([trial])[0]
            trial_loss = loss(trial_sums, n0)
            if not trial_loss < current:
                break
            theta, current, current_sums = trial, trial_loss, trial_sums
        step = step / 2
    return theta, current_sums, n0


def align_volumes(reference, volume, dof: str = "rigid", levels: int = 3, rounds: int = 6, max_iter: int = 30, step: float = 1.0) -> Dict:
    """The correction of the module docstring for the ``Volume`` ``volume`` against the ``Volume`` ``reference``: ``theta`` (6
    floats), ``matrix`` (G, (4,4) float64), ``rotation_deg``, ``translation_mm`` (|t|), ``ncc_before`` / ``ncc_after`` (r at
    level 0 under 0 and under ``theta``), ``levels`` used, ``evaluations`` (poses evaluated), ``accepted``, ``skipped`` (no shared
    voxel) and ``centre`` (c)."""
    if dof not in DOFS:
        raise ValueError(f"align {dof!r}: one of {', '.join(DOFS)} expected")
    ref_image = reference.image if reference.image.is_floating_point() else reference.image.float()
    dtype, device = ref_image.dtype, ref_image.device
    centre = centroid(reference)
    used = usable_levels(reference, volume, levels)
    counter = [0]
    zero = [0.0] * 6
    theta, before, after, skipped = list(zero), math.nan, math.nan, False
    for level in range(used - 1, -1, -1):
        problem = _Problem(pyramid_level(reference, level, dtype, device), pyramid_level(volume, level, dtype, device), centre, counter)
        start = problem.sums([theta])[0]  # (K = 1: the level's n0)
        if level == used - 1 and start[0] == 0:
            skipped = True
            break
        theta, sums, _ = descend(problem, theta, DOFS[dof], float(step) * 2.0 ** level, rounds, max_iter, start)
        if level == 0:
            after = correlation(sums)
            before = after if theta == zero else correlation(problem.sums([zero])[0])
    accepted = not skipped and theta != zero and after > before
    if not accepted:
        if not skipped and theta != zero:
            logging.warning("evaluate: the alignment did not raise the correlation (%.6f after, %.6f before): the poses are kept", after, before)
        theta, after = list(zero), before
    G = correction(theta, centre)
    return {"theta": theta, "matrix": G, "rotation_deg": math.sqrt(sum(v * v for v in theta[:3])),
            "translation_mm": float(G[:3, 3].norm()), "ncc_before": before, "ncc_after": after, "levels": used,
            "evaluations": counter[0], "accepted": accepted, "skipped": skipped, "centre": centre}


def report_entry(result: Dict) -> Dict:
    """``align_volumes``'s result without tensors: the ``alignment`` entry of a report."""
    entry = {k: result[k] for k in ("theta", "rotation_deg", "translation_mm", "ncc_before", "ncc_after", "levels", "evaluations", "accepted")}
    entry["matrix"] = result["matrix"].tolist()
    return entry
