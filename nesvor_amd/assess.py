"""Stack quality assessment and the choice of the template stack (the ``assess`` command, ``--template-stack auto``).

The classical motion correction (nesvor_amd/registration.py) aligns everything to ONE stack, the template: the stack
registration registers the others to it and centres the world frame on it.  If that stack is the one the subject moved in, the
whole pipeline is aligned to the worst data of the set.  Classical pipelines therefore score every stack for motion first and
take the least-moved one; upstream NeSVoR added an ``assess`` command for this in releases after the one this project models,
so the definitions below are this module's.

Scores are per stack, higher is better, computed in float64 on the host from masked moments of slice pairs:

* ``ncc``: the mean normalised cross-correlation of ADJACENT non-empty slices, over their common masked pixels.  A pair counts
  when it overlaps in at least ``MIN_OVERLAP`` pixels and both variances are positive; no countable pair: ``nan`` (ranked last).
* ``matrix-rank``: the Gram matrix G[i][j] = sum a b over all pairs of the stack's non-empty slices is that of the stack's data
  matrix; with its singular values sigma = sqrt(eigenvalues) and p = sigma / sum sigma the effective rank is
  exp(-sum p log p).  A still stack's slices vary smoothly (low rank); motion raises it.  Score = -(effective rank) / (number
  of non-empty slices).  No free parameter.  It compares stacks of ONE orientation: different orientations cut the anatomy
  differently and differ in rank without any motion.
* ``volume``: the masked pixels of the stack times the voxel volume (pixel area times slice spacing) in mm^3.

The moments of pair (a, b), over the pixels valid in both slices, are {count, sum a, sum b, sum a^2, sum b^2, sum a b}
(``pair_moments``): on HIP fp32 tensors ONE call of ``torch.ops.nesvor.pair_moments`` (csrc/assess.hip: reproducible sums, no
P x h x w temporaries) for all stacks' pairs; ``NESVOR_ASSESS=composed``, host tensors and other dtypes take the torch expression
in float64 (``pair_moments_composed``, the yardstick of tests/test_assess.py and tests/test_gpu_assess.py).
"""
import logging
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

MIN_OVERLAP = 16  # common masked pixels an adjacent pair needs to count for the ncc score
N_MOMENTS = 6
METRICS = ("ncc", "matrix-rank", "volume")
_COMPOSED_CHUNK = 256  # pairs gathered at a time by the torch expression


def _fused(slices: torch.Tensor) -> bool:
    return os.environ.get("NESVOR_ASSESS", "") != "composed" and slices.is_cuda and slices.dtype == torch.float32


def _host_pairs(pairs, n: int) -> torch.Tensor:
    """``pairs`` as a host (P,2) int64 tensor with every index in [0, n); ``ValueError`` otherwise."""
    p = torch.as_tensor(pairs).cpu()
    if p.numel() == 0:
        return torch.zeros((0, 2), dtype=torch.int64)
    if p.is_floating_point() or p.is_complex() or p.dtype == torch.bool:
        raise ValueError(f"pair_moments: integer slice indices expected, got {p.dtype}")
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"pair_moments: pairs of shape (P, 2) expected, got {tuple(p.shape)}")
    p = p.to(torch.int64)
    if int(p.min()) < 0 or int(p.max()) >= n:
        raise ValueError(f"pair_moments: slice indices must be in [0, {n}), got {int(p.min())} .. {int(p.max())}")
    return p


def pair_moments_composed(slices: torch.Tensor, mask: Optional[torch.Tensor], pairs: torch.Tensor) -> torch.Tensor:
    """(P,6) float64 {count, sum a, sum b, sum a^2, sum b^2, sum a b} over the pixels valid in both slices of every pair, as a
    torch expression in float64 on the tensors' device.  ``pairs``: (P,2) integer tensor, indices in range."""
    n = slices.shape[0]
    x = slices.reshape(n, -1).double()
    valid = None if mask is None else mask.reshape(n, -1).bool()
    pairs = pairs.to(device=slices.device, dtype=torch.int64).reshape(-1, 2)
    out = torch.zeros((pairs.shape[0], N_MOMENTS), dtype=torch.float64, device=slices.device)
    zero = torch.zeros((), dtype=torch.float64, device=slices.device)
    for start in range(0, pairs.shape[0], _COMPOSED_CHUNK):
        ia, ib = pairs[start:start + _COMPOSED_CHUNK, 0], pairs[start:start + _COMPOSED_CHUNK, 1]
        a, b = x[ia], x[ib]
        if valid is None:
            both = torch.ones_like(a, dtype=torch.bool)
        else:
            both = valid[ia] & valid[ib]
            a, b = torch.where(both, a, zero), torch.where(both, b, zero)
        out[start:start + _COMPOSED_CHUNK] = torch.stack([both.double().sum(1), a.sum(1), b.sum(1), (a * a).sum(1), (b * b).sum(1),
                                                          (a * b).sum(1)], dim=1)
    return out


def pair_moments(slices: torch.Tensor, mask: Optional[torch.Tensor], pairs) -> torch.Tensor:
    """(P,6) float64 moments of the slice pairs ``pairs`` (a host integer tensor or a list of index pairs) of ``slices``
    (n, ..., h, w) under ``mask`` (bool or uint8, same shape, or None).  The indices are range-checked HERE, on the host, before
    anything is launched (``ValueError``): the kernel does not check them."""
    n = int(slices.shape[0])
    if mask is not None and mask.numel() != slices.numel():
        raise ValueError("pair_moments: mask must have the shape of slices")
    host = _host_pairs(pairs, n)
    if _fused(slices):
        return torch.ops.nesvor.pair_moments(slices.contiguous(), None if mask is None else mask.reshape(slices.shape).contiguous(),
                                             host.to(torch.int32).to(slices.device))
    return pair_moments_composed(slices, mask, host)


# ---------------------------------------------------------------------------------------------------------------------
# scores from moments (host, float64)
# ---------------------------------------------------------------------------------------------------------------------
def ncc_of_pairs(moments: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """NCC per pair of (K,6) moments and whether the pair counts (overlap >= MIN_OVERLAP, both variances > 0)."""
    m = moments.detach().double().cpu().reshape(-1, N_MOMENTS)
    cnt, sa, sb, saa, sbb, sab = m.unbind(1)
    safe = cnt.clamp(min=1)
    va, vb, cov = saa - sa * sa / safe, sbb - sb * sb / safe, sab - sa * sb / safe
    counts = (cnt >= MIN_OVERLAP) & (va > 0) & (vb > 0)
    den = torch.sqrt(torch.where(counts, va * vb, torch.ones_like(va)))
    return torch.where(counts, cov / den, torch.zeros_like(cov)), counts


def ncc_score(moments: torch.Tensor) -> float:
    """Mean NCC of the countable pairs among the (K,6) moments of a stack's adjacent slices; ``nan`` without one."""
    ncc, counts = ncc_of_pairs(moments)
    return float(ncc[counts].mean()) if bool(counts.any()) else float("nan")


def effective_rank(gram: torch.Tensor) -> float:
    """exp of the entropy of the normalised singular values of the data matrix whose Gram matrix is ``gram`` (k,k)."""
    lam = torch.linalg.eigvalsh(gram.detach().double().cpu()).clamp(min=0)
    sigma = torch.sqrt(lam)
    total = float(sigma.sum())
    if not total > 0:
        return float("nan")
    p = sigma / total
    p = p[p > 0]
    return float(torch.exp(-(p * torch.log(p)).sum()))


def matrix_rank_score(gram: torch.Tensor) -> float:
    k = int(gram.shape[0])
    return -effective_rank(gram) / k if k > 0 else float("nan")


def volume_score(self_moments: torch.Tensor, voxel_volume: float) -> float:
    """Masked pixels (the counts of the (K,6) self-pair moments) times the voxel volume in mm^3."""
    return float(self_moments.detach().double().cpu().reshape(-1, N_MOMENTS)[:, 0].sum()) * float(voxel_volume)


def _gram(moments: torch.Tensor, k: int) -> torch.Tensor:
    """(k,k) symmetric matrix of sum a b from the moments of the pairs i <= j in row-major order."""
    g = torch.zeros((k, k), dtype=torch.float64)
    iu = torch.triu_indices(k, k)
    g[iu[0], iu[1]] = moments.detach().double().cpu().reshape(-1, N_MOMENTS)[:, 5]
    return g + g.triu(1).T


def stack_pairs(k: int, metric: str) -> List[Tuple[int, int]]:
    """The pairs a metric needs among k non-empty slices (indices 0..k-1): adjacent, all i <= j (row-major), or self-pairs."""
    if metric == "ncc":
        return [(i, i + 1) for i in range(k - 1)]
    if metric == "matrix-rank":
        return [(i, j) for i in range(k) for j in range(i, k)]
    if metric == "volume":
        return [(i, i) for i in range(k)]
    raise ValueError(f"unknown metric {metric!r}: one of {', '.join(METRICS)}")


def score_from_moments(moments: torch.Tensor, k: int, metric: str, voxel_volume: float = 1.0) -> float:
    """A stack's score from the moments of ``stack_pairs(k, metric)``."""
    if metric == "ncc":
        return ncc_score(moments)
    if metric == "matrix-rank":
        return matrix_rank_score(_gram(moments, k))
    if metric == "volume":
        return volume_score(moments, voxel_volume)
    raise ValueError(f"unknown metric {metric!r}: one of {', '.join(METRICS)}")


def rank_scores(scores: Sequence[float]) -> List[int]:
    """Rank per entry, 0 = best (highest score); ``nan`` ranks last, ties go to the lower index."""
    order = sorted(range(len(scores)), key=lambda i: (math.isnan(scores[i]), 0.0 if math.isnan(scores[i]) else -scores[i], i))
    ranks = [0] * len(scores)
    for r, i in enumerate(order):
        ranks[i] = r
    return ranks


# ---------------------------------------------------------------------------------------------------------------------
# stacks
# ---------------------------------------------------------------------------------------------------------------------
def assess_stacks(stacks: List, metric: str = "ncc") -> List[Dict]:
    """One dict per stack, in input order: ``stack_idx``, ``n_slices`` (non-empty), ``metric``, ``score`` (higher is better),
    ``rank`` (0 is best).  The masked stacks (``slices * mask``, as the registration takes them) are zero-padded to one (h, w)
    and concatenated; ONE ``pair_moments`` call serves all stacks' pairs."""
    if metric not in METRICS:
        raise ValueError(f"unknown metric {metric!r}: one of {', '.join(METRICS)}")
    if not stacks:
        return []
    h, w = max(s.slices.shape[-2] for s in stacks), max(s.slices.shape[-1] for s in stacks)
    pad = lambda t: F.pad(t, (0, w - t.shape[-1], 0, h - t.shape[-2]))
    masks = [s.mask.reshape(s.slices.shape).bool() for s in stacks]
    data = torch.cat([pad(s.slices * m) for s, m in zip(stacks, masks)]).contiguous()
    mask = torch.cat([pad(m) for m in masks]).contiguous()
    nonempty = mask.flatten(1).any(1).cpu()
    pairs, spans, start = [], [], 0
    for s in stacks:
        n = s.slices.shape[0]
        ids = (torch.nonzero(nonempty[start:start + n]).flatten() + start).tolist()
        local = stack_pairs(len(ids), metric)
        spans.append((len(pairs), len(local), len(ids)))
        pairs += [(ids[i], ids[j]) for i, j in local]
        start += n
    moments = pair_moments(data, mask, torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)).cpu()
    scores = []
    for s, (first, count, k) in zip(stacks, spans):
        voxel = float(s.resolution_x) * float(s.resolution_y) * float(s.gap)
        scores.append(score_from_moments(moments[first:first + count], k, metric, voxel))
    ranks = rank_scores(scores)
    return [{"stack_idx": j, "n_slices": spans[j][2], "metric": metric, "score": scores[j], "rank": ranks[j]} for j in range(len(stacks))]


def format_table(rows: List[Dict]) -> str:
    lines = ["stack  slices  %-12s  rank" % (rows[0]["metric"] if rows else "score")]
    lines += ["%5d  %6d  %12.6g  %4d" % (r["stack_idx"], r["n_slices"], r["score"], r["rank"]) for r in rows]
    return "\n".join(lines)


def choose_template(stacks: List, spec: Union[str, int] = "0", metric: str = "ncc") -> int:
    """The index of the template stack: ``spec`` is an index (integer string) or ``auto`` = the best stack under ``metric``."""
    spec = str(spec).strip()
    if spec == "auto":
        rows = assess_stacks(stacks, metric)
        best = min(rows, key=lambda r: r["rank"])["stack_idx"]
        logging.info("Stack assessment (%s, higher is better):\n%s", metric, format_table(rows))
        logging.info("Template stack: %d (--template-stack auto, metric %s)", best, metric)
        return best
    try:
        idx = int(spec)
    except ValueError:
        raise SystemExit(f"--template-stack: 'auto' or a stack index expected, got {spec!r}")
    if not 0 <= idx < len(stacks):
        raise SystemExit(f"--template-stack {idx}: there are {len(stacks)} input stacks (indices 0 .. {len(stacks) - 1})")
    return idx
