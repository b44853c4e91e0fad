"""Float64 reference of the hash-grid encoding for the kernel tests (a plain module, not a conftest): forward, table gradient
and the input gradient PER LEVEL, written out without autograd so that a 33 M-entry table costs one ``index_add_`` per corner.

What is shared with the kernels, and with ``oracle/hashgrid.py``, is everything that decides WHICH entries a point touches:

* the position of a point at a level is ``oracle.hashgrid._pos``: the exact product ``scale * u`` plus 0.5, rounded ONCE to
  float32 (the kernels' ``fmaf``); ``cell = floor(pos)``, ``w = pos - cell`` (exact in float32);
* the entry of a corner is ``oracle.hashgrid._corner_index``.

Everything behind that - corner weights, the 8-term sums, the scatter - is float64, so the reference's own error (~1e-16) is far
below what any float32 kernel is held to.  The input gradient is returned per level: the levels' shares differ by the ratio of
their scales (3e-5 between the coarsest and the finest level of ``(16, 2, 19, 16, 2.0)``), and a sum over levels shows only the
finest ones.
"""
import torch

from oracle import hashgrid as O
from oracle.hashgrid import _corner_index, _pos  # (bound here: a test that patches the oracle's does not change the reference)

_CORNERS = [(cx, cy, cz) for cz in (0, 1) for cy in (0, 1) for cx in (0, 1)]  # (the oracle's order of summation)


def levels_of(spec_tuple):
    L, _, log2_T, base, scale = spec_tuple
    return O.make_levels(L, log2_T, base, scale)


def reference(spec_tuple, u, table, dy):
    """``spec_tuple`` = (L, F, log2 T, base resolution, per-level scale); ``u`` (N, 3) float32 in [0, 1]; ``table`` flat float64;
    ``dy`` (N, L F) float64 -> float64 ``pe`` (N, L, F), ``grad_table`` (flat), ``grad_u`` (L, N, 3)."""
    L, F = spec_tuple[0], spec_tuple[1]
    assert u.dtype == torch.float32 and table.dtype == torch.float64 and dy.dtype == torch.float64
    levels = levels_of(spec_tuple)
    N = u.shape[0]
    tab = table.view(-1, F)
    assert tab.shape[0] == levels[-1].offset + levels[-1].size and tuple(dy.shape) == (N, L * F)
    pe = torch.zeros(N, L, F, dtype=torch.float64)
    grad_table = torch.zeros_like(tab)
    grad_u = torch.zeros(L, N, 3, dtype=torch.float64)
    for li, lv in enumerate(levels):
        pos = _pos(u, lv.scale)
        assert pos.dtype == torch.float32
        cell = torch.floor(pos)
        w = (pos - cell).double()
        g = cell.long()
        dyl = dy[:, li * F : (li + 1) * F]
        feat = torch.zeros(N, F, dtype=torch.float64)
        for c in _CORNERS:
            wd = [w[:, d] if c[d] else 1 - w[:, d] for d in range(3)]
            idx = _corner_index(lv, g[:, 0] + c[0], g[:, 1] + c[1], g[:, 2] + c[2]) + lv.offset
            wgt = wd[0] * wd[1] * wd[2]
            rows = tab[idx]
            feat = feat + wgt[:, None] * rows
            grad_table.index_add_(0, idx, wgt[:, None] * dyl)
            fdy = (rows * dyl).sum(-1)
            for d in range(3):
                o0, o1 = [k for k in range(3) if k != d]
                grad_u[li, :, d] += lv.scale * (1.0 if c[d] else -1.0) * wd[o0] * wd[o1] * fdy
        pe[:, li] = feat
    return pe, grad_table.view(-1), grad_u


# The grids of tests/test_gpu_hashgrid_grids.py: name -> ((L, F, log2 T, base, scale), most chunks at one level, chunks over all
# levels, inside the owner method's plan).  A chunk is the largest power of two of entries with chunk * F <= 8192 floats (the owner
# pass's LDS accumulator, kOwnerLdsFloats in csrc/hashgrid.hip); the plan takes up to 256 chunks per level and 4064 over all levels.
# The counts are asserted (tests/test_host_logic.py), so that a change of the chunk size does not silently move the edges.
GRIDS = {
    "cli_130mm": ((12, 2, 19, 9, 1.3819), 128, 743, True),  # the command's defaults on a 130 mm box
    "cli_60mm": ((12, 2, 19, 4, 1.3819), 128, 423, True),  # coarse levels of 4-6 vertices
    "cli_fine": ((14, 2, 19, 13, 1.3819), 128, 1140, True),  # --finest-resolution 0.25 on 200 mm; E = 28
    "tcnn_default": ((16, 2, 19, 16, 2.0), 128, 1737, True),  # nesvor_amd.tinycudann.Encoding's defaults: finest resolution 524 288
    "L17": ((17, 2, 12, 4, 1.2), 1, 17, True),  # the first level on lane 16 of the 32-level scans; E = 34
    "L17_F1": ((17, 1, 12, 4, 1.2), 1, 17, True),  # E = 17, odd
    "L32": ((32, 2, 12, 3, 1.15), 1, 32, True),  # the level limit
    "L32_F8": ((32, 8, 10, 3, 1.15), 1, 32, True),  # E = 256
    "L1": ((1, 2, 19, 16, 2.0), 1, 1, True),  # one dense level
    "all_dense": ((5, 2, 19, 4, 1.5), 3, 7, True),  # no hashed level
    "all_hashed_F4": ((6, 4, 10, 16, 1.3819), 1, 6, True),  # no dense level, F > 2
    "T20_256chunks": ((8, 2, 20, 16, 1.6), 256, 1118, True),  # the chunk limit at F = 2
    "F4_256chunks": ((10, 4, 19, 9, 1.3819), 256, 970, True),  # ... at F = 4
    "F8_256chunks": ((8, 8, 18, 9, 1.3819), 256, 657, True),  # ... at F = 8
    "F1_256chunks": ((10, 1, 21, 9, 1.3819), 256, 601, True),  # ... at F = 1
    "near_bucket_limit": ((31, 2, 19, 81, 1.05), 128, 3968, True),  # 3968 buckets of 4064
    "T21_512chunks": ((8, 2, 21, 16, 1.6), 512, 1913, False),  # outside the plan: chunks per level
    "many_buckets": ((32, 2, 19, 81, 1.05), 128, 4096, False),  # outside the plan: 4096 buckets
}
OWNER_LDS_FLOATS, MAX_CHUNKS, MAX_BUCKETS = 8192, 256, 4064


def chunk_counts(spec_tuple):
    """-> (most chunks at one level, chunks over all levels) under the plan's chunking rule."""
    chunk = 1
    while chunk * 2 * spec_tuple[1] <= OWNER_LDS_FLOATS:
        chunk *= 2
    n = [-(-lv.size // chunk) for lv in levels_of(spec_tuple)]
    return max(n), sum(n)
