"""Fixtures and float64 yardsticks shared by tests/test_masking.py (CPU) and tests/test_gpu_masking.py: hand-posed stacks with
generic small rotations, plain numpy loops for the four masking rules, and the boundary condition under which a fused mask can
be compared with the composed one bit for bit.

Nothing here touches a GPU: the stacks carry (n,3,4) pose matrices (``RigidTransform`` converts axis-angle poses on the device
only), built from rotation vectors by Rodrigues' formula in float64.
"""
import numpy as np
import torch


def rodrigues(rotvec) -> np.ndarray:
    r = np.asarray(rotvec, dtype=np.float64)
    theta = np.linalg.norm(r)
    if theta == 0:
        return np.eye(3)
    k = r / theta
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


def stack_matrices(n, gap, pose, motion=0.0, seed=0) -> torch.Tensor:
    """(n,3,4) float32 [R | t] with x' = R (x + t): rotation ``pose[:3]`` (a rotation vector), in-frame offset ``pose[3:]``, slice k
    at z = t_z + (k - (n - 1) / 2) gap; ``motion`` > 0 perturbs every slice's rotation vector and offset by N(0, motion^2)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 3, 4))
    for k in range(n):
        d = rng.normal(0, motion, 6) if motion > 0 else np.zeros(6)
        out[k, :, :3] = rodrigues(np.asarray(pose[:3], dtype=np.float64) + 0.05 * d[:3])
        out[k, :, 3] = np.asarray(pose[3:], dtype=np.float64) + d[3:] + np.array([0, 0, (k - (n - 1) / 2) * gap])
    return torch.tensor(out, dtype=torch.float32)


def stratified_intensities(shape, seed, zero_share=0.15, lo=0.05, hi=1.0) -> torch.Tensor:
    """float32 of ``shape``: one value from every one of N equal strata of (lo, hi), away from the strata's ends, in a random
    spatial order (so every histogram bin of a kept subset is populated evenly), then ``zero_share`` of the voxels set to 0."""
    rng = np.random.default_rng(seed)
    N = int(np.prod(shape))
    v = lo + (np.arange(N) + rng.uniform(0.1, 0.9, N)) / N * (hi - lo)
    v = v[rng.permutation(N)]
    v[rng.uniform(size=N) < zero_share] = 0.0
    return torch.tensor(v.reshape(shape), dtype=torch.float32)


def make_stack(shape, rx, ry, thickness, gap, pose, seed=0, motion=0.0, device="cpu"):
    from nesvor_amd.image import Stack
    from nesvor_amd.transform import RigidTransform

    n, h, w = shape
    slices = stratified_intensities((n, 1, h, w), seed).to(device)
    return Stack(slices, slices > 0, RigidTransform(stack_matrices(n, gap, pose, motion, seed).to(device), trans_first=True),
                 resolution_x=rx, resolution_y=ry, thickness=thickness, gap=gap)


# scene -> stack specs (shape, rx, ry, thickness, gap, pose, motion): generic small rotations, different shapes and pixel sizes
SCENES = {
    # three stacks; another stack of 65 slices (two LDS chunks, the second with one row) with per-slice motion; thickness > gap
    "trio": [((4, 40, 52), 1.0, 1.1, 4.0, 3.5, [0.1, 0.1, 0.1, 0.1, 0.1, 0.1], 0.0),
             ((65, 5, 7), 7.0, 9.0, 1.2, 0.9, [-0.1, 0.0, -0.4, 0.1, 0.5, 0.1], 0.1),
             ((3, 33, 31), 1.5, 1.3, 6.0, 5.0, [-0.12, -0.01, 0.1, -1.0, 2.0, -1.5], 0.0)],
    # two stacks; another stack of 130 slices (three chunks) and one of a single slice; gap > thickness
    "row": [((1, 1, 257), 0.5, 0.5, 3.0, 3.0, [0.1, -0.2, 0.05, 0.3, -0.2, 0.4], 0.0),
            ((130, 3, 20), 2.0, 3.0, 0.5, 0.8, [0.0, 1.4, 0.1, 0.2, 0.1, -0.3], 0.0)],
    # two stacks; another stack of 64 slices (exactly one chunk); gap > thickness for both
    "pair": [((2, 1, 65), 0.8, 0.8, 2.0, 2.5, [-0.2, 0.2, -0.1, 0.5, -0.4, 0.2], 0.0),
             ((64, 10, 10), 3.0, 3.0, 0.6, 0.7, [0.2, 1.3, -0.1, -0.2, 0.3, 0.1], 0.0)],
    # a stack wholly outside the other: two all-zero masks
    "apart": [((1, 16, 16), 1.0, 1.0, 2.0, 2.0, [0.1, 0.1, 0.1, 0.1, 0.1, 0.1], 0.0),
              ((1, 1, 1), 1.0, 1.0, 2.0, 2.0, [-0.1, 0.0, -0.4, 40.0, 50.0, 60.0], 0.0)],
    # one stack (for the threshold and the volume mask alone)
    "solo": [((3, 33, 31), 1.5, 1.3, 6.0, 5.0, [-0.12, -0.01, 0.1, -1.0, 2.0, -1.5], 0.0)],
}


# Per scene the seed of a small pose jitter (N(0, 0.02) on the rotation vectors, N(0, 0.5 mm) on the offsets), chosen on the CPU so
# that the float64 restatement alone meets the boundary condition below for every stack of the scene (rule_violations: with the
# other stacks' slabs, with ball_volume()'s mask and with THRESHOLD).  tests/test_masking.py asserts that it does.
JITTER = {"trio": 294, "row": 0, "pair": 3, "apart": 0, "solo": 0}
THRESHOLD = 0.3
# (scene, stack, n_bins) of the Otsu comparisons on the stacks' own masks: many bins only where the voxels populate them (a run of
# empty bins around the best split is a run of equal variances: no runner-up margin); (apart, 1) is the one-voxel stack
OTSU_CASES = [("trio", 0, 1024), ("trio", 0, 256), ("trio", 1, 200), ("trio", 2, 200), ("solo", 0, 256), ("row", 1, 256), ("pair", 1, 200),
              ("row", 0, 2), ("pair", 0, 2), ("apart", 0, 2), ("apart", 1, 2), ("apart", 1, 256)]


def scene(name, device="cpu", jitter=None):
    rng = np.random.default_rng(JITTER[name] if jitter is None else jitter)
    out = []
    for i, (shape, rx, ry, th, gap, pose, motion) in enumerate(SCENES[name]):
        pose = np.asarray(pose, dtype=np.float64) + np.concatenate([rng.normal(0, 0.02, 3), rng.normal(0, 0.5, 3)])
        out.append(make_stack(shape, rx, ry, th, gap, pose, seed=17 * i + len(name), motion=motion, device=device))
    return out


def ball_volume(device="cpu"):
    """A (5,6,7) mask volume of 1.7 mm voxels under a rotated pose: a ball around the lattice centre; some voxels of the "solo" and
    "trio" stacks lie outside its lattice."""
    from nesvor_amd.image import Volume
    from nesvor_amd.transform import RigidTransform

    z, y, x = np.meshgrid(np.arange(5) - 2.0, np.arange(6) - 2.5, np.arange(7) - 3.0, indexing="ij")
    img = torch.tensor(((x / 3.2) ** 2 + (y / 2.7) ** 2 + (z / 2.2) ** 2 <= 1).astype(np.float32), device=device)
    mat = np.concatenate([rodrigues([0.3, -0.2, 0.25]), np.array([[0.4], [-0.7], [0.9]])], 1)[None]
    return Volume(img, img > 0, RigidTransform(torch.tensor(mat, dtype=torch.float32, device=device), trans_first=True), 1.7, 1.7, 1.7)


# ---------------------------------------------------------------------------------------------------------------------
# plain loops (the CPU yardstick of the composed path)
# ---------------------------------------------------------------------------------------------------------------------
def positions_loop(st) -> np.ndarray:
    """(n,h,w,3) float64 world positions of the pixels of a stack."""
    T = st.transformation.matrix(True).double().cpu().numpy()
    n, _, h, w = st.slices.shape
    out = np.zeros((n, h, w, 3))
    for s in range(n):
        for r in range(h):
            for c in range(w):
                x = np.array([(c - (w - 1) / 2) * st.resolution_x, (r - (h - 1) / 2) * st.resolution_y, 0.0])
                out[s, r, c] = T[s, :, :3] @ (x + T[s, :, 3])
    return out


def intersection_loop(stacks, j) -> np.ndarray:
    """(n,h,w) bool: the voxels of stack j that some slice of every other stack contains."""
    p = positions_loop(stacks[j])
    keep = np.ones(p.shape[:3], dtype=bool)
    for k, other in enumerate(stacks):
        if k == j:
            continue
        T = other.transformation.matrix(True).double().cpu().numpy()
        h, w = other.slices.shape[-2:]
        ext = np.array([w * other.resolution_x / 2, h * other.resolution_y / 2, max(other.thickness, other.gap) / 2])
        for idx in np.ndindex(*keep.shape):
            found = False
            for t in range(T.shape[0]):
                q = T[t, :, :3].T @ p[idx] - T[t, :, 3]
                if np.all(np.abs(q) <= ext):
                    found = True
                    break
            keep[idx] = keep[idx] and found
    return keep


def volume_loop(st, volume) -> np.ndarray:
    """(n,h,w) float64: the mask volume's 0 / 1 array interpolated at the pixels of a stack, 0 off the lattice."""
    p = positions_loop(st)
    T = volume.transformation.matrix(True).double().cpu().numpy()[0]
    arr = (volume.image > 0).cpu().numpy().astype(np.float64)
    D, H, W = arr.shape
    res = np.array([volume.resolution_x, volume.resolution_y, volume.resolution_z], dtype=np.float64)
    out = np.zeros(p.shape[:3])
    for idx in np.ndindex(*out.shape):
        u = (T[:, :3].T @ p[idx] - T[:, 3]) / res + (np.array([W, H, D]) - 1) / 2
        i0 = np.floor(u).astype(int)
        f = u - i0
        acc = 0.0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    x, y, z = i0[0] + dx, i0[1] + dy, i0[2] + dz
                    if 0 <= x < W and 0 <= y < H and 0 <= z < D:
                        acc += arr[z, y, x] * (f[2] if dz else 1 - f[2]) * (f[1] if dy else 1 - f[1]) * (f[0] if dx else 1 - f[0])
        out[idx] = acc
    return out


def otsu_numpy(values: np.ndarray, n_bins: int):
    """The float64 restatement of Otsu's rule on the kept intensities: -> (threshold as float64 or -inf, counts, variances)."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size < 2 or v.min() == v.max():
        return -np.inf, np.zeros(n_bins, dtype=np.int64), np.zeros(n_bins - 1)
    lo, hi = v.min(), v.max()
    width = (hi - lo) / n_bins
    b = np.minimum(np.floor((v - lo) / width), n_bins - 1).astype(np.int64)
    counts = np.bincount(b, minlength=n_bins).astype(np.int64)
    centres = lo + (np.arange(n_bins) + 0.5) * width
    cum_n, cum_s = np.cumsum(counts.astype(np.float64)), np.cumsum(counts * centres)
    var = np.zeros(n_bins - 1)
    for i in range(n_bins - 1):
        n0, n1 = cum_n[i], cum_n[-1] - cum_n[i]
        if n0 > 0 and n1 > 0:
            d = cum_s[i] / n0 - (cum_s[-1] - cum_s[i]) / n1
            var[i] = ((n0 / cum_n[-1]) * (n1 / cum_n[-1])) * (d * d)
    i = int(np.argmax(var))  # the first maximum
    return centres[i], counts, var


# ---------------------------------------------------------------------------------------------------------------------
# the boundary condition
# ---------------------------------------------------------------------------------------------------------------------
def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x)))) if np.isfinite(x) else 0.0


def rule_violations(slices, mask, transforms, rx, ry, threshold=None, volume=None, volume_geometry=None, slabs=None, slab_extents=None,
                    slab_offsets=None) -> dict:
    """How many voxels of the incoming mask (all voxels without one) sit too close to a decision of steps 1 to 3 for a
    bit-for-bit comparison, evaluated in float64: an intensity within one fp32 ulp of the threshold, an interpolated mask value
    within 1e-4 of 0.5, a position within 1e-3 mm of the boundary of an other stack's slabs.  The last one is measured per other
    stack as |max over its slices of the smallest margin to the slice's six faces| - the distance to the boundary of the union
    where slabs overlap, and conservative (it also counts faces shared by two abutting slabs) where they tile."""
    from nesvor_amd import masking

    valid = torch.ones(slices.shape, dtype=torch.bool, device=slices.device) if mask is None else mask.reshape(slices.shape) != 0
    valid = valid.reshape(-1)
    out = {"threshold": 0, "volume": 0, "slab": 0}
    if threshold is not None:
        t = float(threshold.reshape(-1)[0])
        out["threshold"] = int((((slices.reshape(-1).double() - t).abs() <= ulp32(t)) & valid).sum())
    if volume is None and (slab_offsets is None or slab_offsets.numel() < 2):
        return out
    p = masking.pixel_positions(transforms, int(slices.shape[-2]), int(slices.shape[-1]), rx, ry)
    if volume is not None:
        out["volume"] = int((((masking.volume_value_composed(p, volume, volume_geometry) - 0.5).abs() < 1e-4) & valid).sum())
    if slab_offsets is not None and slab_offsets.numel() > 1:
        out["slab"] = int(((masking.slab_distance_composed(p, slabs, slab_extents, slab_offsets).abs() < 1e-3).any(1) & valid).sum())
    return out


def otsu_violations(slices, mask, n_bins) -> dict:
    """The same for Otsu on the voxels of ``mask``: a bin coordinate within 1e-9 of an interior bin edge 1 .. n_bins - 1 (the two
    ends are no decisions: the minimum's coordinate is an exact 0, the maximum's is clamped into the last bin from either side),
    a best split not ahead of the runner-up by more than 1e-9 relative, an intensity within one fp32 ulp of the threshold."""
    v = slices.reshape(-1).double().cpu().numpy()
    keep = np.ones(v.shape, dtype=bool) if mask is None else (mask.reshape(-1) != 0).cpu().numpy()
    v = v[keep & ~np.isnan(v)]
    t, counts, var = otsu_numpy(v, n_bins)
    out = {"bin_edge": 0, "runner_up": 0, "threshold": 0}
    if not np.isfinite(t):
        return out
    c = (v - v.min()) / ((v.max() - v.min()) / n_bins)
    near = np.abs(c - np.round(c)) < 1e-9
    out["bin_edge"] = int((near & (np.round(c) >= 1) & (np.round(c) <= n_bins - 1)).sum())
    if n_bins > 2:
        order = np.sort(var)[::-1]
        out["runner_up"] = int(not order[0] > order[1] * (1 + 1e-9))
    out["threshold"] = int((np.abs(v - float(np.float32(t))) <= ulp32(t)).sum())
    return out
