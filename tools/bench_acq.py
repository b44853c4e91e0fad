"""Times the slice-acquisition kernels (csrc/slice_acq.hip) and the svr similarity sums (csrc/svr.hip) on their own.

    python tools/bench_acq.py [--repeats 21]
    python tools/bench_acq.py --libs OLD.so NEW.so [--rounds 3]

* the four float operators - A, A^T, the backward of A (volume and pose gradients) and the backward of A^T (slice and pose
  gradients) - on one stack of 77 slices of 151^2 pixels of 1.5 mm against a 128^3 volume of 1 mm with the (9,5,5) PSF;
* ``nesvor_svr_similarity`` on DESIGN.md's registration case: 40 slices of 77^2, 13 poses each (one finite-difference gradient),
  the 153 non-zero taps of the same PSF, a 64^3 volume.
HIP events, warm, medians and ranges; one JSON object per line.  The library is the one ``NESVOR_HIP_LIB`` names (nesvor_amd/_lib.py).
``--libs``: every library in a child process of its own, alternating, ``--rounds`` times; then per library and call the median of
the rounds' medians and their range - the spread to hold a difference between two builds against.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, warmup, repeats):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def _poses(n, spacing, g):
    """(n,3,4): slice k at z = (k - (n - 1) / 2) spacing, tilted by up to 3 degrees about a seeded axis, moved by up to 1.5 voxels."""
    import torch

    ax = torch.randn(n, 3, generator=g)
    ax = ax / ax.norm(dim=1, keepdim=True)
    ang = (torch.rand(n, generator=g) * 2 - 1) * math.radians(3.0)
    K = torch.zeros(n, 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    R = torch.eye(3) + torch.sin(ang)[:, None, None] * K + (1 - torch.cos(ang))[:, None, None] * (K @ K)
    t = (torch.rand(n, 3, generator=g) * 2 - 1) * 1.5
    t[:, 2] += (torch.arange(n) - (n - 1) / 2) * spacing
    return torch.cat([R, t[:, :, None]], 2).contiguous()


def bench_operators(repeats, device):
    import torch
    from nesvor_amd import slice_acq_cuda as A
    from nesvor_amd.utils import get_PSF

    g = torch.Generator().manual_seed(77)
    n, hw, N, res = 77, 151, 128, 1.5
    psf = get_PSF(res_ratio=(1.5, 1.5, 3.0)).to(device)
    tf = _poses(n, 1.5, g).to(device)
    vol = torch.rand((1, 1, N, N, N), generator=g).to(device)
    y = torch.rand((n, 1, hw, hw), generator=g).to(device)
    gy = torch.randn((n, 1, hw, hw), generator=g).to(device)
    gv = torch.randn((1, 1, N, N, N), generator=g).to(device)
    calls = {
        "forward": lambda: A.forward(tf, vol, None, None, psf, (hw, hw), res, True, False),
        "adjoint_forward": lambda: A.adjoint_forward(tf, psf, y, None, None, (N, N, N), res, False, False),
        "backward": lambda: A.backward(tf, vol, None, psf, gy, None, res, False, True, True),
        "adjoint_backward": lambda: A.adjoint_backward(tf, gv, None, None, psf, y, None, None, res, False, False, True, True),
    }
    for name, fn in calls.items():
        print(json.dumps({"what": f"slice_acq {name}", "slices": n, "slice_size": hw, "volume": N, "psf": list(psf.shape),
                          "taps": int((psf != 0).sum()), "repeats": repeats, **_time(fn, 3, repeats)}), flush=True)


def bench_svr(repeats, device):
    import torch
    from nesvor_amd.utils import get_PSF

    g = torch.Generator().manual_seed(40)
    n, hw, N, K, res = 40, 77, 64, 13, 1.5
    psf = get_PSF(res_ratio=(1.5, 1.5, 3.0)).to(device)
    base = _poses(n, 1.5, g)
    tf = base[:, None].repeat(1, K, 1, 1)
    for k in range(1, K):  # one finite-difference gradient: +- half a voxel along each axis, +- a small turn about each axis
        a = (k - 1) // 2 % 3
        if k <= 6:
            tf[:, k, a, 3] += 0.5 if k % 2 else -0.5
        else:
            tf[:, k, :, (a + 1) % 3] += (0.01 if k % 2 else -0.01) * base[:, :, (a + 2) % 3]
    tf = tf.contiguous().to(device)
    vol = torch.rand((N, N, N), generator=g).to(device)
    J = torch.rand((n, hw, hw), generator=g).to(device)
    m = (torch.rand((n, hw, hw), generator=g) < 0.7).to(device)
    fn = lambda: torch.ops.nesvor.svr_similarity(vol, psf, tf, J, m, res)
    print(json.dumps({"what": "svr_similarity", "slices": n, "slice_size": hw, "volume": N, "poses": K, "taps": int((psf != 0).sum()),
                      "repeats": repeats, "valid_share": float(fn()[..., 0].sum() / (K * m.sum())), **_time(fn, 3, repeats)}), flush=True)


def compare(libs, rounds, repeats):
    """Child processes, one per (round, library), alternating; a child that fails ends the run."""
    med = {}
    for r in range(rounds):
        for lib in libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(repeats)], env=dict(os.environ, NESVOR_HIP_LIB=lib),
                                 stdout=subprocess.PIPE, text=True, timeout=300)
            if out.returncode != 0:
                raise SystemExit(f"bench_acq.py: the child with {lib} ended with status {out.returncode}")
            for line in out.stdout.splitlines():
                d = json.loads(line)
                print(json.dumps({"lib": lib, "round": r, **d}), flush=True)
                med.setdefault((lib, d["what"]), []).append(d["median_ms"])
    for (lib, what), v in med.items():
        print(json.dumps({"lib": lib, "what": what, "rounds": rounds, "median_of_medians_ms": statistics.median(v), "min_median_ms": min(v),
                          "max_median_ms": max(v)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--libs", nargs="*", default=[])
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.libs:
        return compare([os.path.abspath(p) for p in a.libs], a.rounds, a.repeats)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_acq.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401

    device = torch.device("cuda:0")
    bench_operators(a.repeats, device)
    bench_svr(a.repeats, device)


if __name__ == "__main__":
    main()
