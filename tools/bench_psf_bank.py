"""Times the PSF-bank entry points (per-stack slice profiles: csrc/slice_acq.hip, csrc/svr.hip, nesvor_amd/psf_bank.py) against the
composed path and against the one-PSF entry points.

    python tools/bench_psf_bank.py [--repeats 21]

Workload: 3 stacks of 40 slices of 128^2 pixels of 1.5 mm against a 128^3 volume of 1 mm, thicknesses 3 / 3 / 4.5 mm (2 members).
* fused bank against composed (``NESVOR_PSF_BANK=composed``: one one-PSF launch per member): one A, one A^T (equalised), one
  13-pose similarity gradient, and a whole 30-step ``reconstruct_volume``; the peak device memory either path adds;
* a bank of ONE member against the one-PSF entry point on the same input, with the spread (max - median) the one-PSF entry
  shows against itself.
HIP events, warm, the arms alternating inside every repeat, medians and ranges; one JSON object per line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _alternate(arms, warmup, repeats):
    """arms: {name: fn}; every repeat times each arm once, in turn -> {name: [ms]}."""
    import torch

    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[name].append(s.elapsed_time(e))
    return ms


def _stats(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "max_minus_median_ms": round(max(v) - med, 4)}


def _peak(fn):
    """Peak device memory ``fn`` adds to what is allocated when it starts, in MB."""
    import torch

    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_psf_bank.py measures on the GPU: no HIP device found")
    from bench_acq import _poses
    from nesvor_amd.psf_bank import bank_for
    from nesvor_amd.slice_acquisition import (slice_acquisition, slice_acquisition_adjoint, slice_acquisition_adjoint_bank,
                                              slice_acquisition_bank)
    from nesvor_amd.svr import reconstruct_volume
    from nesvor_amd.transform import RigidTransform
    from nesvor_amd.utils import get_PSF

    device = torch.device("cuda:0")
    g = torch.Generator().manual_seed(120)
    n_stack, hw, N, res_s, K = 40, 128, 128, 1.5, 13
    thick = [3.0, 3.0, 4.5]
    turns = [torch.eye(3), torch.tensor([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]), torch.tensor([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])]
    tf = []
    for t, turn in zip(thick, turns):  # (x = R (p + t) + centre: a stack's rotation goes in front of its slices')
        p = _poses(n_stack, t, g)
        tf.append(torch.cat([turn @ p[:, :, :3], p[:, :, 3:]], 2))
    tf = torch.cat(tf).contiguous().to(device)
    n = tf.shape[0]
    per_slice = [t for t in thick for _ in range(n_stack)]
    bank = bank_for(per_slice, res_s, 1.0, device)
    vol = torch.rand((1, 1, N, N, N), generator=g).to(device)
    y = (torch.rand((n, 1, hw, hw), generator=g) + 0.1).to(device)
    m = (torch.rand((n, 1, hw, hw), generator=g) < 0.7).to(device)
    tfk = tf[:, None].repeat(1, K, 1, 1)
    for k in range(1, K):  # one finite-difference gradient, as tools/bench_acq.py builds it
        ax = (k - 1) // 2 % 3
        if k <= 6:
            tfk[:, k, ax, 3] += 0.5 if k % 2 else -0.5
        else:
            tfk[:, k, :, (ax + 1) % 3] += (0.01 if k % 2 else -0.01) * tf[:, :, (ax + 2) % 3]
    tfk = tfk.contiguous()
    common = {"slices": n, "slice_size": hw, "volume": N, "members": [list(p.shape) for p in bank.psfs], "repeats": a.repeats}

    def composed(fn):
        def run():
            os.environ["NESVOR_PSF_BANK"] = "composed"
            try:
                return fn()
            finally:
                os.environ.pop("NESVOR_PSF_BANK", None)
        return run

    def sums_composed():
        out = []
        for _, psf, idx in bank.members():
            out.append(torch.ops.nesvor.svr_similarity(vol[0, 0], psf, tfk[idx].contiguous(), y[idx].contiguous(), m[idx].contiguous(), res_s))
        return out

    calls = {
        "A": lambda: slice_acquisition_bank(tf, vol, None, m, bank, (hw, hw), res_s, False),
        "A^T equalised": lambda: slice_acquisition_adjoint_bank(tf, bank, y, m, None, (N, N, N), res_s, False, True),
    }
    for what, fn in calls.items():
        ms = _alternate({"fused": fn, "composed": composed(fn)}, 3, a.repeats)
        print(json.dumps({"what": what, **common, "fused": _stats(ms["fused"]), "composed": _stats(ms["composed"]),
                          "fused_peak_mb": _peak(fn), "composed_peak_mb": _peak(composed(fn))}), flush=True)
    fused_sums = lambda: torch.ops.nesvor.svr_similarity_bank(vol[0, 0], bank.flat, bank.table, bank.ids, tfk, y, m, res_s)
    ms = _alternate({"fused": fused_sums, "composed": sums_composed}, 3, a.repeats)
    print(json.dumps({"what": "13-pose similarity gradient", **common, "fused": _stats(ms["fused"]), "composed": _stats(ms["composed"]),
                      "fused_peak_mb": _peak(fused_sums), "composed_peak_mb": _peak(sums_composed)}), flush=True)

    # a whole reconstruction: the three stacks at world poses in mm (voxels of 1 mm: the same numbers)
    stacks = [(y[j * n_stack:(j + 1) * n_stack] * m[j * n_stack:(j + 1) * n_stack]).contiguous() for j in range(3)]
    poses = [RigidTransform(tf[j * n_stack:(j + 1) * n_stack].contiguous()) for j in range(3)]
    rec = lambda: reconstruct_volume(stacks, None, poses, res_s, per_slice, 1.0, n_iter=a.steps)
    ms = _alternate({"fused": rec, "composed": composed(rec)}, 1, max(a.repeats // 3, 3))
    print(json.dumps({"what": f"reconstruct_volume, {a.steps} steps", **common, "volume_shape": list(rec().image.shape),
                      "fused": _stats(ms["fused"]), "composed": _stats(ms["composed"]), "fused_peak_mb": _peak(rec),
                      "composed_peak_mb": _peak(composed(rec))}), flush=True)

    # a bank of one against the one-PSF entry point, and that entry point against itself
    psf = get_PSF(res_ratio=(res_s, res_s, 3.0), device=device)
    one = bank_for([3.0] * n, res_s, 1.0, device)
    assert torch.is_tensor(one) and torch.equal(one, psf)
    from nesvor_amd.psf_bank import PsfBank

    bank1 = PsfBank([psf], [0] * n)
    pairs = {
        "A": (lambda: slice_acquisition_bank(tf, vol, None, m, bank1, (hw, hw), res_s, False),
              lambda: slice_acquisition(tf, vol, None, m, psf, (hw, hw), res_s, False, False)),
        "A^T equalised": (lambda: slice_acquisition_adjoint_bank(tf, bank1, y, m, None, (N, N, N), res_s, False, True),
                          lambda: slice_acquisition_adjoint(tf, psf, y, m, None, (N, N, N), res_s, False, True)),
        "13-pose similarity gradient": (lambda: torch.ops.nesvor.svr_similarity_bank(vol[0, 0], bank1.flat, bank1.table, bank1.ids, tfk, y, m, res_s),
                                        lambda: torch.ops.nesvor.svr_similarity(vol[0, 0], psf, tfk, y, m, res_s)),
    }
    for what, (b, o) in pairs.items():
        ms = _alternate({"bank_of_one": b, "one_psf": o}, 3, a.repeats)
        sb, so = _stats(ms["bank_of_one"]), _stats(ms["one_psf"])
        print(json.dumps({"what": f"bank of one: {what}", **common, "bank_of_one": sb, "one_psf": so,
                          "cost_ms": round(sb["median_ms"] - so["median_ms"], 4), "one_psf_spread_ms": so["max_minus_median_ms"]}), flush=True)


if __name__ == "__main__":
    main()
