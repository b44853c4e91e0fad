"""Times the joint-histogram entry point of the mutual-information similarity (csrc/svr_nmi.hip, nesvor_amd/nmi.py) against the moment
sums of csrc/svr.hip on the same inputs, and ``register_slices`` with ``nmi`` against ``ncc``.

    python tools/bench_svr_nmi.py [--repeats 21] [--skip-pipeline]

Workload of the kernel figures: tools/bench_psf_bank.py's - 3 stacks of 40 slices of 128^2 pixels of 1.5 mm against a 128^3 volume of
1 mm, 3 mm slices (one PSF), masks of about 70 % - with the 13 poses of one finite-difference gradient and with K = 1 (the accept
test).  Arms, alternating inside every repeat: ``svr_similarity``; ``svr_joint_histogram`` at 32 and 64 bins; the composed definition
(13 ``slice_acquisition`` launches and the torch integer binning) at 32 bins, whose result must equal the kernel's.  Then the whole
``register_slices`` on the three-stack 48^3 phantom of tests/test_svr.py, host clock around a device synchronise.  HIP events, warm,
medians and ranges; one JSON object per line.  ``NESVOR_HIP_LIB`` names another build of the library (segment lengths were compared
that way: DESIGN.md, "Mutual-information similarity")."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--skip-composed", action="store_true")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_svr_nmi.py measures on the GPU: no HIP device found")
    from bench_acq import _poses
    from bench_psf_bank import _alternate, _stats
    from nesvor_amd import nmi
    from nesvor_amd import ops  # noqa: F401  (registers torch.ops.nesvor)
    from nesvor_amd.slice_acquisition import slice_acquisition
    from nesvor_amd.utils import get_PSF

    device = torch.device("cuda:0")
    g = torch.Generator().manual_seed(120)
    n_stack, hw, N, res_s, K = 40, 128, 128, 1.5, 13
    turns = [torch.eye(3), torch.tensor([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]), torch.tensor([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])]
    tf = []
    for turn in turns:
        p = _poses(n_stack, 3.0, g)
        tf.append(torch.cat([turn @ p[:, :, :3], p[:, :, 3:]], 2))
    tf = torch.cat(tf).contiguous().to(device)
    n = tf.shape[0]
    psf = get_PSF(res_ratio=(res_s, res_s, 3.0), device=device)
    vol = torch.rand((N, N, N), generator=g).to(device)
    y = (torch.rand((n, hw, hw), generator=g) + 0.1).to(device)
    m = (torch.rand((n, hw, hw), generator=g) < 0.7).to(device)
    tfk = tf[:, None].repeat(1, K, 1, 1)
    for k in range(1, K):  # one finite-difference gradient, as tools/bench_acq.py builds it
        ax = (k - 1) // 2 % 3
        if k <= 6:
            tfk[:, k, ax, 3] += 0.5 if k % 2 else -0.5
        else:
            tfk[:, k, :, (ax + 1) % 3] += (0.01 if k % 2 else -0.01) * tf[:, :, (ax + 2) % 3]
    tfk = tfk.contiguous()
    tf1 = tfk[:, :1].contiguous()
    common = {"slices": n, "slice_size": hw, "volume": N, "psf": list(psf.shape), "repeats": a.repeats,
              "lib": os.environ.get("NESVOR_HIP_LIB", "")}
    maps = {}
    for bins in (32, 64):
        maps[bins] = (tuple(nmi.axis_map(vol.min(), vol.max(), bins).tolist()), nmi.axis_map(*nmi.masked_range(y, m), bins).contiguous())

    def hist(t, bins):
        return torch.ops.nesvor.svr_joint_histogram(vol, psf, t, y, m, res_s, *maps[bins][0], maps[bins][1], bins)

    def composed(t, bins):
        out = []
        for k in range(t.shape[1]):
            sim, wgt = slice_acquisition(t[:, k].contiguous(), vol[None, None], None, m[:, None], psf, (hw, hw), res_s, True, False)
            out.append(nmi.joint_histogram(sim[:, 0].flatten(1), y.flatten(1), (m & (wgt[:, 0] > 0)).flatten(1), *maps[bins], bins))
        return torch.stack(out, 1)

    for what, t in (("13-pose gradient", tfk), ("K = 1 accept test", tf1)):
        arms = {"svr_similarity": lambda: torch.ops.nesvor.svr_similarity(vol, psf, t, y, m, res_s),
                "joint_histogram_32": lambda: hist(t, 32), "joint_histogram_64": lambda: hist(t, 64)}
        if not a.skip_composed:
            arms["composed_32"] = lambda: composed(t, 32)
            assert torch.equal(hist(t, 32), composed(t, 32)), "the kernel's histogram differs from the composed definition"
        ms = _alternate(arms, 3, a.repeats)
        print(json.dumps({"what": what, **common, **{k: _stats(v) for k, v in ms.items()}}), flush=True)

    if a.skip_pipeline:
        return
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_svr import _RES_S, _phantom_stacks, _simulated_ncc
    from nesvor_amd.registration import register_slices

    out = {"what": "register_slices, three-stack 48^3 phantom", "runs": 3, "lib": common["lib"]}
    for similarity in ("ncc", "nmi"):
        register_slices(_phantom_stacks(device), res_s=_RES_S, similarity=similarity)  # warm
        secs = []
        for _ in range(3):
            stacks = _phantom_stacks(device)
            torch.cuda.synchronize()
            t0 = time.time()
            done = register_slices(stacks, res_s=_RES_S, similarity=similarity)
            torch.cuda.synchronize()
            secs.append(time.time() - t0)
        out[similarity] = {"median_s": round(statistics.median(secs), 3), "min_s": round(min(secs), 3), "max_s": round(max(secs), 3),
                           "simulated_ncc": round(_simulated_ncc(done), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
