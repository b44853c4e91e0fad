"""Times the stack assessment (nesvor_amd/assess.py) on the GPU, fused against composed.

    python tools/bench_assess.py [--stacks 3] [--slices 40] [--size 128] [--metric matrix-rank] [--repeats 21]

``assess_stacks`` on stacks x slices of size^2 pixels (a disc mask of about 70 %), alternating between the fused pair moments
(``torch.ops.nesvor.pair_moments``, csrc/assess.hip) and the torch expression (``NESVOR_ASSESS=composed``); also the
``pair_moments`` call alone on both paths (the rest - the pair list, the read-back, the eigenvalues of a slices x slices matrix
per stack on the host - is the same).  HIP events, warm, medians.  For the composed path also the device memory its temporaries
take: the peak above the inputs and the total it allocates during one call.  One JSON object per line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _alternate(fns, warmup, repeats):
    """Medians (and ranges) of several callables timed in turn, so that drift hits all of them alike."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def _memory(f):
    """(peak bytes above what was allocated before the call, bytes allocated during the call) of one call of f."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_stats()
    f()
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats()
    return (after["allocated_bytes.all.peak"] - before["allocated_bytes.all.current"],
            after["allocated_bytes.all.allocated"] - before["allocated_bytes.all.allocated"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=3)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--metric", default="matrix-rank", choices=["ncc", "matrix-rank", "volume"])
    ap.add_argument("--repeats", type=int, default=21)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assess.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import assess
    from nesvor_amd.image import Stack

    device = torch.device("cuda:0")
    n, s = a.slices, a.size
    g = torch.Generator().manual_seed(n * s)
    yy, xx = torch.meshgrid(torch.arange(s), torch.arange(s), indexing="ij")
    disc = ((yy - s / 2) ** 2 + (xx - s / 2) ** 2 < (0.47 * s) ** 2)[None, None]
    stacks = []
    for _ in range(a.stacks):
        img = (1 + 0.5 * torch.randn(n, 1, s, s, generator=g)).abs() + 0.1
        stacks.append(Stack((img * disc).to(device), disc.expand(n, 1, s, s).contiguous().to(device), resolution_x=1.0, resolution_y=1.0,
                            thickness=3.0, gap=3.0))
    data = torch.cat([st.slices * st.mask for st in stacks]).contiguous()
    mask = torch.cat([st.mask for st in stacks]).contiguous()
    pairs = torch.tensor([(j * n + i, j * n + k) for j in range(a.stacks) for i, k in assess.stack_pairs(n, a.metric)])
    pairs_dev = pairs.to(torch.int32).to(device)

    def whole(mode):
        def f():
            if mode == "composed":
                os.environ["NESVOR_ASSESS"] = "composed"
            try:
                return assess.assess_stacks(stacks, a.metric)
            finally:
                os.environ.pop("NESVOR_ASSESS", None)
        return f

    os.environ.pop("NESVOR_ASSESS", None)
    fns = {"assess_fused": whole("fused"), "assess_composed": whole("composed"),
           "moments_fused": lambda: torch.ops.nesvor.pair_moments(data, mask, pairs_dev),
           "moments_composed": lambda: assess.pair_moments_composed(data, mask, pairs_dev)}
    r = _alternate(fns, 3, a.repeats)
    peak_c, total_c = _memory(fns["moments_composed"])
    peak_f, total_f = _memory(fns["moments_fused"])
    fused, composed = whole("fused")(), whole("composed")()
    P, pixels = int(pairs.shape[0]), s * s
    print(json.dumps({"what": "assess_stacks", "metric": a.metric, "stacks": a.stacks, "slices": n, "size": s, "pairs": P,
                      "repeats": a.repeats, **r,
                      "speedup_assess": r["assess_composed"]["median_ms"] / r["assess_fused"]["median_ms"],
                      "speedup_moments": r["moments_composed"]["median_ms"] / r["moments_fused"]["median_ms"],
                      "moments_fused_read_bytes": 10 * P * pixels,
                      "moments_fused_TBps": 10 * P * pixels / (r["moments_fused"]["median_ms"] * 1e-3) / 1e12,
                      "composed_peak_temporary_bytes": peak_c, "composed_allocated_bytes": total_c,
                      "fused_peak_temporary_bytes": peak_f, "fused_allocated_bytes": total_f,
                      "scores_fused": [x["score"] for x in fused], "scores_composed": [x["score"] for x in composed],
                      "ranks_fused": [x["rank"] for x in fused], "ranks_composed": [x["rank"] for x in composed]}), flush=True)


if __name__ == "__main__":
    main()
