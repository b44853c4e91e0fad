"""Times one EM round of the robust statistics (nesvor_amd/robust.py) on the GPU, fused against composed.

    python tools/bench_robust.py [--slices 120] [--size 128] [--repeats 21]

``RobustStatistics.update`` on n slices of size^2 pixels (a mask of 70 %), alternating between the fused E-step
(``torch.ops.nesvor.robust_estep``, csrc/robust.hip) and the torch expression ``NESVOR_ROBUST=composed`` runs; also the
E-step alone on both paths (the rest of a round is the same few dozen operations on n-vectors).  HIP events, warm, medians.
One JSON object per line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=120)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=21)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust.py measures on the GPU: no HIP device found")
    import nesvor_amd.ops  # noqa: F401
    from nesvor_amd import robust

    device = torch.device("cuda:0")
    n, s = a.slices, a.size
    g = torch.Generator().manual_seed(n * s)
    sim = (0.1 + 0.8 * torch.rand(n, 1, s, s, generator=g)).to(device)
    gain = (0.7 + 0.6 * torch.rand(n, 1, 1, 1, generator=g)).to(device)
    y = (sim + 0.02 * torch.randn(n, 1, s, s, generator=g).to(device)) / gain
    mask = (torch.rand(n, 1, s, s, generator=g) < 0.7).to(device)
    os.environ.pop("NESVOR_ROBUST", None)
    state = robust.RobustStatistics().init(sim, y, mask)
    scale, model = state.scale.clone(), state.model.clone()

    def round_of(mode):
        def f():
            if mode == "composed":
                os.environ["NESVOR_ROBUST"] = "composed"
            try:
                state.scale, state.model = scale, model  # every round from one state
                state.slice_weight = torch.ones_like(scale)
                state.update(sim, y, mask)
            finally:
                os.environ.pop("NESVOR_ROBUST", None)
        return f

    fns = {"round_fused": round_of("fused"), "round_composed": round_of("composed"),
           "estep_fused": lambda: torch.ops.nesvor.robust_estep(sim, y, mask, scale, model),
           "estep_composed": lambda: robust.estep_composed(sim, y, mask, scale, model)}
    r = _alternate(fns, 3, a.repeats)
    pixels = n * s * s
    print(json.dumps({"what": "one EM round", "slices": n, "size": s, "repeats": a.repeats, **r,
                      "speedup_round": r["round_composed"]["median_ms"] / r["round_fused"]["median_ms"],
                      "speedup_estep": r["estep_composed"]["median_ms"] / r["estep_fused"]["median_ms"],
                      "estep_fused_bytes": 13 * pixels,
                      "estep_fused_TBps": 13 * pixels / (r["estep_fused"]["median_ms"] * 1e-3) / 1e12}), flush=True)


if __name__ == "__main__":
    main()
