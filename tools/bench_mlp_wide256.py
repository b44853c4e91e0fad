"""Forward + backward of one wide network (default 256 x 2 hidden, 32 inputs, 16 outputs, N = 2^18) through the hand-written
wide kernels (``mlp.wide_mlp``: csrc/mlp_wide.hip's chunked-image kernels above width 128) and through ``mlp.library_mlp``
(rocBLAS under autograd - what these widths ran on before), both differentiated in the input and the parameters.

    python tools/bench_mlp_wide256.py [--width 256] [--depth 2] [--n-log2 18] [--repeats 20] [--regions 5]

Timed with the HIP-event helper of the package (``_lib.kernel_timer``): after a warm-up, ``--regions`` regions of ``--repeats``
forward + backward passes each; the figure is the median region divided by the repeats.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--width", type=int, default=256)
    p.add_argument("--depth", type=int, default=2)
    p.add_argument("--n-log2", type=int, default=18)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--regions", type=int, default=5)
    a = p.parse_args()
    from nesvor_amd import _lib, mlp

    dev = torch.device("cuda:0")
    k_b, out_dim, S, N = 32, 16, 256, 1 << a.n_log2
    torch.manual_seed(0)
    dims = [k_b] + [a.width] * a.depth + [out_dim]
    layers = []
    for i, o in zip(dims, dims[1:]):
        layers += [nn.Linear(i, o), nn.ReLU()]
    net = nn.Sequential(*layers[:-1]).to(dev)
    assert mlp.wide_supported(net)
    xb = torch.randn(k_b, N, device=dev, requires_grad=True)
    dy = torch.randn(out_dim, N, device=dev)

    def run(fn):
        y = fn(net, None, xb, 0, k_b, S)
        y.backward(dy)
        xb.grad = None
        net.zero_grad(set_to_none=True)

    paths = {"wide_mlp": mlp.wide_mlp, "library_mlp": mlp.library_mlp}
    for fn in paths.values():  # warm-up: allocator, dynamic-LDS limits, rocBLAS kernel selection
        for _ in range(5):
            run(fn)
    torch.cuda.synchronize()
    _lib.kernel_timer.reset(True)
    for _ in range(a.regions):
        for name, fn in paths.items():
            with _lib.kernel_timer.span(name):
                for _ in range(a.repeats):
                    run(fn)
    torch.cuda.synchronize()
    rec = _lib.kernel_timer.records
    out = {"width": a.width, "depth": a.depth, "k_b": k_b, "out_dim": out_dim, "N": N, "repeats": a.repeats, "regions": a.regions}
    for name in paths:
        ts = sorted(s.elapsed_time(e) / a.repeats for s, e in rec[name])
        out[name + "_ms"] = round(ts[len(ts) // 2], 4)
        out[name + "_ms_min_max"] = [round(ts[0], 4), round(ts[-1], 4)]
    for k in ("mlp_fwd", "mlp_bwd"):  # the wide launches alone (events around each native call)
        ts = sorted(s.elapsed_time(e) for s, e in rec[k])
        out[k + "_launch_ms"] = round(ts[len(ts) // 2], 4)
    out["library_over_wide"] = round(out["library_mlp_ms"] / out["wide_mlp_ms"], 3)
    _lib.kernel_timer.reset(False)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
