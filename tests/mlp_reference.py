"""Shared reference code of the MLP kernel tests (a plain module, not a conftest): random networks and inputs, the layouts of
the kernels' saved buffers, and the same network evaluated in torch - in float64 (the reference), in float32 (the yardstick an
fp32-accuracy kernel is measured against) or with the 16-bit operand modes' rounding points spelled out.

Layouts (csrc/mlp.hip, csrc/mlp_wide.hip):

* full save: one buffer per hidden layer, accumulator fragments [16-sample group][16-feature block][lane = 16 q + j][r]
  = feature 16 block + 4 q + r of sample 16 group + j; fp32, or the 16-bit type in the BF16 / FP16 modes; 4 blocks at width 64,
  8 in the wide kernels above it;
* compact save: ``saved[0]`` holds one uint32 per (group, lane = 16 q + j): bit 16 l + 4 b + r = [pre-activation of unit
  16 b + 4 q + r of hidden layer l has its sign bit clear] for sample 16 group + j;
* partial sums: rows to be summed, columns W0, b0, W1, b1, ... (a bias-free network: W0, W1, ...).
"""
import math

import torch

UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # |round(x) - x| <= u |x| (8 / 11 significand bits)


def make_net(device, depth, k_in, out_dim, biased, seed, width=64):
    """Xavier-uniform weights, N(0, 0.1^2) biases (zeros when not ``biased``) of a Linear/ReLU stack -> (W, B) lists."""
    g = torch.Generator().manual_seed(seed)
    dims = [k_in] + [width] * depth + [out_dim]
    W = [(torch.rand(o, i, generator=g) * 2 - 1) * math.sqrt(6.0 / (i + o)) for i, o in zip(dims, dims[1:])]
    B = [(0.1 * torch.randn(o, generator=g)) if biased else torch.zeros(o) for o in dims[1:]]
    return [w.to(device) for w in W], [b.to(device) for b in B]


def make_inputs(device, k_a, rows, N, S, out_dim, seed):
    """-> (xa (N / S, k_a) | None, xb (rows, N), dy (out_dim, N)), standard normal."""
    g = torch.Generator().manual_seed(seed)
    xa = torch.randn(N // S, k_a, generator=g).to(device) if k_a else None
    xb = torch.randn(rows, N, generator=g).to(device)
    dy = torch.randn(out_dim, N, generator=g).to(device)
    return xa, xb, dy


def network_input(xa, xb, b_row0, k_b, S, dtype=torch.float64):
    """The network's input rows (N, k_a + k_b): [pixel features broadcast over each pixel's S samples | rows of xb]."""
    x = xb[b_row0 : b_row0 + k_b].t().to(dtype)
    if xa is not None:
        x = torch.cat([xa.to(dtype).repeat_interleave(S, 0), x], 1)
    return x


def saved_rows(s, N, blocks=4):
    """Full-save fragments [group][block][lane = 16 q + j][r] -> (N, 16 blocks) float64 activations (feature 16 block + 4 q + r,
    sample 16 group + j)."""
    G = s.numel() // (256 * blocks)
    return s.view(G, blocks, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(G * 16, 16 * blocks)[:N].double()


def compact_gates(words, N, depth):
    """Compact save (``saved[0]`` of N / 16 * 64 words) -> one (N, 64) bool tensor per hidden layer: the gates the backward uses."""
    w = words.view(torch.int32).view(N // 16, 4, 16)  # [group][q][sample]
    bits = ((w[..., None] >> torch.arange(32, device=w.device, dtype=torch.int32)) & 1) != 0  # [group][q][sample][bit]
    out = []
    for l in range(depth):
        b = bits[..., 16 * l : 16 * l + 16].view(N // 16, 4, 16, 4, 4)  # [group][q][sample][block][r]
        out.append(b.permute(0, 2, 3, 1, 4).reshape(N, 64))  # unit 16 block + 4 q + r
    return out


def split_partial(flat, W, B):
    """Summed partial row -> [(dW, db | None) per layer] (``B`` empty or of None entries: a bias-free network)."""
    off, out = 0, []
    for i, w in enumerate(W):
        dw = flat[off : off + w.numel()].view_as(w)
        off += w.numel()
        b = B[i] if B else None
        db = None
        if b is not None:
            db = flat[off : off + b.numel()]
            off += b.numel()
        out.append((dw, db))
    assert off == flat.numel()
    return out


def forward_chain(W, B, x, dtype=torch.float64):
    """The plain network in ``dtype``: -> (pre-activations of every hidden layer, y (N, out_dim))."""
    pre, h = [], x.to(dtype)
    for l, w in enumerate(W):
        z = h @ w.to(dtype).t()
        if B and B[l] is not None:
            z = z + B[l].to(dtype)
        if l == len(W) - 1:
            return pre, z
        pre.append(z)
        h = z.relu()


def gated_chain(W, B, x, dy, gates, dtype=torch.float64):
    """Forward and backward of the network in ``dtype`` with the backward's ReLU gates GIVEN (the kernel's own: either choice is a
    valid subgradient where a pre-activation is within rounding of zero) -> dict(pre, y, dx (N, k_in), grads [(dW, db)]).
    ``dtype`` float64: the reference; float32: the yardstick of the fp32-accuracy kernels (same terms, another order)."""
    pre, y = forward_chain(W, B, x, dtype)
    hs = [p.relu() for p in pre]
    d = dy.t().to(dtype)
    grads = [None] * len(W)
    # The bias gradient as the product with a column of ones - the same GEMM as dW, so that the float32 evaluation sums it as
    # the kernels do, in chains.  (torch.sum is a pairwise tree: its float32 error grows with log N, not sqrt N, and a healthy
    # chain sum of 2^18 terms - 2e-8 of the largest db - already exceeds four times the tree's 5e-9.)
    ones = torch.ones(d.shape[0], 16, dtype=dtype, device=d.device)
    for l in range(len(W) - 1, -1, -1):
        inp = hs[l - 1] if l > 0 else x.to(dtype)
        grads[l] = (d.t() @ inp, (d.t() @ ones)[:, 0])
        d = d @ W[l].to(dtype)
        if l > 0:
            d = d * gates[l - 1].to(dtype)
    return {"pre": pre, "y": y, "dx": d, "grads": grads}


def emulated_backward(W, B, xa, xb, dy, saved, b_row0, k_b, S, dt):
    """float64 backward with the 16-bit kernels' rounding points (csrc/mlp.hip, mlp_bwd_dx16_kernel's header): dY and every dpre
    rounded to the 16-bit type before a product, weights and the network input rounded, saved activations as the forward wrote
    them.  ``dt`` None: no rounding.  -> (dX (N, k_in), [(dW, db) per layer])"""
    N = xb.shape[1]
    rn = (lambda t: t.to(dt).double()) if dt is not None else (lambda t: t.double())
    x = network_input(xa, xb, b_row0, k_b, S)
    H = [saved_rows(s, N) for s in saved]
    g = dy.t().double()
    grads = [None] * len(W)
    a = rn(g)
    grads[-1] = (a.t() @ H[-1], g.sum(0))
    dh = a @ rn(W[-1])
    for l in range(len(W) - 2, -1, -1):
        dpre = dh * (H[l] > 0)
        a = rn(dpre)
        inp = H[l - 1] if l > 0 else rn(x)
        grads[l] = (a.t() @ inp, dpre.sum(0))
        dh = a @ rn(W[l])
    return dh, grads


def emulated_forward_layers(W, B, x, H, dt):
    """The 16-bit operand modes' forward, layer by layer on the activations the kernel itself saved (``H``: (N, 64) float64 per
    hidden layer): both operands of every product rounded to ``dt``, float64 accumulation, fp32 bias.  -> (pre-activations of
    every hidden layer, y (N, out_dim)).  Layer l's result depends on the kernel only through its saved layer l - 1, so a value on
    a 16-bit rounding boundary that the kernel rounded the other way does not travel through the reference."""
    rn = lambda t: t.to(dt).double()
    pre = []
    for l, w in enumerate(W):
        inp = rn(x) if l == 0 else H[l - 1]
        z = inp @ rn(w).t() + B[l].double()
        if l == len(W) - 1:
            return pre, z
        pre.append(z)


def rel_err(a, b):
    """max |a - b| / max |b| in float64."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def bits_equal(a, b):
    """Bit patterns (saved gate words are arbitrary bit patterns, some of them NaNs as floats)."""
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))
