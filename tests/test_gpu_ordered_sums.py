"""The summation order of the slice-statistics kernels (csrc/slice_sums.h), pinned: the per-entry sums of ``pair_moments``,
``robust_estep`` and ``structural_ssim`` are rebuilt on the host from the fp32 per-pixel terms in the documented order and must
equal the kernel's output bit for bit.

The order.  A workgroup is 256 pixels of one entry: pixel ``pix`` of a flat slice goes to workgroup ``pix // 256`` for
``pair_moments`` and ``robust_estep``; ``structural_ssim`` has 16 x 16 tiles, numbered ``tile_y * tiles_x + tile_x``, with thread
``ty * 16 + tx``.  Thread t is lane ``t % 64`` of wave ``t // 64``; a lane off the mask or past the edge holds 0.  A wave adds
its 64 lanes as a balanced pairwise tree (``x[0::2] + x[1::2]``, six times) in fp32 - in double for the six float sums of
``structural_ssim`` - the four waves are added as ``(w0 + w1) + (w2 + w3)`` in double and the workgroups of an entry one after
the other from 0 in double.

Values are of the order of 1e3 with a spread, so that the order shows: wherever an entry has 64 valid pixels or more, the same
terms added one after the other in fp32 must give other bits than the tree (asserted).  ``p`` and the SSIM map are the kernel's
own: their expf and division chains are not reproduced here, the sums over them are."""
import pytest
import torch

LINEAR = [(2, 1, 1), (3, 1, 65), (3, 17, 31)]  # one lane; a second wave with one live lane; three workgroups, the last of 15 pixels
TILED = [(2, 1, 1), (3, 1, 65), (2, 19, 23), (1, 5, 5)]  # ...; 2 x 2 ragged tiles; one ragged tile
KINDS = ["none", "random", "entry"]  # no mask; about 70 % valid; that and one entry fully masked out
THRESHOLD, DYNAMIC_RANGE = 0.5, 1e3
_DATA = {}


def _data(shape, kind):
    """sim of 1 .. 1e3 (squared uniform: a spread of magnitudes), y = (sim + noise of 30) / gain, the gains as scales, and the
    mask; on the host, shared by the tests and never written."""
    key = (shape, kind)
    if key not in _DATA:
        n, h, w = shape
        g = torch.Generator().manual_seed(1000 * n + 10 * h + w)
        sim = 1 + 1e3 * torch.rand(n, h, w, generator=g) ** 2
        scale = 0.7 + 0.6 * torch.rand(n, generator=g)
        y = (sim + 30 * torch.randn(n, h, w, generator=g)) / scale.view(n, 1, 1)
        mask = None
        if kind != "none":
            mask = torch.rand(n, h, w, generator=g) < 0.7
            if kind == "entry":
                mask[n - 1] = False
        _DATA[key] = (sim, y, mask, scale)
    return _DATA[key]


def _chunks(t):
    """(e, h, w) -> (e, workgroups, 256): 256 consecutive pixels per workgroup, 0 past the edge."""
    flat = t.flatten(1)
    pad = -flat.shape[1] % 256
    return torch.nn.functional.pad(flat, (0, pad)).reshape(flat.shape[0], -1, 256)


def _tiles(t):
    """(e, h, w) -> (e, tiles, 256): 16 x 16 tiles in row-major order, thread ty * 16 + tx, 0 past the edge."""
    e, h, w = t.shape
    t = torch.nn.functional.pad(t, (0, -w % 16, 0, -h % 16))
    ty, tx = t.shape[1] // 16, t.shape[2] // 16
    return t.reshape(e, ty, 16, tx, 16).permute(0, 1, 3, 2, 4).reshape(e, ty * tx, 256)


def _ordered(terms, in_double=False):
    """(e, workgroups, 256) fp32 -> (e) float64 in the kernels' order; ``in_double``: the wave's tree runs in double too."""
    x = terms.reshape(*terms.shape[:2], 4, 64)
    x = x.double() if in_double else x
    for _ in range(6):
        x = x[..., 0::2] + x[..., 1::2]
    wave = x[..., 0].double()
    group = (wave[..., 0] + wave[..., 1]) + (wave[..., 2] + wave[..., 3])
    total = torch.zeros(terms.shape[0], dtype=torch.float64)
    for g in range(group.shape[1]):
        total = total + group[:, g]
    return total


def _sequential(terms):
    """The same terms added one after the other in fp32."""
    flat = terms.flatten(1)
    total = torch.zeros(flat.shape[0], dtype=torch.float32)
    for i in range(flat.shape[1]):
        total = total + flat[:, i]
    return total.double()


def _check(got, columns, in_double=()):
    """``got`` (e, N) from the kernel against the N term arrays ``columns`` (each (e, workgroups, 256) fp32, column 0 the
    validity): equal bits in the documented order, exact zeros for an entry without a valid pixel, and an order that shows."""
    assert all(c.dtype == torch.float32 for c in columns)
    want = torch.stack([_ordered(c, j in in_double) for j, c in enumerate(columns)], 1)
    plain = torch.stack([_sequential(c) for c in columns], 1)
    count = columns[0].flatten(1).sum(1)
    got = got.cpu()
    print(f"valid pixels {count.tolist()}; entries whose sequential fp32 sums differ from the tree: "
          f"{int((plain != want).any(1).sum())} of {len(count)}; kernel == tree: {torch.equal(got, want)}")
    if float(count.max()) >= 64:
        assert bool((plain != want).any()), "the values do not make the order visible"
    assert bool((want[count == 0] == 0).all()) and bool((got[count == 0] == 0).all())
    assert got.dtype == torch.float64 and torch.equal(got, want)


def pair_moment_terms(x, mask, pairs):
    a, b = x[[p[0] for p in pairs]], x[[p[1] for p in pairs]]
    on = torch.ones_like(a, dtype=torch.bool) if mask is None else mask[[p[0] for p in pairs]] & mask[[p[1] for p in pairs]]
    a, b = a * on, b * on
    return [_chunks(t) for t in (on.float(), a, b, a * a, b * b, a * b)]


def robust_terms(sim, y, mask, scale, p):
    on = torch.ones_like(sim, dtype=torch.bool) if mask is None else mask
    e = scale.view(-1, 1, 1) * y - sim
    e2 = e * e * on
    q = 1 - p
    py = p * y
    return [_chunks(t) for t in (on.float(), p * on, p * e2, q * q * on, py * sim * on, py * y * on, e2)]


def structural_terms(sim, y, mask, scale, ssim):
    on = torch.ones_like(sim, dtype=torch.bool) if mask is None else mask
    i, j = scale.view(-1, 1, 1) * y * on, sim * on
    below = on & (ssim < THRESHOLD)
    return [_tiles(t) for t in (on.float(), ssim * on, below.float(), i, j, i * i, j * j, i * j)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", LINEAR)
def test_pair_moments_sum_in_the_documented_order(device, shape, kind):
    """Every pair of the stack: ordinary, self- and reversed pairs."""
    import nesvor_amd  # noqa: F401  (registers torch.ops.nesvor)

    x, _, mask, _ = _data(shape, kind)
    pairs = [(i, j) for i in range(shape[0]) for j in range(shape[0])]
    dev_mask = None if mask is None else mask.to(device)
    got = torch.ops.nesvor.pair_moments(x.to(device), dev_mask, torch.tensor(pairs, dtype=torch.int32, device=device))
    _check(got, pair_moment_terms(x, mask, pairs))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", LINEAR)
def test_robust_estep_sums_in_the_documented_order(device, shape, kind):
    import nesvor_amd  # noqa: F401

    sim, y, mask, scale = _data(shape, kind)
    model = torch.tensor([900.0, 0.9, 1e-3])  # sigma of the noise, so that p spreads over (0, 1)
    dev_mask = None if mask is None else mask.to(device)
    p, got = torch.ops.nesvor.robust_estep(sim.to(device), y.to(device), dev_mask, scale.to(device), model.to(device))
    p = p.cpu()
    if mask is not None:
        assert bool((p[~mask] == 0).all())
    _check(got, robust_terms(sim, y, mask, scale, p))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", TILED)
def test_structural_ssim_sums_in_the_documented_order(device, shape, kind):
    import nesvor_amd  # noqa: F401

    sim, y, mask, scale = _data(shape, kind)
    dev_mask = None if mask is None else mask.to(device)
    ssim, got = torch.ops.nesvor.structural_ssim(sim.to(device), y.to(device), dev_mask, scale.to(device), THRESHOLD, DYNAMIC_RANGE)
    ssim = ssim.cpu()
    if mask is not None:
        assert bool((ssim[~mask] == 0).all())
    _check(got, structural_terms(sim, y, mask, scale, ssim), in_double=(1, 3, 4, 5, 6, 7))
