"""The kernels of csrc/loss.hip, each driven through the C ABI at the edges of its code paths and compared with a float64
restatement on the CPU (tests/loss_reference.py) under the two acceptance rules of tests/step_reference.py:

* nesvor_imaging_loss: the imaging model, three losses and every gradient in one launch.  S = 64, 128, 256, 512 run
  imaging_loss_cached_kernel<REG, K> (K = 1, 2, 4, 8: a pixel's samples in registers, the mirror through a wave permute), every
  other S imaging_loss_kernel<REG> (lane-strided trips of 64 samples, two passes) - S = 192 and 1024 included, which are
  multiples of 64 without a cached instantiation.  Calibrated rule per output: err_kernel <= 4 err_torch_fp32 + 8 2^-24 scale.
* nesvor_slice_grads: per-pixel -> per-slice sums by global atomics; the slice-embedding gradient has three paths (_path below).
* nesvor_slice_grads_by_slice: the same sums by one workgroup per slice, reproducible.
  Sum rule for both: |err| <= (T + 2) 2^-24 sum|terms| per output element, the value the output held before counted as a term.

Every output buffer is longer than the kernel needs and prefilled; "untouched" and "bit for bit" are torch.equal.
"""
import ctypes

import pytest
import torch

import loss_reference as L

pytestmark = pytest.mark.gpu

CANARY = -7.25
PAD = 67  # floats behind every output
REGS = ["edge", "TV", "L2"]
FULL = (True, True, True, True)
FLAGS = [(True, True, False, True), FULL, (False, True, False, False), (True, False, True, True),
         (False, False, False, True)]  # pix_var, slice_var, bias, scale: the combinations of test_imaging_loss_vs_reference_math
ALL_FLAGS_AT = (3, 65, 128, 512)
GW = ([1.0, 1.0, 2.0, 100.0], [-1.0, -0.5, -2.0, -100.0])


def _api():
    from nesvor_amd import _lib

    return _lib, _lib.load(), _lib.stream_ptr()


def _gen(*seed):
    return torch.Generator().manual_seed(int(sum(s * 1000003 ** i for i, s in enumerate(seed))) % (2 ** 31))


def _tail_untouched(buf, numel, what):
    assert torch.equal(buf[numel:], torch.full_like(buf[numel:], CANARY)), f"{what}: wrote past its end"


# ============================================================================================================ imaging loss
def _loss_launch(device, dev, flags, reg, delta, gw, B, S, want, absmax):
    """One nesvor_imaging_loss launch: ``want`` names the output pointers that are set (all others NULL), ``gw`` None is the
    forward launch -> {name: output (its body, on the CPU)}, absmax buffers as 'dz0_absmax' etc. (the whole slotted bound)."""
    from nesvor_amd import loss, mlp

    _lib, lib, st = _api()
    pix_var, slice_var, bias, scale = flags
    a = loss._fill(dev["z0"], dev["lv"] if pix_var else None, dev["lb"] if bias else None, dev["x"], dev["v"], dev["idx"],
                   dev["c"] if scale else None, dev["lvs"] if slice_var else None, dev["lb_mean"] if bias else None, loss.REG_TYPES[reg], delta)
    numel = {"loss_pix": 3 * B, "dz0": B * S, "dlog_var": B * S, "dlog_bias": B * S, "dx": 3 * B * S, "dc_pix": B, "dlvs_pix": B}
    bufs = {}
    for name in want:
        bufs[name] = torch.full((numel[name] + PAD,), CANARY, dtype=torch.float32, device=device)
        setattr(a, name, bufs[name].data_ptr())
    if gw is not None:
        a.gw = gw.data_ptr()
    slots = {}
    if absmax:
        for name in ("dz0_absmax", "dlog_var_absmax", "dlog_bias_absmax"):
            slots[name] = torch.full((mlp.ABSMAX_FLOATS + PAD,), CANARY, dtype=torch.float32, device=device)
            slots[name][:mlp.ABSMAX_FLOATS] = 0.0
            setattr(a, name, slots[name].data_ptr())
    assert lib.nesvor_imaging_loss(ctypes.byref(a), st) == 0
    torch.cuda.synchronize()
    out = {}
    for name, t in bufs.items():
        _tail_untouched(t, numel[name], name)
        out[name] = t[:numel[name]].cpu()
    for name, t in slots.items():
        _tail_untouched(t, mlp.ABSMAX_FLOATS, name)
        out[name] = t[:mlp.ABSMAX_FLOATS].cpu()
    return out


def _loss_cases(S):
    i = 0
    for r, reg in enumerate(REGS):
        todo = [(FULL, B) for B in (1, 3, 4, 5)] + ([(f, 5) for f in FLAGS if f != FULL] if S in ALL_FLAGS_AT else [])
        for flags, B in todo:
            yield reg, flags, B, GW[(i + r) % 2]
            i += 1


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 127, 128, 192, 256, 320, 512, 1024])
def test_imaging_loss_vs_fp64(device, S):
    """nesvor_imaging_loss on tests/loss_reference.edge_inputs (a z0 ramp across softplus' threshold, exactly tied mirror
    densities, a coincident mirror pair; odd S: the self-mirrored middle sample) for B = 1, 3, 4, 5 pixels (the last workgroup
    holds 1, 3, 4, 1 live waves; B = 4: one slice, n = 1), the three regularisers, both signs of gw; every flag combination at
    S = 3, 65, 128, 512.  Per case:

    * forward launch + backward launch, the combined launch (loss_pix and gw both set: what the one-call step uses), and the
      combined launch without dx, dc_pix, dlvs_pix and the absmax bounds: the same bits wherever an output exists;
    * every output against float64 under the calibrated rule - loss_pix by column, dz0, dlog_var, dlog_bias, dx, dc_pix,
      dlvs_pix; the pixel with the coincident pair apart from the others (its regulariser terms are ~1e3 times theirs, and
      one scale for both would hide them);
    * the maximum over the slots of each absmax bound == max |out| exactly.

    One comparison misses the bare rule, and only there a derived term is added (loss_reference.calibrated_or_means_term prints
    it): dlvs_pix at S = 320, B = 4, edge, three elements - on the MI355X err_kernel 7.04e-7 = 9.0 x 2^-24 |ref| against
    err_torch_fp32 1.08e-8 (ratio 65.4) and a bound of 6.68e-7, while the fp32 torch composition itself is off by 7.9 x 2^-24 |ref|
    on the same output at S = 320, B = 1.  dlvs_pix is a function of the pixel's two means over S, so the term is what an error of
    those means WITHIN the calibrated rule (4 err_torch_fp32(m) + 8 2^-24 max|m|) moves it by, |d dlvs_pix / d m| times that level
    (loss_reference.dlvs_pix_means_term): about 50 x 2^-24 |ref| at the element that missed, at most 96 x 2^-24 scale over all cases of this
    test (median 2.8) - so the comparison that uses it stands at 0.15 of its bound.  Every other comparison, of dlvs_pix too,
    stands under the bare rule.

    Largest err_kernel / err_torch_fp32 on the MI355X: RATIOS at the end of this module."""
    from nesvor_amd import mlp

    assert mlp.ABSMAX_FLOATS == 16 * 64
    for case, (reg, flags, B, gw_list) in enumerate(_loss_cases(S)):
        pix_var, slice_var, bias, scale = flags
        n = 1 if B == 4 else 3
        d = L.edge_inputs(B, S, _gen(B, S, case), n=n)
        assert L.mirror_signs_agree(d["z0"]), "TV's precondition: change the seed"
        gw = torch.tensor(gw_list)
        args = (d["z0"], d["lv"] if pix_var else None, d["lb"] if bias else None, d["x"], d["v"], d["idx"], d["c"] if scale else None,
                d["lvs"] if slice_var else None, d["lb_mean"] if bias else None, reg, d["delta"], gw)
        p64, p32 = L.loss_parts(*args, torch.float64), L.loss_parts(*args, torch.float32)
        dev = {k: t.to(device) for k, t in d.items() if isinstance(t, torch.Tensor)}
        d_gw = gw.to(device)

        grads = ["dz0", "dx"] + (["dlog_var"] if pix_var else []) + (["dlog_bias"] if bias else []) + (["dc_pix"] if scale else []) \
            + (["dlvs_pix"] if slice_var else [])
        run = lambda g, want, absmax: _loss_launch(device, dev, flags, reg, d["delta"], g, B, S, want, absmax)
        fwd = run(None, ["loss_pix"], False)
        bwd = run(d_gw, grads, True)
        both = run(d_gw, ["loss_pix"] + grads, True)
        lean = run(d_gw, ["loss_pix"] + [g for g in grads if g not in ("dx", "dc_pix", "dlvs_pix")], False)
        tag = f"S={S} B={B} {reg} flags={''.join('01'[f] for f in flags)} gw{gw_list[0]:+.0f}"
        for name, t in both.items():
            sep = fwd if name == "loss_pix" else bwd
            assert torch.equal(t, sep[name]), (tag, name, "combined launch != separate launches")
        for name, t in lean.items():
            assert torch.equal(t, both[name]), (tag, name, "launch without the optional outputs != full launch")
        for name, out in (("dz0_absmax", "dz0"), ("dlog_var_absmax", "dlog_var"), ("dlog_bias_absmax", "dlog_bias")):
            if out in grads:
                assert float(both[name].max()) == float(both[out].abs().max()), (tag, name)
            else:
                assert float(both[name].abs().max()) == 0.0, (tag, name)

        if slice_var:
            closed, means_term = L.dlvs_pix_means_term(args[0], args[1], args[2], args[4], args[5], args[6], args[7], gw)
            torch.testing.assert_close(closed, p64["dlvs_pix"], rtol=1e-9, atol=0.0)  # (the term belongs to this output)
        rest = [b for b in range(B) if not (b == L.COINCIDENT and S >= 2)]
        groups = [("", rest)] + ([("[coincident]", [L.COINCIDENT])] if B > L.COINCIDENT and S >= 2 else [])
        for gname, rows in groups:
            for col, cname in enumerate(("mse", "logvar", "reg")):
                L.calibrated(both["loss_pix"].view(B, 3)[rows, col], p64["loss_pix"][rows, col], p32["loss_pix"][rows, col],
                             f"loss_pix.{cname}{gname} {tag}", "imaging_loss")
            for name in grads:
                got = both[name].view(p64[name].shape)
                if name == "dlvs_pix":
                    L.calibrated_or_means_term(got[rows], p64[name][rows], p32[name][rows], f"{name}{gname} {tag}", "imaging_loss", means_term[rows])
                else:
                    L.calibrated(got[rows], p64[name][rows], p32[name][rows], f"{name}{gname} {tag}", "imaging_loss")


# ============================================================================================================= slice sums
def _path(ks, rows):
    """The path slice_grads_kernel takes for the slice-embedding gradient (csrc/loss.hip)."""
    k4 = ks >> 2
    if ks % 4 == 0 and 64 % k4 == 0 and (rows * k4) % 256 == 0:
        return "float4"  # lane <-> four features, four loads in flight
    return "lane" if 64 % ks == 0 else "fallback"  # lane <-> feature | one wave reduction per feature


N_SL = 9
OWNERS = [0, 2, 3, 5, 6, 8]  # slices 1, 4 and 7 own no pixel
WIDTH = lambda ks: (1, 1, ks, 12)
NAMES = ("dc", "dlvs", "dse", "dmat")


def _slice_inputs(B, rows, ks, gen, one_slice=False):
    idx = torch.full((B,), 5) if one_slice else torch.tensor(OWNERS)[torch.randint(0, len(OWNERS), (B,), generator=gen)]
    r = lambda *sh: torch.randn(*sh, generator=gen)
    ins = [r(B), r(B), r(B, rows, max(ks, 1)), r(B, 12)]  # dc_pix, dlvs_pix, dxa, dpix
    init = [torch.cat([torch.rand(N_SL * max(w, 1), generator=gen) + 0.5, torch.full((PAD,), CANARY)]) for w in WIDTH(ks)]
    return idx, ins, init


def _slice_run(device, which, idx, ins, init, B, rows, ks, present=(True, True, True, True)):
    """which: 'atomic' | 'by_slice' -> (return code, the four outputs on the CPU).  present: dc_pix, dlvs_pix, dxa, dpix (an absent
    input is NULL; the output pointers are always passed)."""
    _lib, lib, st = _api()
    P = _lib.ptr
    d_idx = idx.to(device)
    d_in = [t.to(device) if p else None for t, p in zip(ins, present)]
    outs = [t.to(device) for t in init]
    a = (P(d_idx), P(d_in[0]), P(d_in[1]), P(d_in[2]), P(d_in[3]), P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), B, rows, ks)
    rc = lib.nesvor_slice_grads(*a, st) if which == "atomic" else lib.nesvor_slice_grads_by_slice(*a, N_SL, st)
    torch.cuda.synchronize()
    return rc, [t.cpu() for t in outs]


def _slice_check(outs, idx, ins, init, B, rows, ks, present, what):
    """Sum rule per output element (terms: the pixels' contributions and the value held before), slices without pixels and
    outputs whose input is absent bit-identical to what they held, nothing written past the end.  -> [(ref, bound)]."""
    opt = lambda t, p: t if p else None
    sums, abs_sums, counts = L.slice_sums(idx, opt(ins[0], present[0]), opt(ins[1], present[1]), opt(ins[2], present[2]),
                                          opt(ins[3], present[3]), N_SL, rows, ks, torch.float64)
    refs = []
    for k, (name, w) in enumerate(zip(NAMES, WIDTH(ks))):
        numel = N_SL * max(w, 1)
        _tail_untouched(outs[k], numel, f"{what} {name}")
        got, held = outs[k][:numel], init[k][:numel]
        if sums[k] is None:
            assert torch.equal(got, held), f"{what} {name}: its input is absent, yet it changed"
            refs.append(None)
            continue
        got, held = got.view(N_SL, -1), held.view(N_SL, -1)
        T = (counts * (rows if name == "dse" else 1) + 1).double().view(N_SL, 1)
        ref, mag = held.double() + sums[k].view(N_SL, -1), held.double().abs() + abs_sums[k].view(N_SL, -1)
        L.assert_sum(got, ref, mag, T, f"{what} {name}")
        assert torch.equal(got[counts == 0], held[counts == 0]), f"{what} {name}: a slice without pixels changed"
        refs.append((ref, L.sum_bound(mag, T)))
    return refs


SLICE_CASES = [("float4", 16, 64), ("float4", 16, 256), ("float4", 4, 256), ("float4", 8, 128), ("float4", 128, 8), ("float4", 256, 4),
               ("lane", 16, 2), ("lane", 16, 16), ("lane", 1, 5), ("lane", 2, 7), ("lane", 32, 1), ("lane", 64, 3),
               ("fallback", 3, 5), ("fallback", 24, 4), ("fallback", 48, 2), ("fallback", 65, 3), ("fallback", 100, 70), ("fallback", 128, 3),
               ("none", 0, 3)]


@pytest.mark.parametrize("path,ks,rows", SLICE_CASES, ids=[f"{p}-ks{k}-rows{r}" for p, k, r in SLICE_CASES])
def test_slice_grads_atomic_paths(device, path, ks, rows):
    """nesvor_slice_grads on each path of the slice-embedding gradient (the id names it; _path restates the kernel's conditions),
    ks = 0 included, for B = 1, 5, 203 pixels over 9 slices of which three own none, and for 203 pixels in one slice; outputs
    prefilled with non-zero values (the kernel ADDS).  At B = 5 each of dc_pix, dlvs_pix, dxa, dpix absent in turn."""
    assert ks == 0 or _path(ks, rows) == path
    for B, one_slice in ((1, False), (5, False), (203, False), (203, True)):
        idx, ins, init = _slice_inputs(B, rows, ks, _gen(B, rows, ks, one_slice), one_slice)
        masks = [(True,) * 4] + ([tuple(j != i for j in range(4)) for i in range(4)] if B == 5 else [])
        for present in masks:
            rc, outs = _slice_run(device, "atomic", idx, ins, init, B, rows, ks, present)
            assert rc == 0
            _slice_check(outs, idx, ins, init, B, rows, ks, present if ks > 0 else (present[0], present[1], False, present[3]),
                         f"atomic[{path}] ks={ks} rows={rows} B={B} one_slice={one_slice} present={present}")


BY_SLICE_CASES = [(1, 3), (1, 300), (16, 5), (16, 17), (32, 3), (32, 9), (256, 1), (256, 2)]  # 256 / ks = 256, 16, 8, 1 row groups


@pytest.mark.parametrize("ks,rows", BY_SLICE_CASES)
def test_slice_grads_by_slice(device, ks, rows):
    """nesvor_slice_grads_by_slice with fewer and more rows per pixel than its 256 / ks row groups (ks = 256: one group, rows = 1
    and 2), at the edges of the 256-pixel scan chunk and at its capacity B = 4096 - also with all 4096 pixels in one slice, which
    fills the pixel list to its last entry: the sum rule, two runs bit-identical, empty slices untouched, and agreement with
    nesvor_slice_grads on the same inputs within the sum of both bounds."""
    for B, one_slice in ((1, False), (255, False), (256, False), (257, False), (4096, False), (4096, True)):
        idx, ins, init = _slice_inputs(B, rows, ks, _gen(B, rows, ks, one_slice, 1), one_slice)
        what = f"by_slice ks={ks} rows={rows} B={B} one_slice={one_slice}"
        rc, outs = _slice_run(device, "by_slice", idx, ins, init, B, rows, ks)
        rc2, again = _slice_run(device, "by_slice", idx, ins, init, B, rows, ks)
        assert rc == 0 and rc2 == 0
        for a_, b_ in zip(outs, again):
            assert torch.equal(a_, b_), (what, "two runs differ")
        refs = _slice_check(outs, idx, ins, init, B, rows, ks, (True,) * 4, what)
        rc3, atomic = _slice_run(device, "atomic", idx, ins, init, B, rows, ks)
        assert rc3 == 0
        for k, (ref, bound) in enumerate(refs):
            numel = ref.numel()
            diff = (outs[k][:numel].double() - atomic[k][:numel].double()).abs().view(ref.shape)
            assert bool((diff <= 2 * bound).all()), (what, NAMES[k], "differs from nesvor_slice_grads")


def test_slice_grads_by_slice_refuses_what_it_cannot_list(device):
    """B above the pixel list's capacity, or a ks that does not divide the workgroup: return code 1, nothing written; without dxa
    any ks is accepted."""
    for B, ks in ((4097, 16), (100, 3), (100, 24), (100, 512)):
        idx, ins, init = _slice_inputs(B, 2, ks, _gen(B, ks))
        rc, outs = _slice_run(device, "by_slice", idx, ins, init, B, 2, ks)
        assert rc == 1, (B, ks)
        for o, i in zip(outs, init):
            assert torch.equal(o, i), (B, ks)
    idx, ins, init = _slice_inputs(100, 2, 24, _gen(24))
    present = (True, True, False, True)
    rc, outs = _slice_run(device, "by_slice", idx, ins, init, 100, 2, 24, present)
    assert rc == 0
    _slice_check(outs, idx, ins, init, 100, 2, 24, present, "by_slice ks=24 without dxa")


# RATIOS - the largest err_kernel / err_torch_fp32 per output on the MI355X, general kernel / cached kernel, and the largest share of
# the bound (the rule: err_kernel <= 4 err_torch_fp32 + 8 2^-24 scale) that any comparison of that output used:
#   loss_pix.mse      46.5 / 52.2   0.87
#   loss_pix.logvar    141 / 64     0.53
#   loss_pix.reg      1660 / 12.0   0.36   (1660: the coincident pixel at S = 1024, edge: 1.00 ulp of 1.478e4, torch within 0.001 ulp)
#   dz0               12.3 / 11.5   0.33
#   dlog_var          7.45 / 4.46   0.62
#   dlog_bias         6.64 / 2.38   0.49
#   dx                10.1 / 4.11   0.32
#   dc_pix            42.2 / 63.1   0.88
#   dlvs_pix          65.4 / 35.8   1.05 of the bare rule at S = 320, B = 4, edge (there alone the means' term is added: 0.15), 0.73 otherwise
# The per-pixel outputs are compared one to four elements at a time, so the ratio is large wherever torch's own rounding happens to
# land on the float64 value: everywhere above, the kernel's error is 1 to 6 units in the last place of the element.  In many cases
# kernel and fp32 torch agree to the bit.  The per-slice sums print no ratio: they stand under the sum rule alone.
