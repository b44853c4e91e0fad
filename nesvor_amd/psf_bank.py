"""Per-slice PSFs for the classical pipeline: a PSF BANK, the host side of ``nesvor_slice_acq_forward_bank`` /
``nesvor_slice_acq_adjoint_forward_bank`` / ``nesvor_svr_similarity_bank`` (include/nesvor_hip.h).

Stacks of unequal slice thickness need one slice profile each.  A bank holds the distinct PSFs ("members") once and one id per
slice; the kernels look a slice's PSF up per workgroup (A, the similarity sums) or per step of the voxel gather's slice loop
(A^T), so A and A^T stay one launch each whatever the number of members.  Host logic only: nothing here launches."""
from typing import List, Sequence, Union

import torch

from .utils import get_PSF

SAME_THICKNESS = 1e-3  # mm: thicknesses closer than this share a member
MAX_MEMBERS = 32  # kMaxBankMembers of csrc/acq_taps.h: the table travels as a kernel argument


class PsfBank:
    """``psfs``: the members, fp32 (d_p,h_p,w_p) each, on one device; ``ids``: one member index per slice (any integer sequence
    or tensor; validated here, on the host, before anything is uploaded).

    ``flat``: the members concatenated (device, fp32); ``table``: (P,4) int32 on the HOST, row p = {offset in floats, d_p, h_p,
    w_p}; ``ids``: (n) int32 on the device; ``host_ids``: the same as a list."""

    def __init__(self, psfs: Sequence[torch.Tensor], ids) -> None:
        psfs = [p.contiguous() for p in psfs]
        if not 1 <= len(psfs) <= MAX_MEMBERS:
            raise ValueError(f"PsfBank: 1 .. {MAX_MEMBERS} members expected, got {len(psfs)}")
        if any(p.ndim != 3 or p.numel() == 0 or p.dtype != torch.float32 for p in psfs):
            raise ValueError("PsfBank: every member must be a non-empty float32 (d, h, w) array")
        if any(p.device != psfs[0].device for p in psfs):
            raise ValueError("PsfBank: the members must be on one device")
        host_ids = [int(i) for i in (ids.tolist() if torch.is_tensor(ids) else ids)]
        bad = [i for i in host_ids if not 0 <= i < len(psfs)]
        if bad:
            raise ValueError(f"PsfBank: slice ids must lie in [0, {len(psfs)}), got {bad[0]}")
        self.psfs: List[torch.Tensor] = psfs
        self.host_ids: List[int] = host_ids
        self.flat = torch.cat([p.flatten() for p in psfs])
        offsets, at = [], 0
        for p in psfs:
            offsets.append(at)
            at += p.numel()
        self.table = torch.tensor([[o, *p.shape] for o, p in zip(offsets, psfs)], dtype=torch.int32)
        self.ids = torch.tensor(host_ids, dtype=torch.int32).to(self.flat.device)

    @property
    def device(self):
        return self.flat.device

    @property
    def n_members(self) -> int:
        return len(self.psfs)

    def __len__(self) -> int:
        return len(self.host_ids)

    def max_elements(self) -> int:
        return max(p.numel() for p in self.psfs)

    def members(self):
        """(member index, its PSF, the indices of its slices as a device int64 tensor), for the members that have slices."""
        for g, p in enumerate(self.psfs):
            idx = [k for k, i in enumerate(self.host_ids) if i == g]
            if idx:
                yield g, p, torch.tensor(idx, dtype=torch.int64, device=self.device)

    def op_args(self, idx=None):
        """``(psf_bank, psf_table, psf_id)`` as the ``_bank`` ops take them, for all slices or for ``slices[idx]`` (an index tensor
        or sequence): the subset's ids, int32 and contiguous on the bank's device.  The members stay as they are - one without a
        slice in the subset does no harm (``subset`` drops them, at the price of a new bank)."""
        if idx is None:
            return self.flat, self.table, self.ids
        return self.flat, self.table, self.ids[torch.as_tensor(idx, dtype=torch.int64, device=self.device)].contiguous()

    def subset(self, idx) -> "PsfBank":
        """The bank of ``slices[idx]``: ids remapped, members no slice uses dropped (order of first appearance kept)."""
        idx = [int(i) for i in (idx.tolist() if torch.is_tensor(idx) else idx)]
        remap, psfs, ids = {}, [], []
        for k in idx:
            g = self.host_ids[k]
            if g not in remap:
                remap[g] = len(psfs)
                psfs.append(self.psfs[g])
            ids.append(remap[g])
        if not psfs:  # (no slice: keep a member, so that the bank stays valid)
            psfs = self.psfs[:1]
        return PsfBank(psfs, ids)


def as_thickness_list(s_thick, n: int):
    """``s_thick`` as the pipeline takes it: a float (None is returned: today's one-PSF path) or one value per slice (a list)."""
    if torch.is_tensor(s_thick):
        s_thick = s_thick.tolist()
    if isinstance(s_thick, (int, float)):
        return None
    t = [float(v) for v in s_thick]
    if len(t) != n:
        raise ValueError(f"one thickness per slice expected: {n} slices, {len(t)} thicknesses")
    return t


def group_thicknesses(thicknesses: Sequence[float]):
    """-> (the distinct thicknesses in order of first appearance, one id per entry); values within SAME_THICKNESS of a
    member's (first) thickness share it."""
    members: List[float] = []
    ids = []
    for t in thicknesses:
        for g, m in enumerate(members):
            if abs(float(t) - m) <= SAME_THICKNESS:
                ids.append(g)
                break
        else:
            ids.append(len(members))
            members.append(float(t))
    return members, ids


def bank_for(thicknesses_per_slice: Sequence[float], res_s: float, res_r: float, device, scale: float = 1.0) -> Union[PsfBank, torch.Tensor]:
    """The PSFs of slices of ``res_s`` pixels and their own thicknesses on a ``res_r * scale`` grid (``scale``: a pyramid
    level's factor): member g is ``get_PSF((res_s / res_r, res_s / res_r, t_g / (res_r * scale)))`` as the one-PSF path builds
    it.  One member only: that PSF as a plain tensor - no bank is built and the one-PSF entry points run."""
    members, ids = group_thicknesses(thicknesses_per_slice)
    if not members:
        raise ValueError("bank_for: no slice")
    psfs = [get_PSF(res_ratio=(res_s / res_r, res_s / res_r, t / (res_r * scale)), device=device) for t in members]
    return psfs[0] if len(psfs) == 1 else PsfBank(psfs, ids)
