"""What tests/test_denoise.py and tests/test_gpu_denoise.py share: the phantom stack of the quality test and the masked PSNR."""
import math

import torch
import torch.nn.functional as F

_CLEAN = {}


def phantom_stack(sigma: float, seed: int = 0):
    """(clean, noisy, mask), each (12,1,47,47) fp32 on the host: planes 12, 14 .. 34 of ``phantom3d(n=48)``, each blurred in-plane
    by the separable 3-tap window [1/4, 1/2, 1/4] (zero padding), the mask clean > 0.01, Gaussian noise of ``sigma`` added
    everywhere.  The clean planes are built once and never written."""
    if not _CLEAN:
        from nesvor_amd.phantom import phantom3d

        vol = torch.tensor(phantom3d(n=48), dtype=torch.float64)
        planes = vol[12:35:2].unsqueeze(1)
        k = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64)
        planes = F.conv2d(F.conv2d(planes, k.view(1, 1, 1, 3), padding=(0, 1)), k.view(1, 1, 3, 1), padding=(1, 0))
        _CLEAN["clean"] = planes.float().contiguous()
        _CLEAN["mask"] = _CLEAN["clean"] > 0.01
    clean, mask = _CLEAN["clean"], _CLEAN["mask"]
    g = torch.Generator().manual_seed(seed)
    noisy = clean + sigma * torch.randn(clean.shape, generator=g)
    return clean, noisy.contiguous(), mask


def masked_psnr(x: torch.Tensor, clean: torch.Tensor, mask: torch.Tensor) -> float:
    """10 log10(1 / mean over the mask of (x - clean)^2): the peak is 1, the phantom's range."""
    mse = float(((x.double().cpu() - clean.double()) ** 2)[mask].mean())
    return -10.0 * math.log10(mse)
