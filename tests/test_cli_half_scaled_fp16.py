"""CPU: ``reconstruct --mlp-fp16`` without ``--single-precision`` selects the scaled-fp16 mode of the half-precision model
structure (bias-free networks), and refuses it together with ``--fp16-loss-scaling`` or ``--mlp-bf16``."""
from types import SimpleNamespace

import pytest
import torch


class _Reached(Exception):
    """Raised by the stubbed data loader: argument checking is over and the run would start."""

    def __init__(self, args):
        super().__init__("reached data loading")
        self.cli_args = args


def _reconstruct(monkeypatch, extra):
    from nesvor_amd import cli, image_io

    def stop(path, device):
        raise _Reached(cli_args)

    monkeypatch.setattr(image_io, "load_slices", stop)
    cli_args = cli.build_parser().parse_args(["reconstruct", "--input-slices", "x", "--output-volume", "v.nii.gz"] + extra)
    cli.reconstruct(cli_args)


def test_reconstruct_accepts_mlp_fp16_for_the_half_precision_structure(monkeypatch):
    from nesvor_amd import mlp
    from nesvor_amd.tinycudann import Network

    with pytest.raises(_Reached) as r:
        _reconstruct(monkeypatch, ["--mlp-fp16"])
    args = r.value.cli_args
    assert args.dtype == torch.float16 and args.mlp_fp16 and not args.single_precision and not args.fp16_loss_scaling
    # the mode this selects for a bias-free network: scaled fp16 (4), which NetParams evaluates with NULL biases
    net = Network(32, 16, {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64,
                           "n_hidden_layers": 1})
    assert mlp.inference_operands(SimpleNamespace(density_net=net), args) == mlp.FP16S
    mlp.set_network_operands([net], mlp.FP16S)
    p = mlp.NetParams(net)
    assert p.bias_free and p.biases == [None, None] and p.n_columns() == 64 * 32 + 16 * 64
    # the default half-precision structure keeps its bf16 operands and zero-bias vector
    assert mlp.inference_operands(SimpleNamespace(density_net=net), SimpleNamespace()) is True


@pytest.mark.parametrize("other", ["--fp16-loss-scaling", "--mlp-bf16"])
def test_reconstruct_refuses_mlp_fp16_with_loss_scaling_or_bf16(monkeypatch, other):
    with pytest.raises(SystemExit):
        _reconstruct(monkeypatch, ["--mlp-fp16", other])


def test_single_precision_mlp_fp16_is_unchanged(monkeypatch):
    with pytest.raises(_Reached) as r:
        _reconstruct(monkeypatch, ["--single-precision", "--mlp-fp16"])
    assert r.value.cli_args.dtype == torch.float32 and r.value.cli_args.mlp_fp16
