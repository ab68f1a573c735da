"""CPU checks of ops.voxel_conv3d: the argument validation that needs no
device, and the packed weight layout."""
import pytest
import torch


@pytest.mark.parametrize("change, match", [
    (dict(grid=torch.zeros(1, 4, 5, 5, 5).double()), "grid.*float64"),
    (dict(grid=torch.zeros(1, 4, 5, 5)), "grid"),
    (dict(grid=torch.zeros(1, 4, 5, 5, 6)), r"grid.*\[1, 4, 5, 5, 6\]"),
    (dict(grid=torch.zeros(1, 5, 5, 5, 4).transpose(1, 4)), "contiguous"),
    (dict(grid=torch.zeros(1, 3, 5, 5, 5)), "takes 4 channels.*has 3"),
    (dict(weight=torch.zeros(6, 4, 3, 3, 3).double()), "weight.*float64"),
    (dict(weight=torch.zeros(6, 4, 3, 3)), "weight"),
    (dict(weight=torch.zeros(6, 4, 5, 5, 5)), r"weight.*\[6, 4, 5, 5, 5\]"),
    (dict(bias=torch.zeros(7)), r"bias.*\[7\]"),
    (dict(bias=torch.zeros(6).double()), "bias.*float64"),
    (dict(weight=torch.zeros(513, 4, 3, 3, 3), bias=None), "513"),
    (dict(packed=torch.zeros(27 * 8 * 32 + 32).double()), "packed.*float64"),
    (dict(packed=torch.zeros(27 * 8 * 32)), r"packed.*\[6944\]"),
    (dict(out=torch.zeros(1, 6, 5, 5, 5)), "out.*cpu"),
])
def test_validation_needs_no_device(change, match):
    from o3dml_amd import ops
    args = dict(grid=torch.zeros(1, 4, 5, 5, 5), weight=torch.zeros(6, 4, 3, 3, 3), bias=torch.zeros(6))
    args.update(change)
    with pytest.raises(RuntimeError, match="voxel_conv3d.*" + match):
        ops.voxel_conv3d(**args)


def test_pack_layout():
    """[27, kpad, cpad] tap-major, then the bias [cpad]; zeros in the padding."""
    from o3dml_amd import ops
    g = torch.Generator().manual_seed(0)
    w, b = torch.randn(33, 9, 3, 3, 3, generator=g), torch.randn(33, generator=g)
    packed = ops.voxel_conv3d_pack(w, b)
    kpad, cpad = 16, 64
    assert packed.dtype == torch.float32 and packed.numel() == 27 * kpad * cpad + cpad
    body, tail = packed[:27 * kpad * cpad].view(3, 3, 3, kpad, cpad), packed[27 * kpad * cpad:]
    assert torch.equal(body[..., :9, :33].permute(4, 3, 0, 1, 2), w)
    assert torch.equal(tail[:33], b)
    assert body.abs().sum() == w.abs().sum() and tail[33:].abs().sum() == 0
    assert torch.equal(ops.voxel_conv3d_pack(w)[27 * kpad * cpad:], torch.zeros(cpad))
