"""CPU checks of ops.voxel_conv3d_wgrad and ops.voxel_conv3d_grad_input: the
argument validation that needs no device, and the workspace-size function."""
import pytest
import torch

Z = torch.zeros


@pytest.mark.parametrize("op, args, match", [
    ("wgrad", (Z(1, 4, 5, 5, 5).double(), Z(1, 6, 5, 5, 5)), "grid.*float64"),
    ("wgrad", (Z(1, 4, 5, 5, 5), Z(1, 6, 5, 5)), "grad_out"),
    ("wgrad", (Z(1, 4, 5, 5, 5), Z(1, 5, 5, 5, 6).transpose(1, 4)), "grad_out.*contiguous"),
    ("wgrad", (Z(1, 4, 5, 5, 5), Z(2, 6, 5, 5, 5)), "share B and r"),
    ("wgrad", (Z(1, 4, 2, 2, 2), Z(1, 513, 2, 2, 2)), "513"),
    ("grad_input", (Z(1, 6, 5, 5, 5), Z(6, 4, 3, 3)), "weight"),
    ("grad_input", (Z(1, 6, 5, 5, 5), Z(6, 513, 3, 3, 3)), "Cin = 513"),
    ("grad_input", (Z(1, 5, 5, 5, 5), Z(6, 4, 3, 3, 3)), "gives 6 channels.*has 5"),
])
def test_validation_needs_no_device(op, args, match):
    from o3dml_amd import ops
    with pytest.raises(RuntimeError, match="voxel_conv3d.*" + match):
        getattr(ops, "voxel_conv3d_" + op)(*args)


def test_workspace_size():
    """Slabs x padded blocks; a few tens of MB at the model's largest layer; -1 where a limit is exceeded."""
    from o3dml_amd import _lib
    size = _lib.load().o3dml_voxel_conv3d_wgrad_workspace_size
    block = 27 * 1024
    assert size(2, 9, 16, 1) == block + 32                      # one box pair: one slab
    assert size(8, 64, 64, 32) == 64 * (4 * block + 2 * 32)     # 4 blocks, 64 slabs
    assert size(8, 128, 128, 16) == 16 * (16 * block + 4 * 32) and 4 * size(8, 128, 128, 16) < 32 << 20
    assert size(2, 33, 64, 4) > size(2, 32, 64, 4) == 2 * (2 * block + 2 * 32)  # 4 boxes: two slabs either way
    assert size(0, 8, 8, 4) == block + 32
    assert [size(8, 8, 513, 4), size(8, 0, 8, 4), size(8, 8, 8, 0), size(8, 8, 8, 1291), size(-1, 8, 8, 4)] == [-1] * 5
