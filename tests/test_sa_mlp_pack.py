"""CPU checks of ops.sa_mlp_max: the packed weight layout of an odd-width chain
and the argument validation that needs no device."""
import pytest
import torch


def test_pack_layout():
    from o3dml_amd import _lib, ops
    widths = [7, 5, 33]
    weights = [torch.randn(o, i) for i, o in zip(widths[:-1], widths[1:])]
    biases = [torch.randn(o) for o in widths[1:]]
    packed = ops.sa_mlp_pack(weights, biases)
    wd = torch.tensor(widths, dtype=torch.int32)
    assert packed.dtype == torch.float32 and packed.numel() == 8 * 32 + 32 + 8 * 64 + 64
    assert _lib.load().o3dml_sa_mlp_max_packed_size(2, wd.data_ptr()) == packed.numel()
    off = 0
    for (kpad, cpad), w, b in zip(((8, 32), (8, 64)), weights, biases):
        wt, off = packed[off:off + kpad * cpad].view(kpad, cpad), off + kpad * cpad
        bp, off = packed[off:off + cpad], off + cpad
        assert torch.equal(wt[:w.shape[1], :w.shape[0]], w.T) and torch.equal(bp[:len(b)], b)
        # the padding is zeros
        assert wt.count_nonzero() == w.count_nonzero() and bp.count_nonzero() == b.count_nonzero()


@pytest.mark.parametrize("change, match", [
    (dict(weights=[torch.zeros(513, 7)], biases=[torch.zeros(513)]), "limits"),
    (dict(weights=[torch.zeros(4, 7)] * 5, biases=[torch.zeros(4)] * 5), "layers"),
    (dict(weights=[torch.zeros(4, 7), torch.zeros(4, 5)], biases=[torch.zeros(4)] * 2), "chain"),
    (dict(weights=[torch.zeros(4, 7).double()]), "float32"),
    (dict(xyz=torch.zeros(1, 9, 3).double()), "xyz"),
    (dict(idx=torch.zeros(1, 2, 3, dtype=torch.int64)), "int32"),
    (dict(features=torch.zeros(1, 8, 4)), "share"),
    (dict(use_xyz=False), "takes 7"),
    (dict(new_xyz=torch.zeros(1, 3, 3)), "new_xyz"),
])
def test_validation_needs_no_device(change, match):
    from o3dml_amd import ops
    args = dict(xyz=torch.zeros(1, 9, 3), new_xyz=torch.zeros(1, 2, 3), features=torch.zeros(1, 9, 4),
                idx=torch.zeros(1, 2, 3, dtype=torch.int32), weights=[torch.zeros(4, 7)], biases=[torch.zeros(4)])
    args.update(change)
    with pytest.raises(RuntimeError, match=match):
        ops.sa_mlp_max(**args)
