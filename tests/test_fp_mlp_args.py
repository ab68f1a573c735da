"""CPU checks of ops.fp_mlp: the argument validation that needs no device."""
import pytest
import torch


@pytest.mark.parametrize("change, match", [
    (dict(known_feats=torch.zeros(1, 6, 4).double()), "known_feats"),
    (dict(dist2=torch.zeros(1, 9, 3).double()), "dist2"),
    (dict(idx=torch.zeros(1, 9, 3, dtype=torch.int64)), "int32"),
    (dict(unknown_feats=torch.zeros(9, 3)), "unknown_feats"),
    (dict(known_feats=torch.zeros(1, 4, 6).transpose(1, 2)), "contiguous"),
    (dict(known_feats=torch.zeros(2, 6, 4)), "share"),
    (dict(unknown_feats=torch.zeros(1, 8, 3)), "share"),
    (dict(unknown_feats=None), "takes 7"),
    (dict(weights=[torch.zeros(7, 7)] * 5, biases=[torch.zeros(7)] * 5), "layers"),
    (dict(weights=[torch.zeros(4, 7).double()]), "float32"),
])
def test_validation_needs_no_device(change, match):
    from o3dml_amd import ops
    args = dict(unknown_feats=torch.zeros(1, 9, 3), known_feats=torch.zeros(1, 6, 4), dist2=torch.zeros(1, 9, 3),
                idx=torch.zeros(1, 9, 3, dtype=torch.int32), weights=[torch.zeros(4, 7)], biases=[torch.zeros(4)])
    args.update(change)
    with pytest.raises(RuntimeError, match="fp_mlp.*" + match):
        ops.fp_mlp(**args)
