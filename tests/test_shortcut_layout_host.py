"""Host: the layout sehip.shortcut_add picks from its operands' strides (sehip.ops._common_layout) -- also where torch calls a tensor
contiguous in both memory formats: 1 x 1 images, and tensors without any element (an empty batch), whose strides alone say in which
format the results are to be allocated."""
import pytest
import torch

CL = torch.channels_last


def layout_of(*tensors):
    from sehip import ops
    return ops._common_layout("test", *tensors)


def test_dense_operands_keep_their_layout():
    from sehip import ops
    s, x = torch.zeros(2, 9, 3, 3), torch.zeros(2, 5, 3, 3)
    assert layout_of(s, x) == (ops.LAYOUT_NCHW, torch.contiguous_format)
    assert layout_of(s.contiguous(memory_format=CL), x.contiguous(memory_format=CL)) == (ops.LAYOUT_NHWC, CL)
    with pytest.raises(ops.SehipError, match="layout"):
        layout_of(s.contiguous(memory_format=CL), x)
    with pytest.raises(ops.SehipError, match="layout"):
        layout_of(s[:, :, :, ::2], x[:, :, :, ::2])


@pytest.mark.parametrize("s_shape, x_shape", [((0, 9, 2, 2), (0, 5, 5, 5)),        # empty batch
                                              ((2, 9, 0, 0), (2, 5, 1, 1)),        # a 1 x 1 image pooled away
                                              ((2, 9, 1, 1), (2, 5, 2, 2))])       # 1 x 1 output
def test_strides_decide_where_both_formats_hold(s_shape, x_shape):
    """An empty or 1 x 1 tensor is contiguous in both formats; what is allocated for the result follows the operands' strides."""
    from sehip import ops
    s, x = torch.empty(s_shape), torch.empty(x_shape)
    code, fmt = layout_of(s, x)
    assert (code, fmt) == (ops.LAYOUT_NCHW, torch.contiguous_format)
    s, x = torch.empty(s_shape, memory_format=CL), torch.empty(x_shape, memory_format=CL)
    code, fmt = layout_of(s, x)
    assert (code, fmt) == (ops.LAYOUT_NHWC, CL)
    assert torch.empty(s_shape, memory_format=fmt).is_contiguous(memory_format=CL)
    assert torch.empty(x_shape, memory_format=fmt).is_contiguous(memory_format=CL)
