"""What the GPU tests of the flat-buffer optimizer kernels share (test_gpu_adagrad.py, test_gpu_sgd.py, test_gpu_flat_update.py): bit
patterns, device buffers at a chosen alignment, and the sizes that reach every path of the streaming loop."""
import numpy as np
import torch


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


def _dev(a, offset):
    """``a`` on the device, 256-byte aligned (offset 0) or ``offset`` elements past such an address."""
    buf = torch.zeros(len(a) + offset, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[offset:]
    view.copy_(torch.from_numpy(a))
    return view


def _big_n(cap):
    """For the grid cap ``cap``: one more trip of the grid-stride loop than the capped grid covers, and a tail."""
    return cap * 256 * 4 + 5


SIZES = [1, 3, 4, 5, 63, 64, 65, 1023, 4103, "big"]
