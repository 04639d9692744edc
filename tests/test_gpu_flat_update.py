"""GPU: the 16-byte decision that se_adagrad_step, se_sgd_step and se_grad_clip_factor share (csrc/flat_update.h) with exactly ONE
buffer of a call misaligned -- the other GPU tests offset all buffers together.  Each buffer in turn lies 4 bytes past a 256-byte
boundary while the others are aligned, and one call is bit-equal to the oracle of the host tests."""
import numpy as np
import pytest

from _flat_buffers import _bits, _dev
from test_adagrad_host import adagrad_inputs, adagrad_oracle
from test_sgd_host import F, clip_oracle, exact_sum_inputs, sgd_inputs, sgd_oracle

pytestmark = pytest.mark.gpu

LR, MOM = 0.01, 0.9


def _one_odd(hosts, odd):
    """``hosts`` on the device, the one at index ``odd`` one element past a 256-byte boundary and every other on one."""
    devs = [_dev(h, int(k == odd)) for k, h in enumerate(hosts)]
    assert [d.data_ptr() % 16 for d in devs] == [4 * (k == odd) for k in range(len(hosts))]
    return devs


@pytest.mark.parametrize("n", [4, 69])      # one 16-byte unit; 17 units and a tail of 1 -- had the 16-byte path been taken
def test_one_misaligned_buffer_of_a_call(n):
    import sehip
    ph, ah, gh, l2h = adagrad_inputs(n, 400 + n)
    wp, wa = adagrad_oracle(ph, ah, gh, l2h, LR, 0.5)
    for odd in range(4):                    # p, accum, g, l2
        p, a, g, l2 = _one_odd((ph, ah, gh, l2h), odd)
        sehip.adagrad_step_(p, a, g, l2, lr=LR, grad_scale=0.5)
        assert np.array_equal(_bits(p), _bits(wp)) and np.array_equal(_bits(a), _bits(wa)), ("adagrad", n, odd)
        assert np.array_equal(_bits(g), _bits(gh)) and np.array_equal(_bits(l2), _bits(l2h)), ("adagrad", n, odd)

    ph, vh, gh, l2h = sgd_inputs(n, 500 + n)
    wp, wv = sgd_oracle(ph, vh, gh, l2h, LR, 0.5, None, MOM, True)
    for odd in range(4):                    # p, v, g, l2
        p, v, g, l2 = _one_odd((ph, vh, gh, l2h), odd)
        sehip.sgd_step_(p, v, g, l2, lr=LR, grad_scale=0.5, momentum=MOM, nesterov=True)
        assert np.array_equal(_bits(p), _bits(wp)) and np.array_equal(_bits(v), _bits(wv)), ("sgd", n, odd)
        assert np.array_equal(_bits(g), _bits(gh)) and np.array_equal(_bits(l2), _bits(l2h)), ("sgd", n, odd)

    # squares that sum exactly in float64 in any order (test_sgd_host.exact_sum_inputs): the oracle's bits whatever the order
    gh, ph, l2h = exact_sum_inputs(n, 600 + n)
    want = np.array(clip_oracle(gh, ph, l2h, 1.0, 1.0), dtype=F)
    for odd in range(3):                    # g, p, l2
        g, p, l2 = _one_odd((gh, ph, l2h), odd)
        stats = sehip.grad_clip_factor(g, p, l2, clipnorm=1.0)
        assert np.array_equal(_bits(stats), _bits(want)), ("clip", n, odd)
        assert np.array_equal(_bits(g), _bits(gh)) and np.array_equal(_bits(p), _bits(ph)), ("clip", n, odd)
