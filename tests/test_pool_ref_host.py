"""tests/pool_ref.py against F.max_pool2d(3, 2, 1) and its backward on the CPU in f32, bit for bit (no GPU)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pool_ref as R

EXTENTS = [(1, 1), (1, 4), (2, 3), (3, 2), (4, 5), (5, 7), (7, 8), (8, 9), (9, 10), (10, 17), (17, 1)]


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _torch(x, dy):
    xx = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(xx, 3, 2, 1)
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1).numpy(), xx.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("ih,iw", EXTENTS)
def test_matches_torch(ih, iw):
    for C in (4, 24):
        x = R.edge_input(2, ih, iw, C, seed=ih * 31 + iw)
        rng = np.random.default_rng(1)
        dy = rng.standard_normal((2, R.out_size(ih), R.out_size(iw), C)).astype(np.float32)
        y, dx = _torch(x, dy)
        got, idx = R.forward(x)
        assert _same(got, y), (ih, iw, C)
        assert _same(R.backward(x, dy), dx), (ih, iw, C)
        # accumulating adds the existing values after the windows' sum
        old = rng.standard_normal(x.shape).astype(np.float32)
        assert _same(R.backward(x, dy, old), dx + old)


def test_the_edge_input_holds_its_edges():
    x = R.edge_input(2, 9, 10, 24, seed=5)
    y, idx = R.forward(x)
    assert np.isnan(x).sum() == 2 and np.isinf(y[y > 0]).sum() >= 1
    assert (y[:, 0, 0, 3] == -np.inf).all() and (idx[:, 0, 0, 3] == 0).all()          # the corner window
    assert (y[:, 1, 1, 22] == -np.inf).all() and (idx[:, 1, 1, 22] == 1 * 10 + 1).all()  # the interior one
    assert (y[1, :, :, 21] == -np.inf).all()
    assert np.isnan(y[1, 0, 0, 23])  # the NaN holds against the 100 after it
    z = y[..., 0].view(np.uint32)
    assert set(np.unique(z).tolist()) == {0, 0x80000000}  # ties of +0 and -0: the first tap's sign survives


def test_all_minus_inf_window_gradient_goes_to_the_first_in_bounds_tap():
    x = np.full((1, 4, 4, 1), -np.inf, np.float32)
    dy = np.arange(1, 5, dtype=np.float32).reshape(1, 2, 2, 1)
    want = np.zeros((4, 4), np.float32)
    want[0, 0], want[0, 1], want[1, 0], want[1, 1] = 1, 2, 3, 4  # first in-bounds taps of the four windows
    assert np.array_equal(R.backward(x, dy)[0, :, :, 0], want)
    assert _same(R.backward(x, dy), _torch(x, dy)[1])
