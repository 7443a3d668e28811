"""The algebra behind the backward call's pose gradients when d(coords) itself is not asked for (elementwise.h,
first_layer_image_block role 0): dtheta[b] and ddx[b] follow from the per-image sums the first-layer parameter gradients need
anyway,

    G0[k] = sum_i dh0[i,k] x0''[i],   G1[k] = sum_i dh0[i,k] x1''[i],   S[k] = sum_i dh0[i,k],

with x0'' = c g0 - s g1 + dx0, x1'' = s g0 + c g1 + dx1 and (w0, w1)[k] the coordinate weights of feature k:

    ddx[b]    = ( sum_k w0[k] S[k],  sum_k w1[k] S[k] )
    dtheta[b] =   sum_k ( w1[k] (G0[k] - dx0 S[k])  -  w0[k] (G1[k] - dx1 S[k]) )

checked here in float64 against the row-wise definition (d(coords)[i] = sum_k dh0[i,k] (w0, w1)[k], then the chain rule through
the rotation and the shift, as pose_bwd_kernel and role 1 do it).  No GPU."""
import numpy as np
import pytest


def _rowwise(dh, w, grid, theta, dx):
    c, s = np.cos(theta), np.sin(theta)
    dc = dh @ w                                             # [N, 2]
    dtheta = (dc[:, 0] * (-s * grid[:, 0] - c * grid[:, 1]) + dc[:, 1] * (c * grid[:, 0] - s * grid[:, 1])).sum()
    return dtheta, dc.sum(0)


def _from_sums(dh, w, grid, theta, dx):
    c, s = np.cos(theta), np.sin(theta)
    x0 = c * grid[:, 0] - s * grid[:, 1] + dx[0]
    x1 = s * grid[:, 0] + c * grid[:, 1] + dx[1]
    G0, G1, S = dh.T @ x0, dh.T @ x1, dh.sum(0)
    ddx = np.array([(w[:, 0] * S).sum(), (w[:, 1] * S).sum()])
    dtheta = (w[:, 1] * (G0 - dx[0] * S) - w[:, 0] * (G1 - dx[1] * S)).sum()
    return dtheta, ddx


@pytest.mark.parametrize("N,H,seed", [(784, 500, 0), (50, 33, 1), (1, 1, 2)])
@pytest.mark.parametrize("pose", ["rotate+translate", "rotate", "translate"])
def test_pose_gradients_from_the_per_image_sums(N, H, seed, pose):
    rs = np.random.RandomState(seed)
    dh = rs.normal(size=(N, H))
    w = rs.uniform(-1, 1, size=(H, 2))
    grid = rs.uniform(-1, 1, size=(N, 2))
    theta = rs.uniform(-3, 3) if "rotate" in pose else 0.0
    dx = 0.3 * rs.normal(size=2) if "translate" in pose else np.zeros(2)
    t_row, d_row = _rowwise(dh, w, grid, theta, dx)
    t_sum, d_sum = _from_sums(dh, w, grid, theta, dx)
    # either form is a sum of the N H terms dh0[i,k] w[k,p] f[i] with |f| <= |g| + |dx| < 4, nested in chains of at most
    # N + H + 8 additions: the classical bound of a float64 sum of that depth, for the two forms together
    tol = 2 * (N + H + 8) * 2.0 ** -52 * np.abs(dh).sum() * np.abs(w).max() * 4.0
    assert abs(t_row - t_sum) <= tol
    assert np.abs(d_row - d_sum).max() <= tol


def test_pad_rows_drop_out():
    """Pad rows carry dh0 = 0 and x'' = 0 in the kernels: appending them changes none of the sums."""
    rs = np.random.RandomState(3)
    dh, w, grid = rs.normal(size=(20, 7)), rs.normal(size=(7, 2)), rs.uniform(-1, 1, size=(20, 2))
    dx = np.array([0.2, -0.1])
    a = _from_sums(dh, w, grid, 0.7, dx)
    b = _from_sums(np.vstack([dh, np.zeros((12, 7))]), w, np.vstack([grid, rs.normal(size=(12, 2))]), 0.7, dx)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
