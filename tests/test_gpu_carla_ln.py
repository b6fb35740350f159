"""GPU parity of the CaRL agent's LayerNorm + ReLU kernels through the test hooks
ppo_carla_debug_ln_forward / _backward (k_carla_ln, k_carla_ln_big at F = 70 688; k_carla_ln_dgb +
k_carla_ln_dgb_sum + k_carla_ln_bwd: the launches the agent itself uses, include/ppo_carla.h) against fp64
PyTorch relu(layer_norm(z)) and its autograd.

Shapes: F in {256, 512, 1024 inside rows of 1 280 (conv6 / state_linear writing into the encoder row),
70 688 ([8, 94, 94])}, n in {1, 3, 70}; F = 256 also out of a 259-wide row (linear.3 writing into the
[features | value measurements] row: the scalar path). Two cases have a row mean of 50 with unit spread,
where E[z^2] - mean^2 loses every digit of the variance. z, gamma ~ U(0.5, 1.5) and beta are built so that no
pre-ReLU value lies within 1e-3 of zero (the bias of an offending element is moved), so the ReLU mask is the
same in every precision.

Bar, per output (y, {mean, rstd}, dz, dgamma, dbeta), on the largest absolute difference to fp64:
  d(gpu) <= 1.5 * d(fp32 PyTorch on the same case) + 32 * 2^-24 * max |reference|
1.5 x is the project's rule for another summation order; the floor covers outputs PyTorch gets exact to
the last bit. Two calls are bitwise equal (fixed-order sums, no atomics).

Measured on an MI355X, largest distance to fp64 over all cases, GPU / fp32 PyTorch (CPU):
  y 2.3e-6 / 7.1e-6 (both at a row mean of 50; 1.0e-6 / 1.0e-6 at mean 0), {mean, rstd} 1.5e-6 / 4.9e-6,
  dz 9.6e-7 / 2.4e-6, dgamma 7.8e-6 / 1.2e-5, dbeta 4.2e-6 / 3.7e-6 (n = 70 rows);
  the largest d(gpu) / bar is 0.20 (dgamma, F = 256, row mean 50)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

MARGIN = 1e-3
CASES = [(n, F, F, F, 0.0) for F in (256, 512, 70688) for n in (1, 3, 70)]
CASES += [(n, 1024, 1280, 1280, 0.0) for n in (1, 3, 70)]
CASES += [(3, 256, 256, 259, 0.0), (70, 256, 259, 256, 0.0), (3, 256, 256, 256, 50.0), (3, 70688, 70688, 70688, 50.0)]


def _case(n, F, zs, ys, mean, seed):
    rng = np.random.default_rng(seed)
    z = np.full((n, zs), 1e6, np.float32)  # columns beyond F must never be read
    z[:, :F] = (mean + rng.standard_normal((n, F))).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, F).astype(np.float32)
    beta = rng.uniform(-0.1, 0.1, F).astype(np.float32)
    dy = rng.standard_normal((n, F)).astype(np.float32)
    z64 = torch.tensor(z[:, :F], dtype=torch.float64)
    xh = torch.nn.functional.layer_norm(z64, (F,), None, None, 1e-5).numpy()
    for k in range(1, 200):  # keep every pre-ReLU value MARGIN (and a half) away from zero
        bad = (np.abs(xh * gamma.astype(np.float64) + beta.astype(np.float64)) < 1.5 * MARGIN).any(0)
        if not bad.any():
            break
        beta[bad] += np.float32(4 * MARGIN)
    assert (np.abs(xh * gamma.astype(np.float64) + beta.astype(np.float64)) >= MARGIN).all()
    return z, gamma, beta, dy


def _torch(z, gamma, beta, dy, dtype):
    F_ = gamma.size
    zt = torch.tensor(z[:, :F_], dtype=dtype, requires_grad=True)
    g = torch.tensor(gamma, dtype=dtype, requires_grad=True)
    b = torch.tensor(beta, dtype=dtype, requires_grad=True)
    u, mean, rstd = torch.native_layer_norm(zt, (F_,), g, b, 1e-5)
    y = torch.relu(u)
    y.backward(torch.tensor(dy, dtype=dtype))
    stat = torch.stack([mean.reshape(-1), rstd.reshape(-1)], 1)
    return {k: v.detach().double().numpy() for k, v in
            (("y", y), ("stat", stat), ("dz", zt.grad), ("dgamma", g.grad), ("dbeta", b.grad))}


def _gpu(z, gamma, beta, dy, n, F, zs, ys):
    zd, gd, bd = DeviceArray.from_numpy(z), DeviceArray.from_numpy(gamma), DeviceArray.from_numpy(beta)
    y, stat = ppo_amd.carla_ln_forward(zd, gd, bd, n, F, zs, ys)
    dz, dgam, dbet = ppo_amd.carla_ln_backward(zd, gd, stat, y, DeviceArray.from_numpy(dy), n, F, zs, ys)
    return {"y": y.numpy(), "stat": stat.numpy(), "dz": dz.numpy(), "dgamma": dgam.numpy(), "dbeta": dbet.numpy()}


@pytest.mark.parametrize("n,F,zs,ys,mean", CASES)
def test_ln_hooks_vs_fp64_torch(n, F, zs, ys, mean):
    torch.set_num_threads(8)
    ppo_amd.set_device(0)
    z, gamma, beta, dy = _case(n, F, zs, ys, mean, seed=n * 1000 + F + zs + ys)
    r64, r32 = _torch(z, gamma, beta, dy, torch.float64), _torch(z, gamma, beta, dy, torch.float32)
    got = _gpu(z, gamma, beta, dy, n, F, zs, ys)
    again = _gpu(z, gamma, beta, dy, n, F, zs, ys)
    for k in got:
        np.testing.assert_array_equal(got[k], again[k])
    assert (got["y"][:, F:] == 0).all()  # nothing written beyond F in a wider row
    got["y"] = got["y"][:, :F]
    fails = []
    for k in ("y", "stat", "dz", "dgamma", "dbeta"):
        d_gpu = np.abs(got[k].astype(np.float64) - r64[k]).max()
        d_t32 = np.abs(r32[k] - r64[k]).max()
        bar = 1.5 * d_t32 + 32 * 2.0 ** -24 * np.abs(r64[k]).max()
        print(f"\nln n={n} F={F} strides {zs}/{ys} mean {mean}: {k}: d(gpu) {d_gpu:.3e} d(torch fp32) {d_t32:.3e} "
              f"bar {bar:.3e} ratio {d_gpu / bar:.3f}", end="")
        if not d_gpu <= bar:
            fails.append((k, d_gpu, d_t32, bar))
    assert not fails, fails


def test_ln_hook_argument_errors():
    x = DeviceArray.from_numpy(np.zeros((2, 8), np.float32))
    with pytest.raises(ppo_amd.PPOError, match="strides at least F"):
        ppo_amd.carla_ln_forward(x, x, x, 2, 8, in_stride=4)
