"""Shared by tests/test_cartpole_cpu.py and tests/test_gpu_cartpole.py: the host driver
(tests/native/cartpole_driver.cpp, built with g++ -ffp-contract=off), its output layout, the float64
restatement of Gymnasium's cartpole.py and the inputs of the desynchronisation condition."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "cartpole_driver.cpp")
ENV_ID = "CartPoleContinuous-v1"
OD, AD, MAX_STEPS = 4, 1, 500
X_THRESHOLD = 2.4
THETA_THRESHOLD = 12 * 2 * np.pi / 360

# the desynchronisation condition's inputs (E, seed, T; actions uniform in [-3, 3])
DESYNC_E, DESYNC_SEED, DESYNC_T = 37, 6, 450


def build_driver(path, opt="-O2"):
    subprocess.run(["g++", opt, "-std=c++20", "-ffp-contract=off", "-pthread", SRC, "-o", path], check=True)
    return path


def run_driver(exe, *args):
    subprocess.run([exe] + [str(a) for a in args], check=True)


def parse_vec(raw, E, T):
    out = np.frombuffer(raw, np.float32)
    per = E * OD + 5 * E
    assert out.size == E * OD + T * per
    steps = out[E * OD:].reshape(T, per)
    return out[:E * OD].reshape(E, OD), {
        "obs": steps[:, :E * OD].reshape(T, E, OD), "rew": steps[:, E * OD:E * OD + E],
        "term": steps[:, E * OD + E:E * OD + 2 * E], "trunc": steps[:, E * OD + 2 * E:E * OD + 3 * E],
        "ret": steps[:, E * OD + 3 * E:E * OD + 4 * E], "len": steps[:, E * OD + 4 * E:]}


def host_vec(exe, tmp_path, E, T, seed, tag, act, gamma=None, clip=1):
    """vec (gamma None) or vecw: (raw bytes, obs0 [E, 4], per-step dict)"""
    act = np.ascontiguousarray(act, np.float32)
    act.tofile(tmp_path / f"a_{tag}.f32")
    if gamma is None:
        run_driver(exe, "vec", E, T, seed, clip, tmp_path / f"a_{tag}.f32", tmp_path / f"v_{tag}.out")
    else:
        run_driver(exe, "vecw", E, T, seed, clip, tmp_path / f"a_{tag}.f32", tmp_path / f"v_{tag}.out", gamma)
    raw = (tmp_path / f"v_{tag}.out").read_bytes()
    return (raw,) + parse_vec(raw, E, T)


def desync_actions():
    return np.random.default_rng(DESYNC_SEED).uniform(-3, 3, (DESYNC_T, DESYNC_E, AD)).astype(np.float32)


def assert_desynchronised(done, group=4):
    """The desynchronisation condition on done [T, E] (= term or trunc): episodes end on at least 10
    distinct steps, every env finishes at least 5 episodes, and on some step one env finishes while
    the other envs of its workgroup (`group` consecutive envs: the smallest the rollout kernels use) do not."""
    done = np.asarray(done) != 0
    T, E = done.shape
    steps = np.nonzero(done.any(1))[0]
    assert len(steps) >= 10, len(steps)
    assert (done.sum(0) >= 5).all(), done.sum(0)
    lone = False
    for g0 in range(0, E - group + 1, group):
        blk = done[:, g0:g0 + group]
        lone = lone or bool((blk.sum(1) == 1).any())
    assert lone
    assert not (done.all(1) | ~done.any(1)).all()  # the dones of some step are not all equal


def gym_step_f64(x):
    """cartpole.py's step in float64 (euler, sutton_barto_reward False), the force 10 * clip(a, -1, 1).
    x [n, 5] = (x, xdot, theta, thetadot, a); returns the new state [n, 4] and terminated [n]."""
    x_, xd, th, thd, a = (x[:, i].astype(np.float64) for i in range(5))
    gravity, masscart, masspole, length, force_mag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    total_mass = masspole + masscart
    polemass_length = masspole * length
    force = force_mag * np.clip(a, -1.0, 1.0)
    costheta, sintheta = np.cos(th), np.sin(th)
    temp = (force + polemass_length * np.square(thd) * sintheta) / total_mass
    thetaacc = (gravity * sintheta - costheta * temp) / (length * (4.0 / 3.0 - masspole * np.square(costheta) / total_mass))
    xacc = temp - polemass_length * thetaacc * costheta / total_mass
    nx = x_ + tau * xd
    nxd = xd + tau * xacc
    nth = th + tau * thd
    nthd = thd + tau * thetaacc
    term = (nx < -X_THRESHOLD) | (nx > X_THRESHOLD) | (nth < -THETA_THRESHOLD) | (nth > THETA_THRESHOLD)
    return np.stack([nx, nxd, nth, nthd], 1), term
