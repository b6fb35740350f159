"""Shared by tests/test_reacher_cpu.py and tests/test_gpu_reacher.py: the host driver
(tests/native/reacher_driver.cpp, built with g++ -ffp-contract=off), its output layout, and the
float64 restatement of ReacherPlanar-v0's equations (Reacher-v5's task definition over the textbook
two-link arm; not MuJoCo's Reacher) with libm trigonometry."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "reacher_driver.cpp")
ENV_ID = "ReacherPlanar-v0"
OD, AD, SD, MAX_STEPS = 10, 2, 6, 50
GOAL_R = 0.2
MAX_SPEED = 32.0

# the GPU tests' shapes: E = 37 (neither 4 nor 16 divides it), T = 120 (two autoresets inside one
# launch), then T2 = 30 from the state the first left (an episode spans two launches)
GPU_E, GPU_T, GPU_T2, GPU_SEED = 37, 120, 30, 6


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
    """vec (gamma None) or vecw: (raw bytes, obs0 [E, 10], per-step dict)"""
    act = np.ascontiguousarray(act, np.float32)
    assert act.shape == (T, E, AD)
    act.tofile(tmp_path / f"a_{tag}.f32")
    if gamma is None:
        run_driver(exe, "vec", E, T, seed, clip, tmp_path / f"a_{tag}.f32", tmp_path / f"v_{tag}.out")
    else:
        run_driver(exe, "vecw", E, T, seed, clip, tmp_path / f"a_{tag}.f32", tmp_path / f"v_{tag}.out", gamma)
    raw = (tmp_path / f"v_{tag}.out").read_bytes()
    return (raw,) + parse_vec(raw, E, T)


def host_step(exe, tmp_path, x, tag="s"):
    """One teacher-forced env step of x [n, 8] = (q1, q2, q1dot, q2dot, gx, gy, a0, a1): returns the new
    state [n, 6], the reward [n] and the observation [n, 10], fp32."""
    x = np.ascontiguousarray(x, np.float32)
    x.tofile(tmp_path / f"x_{tag}.f32")
    run_driver(exe, "step", tmp_path / f"x_{tag}.f32", tmp_path / f"o_{tag}.f32")
    o = np.fromfile(tmp_path / f"o_{tag}.f32", np.float32).reshape(-1, SD + 1 + OD)
    assert len(o) == len(x)
    return o[:, :SD], o[:, SD], o[:, SD + 1:]


def gpu_actions(T=GPU_T + GPU_T2, E=GPU_E, seed=GPU_SEED):
    """actions uniform in [-3, 3]^2, beyond the action space"""
    return np.random.default_rng(seed).uniform(-3, 3, (T, E, AD)).astype(np.float32)


def wrap_f64(x):
    """into [-pi, pi)"""
    return (x + np.pi) % (2 * np.pi) - np.pi


def circ_dist(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def obs_f64(s):
    q1, q2, v1, v2, gx, gy = (s[:, i] for i in range(6))
    l1, l2 = 0.1, 0.11
    tx = l1 * np.cos(q1) + l2 * np.cos(q1 + q2)
    ty = l1 * np.sin(q1) + l2 * np.sin(q1 + q2)
    dx, dy = tx - gx, ty - gy
    return np.stack([np.cos(q1), np.cos(q2), np.sin(q1), np.sin(q2), gx, gy, v1, v2, dx, dy], 1)


def step_f64(x):
    """The env step in numpy float64 with libm trigonometry. x [n, 8] = (q1, q2, q1dot, q2dot, gx, gy,
    a0, a1); returns the new state [n, 6], the reward [n] and the observation [n, 10]."""
    x = np.asarray(x).astype(np.float64)
    q1, q2, v1, v2, gx, gy = (x[:, i].copy() for i in range(6))
    a = np.clip(x[:, 6:8], -1.0, 1.0)
    l1, l2, m1, m2 = 0.1, 0.11, 1.0, 1.0
    r1, r2 = l1 / 2, l2 / 2
    I1, I2 = m1 * l1 * l1 / 12, m2 * l2 * l2 / 12
    a1 = I1 + I2 + m1 * r1 * r1 + m2 * (l1 * l1 + r2 * r2)
    a2 = m2 * l1 * r2
    a3 = I2 + m2 * r2 * r2
    G, D, dt = 0.2, 0.02, 0.01
    for _ in range(2):
        c2, s2 = np.cos(q2), np.sin(q2)
        m11 = a1 + 2 * a2 * c2
        m12 = a3 + a2 * c2
        m22 = a3
        h = a2 * s2
        t1 = G * a[:, 0] - D * v1 + h * (2 * v1 * v2 + v2 * v2)
        t2 = G * a[:, 1] - D * v2 - h * v1 * v1
        det = m11 * m22 - m12 * m12
        acc1 = (m22 * t1 - m12 * t2) / det
        acc2 = (m11 * t2 - m12 * t1) / det
        v1 = np.clip(v1 + dt * acc1, -MAX_SPEED, MAX_SPEED)
        v2 = np.clip(v2 + dt * acc2, -MAX_SPEED, MAX_SPEED)
        q1 = wrap_f64(q1 + dt * v1)
        q2 = wrap_f64(q2 + dt * v2)
    s = np.stack([q1, q2, v1, v2, gx, gy], 1)
    obs = obs_f64(s)
    rew = -np.sqrt(obs[:, 8] ** 2 + obs[:, 9] ** 2) - 0.1 * (a[:, 0] ** 2 + a[:, 1] ** 2)
    return s, rew, obs
