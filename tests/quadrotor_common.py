"""Shared by tests/test_quadrotor_cpu.py, tests/test_gpu_quadrotor.py and scripts/quadrotor_learning_ref.py:
the host driver (tests/native/quadrotor_driver.cpp, built with g++ -ffp-contract=off), its output
layout, the float64 restatement of QuadrotorHover-v0's equations (the textbook Newton-Euler quadrotor
in "+" configuration; the project's own task) and a scripted float64 PD controller that hovers it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "quadrotor_driver.cpp")
ENV_ID = "QuadrotorHover-v0"
OD, AD, SD, MAX_STEPS = 18, 4, 13, 500
G, FMAX, ARM, KAPPA, IXX, IZZ, CD, CW, DT, MAX_RATE = 9.81, 9.81 / 2, 0.1, 0.02, 0.01, 0.02, 0.1, 0.002, 0.01, 32.0

# the desynchronised run every GPU comparison starts from (asserted on the host env in
# test_quadrotor_cpu.py::test_desynchronisation): E = 37 (neither 4 nor 16 divides it), 300 steps of
# actions uniform in [-1.5, 1.5]^4
GPU_E, GPU_T, GPU_SEED = 37, 300, 5


def build_driver(path, opt="-O2", extra=()):
    subprocess.run(["g++", opt, "-std=c++20", "-ffp-contract=off", "-pthread", *extra, SRC, "-o", path], check=True)
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
    """vec (gamma None) or vecw: (raw bytes, obs0 [E, 18], per-step dict)"""
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
    """One teacher-forced env step of x [n, 17] = (state[13], a[4]): returns the new state [n, 13], the
    reward [n], the termination flag [n] and the observation [n, 18], fp32."""
    x = np.ascontiguousarray(x, np.float32)
    x.tofile(tmp_path / f"x_{tag}.f32")
    run_driver(exe, "step", tmp_path / f"x_{tag}.f32", tmp_path / f"o_{tag}.f32")
    o = np.fromfile(tmp_path / f"o_{tag}.f32", np.float32).reshape(-1, SD + 2 + OD)
    assert len(o) == len(x)
    return o[:, :SD], o[:, SD], o[:, SD + 1], o[:, SD + 2:]


def gpu_actions(T=GPU_T, E=GPU_E, seed=GPU_SEED):
    """actions uniform in [-1.5, 1.5]^4, beyond the action space"""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (T, E, AD)).astype(np.float32)


def rot_f64(q):
    w, x, y, z = (q[:, i] for i in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)


def obs_f64(s):
    return np.concatenate([s[:, 0:3], rot_f64(s[:, 6:10]), s[:, 3:6], s[:, 10:13]], 1)


def step_f64(x):
    """The env step in numpy float64, written from the task's equations. x [n, 17] = (p, v, q, omega, a);
    returns the new state [n, 13], the reward [n], |p'|^2 [n] and the observation [n, 18]."""
    x = np.asarray(x).astype(np.float64)
    p, v, q, om = x[:, 0:3].copy(), x[:, 3:6].copy(), x[:, 6:10].copy(), x[:, 10:13].copy()
    f = 0.5 * (np.clip(x[:, 13:17], -1.0, 1.0) + 1.0) * FMAX
    F = f.sum(1)
    tau = np.stack([ARM * (f[:, 1] - f[:, 3]), ARM * (f[:, 2] - f[:, 0]), KAPPA * (f[:, 0] - f[:, 1] + f[:, 2] - f[:, 3])], 1)
    Iyy = IXX
    for _ in range(2):
        R = rot_f64(q)
        vdot = F[:, None] * R[:, [2, 5, 8]] - CD * v
        vdot[:, 2] -= G
        od = np.stack([(tau[:, 0] - (IZZ - Iyy) * om[:, 1] * om[:, 2] - CW * om[:, 0]) / IXX,
                       (tau[:, 1] - (IXX - IZZ) * om[:, 2] * om[:, 0] - CW * om[:, 1]) / Iyy,
                       (tau[:, 2] - CW * om[:, 2]) / IZZ], 1)
        om = np.clip(om + DT * od, -MAX_RATE, MAX_RATE)
        v = v + DT * vdot
        p = p + DT * v
        w, a, b, c = (q[:, i] for i in range(4))
        ox, oy, oz = (om[:, i] for i in range(3))
        dq = np.stack([-(a * ox + b * oy + c * oz), w * ox + b * oz - c * oy, w * oy + c * ox - a * oz,
                       w * oz + a * oy - b * ox], 1)
        q = q + 0.5 * DT * dq
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
    s = np.concatenate([p, v, q, om], 1)
    obs = obs_f64(s)
    p2 = (p * p).sum(1)
    rp = 1.0 / (1.0 + p2)
    rew = rp + rp * (1.0 / (1.0 + (1.0 - obs[:, 11]) ** 2) + 1.0 / (1.0 + (om * om).sum(1)))
    return s, rew, p2, obs


def pd_controller(obs):
    """A hand-written float64 PD hover controller from the observation [E, 18]: a position loop gives the
    wanted acceleration, whose direction is the wanted body z axis; a rate loop turns the body onto it.
    Returns actions [E, 4] inside the action limits."""
    o = np.asarray(obs, np.float64)
    p, R, v, om = o[:, 0:3], o[:, 3:12].reshape(-1, 3, 3), o[:, 12:15], o[:, 15:18]
    acc = np.clip(-2.0 * p - 2.5 * v, -3.0, 3.0)
    acc[:, 2] += G
    zb = R[:, :, 2]
    F = np.clip((acc * zb).sum(1), 0.2 * G, 1.8 * G)
    zd = acc / np.linalg.norm(acc, axis=1, keepdims=True)
    b = np.einsum("eji,ej->ei", R, zd)  # the wanted z axis in the body frame
    wd = 8.0 * np.stack([-b[:, 1], b[:, 0], np.zeros(len(o))], 1)
    tau = np.array([IXX, IXX, IZZ]) * 20.0 * (wd - om)
    f = np.stack([F / 4 - tau[:, 1] / (2 * ARM) + tau[:, 2] / (4 * KAPPA), F / 4 + tau[:, 0] / (2 * ARM) - tau[:, 2] / (4 * KAPPA),
                  F / 4 + tau[:, 1] / (2 * ARM) + tau[:, 2] / (4 * KAPPA), F / 4 - tau[:, 0] / (2 * ARM) - tau[:, 2] / (4 * KAPPA)], 1)
    return np.clip(2.0 * f / FMAX - 1.0, -1.0, 1.0).astype(np.float32)


class HostQuad:
    """SeqVectorEnv over RecordEpisodeStatistics(gymcpp::QuadrotorHover), clip_actions on: the driver
    built as a shared object, for closed loops (the PD controller, the learning reference)."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            d = tempfile.mkdtemp(prefix="quaddrv")
            so = os.path.join(d, "libquaddrv.so")
            subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", SRC, "-o", so],
                           check=True)
            cls._lib = C.CDLL(so)
            cls._lib.quaddrv_create.restype = C.c_void_p
            cls._lib.quaddrv_create.argtypes = [C.c_int, C.c_int]
            cls._lib.quaddrv_destroy.argtypes = [C.c_void_p]
            cls._lib.quaddrv_reset.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            cls._lib.quaddrv_step.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        return cls._lib

    def __init__(self, E):
        self.E = E
        self.h = self.lib().quaddrv_create(E, 1)
        self.obs = np.zeros((E, OD), np.float32)
        self.rew, self.term, self.done, self.ret, self.len = (np.zeros(E, np.float32) for _ in range(5))

    def reset(self, seed):
        self.lib().quaddrv_reset(self.h, seed, self.obs.ctypes.data)
        return self.obs.copy()

    def step(self, act):
        act = np.ascontiguousarray(act, np.float32)
        assert act.shape == (self.E, AD)
        self.lib().quaddrv_step(self.h, act.ctypes.data, self.obs.ctypes.data, self.rew.ctypes.data, self.term.ctypes.data,
                                self.done.ctypes.data, self.ret.ctypes.data, self.len.ctypes.data)
        # (obs, reward, term, done, return, length): the termination flags after the rewards
        return self.obs.copy(), self.rew.copy(), self.term.copy(), self.done.copy(), self.ret.copy(), self.len.copy()

    def close(self):
        if self.h:
            self.lib().quaddrv_destroy(self.h)
            self.h = None


def pd_prefix_actions(E, seed, T):
    """The PD controller's actions [T, E, 4] over the host env reset with seed (closed loop on the host),
    and the per-step (obs, rew, term, done, ret, len) lists."""
    env = HostQuad(E)
    obs = env.reset(seed)
    acts, steps = [], []
    for _ in range(T):
        a = pd_controller(obs)
        r = env.step(a)
        obs = r[0]
        acts.append(a)
        steps.append(r)
    env.close()
    return np.stack(acts), steps
