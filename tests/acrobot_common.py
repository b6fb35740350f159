"""Shared by tests/test_acrobot_cpu.py and tests/test_gpu_acrobot.py: the host driver
(tests/native/acrobot_driver.cpp, built with g++ -ffp-contract=off), its output layout, the float64
restatement of AcrobotContinuous-v1's step with libm trigonometry and the inputs of the
desynchronisation condition."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "acrobot_driver.cpp")
ENV_ID = "AcrobotContinuous-v1"
OD, AD, SD, MAX_STEPS = 6, 1, 4, 500
MAX_VEL_1, MAX_VEL_2 = 4 * np.pi, 9 * np.pi
DT = 0.2

# the desynchronisation condition's inputs: E envs, T steps, reset seed, the seed of the noise of the
# driver's energy-pumping actions (acrobot_driver.cpp, mode pump). The first seed pair tried was kept.
DESYNC_E, DESYNC_T, DESYNC_SEED, DESYNC_NOISE_SEED = 37, 640, 6, 1


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
    """vec (gamma None) or vecw: (raw bytes, obs0 [E, 6], per-step dict)"""
    act = np.ascontiguousarray(act, np.float32)
    act.tofile(tmp_path / f"a_{tag}.f32")
    if gamma is None:
        run_driver(exe, "vec", E, T, seed, clip, tmp_path / f"a_{tag}.f32", tmp_path / f"v_{tag}.out")
    else:
        run_driver(exe, "vecw", E, T, seed, clip, tmp_path / f"a_{tag}.f32", tmp_path / f"v_{tag}.out", gamma)
    raw = (tmp_path / f"v_{tag}.out").read_bytes()
    return (raw,) + parse_vec(raw, E, T)


def host_pump(exe, tmp_path, E, T, seed, noise_seed, tag="p"):
    """The driver's energy-pumping run: (actions [T, E, 1] as recorded, obs0, per-step dict). The
    recorded actions replayed through vec give the same bytes (test_acrobot_cpu.py checks that)."""
    run_driver(exe, "pump", E, T, seed, noise_seed, tmp_path / f"v_{tag}.out", tmp_path / f"a_{tag}.f32")
    act = np.fromfile(tmp_path / f"a_{tag}.f32", np.float32).reshape(T, E, AD)
    return (act,) + parse_vec((tmp_path / f"v_{tag}.out").read_bytes(), E, T)


def desync_run(exe, tmp_path):
    return host_pump(exe, tmp_path, DESYNC_E, DESYNC_T, DESYNC_SEED, DESYNC_NOISE_SEED, "desync")


def desync_counts(term, trunc):
    """What the desynchronisation condition counts on term / trunc [T, E]."""
    term, trunc = np.asarray(term) != 0, np.asarray(trunc) != 0
    done = term | trunc

    def lone(group):
        E = done.shape[1]
        return int(sum((done[:, g0:g0 + group].sum(1) == 1).sum() for g0 in range(0, E - group + 1, group)))

    return {"terminations": int(term.sum()), "termination_steps": int(term.any(1).sum()), "truncations": int(trunc.sum()),
            "envs_that_terminate": int(term.any(0).sum()), "lone_in_4": lone(4), "lone_in_16": lone(16)}


def assert_desynchronised(term, trunc):
    """Episodes end by termination on at least 40 distinct steps and in at least 24 envs, on some step
    one env finishes alone within its 4-env and within its 16-env group (the group sizes of the
    rollout kernels), and at least one episode ends by truncation."""
    c = desync_counts(term, trunc)
    assert c["termination_steps"] >= 40 and c["terminations"] >= 60 and c["envs_that_terminate"] >= 24, c
    assert c["lone_in_4"] >= 1 and c["lone_in_16"] >= 1 and c["truncations"] >= 1, c
    return c


def deriv_f64(s, a):
    th1, th2, w1, w2 = s
    m1 = m2 = 1.0
    l1 = 1.0
    lc1 = lc2 = 0.5
    i1 = i2 = 1.0
    g = 9.8
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * np.cos(th2)) + i1 + i2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * np.cos(th2)) + i2
    phi2 = m2 * lc2 * g * np.sin(th1 + th2)
    phi1 = -m2 * l1 * lc2 * w2 ** 2 * np.sin(th2) - 2 * m2 * l1 * lc2 * w2 * w1 * np.sin(th2) + (m1 * lc1 + m2 * l1) * g * np.sin(th1) + phi2
    acc2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 ** 2 * np.sin(th2) - phi2) / (m2 * lc2 ** 2 + i2 - d2 ** 2 / d1)
    acc1 = -(d2 * acc2 + phi1) / d1
    return np.stack([w1, w2, acc1, acc2])


def wrap_f64(x):
    """into [-pi, pi)"""
    return x - 2 * np.pi * np.floor((x + np.pi) / (2 * np.pi))


def step_f64(x):
    """The issue's definition in float64 with libm trigonometry. x [n, 5] = (theta1, theta2, theta1dot,
    theta2dot, a). Returns the new state [n, 4], the observation [n, 6], the termination margin
    -cos theta1' - cos(theta1' + theta2') - 1 [n] (terminated where > 0) and the largest |stage angle|
    (an argument of sin or cos inside the four derivative evaluations, theta1 + theta2 not among them:
    the fp32 code never takes a function of the sum) [n]."""
    s = x[:, :4].astype(np.float64).T
    a = np.clip(x[:, 4].astype(np.float64), -1.0, 1.0)
    k1 = deriv_f64(s, a)
    y2 = s + DT / 2 * k1
    k2 = deriv_f64(y2, a)
    y3 = s + DT / 2 * k2
    k3 = deriv_f64(y3, a)
    y4 = s + DT * k3
    k4 = deriv_f64(y4, a)
    n = s + DT / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    stage = np.max(np.abs(np.stack([s[:2], y2[:2], y3[:2], y4[:2]])), axis=(0, 1))
    n[0], n[1] = wrap_f64(n[0]), wrap_f64(n[1])
    n[2] = np.clip(n[2], -MAX_VEL_1, MAX_VEL_1)
    n[3] = np.clip(n[3], -MAX_VEL_2, MAX_VEL_2)
    obs = np.stack([np.cos(n[0]), np.sin(n[0]), np.cos(n[1]), np.sin(n[1]), n[2], n[3]], 1)
    margin = -np.cos(n[0]) - np.cos(n[0] + n[1]) - 1.0
    return n.T, obs, margin, stage


def circ_dist(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 2 * np.pi - d)


class HostAcrobot:
    """SeqVectorEnv over RecordEpisodeStatistics(gymcpp::AcrobotContinuous), clip_actions on: the driver
    built as a shared object, for closed loops (the learning reference)."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            d = tempfile.mkdtemp(prefix="acrodrv")
            so = os.path.join(d, "libacrodrv.so")
            subprocess.run(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", SRC, "-o", so],
                           check=True)
            cls._lib = C.CDLL(so)
            cls._lib.acrodrv_create.restype = C.c_void_p
            cls._lib.acrodrv_create.argtypes = [C.c_int, C.c_int]
            cls._lib.acrodrv_destroy.argtypes = [C.c_void_p]
            cls._lib.acrodrv_reset.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            cls._lib.acrodrv_step.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        return cls._lib

    def __init__(self, E):
        self.E = E
        self.h = self.lib().acrodrv_create(E, 1)
        self.obs = np.zeros((E, OD), np.float32)
        self.rew, self.term, self.done, self.ret, self.len = (np.zeros(E, np.float32) for _ in range(5))

    def reset(self, seed):
        self.lib().acrodrv_reset(self.h, seed, self.obs.ctypes.data)
        return self.obs.copy()

    def step(self, act):
        act = np.ascontiguousarray(act, np.float32)
        assert act.shape == (self.E, AD)
        self.lib().acrodrv_step(self.h, act.ctypes.data, self.obs.ctypes.data, self.rew.ctypes.data, self.term.ctypes.data,
                                self.done.ctypes.data, self.ret.ctypes.data, self.len.ctypes.data)
        # (obs, reward, term, done, return, length): the termination flags after the rewards
        return self.obs.copy(), self.rew.copy(), self.term.copy(), self.done.copy(), self.ret.copy(), self.len.copy()

    def close(self):
        if self.h:
            self.lib().acrodrv_destroy(self.h)
            self.h = None
