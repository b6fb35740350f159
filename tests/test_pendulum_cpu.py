"""Pendulum-v1 on the host: the shared arithmetic of include/ppo_pendulum.h and the host env
gymcpp/pendulum.h, through tests/native/pendulum_driver.cpp (built here with g++ -ffp-contract=off,
as test_host_env.py builds its driver).

  1. the sine / cosine pair against numpy float64 on a dense grid;
  2. one teacher-forced step against a float64 restatement of Gymnasium's PendulumEnv.step;
  3. invariants over 10^4 free-running steps;
  4. the driver built at -O0 and at -O2 writes the same bytes (no contraction, no libm trig);
  5. SeqVectorEnv + RecordEpisodeStatistics semantics (truncation, next-step autoreset, seeding);
  6. the refusals of psyn_create_env and of the CLIs happen before any HIP call.

The bounds of 1 and 2 are twice the maximum error measured on the CPU with the committed polynomial
(DESIGN.md §7): sine / cosine 9.192e-8 (the pair is not allowed more than 2^-21); one step:
observation 3.16e-7, reward 1.934e-6 (|reward| reaches 16.3, half an fp32 ulp there is 9.5e-7),
theta' 2.91e-7 (circular distance)."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pendulum_driver.cpp")
PI32 = np.float32(np.pi)

SINCOS_BOUND = 2 * 9.192e-8
assert SINCOS_BOUND <= 2.0 ** -21
STEP_OBS_BOUND = 2 * 3.16e-7
STEP_REWARD_BOUND = 2 * 1.934e-6
STEP_THETA_BOUND = 2 * 2.91e-7


def _build(path, opt):
    subprocess.run(["g++", opt, "-std=c++20", "-ffp-contract=off", "-pthread", SRC, "-o", path], check=True)
    return path


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("pend")
    return {"O2": _build(str(d / "pd_O2"), "-O2"), "O0": _build(str(d / "pd_O0"), "-O0")}


def _run(exe, *args):
    subprocess.run([exe] + [str(a) for a in args], check=True)


def _sincos_grid():
    n = 1 << 20
    return np.concatenate([np.linspace(-np.pi - 0.5, np.pi + 0.5, n), [-np.pi - 0.5, np.pi + 0.5, 0.0]]).astype(np.float32)


def _step_inputs():
    rng = np.random.default_rng(11)
    n = 100000
    th = np.clip(rng.uniform(-np.pi, np.pi, n).astype(np.float32), -PI32, np.nextafter(PI32, np.float32(0)))
    thd = rng.uniform(-8, 8, n).astype(np.float32)
    a = rng.uniform(-3, 3, n).astype(np.float32)
    corners = np.array(list(itertools.product([PI32, -PI32], [8.0, -8.0], [2, -2, 2.5, -2.5, 1e30, -1e30])), np.float32)
    return np.concatenate([np.stack([th, thd, a], 1), corners]).astype(np.float32)


def gym_step_f64(x):
    """PendulumEnv.step in float64 (g = 10, m = l = 1, dt = 0.05, max_speed 8, max_torque 2)."""
    th, thd, a = (x[:, i].astype(np.float64) for i in range(3))
    g, m, l_, dt = 10.0, 1.0, 1.0, 0.05
    u = np.clip(a, -2.0, 2.0)
    cost = (((th + np.pi) % (2 * np.pi)) - np.pi) ** 2 + 0.1 * thd ** 2 + 0.001 * u ** 2
    nthd = np.clip(thd + (3 * g / (2 * l_) * np.sin(th) + 3.0 / (m * l_ ** 2) * u) * dt, -8.0, 8.0)
    nth = th + nthd * dt
    return np.stack([np.cos(nth), np.sin(nth), nthd], 1), -cost, nth


def test_sincos_against_float64(drivers, tmp_path):
    x = _sincos_grid()
    assert x.size >= (1 << 20) + 3
    x.tofile(tmp_path / "x.f32")
    _run(drivers["O2"], "sincos", tmp_path / "x.f32", tmp_path / "o.f32")
    o = np.fromfile(tmp_path / "o.f32", np.float32)
    s, c = o[:x.size], o[x.size:]
    x64 = x.astype(np.float64)
    es, ec = np.abs(s - np.sin(x64)).max(), np.abs(c - np.cos(x64)).max()
    print(f"max |sin err| {es:.3e}  max |cos err| {ec:.3e}  bound {SINCOS_BOUND:.3e}")
    assert es <= SINCOS_BOUND and ec <= SINCOS_BOUND


def test_one_step_against_gymnasium_float64(drivers, tmp_path):
    x = _step_inputs()
    x.tofile(tmp_path / "x.f32")
    _run(drivers["O2"], "step", tmp_path / "x.f32", tmp_path / "o.f32")
    o = np.fromfile(tmp_path / "o.f32", np.float32).reshape(-1, 6)
    obs, rew, nth = gym_step_f64(x)
    eo = np.abs(o[:, :3] - obs).max()
    er = np.abs(o[:, 3] - rew).max()
    et = np.abs(((o[:, 4].astype(np.float64) - nth + np.pi) % (2 * np.pi)) - np.pi).max()
    print(f"obs {eo:.3e} (bound {STEP_OBS_BOUND:.3e})  reward {er:.3e} ({STEP_REWARD_BOUND:.3e})  "
          f"theta' {et:.3e} ({STEP_THETA_BOUND:.3e})")
    assert eo <= STEP_OBS_BOUND and er <= STEP_REWARD_BOUND and et <= STEP_THETA_BOUND
    # the stored angle is wrapped, the speed clamped, the speed observation is the stored speed
    assert (o[:, 4] >= -PI32).all() and (o[:, 4] < PI32).all()
    assert (np.abs(o[:, 5]) <= 8).all() and np.array_equal(o[:, 2], o[:, 5])


def test_invariants_free_running(drivers, tmp_path):
    T = 10000
    act = np.random.default_rng(5).uniform(-3, 3, T).astype(np.float32)
    act.tofile(tmp_path / "a.f32")
    _run(drivers["O2"], "free", T, 7, tmp_path / "a.f32", tmp_path / "o.f32")
    o = np.fromfile(tmp_path / "o.f32", np.float32).reshape(T, 3)
    assert (o[:, 0] >= -PI32).all() and (o[:, 0] < PI32).all()
    assert (np.abs(o[:, 1]) <= 8).all()
    eps = 1e-5
    assert (o[:, 2] <= 0).all() and (o[:, 2] >= -(np.pi ** 2 + 6.4 + 0.004) - eps).all()
    assert np.ptp(o[:, 0]) > 6.0  # it does swing over the whole circle


def test_no_contraction_O0_equals_O2(drivers, tmp_path):
    _sincos_grid().tofile(tmp_path / "x.f32")
    _step_inputs().tofile(tmp_path / "s.f32")
    E, T = 3, 450
    np.random.default_rng(2).uniform(-3, 3, (T, E, 1)).astype(np.float32).tofile(tmp_path / "a.f32")
    outs = {}
    for k, exe in drivers.items():
        _run(exe, "sincos", tmp_path / "x.f32", tmp_path / f"x_{k}.out")
        _run(exe, "step", tmp_path / "s.f32", tmp_path / f"s_{k}.out")
        _run(exe, "vecw", E, T, 3, 1, tmp_path / "a.f32", tmp_path / f"v_{k}.out", 0.99)
        outs[k] = [(tmp_path / f"{n}_{k}.out").read_bytes() for n in "xsv"]
    assert all(len(b) > 0 for b in outs["O2"])
    assert outs["O0"] == outs["O2"]


def _vec(exe, tmp_path, E, T, seed, tag, act):
    act.tofile(tmp_path / f"a_{tag}.f32")
    _run(exe, "vec", E, T, seed, 1, tmp_path / f"a_{tag}.f32", tmp_path / f"v_{tag}.out")
    raw = (tmp_path / f"v_{tag}.out").read_bytes()
    out = np.frombuffer(raw, np.float32)
    O = 3
    per = E * O + 5 * E
    steps = out[E * O:].reshape(T, per)
    return raw, out[:E * O].reshape(E, O), {
        "obs": steps[:, :E * O].reshape(T, E, O), "rew": steps[:, E * O:E * O + E],
        "term": steps[:, E * O + E:E * O + 2 * E], "trunc": steps[:, E * O + 2 * E:E * O + 3 * E],
        "ret": steps[:, E * O + 3 * E:E * O + 4 * E], "len": steps[:, E * O + 4 * E:]}


def test_vector_semantics(drivers, tmp_path):
    E, T, seed = 3, 450, 9
    act = np.random.default_rng(4).uniform(-3, 3, (T, E, 1)).astype(np.float32)
    raw, o0, s = _vec(drivers["O2"], tmp_path, E, T, seed, "a", act)
    raw2, _, _ = _vec(drivers["O2"], tmp_path, E, T, seed, "b", act)
    assert raw == raw2
    assert not s["term"].any()
    trunc_steps = sorted(set(np.nonzero(s["trunc"])[0].tolist()))
    assert trunc_steps == [199, 400]  # the 200th step; reset on the 201st; the 200th step of episode 2 is step 401
    for t in (200, 401):  # next-step autoreset: reward 0, done 0, a fresh observation
        assert (s["rew"][t] == 0).all() and (s["trunc"][t] == 0).all() and (s["ret"][t] == 0).all()
    for t0, t1 in ((0, 199), (201, 400)):
        ret = np.zeros(E, np.float32)
        for t in range(t0, t1 + 1):
            ret = (ret + s["rew"][t]).astype(np.float32)
        np.testing.assert_array_equal(s["ret"][t1], ret)
        assert (s["len"][t1] == 200).all()
    assert (s["len"][[t for t in range(T) if t not in (199, 400)]] == 0).all()
    # every observation is (cos, sin, speed) of a state: unit norm to rounding
    assert np.abs(np.hypot(s["obs"][..., 0], s["obs"][..., 1]) - 1).max() < 1e-6
    # env i is seeded seed + i
    for i in range(E):
        _, oi, _ = _vec(drivers["O2"], tmp_path, 1, 1, seed + i, f"s{i}", act[:1, :1])
        np.testing.assert_array_equal(oi[0], o0[i])
    assert len({o0[i].tobytes() for i in range(E)}) == E
    # the reset after a truncation continues the env's reset count: not the first observation again
    assert not np.array_equal(s["obs"][200], o0)


def test_refusals_come_before_any_hip_call():
    """psyn_create_env refuses an unknown id, NULL and a non-positive E with a message and no env,
    before it touches the GPU (this machine may have none). A fresh interpreter, as test_capi_cpu does."""
    script = r'''
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import ppo_amd
lib = ppo_amd.lib()
out = []
for env_id, E, null_out in ((b"Walker2d-v5", 4, False), (None, 4, False), (b"Pendulum-v1", 0, False),
                            (b"Pendulum-v1", -3, False), (b"SyntheticCheetah-v0", 0, False), (b"Pendulum-v1", 4, True)):
    h = ctypes.c_void_p()
    rc = lib.psyn_create_env(env_id, E, None if null_out else ctypes.byref(h))
    out.append([rc, bool(h.value), lib.ppo_last_error().decode()])
print(json.dumps(out))
'''
    res = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "ppo.cpp_amd")], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    want = ["unknown env_id Walker2d-v5 (Pendulum-v1, SyntheticCheetah-v0)", "null argument", "num_envs must be positive",
            "num_envs must be positive", "num_envs must be positive", "null argument"]
    assert len(got) == len(want)
    for (rc, made, msg), w in zip(got, want):
        assert rc == -1 and not made and w in msg, (rc, made, msg, w)


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
def test_cli_refuses_host_step_us_with_pendulum(exe):
    """--host_step_us stands in for the physics of the MuJoCo envs the synthetic cheetah replaces:
    with Pendulum-v1 it is refused (ac: the flag applies to SyntheticCheetah-v0 only; ppo: no such flag)."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    r = subprocess.run([path, "--env_id", "Pendulum-v1", "--env_backend", "host", "--host_step_us", "5", "--num_envs", "2",
                        "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem", "t_pend_refuse"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, r.stdout[-500:]
    assert "host_step_us" in r.stderr
    assert "Number of parameters" not in r.stdout  # refused before the agent was created


def test_binding_declares_the_env_ids():
    import ppo_amd
    assert ppo_amd.ENV_DIMS["Pendulum-v1"] == (3, 1, -2.0, 2.0)
    bound = {n for n, _, _ in ppo_amd.SYMBOLS}
    assert {"psyn_create_env", "psyn_env_info"} <= bound
    cfg = ppo_amd.ACPPOConfig(env_id="Pendulum-v1")
    h = ppo_amd.hip_config(cfg)
    assert (h.obs_dim, h.act_dim) == (3, 1)
    L = ppo_amd.agent_layout(ppo_amd.PPO_NET_LN_BETA, 3, 1, 256)
    p = ppo_amd.init_params(L, seed=1, env_id="Pendulum-v1")  # no observation table: the identity
    assert p[L.hi] == 2.0 and p[L.lo] == -2.0
    assert (p[L.omean:L.omean + 3] == 0).all() and (p[L.ostd:L.ostd + 3] == 1).all()
