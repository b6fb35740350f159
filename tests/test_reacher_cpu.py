"""ReacherPlanar-v0 on the host: the shared arithmetic of include/ppo_reacher.h and the host env
gymcpp/reacher.h, through tests/native/reacher_driver.cpp (built here with g++ -ffp-contract=off).
The env is a two-link planar arm with Gymnasium Reacher-v5's task definition over the textbook
two-link manipulator equations; it is not MuJoCo's Reacher.

  1. one teacher-forced step against the float64 restatement reacher_common.step_f64 (libm
     trigonometry), per output: angles (circular distance), joint speeds, reward, observation;
  2. the driver built at -O0 and at -O2 writes the same bytes;
  3. reset: reproducible per (seed, env), q and qdot within their ranges, the goal inside the disc and
     uniform in it (mean radius 2/15 over 10^4 resets);
  4. SeqVectorEnv + RecordEpisodeStatistics semantics over T = 120, E = 5: truncation exactly at steps
     50 and 101, the goal constant within an episode and redrawn at every reset;
  5. the two action dimensions are not interchangeable;
  6. the refusals of psyn_create_env and of the CLIs happen before any HIP call;
  7. the learning fixtures carry their condition, config, seeds and runs.

The bounds of 1 are twice the maximum errors measured on the CPU over the inputs of _step_inputs()
against step_f64: angles 4.4693e-7 rad (half an fp32 ulp at pi is 1.2e-7), joint
speeds 1.7860e-5 rad/s (at |qdot| near 32 the Coriolis torque, up to 17, over det M >= 2.35e-5
amplifies fp32 rounding; half an fp32 ulp of 32 is 1.9e-6), reward 9.2317e-8, observation 1.7860e-5
(its joint-speed entries; the trigonometric entries are below 4.5e-7, the tip entries below 9.4e-8)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import reacher_common as rc

ROOT = rc.ROOT
# measured maxima (this file's docstring); the bounds are twice these
MEASURED = {"angle": 4.4693e-7, "speed": 1.7860e-5, "reward": 9.2317e-8, "obs": 1.7860e-5}
BOUND = {k: 2 * v for k, v in MEASURED.items()}
N_RANDOM = 100000
PI32 = np.float32(np.pi)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("reach")
    return {"O2": rc.build_driver(str(d / "rd_O2"), "-O2"), "O0": rc.build_driver(str(d / "rd_O0"), "-O0")}


def _corners():
    """q2 in {0, +-pi/2, -pi, the largest float below pi} x qdot = (+-32, +-32) x actions: a = +-1 and
    +-1e30 in both dimensions, and pairs whose two dimensions differ."""
    f32 = np.float32
    q2s = [0.0, np.pi / 2, -np.pi / 2, -PI32, np.nextafter(PI32, f32(0))]
    acts = [(1, 1), (-1, -1), (1e30, 1e30), (-1e30, -1e30), (1, -1), (-1, 1), (1e30, -1e30), (0.25, -0.75), (-0.75, 0.25)]
    rows = []
    for q2 in q2s:
        for v1 in (32.0, -32.0):
            for v2 in (32.0, -32.0):
                for a0, a1 in acts:
                    rows.append([0.3, q2, v1, v2, 0.05, -0.12, a0, a1])
    return np.array(rows, np.float32)


def _step_inputs():
    rng = np.random.default_rng(11)
    n = N_RANDOM
    rho, phi = 0.2 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(-np.pi, np.pi, n)
    x = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-32, 32, n),
                  rng.uniform(-32, 32, n), rho * np.cos(phi), rho * np.sin(phi), rng.uniform(-1.5, 1.5, n),
                  rng.uniform(-1.5, 1.5, n)], 1).astype(np.float32)
    x[:, :2] = np.where(x[:, :2] >= PI32, -PI32, x[:, :2])  # fp32 rounding of a value just below pi
    return np.concatenate([x, _corners()]).astype(np.float32)


def step_errors(x, s, rew, obs):
    """largest error per output against step_f64"""
    s64, r64, o64 = rc.step_f64(x)
    return {"angle": float(rc.circ_dist(s[:, :2], s64[:, :2]).max()),
            "speed": float(np.abs(s[:, 2:4] - s64[:, 2:4]).max()),
            "reward": float(np.abs(rew - r64).max()),
            "obs": float(np.abs(obs - o64).max()),
            "obs_by_entry": np.abs(obs - o64).max(0)}


def test_one_step_against_float64(drivers, tmp_path):
    x = _step_inputs()
    r = x[:N_RANDOM]
    assert (r[:, :2] >= -PI32).all() and (r[:, :2] < PI32).all() and np.abs(r[:, 2:4]).max() <= 32
    assert np.hypot(r[:, 4].astype(np.float64), r[:, 5]).max() <= 0.2 + 1e-7 and np.abs(r[:, 6:]).max() <= 1.5
    s, rew, obs = rc.host_step(drivers["O2"], tmp_path, x)
    err = step_errors(x, s, rew, obs)
    print({k: (f"{v:.4e}" if np.isscalar(v) else np.array2string(v, precision=3)) for k, v in err.items()})
    print("bounds", {k: f"{v:.4e}" for k, v in BOUND.items()})
    for k in BOUND:
        assert err[k] <= BOUND[k], (k, err[k], BOUND[k])
    # the new state stays in its domain; the goal slots are untouched, bit for bit
    assert (s[:, :2] >= -PI32).all() and (s[:, :2] < PI32).all() and np.abs(s[:, 2:4]).max() <= 32
    np.testing.assert_array_equal(s[:, 4:6].view(np.uint32), x[:, 4:6].view(np.uint32))
    np.testing.assert_array_equal(obs[:, 4:6].view(np.uint32), x[:, 4:6].view(np.uint32))
    np.testing.assert_array_equal(obs[:, 6:8].view(np.uint32), s[:, 2:4].view(np.uint32))
    # a = +-1e30 is the clipped a = +-1
    c = x[N_RANDOM:]
    big = np.abs(c[:, 6]) > 1e29
    assert big.sum() >= 20
    twin = c[big].copy()
    twin[:, 6:] = np.sign(twin[:, 6:])
    ts, tr, to = rc.host_step(drivers["O2"], tmp_path, twin, "twin")
    np.testing.assert_array_equal(ts.view(np.uint32), s[N_RANDOM:][big].view(np.uint32))
    np.testing.assert_array_equal(tr.view(np.uint32), rew[N_RANDOM:][big].view(np.uint32))
    np.testing.assert_array_equal(to.view(np.uint32), obs[N_RANDOM:][big].view(np.uint32))


def test_no_contraction_O0_equals_O2(drivers, tmp_path):
    _step_inputs().tofile(tmp_path / "s.f32")
    E, T = 3, 120
    np.random.default_rng(2).uniform(-3, 3, (T, E, 2)).astype(np.float32).tofile(tmp_path / "a.f32")
    outs = {}
    for k, exe in drivers.items():
        rc.run_driver(exe, "step", tmp_path / "s.f32", tmp_path / f"s_{k}.out")
        rc.run_driver(exe, "vecw", E, T, 3, 1, tmp_path / "a.f32", tmp_path / f"v_{k}.out", 0.99)
        rc.run_driver(exe, "reset", 5, 100, tmp_path / f"r_{k}.out")
        outs[k] = [(tmp_path / f"{n}_{k}.out").read_bytes() for n in "svr"]
    assert all(len(b) > 0 for b in outs["O2"])
    assert outs["O0"] == outs["O2"]


def test_reset_is_reproducible_in_range_and_uniform_in_the_disc(drivers, tmp_path):
    E, seed = 64, 9
    act = np.zeros((1, E, 2), np.float32)
    raw, o0, _ = rc.host_vec(drivers["O2"], tmp_path, E, 1, seed, "a", act)
    raw2, _, _ = rc.host_vec(drivers["O2"], tmp_path, E, 1, seed, "b", act)
    assert raw == raw2
    for i in (0, 1, 17, 63):  # env i is seeded seed + i
        _, oi, _ = rc.host_vec(drivers["O2"], tmp_path, 1, 1, seed + i, f"s{i}", act[:, :1])
        np.testing.assert_array_equal(oi[0], o0[i])
    assert len({o0[i].tobytes() for i in range(E)}) == E
    # 10^4 resets of one env: ranges, the disc, the mean radius
    n = 10000
    rc.run_driver(drivers["O2"], "reset", 7, n, tmp_path / "r.out")
    s = np.fromfile(tmp_path / "r.out", np.float32).reshape(n, rc.SD)
    assert (np.abs(s[:, :2]) <= np.float32(0.1)).all() and s[:, :2].std() > 0.05
    assert (np.abs(s[:, 2:4]) <= np.float32(0.005)).all() and s[:, 2:4].std() > 0.0025
    rad = np.hypot(s[:, 4].astype(np.float64), s[:, 5].astype(np.float64))
    assert rad.max() <= np.float32(0.2), rad.max()
    # uniform in the disc of radius R: E[r] = 2R/3 = 2/15, Var[r] = R^2/18
    se = 0.2 / np.sqrt(18.0) / np.sqrt(n)
    print(f"goal radius: mean {rad.mean():.6f} (2/15 = {2 / 15:.6f}, 3 se = {3 * se:.6f}), max {rad.max():.6f}")
    assert abs(rad.mean() - 2 / 15) <= 3 * se
    ang = np.arctan2(s[:, 5], s[:, 4])
    assert abs(ang.mean()) < 0.1 and ang.min() < -3.0 and ang.max() > 3.0  # all the way round
    assert len(set(s[:, 4].tolist())) > n - 10  # a goal of its own per reset
    # the observation of a reset state: Reacher-v5's order
    o64 = rc.obs_f64(s[:1].astype(np.float64))
    _, o1, _ = rc.host_vec(drivers["O2"], tmp_path, 1, 1, 7, "one", act[:, :1])
    np.testing.assert_allclose(o1, o64, rtol=0, atol=2e-7)


def test_vector_semantics_truncation_and_goal(drivers, tmp_path):
    E, T, seed = 5, 120, 9
    act = np.random.default_rng(4).uniform(-3, 3, (T, E, 2)).astype(np.float32)
    _, o0, s = rc.host_vec(drivers["O2"], tmp_path, E, T, seed, "a", act)
    assert not s["term"].any()
    assert sorted(set(np.nonzero(s["trunc"])[0].tolist())) == [49, 100]  # the 50th step; reset on the 51st
    for t0, t in ((0, 49), (51, 100)):
        assert (s["trunc"][t] == 1).all() and (s["len"][t] == 50).all()
        ret = np.zeros(E, np.float32)
        for k in range(t0, t + 1):  # RecordEpisodeStatistics adds in fp32, step by step
            ret = (ret + s["rew"][k]).astype(np.float32)
        np.testing.assert_array_equal(s["ret"][t], ret)
        assert (s["rew"][t0:t + 1] < 0).all()
    for t in (50, 101):  # the step after: the reset, reward 0, done 0
        assert (s["rew"][t] == 0).all() and (s["trunc"][t] == 0).all() and (s["len"][t] == 0).all()
        assert (np.abs(s["obs"][t][:, 6:8]) <= np.float32(0.005)).all()  # fresh joint speeds
    # the goal: constant within an episode, different between consecutive episodes and between envs
    goal0 = o0[:, 4:6]
    ep = [(goal0, s["obs"][0:50]), (s["obs"][50][:, 4:6], s["obs"][50:101]), (s["obs"][101][:, 4:6], s["obs"][101:])]
    for g, ob in ep:
        np.testing.assert_array_equal(ob[:, :, 4:6], np.broadcast_to(g, ob[:, :, 4:6].shape))
        assert len({g[e].tobytes() for e in range(E)}) == E
        assert (np.hypot(g[:, 0], g[:, 1]) <= 0.2).all()
    for (g0, _), (g1, _) in zip(ep[:-1], ep[1:]):
        assert (g0 != g1).all(1).all()
    # d = tip - goal on the new state
    ob = s["obs"].reshape(-1, rc.OD).astype(np.float64)
    c1, c2, s1, s2 = ob[:, 0], ob[:, 1], ob[:, 2], ob[:, 3]
    tipx = 0.1 * c1 + 0.11 * (c1 * c2 - s1 * s2)
    tipy = 0.1 * s1 + 0.11 * (s1 * c2 + c1 * s2)
    np.testing.assert_allclose(ob[:, 8], tipx - ob[:, 4], rtol=0, atol=1e-7)
    np.testing.assert_allclose(ob[:, 9], tipy - ob[:, 5], rtol=0, atol=1e-7)


def test_action_dimensions_are_not_interchangeable(drivers, tmp_path):
    rng = np.random.default_rng(8)
    n = 64
    x = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n),
                  rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)],
                 1).astype(np.float32)
    assert (np.abs(x[:, 6] - x[:, 7]) > 1e-3).all()
    y = x.copy()
    y[:, 6], y[:, 7] = x[:, 7], x[:, 6]
    sx, rx, _ = rc.host_step(drivers["O2"], tmp_path, x, "x")
    sy, ry, _ = rc.host_step(drivers["O2"], tmp_path, y, "y")
    assert (sx[:, 2] != sy[:, 2]).all() and (sx[:, 3] != sy[:, 3]).all()
    # each dimension alone moves the arm, and differently
    z0, z1 = x.copy(), x.copy()
    z0[:, 7] = 0
    z1[:, 6] = 0
    s0, _, _ = rc.host_step(drivers["O2"], tmp_path, z0, "z0")
    s1, _, _ = rc.host_step(drivers["O2"], tmp_path, z1, "z1")
    assert (s0[:, 2:4] != sx[:, 2:4]).any(1).all() and (s1[:, 2:4] != sx[:, 2:4]).any(1).all()


def test_refusals_come_before_any_hip_call():
    """psyn_create_env refuses an unknown id (the message keeps its text and names the new id after
    it), NULL and a non-positive E, with a message and no env, before it touches the GPU (this machine
    may have none). A fresh interpreter, as test_capi_cpu does."""
    script = r'''
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import ppo_amd
lib = ppo_amd.lib()
out = []
RP = b"ReacherPlanar-v0"
for env_id, E, null_out in ((b"Walker2d-v5", 4, False), (None, 4, False), (RP, 0, False), (RP, -3, False), (RP, 4, True)):
    h = ctypes.c_void_p()
    rc = lib.psyn_create_env(env_id, E, None if null_out else ctypes.byref(h))
    out.append([rc, bool(h.value), lib.ppo_last_error().decode()])
print(json.dumps(out))
'''
    res = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "ppo.cpp_amd")], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    old = "unknown env_id Walker2d-v5 (Pendulum-v1, SyntheticCheetah-v0), CartPoleContinuous-v1"
    want = [old, "null argument", "num_envs must be positive", "num_envs must be positive", "null argument"]
    assert len(got) == len(want)
    for (rc_, made, msg), w in zip(got, want):
        assert rc_ == -1 and not made and w in msg, (rc_, made, msg, w)
    assert got[0][2].index(rc.ENV_ID) > got[0][2].index(old)  # the new id, after the old text


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
@pytest.mark.parametrize("flag", ["host_step_us", "straggler_us"])
def test_cli_refuses_host_step_us_with_reacher(exe, flag):
    """--host_step_us / --straggler_us stand in for the physics of the MuJoCo envs the synthetic
    cheetah replaces: with ReacherPlanar-v0 they are refused (ac: the flags apply to
    SyntheticCheetah-v0 only, a refusal that needs the host env of this id to exist; ppo: no such flags,
    so its two cases show the flag parser: test_cli_host_backend_knows_the_id is the check of that CLI)."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    r = subprocess.run([path, "--env_id", rc.ENV_ID, "--env_backend", "host", f"--{flag}", "5", "--num_envs", "2",
                        "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem", "t_reach_refuse"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, r.stdout[-500:]
    assert flag in r.stderr
    assert "Number of parameters" not in r.stdout  # refused before the agent was created


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
def test_cli_host_backend_knows_the_id(exe):
    """The same command without the flag gets past the creation of the host envs: no "is not
    implemented" (the answer to an unknown id, which lists this id). Without a GPU it then stops at the
    agent's creation; with one it trains its 8 steps."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    args = ["--env_backend", "host", "--num_envs", "2", "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem",
            "t_reach_known"]
    r = subprocess.run([path, "--env_id", rc.ENV_ID] + args, capture_output=True, text=True, timeout=120)
    assert "is not implemented" not in r.stderr and "needs MuJoCo" not in r.stderr, r.stderr[-500:]
    u = subprocess.run([path, "--env_id", "ReacherPlanar-v1"] + args, capture_output=True, text=True, timeout=120)
    assert u.returncode != 0 and "is not implemented" in u.stderr and rc.ENV_ID in u.stderr
    assert u.stderr.index(rc.ENV_ID) > u.stderr.index("CartPoleContinuous-v1")


def test_binding_declares_the_env_id():
    import ppo_amd
    assert ppo_amd.ENV_DIMS[rc.ENV_ID] == (10, 2, -1.0, 1.0)
    assert ppo_amd.PSYN_REACHER == 3 and ppo_amd.DEVICE_ENV_KINDS[-1] == rc.ENV_ID
    assert ppo_amd.obs_norm(rc.ENV_ID) is None  # answered as CartPoleContinuous-v1 is: n = 0, identity
    cfg = ppo_amd.ACPPOConfig(env_id=rc.ENV_ID)
    h = ppo_amd.hip_config(cfg)
    assert (h.obs_dim, h.act_dim) == (10, 2)
    L = ppo_amd.agent_layout(ppo_amd.PPO_NET_LN_BETA, 10, 2, 256)
    p = ppo_amd.init_params(L, seed=1, env_id=rc.ENV_ID)
    assert p[L.hi] == 1.0 and p[L.lo] == -1.0
    assert (p[L.omean:L.omean + 10] == 0).all() and (p[L.ostd:L.ostd + 10] == 1).all()


@pytest.mark.parametrize("name,agent", [("learning_ref.json", "ppo"), ("learning_ref_ac.json", "ac")])
def test_learning_fixture(name, agent):
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reacher", name)))
    assert ref["env_id"] == rc.ENV_ID and ref["condition_met"] is True
    assert ref["config"]["agent"] == agent and len(ref["seeds"]) == 3 and len(ref["runs"]) == 3
    un = [r["untrained"] for r in ref["runs"]]
    spread = max(un) - min(un)
    for r, seed in zip(ref["runs"], ref["seeds"]):
        assert r["seed"] == seed and r["trained"] - r["untrained"] >= 2 * spread
    for k in ("num_envs", "num_steps", "total_timesteps", "num_minibatches", "update_epochs", "learning_rate", "gamma"):
        assert k in ref["config"]
