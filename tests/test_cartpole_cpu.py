"""CartPoleContinuous-v1 on the host: the shared arithmetic of include/ppo_cartpole.h and the host env
gymcpp/cartpole.h, through tests/native/cartpole_driver.cpp (built here with g++ -ffp-contract=off).

  1. one teacher-forced step against a float64 restatement of Gymnasium's cartpole.py step
     (cartpole_common.gym_step_f64), the termination flag included;
  2. the driver built at -O0 and at -O2 writes the same bytes; reset is reproducible per (seed, env)
     and its four values lie in [-0.05, 0.05];
  3. SeqVectorEnv + RecordEpisodeStatistics semantics with episodes that terminate: the terminating
     step carries reward 1 and done 1, the next step is the reset with reward 0 and done 0, truncation
     at step 500 under the driver's balancing actions, episode return = episode length;
  4. the desynchronisation condition the GPU tests build on (E = 37, seed 6, actions in [-3, 3]);
  5. the refusals of psyn_create_env and of the CLIs happen before any HIP call.

The bound of 1 is twice the maximum error of the new state measured on the CPU over the inputs of
_step_inputs(): 1.949e-7, reached by thetadot' (|thetadot'| up to 4.1, where half an
fp32 ulp is 2.4e-7); x' 1.2e-7, xdot' 1.5e-7, theta' 1.6e-8."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cartpole_common as cc

ROOT = cc.ROOT
STEP_MEASURED = 1.949e-7
STEP_BOUND = 2 * STEP_MEASURED
X32, TH32 = np.float32(cc.X_THRESHOLD), np.float32(cc.THETA_THRESHOLD)
N_RANDOM = 100000


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("cart")
    return {"O2": cc.build_driver(str(d / "cd_O2"), "-O2"), "O0": cc.build_driver(str(d / "cd_O0"), "-O0")}


def _corners():
    """Thresholds +-1 ulp in x (xdot = 0: x' = x exactly) and in theta (thetadot = 0: theta' = theta),
    each with a = +-1 and +-1e30."""
    f32 = np.float32
    rows = []
    for sign, a in itertools.product((1, -1), (1.0, -1.0, 1e30, -1e30)):
        for v in (X32, np.nextafter(X32, f32(3)), np.nextafter(X32, f32(0))):
            rows.append([sign * v, 0.0, 0.01, 0.3, a])
        for v in (TH32, np.nextafter(TH32, f32(1)), np.nextafter(TH32, f32(0))):
            rows.append([0.5, 0.3, sign * v, 0.0, a])
    return np.array(rows, np.float32)


def _step_inputs():
    rng = np.random.default_rng(11)
    n = N_RANDOM
    x = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-0.26, 0.26, n), rng.uniform(-3.5, 3.5, n),
                  rng.uniform(-1.5, 1.5, n)], 1).astype(np.float32)
    return np.concatenate([x, _corners()]).astype(np.float32)


def test_one_step_against_gymnasium_float64(drivers, tmp_path):
    x = _step_inputs()
    assert np.abs(x[:N_RANDOM, 0]).max() <= 3 and np.abs(x[:N_RANDOM, 2]).max() <= 0.26
    x.tofile(tmp_path / "x.f32")
    cc.run_driver(drivers["O2"], "step", tmp_path / "x.f32", tmp_path / "o.f32")
    o = np.fromfile(tmp_path / "o.f32", np.float32).reshape(-1, 6)
    assert len(o) == len(x)
    s64, t64 = cc.gym_step_f64(x)
    err = np.abs(o[:, :4] - s64)
    print(f"max |err| of (x', xdot', theta', thetadot') {err.max(0)}  overall {err.max():.4e}  bound {STEP_BOUND:.4e}")
    assert err.max() <= STEP_BOUND
    assert (o[:, 4] == 1.0).all()  # reward 1 on every step, the terminating one included
    assert set(np.unique(o[:, 5]).tolist()) == {0.0, 1.0}
    # the termination flag equals the float64 one wherever the float64 |x'| and |theta'| are farther
    # from their thresholds than the bound
    near = (np.abs(np.abs(s64[:, 0]) - cc.X_THRESHOLD) <= STEP_BOUND) | (np.abs(np.abs(s64[:, 2]) - cc.THETA_THRESHOLD) <= STEP_BOUND)
    share, share_rand = near.mean(), near[:N_RANDOM].sum() / len(x)
    print(f"near-threshold cases: {near.sum()} of {len(x)} ({share:.2e}); random inputs alone {near[:N_RANDOM].sum()}")
    assert share <= 1e-3 and share_rand <= 1e-3 and near[:N_RANDOM].mean() <= 1e-3
    cmp_ = ~near
    np.testing.assert_array_equal(o[cmp_, 5] != 0, t64[cmp_])
    by_x = cmp_ & (np.abs(s64[:, 0]) > cc.X_THRESHOLD)
    by_th = cmp_ & (np.abs(s64[:, 2]) > cc.THETA_THRESHOLD)
    print(f"compared: {by_x.sum()} terminations by x, {by_th.sum()} by theta, {(cmp_ & ~t64).sum()} non-terminations")
    assert by_x.sum() > 100 and by_th.sum() > 100 and (by_th & ~by_x).any() and (by_x & ~by_th).any()
    assert (cmp_ & ~t64).sum() > 100
    # the corners: x' = x and theta' = theta exactly, and the flag is the fp32 comparison of the new state
    c, oc = x[N_RANDOM:], o[N_RANDOM:]
    mx, mt = c[:, 1] == 0, c[:, 3] == 0
    np.testing.assert_array_equal(oc[mx, 0], c[mx, 0])
    np.testing.assert_array_equal(oc[mt, 2], c[mt, 2])
    want = (np.abs(oc[:, 0]) > X32) | (np.abs(oc[:, 2]) > TH32)
    np.testing.assert_array_equal(oc[:, 5] != 0, want)
    assert want.any() and not want.all()
    # a = +-1e30 is the clipped a = +-1
    big = np.abs(c[:, 4]) > 1e29
    twin = c.copy()
    twin[:, 4] = np.sign(twin[:, 4])
    for row, o_big in zip(twin[big], oc[big]):
        k = np.nonzero((c == row).all(1))[0][0]
        np.testing.assert_array_equal(oc[k], o_big)


def test_no_contraction_O0_equals_O2(drivers, tmp_path):
    _step_inputs().tofile(tmp_path / "s.f32")
    E, T = 3, 450
    np.random.default_rng(2).uniform(-3, 3, (T, E, 1)).astype(np.float32).tofile(tmp_path / "a.f32")
    outs = {}
    for k, exe in drivers.items():
        cc.run_driver(exe, "step", tmp_path / "s.f32", tmp_path / f"s_{k}.out")
        cc.run_driver(exe, "vecw", E, T, 3, 1, tmp_path / "a.f32", tmp_path / f"v_{k}.out", 0.99)
        cc.run_driver(exe, "balance", E, 600, 3, tmp_path / f"b_{k}.out")
        outs[k] = [(tmp_path / f"{n}_{k}.out").read_bytes() for n in "svb"]
    assert all(len(b) > 0 for b in outs["O2"])
    assert outs["O0"] == outs["O2"]


def test_reset_is_reproducible_and_small(drivers, tmp_path):
    E, seed = 64, 9
    act = np.zeros((1, E, 1), np.float32)
    raw, o0, _ = cc.host_vec(drivers["O2"], tmp_path, E, 1, seed, "a", act)
    raw2, _, _ = cc.host_vec(drivers["O2"], tmp_path, E, 1, seed, "b", act)
    assert raw == raw2
    # 0.1 u - 0.05 in fp32 with u in (0, 1]: within [-0.05f, 0.05f] (0.1f is exactly 2 * 0.05f)
    assert (np.abs(o0) <= np.float32(0.05)).all() and o0.std() > 0.02
    for i in (0, 1, 17, 63):  # env i is seeded seed + i
        _, oi, _ = cc.host_vec(drivers["O2"], tmp_path, 1, 1, seed + i, f"s{i}", act[:, :1])
        np.testing.assert_array_equal(oi[0], o0[i])
    assert len({o0[i].tobytes() for i in range(E)}) == E
    assert len(set(o0.reshape(-1).tolist())) == 4 * E  # four draws of their own per env


def test_vector_semantics_termination(drivers, tmp_path):
    E, T, seed = 5, 300, 9
    act = np.random.default_rng(4).uniform(-3, 3, (T, E, 1)).astype(np.float32)
    _, o0, s = cc.host_vec(drivers["O2"], tmp_path, E, T, seed, "a", act)
    assert not s["trunc"].any() and s["term"].sum() >= 5 * E
    first = None
    for e in range(E):
        ends = np.nonzero(s["term"][:, e])[0]
        start = 0
        for t in ends:
            # the terminating step: reward 1, done 1, a state beyond a threshold, the episode's statistics
            assert s["rew"][t, e] == 1 and s["term"][t, e] == 1
            ob = s["obs"][t, e]
            assert abs(ob[0]) > X32 or abs(ob[2]) > TH32
            assert s["len"][t, e] == t - start + 1 and s["ret"][t, e] == s["len"][t, e]  # return = length
            assert (s["rew"][start:t + 1, e] == 1).all() and (s["len"][start:t, e] == 0).all()
            # the next step is the reset: reward 0, done 0, a fresh small state
            if t + 1 < T:
                assert s["rew"][t + 1, e] == 0 and s["term"][t + 1, e] == 0 and s["trunc"][t + 1, e] == 0
                assert s["len"][t + 1, e] == 0 and (np.abs(s["obs"][t + 1, e]) <= np.float32(0.05)).all()
                first = s["obs"][t + 1, e] if first is None else first
            start = t + 2
    assert first is not None and not any(np.array_equal(first, o0[e]) for e in range(E))  # the reset count goes on


def test_truncation_at_500_under_balancing_actions(drivers, tmp_path):
    E, T = 3, 1100
    cc.run_driver(drivers["O2"], "balance", E, T, 9, tmp_path / "b.out")
    _, s = cc.parse_vec((tmp_path / "b.out").read_bytes(), E, T)
    assert not s["term"].any()
    assert sorted(set(np.nonzero(s["trunc"])[0].tolist())) == [499, 1000]  # the 500th step; reset on the 501st
    for t in (499, 1000):
        assert (s["trunc"][t] == 1).all() and (s["rew"][t] == 1).all()
        assert (s["len"][t] == 500).all() and (s["ret"][t] == 500).all()
    for t in (500, 1001):
        assert (s["rew"][t] == 0).all() and (s["trunc"][t] == 0).all() and (s["len"][t] == 0).all()
    assert np.abs(s["obs"][..., 0]).max() < 1.0 and np.abs(s["obs"][..., 2]).max() < 0.1


def test_desynchronisation_condition(drivers, tmp_path):
    """E = 37, seed 6, actions uniform in [-3, 3], 450 steps: what the GPU tests inherit."""
    _, _, s = cc.host_vec(drivers["O2"], tmp_path, cc.DESYNC_E, cc.DESYNC_T, cc.DESYNC_SEED, "d", cc.desync_actions())
    done = (s["term"] != 0) | (s["trunc"] != 0)
    print(f"episodes end on {done.any(1).sum()} distinct steps; per env {done.sum(0).min()}..{done.sum(0).max()} episodes")
    cc.assert_desynchronised(done, group=4)
    cc.assert_desynchronised(done, group=16)


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
CP = b"CartPoleContinuous-v1"
for env_id, E, null_out in ((b"Walker2d-v5", 4, False), (None, 4, False), (CP, 0, False), (CP, -3, False), (CP, 4, True)):
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
            "num_envs must be positive", "null argument"]
    assert len(got) == len(want)
    for (rc, made, msg), w in zip(got, want):
        assert rc == -1 and not made and w in msg, (rc, made, msg, w)
    old = "unknown env_id Walker2d-v5 (Pendulum-v1, SyntheticCheetah-v0)"
    assert got[0][2].index(cc.ENV_ID) > got[0][2].index(old)  # the new id, after the old text


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
@pytest.mark.parametrize("flag", ["host_step_us", "straggler_us"])
def test_cli_refuses_host_step_us_with_cartpole(exe, flag):
    """--host_step_us / --straggler_us stand in for the physics of the MuJoCo envs the synthetic
    cheetah replaces: with CartPoleContinuous-v1 they are refused (ac: the flags apply to
    SyntheticCheetah-v0 only, a refusal that needs the host env of this id to exist; ppo: no such flags,
    so its two cases show the flag parser and pass without this env: test_cli_host_backend_knows_the_id
    is the check of that CLI)."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    r = subprocess.run([path, "--env_id", cc.ENV_ID, "--env_backend", "host", f"--{flag}", "5", "--num_envs", "2",
                        "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem", "t_cart_refuse"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, r.stdout[-500:]
    assert flag in r.stderr
    assert "Number of parameters" not in r.stdout  # refused before the agent was created


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
def test_cli_host_backend_knows_the_id(exe):
    """The refusals above are about this env only if the CLI knows it: for ppo_continuous_action, which
    has no such flags at all, they show the flag parser alone. The same command without the flag gets
    past the creation of the host envs: no "is not implemented" (the answer to an unknown id). Without
    a GPU it then stops at the agent's creation; with one it trains its 8 steps."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    args = ["--env_backend", "host", "--num_envs", "2", "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem",
            "t_cart_known"]
    r = subprocess.run([path, "--env_id", cc.ENV_ID] + args, capture_output=True, text=True, timeout=120)
    assert "is not implemented" not in r.stderr and "needs MuJoCo" not in r.stderr, r.stderr[-500:]
    u = subprocess.run([path, "--env_id", "CartPoleContinuous-v0"] + args, capture_output=True, text=True, timeout=120)
    assert u.returncode != 0 and "is not implemented" in u.stderr and cc.ENV_ID in u.stderr


def test_binding_declares_the_env_id():
    import ppo_amd
    assert ppo_amd.ENV_DIMS[cc.ENV_ID] == (4, 1, -1.0, 1.0)
    assert ppo_amd.PSYN_CARTPOLE == 2 and cc.ENV_ID in ppo_amd.DEVICE_ENV_KINDS
    assert ppo_amd.obs_norm(cc.ENV_ID) is None  # answered as HalfCheetah-v5 is: n = 0, zeros and ones
    cfg = ppo_amd.ACPPOConfig(env_id=cc.ENV_ID)
    h = ppo_amd.hip_config(cfg)
    assert (h.obs_dim, h.act_dim) == (4, 1)
    L = ppo_amd.agent_layout(ppo_amd.PPO_NET_LN_BETA, 4, 1, 256)
    p = ppo_amd.init_params(L, seed=1, env_id=cc.ENV_ID)
    assert p[L.hi] == 1.0 and p[L.lo] == -1.0
    assert (p[L.omean:L.omean + 4] == 0).all() and (p[L.ostd:L.ostd + 4] == 1).all()
