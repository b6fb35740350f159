"""AcrobotContinuous-v1 on the host: the shared arithmetic of include/ppo_acrobot.h and the host env
gymcpp/acrobot.h, through tests/native/acrobot_driver.cpp (built here with g++ -ffp-contract=off).

  1. one teacher-forced step against the float64 restatement with libm trigonometry
     (acrobot_common.step_f64), the termination flag and the reward included;
  2. acro_reduce, and pend_sincos after it, against float64 over twice the largest |stage angle| that
     test 1's sample and corners reach;
  3. the driver built at -O0 and at -O2 writes the same bytes; reset statistics;
  4. SeqVectorEnv + RecordEpisodeStatistics semantics with episodes that terminate on success: the
     terminating step carries reward 0 and done 1, every other step -1, the next step is the reset
     with reward 0 and done 0, episode return = 1 - episode length, truncation at step 500;
  5. the desynchronisation condition the GPU tests build on (E = 37, the driver's energy-pumping
     actions with noise, recorded for replay);
  6. the refusals of psyn_create_env and of the CLIs happen before any HIP call; the binding's
     declarations; the learning fixtures.

Measured on the CPU over the inputs of _step_inputs() (10^5 random states and 80 corners),
each bound being twice its figure:
  angles (circular distance)              2.4814e-5 rad
  speeds                                  2.2844e-3 rad/s  (median 5.3e-7, 99.9 % within 2.5e-4: the
                                          worst cases carry stage accelerations of hundreds of rad/s^2,
                                          which the unclipped stages amplify)
  observation, cos / sin                  1.9785e-5
  observation, speeds                     2.2844e-3
  -cos th1' - cos(th1' + th2') (fp32 obs) 1.8897e-5
  reward                                  0 wherever the termination flags agree
The largest |stage angle| is 31.528 rad (random states; 29.490 at the corners), so acro_reduce is
tested over |x| <= 63.06 rad: the reduced angle is within 1.1127e-7 rad of the float64 one (circular
distance), exceeds pi by at most 2.8e-6, and sin / cos after it are within 1.5639e-7 / 1.6568e-7.
16.77 % of the compared cases terminate (16 782 of 100 079); 1 case lies within the bound of the
threshold and is left out."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import acrobot_common as ac

ROOT = ac.ROOT
f32 = np.float32
N_RANDOM = 100000
ANGLE_MEASURED, SPEED_MEASURED, TRIG_MEASURED, MARGIN_MEASURED = 2.4814e-5, 2.2844e-3, 1.9785e-5, 1.8897e-5
ANGLE_BOUND, SPEED_BOUND, TRIG_BOUND, MARGIN_BOUND = (2 * v for v in (ANGLE_MEASURED, SPEED_MEASURED, TRIG_MEASURED, MARGIN_MEASURED))
STAGE_MEASURED = 31.528  # the largest |stage angle| of _step_inputs()
REDUCE_MEASURED, SIN_MEASURED, COS_MEASURED = 1.1127e-7, 1.5639e-7, 1.6568e-7
BELOW_PI = np.nextafter(f32(np.pi), f32(0))


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("acro")
    return {"O2": ac.build_driver(str(d / "ad_O2"), "-O2"), "O0": ac.build_driver(str(d / "ad_O0"), "-O0")}


def _corners():
    """Both speeds at +- their bounds x theta2 in {0, +-pi/2, -pi, the largest float below pi} x a in {+-1, +-1e30}"""
    rows = []
    for s1, s2 in itertools.product((1, -1), (1, -1)):
        for th2 in (0.0, np.pi / 2, -np.pi / 2, -np.pi, BELOW_PI):
            for a in (1.0, -1.0, 1e30, -1e30):
                rows.append([0.3, th2, s1 * ac.MAX_VEL_1, s2 * ac.MAX_VEL_2, a])
    return np.array(rows, f32)


def _step_inputs():
    rng = np.random.default_rng(11)
    n = N_RANDOM
    x = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-ac.MAX_VEL_1, ac.MAX_VEL_1, n),
                  rng.uniform(-ac.MAX_VEL_2, ac.MAX_VEL_2, n), rng.uniform(-1.5, 1.5, n)], 1).astype(f32)
    x = np.concatenate([x, _corners()]).astype(f32)
    x[:, :2] = np.clip(x[:, :2], -f32(np.pi), BELOW_PI)  # the fp32 rounding of +-pi stays inside [-pi, pi)
    return x


@pytest.fixture(scope="module")
def stepped(drivers, tmp_path_factory):
    """(inputs, the driver's outputs [n, 12], step_f64's outputs): computed once, not modified"""
    d = tmp_path_factory.mktemp("acro_step")
    x = _step_inputs()
    x.tofile(d / "x.f32")
    ac.run_driver(drivers["O2"], "step", d / "x.f32", d / "o.f32")
    o = np.fromfile(d / "o.f32", f32).reshape(-1, 12)
    assert len(o) == len(x)
    return x, o, ac.step_f64(x)


def test_one_step_against_float64(stepped):
    x, o, (s64, o64, margin, stage) = stepped
    assert len(_corners()) == 80 and np.abs(x[:, 4]).max() > 1e29
    ea = np.maximum(ac.circ_dist(o[:, 0], s64[:, 0]), ac.circ_dist(o[:, 1], s64[:, 1]))
    ev = np.abs(o[:, 2:4] - s64[:, 2:4])
    eo = np.abs(o[:, 4:10] - o64)
    m32 = -o[:, 4].astype(np.float64) - (o[:, 4].astype(np.float64) * o[:, 6] - o[:, 5].astype(np.float64) * o[:, 7]) - 1.0
    em = np.abs(m32 - margin)
    print(f"max err: angles {ea.max():.4e} (bound {ANGLE_BOUND:.4e}), speeds {ev.max():.4e} ({SPEED_BOUND:.4e}), "
          f"obs trig {eo[:, :4].max():.4e} ({TRIG_BOUND:.4e}), obs speeds {eo[:, 4:].max():.4e} ({SPEED_BOUND:.4e}), "
          f"termination margin {em.max():.4e} ({MARGIN_BOUND:.4e}); corners alone: angles {ea[N_RANDOM:].max():.4e}, "
          f"speeds {ev[N_RANDOM:].max():.4e}; largest |stage angle| {stage.max():.3f}")
    assert ea.max() <= ANGLE_BOUND and ev.max() <= SPEED_BOUND
    assert eo[:, :4].max() <= TRIG_BOUND and eo[:, 4:].max() <= SPEED_BOUND and em.max() <= MARGIN_BOUND
    # the stored state: angles in [-pi, pi), speeds within their bounds; the observation is that state's
    assert (o[:, :2] >= -f32(np.pi)).all() and (o[:, :2] < f32(np.pi)).all()
    assert (np.abs(o[:, 2]) <= f32(ac.MAX_VEL_1)).all() and (np.abs(o[:, 3]) <= f32(ac.MAX_VEL_2)).all()
    np.testing.assert_array_equal(o[:, 8:10], o[:, 2:4])
    assert (np.abs(o[:, 2]) == f32(ac.MAX_VEL_1)).any() and (np.abs(o[:, 3]) == f32(ac.MAX_VEL_2)).any()  # the clips act
    # the termination flag equals float64's wherever float64's margin is farther from 0 (the sum from
    # 1) than the bound; the cases left out are at most 1e-3 of the sample
    term, t64 = o[:, 11] != 0, margin > 0
    assert set(np.unique(o[:, 11]).tolist()) == {0.0, 1.0}
    near = np.abs(margin) <= MARGIN_BOUND
    print(f"near-threshold cases: {near.sum()} of {len(x)} ({near.mean():.2e})")
    assert near.mean() <= 1e-3 and near[:N_RANDOM].mean() <= 1e-3
    np.testing.assert_array_equal(term[~near], t64[~near])
    n_term, n_not = int((~near & t64).sum()), int((~near & ~t64).sum())
    print(f"compared: {n_term} terminations, {n_not} non-terminations ({n_term / (n_term + n_not):.2%} terminate)")
    assert n_term >= 0.1 * len(x) and n_not >= 0.1 * len(x)  # a substantial share of both outcomes
    # reward: 0 on a terminating step, -1 otherwise; so it equals float64's wherever the flags agree
    np.testing.assert_array_equal(o[:, 10], np.where(term, 0.0, -1.0).astype(f32))
    # a = +-1e30 is the clipped a = +-1
    c, oc = x[N_RANDOM:], o[N_RANDOM:]
    big = np.abs(c[:, 4]) > 1e29
    assert big.sum() == 40
    twin = c.copy()
    twin[:, 4] = np.sign(twin[:, 4])
    for row, o_big in zip(twin[big], oc[big]):
        k = np.nonzero((c == row).all(1))[0][0]
        np.testing.assert_array_equal(oc[k], o_big)


def test_reduce_and_sincos_over_twice_the_stage_range(stepped, drivers, tmp_path):
    """The range comes from the step test's own sample: twice its largest |stage angle|. Random
    arguments, and every multiple of pi in the range with its fp32 neighbours (where k = rint(x / 2 pi)
    is about to change)."""
    stage = stepped[2][3]
    print(f"largest |stage angle| {stage.max():.4f} rad (random {stage[:N_RANDOM].max():.4f}, corners {stage[N_RANDOM:].max():.4f})")
    assert 0.9 * STAGE_MEASURED <= stage.max() <= 1.001 * STAGE_MEASURED  # the figure the header and DESIGN.md quote
    R = 2 * stage.max()
    assert R > 60
    rng = np.random.default_rng(5)
    m = (np.arange(-int(R / np.pi), int(R / np.pi) + 1) * np.pi).astype(f32)
    xs = np.concatenate([rng.uniform(-R, R, 400000).astype(f32), m, np.nextafter(m, f32(1e9)), np.nextafter(m, f32(-1e9))])
    xs.tofile(tmp_path / "r.f32")
    ac.run_driver(drivers["O2"], "reduce", tmp_path / "r.f32", tmp_path / "ro.f32")
    r = np.fromfile(tmp_path / "ro.f32", f32).reshape(-1, 4)
    x64 = xs.astype(np.float64)
    er = ac.circ_dist(r[:, 0], ac.wrap_f64(x64)).max()
    ew = ac.circ_dist(r[:, 1], ac.wrap_f64(x64)).max()
    es, ecs = np.abs(r[:, 2] - np.sin(x64)).max(), np.abs(r[:, 3] - np.cos(x64)).max()
    over = np.abs(r[:, 0].astype(np.float64)).max() - np.pi
    print(f"|x| <= {R:.2f}: reduce {er:.4e}, reduce + wrap {ew:.4e}, sin {es:.4e}, cos {ecs:.4e}, |reduced| - pi <= {over:.2e}")
    assert er <= 2 * REDUCE_MEASURED and es <= 2 * SIN_MEASURED and ecs <= 2 * COS_MEASURED
    # pend_wrap adds one rounding at magnitude pi (half an ulp there is 1.2e-7)
    assert ew <= 2 * REDUCE_MEASURED + 2.4e-7
    assert over <= 0.4  # pend_wrap's and pend_sincos's domains hold with a wide margin
    assert (r[:, 1] >= -f32(np.pi)).all() and (r[:, 1] < f32(np.pi)).all()
    # inside one period the reduction is the identity
    inner = np.abs(xs) < 3.0
    np.testing.assert_array_equal(r[inner, 0], xs[inner])


def test_no_contraction_O0_equals_O2(drivers, tmp_path):
    _step_inputs()[::10].tofile(tmp_path / "s.f32")
    E, T = 3, 300
    np.random.default_rng(2).uniform(-1.5, 1.5, (T, E, 1)).astype(f32).tofile(tmp_path / "a.f32")
    outs = {}
    for k, exe in drivers.items():
        ac.run_driver(exe, "step", tmp_path / "s.f32", tmp_path / f"s_{k}.out")
        ac.run_driver(exe, "vecw", E, T, 3, 1, tmp_path / "a.f32", tmp_path / f"v_{k}.out", 0.99)
        ac.run_driver(exe, "pump", E, 300, 3, 1, tmp_path / f"b_{k}.out", tmp_path / f"ba_{k}.out")
        outs[k] = [(tmp_path / f"{n}_{k}.out").read_bytes() for n in ("s", "v", "b", "ba")]
    assert all(len(b) > 0 for b in outs["O2"])
    assert outs["O0"] == outs["O2"]


def test_reset_statistics(drivers, tmp_path):
    E, seed = 64, 9
    act = np.zeros((1, E, 1), f32)
    raw, o0, _ = ac.host_vec(drivers["O2"], tmp_path, E, 1, seed, "a", act)
    raw2, _, _ = ac.host_vec(drivers["O2"], tmp_path, E, 1, seed, "b", act)
    assert raw == raw2
    # 0.2 u - 0.1 in fp32 with u in (0, 1]: within [-0.1f, 0.1f]; the observation is (cos, sin, cos, sin, w1, w2)
    th1, th2 = np.arctan2(o0[:, 1], o0[:, 0]), np.arctan2(o0[:, 3], o0[:, 2])
    st = np.stack([th1, th2, o0[:, 4], o0[:, 5]], 1)
    assert (np.abs(o0[:, 4:]) <= f32(0.1)).all() and (np.abs(st[:, :2]) <= 0.1 + 1e-6).all()
    np.testing.assert_allclose(o0[:, 0] ** 2 + o0[:, 1] ** 2, 1.0, atol=5e-7)
    # uniform in +-0.1: standard deviation 0.2 / sqrt(12) = 0.0577, mean 0 (256 values: 3 sigma of the mean is 0.011)
    assert abs(st.mean()) < 0.011 and 0.05 < st.std() < 0.065
    assert (st.std(0) > 0.045).all()
    for i in (0, 1, 17, 63):  # env i is seeded seed + i
        _, oi, _ = ac.host_vec(drivers["O2"], tmp_path, 1, 1, seed + i, f"s{i}", act[:, :1])
        np.testing.assert_array_equal(oi[0], o0[i])
    assert len({o0[i].tobytes() for i in range(E)}) == E
    assert len(set(o0[:, 4:].reshape(-1).tolist())) == 2 * E  # draws of their own per env and slot


def test_desynchronisation_and_vector_semantics(drivers, tmp_path):
    """E = 37, 640 steps, reset seed 6, noise seed 1 (the first pair tried, kept): the driver's
    energy-pumping actions a = sign(theta2dot) + U(-0.5, 0.5), every ninth env the noise alone. The
    recorded actions replayed through vec give the same bytes: what the GPU tests replay.
    Measured: 177 terminations on 148 distinct steps in 33 envs, 4 truncations (envs 8, 17, 26, 35 at
    step 500), lone finishers 164 times within a 4-env group and 130 times within a 16-env group."""
    E, T = ac.DESYNC_E, ac.DESYNC_T
    assert E == 37 and T >= 600
    act, o0, s = ac.desync_run(drivers["O2"], tmp_path)
    assert act.shape == (T, E, 1) and act.min() < -1.4 and act.max() > 1.4  # beyond the action space: clip_actions acts
    _, o0b, sb = ac.host_vec(drivers["O2"], tmp_path, E, T, ac.DESYNC_SEED, "replay", act)
    np.testing.assert_array_equal(o0, o0b)
    for k in s:
        np.testing.assert_array_equal(s[k], sb[k], err_msg=k)
    c = ac.assert_desynchronised(s["term"], s["trunc"])
    print(c)
    assert c == {"terminations": 177, "termination_steps": 148, "truncations": 4, "envs_that_terminate": 33,
                 "lone_in_4": 164, "lone_in_16": 130}
    term, trunc = s["term"] != 0, s["trunc"] != 0
    assert not (term & trunc).any()
    # the envs that never swing up truncate on the 500th step, with return -500
    for e in (8, 17, 26, 35):
        assert not term[:, e].any() and np.nonzero(trunc[:, e])[0].tolist() == [499]
        assert s["rew"][499, e] == -1 and s["len"][499, e] == 500 and s["ret"][499, e] == -500
        assert s["rew"][500, e] == 0 and s["len"][500, e] == 0  # the reset step
    # a terminating step pays 0, ends an episode of return 1 - length, and the next step is the reset
    for t, e in zip(*np.nonzero(term)):
        assert s["rew"][t, e] == 0 and s["len"][t, e] >= 2 and s["ret"][t, e] == 1 - s["len"][t, e]
        ob = s["obs"][t, e].astype(np.float64)
        assert -ob[0] - (ob[0] * ob[2] - ob[1] * ob[3]) > 1.0 - 1e-6
        if t + 1 < T:
            assert s["rew"][t + 1, e] == 0 and not term[t + 1, e] and not trunc[t + 1, e] and s["len"][t + 1, e] == 0
            assert (np.abs(s["obs"][t + 1, e, 4:]) <= f32(0.1)).all() and s["obs"][t + 1, e, 0] > 0.99
    done = term | trunc
    after = np.zeros_like(done)
    after[1:] = done[:-1]
    np.testing.assert_array_equal(s["rew"][~done & ~after], -1.0)
    assert (s["len"][~done] == 0).all()


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
AC = b"AcrobotContinuous-v1"
for env_id, E, null_out in ((b"Walker2d-v5", 4, False), (None, 4, False), (AC, 0, False), (AC, -3, False), (AC, 4, True)):
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
    assert got[0][2].index(ac.ENV_ID) > got[0][2].index("QuadrotorHover-v0")  # the new id, after the old text


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
@pytest.mark.parametrize("flag", ["host_step_us", "straggler_us"])
def test_cli_refuses_host_cost_flags_with_acrobot(exe, flag):
    """--host_step_us / --straggler_us stand in for the physics of the MuJoCo envs the synthetic
    cheetah replaces: with AcrobotContinuous-v1 they are refused (ac: the flags apply to
    SyntheticCheetah-v0 only; ppo: no such flags, so its two cases show the flag parser, and
    test_cli_host_backend_knows_the_id is the check of that CLI)."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    r = subprocess.run([path, "--env_id", ac.ENV_ID, "--env_backend", "host", f"--{flag}", "5", "--num_envs", "2",
                        "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem", "t_acro_refuse"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, r.stdout[-500:]
    assert flag in r.stderr
    assert "Number of parameters" not in r.stdout  # refused before the agent was created
    if exe.startswith("ac"):
        assert "is not implemented" not in r.stderr  # refused for the flag, not for the id


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
def test_cli_host_backend_knows_the_id(exe):
    """The same command without the flag gets past the creation of the host envs: no "is not
    implemented" (the answer to an unknown id, whose list now names this id after the old ones).
    Without a GPU it then stops at the agent's creation; with one it trains its 8 steps."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    args = ["--env_backend", "host", "--num_envs", "2", "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem",
            "t_acro_known"]
    r = subprocess.run([path, "--env_id", ac.ENV_ID] + args, capture_output=True, text=True, timeout=120)
    assert "is not implemented" not in r.stderr and "needs MuJoCo" not in r.stderr, r.stderr[-500:]
    u = subprocess.run([path, "--env_id", "AcrobotContinuous-v0"] + args, capture_output=True, text=True, timeout=120)
    assert u.returncode != 0 and "is not implemented" in u.stderr
    assert u.stderr.index(ac.ENV_ID) > u.stderr.index("QuadrotorHover-v0")


def test_binding_declares_the_env_id():
    import ppo_amd
    assert ppo_amd.ENV_DIMS[ac.ENV_ID] == (6, 1, -1.0, 1.0)
    assert ppo_amd.PSYN_ACROBOT == 5 and ac.ENV_ID in ppo_amd.DEVICE_ENV_KINDS
    assert ppo_amd.DEVICE_ENV_KINDS[-1] == "ReacherPlanar-v0"  # new ids go before the last entry
    cfg = ppo_amd.ACPPOConfig(env_id=ac.ENV_ID)
    h = ppo_amd.hip_config(cfg)
    assert (h.obs_dim, h.act_dim) == (6, 1)
    L = ppo_amd.agent_layout(ppo_amd.PPO_NET_LN_BETA, 6, 1, 256)
    p = ppo_amd.init_params(L, seed=1, env_id=ac.ENV_ID)
    assert p[L.hi] == 1.0 and p[L.lo] == -1.0
    assert (p[L.omean:L.omean + 6] == 0).all() and (p[L.ostd:L.ostd + 6] == 1).all()  # no table: the identity


def test_learning_fixture():
    """The rule of this task: every untrained return is -500 (the mean-action policy never swings up),
    so the spread is 0 and every seed must improve by at least 50, a tenth of the return range. The PPO
    agent's reference meets it. The AC agent's does not in any config tried (its sampled actions never
    swing up, so it never sees a reward other than -1): it ships without a learning test
    and without a reference file."""
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "acrobot", "learning_ref.json")))
    assert ref["env_id"] == ac.ENV_ID and ref["condition_met"] is True and ref["required_improvement"] == 50.0
    assert ref["config"]["agent"] == "ppo" and ref["seeds"] == [1, 2, 3] and len(ref["runs"]) == 3
    assert ref["eval_episodes"] == 64
    for r, seed in zip(ref["runs"], ref["seeds"]):
        assert r["seed"] == seed and r["untrained"] == -500.0 and r["eval_episodes"] >= 64
        assert r["trained"] - r["untrained"] >= 50.0
    for k in ("num_envs", "num_steps", "total_timesteps", "num_minibatches", "update_epochs", "learning_rate", "gamma"):
        assert k in ref["config"]
    assert not os.path.exists(os.path.join(ROOT, "tests", "golden", "acrobot", "learning_ref_ac.json"))


@pytest.mark.parametrize("agent,kind,H", [("ppo", 0, 64), ("ac", 1, 256)])
def test_swing_up_parameter_fixtures(agent, kind, H):
    """tests/golden/acrobot/params_{ppo,ac}.npy (scripts/acrobot_learning_ref.py --agent ppo --params_at 16
    and --clone_pump 6): policies whose sampled actions swing up, for the GPU comparisons of the rollout
    and evaluation kernels. Here: the size fits the agent's layout, and over the host env the oracle's
    sampled actions (the AC agent's mean actions too) end episodes by termination on several distinct
    steps within 240 steps, long before truncation."""
    import oracle_lib as O
    import ppo_amd
    assert (ppo_amd.PPO_NET_TANH_NORMAL, ppo_amd.PPO_NET_LN_BETA)[kind] == kind
    L = O.layout_init(kind, ac.OD, ac.AD, H)
    p = np.load(os.path.join(ROOT, "tests", "golden", "acrobot", f"params_{agent}.npy")).astype(np.float32)
    assert p.size == L.P == ppo_amd.agent_layout(kind, ac.OD, ac.AD, H).P and np.isfinite(p).all()
    E, T = 16, 240
    for mode in ((0, 2) if agent == "ac" else (0,)):  # the oracle's numbering: 0 sample, 2 mean
        env = ac.HostAcrobot(E)
        wrap = O.VecWrappers(E, ac.OD, 0.99) if agent == "ppo" else None
        obs = env.reset(1)
        obs = wrap.reset(obs) if wrap else obs
        terms, was_done = np.zeros((T, E), bool), np.zeros(E, np.float32)
        for t in range(T):
            a, _, _, _ = O.get_action_and_value(L, p, obs, mode, seed=1, rank=0, env_base=0, step_id=t)
            obs, rew, term, done, _, _ = env.step(a)
            if wrap:
                obs, _ = wrap.step(obs, rew, term, was_done)
            was_done = done
            terms[t] = term != 0
        env.close()
        print(f"{agent} mode {mode}: {terms.sum()} terminations on {terms.any(1).sum()} steps, first at {np.nonzero(terms.any(1))[0][:1]}")
        assert terms.sum() >= E // 2 and terms.any(1).sum() >= 5 and terms.any(0).sum() >= E // 2
