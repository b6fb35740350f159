"""QuadrotorHover-v0 on the host: the shared arithmetic of include/ppo_quadrotor.h and the host env
gymcpp/quadrotor.h, through tests/native/quadrotor_driver.cpp (built here with g++
-ffp-contract=off). The env is the textbook Newton-Euler quadrotor in "+" configuration hovering at
the origin (O = 18, A = 4, it terminates when |p|^2 > 9 and truncates after 500 steps); the task is
the project's own.

  1. one teacher-forced step against the float64 restatement quadrotor_common.step_f64, per output
     group: p, v, q (up to sign), omega, each observation group, the reward and |p'|^2;
  2. the termination flag against float64 wherever float64's |p'|^2 is farther from 9 than the bound,
     and the threshold corners exactly as the fp32 comparison;
  3. the driver built at -O0 and at -O2 writes the same bytes;
  4. reset: ranges, |q| = 1, twelve uniforms;
  5. invariants over 10^4 random steps: |q|, R orthonormal, |omega_i| <= 32, reward in (0, 3];
  6. SeqVectorEnv + RecordEpisodeStatistics semantics: next-step autoreset, termination mid-batch,
     truncation at 500 under a scripted float64 PD controller;
  7. the four action dimensions are not interchangeable;
  8. the refusals of psyn_create_env and of the CLIs happen before any HIP call;
  9. the learning fixtures carry their condition, config, seeds and runs;
 10. the desynchronisation condition every GPU comparison starts from.

The bounds of 1 are twice the maximum errors measured on the CPU over the inputs of _step_inputs()
against step_f64 (`pytest tests/test_quadrotor_cpu.py -k float64 -s` prints them):
p 2.4221e-7 (half an fp32 ulp of 4 is 2.4e-7), v 9.7385e-7 (half an ulp of 16 is 9.5e-7), q up to
sign 1.5428e-7, omega 3.2055e-6 (half an ulp of 32 is 1.9e-6; the gyroscopic term
(I_zz - I_yy) w_y w_z / I_xx reaches 1024 rad/s^2), reward 2.0905e-7, |p'|^2 3.5306e-6 (an ulp of 32
is 3.8e-6), observation: p 2.4221e-7, R 6.9828e-7 (R doubles the quaternion's products), v 9.7385e-7,
omega 3.2055e-6. Over 10^4 random steps | |q| - 1 | reaches 1.4823e-7 and | R R^T - I | 1.1246e-6.

The desynchronised run (E = 37, seed 5, actions uniform in [-1.5, 1.5]^4, 300 steps; the counts are
asserted in test_desynchronisation and recorded in DESIGN.md §7): 182 episodes end on 128 distinct
steps, every env finishes 4 to 6 episodes, a 4-env group has a lone finisher on 172 (step, group)
pairs and a 16-env group on 136."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import quadrotor_common as qc

ROOT = qc.ROOT
# measured maxima (this file's docstring); the bounds are twice these
MEASURED = {"p": 2.4221e-7, "v": 9.7385e-7, "q": 1.5428e-7, "omega": 3.2055e-6, "reward": 2.0905e-7, "p2": 3.5306e-6,
            "obs_p": 2.4221e-7, "obs_R": 6.9828e-7, "obs_v": 9.7385e-7, "obs_omega": 3.2055e-6}
BOUND = {k: 2 * v for k, v in MEASURED.items()}
# | |q| - 1 | and | R R^T - I | over the 10^4 random steps of test_invariants_over_random_steps: measured
MEASURED_NORM, MEASURED_ORTHO = 1.4823e-7, 1.1246e-6
N_RANDOM = 100000
f32 = np.float32


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("quad")
    return {"O2": qc.build_driver(str(d / "qd_O2"), "-O2"), "O0": qc.build_driver(str(d / "qd_O0"), "-O0")}


HALF_TURNS = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
ACT_CORNERS = [(1, 1, 1, 1), (-1, -1, -1, -1), (1e30, 1e30, 1e30, 1e30), (-1e30, -1e30, -1e30, -1e30), (1, -1, 1, -1),
               (-1, 1, 1e30, -1e30), (1e30, -1, -1e30, 1), (0.25, -0.75, 1, -1e30)]


def _corners():
    """omega at +-32 x q at the identity and the three half-turns x actions at +-1 and +-1e30, mixed
    per dimension."""
    rows = []
    for q in HALF_TURNS:
        for w in ((32, 32, 32), (-32, -32, -32), (32, -32, 32), (-32, 32, -32)):
            for a in ACT_CORNERS:
                rows.append([0.5, -0.25, 1.0, 1.0, -2.0, 0.5, *q, *w, *a])
    return np.array(rows, f32)


def _threshold_corners():
    """|p|^2 at 9 and one ulp either side, along each axis in both directions, at rest in exact hover
    (v = 0, q the identity, omega = 0, a = 0: F = g exactly, so p' = p bit for bit)."""
    rows = []
    for ax in range(3):
        for sg in (1, -1):
            for x in (np.nextafter(f32(3), f32(0)), f32(3), np.nextafter(f32(3), f32(4))):
                r = np.zeros(17, f32)
                r[ax] = sg * x
                r[6] = 1
                rows.append(r)
    return np.array(rows, f32)


def _step_inputs():
    rng = np.random.default_rng(11)
    n = N_RANDOM
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x = np.concatenate([rng.uniform(-3.5, 3.5, (n, 3)), rng.uniform(-12, 12, (n, 3)), q, rng.uniform(-32, 32, (n, 3)),
                        rng.uniform(-1.5, 1.5, (n, 4))], 1)
    return np.concatenate([x.astype(f32), _corners(), _threshold_corners()]).astype(f32)


def step_errors(x, s, rew, obs):
    """largest error per output group against step_f64, and float64's |p'|^2"""
    s64, r64, p2_64, o64 = qc.step_f64(x)
    qe = np.minimum(np.abs(s[:, 6:10] - s64[:, 6:10]).max(1), np.abs(s[:, 6:10] + s64[:, 6:10]).max(1))
    s_ = s.astype(np.float64)
    p2 = (s_[:, :3] ** 2).sum(1)
    err = {"p": np.abs(s[:, 0:3] - s64[:, 0:3]).max(), "v": np.abs(s[:, 3:6] - s64[:, 3:6]).max(), "q": qe.max(),
           "omega": np.abs(s[:, 10:13] - s64[:, 10:13]).max(), "reward": np.abs(rew - r64).max(),
           "p2": np.abs(p2 - p2_64).max(),
           "obs_p": np.abs(obs[:, 0:3] - o64[:, 0:3]).max(), "obs_R": np.abs(obs[:, 3:12] - o64[:, 3:12]).max(),
           "obs_v": np.abs(obs[:, 12:15] - o64[:, 12:15]).max(), "obs_omega": np.abs(obs[:, 15:18] - o64[:, 15:18]).max()}
    return {k: float(v) for k, v in err.items()}, p2_64


def test_one_step_against_float64(drivers, tmp_path):
    x = _step_inputs()
    r = x[:N_RANDOM]
    assert np.abs(r[:, :3]).max() <= 3.5 and np.abs(r[:, 3:6]).max() <= 12 and np.abs(r[:, 10:13]).max() <= 32
    assert np.abs(r[:, 13:]).max() <= 1.5 and np.abs(np.linalg.norm(r[:, 6:10].astype(np.float64), axis=1) - 1).max() < 2e-7
    s, rew, term, obs = qc.host_step(drivers["O2"], tmp_path, x)
    err, _ = step_errors(x, s, rew, obs)
    print({k: f"{v:.4e}" for k, v in err.items()})
    print("bounds", {k: f"{v:.4e}" for k, v in BOUND.items()})
    for k in BOUND:
        assert err[k] <= BOUND[k], (k, err[k], BOUND[k])
    # the observation is the new state: p, v, omega bit for bit
    np.testing.assert_array_equal(obs[:, 0:3].view(np.uint32), s[:, 0:3].view(np.uint32))
    np.testing.assert_array_equal(obs[:, 12:15].view(np.uint32), s[:, 3:6].view(np.uint32))
    np.testing.assert_array_equal(obs[:, 15:18].view(np.uint32), s[:, 10:13].view(np.uint32))
    assert np.abs(s[:, 10:13]).max() <= 32 and np.isfinite(s).all() and np.isfinite(obs).all()
    # a = +-1e30 is the clipped a = +-1
    c = x[N_RANDOM:N_RANDOM + len(_corners())]
    big = (np.abs(c[:, 13:]) > 1e29).any(1)
    assert big.sum() >= 64
    twin = c[big].copy()
    twin[:, 13:] = np.clip(twin[:, 13:], -1, 1)
    ts, tr, tt, to = qc.host_step(drivers["O2"], tmp_path, twin, "twin")
    sl = slice(N_RANDOM, N_RANDOM + len(c))
    np.testing.assert_array_equal(ts.view(np.uint32), s[sl][big].view(np.uint32))
    np.testing.assert_array_equal(tr.view(np.uint32), rew[sl][big].view(np.uint32))
    np.testing.assert_array_equal(to.view(np.uint32), obs[sl][big].view(np.uint32))
    # a NaN action is a = -1 (fmaxf(NaN, -1) = -1)
    nan = c[:8].copy()
    nan[:, 13] = np.nan
    ref = nan.copy()
    ref[:, 13] = -1
    ns, nr, _, _ = qc.host_step(drivers["O2"], tmp_path, nan, "nan")
    rs, rr, _, _ = qc.host_step(drivers["O2"], tmp_path, ref, "nanref")
    np.testing.assert_array_equal(ns.view(np.uint32), rs.view(np.uint32))
    np.testing.assert_array_equal(nr.view(np.uint32), rr.view(np.uint32))


def test_termination_flag_against_float64(drivers, tmp_path):
    x = _step_inputs()
    s, rew, term, obs = qc.host_step(drivers["O2"], tmp_path, x)
    assert set(np.unique(term).tolist()) <= {0.0, 1.0}
    _, p2_64 = step_errors(x, s, rew, obs)
    n = N_RANDOM + len(_corners())
    near = np.abs(p2_64[:n] - 9.0) <= BOUND["p2"]
    print(f"left out: {int(near.sum())} of {n} (float64 |p'|^2 within {BOUND['p2']:.4e} of 9); terminated: {int(term[:n].sum())}")
    assert near.sum() <= 1e-3 * n
    assert near.sum() == 0  # the count for these inputs
    np.testing.assert_array_equal(term[:n][~near], (p2_64[:n][~near] > 9.0).astype(f32))
    assert 0.3 < term[:N_RANDOM].mean() < 0.9  # both answers are well represented
    # the threshold corners: exact hover leaves p where it was, and the flag is the fp32 comparison
    tc, ts, tt = x[n:], s[n:], term[n:]
    np.testing.assert_array_equal(ts.view(np.uint32), tc[:, :13].view(np.uint32))
    p = ts[:, :3]
    p2_32 = (p[:, 0] * p[:, 0] + (p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])).astype(f32)  # one nonzero term: exact order
    np.testing.assert_array_equal(tt, (p2_32 > f32(9)).astype(f32))
    np.testing.assert_array_equal(tt.reshape(6, 3), np.tile(np.array([0, 0, 1], f32), (6, 1)))
    # the reward is given on the terminating step too
    assert (rew[n:] > 0).all() and (rew[:n][term[:n] == 1] > 0).all()


def test_no_contraction_O0_equals_O2(drivers, tmp_path):
    _step_inputs().tofile(tmp_path / "s.f32")
    E, T = 3, 200
    np.random.default_rng(2).uniform(-1.5, 1.5, (T, E, 4)).astype(f32).tofile(tmp_path / "a.f32")
    outs = {}
    for k, exe in drivers.items():
        qc.run_driver(exe, "step", tmp_path / "s.f32", tmp_path / f"s_{k}.out")
        qc.run_driver(exe, "vecw", E, T, 3, 1, tmp_path / "a.f32", tmp_path / f"v_{k}.out", 0.99)
        qc.run_driver(exe, "reset", 5, 100, tmp_path / f"r_{k}.out")
        outs[k] = [(tmp_path / f"{n}_{k}.out").read_bytes() for n in "svr"]
    assert all(len(b) > 0 for b in outs["O2"])
    assert outs["O0"] == outs["O2"]


def test_reset_ranges_unit_quaternion_and_twelve_uniforms(drivers, tmp_path):
    E, seed = 64, 9
    act = np.zeros((1, E, 4), f32)
    raw, o0, _ = qc.host_vec(drivers["O2"], tmp_path, E, 1, seed, "a", act)
    raw2, _, _ = qc.host_vec(drivers["O2"], tmp_path, E, 1, seed, "b", act)
    assert raw == raw2
    for i in (0, 1, 17, 63):  # env i is seeded seed + i
        _, oi, _ = qc.host_vec(drivers["O2"], tmp_path, 1, 1, seed + i, f"s{i}", act[:, :1])
        np.testing.assert_array_equal(oi[0], o0[i])
    assert len({o0[i].tobytes() for i in range(E)}) == E
    n = 10000
    qc.run_driver(drivers["O2"], "reset", 7, n, tmp_path / "r.out")
    s = np.fromfile(tmp_path / "r.out", f32).reshape(n, qc.SD)
    assert np.abs(s[:, 0:3]).max() <= 1 and s[:, 0:3].std() > 0.5
    assert np.abs(s[:, 3:6]).max() <= 0.5 and s[:, 3:6].std() > 0.25
    assert np.abs(s[:, 10:13]).max() <= 0.5 and s[:, 10:13].std() > 0.25
    qn = np.linalg.norm(s[:, 6:10].astype(np.float64), axis=1)
    assert np.abs(qn - 1).max() <= 2 * MEASURED_NORM, np.abs(qn - 1).max()
    e = s[:, 7:10].astype(np.float64) / s[:, 6:7]  # q = normalise(1, e)
    assert np.abs(e).max() <= 0.2 + 1e-6 and e.std() > 0.1 and (s[:, 6] > 0.94).all()
    # the observation of a reset state
    _, o1, _ = qc.host_vec(drivers["O2"], tmp_path, 1, 1, 7, "one", act[:, :1])
    np.testing.assert_allclose(o1, qc.obs_f64(s[:1].astype(np.float64)), rtol=0, atol=5e-7)
    # quad_reset reads twelve uniforms, in the order p, v, e, omega: each output group follows its own
    # three draws and no other
    u = np.random.default_rng(3).uniform(0.01, 1, (50, 12)).astype(f32)
    u.tofile(tmp_path / "u.f32")
    qc.run_driver(drivers["O2"], "draws", tmp_path / "u.f32", tmp_path / "d.out")
    base = np.fromfile(tmp_path / "d.out", f32).reshape(50, qc.SD)
    groups = {0: [0], 1: [1], 2: [2], 3: [3], 4: [4], 5: [5], 6: [6, 7, 8, 9], 7: [6, 7, 8, 9], 8: [6, 7, 8, 9],
              9: [10], 10: [11], 11: [12]}
    for k, cols in groups.items():
        v = u.copy()
        v[:, k] = np.where(u[:, k] < 0.5, u[:, k] + 0.25, u[:, k] - 0.25)
        v.tofile(tmp_path / "u2.f32")
        qc.run_driver(drivers["O2"], "draws", tmp_path / "u2.f32", tmp_path / "d2.out")
        d = np.fromfile(tmp_path / "d2.out", f32).reshape(50, qc.SD)
        changed = sorted(set(np.nonzero((d != base).any(0))[0].tolist()))
        assert changed == cols, (k, changed)
    np.testing.assert_allclose(base[:, 0:3], 2.0 * u[:, 0:3].astype(np.float64) - 1, rtol=0, atol=1.2e-7)
    np.testing.assert_allclose(base[:, 3:6], u[:, 3:6].astype(np.float64) - 0.5, rtol=0, atol=6e-8)
    np.testing.assert_allclose(base[:, 10:13], u[:, 9:12].astype(np.float64) - 0.5, rtol=0, atol=6e-8)
    # the env's thirteenth uniform does not exist: two resets of one env differ in every state value
    assert (s[0] != s[1]).all()


def test_invariants_over_random_steps(drivers, tmp_path):
    x = _step_inputs()[:10000]
    s, rew, term, obs = qc.host_step(drivers["O2"], tmp_path, x)
    qn = np.linalg.norm(s[:, 6:10].astype(np.float64), axis=1)
    R = obs[:, 3:12].astype(np.float64).reshape(-1, 3, 3)
    ortho = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
    print(f"| |q| - 1 | max {np.abs(qn - 1).max():.4e} (bound {2 * MEASURED_NORM:.4e}); R R^T - I max {ortho:.4e} "
          f"(bound {2 * MEASURED_ORTHO:.4e}); reward in [{rew.min():.4e}, {rew.max():.6f}]")
    assert np.abs(qn - 1).max() <= 2 * MEASURED_NORM
    assert ortho <= 2 * MEASURED_ORTHO
    assert np.abs(np.linalg.det(R) - 1).max() <= 6 * MEASURED_ORTHO  # a rotation, not a reflection
    assert np.abs(s[:, 10:13]).max() <= 32
    assert (rew > 0).all() and (rew <= 3).all()
    # r = 3 exactly at the goal state: p = 0, upright, at rest, hovering
    g = np.zeros((1, 17), f32)
    g[0, 6] = 1
    gs, gr, gt, _ = qc.host_step(drivers["O2"], tmp_path, g, "goal")
    assert gr[0] == 3.0 and gt[0] == 0.0
    np.testing.assert_array_equal(gs.view(np.uint32), g[:, :13].view(np.uint32))


def test_vector_semantics_autoreset_and_termination(drivers, tmp_path):
    E, T, seed = 5, 300, 9
    act = np.random.default_rng(4).uniform(-1.5, 1.5, (T, E, 4)).astype(f32)
    _, o0, s = qc.host_vec(drivers["O2"], tmp_path, E, T, seed, "a", act)
    assert not s["trunc"].any() and s["term"].sum() >= 2 * E
    ends = [np.nonzero(s["term"][:, e])[0] for e in range(E)]
    assert len({int(t) for en in ends for t in en}) > E  # mid-batch: the envs end on steps of their own
    for e in range(E):
        t0 = 0
        for t in ends[e]:
            # the terminating step: |p|^2 > 9 on the observation it returns, its reward is given
            p = s["obs"][t, e, :3]
            assert f32(p[0] * p[0] + (p[1] * p[1] + p[2] * p[2])) > 8.99999 and s["rew"][t, e] > 0
            assert s["len"][t, e] == t - t0 + 1
            ret = f32(0)
            for k in range(t0, t + 1):  # RecordEpisodeStatistics adds in fp32, step by step
                ret = f32(ret + s["rew"][k, e])
            assert s["ret"][t, e] == ret
            if t + 1 < T:  # the next step is the reset: reward 0, done 0, a fresh state
                assert s["rew"][t + 1, e] == 0 and s["term"][t + 1, e] == 0 and s["len"][t + 1, e] == 0
                assert np.abs(s["obs"][t + 1, e, :3]).max() <= 1 and np.abs(s["obs"][t + 1, e, 12:]).max() <= 0.5
            t0 = t + 2
        inside = np.ones(T, bool)
        inside[ends[e]] = False
        inside[[t + 1 for t in ends[e] if t + 1 < T]] = False
        assert (s["len"][inside, e] == 0).all() and (s["rew"][inside, e] > 0).all()


def test_truncation_at_500_under_the_pd_controller():
    E, seed, T = 8, 21, 503
    acts, steps = qc.pd_prefix_actions(E, seed, T)
    assert np.abs(acts).max() <= 1
    term = np.stack([r[2] for r in steps])
    done = np.stack([r[3] for r in steps])
    ret = np.stack([r[4] for r in steps])
    ln = np.stack([r[5] for r in steps])
    rew = np.stack([r[1] for r in steps])
    assert not term.any()
    assert sorted(set(np.nonzero(done)[0].tolist())) == [499]  # the 500th step, every env; reset on the 501st
    assert (ln[499] == 500).all() and (done[499] == 1).all()
    print("PD controller returns", ret[499])
    assert (ret[499] > 1000).all()  # it hovers: the reward approaches 3 per step
    assert (rew[500] == 0).all() and (ln[500] == 0).all() and (rew[501] > 0).all()


def test_action_dimensions_are_not_interchangeable(drivers, tmp_path):
    x = _step_inputs()[:64].copy()
    rng = np.random.default_rng(8)
    x[:, 13:] = rng.uniform(-1, 1, (64, 4))
    x[:, 10:13] = rng.uniform(-2, 2, (64, 3))  # away from the rate clip, which would hide a torque
    a = x[:, 13:]
    sx, _, _, _ = qc.host_step(drivers["O2"], tmp_path, x, "x")
    for i in range(4):
        for j in range(i + 1, 4):
            assert (np.abs(a[:, i] - a[:, j]) > 1e-4).all()
            y = x.copy()
            y[:, 13 + i], y[:, 13 + j] = x[:, 13 + j], x[:, 13 + i]
            sy, _, _, _ = qc.host_step(drivers["O2"], tmp_path, y, f"y{i}{j}")
            assert (sx[:, 10:13] != sy[:, 10:13]).any(1).all(), (i, j)  # another torque
    # each rotor alone changes the step, and differently from every other
    outs = []
    for i in range(4):
        z = x.copy()
        z[:, 13:] = -1
        z[:, 13 + i] = 1
        outs.append(qc.host_step(drivers["O2"], tmp_path, z, f"z{i}")[0])
    for i in range(4):
        for j in range(i + 1, 4):
            assert (outs[i][:, 10:13] != outs[j][:, 10:13]).any(1).all()


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
QH = b"QuadrotorHover-v0"
for env_id, E, null_out in ((b"Walker2d-v5", 4, False), (None, 4, False), (QH, 0, False), (QH, -3, False), (QH, 4, True)):
    h = ctypes.c_void_p()
    rc = lib.psyn_create_env(env_id, E, None if null_out else ctypes.byref(h))
    out.append([rc, bool(h.value), lib.ppo_last_error().decode()])
print(json.dumps(out))
'''
    res = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "ppo.cpp_amd")], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    old = "unknown env_id Walker2d-v5 (Pendulum-v1, SyntheticCheetah-v0), CartPoleContinuous-v1, ReacherPlanar-v0"
    want = [old, "null argument", "num_envs must be positive", "num_envs must be positive", "null argument"]
    assert len(got) == len(want)
    for (rc_, made, msg), w in zip(got, want):
        assert rc_ == -1 and not made and w in msg, (rc_, made, msg, w)
    assert got[0][2].index(qc.ENV_ID) > got[0][2].index(old)  # the new id, after the old text


@pytest.mark.parametrize("exe", ["ac_ppo_continuous_action", "ppo_continuous_action"])
@pytest.mark.parametrize("flag", ["host_step_us", "straggler_us"])
def test_cli_refuses_host_step_us_with_quadrotor(exe, flag):
    """--host_step_us / --straggler_us stand in for the physics of the MuJoCo envs the synthetic
    cheetah replaces: with QuadrotorHover-v0 they are refused (ac: the flags apply to
    SyntheticCheetah-v0 only, a refusal that needs the host env of this id to exist; ppo: no such flags,
    so its two cases show the flag parser: test_cli_host_backend_knows_the_id is the check of that CLI)."""
    path = os.path.join(ROOT, "ppo.cpp_amd", "bin", exe)
    r = subprocess.run([path, "--env_id", qc.ENV_ID, "--env_backend", "host", f"--{flag}", "5", "--num_envs", "2",
                        "--num_steps", "4", "--total_timesteps", "8", "--exp_name_stem", "t_quad_refuse"],
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
            "t_quad_known"]
    r = subprocess.run([path, "--env_id", qc.ENV_ID] + args, capture_output=True, text=True, timeout=120)
    assert "is not implemented" not in r.stderr and "needs MuJoCo" not in r.stderr, r.stderr[-500:]
    u = subprocess.run([path, "--env_id", "QuadrotorHover-v1"] + args, capture_output=True, text=True, timeout=120)
    assert u.returncode != 0 and "is not implemented" in u.stderr and qc.ENV_ID in u.stderr
    assert u.stderr.index(qc.ENV_ID) > u.stderr.index("ReacherPlanar-v0")


def test_binding_declares_the_env_id():
    import ppo_amd
    assert ppo_amd.ENV_DIMS[qc.ENV_ID] == (18, 4, -1.0, 1.0)
    assert ppo_amd.PSYN_QUADROTOR == 4 and qc.ENV_ID in ppo_amd.DEVICE_ENV_KINDS
    assert ppo_amd.obs_norm(qc.ENV_ID) is None  # answered as CartPoleContinuous-v1 is: n = 0, identity
    cfg = ppo_amd.ACPPOConfig(env_id=qc.ENV_ID)
    h = ppo_amd.hip_config(cfg)
    assert (h.obs_dim, h.act_dim) == (18, 4)
    L = ppo_amd.agent_layout(ppo_amd.PPO_NET_LN_BETA, 18, 4, 256)
    p = ppo_amd.init_params(L, seed=1, env_id=qc.ENV_ID)
    assert p[L.hi] == 1.0 and p[L.lo] == -1.0
    assert (p[L.omean:L.omean + 18] == 0).all() and (p[L.ostd:L.ostd + 18] == 1).all()


@pytest.mark.parametrize("name,agent", [("learning_ref.json", "ppo"), ("learning_ref_ac.json", "ac")])
def test_learning_fixture(name, agent):
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "quadrotor", name)))
    assert ref["env_id"] == qc.ENV_ID and ref["condition_met"] is True
    assert ref["config"]["agent"] == agent and len(ref["seeds"]) == 3 and len(ref["runs"]) == 3
    un = [r["untrained"] for r in ref["runs"]]
    spread = max(un) - min(un)
    for r, seed in zip(ref["runs"], ref["seeds"]):
        assert r["seed"] == seed and r["trained"] - r["untrained"] >= 2 * spread
    for k in ("num_envs", "num_steps", "total_timesteps", "num_minibatches", "update_epochs", "learning_rate", "gamma"):
        assert k in ref["config"]


def desync_counts(term, trunc):
    """(episodes, distinct end steps, fewest and most episodes per env, lone finishers per 4-env and per
    16-env group) of a [T, E] run"""
    done = (term != 0) | (trunc != 0)
    T, E = done.shape
    lone = {}
    for g in (4, 16):
        lone[g] = sum(int(done[t, b:b + g].sum() == 1) for t in range(T) for b in range(0, E, g))
    per_env = done.sum(0)
    return int(done.sum()), int(done.any(1).sum()), int(per_env.min()), int(per_env.max()), lone[4], lone[16]


def test_desynchronisation(drivers, tmp_path):
    """The condition every GPU comparison of tests/test_gpu_quadrotor.py starts from: E = 37, the fixed
    seed, actions uniform in [-1.5, 1.5]^4, 300 steps."""
    E, T = qc.GPU_E, qc.GPU_T
    act = qc.gpu_actions()
    assert act.shape == (T, E, 4) and act.min() < -1.4 and act.max() > 1.4
    _, _, s = qc.host_vec(drivers["O2"], tmp_path, E, T, qc.GPU_SEED, "d", act)
    counts = desync_counts(s["term"], s["trunc"])
    print("episodes, distinct end steps, min / max per env, lone finishers per 4-group, per 16-group:", counts)
    episodes, distinct, lo, hi, lone4, lone16 = counts
    assert distinct >= 50            # episodes end on many distinct steps
    assert lo >= 2                   # every env finishes at least two episodes
    assert lone4 >= 1 and lone16 >= 1  # an env of a 4-env group, and one of a 16-env group, finishes alone on its step
    assert counts == (182, 128, 4, 6, 172, 136)  # the recorded counts of this seed
