"""GPU tests of the CaRL act lanes (ppo_carla_lane_*: one host thread, one stream and one private set of
the forward's buffers per env; include/ppo_carla.h "act lanes") and of k_carla_lane_in through its hook.

Everything here is an exact comparison. k_carla_lane_in moves floats (numpy is the reference, compared
as bit patterns). A lane act runs the kernels of ppo_carla_rollout_act(step, env, env + 1) — the same
launches on one row with the same sampling keys, none of them with atomics — on its own buffers, so a
collection through lanes equals the serial one bit for bit whatever the interleaving, and so do GAE and
the training that follow. A forward buffer shared by two lanes would show as a difference.

Sizes: T = 3 steps, E = 3 envs, 1 epoch of 3 minibatches (3 rows each)."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

T, E = 3, 3
STORED = ("bev", "meas", "vmeas", "dones", "actions", "logp", "values", "rewards")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# k_carla_lane_in
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nm,nv", [(8, 3), (1, 0), (31, 31), (40, 30)])  # 70 floats: past the 62 of the argument block
@pytest.mark.parametrize("step,env", [(0, 0), (1, 2)])
def test_lane_in_matches_numpy(nm, nv, step, env):
    ppo_amd.set_device(0)
    rng = np.random.default_rng(100 * nm + nv + 7 * step + env)
    t, e = 2, 3
    row = step * e + env
    # every bit pattern travels unchanged, NaNs and denormals included
    meas = rng.integers(0, 2**32, nm, dtype=np.uint32).view(np.float32)
    vmeas = rng.integers(0, 2**32, nv, dtype=np.uint32).view(np.float32)
    done, reward = 1.0, float(np.float32(rng.standard_normal()))
    host = dict(meas=np.full((t, e, nm), -7.0, np.float32), vmeas=np.full((t, e, max(nv, 1)), -7.0, np.float32),
                dones=np.full((t, e), -7.0, np.float32), rewards=np.full((t, e), -7.0, np.float32))
    dev = {k: DeviceArray.from_numpy(v) for k, v in host.items()}
    ppo_amd.carla_lane_in(meas, vmeas, done, reward, dev["meas"].ptr + 4 * row * nm,
                          dev["vmeas"].ptr + 4 * row * nv if nv else None, dev["dones"].ptr + 4 * row,
                          dev["rewards"].ptr + 4 * row)
    ref = {k: v.copy() for k, v in host.items()}
    ref["meas"].reshape(t * e, nm)[row] = meas
    if nv:
        ref["vmeas"].reshape(t * e, nv)[row] = vmeas
    ref["dones"].reshape(-1)[row] = done
    ref["rewards"].reshape(-1)[row] = np.float32(reward)
    for k in host:  # the row, and every neighbouring row untouched
        np.testing.assert_array_equal(_bits(dev[k].numpy()), _bits(ref[k]), err_msg=k)
    # a reward alone (ppo_carla_lane_reward's launch): nothing else moves
    ppo_amd.carla_lane_in(np.zeros(0, np.float32), np.zeros(0, np.float32), 0.0, 0.25, reward_row=dev["rewards"].ptr + 4 * row)
    ref["rewards"].reshape(-1)[row] = 0.25
    for k in host:
        np.testing.assert_array_equal(_bits(dev[k].numpy()), _bits(ref[k]), err_msg=k)
    for d in dev.values():
        d.free()


# ------------------------------------------------------------------------------------------------
# lanes against serial acts
# ------------------------------------------------------------------------------------------------
def _params(L, seed):
    """uniform +-1 / sqrt(fan_in) weights and biases, LayerNorm weights near 1, action space [-1, 1]"""
    rng = np.random.default_rng(seed)
    p = np.zeros(L.P, np.float32)
    gammas = set(list(L.conv_g) + list(L.lin_g) + list(L.st_g) + list(L.v_g) + list(L.pi_g)) - {-1}
    for k in range(2, L.ntensors, 2):
        w, nw, b, nb = L.t_off[k], L.t_len[k], L.t_off[k + 1], L.t_len[k + 1]
        if w in gammas:
            p[w:w + nw] = 1.0 + rng.uniform(-0.1, 0.1, nw)
            p[b:b + nb] = rng.uniform(-0.1, 0.1, nb)
        else:
            bound = 1.0 / np.sqrt(nw / nb)
            p[w:w + nw] = rng.uniform(-bound, bound, nw)
            p[b:b + nb] = rng.uniform(-bound, bound, nb)
    p[L.hi], p[L.lo] = 1.0, -1.0
    return p


def _observations(seed, t, e, c, hw):
    rng = np.random.default_rng(seed)
    return dict(bev=rng.integers(0, 256, size=(t + 1, e, c, hw, hw), dtype=np.uint8),
                meas=rng.uniform(-1, 1, (t + 1, e, 8)).astype(np.float32),
                vmeas=rng.uniform(-1, 1, (t + 1, e, 3)).astype(np.float32),
                done=(rng.uniform(0, 1, (t + 1, e)) < 0.3).astype(np.float32),
                reward=rng.standard_normal((t, e)).astype(np.float32))


def _pair(agent_kw, t, e, mb, params_seed=3):
    """two agents with the same seed, parameters and Adam state, a rollout object each"""
    out = []
    for _ in range(2):
        ag = ppo_amd.CarlaAgent(max_batch=max(e, t * e // mb), seed=7, **agent_kw)
        p = _params(ag.layout2, params_seed)
        ag.load_params(p)
        out.append((ag, ppo_amd.CarlaRollout(ag, t, e, 1, mb, 0.99, 0.95, seed=5)))
    return out


def _serial(roll, obs, t_steps, e_envs):
    """env by env and step by step through ppo_carla_rollout_act(step, e, e + 1)"""
    acts = np.zeros((t_steps, e_envs, 2), np.float32)
    for e in range(e_envs):
        for t in range(t_steps):
            out = DeviceArray((1, 2))
            roll.act(t, e, e + 1, *[DeviceArray.from_numpy(obs[k][t, e:e + 1]) for k in ("bev", "meas", "vmeas", "done")],
                     out)
            roll.reward(t, e, e + 1, DeviceArray.from_numpy(obs["reward"][t, e:e + 1]))
            acts[t, e] = out.numpy()[0]
    ppo_amd.check(ppo_amd.lib().ppo_device_sync())
    return acts


def _threaded(lanes, obs, t_steps):
    """one Python thread per lane / env; each sleeps another few milliseconds between its steps"""
    acts = np.zeros((t_steps, len(lanes), 2), np.float32)
    errors = []

    def work(e):
        try:
            for t in range(t_steps):
                acts[t, e] = lanes[e].act(t, e, obs["bev"][t, e], obs["meas"][t, e], obs["vmeas"][t, e], obs["done"][t, e])
                lanes[e].reward(t, e, obs["reward"][t, e])
                time.sleep(0.001 * (1 + 4 * ((e + 1) % 3)))  # 5, 9 and 1 ms: env 2 runs ahead of env 0
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))

    threads = [threading.Thread(target=work, args=(e,)) for e in range(len(lanes))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    return acts


def _same_storage(a, b):
    for k in STORED:
        x, y = a.buffer(k).numpy(), b.buffer(k).numpy()
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=k)


CASES = {
    "default": (dict(), 15, 192, 2),
    "layer_norm": (dict(encoder="roach_ln", layer_norm=True, policy_layer_norm=True), 15, 192, 1),
    # 37 249-byte rows: every storage row after the first is unaligned, conv1 takes the generic kernel
    "bev_1x193x193": (dict(obs_channels=1, bev=193), 1, 193, 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_lanes_equal_serial_acts(case):
    ppo_amd.set_device(0)
    agent_kw, c, hw, iterations = CASES[case]
    (ag_a, ro_a), (ag_b, ro_b) = _pair(agent_kw, T, E, 3)
    lanes = [ro_b.lane() for _ in range(E)]
    try:
        for it in range(iterations):  # the second one starts behind a train: the lanes wait for its events
            obs = _observations(20 + it, T, E, c, hw)
            assert ro_a.iteration == ro_b.iteration == it
            acts_a = _serial(ro_a, obs, T, E)
            acts_b = _threaded(lanes, obs, T)
            for ln in lanes:
                ln.sync()  # the rewards are asynchronous
            np.testing.assert_array_equal(ro_b.buffer("bev").numpy(), obs["bev"][:T])
            np.testing.assert_array_equal(ro_b.buffer("rewards").numpy(), obs["reward"])
            _same_storage(ro_a, ro_b)
            np.testing.assert_array_equal(_bits(acts_a), _bits(acts_b))
            np.testing.assert_array_equal(_bits(acts_b), _bits(ro_b.buffer("actions").numpy()))
            assert np.isfinite(acts_b).all() and len(np.unique(acts_b)) > T * E  # sampled, not constant
            for ro in (ro_a, ro_b):
                ro.gae(*[DeviceArray.from_numpy(obs[k][T]) for k in ("bev", "meas", "vmeas", "done")])
                ro.train(lr=1e-3, want_stats=False)
            pa, pb = ag_a.params(), ag_b.params()
            np.testing.assert_array_equal(_bits(pa), _bits(pb))
            assert not np.array_equal(pa, _params(ag_a.layout2, 3))  # training moved them
            _same_storage(ro_a, ro_b)
    finally:
        ro_b.close(), ro_a.close(), ag_a.close(), ag_b.close()


def test_two_lanes_at_once_share_no_forward_buffer():
    """One step from two lanes released together, 20 times: every round must store what the serial acts
    stored. Equality only: the two rows differ in every input array, so a buffer written by both lanes
    would change at least one row's results."""
    ppo_amd.set_device(0)
    (ag_a, ro_a), (ag_b, ro_b) = _pair(dict(), 1, 2, 1)
    obs = _observations(31, 1, 2, 15, 192)
    for k in ("bev", "meas", "vmeas"):
        assert not np.array_equal(obs[k][0, 0], obs[k][0, 1])
    obs["done"][0] = (0.0, 1.0)
    lanes = [ro_b.lane(), ro_b.lane()]
    rounds = 20
    start, done = threading.Barrier(3), threading.Barrier(3)
    acts = np.zeros((rounds, 2, 2), np.float32)
    errors = []

    def work(e):
        try:
            for r in range(rounds):
                start.wait(timeout=60)
                acts[r, e] = lanes[e].act(0, e, obs["bev"][0, e], obs["meas"][0, e], obs["vmeas"][0, e], obs["done"][0, e])
                lanes[e].reward(0, e, obs["reward"][0, e])
                lanes[e].sync()
                done.wait(timeout=60)
        except Exception as ex:  # noqa: BLE001
            errors.append(repr(ex))
            start.abort(), done.abort()

    try:
        ref = _serial(ro_a, obs, 1, 2)
        assert not np.array_equal(ref[0, 0], ref[0, 1])
        threads = [threading.Thread(target=work, args=(e,)) for e in range(2)]
        for th in threads:
            th.start()
        try:
            for r in range(rounds):
                for k in ("actions", "logp", "values", "meas", "dones"):  # stale results cannot pass for new ones
                    ro_b.buffer(k).zero()
                start.wait(timeout=60)
                done.wait(timeout=60)
                _same_storage(ro_a, ro_b)
                np.testing.assert_array_equal(_bits(acts[r]), _bits(ref[0]), err_msg=f"round {r}")
        except threading.BrokenBarrierError:
            pass
        finally:
            start.abort() if errors else None
            for th in threads:
                th.join(timeout=60)
        assert not errors, errors
    finally:
        ro_b.close(), ro_a.close(), ag_a.close(), ag_b.close()
