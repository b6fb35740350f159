"""GPU tests of the CaRL rollout object (ppo_carla_rollout_*: storage, act, GAE, permutations, the
epoch loop) and of its gather kernels (k_carla_gather / k_carla_gather_f32 through the debug hooks).

Everything here is an exact comparison. The gathers move bytes (numpy fancy indexing is the reference).
Act / GAE / train drive the agent through ppo_carla_forward / ppo_carla_update, whose kernels have no
atomics: the same calls on a second agent with the same state give the same bits, so the update's own
parity bars (test_gpu_carla_update.py) carry over without a new tolerance. GAE and the permutation are
compared with the CPU oracle (oracle_lib.gae / perm) bit for bit, as the MLP agents' are.

Sizes: E = 4 envs, T = 6 steps, 3 minibatches of 8 rows, 2 epochs (13 MB of bev)."""
import numpy as np
import pytest

import carla_inputs as CI
import oracle_lib as O

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402

E, T, MB, EP, M = 4, 6, 3, 2, 8
B = T * E
ROW = 15 * 192 * 192  # 552 960 bytes
GAMMA, LAM, SEED = 0.99, 0.95, 5
TRAIN = dict(clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, adam_eps=1e-5)
LR = 3e-4


# ------------------------------------------------------------------------------------------------
# gather hooks
# ------------------------------------------------------------------------------------------------
def _gather_case(row_bytes, idx, src_rows, so, do, rng):
    """dst[i] = src[idx[i]] with the bases moved by so / do bytes; canaries before and after dst"""
    n = len(idx)
    src = rng.integers(0, 256, size=so + src_rows * row_bytes, dtype=np.uint8)
    pad = 64
    dst0 = np.full(do + n * row_bytes + pad, 0xA5, np.uint8)
    d_src, d_dst = DeviceArray.from_numpy(src), DeviceArray.from_numpy(dst0)
    d_idx = DeviceArray.from_numpy(np.asarray(idx if n else [0], np.int32))
    ppo_amd.carla_gather(d_src, d_idx, d_dst, n, row_bytes, so, do)
    got = d_dst.numpy()
    ref = src[so:].reshape(src_rows, row_bytes)[np.asarray(idx, np.int64)].reshape(-1)
    np.testing.assert_array_equal(got[do:do + n * row_bytes], ref)
    assert (got[:do] == 0xA5).all() and (got[do + n * row_bytes:] == 0xA5).all()
    for d in (d_src, d_dst, d_idx):
        d.free()


IDX = [8, 0, 3, 3, 8, 1, 8]  # repeats, and the last of 9 rows three times


@pytest.mark.parametrize("row_bytes", [1, 15, 16, 17, 111747, 552960])
def test_gather_matches_numpy(row_bytes):
    ppo_amd.set_device(0)
    rng = np.random.default_rng(row_bytes)
    offsets = [(0, 0), (1, 0), (0, 1), (1, 1)] if row_bytes <= 111747 else [(0, 0)]
    for so, do in offsets:
        _gather_case(row_bytes, IDX, 9, so, do, rng)
    _gather_case(row_bytes, [8], 9, 0, 0, rng)   # n = 1, the last row
    _gather_case(row_bytes, [], 9, 0, 0, rng)    # n = 0: nothing is written


def test_gather_many_rows():
    """3 000 rows of 17 bytes with repeats: thousands of workgroups, every one with a head and a tail"""
    ppo_amd.set_device(0)
    rng = np.random.default_rng(1)
    _gather_case(17, list(rng.integers(0, 50, 3000)), 50, 1, 0, rng)


def test_gather_more_items_than_the_grid():
    """2^22 + 1 000 one-byte rows: more (row, chunk) items than the launch's 2^22 workgroups, so the grid
    strides; the bytewise path, every row its own workgroup"""
    ppo_amd.set_device(0)
    rng = np.random.default_rng(4)
    n = (1 << 22) + 1000
    src = rng.integers(0, 256, size=251, dtype=np.uint8)
    idx = rng.integers(0, 251, n).astype(np.int32)
    d_src, d_idx = DeviceArray.from_numpy(src), DeviceArray.from_numpy(idx)
    d_dst = DeviceArray.from_numpy(np.full(n + 64, 0xA5, np.uint8))
    ppo_amd.carla_gather(d_src, d_idx, d_dst, n, 1)
    got = d_dst.numpy()
    np.testing.assert_array_equal(got[:n], src[idx])
    assert (got[n:] == 0xA5).all()
    for d in (d_src, d_idx, d_dst):
        d.free()


def test_gather_offsets_beyond_4gib():
    """8 000 stored rows of 552 960 bytes (4.4 GB, left uninitialised): rows 7 766 / 7 767 straddle 2^32
    bytes, row 7 999 ends the allocation; a 32-bit offset anywhere would read another row."""
    ppo_amd.set_device(0)
    rows = [0, 7766, 7767, 7999]
    rng = np.random.default_rng(2)
    data = rng.integers(0, 256, size=(4, ROW), dtype=np.uint8)
    src = DeviceArray((8000, ROW), np.uint8)
    for k, r in enumerate(rows):
        ppo_amd.check(ppo_amd.lib().ppo_memcpy_h2d(src.ptr + r * ROW, data[k].ctypes.data, ROW))
    order = [3, 2, 0, 1]
    d_idx = DeviceArray.from_numpy(np.asarray([rows[k] for k in order], np.int32))
    dst = DeviceArray.from_numpy(np.full(4 * ROW + 64, 0xA5, np.uint8))
    ppo_amd.carla_gather(src, d_idx, dst, 4, ROW)
    got = dst.numpy()
    np.testing.assert_array_equal(got[:4 * ROW].reshape(4, ROW), data[order])
    assert (got[4 * ROW:] == 0xA5).all()
    for d in (src, d_idx, dst):
        d.free()


@pytest.mark.parametrize("idx", [IDX, [8], []])
def test_gather_f32_side_arrays(idx):
    """meas, vmeas, actions and the four per-row scalars in one launch"""
    ppo_amd.set_device(0)
    rng = np.random.default_rng(3)
    widths = [8, 3, 2, 1, 1, 1, 1]
    n = len(idx)
    srcs = [rng.standard_normal((9, w)).astype(np.float32) for w in widths]
    d_src = [DeviceArray.from_numpy(s) for s in srcs]
    d_dst = [DeviceArray.from_numpy(np.full(n * w + 4, -7.0, np.float32)) for w in widths]
    d_idx = DeviceArray.from_numpy(np.asarray(idx if n else [0], np.int32))
    ppo_amd.carla_gather_f32(d_src, d_idx, d_dst, n, widths)
    for s, d, w in zip(srcs, d_dst, widths):
        got = d.numpy()
        np.testing.assert_array_equal(got[:n * w], s[np.asarray(idx, np.int64)].reshape(-1))
        assert (got[n * w:] == -7.0).all()


# ------------------------------------------------------------------------------------------------
# rollout object
# ------------------------------------------------------------------------------------------------
def _observations(seed):
    """T + 1 steps of E envs (the last one is the next observation), rewards, and dones with episode ends"""
    rng = np.random.default_rng(seed)
    obs = dict(bev=rng.integers(0, 256, size=(T + 1, E, 15, 192, 192), dtype=np.uint8),
               meas=rng.uniform(-1, 1, (T + 1, E, 8)).astype(np.float32),
               vmeas=rng.uniform(-1, 1, (T + 1, E, 3)).astype(np.float32),
               done=(rng.uniform(0, 1, (T + 1, E)) < 0.3).astype(np.float32),
               reward=rng.standard_normal((T, E)).astype(np.float32))
    return obs


@pytest.fixture(scope="module")
def params():
    return CI.params(CI.layout())


def _agent(params, comm=False):
    ag = ppo_amd.CarlaAgent(max_batch=M, seed=7)
    ag.load_params(params)
    ag.load_adam(np.zeros(params.size, np.float32), np.zeros(params.size, np.float32), 0)
    if comm:
        ag.comm_init(ppo_amd.Agent.comm_unique_id(), 0, 1)
        ag.comm_broadcast_params(0)
    return ag


def _rollout(ag, rank=0):
    return ppo_amd.CarlaRollout(ag, T, E, EP, MB, GAMMA, LAM, seed=SEED, rank=rank)


def _dev(obs, key, t, e0, e1):
    return DeviceArray.from_numpy(obs[key][t, e0:e1])


def _collect(roll, obs):
    """rollout_act as ranges [0, 3) and [3, 4) per step, then the rewards; returns the action_out rows"""
    acts = np.zeros((T, E, 2), np.float32)
    for t in range(T):
        for e0, e1 in ((0, 3), (3, 4)):
            out = DeviceArray((e1 - e0, 2))
            roll.act(t, e0, e1, _dev(obs, "bev", t, e0, e1), _dev(obs, "meas", t, e0, e1),
                     _dev(obs, "vmeas", t, e0, e1), _dev(obs, "done", t, e0, e1), out)
            acts[t, e0:e1] = out.numpy()
        roll.reward(t, 0, E, DeviceArray.from_numpy(obs["reward"][t]))
    return acts


def _gae(roll, obs, nsteps):
    roll.gae(*[DeviceArray.from_numpy(obs[k][T]) for k in ("bev", "meas", "vmeas", "done")], nsteps)


def test_create_refuses_bad_sizes(params):
    ppo_amd.set_device(0)
    ag = _agent(params)
    try:
        for t, e, ep, mb, msg in [(0, 4, 2, 3, "positive"), (6, 0, 2, 3, "positive"), (6, 4, 0, 3, "positive"),
                                  (6, 4, 2, 0, "positive"), (6, 4, 2, 5, "divisible"),
                                  (6, 4, 2, 2, "max_batch"),      # 12 rows per minibatch > max_batch 8
                                  (1, 9, 1, 3, "max_batch")]:     # 9 envs > max_batch 8
            with pytest.raises(ppo_amd.PPOError, match=msg):
                ppo_amd.CarlaRollout(ag, t, e, ep, mb)
    finally:
        ag.close()


def test_act_stores_inputs_and_the_forward_outputs(params):
    ppo_amd.set_device(0)
    obs = _observations(11)
    ag, ref = _agent(params), _agent(params)
    roll = _rollout(ag)
    try:
        acts = [None, None]
        for it in (0, 1):
            assert roll.iteration == it
            out = _collect(roll, obs)
            ppo_amd.check(ppo_amd.lib().ppo_device_sync())
            np.testing.assert_array_equal(roll.buffer("bev").numpy(), obs["bev"][:T])
            np.testing.assert_array_equal(roll.buffer("meas").numpy(), obs["meas"][:T])
            np.testing.assert_array_equal(roll.buffer("vmeas").numpy(), obs["vmeas"][:T])
            np.testing.assert_array_equal(roll.buffer("dones").numpy(), obs["done"][:T])
            np.testing.assert_array_equal(roll.buffer("rewards").numpy(), obs["reward"])
            a, lp, v = (roll.buffer(k).numpy() for k in ("actions", "logp", "values"))
            np.testing.assert_array_equal(a, out)
            for t in range(T):
                for e0, e1 in ((0, 3), (3, 4)):
                    ra, rlp, _, rv, _, _ = ref.forward(_dev(obs, "bev", t, e0, e1), _dev(obs, "meas", t, e0, e1),
                                                       _dev(obs, "vmeas", t, e0, e1), env_base=e0,
                                                       step_id=it * T + t)
                    np.testing.assert_array_equal(a[t, e0:e1], ra.numpy())
                    np.testing.assert_array_equal(lp[t, e0:e1], rlp.numpy())
                    np.testing.assert_array_equal(v[t, e0:e1], rv.numpy())
            acts[it] = a
            roll.set_iteration(it + 1)
        # the same observations, the next iteration's step ids: other draws
        assert not np.array_equal(acts[0], acts[1])
    finally:
        roll.close(), ag.close(), ref.close()


@pytest.mark.parametrize("nsteps", [6, 4])
def test_gae_matches_the_oracle(params, nsteps):
    ppo_amd.set_device(0)
    obs = _observations(12)
    ag, ref = _agent(params), _agent(params)
    roll = _rollout(ag)
    try:
        _collect(roll, obs)
        _gae(roll, obs, nsteps)
        ppo_amd.check(ppo_amd.lib().ppo_device_sync())
        rew, val, don, adv, ret = (roll.buffer(k).numpy() for k in ("rewards", "values", "dones", "adv", "returns"))
        nv = roll.buffer("next_value").numpy()
        _, _, _, rv, _, _ = ref.forward(*[DeviceArray.from_numpy(obs[k][T]) for k in ("bev", "meas", "vmeas")],
                                        sample_type="mean")
        np.testing.assert_array_equal(nv, rv.numpy())
        if nsteps == T:
            oadv, oret = O.gae(rew, val, don, nv, obs["done"][T], GAMMA, LAM)
        else:  # the bootstrap is the stored step nsteps
            oadv, oret = O.gae(rew[:nsteps], val[:nsteps], don[:nsteps], val[nsteps], don[nsteps], GAMMA, LAM)
        np.testing.assert_array_equal(adv[:nsteps], oadv)
        np.testing.assert_array_equal(ret[:nsteps], oret)
        np.testing.assert_array_equal(ret[:nsteps], adv[:nsteps] + val[:nsteps])
    finally:
        roll.close(), ag.close(), ref.close()


def test_default_permutations(params):
    ppo_amd.set_device(0)
    obs = _observations(13)
    ag = _agent(params)
    roll, roll1 = _rollout(ag), _rollout(ag, rank=1)
    try:
        _collect(roll, obs)
        _gae(roll, obs, T)
        for it, nsteps in ((0, T), (1, 4)):
            assert roll.iteration == it
            roll.train(LR, nsteps, want_stats=False, **TRAIN)
            p = roll.last_perms()
            bc = nsteps * E
            for e in range(EP):
                want = O.perm(bc, SEED, 0, it * EP + e).astype(np.int32)
                assert sorted(want) == list(range(bc))
                np.testing.assert_array_equal(p[e, :bc], want)
                np.testing.assert_array_equal(p[e, bc:], want[:B - bc])   # [16, 24) repeats [0, 8)
        # another rank, the same seed and epoch counter 0: another permutation
        _collect(roll1, obs)
        _gae(roll1, obs, T)
        roll1.train(LR, T, want_stats=False, **TRAIN)
        p1 = roll1.last_perms()
        np.testing.assert_array_equal(p1[0], O.perm(B, SEED, 1, 0).astype(np.int32))
        assert not np.array_equal(p1[0], O.perm(B, SEED, 0, 0).astype(np.int32))
    finally:
        roll.close(), roll1.close(), ag.close()


_FREE = {}  # (inject, nsteps) -> the communicator-free result, for the one-rank communicator case


def _seq_mean(x):
    s = np.float32(0)
    for v in x:
        s = np.float32(s + np.float32(v))
    return np.float32(s / np.float32(len(x)))


def _train_case(params, inject, nsteps, comm):
    """rollout_train on agent A against six ppo_carla_update calls on agent B (minibatches gathered on
    the host with numpy); returns A's state."""
    obs = _observations(14)
    ag, ref = _agent(params, comm), _agent(params, comm)
    roll = _rollout(ag)
    try:
        _collect(roll, obs)
        _gae(roll, obs, nsteps)
        ppo_amd.check(ppo_amd.lib().ppo_device_sync())
        names = ("bev", "meas", "vmeas", "actions", "logp", "adv", "returns", "values")
        h = {k: roll.buffer(k).numpy().reshape((B,) + roll.buffer(k).shape[2:]) for k in names}
        perms = None
        if inject:
            rng = np.random.default_rng(15)
            perms = np.stack([rng.integers(0, nsteps * E, B) for _ in range(EP)]).astype(np.int32)
        st = roll.train(LR, nsteps, DeviceArray.from_numpy(perms) if inject else None, want_stats=True, **TRAIN)
        used = roll.last_perms()
        if inject:
            np.testing.assert_array_equal(used, perms)
        assert roll.iteration == 1
        steps = []
        for e in range(EP):
            for mb in range(MB):
                idx = used[e, mb * M:(mb + 1) * M].astype(np.int64)
                assert idx.min() >= 0 and idx.max() < nsteps * E
                d = [DeviceArray.from_numpy(np.ascontiguousarray(h[k][idx])) for k in names]
                steps.append(ref.update(*d, lr=LR, **TRAIN))
        assert len(steps) == EP * MB == 6
        np.testing.assert_array_equal(ag.params(), ref.params())
        np.testing.assert_array_equal(ag.last_grad(), ref.last_grad())
        (m0, v0, s0), (m1, v1, s1) = ag.adam_state(), ref.adam_state()
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(v0, v1)
        assert s0 == s1 == 6
        assert not np.array_equal(ag.params(), params)
        assert np.float32(st["mean_clipfrac"]) == _seq_mean([s["clipfrac"] for s in steps])
        assert {k: st[k] for k in steps[-1]} == steps[-1]
        return ag.params(), ag.last_grad(), (m0, v0, s0), st
    finally:
        roll.close(), ag.close(), ref.close()


@pytest.mark.parametrize("inject,nsteps", [(True, 6), (False, 6), (True, 4), (False, 4)])
def test_train_equals_the_manual_chain(params, inject, nsteps):
    ppo_amd.set_device(0)
    _FREE[(inject, nsteps)] = _train_case(params, inject, nsteps, comm=False)


def test_train_with_one_rank_communicator_is_bit_identical(params):
    ppo_amd.set_device(0)
    if (False, 6) not in _FREE:
        _FREE[(False, 6)] = _train_case(params, False, 6, comm=False)
    p0, g0, (m0, v0, s0), st0 = _FREE[(False, 6)]
    p1, g1, (m1, v1, s1), st1 = _train_case(params, False, 6, comm=True)
    np.testing.assert_array_equal(p0, p1)
    np.testing.assert_array_equal(g0, g1)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(v0, v1)
    assert s0 == s1 and st0 == st1


def test_carla_trainer_iterates(params):
    """CarlaTrainer.iterate: T act / env-step / reward rounds, GAE and train against caller-supplied arrays"""
    ppo_amd.set_device(0)
    rng = np.random.default_rng(21)
    seen = []

    def env_step(actions):
        assert actions.shape == (E, 2) and np.isfinite(actions).all() and (np.abs(actions) <= 1).all()
        seen.append(actions.copy())
        return (rng.integers(0, 256, size=(E, 15, 192, 192), dtype=np.uint8),
                rng.uniform(-1, 1, (E, 8)).astype(np.float32), rng.uniform(-1, 1, (E, 3)).astype(np.float32),
                rng.standard_normal(E).astype(np.float32), (rng.uniform(0, 1, E) < 0.2).astype(np.float32))

    ag = _agent(params)
    obs = _observations(22)
    tr = ppo_amd.CarlaTrainer(ag, env_step, (obs["bev"][0], obs["meas"][0], obs["vmeas"][0]), T, E, num_iterations=2,
                              update_epochs=EP, num_minibatches=MB, learning_rate=LR, seed=SEED, **TRAIN)
    try:
        assert tr.lr_now() == pytest.approx(LR)
        st = tr.iterate(want_stats=True)
        assert all(np.isfinite(v) for v in st.values()) and 0.0 <= st["mean_clipfrac"] <= 1.0
        assert tr.lr_now() == pytest.approx(LR / 2)
        tr.iterate()
        assert tr.iteration == 2 and tr.rollout.iteration == 2 and tr.global_step == 2 * T * E and len(seen) == 2 * T
        # the stored actions of the last collection are the ones the envs received
        np.testing.assert_array_equal(tr.rollout.buffer("actions").numpy(), np.stack(seen[T:]))
        assert ag.adam_state()[2] == 2 * EP * MB
        assert np.isfinite(ag.params()).all() and not np.array_equal(ag.params(), params)
    finally:
        tr.close(), ag.close()
