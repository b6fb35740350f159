"""ppo_create_ex's kernel plan and ppo_update_ex's launch sequence against a recording of the commit before
the plan existed (tests/golden/capi_plan_parent/plan.json, written on an MI355X by
scripts/record_capi_parent.py from a build of that parent commit).

Each row of TABLE is a (config, options) pair. For a pair that create refuses the fixture holds the
ppo_last_error text; for every other pair the kernel_info string and SHA-256 digests of what three updates
leave behind. The update kernels sum in fixed orders, so the same launches with the same arguments give the
same bits: strings and digests are compared for equality, nothing is measured.

A row that creates: parameters of test_gpu_parity.random_params (seed 5); a [T, E] storage of standard
normal observations, actions inside the action range, the policy's own log-probs and values of them plus
noise, random rewards and sparse dones, all written through the public buffer pointers (seed 7);
ppo_gae_from_values over the collected steps (digest "gae": advantages | returns); then three ppo_update_ex
calls at lr 3e-4, 2e-4, 1e-4. The first is eager, the later ones replay the update graph where it is on.
Digest "stats": the three ppo_update_stats; "params", "adam": the parameters and Adam's m | v after the third.

The rows cover the planner's branches (both agents; OP = 16, 32, 112 and, for the 64-wide agent's split and
LDS-DMA kernels, 384; each option value; every refusal of create, and pairs of refusals to pin their order)
and the update's (launch pairs with a full and with a shorter last pair, whose unused dW partial rows are
zero-filled; the fold, the cooperative clip + Adam; graph and eager; norm_adv and clip_vloss off; a partial
collection; caller permutations; a host communicator, which turns graph and fold off per call)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402
from test_gpu_parity import fill_storage, random_params  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_plan_parent", "plan.json")

LN, TN = ppo_amd.PPO_NET_LN_BETA, ppo_amd.PPO_NET_TANH_NORMAL
# agents: (net_kind, obs_dim, act_dim, hidden)
LN16, LN32, LN32K4, LN112 = (LN, 11, 3, 256), (LN, 17, 6, 256), (LN, 18, 4, 256), (LN, 105, 8, 256)
LN32W = (LN, 17, 17, 256)  # 34 heads: three head tiles, no split-bf16 form, and too many for k_fwdbwd's LDS
TN16, TN32, TN112, TN384 = (TN, 11, 3, 64), (TN, 17, 6, 64), (TN, 105, 8, 64), (TN, 376, 17, 64)
TN256, LN64 = (TN, 17, 6, 256), (LN, 17, 6, 64)
SMALL = dict(E=32, T=16, MB=2, EP=2)     # M = 256
PAIRS = dict(E=64, T=128, MB=1, EP=2)    # M = 8192: upd_split's two launch pairs of 4096 rows, eager by auto
PAIRS_G = dict(E=64, T=64, MB=1, EP=2)   # M = 4096: the smallest minibatch with two pairs; the graph by auto
# M = 4097: pairs of Mq = 2080 and 2017 rows at 64 rows per dW chunk: 33 and 32 chunks, so the last pair's 33rd
# partial row is zero-filled (Mq = ((M + 1) / 2 + 31) & ~31, rows_per_chunk = 64, nchunks = ceil(Mq / 64))
SHORT = dict(E=241, T=17, MB=1, EP=2)


def row(name, agent, options=None, shape=SMALL, **kw):
    return dict(name=name, agent=agent, options=options, **{**shape, **kw})


TABLE = [row(f"default_{n}", a) for n, a in (("ln16", LN16), ("ln32", LN32), ("ln32k4", LN32K4), ("ln112", LN112),
                                             ("tn16", TN16), ("tn32", TN32), ("tn112", TN112),
                                             ("tn384", TN384), ("tn256", TN256))]
# the 64-wide LayerNorm-Beta agent has no k_upd form and lands on k_fwdbwd: its plan only
TABLE += [row("plan_ln64", LN64, plan_only=True)]
TABLE += [row("ln32_" + o.replace("=", "_").replace(",", "_"), LN32, o) for o in (
    "upd_kernel=fwdbwd", "upd_mfma=16", "upd_mfma=32", "upd_mfma=mix", "upd_mfma=bx6", "upd_mfma=auto",
    "dw_mfma=f32", "dw_mfma=bf16x9", "dw_mfma=bf16x8", "dw_mfma=bf16x6", "dw_dma=0", "dw_fused=0", "dw_slices=1",
    "dw_slices=2", "dw_rows=64", "dw_stage=dma", "dw_stage=split_once", "h1_handoff=recompute", "h1_handoff=store",
    "gradnorm=fold", "gradnorm=slices", "gradstep=fused", "gradstep=fused,gradnorm=fold", "update_graph=0",
    "update_graph=1", "values_mfma=f32", "values_mfma=bx6", "gae=serial", "gae=scan", "rollout_kernel=split",
    "rollout_kernel=valu", "rollout_kernel=mfma", "rollout=per_step", "act_kernel=4", "upd_split=1",
    "upd_kernel=fwdbwd,dw_fused=0,update_graph=0")]
TABLE += [row("ln16_upd_mfma_16", LN16, "upd_mfma=16"), row("ln16_dw_stage_dma", LN16, "dw_stage=dma"),
          row("ln112_dw_dma_0", LN112, "dw_dma=0"), row("ln112_upd_mfma_32", LN112, "upd_mfma=32"),
          row("ln112_dw_mfma_f32", LN112, "dw_mfma=f32"),
          row("tn32_upd_mfma_16", TN32, "upd_mfma=16"), row("tn32_dw_rows_64", TN32, "dw_rows=64"),
          row("tn32_dw_rows_48", TN32, "dw_rows=48"), row("tn32_update_graph_0", TN32, "update_graph=0"),
          row("tn32_upd_kernel_fwdbwd", TN32, "upd_kernel=fwdbwd"), row("tn112_gradnorm_fold", TN112, "gradnorm=fold"),
          row("tn384_upd2_split_2", TN384, "upd2_split=2"), row("tn384_upd2_split_3", TN384, "upd2_split=3"),
          row("tn384_f32_dw2", TN384, "upd_mfma=16,dw_dma=0"),
          row("ln32_pairs", LN32, "upd_split=2", PAIRS), row("ln32_pairs_graph", LN32, "upd_split=8", PAIRS_G),
          row("ln32_pairs_short", LN32, "upd_split=2", SHORT), row("ln16_pairs_recompute", LN16, "upd_split=2,h1_handoff=recompute", PAIRS_G),
          row("ln32_no_norm_adv", LN32, norm_adv=0), row("ln32_no_clip_vloss", LN32, clip_vloss=0),
          row("tn32_no_norm_adv_no_clip_vloss", TN32, norm_adv=0, clip_vloss=0),
          row("ln32_partial", LN32, nsteps=10), row("tn32_partial_eager", TN32, "update_graph=0", nsteps=5),
          row("ln32_caller_perms", LN32, perms=True), row("tn32_caller_perms_eager", TN32, "update_graph=0", perms=True),
          row("ln32_host_comm", LN32, comm=True), row("ln32_host_comm_fold", LN32, "gradnorm=fold", comm=True),
          row("ln32_one_minibatch", LN32, E=33, T=3, MB=1, EP=1)]
# what create refuses, in the order of its checks; then pairs of refusals, which pin that order
TABLE += [row("refuse_" + n, a, o, **kw) for n, a, o, kw in (
    ("option_without_eq", LN32, "upd_mfma", {}), ("option_unknown", LN32, "upd_mfma=8", {}),
    ("net_kind", (5, 17, 6, 256), None, {}), ("hidden", (LN, 17, 6, 128), None, {}), ("act_dim", (LN, 17, 21, 256), None, {}),
    ("sizes", LN32, None, dict(EP=0)), ("minibatches", LN32, None, dict(MB=3)), ("batch", LN32, None, dict(E=65536, T=32768)),
    ("no_instantiation", (LN, 40, 6, 256), None, {}), ("rollout_valu", TN32, "rollout_kernel=valu", {}),
    ("rollout_split", LN112, "rollout_kernel=split", {}), ("rollout_split_per_step", LN32, "rollout_kernel=split,rollout=per_step", {}),
    ("mfma32_agent", TN32, "upd_mfma=32", {}), ("mix_agent", TN256, "upd_mfma=mix", {}), ("bx6_agent", TN256, "upd_mfma=bx6", {}),
    ("upd2_split_shape", TN32, "upd2_split=2", {}), ("upd2_split_fwdbwd", TN384, "upd2_split=3,upd_kernel=fwdbwd", {}),
    ("bx6_upd2_shape", TN32, "upd_mfma=bx6", {}), ("bx6_upd2_split", TN384, "upd_mfma=bx6,upd2_split=2", {}),
    ("mfma32_fwdbwd", LN32, "upd_mfma=32,upd_kernel=fwdbwd", {}), ("bx6_heads", LN32W, "upd_mfma=bx6", {}),
    ("bx6_fwdbwd", LN32, "upd_mfma=bx6,upd_kernel=fwdbwd", {}), ("bx6_ln64", LN64, "upd_mfma=bx6", {}),
    ("values_bx6", LN32, "values_mfma=bx6,upd_mfma=16", {}), ("upd_split_shape", LN112, "upd_split=2", {}),
    ("upd_split_unfused", LN32, "upd_split=4,dw_fused=0", {}), ("h1_recompute_f32", LN32, "h1_handoff=recompute,dw_mfma=f32", {}),
    ("h1_recompute_agent", TN256, "h1_handoff=recompute", {}), ("split_once_recompute", LN32, "dw_stage=split_once,h1_handoff=recompute", {}),
    ("split_once_shape", LN112, "dw_stage=split_once", {}),
    # the one refusal after the context exists: k_fwdbwd's LDS for 34 head rows passes the limit
    ("set_lds", LN32W, None, {}), ("set_lds_after_plan", LN32W, "dw_fused=0,gradstep=fused", {}),
    ("two_option_then_hidden", (LN, 17, 6, 128), "gae=parallel", {}), ("two_rollout_then_mfma32", TN32, "rollout_kernel=valu,upd_mfma=32", {}),
    ("two_mfma32_then_upd2_split", TN32, "upd2_split=2,upd_mfma=32", {}),
    ("two_values_then_upd_split", LN112, "upd_split=2,values_mfma=bx6,upd_mfma=16", {}),
    ("two_recompute_then_split_once", LN32, "dw_stage=split_once,h1_handoff=recompute,dw_mfma=f32", {}))]
NAMES = [r["name"] for r in TABLE]
assert len(set(NAMES)) == len(NAMES)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_row(r):
    """What the fixture holds for one row, computed with the loaded library."""
    kind, O_, A, H = r["agent"]
    E, T, MB, EP = r["E"], r["T"], r["MB"], r["EP"]
    hc = ppo_amd.HipConfig(kind, O_, A, H, E, T, MB, EP, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, r.get("norm_adv", 1),
                           r.get("clip_vloss", 1), 1, 0, 1)
    ppo_amd.set_device(0)
    try:
        ag = ppo_amd.Agent(hc, options=r["options"])
    except ppo_amd.PPOError as e:
        return {"error": str(e)}
    try:
        out = {"kernel_info": ag.kernel_info()}
        if r.get("plan_only"):
            return out
        ag.load_params(random_params(ag.layout, np.random.default_rng(5)))
        rng = np.random.default_rng(7)
        n = T * E
        x = rng.standard_normal((n, O_)).astype(np.float32)
        act = (rng.uniform(-0.95, 0.95, (n, A)) if kind == LN else rng.standard_normal((n, A)) * 0.5).astype(np.float32)
        lp, v = [], []
        for i in range(0, n, 4096):  # the policy's own log-probs and values: both branches of the clip occur
            _, l_, _, v_ = ag.get_action_and_value(DeviceArray.from_numpy(x[i:i + 4096]), ppo_amd.PPO_GIVEN,
                                                   DeviceArray.from_numpy(act[i:i + 4096]))
            lp.append(l_.numpy()), v.append(v_.numpy())
        olp = (np.concatenate(lp) + rng.standard_normal(n) * 0.2).astype(np.float32)
        ov = (np.concatenate(v) + rng.standard_normal(n) * 0.1).astype(np.float32)
        zeros = np.zeros(n, np.float32)
        fill_storage(ag, T, E, x, act, olp, zeros, zeros, ov)
        ag.buffer(ppo_amd.BUF_REWARDS, (T, E)).upload(rng.standard_normal((T, E)).astype(np.float32))
        ag.buffer(ppo_amd.BUF_DONES, (T, E)).upload((rng.random((T, E)) < 0.05).astype(np.float32))
        nsteps = r.get("nsteps") or T
        ag.gae_from_values(DeviceArray.from_numpy(rng.standard_normal(E).astype(np.float32)),
                           DeviceArray.from_numpy((rng.random(E) < 0.5).astype(np.float32)), nsteps)
        ag.sync()
        out["gae"] = _sha(ag.buffer(ppo_amd.BUF_ADVANTAGES, (T, E)).numpy()[:nsteps],
                          ag.buffer(ppo_amd.BUF_RETURNS, (T, E)).numpy()[:nsteps])
        perms = None
        if r.get("perms"):
            perms = DeviceArray.from_numpy(np.concatenate([rng.permutation(n) for _ in range(EP)]).astype(np.int32))
        if r.get("comm"):
            ag.comm_init_host(0, 1, lambda buf, average: None)  # one rank: the sum and the average are the values
        stats = []
        for lr in (3e-4, 2e-4, 1e-4):
            st = ag.update(lr, perms=perms, want_stats=True, num_steps_collected=r.get("nsteps"))
            assert st["minibatches"] == EP * MB
            stats.append(np.array([st[k] for k in ("pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl",
                                                   "clipfrac", "grad_norm")], np.float32))
        assert np.isfinite(np.stack(stats)).all(), stats  # digests of NaNs would compare nothing
        out["stats"] = _sha(*stats)
        out["params"] = _sha(ag.params())
        m, v_, step = ag.adam_state()
        assert step == 3 * EP * MB
        out["adam"] = _sha(m, v_)
        return out
    finally:
        ag.close()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_the_table(parent):
    assert sorted(parent) == sorted(NAMES)
    assert sum("error" in v for v in parent.values()) == sum(n.startswith("refuse_") for n in NAMES)


@pytest.mark.parametrize("r", TABLE, ids=NAMES)
def test_plan_and_update_equal_the_parent_commits(parent, r):
    assert run_row(r) == parent[r["name"]]
