"""PPO_ROACH (Beta::roach_deterministic, rl_utils.h:112-131) of the LayerNorm-Beta agent through
ppo_get_action_and_value, for the act kernels the dispatcher chooses (k_act3 at hidden 256 with one and
two input blocks, k_act2 at hidden 64): against an fp64 restatement of the actor where the mode is well
conditioned, exactly on the three boundary branches, and the existing modes bitwise against outputs
recorded from the commit before PPO_ROACH existed (tests/golden/act_modes_parent)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
import oracle_lib as Orc  # noqa: E402
from ppo_amd import DeviceArray  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "act_modes_parent", "outputs.npz")
SHAPES = [(17, 6, 256), (11, 3, 256), (17, 6, 64)]  # k_act3 OP = 32, k_act3 OP = 16, k_act2
ROWS = (1, 3, 70)  # one row, a few, a ragged last 16-row tile over several workgroups
LO, HI = -1.0, 1.0


def make_agent(O_, A, H, kind=1):
    hc = ppo_amd.HipConfig(kind, O_, A, H, 64, 4, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
    return ppo_amd.Agent(hc)


def make_case(O_, A, H):
    """Parameters and 70 input rows. Small head weights around a head bias of +2 keep every
    concentration well above 1 (checked in the test on the fp64 values)."""
    rng = np.random.default_rng(100 * O_ + A + H)
    L = Orc.layout_init(1, O_, A, H)
    p = np.zeros(L.P, np.float32)
    for t in range(L.ntensors):
        o, n = L.t_off[t], L.t_len[t]
        p[o:o + n] = rng.standard_normal(n).astype(np.float32) * 0.1
    p[L.hi], p[L.lo] = HI, LO
    p[L.omean:L.omean + O_] = rng.standard_normal(O_) * 0.2
    p[L.ostd:L.ostd + O_] = rng.uniform(0.8, 1.5, O_)
    for tr in (L.critic, L.actor):
        p[tr[0]:tr[0] + H * O_] = rng.standard_normal(H * O_) / np.sqrt(O_)
        p[tr[4]:tr[4] + H * H] = rng.standard_normal(H * H) / np.sqrt(H)
        p[tr[2]:tr[2] + H] = rng.uniform(0.8, 1.2, H)
        p[tr[6]:tr[6] + H] = rng.uniform(0.8, 1.2, H)
    for w, b in ((L.aW3, L.ab3), (L.bW3, L.bb3)):
        p[w:w + A * H] = rng.standard_normal(A * H) * 0.02
        p[b:b + A] = 2.0 + rng.standard_normal(A) * 0.3
    x = rng.standard_normal((max(ROWS), O_)).astype(np.float32)
    return L, p.astype(np.float32), x


def actor_fp64(L, p, x):
    """The AC actor in fp64 torch: fixed normalisation, Linear-LayerNorm-ReLU twice, two heads,
    softplus + 1. Returns (alpha, beta)."""
    import torch
    import torch.nn.functional as F
    P = torch.from_numpy(p.astype(np.float64))
    H, O_, A = L.H, L.O, L.A
    t = list(L.actor)
    h = (torch.from_numpy(x.astype(np.float64)) - P[L.omean:L.omean + O_]) / P[L.ostd:L.ostd + O_]
    for w, b, g, be, fan in ((t[0], t[1], t[2], t[3], O_), (t[4], t[5], t[6], t[7], H)):
        h = F.linear(h, P[w:w + H * fan].reshape(H, fan), P[b:b + H])
        h = F.relu(F.layer_norm(h, (H,), P[g:g + H], P[be:be + H], 1e-5))
    al = F.softplus(F.linear(h, P[L.aW3:L.aW3 + A * H].reshape(A, H), P[L.ab3:L.ab3 + A])) + 1.0
    be = F.softplus(F.linear(h, P[L.bW3:L.bW3 + A * H].reshape(A, H), P[L.bb3:L.bb3 + A])) + 1.0
    return al, be


def roach_fp64(al, be):
    """The four-way rule, log-prob (torch.xlogy) and entropy of the Beta distribution in fp64."""
    import torch
    s = torch.where((al > 1) & (be > 1), (al - 1) / (al + be - 2),
                    torch.where((al <= 1) & (be > 1), torch.zeros_like(al),
                                torch.where((al > 1) & (be <= 1), torch.ones_like(al), al / (al + be))))
    lbeta = torch.lgamma(al) + torch.lgamma(be) - torch.lgamma(al + be)
    lp = (torch.xlogy(al - 1, s) + torch.xlogy(be - 1, 1 - s) - lbeta).sum(1)
    ent = (lbeta - (al - 1) * torch.digamma(al) - (be - 1) * torch.digamma(be)
           + (al + be - 2) * torch.digamma(al + be)).sum(1)
    return (s * (HI - LO) + LO).numpy(), lp.numpy(), ent.numpy()


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "O%d_A%d_H%d" % s)
def case(request):
    O_, A, H = request.param
    L, p, x = make_case(O_, A, H)
    ag = make_agent(O_, A, H)
    ag.load_params(p)
    yield L, p, x, ag
    ag.close()


@pytest.mark.parametrize("n", ROWS)
def test_roach_against_fp64(case, n):
    """Tolerances: those tests/test_gpu_parity.py applies to the PPO_MEAN action (rtol 1e-4, atol 2e-5)
    and to log-prob / entropy (rtol 1e-4, atol 2e-4) against the oracle."""
    L, p, x, ag = case
    al, be = actor_fp64(L, p, x[:n])
    assert float(al.min()) - 1 >= 0.1 and float(be.min()) - 1 >= 0.1  # the mode is well conditioned
    ra, rlp, rent = roach_fp64(al, be)
    act, lp, ent, _ = ag.get_action_and_value(DeviceArray.from_numpy(x[:n]), ppo_amd.PPO_ROACH)
    ea, elp, eent = np.abs(act.numpy() - ra).max(), np.abs(lp.numpy() - rlp).max(), np.abs(ent.numpy() - rent).max()
    print(f"max |d|: action {ea:.2e} logprob {elp:.2e} entropy {eent:.2e}")
    np.testing.assert_allclose(act.numpy(), ra, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(lp.numpy(), rlp, rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(ent.numpy(), rent, rtol=1e-4, atol=2e-4)
    # the mode is not the mean: the two deterministic actions differ
    am, _, _, _ = ag.get_action_and_value(DeviceArray.from_numpy(x[:n]), ppo_amd.PPO_MEAN)
    assert np.abs(am.numpy() - act.numpy()).max() > 1e-3


@pytest.mark.parametrize("which,expect", [("alpha", LO), ("beta", HI), ("both", LO + 0.5 * (HI - LO))])
def test_roach_boundary_branches_are_exact(case, which, expect):
    """A head with zero weights and bias -100: softplus underflows, the concentration is exactly 1.0f.
    alpha <= 1 < beta gives lo, beta <= 1 < alpha gives hi, both <= 1 the mean lo + 0.5 (hi - lo), bit
    for bit, with finite log-prob and entropy."""
    L, p, x, ag = case
    q = p.copy()
    for w, b in ([(L.aW3, L.ab3)] if which == "alpha" else [(L.bW3, L.bb3)] if which == "beta"
                 else [(L.aW3, L.ab3), (L.bW3, L.bb3)]):
        q[w:w + L.A * L.H] = 0.0
        q[b:b + L.A] = -100.0
    ag.load_params(q)
    try:
        for n in ROWS:
            act, lp, ent, _ = ag.get_action_and_value(DeviceArray.from_numpy(x[:n]), ppo_amd.PPO_ROACH)
            np.testing.assert_array_equal(act.numpy().view(np.uint32),
                                          np.full((n, L.A), expect, np.float32).view(np.uint32))
            assert np.isfinite(lp.numpy()).all() and np.isfinite(ent.numpy()).all()
    finally:
        ag.load_params(p)


def test_existing_modes_keep_their_bits(case):
    """PPO_MEAN and PPO_SAMPLE (action, log-prob, entropy, value) on these inputs, bitwise against the
    outputs the commit before PPO_ROACH produced on an MI355X (recorded, tests/golden/act_modes_parent).
    The 256-wide agent has no second act kernel to compare with: act_kernel= selects among the 64-wide
    tanh agent's kernels only."""
    L, p, x, ag = case
    gold = np.load(GOLDEN)
    for n in ROWS:
        xd = DeviceArray.from_numpy(x[:n])
        for name, mode, kw in (("mean", ppo_amd.PPO_MEAN, {}), ("sample", ppo_amd.PPO_SAMPLE, dict(env_base=5, step_id=123))):
            outs = ag.get_action_and_value(xd, mode, **kw)
            for part, o in zip(("action", "logprob", "entropy", "value"), outs):
                g = gold[f"O{L.O}_A{L.A}_H{L.H}_n{n}_{name}_{part}"]
                np.testing.assert_array_equal(o.numpy().view(np.uint32), g.view(np.uint32), err_msg=f"{name} {part} n={n}")


def test_tanh_agent_refuses_roach():
    ag = make_agent(17, 6, 64, kind=0)
    x = DeviceArray.from_numpy(np.zeros((3, 17), np.float32))
    with pytest.raises(ppo_amd.PPOError, match="Unsupported sample type used. Sample type: 3"):
        ag.get_action_and_value(x, ppo_amd.PPO_ROACH)
    ag.close()
