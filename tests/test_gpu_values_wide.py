"""k_values_w (csrc/ppo_values_wide.hip): the AC agent's batched critic at Humanoid width (LayerNorm-Beta,
H = 256, OP = 384), reached through ppo_values / Agent.values and, after k_rollout_w, as the value pass of
ppo_rollout_synth. It runs k_act3's critic chain, so its values must be get_value's bits; against a numpy
float64 restatement of the critic they are held to twice get_value's measured gap. The contexts are
test_gpu_rollout_wide's Side (update=off, every parameter off its initial value, an obs mean / std that is
not the identity)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")
from ppo_amd import DeviceArray  # noqa: E402
from test_gpu_rollout_wide import Side  # noqa: E402

R = 32  # k_values_w's rows per pass
# id: O, A, n
CASES = {
    "one-row": (376, 17, 1),
    "last-block-short-by-one": (376, 17, R - 1),
    "last-block-of-one-row": (376, 17, R + 1),
    "ragged-o373": (373, 17, 2 * R + 3),           # O % 4 != 0: the ragged last k-block
    "full-op-a20": (384, 20, R + 1),               # O = OP
    "second-block-per-workgroup": (376, 17, 256 * R + 1),  # 257 blocks on 256 CUs: the b += gridDim.x walk and
}                                                           # the one-ahead prefetch past the end (12 MB of obs)
# max |get_value - ref64| over each case's rows (ppo_get_value: k_act3's critic workgroups), measured on an
# MI355X, with the range of the case's float64 values beside it. The bounds are 2x these figures; k_values_w
# measured the same six (it is bitwise get_value).
GET_VALUE_REF_GAP = {
    "one-row": 2.558e-07,                     # the value is 1.198380
    "last-block-short-by-one": 6.602e-07,     # [-0.296797, 1.454911]
    "last-block-of-one-row": 8.108e-07,       # [-0.927467, 1.451877]
    "ragged-o373": 6.855e-07,                 # [-0.786651, 0.948442]
    "full-op-a20": 6.937e-07,                 # [-1.524429, 0.854260]
    "second-block-per-workgroup": 1.291e-06,  # [-1.402305, 2.704188]
}


def critic64(L, p, x):
    """The critic in float64 from the layout's offsets: normalise, (Linear, LayerNorm, ReLU) twice, the head."""
    p, (O, H) = p.astype(np.float64), (L.O, L.H)
    W1, b1, g1, be1, W2, b2, g2, be2 = L.critic
    h = (x.astype(np.float64) - p[L.omean:L.omean + O]) / p[L.ostd:L.ostd + O]
    for W, b, g, be, k in ((W1, b1, g1, be1, O), (W2, b2, g2, be2, H)):
        z = h @ p[W:W + H * k].reshape(H, k).T + p[b:b + H]
        z = (z - z.mean(1, keepdims=True)) / np.sqrt(z.var(1, keepdims=True) + 1e-5)
        h = np.maximum(z * p[g:g + H] + p[be:be + H], 0.0)
    return h @ p[L.cW3:L.cW3 + H] + p[L.cb3]


@functools.lru_cache(maxsize=None)
def critic_outputs(O, A):
    """{n: (values, get_value, ref64)} for every case of this (O, A), on one context; computed once."""
    side, out = Side(O, A, 1, 1, "update=off"), {}
    assert "values=k_values_w" in side.ag.kernel_info()
    params = side.ag.params()
    for n in sorted(c[2] for c in CASES.values() if c[:2] == (O, A)):
        x = (1.5 * np.random.default_rng(n).standard_normal((n, O))).astype(np.float32)
        xd = DeviceArray.from_numpy(x)
        out[n] = side.ag.values(xd).numpy(), side.ag.get_value(xd).numpy(), critic64(side.ag.layout, params, x)
    side.close()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_values_bitwise_get_value_and_within_its_gap_to_fp64(case):
    O, A, n = CASES[case]
    v, gv, ref = critic_outputs(O, A)[n]
    gap_v, gap_gv = np.abs(v - ref).max(), np.abs(gv - ref).max()
    print(f"{case}: ref64 range [{ref.min():.6f}, {ref.max():.6f}], get_value gap {gap_gv:.3e}, values gap {gap_v:.3e}")
    np.testing.assert_array_equal(v.view(np.uint32), gv.view(np.uint32))
    assert gap_v <= 2 * GET_VALUE_REF_GAP[case]


def test_values_wiring():
    # (E, T): 99 rows, below ppo_rollout_synth's row threshold (k_act3's critic), and 8 192 rows, at it (k_values_w:
    # the profiler's "values" slot counts the launch)
    for E, T, pass_is_values_w in ((33, 3, False), (128, 64, True)):
        side = Side(376, 17, E, T, "update=off")
        side.ag.profile()
        out, info = side.rollout(0)
        assert info == "rollout=k_rollout_w" and "values=k_values_w" in side.ag.kernel_info()
        assert ("values" in side.ag.profile_read()) == pass_is_values_w
        stored_obs = DeviceArray.from_numpy(out["obs"].reshape(E * T, 376))
        for fn in (side.ag.values, side.ag.get_value):
            np.testing.assert_array_equal(fn(stored_obs).numpy().view(np.uint32), out["values"].reshape(-1).view(np.uint32))
        with pytest.raises(RuntimeError, match="ppo_values"):
            ppo_amd.check(ppo_amd.lib().ppo_values(side.ag.h, 0, side.next_obs.ptr, side.next_done.ptr, None))
        side.close()
    # a default HalfCheetah context keeps its critic kernel, and Agent.values is that kernel
    E, T = 16, 4
    tr = ppo_amd.Trainer(ppo_amd.ACPPOConfig(env_id="HalfCheetah-v5", num_envs=E, num_steps=T, num_minibatches=1,
                                             update_epochs=1, total_timesteps=E * T))
    tr.rollout()
    assert "values=k_v" in tr.agent.kernel_info()
    stored = tr.agent.buffer(ppo_amd.BUF_VALUES, (T * E,)).numpy()
    again = tr.agent.values(tr.agent.buffer(ppo_amd.BUF_OBS, (T * E, 17))).numpy()
    np.testing.assert_array_equal(again.view(np.uint32), stored.view(np.uint32))
    tr.close()
