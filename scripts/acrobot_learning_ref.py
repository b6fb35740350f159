#!/usr/bin/env python3
"""CPU reference for "the trainer learns AcrobotContinuous-v1" (tests/test_gpu_acrobot.py::test_it_learns
and test_it_learns_ac): Gymnasium's Acrobot-v1 with a continuous torque, the task whose termination is
success (reward -1 per step, 0 on the step that swings the tip above the bar; 500-step truncation).

The loop of scripts/pendulum_learning_ref.py (its run_seed(), evaluate(), argument parser and main()
are used as they are) over the host env gymcpp::AcrobotContinuous behind SeqVectorEnv +
RecordEpisodeStatistics (tests/native/acrobot_driver.cpp built as a shared object,
tests/acrobot_common.py HostAcrobot): oracle_lib.get_action_and_value / gae / update at O = 6, A = 1,
and for the PPO agent the oracle's wrapper chain (oracle_lib.VecWrappers), which gets the env's
termination flag: NormalizeReward restarts its return accumulator after a termination.

Per seed it measures the mean-action return over the first 64 evaluation episodes (all envs reset
with eval_seed) before and after training and writes tests/golden/acrobot/learning_ref[_ac].json.
The untrained mean-action policy never swings up: every untrained return is -500 and their spread is
0, so the project's rule (improve by twice the spread) says nothing here. The config must satisfy, on
this reference alone: in every seed  trained - untrained >= 50, a tenth of the return range.

  python scripts/acrobot_learning_ref.py [--agent ppo|ac] [--num_envs 64] ... [--out PATH] [--curve] [--jobs 3]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import acrobot_common as ac  # noqa: E402
import pendulum_learning_ref as P  # noqa: E402

ENV, OD, AD = ac.ENV_ID, ac.OD, ac.AD
EVAL_EPISODES = P.EVAL_EPISODES
MIN_IMPROVEMENT = 50.0
DEFAULTS = dict(num_envs=64, num_steps=128, total_timesteps=64 * 128 * 20, num_minibatches=32, update_epochs=10,
                learning_rate=3e-3, gamma=0.99, gae_lambda=0.95)


def parser():
    ap = P.parser()
    ap.set_defaults(out=None, **DEFAULTS)
    ap.add_argument("--params_at", type=int, default=0,
                    help="write the first seed's parameters after this many iterations instead of the reference file: "
                         "tests/golden/acrobot/params_<agent>.npy, a policy whose sampled actions swing up "
                         "(tests/test_gpu_acrobot.py compares the rollout kernels on it)")
    ap.add_argument("--clone_pump", type=int, default=0,
                    help="write AC parameters that follow the energy-pumping rule, cloned in this many rounds "
                         "(clone_pump()): tests/golden/acrobot/params_ac.npy")
    return ap


def params_path(agent):
    return os.path.join(ROOT, "tests", "golden", "acrobot", f"params_{agent}.npy")


def clone_pump(iters, seed=1):
    """Parameters of the AC agent (LayerNorm-Beta, H = 256) that follow the energy-pumping rule
    a = sign(theta2dot) of tests/native/acrobot_driver.cpp. The AC agent's sampled actions never swing
    up, so its reference runs never see a reward other than -1 and learn nothing; the
    rollout and evaluation kernels still have to be compared on episodes that terminate. The rule is
    cloned with the oracle's own PPO update: over observations along the rule's swing-ups (32 host envs,
    192 steps, every third kept) the action 0.8 * sign(theta2dot) gets advantage +1 and its opposite -1,
    the old log-probabilities are the current policy's, `iters` rounds of 4 epochs x 8 minibatches at
    lr 1e-3, no value or entropy term."""
    import numpy as np
    import oracle_lib as O
    import ppo_amd
    kind, H = ppo_amd.PPO_NET_LN_BETA, 256
    L = O.layout_init(kind, OD, AD, H)
    p = ppo_amd.init_params(ppo_amd.agent_layout(kind, OD, AD, H), seed=seed, env_id=ENV)
    E, T = 32, 192
    env = ac.HostAcrobot(E)
    obs = env.reset(seed)
    rng = np.random.default_rng(seed)
    xs = []
    for _ in range(T):
        xs.append(obs)
        obs = env.step((np.sign(obs[:, 5:6]) + rng.uniform(-0.5, 0.5, (E, 1))).astype(np.float32))[0]
    env.close()
    x = np.concatenate(xs)[::3]
    push = np.sign(x[:, 5:6]).astype(np.float32)
    push[push == 0] = 1
    bo, ba = np.concatenate([x, x]), np.concatenate([0.8 * push, -0.8 * push]).astype(np.float32)
    adv = np.concatenate([np.ones(len(x)), -np.ones(len(x))]).astype(np.float32)
    m, v, step = np.zeros(L.P, np.float32), np.zeros(L.P, np.float32), 0
    lcfg = O.LossCfg(0.2, 0.0, 0.0, 1, 1)
    for it in range(iters):
        _, lp, _, val = O.get_action_and_value(L, p, bo, 1, ba)
        p, m, v, step, _ = O.update(L, p, m, v, step, bo, ba, lp, adv, val, val, 4, 8, 1e-3, 0.5, 1e-5, lcfg, seed=seed, rank=0,
                                    epoch_counter0=it * 4)
        am, _, _, _ = O.get_action_and_value(L, p, x, 2)
        print(f"  round {it + 1}: the mean action has the rule's sign on {float((np.sign(am) == push).mean()):.4f} of {len(x)} "
              f"observations, mean |a| {float(np.abs(am).mean()):.3f}", flush=True)
    return p


def main():
    a = parser().parse_args()
    if a.params_at > 0 or a.clone_pump > 0:
        import numpy as np
        if a.clone_pump > 0:
            a.agent = "ac"
            p = clone_pump(a.clone_pump, a.seeds[0])
        else:
            p = P.run_seed(a, a.seeds[0], a.curve, max_iters=a.params_at, want_params=True, env_id=ENV, dims=(OD, AD),
                           host=ac.HostAcrobot)
        # the AC agent's parameters as fp16 (any parameters serve; the test loads what the file holds)
        p = np.asarray(p, np.float16 if a.agent == "ac" else np.float32)
        os.makedirs(os.path.dirname(params_path(a.agent)), exist_ok=True)
        np.save(a.out or params_path(a.agent), p)
        print(f"{a.agent}: {p.size} parameters ({p.dtype}), seed {a.seeds[0]}")
        return
    if a.out is None:
        a.out = os.path.join(ROOT, "tests", "golden", "acrobot", "learning_ref.json" if a.agent == "ppo" else "learning_ref_ac.json")
    P.main(a, ENV, (OD, AD), ac.HostAcrobot, min_improvement=MIN_IMPROVEMENT)


if __name__ == "__main__":
    main()
