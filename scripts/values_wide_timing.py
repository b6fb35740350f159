"""Writes profiles/values_wide/values_wide_timing.txt ("k_values_w"), or into the directory given
as the first argument. Times the critic pass alone at Humanoid width (LayerNorm-Beta, H = 256, O = 376,
A = 17) on one update=off context per n, for n = 16 x 128, 256 x 128 and 4 096 x 128 rows of obs: ppo_values
(k_values_w) against ppo_get_value (k_act3's critic workgroups) on the same rows, by HIP events through the
context's profiler ("values" / "act"), in one process, alternating, three repetitions each after a warm-up of
both. One repetition is CALLS launches; the figure is the events' mean per launch. Before the timing the two
outputs are compared bit for bit. After the three sizes, n = 32 x 128, 64 x 128 and 128 x 128 the same way: the
crossover that ppo_rollout_synth's row threshold (kValuesWMinRows, ppo_capi_env.hip) is set at lies between
the first two sizes. The whole-rollout figures come from scripts/rollout_wide_timing.py."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import ppo_amd
from ppo_amd import DeviceArray
O, A, T, CALLS = 376, 17, 128, 16
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "values_wide")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
for E in (16, 256, 4096, 32, 64, 128):  # the three sizes, then the scan for the crossover between the first two
    n = E * T
    hc = ppo_amd.HipConfig(ppo_amd.PPO_NET_LN_BETA, O, A, 256, E, T, 1, 1, 0.99, 0.95, 0.2, 0.01, 0.5, 0.5, 1e-5, 1, 1, 1, 0, 1)
    ag = ppo_amd.Agent(hc, options="update=off")
    ag.load_params(ppo_amd.init_params(ag.layout, seed=3, env_id="Humanoid-v4"))
    x = DeviceArray.from_numpy(np.random.default_rng(E).standard_normal((n, O)).astype(np.float32))
    paths = {"k_values_w": ("values", ag.values), "k_act3": ("act", ag.get_value)}
    outs = [fn(x).numpy().view(np.uint32) for _, fn in paths.values()]  # warm-up of both, and the comparison
    assert np.array_equal(*outs), "the two paths differ"
    ag.profile()
    res = {}
    for rep in range(3):
        for name, (slot, fn) in paths.items():
            ag.sync(); ag.profile_reset()
            for _ in range(CALLS):
                fn(x)
            ms, cnt = ag.profile_read()[slot]
            assert cnt == CALLS
            res.setdefault(name, []).append(ms / cnt)
            say(f"O={O} A={A} n={n} ({E} x {T}) rep {rep} {name:10s} launches={cnt} per launch={ms/cnt*1e3:10.2f} us  per row={ms/cnt/n*1e6:8.3f} ns")
    mw, ma = np.median(res["k_values_w"]), np.median(res["k_act3"])
    say(f"n={n}: median k_values_w {mw*1e3:.2f} us, k_act3 critic {ma*1e3:.2f} us, ratio {ma/mw:.2f}x; "
        f"every k_values_w repetition faster than every k_act3 one: {max(res['k_values_w']) < min(res['k_act3'])}")
    ag.close()
os.makedirs(out_dir, exist_ok=True)
open(os.path.join(out_dir, "values_wide_timing.txt"), "w").write("\n".join(lines) + "\n")
