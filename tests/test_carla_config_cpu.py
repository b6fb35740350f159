"""bin/ac_ppo_carla's configuration (apps/carla_config.h) and the Adam options of the library, without a GPU.

The config hand-off to a leaderboard gym on <port>.conf_lock and the experiment folder's config.json both come
before the trainer's first HIP call, so a child started here gets that far on any machine; a zmtp_peer.Peer
plays the gym, keeps the message, and the child is killed afterwards. tests/golden/carla_config/defaults.json
holds the reference's keys in its order with the values and JSON types of a default GlobalConfig
(carla_config.h:24-138, reals as the double of the fp32 default)."""
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np
import pytest

from zmtp_peer import Peer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ac_ppo_carla")
LIB = os.path.join(ROOT, "ppo.cpp_amd", "lib", "libppo_hip.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "carla_config", "defaults.json")
NO_FLAG = {"py/object", "num_devices", "batch_size", "minibatch_size", "num_iterations", "num_envs_per_proc",
           "batch_size_per_device", "minibatch_per_device", "global_step", "max_training_score", "best_iteration",
           "latest_iteration", "ttc_resolution", "ttc_penalty_ticks", "survival_reward_magnitude"}

needs_app = pytest.mark.skipif(not os.path.exists(APP), reason="bin/ac_ppo_carla not built")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libppo_hip.so not built")


def _defaults():
    with open(FIXTURE) as f:
        return json.load(f)  # dicts keep the file's key order


def _handoff(port, extra=()):
    """starts the trainer, plays the gym of `port` on its conf_lock socket, returns (the text the gym got, the
    text of config.json); the child is killed once config.json is complete. The folder is a short one of
    tempfile's: a unix socket path holds 107 bytes, fewer than a pytest tmp_path plus comm_files/<port>.conf_lock
    can take."""
    with tempfile.TemporaryDirectory(prefix="cc") as d:
        return _handoff_in(d, port, extra)


def _handoff_in(d, port, extra):
    comm, logdir = os.path.join(d, "tc"), os.path.join(d, "logs")
    got, errors, peers = [], [], []

    def gym():
        try:
            conf = Peer.connect("PAIR", f"ipc://{comm}/comm_files/{port}.conf_lock", timeout=60)
            peers.append(conf)  # a gym keeps its socket open until the trainer has closed its end
            got.append(conf.recv()[0].decode())
            conf.send([b"config received"])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    t = threading.Thread(target=gym, daemon=True)
    t.start()
    child = subprocess.Popen([APP, "--team_code_folder", comm, "--logdir", logdir, "--ports", str(port), *extra],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    path = os.path.join(logdir, "PPO_002_1", "config.json")
    text = ""
    try:
        t.join(timeout=60)
        assert not errors and got, (errors, child.poll())
        deadline = time.time() + 60
        while time.time() < deadline:  # written right after the hand-off; without a GPU the child then exits
            if os.path.exists(path):
                with open(path) as f:
                    text = f.read()
                if text.endswith("}\n"):
                    break
            if child.poll() is not None and not os.path.exists(path):
                break
            time.sleep(0.01)
    finally:
        child.kill()
        child.communicate()
        for p in peers:
            p.close()
    return got[0], text, comm, logdir


def _check_against_fixture(conf, comm, logdir, changed):
    ref = _defaults()
    assert list(conf) == list(ref)
    assert conf["py/object"] == "rl_config.GlobalConfig"
    assert conf["team_code_folder"] == comm and conf["logdir"] == logdir
    differing = set()
    for k, v in ref.items():
        if k in ("team_code_folder", "logdir"):
            continue
        assert type(conf[k]) is type(v), (k, conf[k], v)
        if conf[k] != v:
            differing.add(k)
    assert differing == set(changed), differing ^ set(changed)
    for k, v in changed.items():
        assert conf[k] == v, (k, conf[k], v)


@needs_app
def test_default_config_handoff_matches_the_reference():
    sent, on_disk, comm, logdir = _handoff(6301)
    _check_against_fixture(json.loads(sent), comm, logdir, {})
    assert on_disk == sent
    # every real parses to exactly the double of the fp32 field
    conf = json.loads(sent)
    for k, v in conf.items():
        if isinstance(v, float):
            assert float(np.float32(v)) == v, k
    assert conf["gamma"] == float(np.float32(0.99)) and conf["gamma"] != 0.99


@needs_app
def test_non_default_flags_change_exactly_their_keys():
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    flags = {"reward_type": "simple_reward", "use_history": True, "route_width": 20, "weight_decay": f32(0.01),
             "beta_1": f32(0.8), "eval_time": 900.5, "debug_type": "save", "num_eval_runs": 3, "use_ttc": True,
             "consider_tl": False, "gamma": f32(0.98)}
    spelled = {"use_history": "1", "use_ttc": "1", "consider_tl": "0", "weight_decay": "0.01", "beta_1": "0.8",
               "gamma": "0.98"}
    extra = []
    for k, v in flags.items():
        extra += ["--" + k, spelled.get(k, str(v))]
    sent, on_disk, comm, logdir = _handoff(6302, extra)
    conf = json.loads(sent)
    _check_against_fixture(conf, comm, logdir, flags)
    assert conf["beta_1"] == f32(0.8) and conf["beta_1"] != 0.8
    assert on_disk == sent


@needs_app
def test_help_lists_every_flag_and_devices_are_checked(tmp_path):
    r = subprocess.run([APP, "--help"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 0
    for k in list(_defaults()) + ["gpu_ids", "ports"]:
        if k not in NO_FLAG:
            assert f"--{k} " in r.stdout, k
    for k in ("ttc_resolution", "ttc_penalty_ticks", "survival_reward_magnitude"):
        assert f"--{k} " not in r.stdout, k
    base = [APP, "--team_code_folder", str(tmp_path / "tc")]
    for flag, code in (("collect_device", 2), ("train_device", 3)):
        r = subprocess.run(base + ["--" + flag, "tpu"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == code and "tpu" in r.stderr and "Options: cpu, gpu" in r.stderr, (r.returncode, r.stderr)
        r = subprocess.run(base + ["--" + flag, "cpu"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode != 0 and "not built" in r.stderr, (r.returncode, r.stderr)
    # the two variants that stay refused, and an unknown flag
    r = subprocess.run(base + ["--no_such_option", "1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1 and "Flag could not be matched" in r.stderr


@needs_lib
def test_set_adam_refusals_need_no_context():
    """ppo_carla_set_adam checks its numbers, then its agent, before any HIP call (fresh interpreter: ppo_amd
    loads torch first, as every consumer of the library must)."""
    script = r'''
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import ppo_amd
lib = ppo_amd.lib()
out = []
for args in ((0.9, 0.999, 0.0), (1.0, 0.999, 0.0), (-0.1, 0.999, 0.0), (0.9, 1.5, 0.0), (float("nan"), 0.9, 0.0),
             (0.9, 0.999, -1e-3), (0.9, 0.999, float("inf")), (0.9, 0.999, float("nan"))):
    rc = lib.ppo_carla_set_adam(None, *args)
    out.append([rc, lib.ppo_last_error().decode()])
d = ctypes.c_double(0)
rc = lib.ppo_carla_get_adam(None, ctypes.byref(d), ctypes.byref(d), ctypes.byref(d))
out.append([rc, lib.ppo_last_error().decode()])
out.append([lib.ppo_carla_rollout_returns_mean(None, 1, None), lib.ppo_last_error().decode()])
print(json.dumps(out))
'''
    res = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "ppo.cpp_amd")], capture_output=True,
                         text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    want = ["null argument"] + ["beta1 and beta2 must be in [0, 1)"] * 4 + ["weight_decay must be finite"] * 3 + \
           ["ppo_carla_get_adam: null argument", "ppo_carla_rollout_returns_mean: null argument"]
    for (rc, err), w in zip(got, want):
        assert rc == -1 and w in err, (rc, err, w)


@needs_lib
def test_adam3_archive_round_trip_and_cross_loading(tmp_path):
    torch = pytest.importorskip("torch")
    P = pytest.importorskip("ppo_amd")
    L = P.carla_layout2(layer_norm=True)
    rng = np.random.default_rng(17)
    m = rng.standard_normal(L.P).astype(np.float32)
    v = rng.uniform(0, 1, L.P).astype(np.float32)
    m[:2] = 0  # action_space_high / _low carry no state
    v[:2] = 0
    opts = (1.25e-4, 1e-5, float(np.float32(0.8)), 0.99, float(np.float32(0.01)))
    P.save_carla_adam_pth3(L, m, v, 7, *opts, tmp_path / "o3.pth")
    m3, v3, step, *got = P.load_carla_adam_pth3(L, tmp_path / "o3.pth")
    assert np.array_equal(m3, m) and np.array_equal(v3, v) and step == 7 and tuple(got) == opts
    g = getattr(torch.jit.load(str(tmp_path / "o3.pth")).param_groups, "param_groups/0")
    assert tuple(g.options.betas) == opts[2:4] and g.options.weight_decay == opts[4] and g.options.lr == opts[0]
    # default options: the *2 and *3 files are the same bytes, and each loader reads the other's file
    # (an archive carries its file's stem, so the two get one name in two folders)
    for d in ("two", "three"):
        (tmp_path / d).mkdir()
    d2, d3 = tmp_path / "two" / "optimizer.pth", tmp_path / "three" / "optimizer.pth"
    P.save_carla_adam_pth3(L, m, v, 7, 1.25e-4, 1e-5, 0.9, 0.999, 0.0, d3)
    P.save_carla_adam_pth2(L, m, v, 7, 1.25e-4, 1e-5, d2)
    assert d3.read_bytes() == d2.read_bytes()
    m2, v2, step2, lr2, eps2 = P.load_carla_adam_pth2(L, d3)
    assert np.array_equal(m2, m) and np.array_equal(v2, v) and (step2, lr2, eps2) == (7, 1.25e-4, 1e-5)
    m3, v3, step3, *got = P.load_carla_adam_pth3(L, d2)
    assert np.array_equal(m3, m) and np.array_equal(v3, v) and step3 == 7
    assert tuple(got) == (1.25e-4, 1e-5, 0.9, 0.999, 0.0)
    # the *2 loader reads a non-default archive too (and drops its betas and weight decay)
    assert P.load_carla_adam_pth2(L, tmp_path / "o3.pth")[2] == 7
