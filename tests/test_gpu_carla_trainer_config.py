"""bin/ac_ppo_carla with the full configuration, against two scripted leaderboard gyms (zmtp_peer.Peer), as
tests/test_gpu_carla_trainer_app.py: 2 envs, T = 4, one epoch of two minibatches, one iteration per run.

  (a) explicit --beta_1 0.9 --beta_2 0.999 --weight_decay 0 writes the bytes of a run without them;
  (b) --weight_decay 0.01 --beta_1 0.8 --reward_type simple_reward reaches the gyms and the optimizer archive;
  (c) a resume of (b) with --load_file and a larger --total_timesteps alone takes every other setting from the
      folder's config.json, the optimizer's options from its archive, and trains one more iteration;
  the event file carries losses/discounted_returns; ppo_carla_inference starts from (b)'s folder."""
import glob
import json
import os
import shutil
import struct
import subprocess
import tempfile
import threading

import numpy as np
import pytest

from zmtp_peer import Peer

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ac_ppo_carla")
SERVER = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ppo_carla_inference")
PORTS = (6311, 6312)
NB = 15 * 192 * 192
F32 = lambda x: float(np.float32(x))  # noqa: E731


def _state(rng, k):
    term = k > 0 and k % 4 == 3  # reset, step 1, step 2, step 3 (terminal)
    return [rng.integers(0, 256, NB, dtype=np.uint8).tobytes(), rng.uniform(-1, 1, 8).astype(np.float32).tobytes(),
            rng.uniform(-1, 1, 3).astype(np.float32).tobytes(), struct.pack("<f", 0.5), bytes([int(term)]), b"\x00",
            struct.pack("<i", k), struct.pack("<i", 0)], term


def _gym(comm, port, confs, errors):
    """one leaderboard gym: keeps the config it is sent, then serves states until the trainer closes the socket"""
    try:
        rng = np.random.default_rng(port)
        conf = Peer.connect("PAIR", f"ipc://{comm}/comm_files/{port}.conf_lock", timeout=60)
        confs[port] = json.loads(conf.recv()[0])
        conf.send([b"config received"])
        env = Peer.connect("PAIR", f"ipc://{comm}/comm_files/{port}.lock", timeout=60)
        env.send([b"Connected to leaderboard gym."])
        k = 0
        state, term = _state(rng, k)
        env.send(state)
        while True:
            if not term:
                assert len(env.recv()[0]) == 8
            k += 1
            state, term = _state(rng, k)
            env.send(state)
    except (ConnectionError, BrokenPipeError, OSError):
        pass  # the trainer finished and closed its sockets
    except Exception as e:  # noqa: BLE001
        errors.append(repr(e))


def _run(comm, logdir, args):
    """returns (stdout, the config each gym received)"""
    errors, confs = [], {}
    gyms = [threading.Thread(target=_gym, args=(comm, p, confs, errors), daemon=True) for p in PORTS]
    for g in gyms:
        g.start()
    cmd = [APP, "--team_code_folder", comm, "--logdir", logdir, "--ports", str(PORTS[0]), "--ports", str(PORTS[1]), *args]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    for g in gyms:
        g.join(timeout=10)
    assert not errors, errors
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert sorted(confs) == sorted(PORTS) and confs[PORTS[0]] == confs[PORTS[1]]
    return res.stdout, confs[PORTS[0]]


SIZES = ("--num_envs", "2", "--num_steps", "4", "--num_minibatches", "2", "--update_epochs", "1", "--total_timesteps", "8",
         "--seed", "3")


@pytest.fixture(scope="module")
def runs():
    """every run of the module, once. A short folder of tempfile's: a unix socket path holds 107 bytes."""
    assert os.path.exists(APP), "bin/ac_ppo_carla not built (run __graft_entry__.build())"
    with tempfile.TemporaryDirectory(prefix="cc") as d:
        yield _all_runs(d)


def _all_runs(d):
    comm, logdir = os.path.join(d, "tc"), os.path.join(d, "logs")
    out = dict(comm=comm, logdir=logdir)
    out["plain"] = _run(comm, logdir, ("--exp_name", "plain", *SIZES))
    out["explicit"] = _run(comm, logdir, ("--exp_name", "explicit", *SIZES, "--beta_1", "0.9", "--beta_2", "0.999",
                                          "--weight_decay", "0"))
    out["opt"] = _run(comm, logdir, ("--exp_name", "opt", *SIZES, "--weight_decay", "0.01", "--beta_1", "0.8",
                                     "--reward_type", "simple_reward"))
    shutil.copytree(os.path.join(logdir, "opt"), os.path.join(logdir, "opt_first"))  # the resume below prunes it
    folder = os.path.join(logdir, "opt")
    out["resume"] = _run(comm, logdir, ("--exp_name", "opt", "--load_file",
                                        os.path.join(folder, "model_latest_000000000.pth"), "--total_timesteps", "16"))
    return out


def _bytes(logdir, exp, name):
    with open(os.path.join(logdir, exp, name), "rb") as f:
        return f.read()


def test_explicit_default_options_write_the_same_checkpoint(runs):
    for name in ("model_latest_000000000.pth", "optimizer_latest_000000000.pth"):
        assert _bytes(runs["logdir"], "plain", name) == _bytes(runs["logdir"], "explicit", name), name
    _, _, step, _, _, b1, b2, wd = ppo_amd.load_carla_adam_pth3(
        ppo_amd.carla_layout2(), os.path.join(runs["logdir"], "plain", "optimizer_latest_000000000.pth"))
    assert (step, b1, b2, wd) == (2, 0.9, 0.999, 0.0)  # the exact defaults, not the widened fp32 fields


def test_options_reach_the_gyms_the_archive_and_the_event_file(runs):
    _, conf = runs["opt"]
    assert conf["py/object"] == "rl_config.GlobalConfig" and conf["reward_type"] == "simple_reward"
    assert conf["weight_decay"] == F32(0.01) and conf["beta_1"] == F32(0.8) and conf["beta_2"] == F32(0.999)
    folder = os.path.join(runs["logdir"], "opt_first")
    m, v, step, _, eps, b1, b2, wd = ppo_amd.load_carla_adam_pth3(
        ppo_amd.carla_layout2(), os.path.join(folder, "optimizer_latest_000000000.pth"))
    assert (step, b1, b2, wd) == (2, F32(0.8), F32(0.999), F32(0.01)) and np.abs(m).max() > 0
    assert _bytes(runs["logdir"], "opt_first", "model_latest_000000000.pth") != \
        _bytes(runs["logdir"], "plain", "model_latest_000000000.pth")
    with open(os.path.join(folder, "config.json")) as f:
        disk = json.load(f)
    assert disk["reward_type"] == "simple_reward" and disk["latest_iteration"] == 0 and disk["global_step"] == 8
    events = glob.glob(os.path.join(folder, "events.out.tfevents.*"))
    assert events and any(b"losses/discounted_returns" in open(e, "rb").read() for e in events)


def test_resume_takes_its_settings_from_the_folder(runs):
    folder = os.path.join(runs["logdir"], "opt")
    out, conf = runs["resume"]  # --exp_name, --load_file and --total_timesteps 16 only
    assert "Start training from step: 1" in out and out.count("SPS:") == 1, out
    assert conf["reward_type"] == "simple_reward" and conf["weight_decay"] == F32(0.01) and conf["beta_1"] == F32(0.8)
    assert (conf["num_envs"], conf["num_steps"], conf["num_minibatches"], conf["update_epochs"], conf["seed"]) == \
        (2, 4, 2, 1, 3)
    assert conf["total_timesteps"] == 16 and conf["num_iterations"] == 2 and conf["global_step"] == 8
    assert [os.path.basename(f) for f in glob.glob(os.path.join(folder, "model_latest_*.pth"))] == \
        ["model_latest_000000001.pth"]
    _, _, step, _, _, b1, b2, wd = ppo_amd.load_carla_adam_pth3(
        ppo_amd.carla_layout2(), os.path.join(folder, "optimizer_latest_000000001.pth"))
    assert (step, b1, b2, wd) == (4, F32(0.8), F32(0.999), F32(0.01))


def test_inference_server_starts_from_the_trainers_folder(runs):
    with tempfile.TemporaryDirectory(prefix="cc") as ipc:
        _serve_one(os.path.join(runs["logdir"], "opt"), ipc)


def _serve_one(folder, tmp_path):
    rng = np.random.default_rng(9)
    srv = subprocess.Popen([SERVER, "--path_to_conf_file", folder, "--ipc_path", str(tmp_path), "--port", "6313"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        agent = Peer.connect("PAIR", f"ipc://{tmp_path}/6313.lock")
        assert agent.recv() == [b"Connected to eval_agent.py."]
        agent.send([b"mean"])
        agent.send([b""])
        agent.send([rng.integers(0, 256, NB, dtype=np.uint8).tobytes(), rng.uniform(-1, 1, 8).astype(np.float32).tobytes(),
                    rng.uniform(-1, 1, 3).astype(np.float32).tobytes()])
        parts = agent.recv()
        assert [len(x) for x in parts] == [8, 4, 8, 8]
        a = np.frombuffer(parts[0], np.float32)
        assert np.isfinite(a).all() and (np.abs(a) <= 1).all()
        agent.send([b"done"])
        out, err = srv.communicate(timeout=60)
    finally:
        if srv.poll() is None:
            srv.kill()
            srv.communicate()
    assert srv.returncode == 0, err
