"""bin/ac_ppo_carla (apps/ac_ppo_carla.cpp, the reference's src/carla/ac_ppo_carla.cpp loop) against two
CARLA leaderboard gyms played by zmtp_peer.Peer: the config hand-off on <port>.conf_lock, the env protocol
on <port>.lock (hello, then 8-part states; a terminal state is followed by the reset state without an
action in between, as SeqVectorEnvCarla's next-step autoreset expects).

T = 4 steps, 2 envs, 1 epoch of 2 minibatches (4 rows each), 2 iterations; every episode ends at its
step 3. Checks the log lines, the checkpoint pair that remains, that training moved the parameters, and
a resumed third iteration."""
import glob
import os
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
PORTS = (6101, 6102)
NB = 15 * 192 * 192


def _state(rng, k):
    """the k-th state of an env: fixed pseudo-random observation, reward 0.5, terminal at every third step"""
    term = k > 0 and k % 4 == 3  # states 0..3 of an episode: reset, step 1, step 2, step 3 (terminal)
    return [rng.integers(0, 256, NB, dtype=np.uint8).tobytes(), rng.uniform(-1, 1, 8).astype(np.float32).tobytes(),
            rng.uniform(-1, 1, 3).astype(np.float32).tobytes(), struct.pack("<f", 0.5), bytes([int(term)]), b"\x00",
            struct.pack("<i", k), struct.pack("<i", 0)], term


def _gym(comm, port, errors):
    """one leaderboard gym: answers the config, then serves states until the trainer closes the socket"""
    try:
        rng = np.random.default_rng(port)
        conf = Peer.connect("PAIR", f"ipc://{comm}/comm_files/{port}.conf_lock", timeout=60)
        assert b"num_steps" in conf.recv()[0]
        conf.send([b"config received"])
        env = Peer.connect("PAIR", f"ipc://{comm}/comm_files/{port}.lock", timeout=60)
        env.send([b"Connected to leaderboard gym."])
        k = 0
        state, term = _state(rng, k)
        env.send(state)
        while True:
            if not term:  # after a terminal state the trainer asks for the reset state without an action
                action = env.recv()
                assert len(action) == 1 and len(action[0]) == 8
                a = np.frombuffer(action[0], np.float32)
                assert np.isfinite(a).all() and (np.abs(a) <= 1).all()
            k += 1
            state, term = _state(rng, k)
            env.send(state)
    except (ConnectionError, BrokenPipeError, OSError):
        pass  # the trainer finished and closed its sockets
    except Exception as e:  # noqa: BLE001
        errors.append(repr(e))


def _run(comm, logdir, exp, total, extra=()):
    errors = []
    gyms = [threading.Thread(target=_gym, args=(comm, p, errors), daemon=True) for p in PORTS]
    for g in gyms:
        g.start()
    cmd = [APP, "--team_code_folder", comm, "--logdir", logdir, "--exp_name", exp, "--num_envs", "2", "--num_steps", "4",
           "--num_minibatches", "2", "--update_epochs", "1", "--total_timesteps", str(total), "--seed", "3",
           "--ports", str(PORTS[0]), "--ports", str(PORTS[1]), *extra]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    for g in gyms:
        g.join(timeout=10)
    assert not errors, errors
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res.stdout


def _latest(folder):
    return (sorted(os.path.basename(f) for f in glob.glob(os.path.join(folder, "model_latest_*.pth"))),
            sorted(os.path.basename(f) for f in glob.glob(os.path.join(folder, "optimizer_latest_*.pth"))))


def test_trainer_runs_checkpoints_and_resumes():
    assert os.path.exists(APP), "bin/ac_ppo_carla not built (run __graft_entry__.build())"
    L = ppo_amd.carla_layout()
    with tempfile.TemporaryDirectory() as d:
        comm, logdir = os.path.join(d, "team_code"), os.path.join(d, "logs")
        # learning rate 0: the checkpoint holds the initial parameters of seed 3
        _run(comm, logdir, "init", 8, ("--learning_rate", "0"))
        p_init = ppo_amd.load_carla_pth(L, os.path.join(logdir, "init", "model_latest_000000000.pth"))

        out = _run(comm, logdir, "run", 16)
        assert "SPS:" in out and "global_step=8, avg_episodic_return=" in out, out
        folder = os.path.join(logdir, "run")
        assert _latest(folder) == (["model_latest_000000001.pth"], ["optimizer_latest_000000001.pth"])
        p1 = ppo_amd.load_carla_pth(L, os.path.join(folder, "model_latest_000000001.pth"))
        assert np.isfinite(p1).all() and p1.shape == p_init.shape
        assert p1[L.hi] == 1.0 and p1[L.lo] == -1.0
        assert not np.array_equal(p1, p_init)
        m, v, step, _, eps = ppo_amd.load_carla_adam_pth2(ppo_amd.carla_layout2(),
                                                          os.path.join(folder, "optimizer_latest_000000001.pth"))
        assert step == 4 and abs(eps - 1e-5) < 1e-12 and np.abs(m).max() > 0 and (v >= 0).all()  # 2 iterations x 2 minibatches
        assert os.path.exists(os.path.join(folder, "config.json"))
        assert glob.glob(os.path.join(folder, "events.out.tfevents.*"))

        # resume: iteration 2 only
        out = _run(comm, logdir, "run", 24, ("--load_file", os.path.join(folder, "model_latest_000000001.pth")))
        assert "Start training from step: 2" in out and out.count("SPS:") == 1, out
        assert "global_step=24" in out, out
        assert _latest(folder) == (["model_latest_000000002.pth"], ["optimizer_latest_000000002.pth"])
        p2 = ppo_amd.load_carla_pth(L, os.path.join(folder, "model_latest_000000002.pth"))
        assert np.isfinite(p2).all() and not np.array_equal(p2, p1)
        _, _, step, _, _ = ppo_amd.load_carla_adam_pth2(ppo_amd.carla_layout2(),
                                                        os.path.join(folder, "optimizer_latest_000000002.pth"))
        assert step == 6
