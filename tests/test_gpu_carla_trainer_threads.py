"""bin/ac_ppo_carla --collect_mode threads (one std::thread and one act lane per env, the reference's
src/carla/ac_ppo_carla.cpp:355-417) against scripted CARLA leaderboard gyms played by zmtp_peer.Peer, as
test_gpu_carla_trainer_app.py plays them for the lockstep loop.

Every gym here waits 50 ms before it answers an action and records the interval during which it holds an
unanswered one. In lockstep mode the envs are stepped one after the other, so no two such intervals can
overlap; with one thread per env they must. That overlap is the structural proof of concurrency: no wall
time is asserted. Thread timing must not reach the result: two identical runs write the same checkpoint
bytes, and with one env both modes run the same batch-1 forwards with the same keys."""
import glob
import os
import struct
import subprocess
import tempfile
import threading
import time

import numpy as np
import pytest

from zmtp_peer import Peer

pytestmark = pytest.mark.gpu

ppo_amd = pytest.importorskip("ppo_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "ppo.cpp_amd", "bin", "ac_ppo_carla")
PORTS = (6111, 6112, 6113)
NB = 15 * 192 * 192
DELAY = 0.05


def _state(rng, k):
    """the k-th state of an env: fixed pseudo-random observation, reward 0.5, terminal at every third step"""
    term = k > 0 and k % 4 == 3  # states 0..3 of an episode: reset, step 1, step 2, step 3 (terminal)
    return [rng.integers(0, 256, NB, dtype=np.uint8).tobytes(), rng.uniform(-1, 1, 8).astype(np.float32).tobytes(),
            rng.uniform(-1, 1, 3).astype(np.float32).tobytes(), struct.pack("<f", 0.5), bytes([int(term)]), b"\x00",
            struct.pack("<i", k), struct.pack("<i", 0)], term


def _gym(comm, port, errors, held):
    """one leaderboard gym: answers the config, then serves states until the trainer closes the socket;
    held collects (port, received, answered) for every action"""
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
            t0 = None
            if not term:  # after a terminal state the trainer asks for the reset state without an action
                action = env.recv()
                t0 = time.monotonic()
                assert len(action) == 1 and len(action[0]) == 8
                a = np.frombuffer(action[0], np.float32)
                assert np.isfinite(a).all() and (np.abs(a) <= 1).all()
                time.sleep(DELAY)  # the simulator's tick
            k += 1
            state, term = _state(rng, k)
            if t0 is not None:
                held.append((port, t0, time.monotonic()))
            env.send(state)
    except (ConnectionError, BrokenPipeError, OSError):
        pass  # the trainer finished and closed its sockets
    except Exception as e:  # noqa: BLE001
        errors.append(repr(e))


def _run(comm, logdir, exp, ports, mode, steps=4):
    errors, held = [], []
    gyms = [threading.Thread(target=_gym, args=(comm, p, errors, held), daemon=True) for p in ports]
    for g in gyms:
        g.start()
    cmd = [APP, "--team_code_folder", comm, "--logdir", logdir, "--exp_name", exp, "--num_envs", str(len(ports)),
           "--num_steps", str(steps), "--num_minibatches", "2", "--update_epochs", "1", "--total_timesteps",
           str(steps * len(ports)), "--seed", "3", "--collect_mode", mode]
    for p in ports:
        cmd += ["--ports", str(p)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    for g in gyms:
        g.join(timeout=10)
    assert not errors, errors
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res.stdout, held


def _max_held_at_once(held):
    """the largest number of gyms that hold an unanswered action at one instant"""
    events = sorted([(t0, 1) for _, t0, _ in held] + [(t1, -1) for _, _, t1 in held], key=lambda x: (x[0], x[1]))
    best = cur = 0
    for _, d in events:
        cur += d
        best = max(best, cur)
    return best


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_threads_mode_steps_the_gyms_concurrently_and_reproducibly():
    assert os.path.exists(APP), "bin/ac_ppo_carla not built (run __graft_entry__.build())"
    L = ppo_amd.carla_layout()
    with tempfile.TemporaryDirectory() as d:
        comm, logdir = os.path.join(d, "team_code"), os.path.join(d, "logs")
        out, held = _run(comm, logdir, "a", PORTS, "threads")
        assert len(held) >= 3 * 3 and {p for p, _, _ in held} == set(PORTS)
        n = _max_held_at_once(held)
        print("gyms holding an action at one instant:", n)
        assert n >= 2, held
        # log lines and the checkpoint pair, as the lockstep loop's
        assert "SPS:" in out and "global_step=12, avg_episodic_return=" in out, out
        folder = os.path.join(logdir, "a")
        assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(folder, "*_latest_*.pth"))) == \
            ["model_latest_000000000.pth", "optimizer_latest_000000000.pth"]
        p = ppo_amd.load_carla_pth(L, os.path.join(folder, "model_latest_000000000.pth"))
        assert np.isfinite(p).all() and p[L.hi] == 1.0 and p[L.lo] == -1.0
        _, _, step, _, eps = ppo_amd.load_carla_adam_pth2(ppo_amd.carla_layout2(),
                                                          os.path.join(folder, "optimizer_latest_000000000.pth"))
        assert step == 2 and abs(eps - 1e-5) < 1e-12  # 1 iteration x 2 minibatches
        assert os.path.exists(os.path.join(folder, "config.json"))
        # thread timing does not reach the result
        _run(comm, logdir, "b", PORTS, "threads")
        assert _bytes(os.path.join(folder, "model_latest_000000000.pth")) == \
            _bytes(os.path.join(logdir, "b", "model_latest_000000000.pth"))


def test_one_env_gives_the_lockstep_checkpoint():
    assert os.path.exists(APP), "bin/ac_ppo_carla not built (run __graft_entry__.build())"
    with tempfile.TemporaryDirectory() as d:
        comm, logdir = os.path.join(d, "team_code"), os.path.join(d, "logs")
        _, held = _run(comm, logdir, "threads", PORTS[:1], "threads")
        assert _max_held_at_once(held) == 1
        _run(comm, logdir, "lockstep", PORTS[:1], "lockstep")
        a = _bytes(os.path.join(logdir, "threads", "model_latest_000000000.pth"))
        b = _bytes(os.path.join(logdir, "lockstep", "model_latest_000000000.pth"))
        assert len(a) > 1000 and a == b
